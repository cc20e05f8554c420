// Grouped 3x3 convolution (pad 1, stride 1 / 2, Cin == Cout == C, G groups of cg = C / G channels) on NHWC bf16:
// forward, input gradient and weight gradient of ResNeXt's conv2 (gfx950).
//
// The per-group GEMM is tiny (N = cg, K = 9 cg; ~9 cg / 2 flop per byte), so all three are organised as streams: a
// block owns one 64-channel SLAB (64 / cg whole groups, or one group at cg = 64) and a contiguous range of BANDS
// (R output rows x the full output width of one image). Per band the input patch of the slab -- the band's pixels
// plus the taps' halo, 128 contiguous bytes per pixel -- is staged in LDS once and the taps read it as shifted
// windows; out-of-image pixels are out-of-range buffer offsets (zeros). Only block-diagonal MFMA work is issued:
//   * cg <= 16: a 16-channel output tile meets exactly its own 16 input channels (v_mfma_f32_16x16x16_bf16 per tap);
//     the weight operand is the 16x16 per-tap block with zeros off the group diagonal, expanded from the real
//     [C][3][3][cg] weights into LDS once per block (never in HBM);
//   * cg = 32 / 64: the tile meets its group's 32 / 64 input channels (v_mfma_f32_16x16x32_bf16), no wasted work.
// Forward / dgrad (one kernel, a tap table): wave w takes the band's 16-pixel groups w, w + 4, ..; accumulators go
// through a per-wave fp32 LDS tile so that every lane then owns one 16-byte chunk (a fixed 8 channels) of a pixel:
// affine -> ReLU -> bf16 store -> shifted BatchNorm statistics of the stored values in registers, one fold and one
// atomic per channel and block (the contract of conv_epilogue.h). The stride-1 dgrad is the forward on the per-group
// transposed weights with the taps mirrored; the stride-2 dgrad runs once per output parity class with that class's
// taps (1, 2, 2 or 4 of them).
// Weight gradient: pixels are the MFMA k index; the dY band and the X patch are both read with transposing LDS loads
// (ds_read_b64_tr_b16; row swizzle of conv_wgrad_halo.h). Wave w owns output channels 16 w .. 16 w + 15 of the slab
// for all 9 taps against its group's input channels, keeps the accumulators over its whole band range and adds only
// the diagonal blocks into the zeroed fp32 gradient slot [C][3][3][cg] with atomics (split over band ranges).
// All global accesses go through buffer descriptors based at the band's image and slab, 32-bit offsets inside.

#include <algorithm>

#include "conv_epilogue.h"

namespace {

struct GConvArgs {
    const bf16_t* X;      // operand NHWC [N][H][W][C]
    const bf16_t* Wk;     // [C][3][3][cg] (dgrad: the per-group transposed shadow)
    bf16_t* Y;            // output NHWC [N][YH][YW][C]
    const float* affine;  // [2][C] scale, shift, or null
    float* stats;         // [STAT_SLOTS][2][C] slab or null
    const float* shift;   // [C] or null
    int N, H, W, C, cg;
    int GH, GW;           // output pixel grid of this launch (a parity class of Y for the stride-2 dgrad)
    int YH, YW, sY, oy, ox;
    int sA;               // operand sample stride
    int ntap;
    uint64_t tapw;        // 4 bits per tap: its index 3 ky + kx in Wk
    uint32_t tapdy, tapdx;  // 2 bits per tap: operand row / column offset from the patch origin
    int y0off, x0off;     // patch origin = (grid row * sA + y0off, x0off)
    int R, PR, PC;        // band rows; patch rows / columns
    int relu;
};

struct GWgradArgs {
    const bf16_t* dY;  // [N][OH][OW][C]
    const bf16_t* X;   // [N][H][W][C]
    float* dW;         // [C][3][3][cg] fp32, +=
    int N, H, W, C, cg, OH, OW, stride;
    int R, PR, PC, KP;  // band rows; patch rows / columns; band pixels rounded up to 32 (k rows staged)
};

__device__ __forceinline__ int gw_swz(int q) { return (q >> 1) & 3; }
// physical 16-B chunk slot of logical chunk c of row q: 32-B segments swizzled (conv_wgrad_halo.h)
__device__ __forceinline__ int gw_slot(int c, int q) { return (((c >> 1) ^ gw_swz(q)) << 1) | (c & 1); }

// first input channel (within the slab) that output tile nt (16 channels) of the slab meets
template <int KC>
__device__ __forceinline__ int tile_in0(int nt) { return KC == 16 ? nt * 16 : KC == 32 ? (nt >> 1) * 32 : 0; }

constexpr int GC_EP = 272;  // fp32 staging pitch per pixel, bytes (64 channels + 16 B)
template <int KC> constexpr int gc_wpitch() { return KC * 2 + (KC == 64 ? 16 : 0); }

template <int KC>  // input channels per output tile and tap: 16 (cg 4, 8, 16), 32, 64
__global__ __launch_bounds__(256) void gconv_kernel(const GConvArgs a, int nbands, int nranges) {
    constexpr int WP = gc_wpitch<KC>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sW = smem;                          // [ntap][64][WP] block-diagonal weights
    char* sP = sW + a.ntap * 64 * WP;         // [PR][PC][128 B] patch, chunk c of pixel q at c ^ (q & 7)
    char* sE = sP + a.PR * a.PC * 128;        // [4 waves][16 px][GC_EP] fp32 staging

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslab = a.C >> 6;
    const int slab = blockIdx.x % nslab, range = blockIdx.x / nslab;
    const int c0 = slab * 64;
    const int b0 = (int)((long)nbands * range / nranges), b1 = (int)((long)nbands * (range + 1) / nranges);
    if (b0 >= b1) return;  // whole block
    const int bpi = (a.GH + a.R - 1) / a.R;

    // ---- weights: per tap and output channel n the KC input channels its tile meets, zeros outside n's group
    constexpr int NPC = KC / 4;
    for (int id = tid; id < a.ntap * 64 * NPC; id += 256) {
        const int j = id % NPC, n = (id / NPC) & 63, t = id / (NPC * 64);
        const int in_ch = tile_in0<KC>(n >> 4) + j * 4;
        const int wt = (int)((a.tapw >> (4 * t)) & 15);
        u32x2 v = u32x2{0u, 0u};
        if (in_ch / a.cg == n / a.cg)
            v = *reinterpret_cast<const u32x2*>(a.Wk + ((size_t)(c0 + n) * 9 + wt) * a.cg + (in_ch % a.cg));
        *reinterpret_cast<u32x2*>(sW + (t * 64 + n) * WP + j * 8) = v;
    }

    const int fr = lane & 15, kq = lane >> 4;
    const int ec = lane & 7;  // epilogue: this lane's 8-channel chunk
    const bool want_st = a.stats != nullptr;
    float csh[8], asc[8], ash[8], s1[8], s2[8];
    load8(want_st && a.shift != nullptr, a.shift, c0 + ec * 8, csh);
    load8(a.affine != nullptr, a.affine, c0 + ec * 8, asc, 1.f);
    load8(a.affine != nullptr, a.affine + a.C, c0 + ec * 8, ash);
#pragma unroll
    for (int c = 0; c < 8; ++c) s1[c] = s2[c] = 0.f;
    char* eW = sE + wid * 16 * GC_EP;
    const size_t ximg = (size_t)a.H * a.W * a.C, yimg = (size_t)a.YH * a.YW * a.C;
    const int nch = a.PR * a.PC * 8;  // 16-B chunks per patch

    for (int b = b0; b < b1; ++b) {
        const int img = b / bpi, y0 = (b - img * bpi) * a.R;
        const int P = min(a.R, a.GH - y0) * a.GW;  // band pixels
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc_n(a.X + img * ximg + c0, (ximg - c0) * 2);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc_n(a.Y + img * yimg + c0, (yimg - c0) * 2);
        const int iy0 = y0 * a.sA + a.y0off;
        __syncthreads();  // the previous band's patch reads are done (first band: the weights are in)
        for (int id0 = tid; id0 < nch; id0 += 1024) {
            u32x4 v[4];
            int dst[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int id = id0 + u * 256;
                const int c = id & 7, q = id >> 3;
                const int pr = q / a.PC, pc = q - pr * a.PC;
                const int iy = iy0 + pr, ix = a.x0off + pc;
                const bool in = id < nch && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                v[u] = buf_ld16(rx, in ? (uint32_t)(((iy * a.W + ix) * a.C + c * 8) * 2) : BUF_OOB);
                dst[u] = id < nch ? q * 128 + ((c ^ (q & 7)) << 4) : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (dst[u] >= 0) *reinterpret_cast<u32x4*>(sP + dst[u]) = v[u];
        }
        __syncthreads();

        const int ng = (P + 15) >> 4;
        for (int g = wid; g < ng; g += 4) {
            const int p = min(g * 16 + fr, P - 1);  // rows past the band repeat its last pixel (never stored)
            const int gy = p / a.GW, gx = p - gy * a.GW;
            const int q0 = gy * a.sA * a.PC + gx * a.sA;
            f32x4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < a.ntap; ++t) {
                const int q = q0 + (int)((a.tapdy >> (2 * t)) & 3) * a.PC + (int)((a.tapdx >> (2 * t)) & 3);
                const char* row = sP + q * 128;
                const int sw = q & 7;
                const char* wrow = sW + (t * 64 + fr) * WP;
                if constexpr (KC == 16) {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        const s16x4 fx = *reinterpret_cast<const s16x4*>(row + (((nt * 2 + (kq >> 1)) ^ sw) << 4) +
                                                                         (kq & 1) * 8);
                        const s16x4 fw = *reinterpret_cast<const s16x4*>(wrow + nt * 16 * WP + kq * 8);
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fw, fx, acc[nt], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int ks = 0; ks < KC / 32; ++ks) {
                            const int ch = (tile_in0<KC>(nt) >> 3) + ks * 4 + kq;
                            const bf16x8 fx = *reinterpret_cast<const bf16x8*>(row + ((ch ^ sw) << 4));
                            const bf16x8 fw =
                                *reinterpret_cast<const bf16x8*>(wrow + nt * 16 * WP + ks * 64 + kq * 16);
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fx, acc[nt], 0, 0, 0);
                        }
                }
            }
            // lane holds channels 16 nt + 4 kq + r of pixel fr -> the wave's fp32 staging tile (written and read
            // back by this wave only: LDS order, no block barrier)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
                *reinterpret_cast<f32x4*>(eW + fr * GC_EP + (nt * 16 + kq * 4) * 4) = acc[nt];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int px = (lane >> 3) + 8 * k, pp = g * 16 + px;
                const bool valid = pp < P;
                float v[8];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const f32x4 tv = *reinterpret_cast<const f32x4*>(eW + px * GC_EP + ec * 32 + hh * 16);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[4 * hh + r] = tv[r];
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    v[c] = fmaf(v[c], asc[c], ash[c]);
                    if (a.relu) v[c] = fmaxf(v[c], 0.f);
                }
                u32x4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = pack_bf2(v[2 * c], v[2 * c + 1]);
                const int py = pp / a.GW, pxx = pp - py * a.GW;
                const int yy = (y0 + py) * a.sY + a.oy, xx = pxx * a.sY + a.ox;
                buf_st16(ry, valid ? (uint32_t)(((yy * a.YW + xx) * a.C + ec * 8) * 2) : BUF_OOB, o);
                if (want_st) stat_fwd(o, valid ? 1.f : 0.f, csh, s1, s2);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if (!want_st) return;
    float* slab_p = stat_slab(a.stats, 2, a.C) + c0 + ec * 8;
    flush_chunk_lanes<8>(s1, slab_p, lane);
    flush_chunk_lanes<8>(s2, slab_p + a.C, lane);
}

template <int KC>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const GWgradArgs a, int nbands, int nranges) {
    constexpr int NJ = KC / 16;  // 16-channel input segments per output tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sD = smem;                 // [KP][128 B] dY band (rows past the band: zeros)
    char* sP = smem + a.KP * 128;    // [PR][PC][128 B] X patch

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nslab = a.C >> 6;
    const int slab = blockIdx.x % nslab, range = blockIdx.x / nslab;
    const int c0 = slab * 64;
    const int b0 = (int)((long)nbands * range / nranges), b1 = (int)((long)nbands * (range + 1) / nranges);
    if (b0 >= b1) return;  // whole block
    const int bpi = (a.OH + a.R - 1) / a.R;
    const size_t ximg = (size_t)a.H * a.W * a.C, dimg = (size_t)a.OH * a.OW * a.C;
    const int nch = a.PR * a.PC * 8;
    const int seg0 = tile_in0<KC>(wid) >> 4;  // first input segment of this wave's output tile

    // tr16 fragment lanes (conv_wgrad_halo.h): lane 4 q + p of a 16-lane group reads row q, columns 4 p .. 4 p + 3
    // of a 16-channel segment; the 32-lane half h reads rows 8 (2 r + h) + 4 g + q of the k-step in read r
    const int h = lane >> 5, g = (lane >> 4) & 1, q4 = (lane >> 2) & 3, p4 = lane & 3;

    f32x4 acc[9][NJ];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int b = b0; b < b1; ++b) {
        const int img = b / bpi, y0 = (b - img * bpi) * a.R;
        const int P = min(a.R, a.OH - y0) * a.OW;
        const __amdgpu_buffer_rsrc_t rd = buf_rsrc_n(a.dY + img * dimg + c0, (dimg - c0) * 2);
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc_n(a.X + img * ximg + c0, (ximg - c0) * 2);
        const int pix0 = y0 * a.OW, iy0 = y0 * a.stride - 1;
        __syncthreads();  // the previous band's reads are done
        for (int id = tid; id < a.KP * 8; id += 256) {
            const int c = id & 7, row = id >> 3;
            const u32x4 v = buf_ld16(rd, row < P ? (uint32_t)(((pix0 + row) * a.C + c * 8) * 2) : BUF_OOB);
            *reinterpret_cast<u32x4*>(sD + row * 128 + (gw_slot(c, row) << 4)) = v;
        }
        for (int id0 = tid; id0 < nch; id0 += 1024) {
            u32x4 v[4];
            int dst[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int id = id0 + u * 256;
                const int c = id & 7, q = id >> 3;
                const int pr = q / a.PC, pc = q - pr * a.PC;
                const int iy = iy0 + pr, ix = pc - 1;
                const bool in = id < nch && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                v[u] = buf_ld16(rx, in ? (uint32_t)(((iy * a.W + ix) * a.C + c * 8) * 2) : BUF_OOB);
                dst[u] = id < nch ? q * 128 + (gw_slot(c, q) << 4) : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (dst[u] >= 0) *reinterpret_cast<u32x4*>(sP + dst[u]) = v[u];
        }
        __syncthreads();

        const int nks = (P + 31) >> 5;
        for (int ks = 0; ks < nks; ++ks) {
            int ad[2], q0[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int pk = ks * 32 + (2 * r + h) * 8 + 4 * g + q4;  // band pixel = k row
                ad[r] = pk * 128 + ((wid ^ gw_swz(pk)) << 5) + 8 * p4;
                const int pp = pk < P ? pk : 0;  // a padded k row (zero dY) reads a staged patch pixel: 0 x finite
                const int py = pp / a.OW, px = pp - py * a.OW;
                q0[r] = py * a.stride * a.PC + px * a.stride;
            }
            const bf16x8 fa = tr16_frag(sD + ad[0], sD + ad[1]);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ti = t / 3, tj = t - ti * 3;
                const int qa = q0[0] + ti * a.PC + tj, qb = q0[1] + ti * a.PC + tj;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const bf16x8 fb = tr16_frag(sP + qa * 128 + (((seg0 + j) ^ gw_swz(qa)) << 5) + 8 * p4,
                                                sP + qb * 128 + (((seg0 + j) ^ gw_swz(qb)) << 5) + 8 * p4);
                    acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[t][j], 0, 0, 0);
                }
            }
        }
    }

    // acc[t][j][r]: output channel 16 wid + 4 (lane >> 4) + r, input channel 16 (seg0 + j) + (lane & 15) of the slab;
    // only the pairs of one group exist in dW
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = 16 * wid + 4 * (lane >> 4) + r, ci = 16 * (seg0 + j) + (lane & 15);
            if (co / a.cg != ci / a.cg) continue;
            float* dst = a.dW + (size_t)(c0 + co) * 9 * a.cg + (ci % a.cg);
#pragma unroll
            for (int t = 0; t < 9; ++t) atomicAdd(dst + t * a.cg, acc[t][j][r]);
        }
}

constexpr size_t GC_PATCH_MAX = 72 * 1024;  // patch bytes per band
constexpr int GC_BAND_PIX = 256;            // band pixels

bool gconv_shape_ok(int C, int cg, int stride) {
    return C > 0 && C % 64 == 0 && (cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64) && C % cg == 0 &&
           (stride == 1 || stride == 2);
}

// rows per band: as many as keep the band within GC_BAND_PIX pixels and the patch within GC_PATCH_MAX bytes
int gconv_band_rows(int GH, int GW, int sA, int ey, int ex) {
    int R = std::max(1, std::min(GH, GC_BAND_PIX / std::max(1, GW)));
    while (R > 1 && (size_t)((R - 1) * sA + ey) * ((GW - 1) * sA + ex) * 128 > GC_PATCH_MAX) --R;
    return R;
}

int gconv_ranges(int nbands, int nslab) {
    return std::max(1, std::min(nbands, (4 * device_cus() + nslab - 1) / nslab));
}

template <typename K, typename A>
int gconv_go(K kern, const A& a, int nbands, size_t lds, hipStream_t st) {
    if (lds > 160 * 1024) return -106;
    const int nslab = a.C / 64, nranges = gconv_ranges(nbands, nslab);
    if (lds > 64 * 1024) {
        const hipError_t e =
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(nslab * nranges), dim3(256), lds, st, a, nbands, nranges);
    CONV_COUNTED();
    IMK_CHECK_LAUNCH();
    return 0;
}

// taps: ky in [0, 3) x kx in [0, 3) with row offset dy(ky) (or skipped where dy < -8), likewise columns
int gconv_launch(GConvArgs a, const int (&dys)[3], const int (&dxs)[3], hipStream_t st) {
    int miny = 99, maxy = -99, minx = 99, maxx = -99;
    for (int k = 0; k < 3; ++k) {
        if (dys[k] > -9) miny = std::min(miny, dys[k]), maxy = std::max(maxy, dys[k]);
        if (dxs[k] > -9) minx = std::min(minx, dxs[k]), maxx = std::max(maxx, dxs[k]);
    }
    a.ntap = 0, a.tapw = 0, a.tapdy = a.tapdx = 0;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            if (dys[ky] <= -9 || dxs[kx] <= -9) continue;
            a.tapw |= (uint64_t)(ky * 3 + kx) << (4 * a.ntap);
            a.tapdy |= (uint32_t)(dys[ky] - miny) << (2 * a.ntap);
            a.tapdx |= (uint32_t)(dxs[kx] - minx) << (2 * a.ntap);
            ++a.ntap;
        }
    a.y0off = miny, a.x0off = minx;
    const int ey = maxy - miny + 1, ex = maxx - minx + 1;
    a.R = gconv_band_rows(a.GH, a.GW, a.sA, ey, ex);
    a.PR = (a.R - 1) * a.sA + ey, a.PC = (a.GW - 1) * a.sA + ex;
    const int nbands = a.N * ((a.GH + a.R - 1) / a.R);
    const int KC = a.cg <= 16 ? 16 : a.cg;
    const size_t wp = KC * 2 + (KC == 64 ? 16 : 0);
    const size_t lds = (size_t)a.ntap * 64 * wp + (size_t)a.PR * a.PC * 128 + 4 * 16 * GC_EP;
    switch (KC) {
        case 16: return gconv_go(gconv_kernel<16>, a, nbands, lds, st);
        case 32: return gconv_go(gconv_kernel<32>, a, nbands, lds, st);
        default: return gconv_go(gconv_kernel<64>, a, nbands, lds, st);
    }
}

bool gconv_fits32(size_t h, size_t w, size_t c) { return h * w * c * 2 < (1ull << 31); }

}  // namespace

// y [N][OH][OW][C] = grouped conv3x3(x [N][H][W][C], w [C][3][3][cg]), pad 1; affine [2][C] / relu: the eval
// epilogue; stats / shift: the training epilogue's BatchNorm slab (conv_args.h). -106: a shape the kernels do not cover
IMK_EXPORT int imk_gconv_fwd(const void* x, const void* w, void* y, const void* affine, void* stats, const void* shift,
                             int N, int H, int W, int C, int cg, int stride, int relu, void* stream) {
    if (!gconv_shape_ok(C, cg, stride) || N < 1 || H < 1 || W < 1 || !gconv_fits32(H, W, C)) return -106;
    GConvArgs a{};
    a.X = (const bf16_t*)x, a.Wk = (const bf16_t*)w, a.Y = (bf16_t*)y;
    a.affine = (const float*)affine, a.stats = (float*)stats, a.shift = (const float*)shift;
    a.N = N, a.H = H, a.W = W, a.C = C, a.cg = cg;
    a.GH = a.YH = (H - 1) / stride + 1, a.GW = a.YW = (W - 1) / stride + 1;
    a.sY = 1, a.oy = a.ox = 0, a.sA = stride, a.relu = relu;
    const int d[3] = {-1, 0, 1};
    return gconv_launch(a, d, d, (hipStream_t)stream);
}

// dx [N][H][W][C] = dgrad(dy [N][OH][OW][C], wt [C][3][3][cg] per-group transposed); every dx pixel is written
IMK_EXPORT int imk_gconv_dgrad(const void* dy, const void* wt, void* dx, int N, int OH, int OW, int C, int cg, int H,
                               int W, int stride, void* stream) {
    if (!gconv_shape_ok(C, cg, stride) || N < 1 || OH != (H - 1) / stride + 1 || OW != (W - 1) / stride + 1 ||
        !gconv_fits32(H, W, C))
        return -106;
    GConvArgs a{};
    a.X = (const bf16_t*)dy, a.Wk = (const bf16_t*)wt, a.Y = (bf16_t*)dx;
    a.N = N, a.H = OH, a.W = OW, a.C = C, a.cg = cg;
    a.YH = H, a.YW = W, a.sA = 1;
    if (stride == 1) {  // dx[y] = sum_ky dy[y + 1 - ky] w[ky]: the mirrored taps
        a.GH = H, a.GW = W, a.sY = 1;
        const int d[3] = {1, 0, -1};
        return gconv_launch(a, d, d, (hipStream_t)stream);
    }
    // stride 2: dx row 2 r + ph takes tap ky where ph + 1 - ky is even, from dy row r + (ph + 1 - ky) / 2
    const int dcls[2][3] = {{-9, 0, -9}, {1, -9, 0}};
    for (int ph = 0; ph < 2; ++ph)
        for (int pw = 0; pw < 2; ++pw) {
            a.GH = (H - ph + 1) / 2, a.GW = (W - pw + 1) / 2;
            if (a.GH < 1 || a.GW < 1) continue;
            a.sY = 2, a.oy = ph, a.ox = pw;
            const int rc = gconv_launch(a, dcls[ph], dcls[pw], (hipStream_t)stream);
            if (rc) return rc;
        }
    return 0;
}

// dw [C][3][3][cg] fp32 += wgrad(dy [N][OH][OW][C], x [N][H][W][C])
IMK_EXPORT int imk_gconv_wgrad(const void* dy, const void* x, void* dw, int N, int H, int W, int C, int cg, int OH,
                               int OW, int stride, void* stream) {
    if (!gconv_shape_ok(C, cg, stride) || N < 1 || OH != (H - 1) / stride + 1 || OW != (W - 1) / stride + 1 ||
        !gconv_fits32(H, W, C))
        return -106;
    GWgradArgs a{};
    a.dY = (const bf16_t*)dy, a.X = (const bf16_t*)x, a.dW = (float*)dw;
    a.N = N, a.H = H, a.W = W, a.C = C, a.cg = cg, a.OH = OH, a.OW = OW, a.stride = stride;
    a.R = gconv_band_rows(OH, OW, stride, 3, 3);
    a.PR = (a.R - 1) * stride + 3, a.PC = (OW - 1) * stride + 3;
    a.KP = (a.R * OW + 31) / 32 * 32;
    const int nbands = N * ((OH + a.R - 1) / a.R);
    const size_t lds = (size_t)a.KP * 128 + (size_t)a.PR * a.PC * 128;
    switch (cg <= 16 ? 16 : cg) {
        case 16: return gconv_go(gconv_wgrad_kernel<16>, a, nbands, lds, (hipStream_t)stream);
        case 32: return gconv_go(gconv_wgrad_kernel<32>, a, nbands, lds, (hipStream_t)stream);
        default: return gconv_go(gconv_wgrad_kernel<64>, a, nbands, lds, (hipStream_t)stream);
    }
}
