// Narrow 3x3 convolutions (pad 1) of the ResNet-D deep stem on NHWC bf16 (gfx950): forward, input gradient and
// weight gradient of
//   conv A   4 (3 real) -> 32 channels, stride 2     conv B   32 -> 32, stride 1     conv C   32 -> 64, stride 1
// at the network's largest maps (112 x 112). At 32 .. 64 channels they are HBM streams (~144 flop / byte), so all
// three kernels are organised like the grouped convs (conv_group.hip): a persistent grid sized to the CUs, each block
// owning a contiguous range of BANDS -- R output rows x a width tile of TW output columns of one image. Per band the
// input patch (band + halo) is staged in LDS once through 16-byte buffer loads based at the image (out-of-image
// taps are out-of-range offsets: zeros; the 4-channel image: one 8-byte load per pixel) and the nine taps read it as
// shifted windows. The whole weight tensor (at most 64 x 288 bf16) sits in LDS for the block's lifetime.
//
// Forward / stride-1 dgrad (one kernel): wave w takes the band's 16-pixel groups w, w + 4, ... With 32 input channels
// one tap is one v_mfma_f32_16x16x32_bf16 k-step per 16-channel output tile (64 channels, the dgrad of conv C: two).
// The weights are the MFMA's first operand and the pixels its second, so a lane ends up with 4 consecutive channels
// of ONE pixel and the accumulator goes to the wave's fp32 LDS tile as one 16-byte write (with the pixels first the
// lane would hold one channel of 4 pixels: four scattered writes; the products are the same). For the 4-channel
// image a kernel row is 3 taps x 4 channels = 12 contiguous bf16: it is padded to 16 and runs as one
// v_mfma_f32_16x16x16_bf16 per kernel row, K = 48 for 36 real values (25 % padding; the 16x16x32 shape would pad a
// row to 32: 62 %). The padded lanes multiply zero weights with staged (finite) pixels.
// Epilogue (the contract of conv_args.h / conv_epilogue.h): the fp32 tile is read back so that a lane owns one
// 16-byte chunk -- a fixed 8 channels -- of a pixel: affine -> ReLU -> bf16 store -> shifted BatchNorm sums of the
// STORED values in registers. The dgrad is the forward on the transposed shadow [Ci][3][3][Co] with mirrored taps.
// Weight gradient: pixels are the MFMA k index; the dY band and the X patch are read with transposing LDS loads
// (ds_read_b64_tr_b16, lanes as in conv_group.hip). A wave keeps its [16 co][9 taps][16 or 32 ci] accumulators over
// the block's whole band range.
// No float atomics: every block writes its BatchNorm sums / its weight-gradient accumulators as one fp32 PARTIAL,
// and a second small launch (nconv_fold_kernel) adds the partials in index order to the slab / the gradient slot.
// Two runs give the same bits, and no kernel argument changes from step to step.
// All global accesses go through buffer descriptors based at the band's image, 32-bit offsets inside.

#include <algorithm>

#include "conv_epilogue.h"

namespace {

constexpr int NC_R = 8, NC_TW = 32;  // band: output rows x output columns (256 pixels: 16 groups of 16)

struct NConvArgs {
    const bf16_t* X;      // operand NHWC [N][H][W][CI]
    const bf16_t* Wk;     // [CO][3][3][cw] (cw = CI, or 3 / 4 for the image)
    bf16_t* Y;            // output NHWC [N][OH][OW][CO]
    const float* affine;  // [2][CO] scale, shift, or null
    float* part;          // [blocks][2][CO] statistics partials, or null
    const float* shift;   // [CO] or null
    int N, H, W, OH, OW, stride, cw, mirror, relu;
    int nbx, nby;         // width tiles / bands per image
    int PR, PC;           // patch rows / columns
};

struct NWgradArgs {
    const bf16_t* dY;  // [N][OH][OW][CO]
    const bf16_t* X;   // [N][H][W][CI]
    float* part;       // [blocks * PW][CO][9][CI] fp32 partials
    int N, H, W, OH, OW, stride;
    int nbx, nby, PR, PC;
};

__device__ __forceinline__ u32x2 buf_ld8(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
}

// physical 16-B chunk of logical chunk c of LDS row q with NSEG 32-byte segments per row (tr16 reads: 4 consecutive
// rows x 32 B per 16-lane group)
template <int NSEG>
__device__ __forceinline__ int nw_slot(int c, int q) { return (((c >> 1) ^ ((q >> 1) & (NSEG - 1))) << 1) | (c & 1); }

template <int CI>
constexpr int nc_wpitch() { return CI == 4 ? 40 : CI * 2 + 16; }  // bytes per output channel and tap (kernel row)

template <int CI, int CO>
__global__ __launch_bounds__(256) void nconv_kernel(const NConvArgs a, int nbands, int nranges) {
    constexpr int WP = nc_wpitch<CI>();
    constexpr int NT = CO / 16;              // 16-channel output tiles
    constexpr int CB = CI * 2;               // operand bytes per pixel
    constexpr int NCH = CI == 4 ? 1 : CI / 8;  // 16-B chunks per operand pixel
    constexpr int NWR = CI == 4 ? 3 : 9;     // weight rows per output channel: kernel rows / taps
    constexpr int CH = CO / 8;               // 16-B chunks per output pixel
    constexpr int EP = CO * 4 + 16;          // fp32 staging pitch per pixel
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sW = smem;                         // [NWR][CO][WP]
    char* sP = sW + ((NWR * CO * WP + 15) & ~15);  // [PR][PC][CB] patch; chunk c of pixel q at c ^ (q & (NCH - 1))
    char* sE = sP + ((a.PR * a.PC * CB + 15) & ~15);  // [4 waves][16 px][EP] fp32 staging

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int range = blockIdx.x;
    const int b0 = (int)((long)nbands * range / nranges), b1 = (int)((long)nbands * (range + 1) / nranges);
    const int bpi = a.nbx * a.nby;

    if constexpr (CI == 4) {  // [ky][co][16]: k = 4 kx + c, zeros at kx = 3 and c >= cw
        for (int id = tid; id < 3 * CO * 16; id += 256) {
            const int k = id & 15, n = (id >> 4) % CO, ky = id / (16 * CO);
            const int kx = k >> 2, c = k & 3;
            bf16_t v = 0;
            if (kx < 3 && c < a.cw) v = a.Wk[((size_t)(n * 3 + ky) * 3 + kx) * a.cw + c];
            *reinterpret_cast<bf16_t*>(sW + (ky * CO + n) * WP + k * 2) = v;
        }
    } else {
        constexpr int NPC = CI / 4;  // 8-byte pieces per tap
        for (int id = tid; id < 9 * CO * NPC; id += 256) {
            const int j = id % NPC, t = (id / NPC) % 9, n = id / (NPC * 9);
            const u32x2 v = *reinterpret_cast<const u32x2*>(a.Wk + ((size_t)n * 9 + t) * CI + j * 4);
            *reinterpret_cast<u32x2*>(sW + (t * CO + n) * WP + j * 8) = v;
        }
    }

    const int fr = lane & 15, kq = lane >> 4;
    const int ec = lane % CH, epx = lane / CH;  // epilogue: this lane's 8-channel chunk, its pixel of a pass
    const bool want_st = a.part != nullptr;
    float csh[8], asc[8], ash[8], s1[8], s2[8];
    load8(want_st && a.shift != nullptr, a.shift, ec * 8, csh);
    load8(a.affine != nullptr, a.affine, ec * 8, asc, 1.f);
    load8(a.affine != nullptr, a.affine + CO, ec * 8, ash);
#pragma unroll
    for (int c = 0; c < 8; ++c) s1[c] = s2[c] = 0.f;
    char* eW = sE + wid * 16 * EP;
    const size_t ximg = (size_t)a.H * a.W * CI, yimg = (size_t)a.OH * a.OW * CO;
    const int npx = a.PR * a.PC;  // patch pixels
    const int s = a.stride;

    for (int b = b0; b < b1; ++b) {
        const int img = b / bpi, rem = b - img * bpi;
        const int by = rem / a.nbx, bx = rem - by * a.nbx;
        const int y0 = by * NC_R, x0 = bx * NC_TW;
        const int tw = min(NC_TW, a.OW - x0);
        const int P = min(NC_R, a.OH - y0) * tw;  // band pixels
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc_n(a.X + img * ximg, ximg * 2);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc_n(a.Y + img * yimg, yimg * 2);
        const int iy0 = y0 * s - 1, ix0 = x0 * s - 1;
        __syncthreads();  // the previous band's patch reads are done (first band: the weights are in)
        if constexpr (CI == 4) {
            for (int q = tid; q < npx; q += 256) {
                const int pr = q / a.PC, pc = q - pr * a.PC;
                const int iy = iy0 + pr, ix = ix0 + pc;
                const bool in = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                *reinterpret_cast<u32x2*>(sP + q * 8) = buf_ld8(rx, in ? (uint32_t)((iy * a.W + ix) * 8) : BUF_OOB);
            }
        } else {
            for (int id = tid; id < npx * NCH; id += 256) {
                const int c = id % NCH, q = id / NCH;
                const int pr = q / a.PC, pc = q - pr * a.PC;
                const int iy = iy0 + pr, ix = ix0 + pc;
                const bool in = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const u32x4 v = buf_ld16(rx, in ? (uint32_t)(((iy * a.W + ix) * CI + c * 8) * 2) : BUF_OOB);
                *reinterpret_cast<u32x4*>(sP + q * CB + ((c ^ (q & (NCH - 1))) << 4)) = v;
            }
        }
        __syncthreads();

        const int ng = (P + 15) >> 4;
        for (int g = wid; g < ng; g += 4) {
            const int p = min(g * 16 + fr, P - 1);  // rows past the band repeat its last pixel (never stored)
            const int gy = p / tw, gx = p - gy * tw;
            const int q0 = gy * s * a.PC + gx * s;
            f32x4 acc[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (CI == 4) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    // taps kx = kq of kernel row ky: the pixel at column offset kq (kq = 3: zero weights)
                    const s16x4 fx = *reinterpret_cast<const s16x4*>(sP + (q0 + ky * a.PC + kq) * 8);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const s16x4 fw = *reinterpret_cast<const s16x4*>(sW + (ky * CO + nt * 16 + fr) * WP + kq * 8);
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fw, fx, acc[nt], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int ky = t / 3, kx = t - ky * 3;
                    const int q = q0 + (a.mirror ? 2 - ky : ky) * a.PC + (a.mirror ? 2 - kx : kx);
                    const char* row = sP + q * CB;
                    const int sw = q & (NCH - 1);
#pragma unroll
                    for (int ks = 0; ks < CI / 32; ++ks) {
                        const bf16x8 fx = *reinterpret_cast<const bf16x8*>(row + (((ks * 4 + kq) ^ sw) << 4));
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            const bf16x8 fw = *reinterpret_cast<const bf16x8*>(sW + (t * CO + nt * 16 + fr) * WP +
                                                                               ks * 64 + kq * 16);
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fx, acc[nt], 0, 0, 0);
                        }
                    }
                }
            }
            // lane holds channels 16 nt + 4 kq + r of pixel fr -> the wave's fp32 staging tile (written and read
            // back by this wave only: LDS order, no block barrier)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                *reinterpret_cast<f32x4*>(eW + fr * EP + (nt * 16 + kq * 4) * 4) = acc[nt];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int k = 0; k < CH / 4; ++k) {
                const int px = epx + (64 / CH) * k, pp = g * 16 + px;
                const bool valid = pp < P;
                float v[8];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const f32x4 tv = *reinterpret_cast<const f32x4*>(eW + px * EP + ec * 32 + hh * 16);
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
                const int py = pp / tw, pxx = pp - py * tw;
                buf_st16(ry, valid ? (uint32_t)((((y0 + py) * a.OW + x0 + pxx) * CO + ec * 8) * 2) : BUF_OOB, o);
                if (want_st) stat_fwd(o, valid ? 1.f : 0.f, csh, s1, s2);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if (!want_st) return;
    // the block's sums: lanes that share a chunk, then the four waves in order, one partial row per block
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int o = CH; o < 64; o <<= 1) {
            s1[c] += __shfl_xor(s1[c], o, 64);
            s2[c] += __shfl_xor(s2[c], o, 64);
        }
    __syncthreads();  // every wave is done with its staging tile
    float* sS = reinterpret_cast<float*>(sE);  // [4 waves][2][CO]
    if (lane < CH) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            sS[(wid * 2 + 0) * CO + ec * 8 + c] = s1[c];
            sS[(wid * 2 + 1) * CO + ec * 8 + c] = s2[c];
        }
    }
    __syncthreads();
    if (tid < 2 * CO)
        a.part[(size_t)blockIdx.x * 2 * CO + tid] =
            ((sS[tid] + sS[2 * CO + tid]) + sS[4 * CO + tid]) + sS[6 * CO + tid];
}

// CI = 32: wave w owns output tile w % NT (16 channels) against NJ 16-channel input segments for all 9 taps.
// CI = 4: wave w owns output tile w & 1 for the 3 kernel rows (16 columns = 4 taps x 4 channels, the 4th tap unused)
// and every second k-step (w >> 1): two partials per block.
template <int CI, int CO>
__global__ __launch_bounds__(256) void nconv_wgrad_kernel(const NWgradArgs a, int nbands, int nranges) {
    constexpr int NT = CO / 16;
    constexpr int DB = CO * 2;                       // dY bytes per pixel
    constexpr int NJ = CI == 4 ? 1 : 2 * NT / 4;     // input segments per wave
    constexpr int NA = CI == 4 ? 3 : 9;              // accumulator rows: kernel rows / taps
    constexpr int KP = NC_R * NC_TW;                 // k rows staged per band
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sD = smem;             // [KP][DB] dY band (rows past the band: zeros)
    char* sP = smem + KP * DB;   // [PR][PC][CI * 2] X patch

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int range = blockIdx.x;
    const int b0 = (int)((long)nbands * range / nranges), b1 = (int)((long)nbands * (range + 1) / nranges);
    const int bpi = a.nbx * a.nby;
    const size_t ximg = (size_t)a.H * a.W * CI, dimg = (size_t)a.OH * a.OW * CO;
    const int npx = a.PR * a.PC, s = a.stride;
    const int tile = CI == 4 ? (wid & 1) : wid % NT;
    const int seg0 = CI == 4 ? 0 : (wid / NT) * NJ;
    const int kpar = CI == 4 ? (wid >> 1) : 0, kstep = CI == 4 ? 2 : 1;

    // tr16 fragment lanes (conv_group.hip): lane 4 q + p of a 16-lane group reads row q, columns 4 p .. 4 p + 3 of a
    // 16-channel segment; the 32-lane half h reads rows 8 (2 r + h) + 4 g + q of the k-step in read r
    const int h = lane >> 5, g = (lane >> 4) & 1, q4 = (lane >> 2) & 3, p4 = lane & 3;

    f32x4 acc[NA][NJ];
#pragma unroll
    for (int t = 0; t < NA; ++t)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int b = b0; b < b1; ++b) {
        const int img = b / bpi, rem = b - img * bpi;
        const int by = rem / a.nbx, bx = rem - by * a.nbx;
        const int y0 = by * NC_R, x0 = bx * NC_TW;
        const int tw = min(NC_TW, a.OW - x0);
        const int P = min(NC_R, a.OH - y0) * tw;
        const __amdgpu_buffer_rsrc_t rd = buf_rsrc_n(a.dY + img * dimg, dimg * 2);
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc_n(a.X + img * ximg, ximg * 2);
        const int iy0 = y0 * s - 1, ix0 = x0 * s - 1;
        __syncthreads();  // the previous band's reads are done
        for (int id = tid; id < KP * (CO / 8); id += 256) {
            const int c = id % (CO / 8), row = id / (CO / 8);
            const int py = row / tw, px = row - py * tw;
            const u32x4 v =
                buf_ld16(rd, row < P ? (uint32_t)((((y0 + py) * a.OW + x0 + px) * CO + c * 8) * 2) : BUF_OOB);
            *reinterpret_cast<u32x4*>(sD + row * DB + (nw_slot<NT>(c, row) << 4)) = v;
        }
        if constexpr (CI == 4) {
            for (int q = tid; q < npx; q += 256) {
                const int pr = q / a.PC, pc = q - pr * a.PC;
                const int iy = iy0 + pr, ix = ix0 + pc;
                const bool in = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                *reinterpret_cast<u32x2*>(sP + q * 8) = buf_ld8(rx, in ? (uint32_t)((iy * a.W + ix) * 8) : BUF_OOB);
            }
        } else {
            for (int id = tid; id < npx * (CI / 8); id += 256) {
                const int c = id % (CI / 8), q = id / (CI / 8);
                const int pr = q / a.PC, pc = q - pr * a.PC;
                const int iy = iy0 + pr, ix = ix0 + pc;
                const bool in = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const u32x4 v = buf_ld16(rx, in ? (uint32_t)(((iy * a.W + ix) * CI + c * 8) * 2) : BUF_OOB);
                *reinterpret_cast<u32x4*>(sP + q * (CI * 2) + (nw_slot<CI / 16>(c, q) << 4)) = v;
            }
        }
        __syncthreads();

        const int nks = (P + 31) >> 5;
        for (int ks = kpar; ks < nks; ks += kstep) {
            int ad[2], q0[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int pk = ks * 32 + (2 * r + h) * 8 + 4 * g + q4;  // band pixel = k row
                ad[r] = pk * DB + ((tile ^ ((pk >> 1) & (NT - 1))) << 5) + 8 * p4;
                const int pp = pk < P ? pk : 0;  // a padded k row (zero dY) reads a staged patch pixel: 0 x finite
                const int py = pp / tw, px = pp - py * tw;
                q0[r] = py * s * a.PC + px * s;
            }
            const bf16x8 fa = tr16_frag(sD + ad[0], sD + ad[1]);
            if constexpr (CI == 4) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    // the 16 columns of kernel row ky: pixels at column offsets 0 .. 3 (p4), 4 channels each
                    const bf16x8 fb = tr16_frag(sP + (q0[0] + ky * a.PC + p4) * 8, sP + (q0[1] + ky * a.PC + p4) * 8);
                    acc[ky][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[ky][0], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int ti = t / 3, tj = t - ti * 3;
                    const int qa = q0[0] + ti * a.PC + tj, qb = q0[1] + ti * a.PC + tj;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        constexpr int XS = CI / 16;
                        const bf16x8 fb =
                            tr16_frag(sP + qa * (CI * 2) + (((seg0 + j) ^ ((qa >> 1) & (XS - 1))) << 5) + 8 * p4,
                                      sP + qb * (CI * 2) + (((seg0 + j) ^ ((qb >> 1) & (XS - 1))) << 5) + 8 * p4);
                        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[t][j], 0, 0, 0);
                    }
                }
            }
        }
    }

    // acc[t][j][r]: output channel 16 tile + 4 (lane >> 4) + r; column lane & 15 of input segment seg0 + j (CI = 4:
    // tap kx = column >> 2, channel column & 3 of kernel row t)
    float* part = a.part + (size_t)(blockIdx.x * kstep + kpar) * CO * 9 * CI;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = 16 * tile + 4 * (lane >> 4) + r, col = lane & 15;
        if constexpr (CI == 4) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
                if (col < 12) part[(co * 9 + ky * 3) * 4 + col] = acc[ky][0][r];
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < 9; ++t) part[(co * 9 + t) * CI + 16 * (seg0 + j) + col] = acc[t][j][r];
        }
    }
}

// dst[(i / ci) * cw + i % ci] += part[0][i] + part[1][i] + ... in index order, for i % ci < cw (ci = cw = 1: a plain
// vector). One thread per element: the only writer of its destination
__global__ __launch_bounds__(256) void nconv_fold_kernel(const float* __restrict__ part, int nparts, int n, int ci,
                                                         int cw, float* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sum = 0.f;
    for (int k = 0; k < nparts; ++k) sum += part[(size_t)k * n + i];
    const int c = i % ci;
    if (c < cw) dst[(size_t)(i / ci) * cw + c] += sum;
}

bool nconv_shape_ok(int Ci, int Co, int stride) {
    return (Ci == 4 && Co == 32 && stride == 2) || (Ci == 32 && (Co == 32 || Co == 64) && stride == 1) ||
           (Ci == 64 && Co == 32 && stride == 1);
}

bool nconv_fits32(size_t h, size_t w, size_t c) { return h * w * c * 2 < (1ull << 31); }

// blocks of the persistent grid: two per CU (the forward's LDS: 75 .. 100 KB of 160), at most one per band
int nconv_ranges(int nbands) { return std::max(1, std::min(nbands, 2 * device_cus())); }

void nconv_geom(int OH, int OW, int stride, int extra, int& nbx, int& nby, int& PR, int& PC) {
    nbx = (OW + NC_TW - 1) / NC_TW, nby = (OH + NC_R - 1) / NC_R;
    PR = (NC_R - 1) * stride + 3, PC = (NC_TW - 1) * stride + 3 + extra;
}

template <typename K, typename A>
int nconv_go(K kern, const A& a, int nbands, int nranges, size_t lds, hipStream_t st) {
    if (lds > 160 * 1024) return -106;
    if (lds > 64 * 1024) {
        const hipError_t e =
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(nranges), dim3(256), lds, st, a, nbands, nranges);
    CONV_COUNTED();
    IMK_CHECK_LAUNCH();
    return 0;
}

int nconv_fold(const float* part, int nparts, int n, int ci, int cw, float* dst, hipStream_t st) {
    hipLaunchKernelGGL(nconv_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, st, part, nparts, n, ci, cw, dst);
    IMK_CHECK_LAUNCH();
    return 0;
}

template <int CI, int CO>
int nconv_run(NConvArgs a, float* stats, hipStream_t st) {
    nconv_geom(a.OH, a.OW, a.stride, CI == 4 ? 1 : 0, a.nbx, a.nby, a.PR, a.PC);
    const int nbands = a.N * a.nbx * a.nby, nranges = nconv_ranges(nbands);
    constexpr int NWR = CI == 4 ? 3 : 9;
    const size_t lds = ((size_t)(NWR * CO * nc_wpitch<CI>() + 15) & ~(size_t)15) +
                       (((size_t)a.PR * a.PC * CI * 2 + 15) & ~(size_t)15) + (size_t)4 * 16 * (CO * 4 + 16);
    if (stats == nullptr) a.part = nullptr;
    const int rc = nconv_go(nconv_kernel<CI, CO>, a, nbands, nranges, lds, st);
    if (rc || stats == nullptr) return rc;
    return nconv_fold(a.part, nranges, 2 * CO, 1, 1, stats, st);  // slab slot 0 (zeroed per step) += the block sums
}

template <int CI, int CO>
int nconv_wgrad_run(NWgradArgs a, float* dw, int cw, hipStream_t st) {
    nconv_geom(a.OH, a.OW, a.stride, CI == 4 ? 1 : 0, a.nbx, a.nby, a.PR, a.PC);
    const int nbands = a.N * a.nbx * a.nby, nranges = nconv_ranges(nbands);
    const size_t lds = (size_t)NC_R * NC_TW * CO * 2 + (size_t)a.PR * a.PC * CI * 2;
    const int rc = nconv_go(nconv_wgrad_kernel<CI, CO>, a, nbands, nranges, lds, st);
    if (rc) return rc;
    return nconv_fold(a.part, nranges * (CI == 4 ? 2 : 1), CO * 9 * CI, CI, cw, dw, st);
}

}  // namespace

// fp32 workspace the calls below need for their partials (`ws`): forward with statistics (wgrad 0) / weight gradient
IMK_EXPORT long imk_nconv_ws_floats(int N, int OH, int OW, int Ci, int Co, int wgrad) {
    const int nbands = N * ((OW + NC_TW - 1) / NC_TW) * ((OH + NC_R - 1) / NC_R);
    const long blocks = nconv_ranges(nbands);
    return wgrad ? blocks * (Ci == 4 ? 2 : 1) * Co * 9 * Ci : blocks * 2 * Co;
}

// y [N][OH][OW][Co] = conv3x3(x [N][H][W][Ci], w [Co][3][3][cw]), pad 1; mirror: the taps mirrored (the stride-1
// dgrad on the transposed shadow). affine [2][Co] / relu: the eval epilogue; stats (slot 0 of the [STAT_SLOTS][2][Co]
// slab, +=) / shift / ws: the training epilogue's BatchNorm sums. -106: a shape the kernels do not cover
IMK_EXPORT int imk_nconv_fwd(const void* x, const void* w, void* y, const void* affine, void* stats, const void* shift,
                             void* ws, int N, int H, int W, int Ci, int Co, int cw, int stride, int mirror, int relu,
                             void* stream) {
    if (!nconv_shape_ok(Ci, Co, stride) || N < 1 || H < 1 || W < 1 || !nconv_fits32(H, W, std::max(Ci, Co)) ||
        (Ci == 4 ? (cw < 1 || cw > 4 || mirror) : cw != Ci) || (stats != nullptr && ws == nullptr))
        return -106;
    NConvArgs a{};
    a.X = (const bf16_t*)x, a.Wk = (const bf16_t*)w, a.Y = (bf16_t*)y;
    a.affine = (const float*)affine, a.part = (float*)ws, a.shift = (const float*)shift;
    a.N = N, a.H = H, a.W = W, a.stride = stride, a.cw = cw, a.mirror = mirror, a.relu = relu;
    a.OH = (H - 1) / stride + 1, a.OW = (W - 1) / stride + 1;
    hipStream_t st = (hipStream_t)stream;
    if (Ci == 4) return nconv_run<4, 32>(a, (float*)stats, st);
    if (Ci == 64) return nconv_run<64, 32>(a, (float*)stats, st);
    return Co == 32 ? nconv_run<32, 32>(a, (float*)stats, st) : nconv_run<32, 64>(a, (float*)stats, st);
}

// dw [Co][3][3][cw] fp32 += wgrad(dy [N][OH][OW][Co], x [N][H][W][Ci]) (cw = Ci, or 3 / 4 for the 4-channel image)
IMK_EXPORT int imk_nconv_wgrad(const void* dy, const void* x, void* dw, void* ws, int N, int H, int W, int Ci, int Co,
                               int cw, int stride, void* stream) {
    if (!nconv_shape_ok(Ci, Co, stride) || Ci == 64 || N < 1 || H < 1 || W < 1 || ws == nullptr ||
        !nconv_fits32(H, W, std::max(Ci, Co)) || (Ci == 4 ? (cw < 1 || cw > 4) : cw != Ci))
        return -106;
    NWgradArgs a{};
    a.dY = (const bf16_t*)dy, a.X = (const bf16_t*)x, a.part = (float*)ws;
    a.N = N, a.H = H, a.W = W, a.stride = stride;
    a.OH = (H - 1) / stride + 1, a.OW = (W - 1) / stride + 1;
    hipStream_t st = (hipStream_t)stream;
    if (Ci == 4) return nconv_wgrad_run<4, 32>(a, (float*)dw, cw, st);
    return Co == 32 ? nconv_wgrad_run<32, 32>(a, (float*)dw, cw, st) : nconv_wgrad_run<32, 64>(a, (float*)dw, cw, st);
}
