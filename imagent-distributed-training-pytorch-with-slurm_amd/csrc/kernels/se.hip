// Squeeze-and-excitation block tail (SE-ResNet / SE-ResNeXt) on NHWC bf16 (gfx950):
//     out = relu(s[n,c] * u + idt),  u = sc_c * a + sh_c (the block's last training BatchNorm applied to the raw conv
//     output a),  s = sigmoid(W2 relu(W1 z + b1) + b2),  z[n,c] = mean_hw u = sc_c * X1[n,c] / HW + sh_c.
//
// Forward: one extra streaming pass (se_reduce_kernel<false>: X1 = sum_hw a, the affine applied to the pooled value),
// one small launch for the gate (se_excite_fwd_kernel, bf16 MFMA) and the tail pass (se_scale_add_relu_kernel).
// Backward: se_reduce_kernel<true> writes g = dout * [out > 0] and the per-(n,c) sums G1 = sum_hw g, G2 = sum_hw g a;
// everything that does not scale with HW follows from them (dS = sc G2 + sh G1, the gate's backward, the SE weight
// gradients and the BatchNorm's two reductions: sum du = sum_n (s G1 + HW dpool), sum du xhat = invstd sum_n [s (G2 -
// mean G1) + dpool (X1 - HW mean)]) in se_excite_bwd_tile_kernel / se_wgrad_partial_kernel / se_excite_bwd_fold_kernel;
// se_bn_apply_bwd_kernel is then the BatchNorm's usual apply pass with du = s g + dpool recomputed per element.
//
// Every reduction has a fixed order: per-block partials go to a workspace and are folded in index order; no kernel
// here uses a float atomic, and none takes an argument that changes from step to step.
#include "common.h"

namespace {

constexpr int SE_T = 256;   // threads per block
constexpr int SE_NT = 16;   // samples per gate tile: the column tile of one 16x16 MFMA
constexpr int SE_RMAX = 128;  // widest bottleneck of the gate (C = 2048)

struct f8 {
    float v[8];
};

__device__ __forceinline__ f8 ld8(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    return f8{{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}};
}
__device__ __forceinline__ void st8(float* p, const f8& x) {
    *reinterpret_cast<f32x4*>(p) = f32x4{x.v[0], x.v[1], x.v[2], x.v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{x.v[4], x.v[5], x.v[6], x.v[7]};
}
__device__ __forceinline__ f8 bf8(u32x4 w) {
    return f8{{lo_bf(w[0]), hi_bf(w[0]), lo_bf(w[1]), hi_bf(w[1]), lo_bf(w[2]), hi_bf(w[2]), lo_bf(w[3]), hi_bf(w[3])}};
}
__device__ __forceinline__ u32x4 pack8(const f8& x) {
    return u32x4{pack_bf2(x.v[0], x.v[1]), pack_bf2(x.v[2], x.v[3]), pack_bf2(x.v[4], x.v[5]), pack_bf2(x.v[6], x.v[7])};
}
__device__ __forceinline__ u32x4 ld16(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
// x = hi + mid + lo in bf16 terms (the residuals are exact in fp32); returns hi and leaves the rest in x
__device__ __forceinline__ bf16_t split_bf(float& x) {
    const bf16_t b = f2bf(x);
    x -= bf2f(b);
    return b;
}
__device__ __forceinline__ void split8(f8 x, bf16x8 out[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t lo = split_bf(x.v[2 * j]), hi = split_bf(x.v[2 * j + 1]);
            w[j] = lo | (hi << 16);
        }
        out[k] = __builtin_bit_cast(bf16x8, u32x4{w[0], w[1], w[2], w[3]});
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The pooled sums of one streaming pass. A block owns (sample n, slab of SC 16-byte chunks = 8 SC channels, rows
// [split * rows, (split + 1) * rows) of the HW pixels): lane (rs, cl) walks rows rs, rs + RB, .. (RB = 256 / SC) of chunk
// cl, four rows in flight, keeps its 8 channel sums in registers, and the RB row classes are then added in index order
// through LDS. part [S][K][N][C] (K = 1: X1; K = 2: G1, G2); with S = 1 that is the result itself.
// BWD: also writes g = dout where out > 0, else 0.
template <bool BWD>
__global__ __launch_bounds__(SE_T) void se_reduce_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ dout,
                                                         const bf16_t* __restrict__ out, bf16_t* __restrict__ g,
                                                         float* __restrict__ part, int N, int HW, int C, int SC,
                                                         int slabs, int S, int rows) {
    __shared__ float red[SE_T * 8];
    const int t = threadIdx.x;
    int b = blockIdx.x;
    const int split = b % S;
    b /= S;
    const int slab = b % slabs, n = b / slabs;
    const int RB = SE_T / SC, cl = t % SC, rs = t / SC;
    const int c8 = slab * SC + cl;
    const bool on = c8 < (C >> 3);
    const int r0 = split * rows, r1 = min(HW, r0 + rows);
    const size_t base = (size_t)n * HW * C + (size_t)c8 * 8;
    f8 s1{}, s2{};
    if (on) {
        for (int r = r0 + rs; r < r1; r += 4 * RB) {
            u32x4 va[4], vd[4], vo[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rr = r + u * RB;
                const size_t o = base + (size_t)(rr < r1 ? rr : r) * C;  // (a row past the range re-reads row r)
                va[u] = ld16(a + o);
                if (BWD) {
                    vd[u] = ld16(dout + o);
                    vo[u] = ld16(out + o);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rr = r + u * RB;
                if (rr >= r1) break;
                const f8 fa = bf8(va[u]);
                if (BWD) {
                    u32x4 vg;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t m = (lo_bf(vo[u][j]) > 0.f ? 0x0000ffffu : 0u) |
                                           (hi_bf(vo[u][j]) > 0.f ? 0xffff0000u : 0u);
                        vg[j] = vd[u][j] & m;
                    }
                    *reinterpret_cast<u32x4*>(g + base + (size_t)rr * C) = vg;
                    const f8 fg = bf8(vg);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        s1.v[j] += fg.v[j];
                        s2.v[j] = fmaf(fg.v[j], fa.v[j], s2.v[j]);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) s1.v[j] += fa.v[j];
                }
            }
        }
    }
    const int wid = SC * 8;  // channels of the slab
#pragma unroll
    for (int k = 0; k < (BWD ? 2 : 1); ++k) {
        if (k) __syncthreads();
        const f8& sv = k ? s2 : s1;
#pragma unroll
        for (int j = 0; j < 8; ++j) red[rs * wid + cl * 8 + j] = sv.v[j];
        __syncthreads();
        const int c = slab * wid + t;
        if (t < wid && c < C) {
            float acc = red[t];
            for (int q = 1; q < RB; ++q) acc += red[q * wid + t];
            part[(((size_t)split * (BWD ? 2 : 1) + k) * N + n) * C + c] = acc;
        }
    }
}

// out[i] = part[0][i] + part[1][i] + .. in index order
__global__ __launch_bounds__(SE_T) void se_fold_kernel(const float* __restrict__ part, float* __restrict__ out, long len,
                                                       int S) {
    for (long i = (long)blockIdx.x * SE_T + threadIdx.x; i < len; i += (long)gridDim.x * SE_T) {
        float acc = part[i];
        for (int s = 1; s < S; ++s) acc += part[(long)s * len + i];
        out[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The gate of 16 samples per block on v_mfma_f32_16x16x32_bf16, samples as the MFMA's columns. The weights are the
// arena's bf16 shadows; z and h enter as three bf16 terms each (hi + mid + lo = the fp32 value: every product is exact
// in the fp32 accumulator), because one rounding of z or h to bf16 moves s by ~1e-3 and with it the sign of
// s u + idt at ~1e-4 of the elements: ReLU masks (of the output, of h) that differ from the fp32 gate's.
// GEMM 1, h^T [R][16] = W1 [R][C] z^T: the k range (channels) is dealt to the four waves in steps of 32; a lane forms
// its 8 k-values of z from X1 in registers (and stores them as fp32 z), the W1 fragments come straight from the bf16
// shadow, rows past R are zero registers. The four waves' partial tiles are added in wave order through LDS, bias and
// ReLU follow, and h stays in LDS as its bf16 terms (k padded with zeros to a multiple of 32) for
// GEMM 2, s^T [C][16] = W2 [C][R] h^T: the 16-channel tiles are dealt to the waves; a lane ends with 4 consecutive
// channels of one sample: bias, sigmoid, one 16-byte store.
__global__ __launch_bounds__(SE_T) void se_excite_fwd_kernel(const float* __restrict__ X1, const float* __restrict__ ss,
                                                             const bf16_t* __restrict__ W1, const float* __restrict__ b1,
                                                             const bf16_t* __restrict__ W2, const float* __restrict__ b2,
                                                             float* __restrict__ z, float* __restrict__ h,
                                                             float* __restrict__ s, int N, int C, int R, float inv_hw) {
    __shared__ float hp[4][SE_RMAX][SE_NT + 1];
    __shared__ __attribute__((aligned(16))) bf16_t hs[3][SE_NT][SE_RMAX + 8];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * SE_NT, n = n0 + col;
    const bool nok = n < N;
    const int RT = (R + 15) >> 4;
    f32x4 acc[SE_RMAX / 16];
#pragma unroll
    for (int i = 0; i < SE_RMAX / 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = w * 32; k0 < C; k0 += 128) {
        const int c = k0 + kq * 8;
        f8 zv{};
        if (nok) {
            const f8 x = ld8(X1 + (size_t)n * C + c);
            if (ss != nullptr) {
                const f8 sc = ld8(ss + c), sh = ld8(ss + C + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) zv.v[j] = fmaf(x.v[j] * inv_hw, sc.v[j], sh.v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) zv.v[j] = x.v[j] * inv_hw;
            }
            st8(z + (size_t)n * C + c, zv);
        }
        bf16x8 fb[3];
        split8(zv, fb);
#pragma unroll
        for (int rt = 0; rt < SE_RMAX / 16; ++rt) {
            if (rt < RT) {
                const int r = rt * 16 + col;
                u32x4 wv{0u, 0u, 0u, 0u};
                if (r < R) wv = ld16(W1 + (size_t)r * C + c);
                const bf16x8 fw = __builtin_bit_cast(bf16x8, wv);
#pragma unroll
                for (int p = 2; p >= 0; --p)  // (small terms first)
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fb[p], acc[rt], 0, 0, 0);
            }
        }
    }
    // acc[rt][i]: row r = 16 rt + 4 kq + i of h^T, sample col
#pragma unroll
    for (int rt = 0; rt < SE_RMAX / 16; ++rt)
        if (rt < RT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hp[w][rt * 16 + kq * 4 + i][col] = acc[rt][i];
        }
    __syncthreads();
    const int KP = (R + 31) & ~31;  // GEMM 2's k range
    for (int e = t; e < KP * SE_NT; e += SE_T) {
        const int r = e >> 4, nn = e & 15;
        float v = 0.f;
        if (r < R) {
            v = fmaxf(((hp[0][r][nn] + hp[1][r][nn]) + hp[2][r][nn]) + hp[3][r][nn] + b1[r], 0.f);
            if (n0 + nn < N) h[(size_t)(n0 + nn) * R + r] = v;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) hs[p][nn][r] = split_bf(v);
    }
    __syncthreads();
    const int KS = KP >> 5;
    bf16x8 fh[SE_RMAX / 32][3];
#pragma unroll
    for (int ks = 0; ks < SE_RMAX / 32; ++ks)
#pragma unroll
        for (int p = 0; p < 3; ++p)
            fh[ks][p] = __builtin_bit_cast(
                bf16x8, ks < KS ? *reinterpret_cast<const u32x4*>(&hs[p][col][ks * 32 + kq * 8]) : u32x4{0u, 0u, 0u, 0u});
    for (int ct = w; ct < (C >> 4); ct += 4) {
        const int crow = ct * 16 + col;
        f32x4 a2{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < SE_RMAX / 32; ++ks) {
            if (ks < KS) {
                const int k = ks * 32 + kq * 8;
                u32x4 wv{0u, 0u, 0u, 0u};
                if (k < R) wv = ld16(W2 + (size_t)crow * R + k);
                const bf16x8 fw = __builtin_bit_cast(bf16x8, wv);
#pragma unroll
                for (int p = 2; p >= 0; --p) a2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fh[ks][p], a2, 0, 0, 0);
            }
        }
        if (nok) {
            const int c4 = ct * 16 + kq * 4;
            const f32x4 bias = *reinterpret_cast<const f32x4*>(b2 + c4);
            f32x4 sv;
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = 1.f / (1.f + expf(-(a2[i] + bias[i])));
            *reinterpret_cast<f32x4*>(s + (size_t)n * C + c4) = sv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Streaming passes over one sample per blockIdx.y. The block's stride over the sample's 16-byte chunks is a multiple of
// the chunks per row wherever that divides 256, so a thread's channels rarely change: its per-(n, channel) constants
// are formed once and kept in registers.

// out = relu(s * (sc * a + sh) + idt) as fma(a, s sc, s sh) + idt; ss null: the identity affine (inference, where the
// conv's epilogue has applied the folded BatchNorm)
__global__ __launch_bounds__(SE_T) void se_scale_add_relu_kernel(const bf16_t* __restrict__ a,
                                                                 const bf16_t* __restrict__ idt,
                                                                 const float* __restrict__ ss, const float* __restrict__ s,
                                                                 bf16_t* __restrict__ out, int HW, int C) {
    const int cpr = C >> 3, n = blockIdx.y;
    const long per = (long)HW * cpr;
    const size_t base = (size_t)n * HW * C;
    int last = -1;
    f8 A{}, B{};
    for (long i = (long)blockIdx.x * SE_T + threadIdx.x; i < per; i += (long)gridDim.x * SE_T) {
        const int c8 = (int)(i % cpr);
        if (c8 != last) {
            last = c8;
            const f8 sv = ld8(s + (size_t)n * C + c8 * 8);
            if (ss != nullptr) {
                const f8 sc = ld8(ss + c8 * 8), sh = ld8(ss + C + c8 * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) A.v[j] = sv.v[j] * sc.v[j], B.v[j] = sv.v[j] * sh.v[j];
            } else {
                A = sv;
                B = f8{};
            }
        }
        const size_t o = base + (size_t)i * 8;
        const f8 fa = bf8(ld16(a + o)), fi = bf8(ld16(idt + o));
        f8 y;
#pragma unroll
        for (int j = 0; j < 8; ++j) y.v[j] = fmaxf(fmaf(fa.v[j], A.v[j], B.v[j]) + fi.v[j], 0.f);
        *reinterpret_cast<u32x4*>(out + o) = pack8(y);
    }
}

// dA = sc (du - Sdu / M - xhat Sdux / M), du = s g + dpool, xhat = (a - mean) invstd: per (n, channel)
// dA = g (sc s) + a kx + (sc dpool + k0), kx = -sc invstd Sdux / M, k0 = -sc Sdu / M - kx mean
__global__ __launch_bounds__(SE_T) void se_bn_apply_bwd_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ a,
                                                               const float* __restrict__ s,
                                                               const float* __restrict__ dpool,
                                                               const float* __restrict__ ss,
                                                               const float* __restrict__ save,
                                                               const float* __restrict__ bsum, bf16_t* __restrict__ dA,
                                                               int HW, int C, float inv_m) {
    const int cpr = C >> 3, n = blockIdx.y;
    const long per = (long)HW * cpr;
    const size_t base = (size_t)n * HW * C;
    int last = -1;
    f8 A{}, B{}, K{};
    for (long i = (long)blockIdx.x * SE_T + threadIdx.x; i < per; i += (long)gridDim.x * SE_T) {
        const int c8 = (int)(i % cpr);
        if (c8 != last) {
            last = c8;
            const int c = c8 * 8;
            const f8 sv = ld8(s + (size_t)n * C + c), dp = ld8(dpool + (size_t)n * C + c), sc = ld8(ss + c);
            const f8 mean = ld8(save + c), istd = ld8(save + C + c), sdu = ld8(bsum + c), sdx = ld8(bsum + C + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float kx = -sc.v[j] * istd.v[j] * sdx.v[j] * inv_m;
                const float k0 = -sc.v[j] * sdu.v[j] * inv_m - kx * mean.v[j];
                K.v[j] = kx;
                A.v[j] = sc.v[j] * sv.v[j];
                B.v[j] = fmaf(sc.v[j], dp.v[j], k0);
            }
        }
        const size_t o = base + (size_t)i * 8;
        const f8 fg = bf8(ld16(g + o)), fa = bf8(ld16(a + o));
        f8 y;
#pragma unroll
        for (int j = 0; j < 8; ++j) y.v[j] = fmaf(fg.v[j], A.v[j], fmaf(fa.v[j], K.v[j], B.v[j]));
        *reinterpret_cast<u32x4*>(dA + o) = pack8(y);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The gate's backward for 16 samples per block, fp32 on the VALU (weights from the bf16 shadows).
// Phase 1, per 128-channel chunk: dz2 = (sc G2 + sh G1) s (1 - s) to global and LDS; lane (sample nn, 8 rows rg of R)
// adds dz2[nn][c] W2[c][8 rg ..] over the chunk. dh = (dz2 W2) [h > 0] to global and LDS.
// Phase 2: lane (sample nn, 8 channels) forms dpool = (dh W1) / HW and this sample's terms of the BatchNorm's two
// reductions; the 16 samples (adjacent lanes) are added by a butterfly.
// part [tiles][3 C + R]: this tile's sum du | sum du (x - mean) | sum dz2 (db2) | sum dh (db1).
__global__ __launch_bounds__(SE_T) void se_excite_bwd_tile_kernel(
    const float* __restrict__ G, const float* __restrict__ X1, const float* __restrict__ ss,
    const float* __restrict__ save, const float* __restrict__ s, const float* __restrict__ h,
    const bf16_t* __restrict__ W1, const bf16_t* __restrict__ W2, float* __restrict__ dz2, float* __restrict__ dh,
    float* __restrict__ dpool, float* __restrict__ part, int N, int C, int R, float hw) {
    __shared__ float dzs[SE_NT][129];
    __shared__ float dhs[SE_NT][SE_RMAX + 1];
    const int t = threadIdx.x, nn = t & 15, rg = t >> 4;
    const int n0 = blockIdx.x * SE_NT;
    const float* G1 = G;
    const float* G2 = G + (size_t)N * C;
    float* prt = part + (size_t)blockIdx.x * (3 * C + R);
    f8 acc{};
    for (int c0 = 0; c0 < C; c0 += 128) {
        {
            const int pn = t >> 4, c = c0 + (t & 15) * 8;
            f8 v{};
            if (c < C && n0 + pn < N) {
                const size_t o = (size_t)(n0 + pn) * C + c;
                const f8 g1 = ld8(G1 + o), g2 = ld8(G2 + o), sv = ld8(s + o), sc = ld8(ss + c), sh = ld8(ss + C + c);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    v.v[j] = fmaf(sc.v[j], g2.v[j], sh.v[j] * g1.v[j]) * sv.v[j] * (1.f - sv.v[j]);
                st8(dz2 + o, v);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) dzs[pn][(t & 15) * 8 + j] = v.v[j];
        }
        __syncthreads();
        if (t < 128 && c0 + t < C) {
            float b = dzs[0][t];
#pragma unroll
            for (int q = 1; q < SE_NT; ++q) b += dzs[q][t];
            prt[2 * C + c0 + t] = b;
        }
        if (rg * 8 < R) {
            const int cn = min(128, C - c0);
            for (int cc = 0; cc < cn; ++cc) {
                const float d = dzs[nn][cc];
                const f8 wv = bf8(ld16(W2 + (size_t)(c0 + cc) * R + rg * 8));
#pragma unroll
                for (int j = 0; j < 8; ++j) acc.v[j] = fmaf(d, wv.v[j], acc.v[j]);
            }
        }
        __syncthreads();
    }
    if (rg * 8 < R) {
        const bool ok = n0 + nn < N;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = rg * 8 + j;
            const float hv = ok ? h[(size_t)(n0 + nn) * R + r] : 0.f;
            const float v = hv > 0.f ? acc.v[j] : 0.f;
            dhs[nn][r] = v;
            if (ok) dh[(size_t)(n0 + nn) * R + r] = v;
        }
    }
    __syncthreads();
    if (t < R) {
        float b = dhs[0][t];
#pragma unroll
        for (int q = 1; q < SE_NT; ++q) b += dhs[q][t];
        prt[3 * C + t] = b;
    }
    const float inv_hw = 1.f / hw;
    const bool ok = n0 + nn < N;
    for (int cg = rg; cg < (C >> 3); cg += 16) {
        const int c = cg * 8;
        f8 p{};
        for (int r = 0; r < R; ++r) {
            const float d = dhs[nn][r];
            const f8 wv = bf8(ld16(W1 + (size_t)r * C + c));
#pragma unroll
            for (int j = 0; j < 8; ++j) p.v[j] = fmaf(d, wv.v[j], p.v[j]);
        }
        f8 e1{}, e2{};
        if (ok) {
            const size_t o = (size_t)(n0 + nn) * C + c;
#pragma unroll
            for (int j = 0; j < 8; ++j) p.v[j] *= inv_hw;
            st8(dpool + o, p);
            const f8 g1 = ld8(G1 + o), g2 = ld8(G2 + o), sv = ld8(s + o), x1 = ld8(X1 + o), mean = ld8(save + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                e1.v[j] = fmaf(sv.v[j], g1.v[j], hw * p.v[j]);
                e2.v[j] = fmaf(sv.v[j], g2.v[j] - mean.v[j] * g1.v[j], p.v[j] * (x1.v[j] - hw * mean.v[j]));
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                e1.v[j] += __shfl_xor(e1.v[j], o, 64);
                e2.v[j] += __shfl_xor(e2.v[j], o, 64);
            }
        }
        if (nn == 0) {
            st8(prt + c, e1);
            st8(prt + C + c, e2);
        }
    }
}

// The N-reductions of the two weight gradients, out[c][r] = sum_n P[n][c] Q[n][r] (which 0: dW2 = dz2^T h; which 1:
// dW1^T = z^T dh), as fp32 register tiles: a block owns 64 channels x 64 rows of R and one range of samples, stages 16
// samples of both operands in LDS, each lane keeps 4 x 4 sums. wp [2][NS][C][R]: one partial per sample range.
__global__ __launch_bounds__(SE_T) void se_wgrad_partial_kernel(const float* __restrict__ dz2, const float* __restrict__ h,
                                                                const float* __restrict__ z, const float* __restrict__ dh,
                                                                float* __restrict__ wp, int N, int C, int R, int NS,
                                                                int chunk) {
    __shared__ __attribute__((aligned(16))) float Ps[SE_NT][64];
    __shared__ __attribute__((aligned(16))) float Qs[SE_NT][64];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int which = blockIdx.z / NS, ns = blockIdx.z % NS;
    const float* P = which ? z : dz2;
    const float* Q = which ? dh : h;
    const int cb = blockIdx.x * 64, rb = blockIdx.y * 64;
    const int nb = ns * chunk, ne = min(N, nb + chunk);
    float acc[4][4] = {};
    const int ln = t >> 4, lc = (t & 15) * 4;
    for (int m = nb; m < ne; m += SE_NT) {
        f32x4 pv{0.f, 0.f, 0.f, 0.f}, qv{0.f, 0.f, 0.f, 0.f};
        if (m + ln < ne) {
            if (cb + lc < C) pv = *reinterpret_cast<const f32x4*>(P + (size_t)(m + ln) * C + cb + lc);
            if (rb + lc < R) qv = *reinterpret_cast<const f32x4*>(Q + (size_t)(m + ln) * R + rb + lc);
        }
        *reinterpret_cast<f32x4*>(&Ps[ln][lc]) = pv;
        *reinterpret_cast<f32x4*>(&Qs[ln][lc]) = qv;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SE_NT; ++k) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(&Ps[k][ty * 4]);
            const f32x4 q = *reinterpret_cast<const f32x4*>(&Qs[k][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(p[i], q[j], acc[i][j]);
        }
        __syncthreads();
    }
    const int r = rb + tx * 4;
    if (r < R) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = cb + ty * 4 + i;
            if (c < C)
                *reinterpret_cast<f32x4*>(wp + (((size_t)which * NS + ns) * C + c) * R + r) =
                    f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        }
    }
}

// Folds, in index order, and the += into the gradient arena: dW2 [C][R], dW1 [R][C], then per channel the BatchNorm's
// sums (bsum [2][C] = sum du, sum du xhat for the apply pass; dbeta, dgamma) and db2, then db1.
__global__ __launch_bounds__(SE_T) void se_excite_bwd_fold_kernel(const float* __restrict__ wp,
                                                                  const float* __restrict__ part,
                                                                  const float* __restrict__ save, float* __restrict__ bsum,
                                                                  float* __restrict__ dW1, float* __restrict__ db1,
                                                                  float* __restrict__ dW2, float* __restrict__ db2,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  int C, int R, int NS, int tiles) {
    const long CR = (long)C * R, total = 2 * CR + C + R;
    const int ps = 3 * C + R;
    for (long i = (long)blockIdx.x * SE_T + threadIdx.x; i < total; i += (long)gridDim.x * SE_T) {
        if (i < 2 * CR) {
            const bool one = i >= CR;
            const long e = one ? i - CR : i;  // dW2: e = c R + r; dW1: e = r C + c, its partial at c R + r
            const long src = one ? (e % C) * R + e / C : e;
            const float* p = wp + (one ? (long)NS * CR : 0) + src;
            float acc = p[0];
#pragma unroll 8
            for (int q = 1; q < NS; ++q) acc += p[(long)q * CR];
            float* d = one ? dW1 : dW2;
            d[e] += acc;
        } else if (i < 2 * CR + C) {
            const int c = (int)(i - 2 * CR);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 8
            for (int q = 0; q < tiles; ++q) {
                const float* p = part + (long)q * ps;
                a0 += p[c];
                a1 += p[C + c];
                a2 += p[2 * C + c];
            }
            a1 *= save[C + c];
            bsum[c] = a0;
            bsum[C + c] = a1;
            dbeta[c] += a0;
            dgamma[c] += a1;
            db2[c] += a2;
        } else {
            const int r = (int)(i - 2 * CR - C);
            float a0 = 0.f;
#pragma unroll 8
            for (int q = 0; q < tiles; ++q) a0 += part[(long)q * ps + 3 * C + r];
            db1[r] += a0;
        }
    }
}

// the work split of the pooled-sum passes: chunks per slab, slabs, HW splits and rows per split
struct SePlan {
    int SC, slabs, S, rows;
};
inline SePlan se_plan(int N, int HW, int C) {
    const int cpr = C >> 3;
    int SC = 32;
    while (SC > 1 && (SC >> 1) >= cpr) SC >>= 1;
    const int RB = SE_T / SC, slabs = (cpr + SC - 1) / SC;
    const long blocks = (long)N * slabs;
    long S = (2L * device_cus() + blocks - 1) / blocks;  // HW splits where N x slabs alone cannot fill the CUs
    S = S < 1 ? 1 : S;
    S = S > 32 ? 32 : S;
    const long smax = HW / (4 * RB) > 1 ? HW / (4 * RB) : 1;  // at least one four-row step per lane
    S = S > smax ? smax : S;
    const int rows = (int)((HW + S - 1) / S);
    return SePlan{SC, slabs, (HW + rows - 1) / rows, rows};
}

inline int se_shape_ok(long N, int HW, int C, int R) {
    return N >= 1 && N <= 65535 && HW >= 1 && C >= 32 && C % 32 == 0 && R >= 8 && R % 8 == 0 && R <= SE_RMAX &&
           (long)HW * C < (1L << 31);
}

inline dim3 se_stream_grid(int N, int HW, int C) {
    const long per = (long)HW * (C >> 3);
    long gx = (per + 4 * SE_T - 1) / (4 * SE_T);
    const long cap = 8192 / N > 1 ? 8192 / N : 1;
    gx = gx > cap ? cap : gx;
    return dim3((unsigned)gx, (unsigned)N);
}

}  // namespace

// fp32 words of the partial workspace of imk_se_squeeze (K = 1) / imk_se_bwd_reduce (K = 2); 0: no HW split
IMK_EXPORT long imk_se_reduce_floats(int N, int HW, int C, int K) {
    const SePlan p = se_plan(N, HW, C);
    return p.S > 1 ? (long)p.S * K * N * C : 0;
}

IMK_EXPORT int imk_se_squeeze(const void* a, float* X1, float* part, int N, int HW, int C, void* stream) {
    if (!se_shape_ok(N, HW, C, 8)) return -1;
    const SePlan p = se_plan(N, HW, C);
    hipStream_t st = (hipStream_t)stream;
    se_reduce_kernel<false><<<N * p.slabs * p.S, SE_T, 0, st>>>((const bf16_t*)a, nullptr, nullptr, nullptr,
                                                                 p.S > 1 ? part : X1, N, HW, C, p.SC, p.slabs, p.S,
                                                                 p.rows);
    IMK_CHECK_LAUNCH();
    if (p.S > 1) {
        const long len = (long)N * C;
        se_fold_kernel<<<stream_grid(len), SE_T, 0, st>>>(part, X1, len, p.S);
        IMK_CHECK_LAUNCH();
    }
    return 0;
}

// G [2][N][C] = (G1, G2)
IMK_EXPORT int imk_se_bwd_reduce(const void* dout, const void* out, const void* a, void* g, float* G, float* part,
                                 int N, int HW, int C, void* stream) {
    if (!se_shape_ok(N, HW, C, 8)) return -1;
    const SePlan p = se_plan(N, HW, C);
    hipStream_t st = (hipStream_t)stream;
    se_reduce_kernel<true><<<N * p.slabs * p.S, SE_T, 0, st>>>((const bf16_t*)a, (const bf16_t*)dout,
                                                                (const bf16_t*)out, (bf16_t*)g, p.S > 1 ? part : G, N,
                                                                HW, C, p.SC, p.slabs, p.S, p.rows);
    IMK_CHECK_LAUNCH();
    if (p.S > 1) {
        const long len = 2L * N * C;
        se_fold_kernel<<<stream_grid(len), SE_T, 0, st>>>(part, G, len, p.S);
        IMK_CHECK_LAUNCH();
    }
    return 0;
}

IMK_EXPORT int imk_se_excite_fwd(const float* X1, const float* ss, const void* W1, const float* b1, const void* W2,
                                 const float* b2, float* z, float* h, float* s, int N, int HW, int C, int R,
                                 void* stream) {
    if (!se_shape_ok(N, HW, C, R)) return -1;
    se_excite_fwd_kernel<<<(N + SE_NT - 1) / SE_NT, SE_T, 0, (hipStream_t)stream>>>(
        X1, ss, (const bf16_t*)W1, b1, (const bf16_t*)W2, b2, z, h, s, N, C, R, 1.f / (float)HW);
    IMK_CHECK_LAUNCH();
    return 0;
}

IMK_EXPORT int imk_se_scale_add_relu(const void* a, const void* idt, const float* ss, const float* s, void* out, int N,
                                     int HW, int C, void* stream) {
    if (!se_shape_ok(N, HW, C, 8)) return -1;
    se_scale_add_relu_kernel<<<se_stream_grid(N, HW, C), SE_T, 0, (hipStream_t)stream>>>(
        (const bf16_t*)a, (const bf16_t*)idt, ss, s, (bf16_t*)out, HW, C);
    IMK_CHECK_LAUNCH();
    return 0;
}

// sample ranges of the weight-gradient partials
static inline void se_wgrad_split(int N, int C, int R, int* NS, int* chunk) {
    const long tiles = 2L * ((C + 63) / 64) * ((R + 63) / 64);
    long ns = (2L * device_cus() + tiles - 1) / tiles;
    const long nmax = (N + SE_NT - 1) / SE_NT;
    ns = ns > nmax ? nmax : ns;
    ns = ns > 64 ? 64 : (ns < 1 ? 1 : ns);
    const int ch = (int)(((N + ns - 1) / ns + SE_NT - 1) / SE_NT) * SE_NT;
    *chunk = ch;
    *NS = (N + ch - 1) / ch;
}

// fp32 words of imk_se_excite_bwd's workspace: dz2 [N][C], dh [N][R], tile partials, weight-gradient partials
IMK_EXPORT long imk_se_excite_bwd_floats(int N, int C, int R) {
    int NS, chunk;
    se_wgrad_split(N, C, R, &NS, &chunk);
    const long tiles = (N + SE_NT - 1) / SE_NT;
    return (long)N * C + (long)N * R + tiles * (3L * C + R) + 2L * NS * C * R;
}

// The gate's backward as a fixed sequence of three launches. G [2][N][C]; save [2][C] = (mean, invstd); ss [2][C];
// dpool [N][C] and bsum [2][C] go to the apply pass; the six gradients are added into their arena slots.
IMK_EXPORT int imk_se_excite_bwd(const float* G, const float* X1, const float* ss, const float* save, const float* z,
                                 const float* h, const float* s, const void* W1, const void* W2, float* ws,
                                 float* dpool, float* bsum, float* dW1, float* db1, float* dW2, float* db2,
                                 float* dgamma, float* dbeta, int N, int HW, int C, int R, void* stream) {
    if (!se_shape_ok(N, HW, C, R)) return -1;
    hipStream_t st = (hipStream_t)stream;
    int NS, chunk;
    se_wgrad_split(N, C, R, &NS, &chunk);
    const int tiles = (N + SE_NT - 1) / SE_NT;
    float* dz2 = ws;
    float* dh = dz2 + (size_t)N * C;
    float* part = dh + (size_t)N * R;
    float* wp = part + (size_t)tiles * (3 * C + R);
    se_excite_bwd_tile_kernel<<<tiles, SE_T, 0, st>>>(G, X1, ss, save, s, h, (const bf16_t*)W1, (const bf16_t*)W2, dz2,
                                                      dh, dpool, part, N, C, R, (float)HW);
    IMK_CHECK_LAUNCH();
    se_wgrad_partial_kernel<<<dim3((C + 63) / 64, (R + 63) / 64, 2 * NS), SE_T, 0, st>>>(dz2, h, z, dh, wp, N, C, R, NS,
                                                                                         chunk);
    IMK_CHECK_LAUNCH();
    se_excite_bwd_fold_kernel<<<stream_grid(2L * C * R + C + R), SE_T, 0, st>>>(wp, part, save, bsum, dW1, db1, dW2, db2,
                                                                                dgamma, dbeta, C, R, NS, tiles);
    IMK_CHECK_LAUNCH();
    return 0;
}

IMK_EXPORT int imk_se_bn_apply_bwd(const void* g, const void* a, const float* s, const float* dpool, const float* ss,
                                   const float* save, const float* bsum, void* dA, int N, int HW, int C,
                                   void* stream) {
    if (!se_shape_ok(N, HW, C, 8)) return -1;
    se_bn_apply_bwd_kernel<<<se_stream_grid(N, HW, C), SE_T, 0, (hipStream_t)stream>>>(
        (const bf16_t*)g, (const bf16_t*)a, s, dpool, ss, save, bsum, (bf16_t*)dA, HW, C,
        1.f / ((float)N * (float)HW));
    IMK_CHECK_LAUNCH();
    return 0;
}
