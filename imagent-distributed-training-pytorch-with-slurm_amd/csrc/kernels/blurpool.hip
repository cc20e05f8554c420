// BlurPool: the anti-aliased downsampling of "Making Convolutional Networks Shift-Invariant Again" (timm's aa_layer):
// a depthwise [1,2,1]^T [1,2,1] / 16 filter at stride 2 over the map with reflect padding 1, NHWC bf16 (gfx950),
// fp32 accumulation. y is ceil(H/2) x ceil(W/2); reflection maps index -1 to 1 and index H to H - 2 (H, W >= 2), the
// latter only on odd maps. The weights are powers of two: every product is exact.
//
// Both directions are column walks. A work item is one 16-byte chunk (8 channels) of one OUTPUT column over a band of
// BAND output rows; the thread walks down the band's input rows and keeps everything it reuses in registers:
//   forward   per input row the horizontal [1,2,1] once (three 16-byte loads, reflection resolved in the column
//             indices before the walk), then out[oy] = (h[2oy-1] + 2 h[2oy] + h[2oy+1]) / 16 with the odd row h[2oy+1]
//             carried into the next output row: 2 row filters per output row instead of 3, 6 loads instead of 9, and a
//             band of BAND output rows reads 2 BAND + 1 input rows (the one shared odd row above it again).
//             With ss (the [2][C] fp32 scale / shift of the BatchNorm in front, ops/bn.py bn_scale_shift) each loaded
//             value becomes relu(sc x + sh) first: BatchNorm + ReLU + pool in one pass from the raw conv output to the
//             quarter-size tensor, the normalised full-resolution tensor is never written or read.
//   backward  the transpose in gather form: the item owns the input column pair (2ox, 2ox+1) and per dy row forms the
//             horizontal transposes of both columns from dy[oy][ox] and dy[oy][ox+1] (two loads), then walks: dx row
//             2oy = 1/2 G(oy), dx row 2oy+1 = 1/4 G(oy) + 1/4 G(oy+1), the reflected taps folded into those weights
//             (row / column 1 takes dy[0] twice; on odd maps row / column H-2 takes the last dy twice). G(oy+1) is
//             carried into the next row pair; every dx pixel is written exactly once: no memset, no atomics.
// Items run chunk-fastest, so a wave's accesses are runs of whole pixels; 64-bit element offsets; a persistent grid of
// 256-thread blocks capped at STREAM_GRID_CAP. The stores are non-temporal (written once, read by a later kernel); the
// loads are not: neighbouring columns share one input column (forward) or one dy pixel (backward) and meet in the
// cache at the same instruction.
// Compiled without the packed fp32 VALU forms (build.py FILE_FLAGS), like avgpool2.hip.

#include "common.h"

namespace {

constexpr int BAND = 4;  // output rows per work item

struct V8 {
    float v[8];
};

__device__ __forceinline__ V8 unpack8(const u32x4 w) {
    V8 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[2 * k] = lo_bf(w[k]), r.v[2 * k + 1] = hi_bf(w[k]);
    return r;
}

__device__ __forceinline__ u32x4 pack8(const V8& a) {
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = pack_bf2(a.v[2 * k], a.v[2 * k + 1]);
    return o;
}

__device__ __forceinline__ u32x4 ld16(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// id -> (chunk, column, band, image) of a [N][bands][OW][C / 8] item space
struct Item {
    int ch, ox, oy0, n;
};
__device__ __forceinline__ Item decode(long id, int cc, int OW, int nb) {
    Item it;
    it.ch = (int)(id % cc);
    long r = id / cc;
    it.ox = (int)(r % OW);
    r /= OW;
    it.oy0 = (int)(r % nb) * BAND;
    it.n = (int)(r / nb);
    return it;
}

template <bool BN>
__global__ __launch_bounds__(256) void blurpool_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ ss,
                                                           bf16_t* __restrict__ y, int N, int H, int W, int C, int OH,
                                                           int OW, int nb) {
    const int cc = C >> 3;
    const long total = (long)N * nb * OW * cc;
    for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
        const Item it = decode(id, cc, OW, nb);
        const int c0 = it.ch * 8;
        float sc[8], sh[8];
        if (BN) {
#pragma unroll
            for (int k = 0; k < 8; k += 4) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ss + c0 + k);
                const f32x4 b = *reinterpret_cast<const f32x4*>(ss + C + c0 + k);
#pragma unroll
                for (int j = 0; j < 4; ++j) sc[k + j] = a[j], sh[k + j] = b[j];
            }
        }
        // the three input columns of this output column: 2ox - 1 (-1 -> 1), 2ox, 2ox + 1 (W -> W - 2)
        const int xc = 2 * it.ox;
        const size_t ol = (size_t)(xc == 0 ? 1 : xc - 1) * C + c0, om = (size_t)xc * C + c0,
                     orr = (size_t)(xc + 1 < W ? xc + 1 : W - 2) * C + c0;
        const bf16_t* img = x + (size_t)it.n * H * W * C;
        // h = [1,2,1] along the row, of the (normalised) pixels
        auto hrow = [&](int r) {
            const bf16_t* p = img + (size_t)r * W * C;
            V8 a = unpack8(ld16(p + ol)), b = unpack8(ld16(p + om)), c = unpack8(ld16(p + orr));
            V8 h;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (BN) {
                    a.v[k] = fmaxf(fmaf(sc[k], a.v[k], sh[k]), 0.f);
                    b.v[k] = fmaxf(fmaf(sc[k], b.v[k], sh[k]), 0.f);
                    c.v[k] = fmaxf(fmaf(sc[k], c.v[k], sh[k]), 0.f);
                }
                h.v[k] = a.v[k] + 2.f * b.v[k] + c.v[k];
            }
            return h;
        };
        const int oy1 = min(OH, it.oy0 + BAND);
        V8 up = hrow(it.oy0 == 0 ? 1 : 2 * it.oy0 - 1);  // row -1 -> 1
        bf16_t* yo = y + (((size_t)it.n * OH + it.oy0) * OW + it.ox) * C + c0;
        for (int oy = it.oy0; oy < oy1; ++oy, yo += (size_t)OW * C) {
            const V8 mid = hrow(2 * oy);
            const V8 dn = hrow(2 * oy + 1 < H ? 2 * oy + 1 : H - 2);  // row H -> H - 2 (odd maps)
            V8 o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o.v[k] = (up.v[k] + 2.f * mid.v[k] + dn.v[k]) * 0.0625f;
            __builtin_nontemporal_store(pack8(o), reinterpret_cast<u32x4*>(yo));
            up = dn;
        }
    }
}

__global__ __launch_bounds__(256) void blurpool_bwd_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
                                                           int N, int H, int W, int C, int OH, int OW, int nb) {
    const int cc = C >> 3;
    const long total = (long)N * nb * OW * cc;
    for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
        const Item it = decode(id, cc, OW, nb);
        const int c0 = it.ch * 8;
        const int xe = 2 * it.ox;             // the even column; the odd one, xe + 1, exists unless W is odd here
        const bool odd = xe + 1 < W, right = it.ox + 1 < OW;
        // the odd column's weights on dy[ox] and dy[ox + 1]: 1/4 each, the reflected tap doubles one of them
        const float wa = it.ox == 0 ? 0.5f : 0.25f;
        const float wb = !right ? 0.f : (((W & 1) && xe + 1 == W - 2) ? 0.5f : 0.25f);
        const bf16_t* g = dy + (size_t)it.n * OH * OW * C + (size_t)it.ox * C + c0;
        // the horizontal transposes of dy row r at the two columns
        auto grow = [&](int r, V8& e, V8& o) {
            const bf16_t* p = g + (size_t)r * OW * C;
            const V8 a = unpack8(ld16(p));
            V8 b;
            if (right) {
                b = unpack8(ld16(p + C));
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) b.v[k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) e.v[k] = 0.5f * a.v[k], o.v[k] = wa * a.v[k] + wb * b.v[k];
        };
        const int oy1 = min(OH, it.oy0 + BAND);
        V8 ce, co, ne, no;
        grow(it.oy0, ce, co);
        bf16_t* px = dx + (((size_t)it.n * H + 2 * it.oy0) * W + xe) * C + c0;
        for (int oy = it.oy0; oy < oy1; ++oy, px += (size_t)2 * W * C) {
            const bool below = oy + 1 < OH;
            if (below) {
                grow(oy + 1, ne, no);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) ne.v[k] = no.v[k] = 0.f;
            }
            V8 t;
#pragma unroll
            for (int k = 0; k < 8; ++k) t.v[k] = 0.5f * ce.v[k];
            __builtin_nontemporal_store(pack8(t), reinterpret_cast<u32x4*>(px));
            if (odd) {
#pragma unroll
                for (int k = 0; k < 8; ++k) t.v[k] = 0.5f * co.v[k];
                __builtin_nontemporal_store(pack8(t), reinterpret_cast<u32x4*>(px + C));
            }
            if (2 * oy + 1 < H) {  // the odd row: 1/4 G(oy) + 1/4 G(oy + 1), a reflected tap doubling one of them
                const float va = oy == 0 ? 0.5f : 0.25f;
                const float vb = !below ? 0.f : (((H & 1) && 2 * oy + 1 == H - 2) ? 0.5f : 0.25f);
                bf16_t* pr = px + (size_t)W * C;
#pragma unroll
                for (int k = 0; k < 8; ++k) t.v[k] = va * ce.v[k] + vb * ne.v[k];
                __builtin_nontemporal_store(pack8(t), reinterpret_cast<u32x4*>(pr));
                if (odd) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) t.v[k] = va * co.v[k] + vb * no.v[k];
                    __builtin_nontemporal_store(pack8(t), reinterpret_cast<u32x4*>(pr + C));
                }
            }
            ce = ne, co = no;
        }
    }
}

inline bool shape_ok(int N, int H, int W, int C) { return C > 0 && C % 8 == 0 && N >= 1 && H >= 2 && W >= 2; }

}  // namespace

// y [N][ceil(H/2)][ceil(W/2)][C] = blurpool(x [N][H][W][C]); with ss ([2][C] fp32 scale, shift) of relu(sc x + sh)
IMK_EXPORT int imk_blurpool_fwd(const void* x, const void* ss, void* y, int N, int H, int W, int C, void* stream) {
    if (!shape_ok(N, H, W, C)) return -100;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, nb = (OH + BAND - 1) / BAND;
    const dim3 grid(stream_grid((long)N * nb * OW * (C / 8)));
    if (ss)
        hipLaunchKernelGGL(blurpool_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                           (const float*)ss, (bf16_t*)y, N, H, W, C, OH, OW, nb);
    else
        hipLaunchKernelGGL(blurpool_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                           (const float*)nullptr, (bf16_t*)y, N, H, W, C, OH, OW, nb);
    IMK_CHECK_LAUNCH();
    return 0;
}

// dx [N][H][W][C] = the transpose of the pool applied to dy [N][ceil(H/2)][ceil(W/2)][C]; all of dx is written
IMK_EXPORT int imk_blurpool_bwd(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
    if (!shape_ok(N, H, W, C)) return -100;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2, nb = (OH + BAND - 1) / BAND;
    hipLaunchKernelGGL(blurpool_bwd_kernel, dim3(stream_grid((long)N * nb * OW * (C / 8))), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)dy, (bf16_t*)dx, N, H, W, C, OH, OW, nb);
    IMK_CHECK_LAUNCH();
    return 0;
}
