// 2x2 / stride-2 average pool, ceil_mode, count_include_pad=False (the ResNet-D shortcut), NHWC bf16 (gfx950).
// One thread per 16-byte chunk (8 channels) of an OUTPUT pixel, grid-stride over N * OH * OW * C / 8 chunks; the
// window's last row / column of an odd map holds 2 or 1 pixels and divides by that count. Both directions are pure
// streams (profiles/hbm_roof.md): non-temporal 16-byte accesses, 64-bit element offsets, a grid of 256-thread blocks
// capped at STREAM_GRID_CAP. The backward walks the same output chunks, so each dy chunk is loaded once and its
// quotient stored to the up to four pixels of its quad.
// A file of its own beside misc.hip: it is compiled without the packed fp32 VALU forms (build.py FILE_FLAGS).

#include "common.h"

namespace {

template <bool BWD>
__global__ __launch_bounds__(256) void avgpool2_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int N,
                                                       int H, int W, int C, int OH, int OW) {
    const int cc = C >> 3;
    const long total = (long)N * OH * OW * cc;
    for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long)gridDim.x * 256) {
        const int ch = (int)(id % cc);
        long r = id / cc;
        const int ox = (int)(r % OW);
        r /= OW;
        const int oy = (int)(r % OH), n = (int)(r / OH);
        const int nh = min(2, H - 2 * oy), nw = min(2, W - 2 * ox);
        const float inv = 1.f / (float)(nh * nw);
        const size_t big = (((size_t)n * H + 2 * oy) * W + 2 * ox) * C + ch * 8;  // the quad's first pixel in [N,H,W,C]
        const size_t small = (size_t)id * 8;                                       // the chunk in [N,OH,OW,C]
        float acc[8];
        if (BWD) {
            const u32x4 g = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + small));
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[2 * k] = lo_bf(g[k]) * inv, acc[2 * k + 1] = hi_bf(g[k]) * inv;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] = 0.f;
            for (int a = 0; a < nh; ++a)
                for (int b = 0; b < nw; ++b) {
                    const u32x4 v = __builtin_nontemporal_load(
                        reinterpret_cast<const u32x4*>(src + big + ((size_t)a * W + b) * C));
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[2 * k] += lo_bf(v[k]), acc[2 * k + 1] += hi_bf(v[k]);
                }
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] *= inv;
        }
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = pack_bf2(acc[2 * k], acc[2 * k + 1]);
        if (BWD) {
            for (int a = 0; a < nh; ++a)
                for (int b = 0; b < nw; ++b)
                    __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(dst + big + ((size_t)a * W + b) * C));
        } else {
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(dst + small));
        }
    }
}

template <bool BWD>
int avgpool2_go(const void* src, void* dst, int N, int H, int W, int C, void* stream) {
    if (C % 8 || N < 1 || H < 1 || W < 1) return -100;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    hipLaunchKernelGGL(avgpool2_kernel<BWD>, dim3(stream_grid((long)N * OH * OW * (C / 8))), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst, N, H, W, C, OH, OW);
    IMK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// y [N][ceil(H/2)][ceil(W/2)][C] = avgpool2(x [N][H][W][C])
IMK_EXPORT int imk_avgpool2_fwd(const void* x, void* y, int N, int H, int W, int C, void* stream) {
    return avgpool2_go<false>(x, y, N, H, W, C, stream);
}

// dx [N][H][W][C] = dy [N][ceil(H/2)][ceil(W/2)][C] spread over its window, divided by the window's pixel count
IMK_EXPORT int imk_avgpool2_bwd(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
    return avgpool2_go<true>(dy, dx, N, H, W, C, stream);
}
