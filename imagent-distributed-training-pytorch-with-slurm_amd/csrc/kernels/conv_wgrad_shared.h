// What the weight-gradient kernels of conv_wgrad.hip share: the argument struct, the pixel -> input-row gather, the
// per-block work decode of the LDS-DMA loops (conv_wgrad_v3.h, conv_wgrad_fp8.h) and their accumulator epilogue.
// The helpers take scalars, not the struct, where they run per row: wave-uniform values stay in scalar registers.
#pragma once

#include <cstdlib>

#include "common.h"

// an integer A/B knob of the environment (host: the launchers and the dispatch read each once)
inline long env_int(const char* name, long dflt) {
    const char* e = getenv(name);
    return e ? atol(e) : dflt;
}

struct WgradArgs {
    const bf16_t* dY;  // [M][Co]  (NHWC of the conv output)
    const bf16_t* X;   // NHWC [N][H][W][Ci]
    float* dW;         // [Co][KH*KW*Ci] fp32, accumulated (+=)
    int N, H, W, Ci, Co;
    int OH, OW, M;
    int KH, KW, stride, pad;
    int m_per_split;   // multiple of BR
    uint32_t mg_ohw, sh_ohw, mg_ow, sh_ow;  // magic division by OH*OW and OW
    int stem;          // bit 0: C == 4 row-segment gather, dW is [Co][KH][32]
    // the X operand is relu(X * xbn[c] + xbn[Ci + c]) (BatchNorm apply + ReLU of the conv's input,
    // never materialised: ops/block.py); out-of-image taps stay 0
    const float* xbn;
};

namespace {

__device__ __forceinline__ uint32_t fdiv(uint32_t n, uint32_t mg, uint32_t sh) {
    return (uint32_t)(((uint64_t)__umulhi(n, mg) + n) >> sh);
}

// the input pixel that output pixel m (of N x OH x OW) reads at tap shift (dh, dw) = (kh - pad, kw - pad)
struct WgradPix {
    uint32_t img;
    int ih, iw;  // may lie outside the image
};
__device__ __forceinline__ WgradPix wgrad_pix(uint32_t m, uint32_t ohw, uint32_t ow_, uint32_t mg_ohw, uint32_t sh_ohw,
                                              uint32_t mg_ow, uint32_t sh_ow, int stride, int dh, int dw) {
    const uint32_t img = fdiv(m, mg_ohw, sh_ohw);
    const uint32_t rem = m - img * ohw;
    const uint32_t oh = fdiv(rem, mg_ow, sh_ow);
    const uint32_t ow = rem - oh * ow_;
    return {img, (int)oh * stride + dh, (int)ow * stride + dw};
}
__device__ __forceinline__ bool wgrad_pix_in(const WgradPix& p, int H, int W) {
    return (unsigned)p.ih < (unsigned)H && (unsigned)p.iw < (unsigned)W;
}
// its row of the NHWC input counted from image img0, in T arithmetic (32 bits hold within one split, below). The
// callers keep the in-image branch themselves: folded into a helper it compiled to a different main loop
template <typename T>
__device__ __forceinline__ T wgrad_pix_row(const WgradPix& p, uint32_t img0, int H, int W) {
    return ((T)(p.img - img0) * (T)H + (T)p.ih) * (T)W + (T)p.iw;
}

// One block of an LDS-DMA loop: output tile (co0, kc0) of TCO x TK -- one filter tap (shift dh, dw) x TK input
// channels from ci0 -- summed over pixel rows mbeg .. mend in nst stages of BR. Blocks are dealt so that the tiles of
// one m-range share an XCD (and its L2). rd / rx: descriptors of the EB-byte operands with the column offset (co0 /
// ci0) in the base, based at the split's first row (dY) / first image img0 (X; its first row when `dense`: a 1x1
// stride-1 conv, X rows = dY rows), so 32-bit offsets hold for any tensor size and rows at or past M are out of range.
// The launchers' grid is exactly ntiles x splits with splits = ceil(M / m_per_split) (conv_wgrad_plan.h) and the block
// remap is a bijection, so mbeg < M in every block: the kernels' `mbeg >= a.M` return is a guard that no launch
// reaches, and the byte counts below (which would wrap, then clamp, for such a block) are never used by one.
struct WgradWork {
    int co0, kc0, mbeg, mend, nst, dh, dw, img0;
    bool dense;
    __amdgpu_buffer_rsrc_t rd, rx;
};
template <int TCO, int TK, int BR, int EB>
__device__ __forceinline__ WgradWork wgrad_work(const WgradArgs& a) {
    WgradWork w;
    const int K = a.KH * a.KW * a.Ci;
    const int nco = (a.Co + TCO - 1) / TCO, nkc = (K + TK - 1) / TK;  // (Co / K = 64: one half-used tile, wgrad_v3_ok)
    const int ntiles = nco * nkc;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = lid % ntiles, split = lid / ntiles;
    w.co0 = (tile % nco) * TCO, w.kc0 = (tile / nco) * TK;
    w.mbeg = split * a.m_per_split;
    w.mend = min(a.M, w.mbeg + a.m_per_split);
    w.nst = (w.mend - w.mbeg + BR - 1) / BR;
    const int tap = w.kc0 / a.Ci, ci0 = w.kc0 - tap * a.Ci;
    w.dh = tap / a.KW - a.pad, w.dw = tap % a.KW - a.pad;
    w.dense = a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && a.OH == a.H && a.OW == a.W;
    w.img0 = w.mbeg / (a.OH * a.OW);
    const size_t dro = (size_t)w.mbeg * a.Co + w.co0;
    const size_t xro = (w.dense ? (size_t)w.mbeg * a.Ci : (size_t)w.img0 * a.H * a.W * a.Ci) + ci0;
    w.rd = buf_rsrc_n(reinterpret_cast<const char*>(a.dY) + dro * EB, ((size_t)a.M * a.Co - dro) * EB);
    w.rx = buf_rsrc_n(reinterpret_cast<const char*>(a.X) + xro * EB, ((size_t)a.N * a.H * a.W * a.Ci - xro) * EB);
    return w;
}

// a wave's 64 x 64 accumulator tile into fp32 dW (row pitch ld; the caller adds the tile's first column to the pointer)
// from row row0 with no-return atomics, times 2^e when SCALE: acc[i][j][r] is row row0 + 16 i + 4 (lane >> 4) + r,
// column 16 j + (lane & 15)
template <bool SCALE = false>
__device__ __forceinline__ void wgrad_atomic_tile(float* dW, int row0, int ld, const f32x4 (&acc)[4][4], int lane,
                                                  int e = 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* dst = dW + (size_t)(row0 + i * 16 + (lane >> 4) * 4 + r) * ld + (lane & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(dst + j * 16, SCALE ? ldexpf(acc[i][j][r], e) : acc[i][j][r]);
        }
}

}  // namespace
