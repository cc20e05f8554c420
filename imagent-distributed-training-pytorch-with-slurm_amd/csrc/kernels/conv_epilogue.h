// Row-chunk epilogue blocks of the forward / dgrad conv kernels (gfx950).
//
// In the streaming, stem, halo and staged epilogues a lane holds one 16-byte chunk -- 8 consecutive channels of one
// output pixel, read back from a bf16 LDS tile -- and always the SAME 8 channels, so the per-channel constants and the
// BatchNorm statistics live in registers. The order all of them keep: constants of the chunk -> the chunk as fp32
// through affine -> + residual / old value -> ReLU, or + old value -> + bias -> BN-backward mask -> rounded to bf16
// and stored -> statistics of the STORED bf16 values (rows past M count as zeros) -> one fold over the lanes that
// share a channel chunk and one atomic per channel and quantity into the block's slab slot.
// Here are the steps that more than one kernel shares, on plain float (&)[8] / u32x4 values (what is live at a site
// is what that site names). Which sites keep their own text, and the measurements behind that:
// profiles/conv_epilogue_refactor.md.
#pragma once

#include "common.h"
#include "conv_args.h"

__device__ __forceinline__ void unpack8(const u32x4 w, float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = lo_bf(w[k]);
        v[2 * k + 1] = hi_bf(w[k]);
    }
}

// the operand BatchNorm: relu(x * sc + sh) on a chunk, rounded back to bf16
__device__ __forceinline__ u32x4 xbn_apply(u32x4 w, const float (&sc)[8], const float (&sh)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = pack_bf2(fmaxf(fmaf(lo_bf(w[k]), sc[2 * k], sh[2 * k]), 0.f),
                        fmaxf(fmaf(hi_bf(w[k]), sc[2 * k + 1], sh[2 * k + 1]), 0.f));
    return w;
}

// the 8 per-channel constants p[n .. n + 7] (n % 8 == 0) as two 16-B loads. Base and index stay apart down to the
// load, so the address is scalar base + lane offset
__device__ __forceinline__ void load8(const float* p, int n, float (&v)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + n + 4 * h);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[4 * h + r] = t[r];
    }
}
// ... `on` false: dflt, p is not read
__device__ __forceinline__ void load8(bool on, const float* p, int n, float (&v)[8], float dflt = 0.f) {
    if (on) {
        load8(p, n, v);
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = dflt;
    }
}

// forward statistics of a stored chunk o: s1 += y - shift, s2 += (y - shift)^2; vf = 1 for a stored row, 0 for a row
// past M (its store is dropped)
__device__ __forceinline__ void stat_fwd(const u32x4 o, float vf, const float (&shift)[8], float (&s1)[8],
                                         float (&s2)[8]) {
    float y[8];
    unpack8(o, y);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float d = (y[c] * vf - shift[c]) * vf;
        s1[c] += d;
        s2[c] += d * d;
    }
}

// the block's slot of a statistics slab [STAT_SLOTS][rows][nout]
__device__ __forceinline__ float* stat_slab(float* stats, int rows, int nout) {
    return stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * rows * nout;
}

// where the lanes of a wave with equal lane % CH share a channel chunk: fold them, then one atomic per channel from
// lanes 0 .. CH - 1 to dst, the slab row at the LANE's first channel
template <int CH>
__device__ __forceinline__ void flush_chunk_lanes(float (&s)[8], float* dst, int lane) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int o = CH; o < 64; o <<= 1) s[c] += __shfl_xor(s[c], o, 64);
    }
    if (lane < CH) {
#pragma unroll
        for (int c = 0; c < 8; ++c) atomicAdd(dst + c, s[c]);
    }
}
