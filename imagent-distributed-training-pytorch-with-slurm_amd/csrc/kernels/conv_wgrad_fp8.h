// 1-byte weight-gradient main loop for gfx950 (MI355X), the fp8 counterpart of conv_wgrad_v3.h:
//   dW[co][tap*Ci + ci] += 2^(e_dy + e_x) * sum_m dY8[m][co] X8[g(m,tap)][ci]
// dY8: NHWC e5m2 bytes (a BatchNorm-backward pass's copy for the fp8 dgrad), X8: NHWC e4m3 bytes (the fp8 forward's
// copy of the conv's input), e_dy / e_x their device-resident power-of-two exponents (ops/fp8.py ActScales), dW fp32
// in the gradient arena. Ci % 128 == 0 and Co % 128 == 0; anything else is the bf16 loop's.
//
// Shared with wgrad_v3_kernel (conv_wgrad_shared.h, conv_wgrad_plan.h): the per-block work decode with its per-split
// buffer descriptors (32-bit offsets hold for tensors over 2^31 bytes) and XCD-aware block order, the pixel gather of
// one filter tap per 128-channel k tile (out-of-image taps as out-of-range offsets: zeros), the fp32-atomic epilogue
// and the launcher's split-K plan; the same NS-deep ring with counted vmcnt and one s_barrier per stage. What this
// file holds is what differs for 1-byte operands:
//  * LDS image: plain 128-B rows (one pixel x 128 channels), 16-B chunk ch of row r at slot ch ^ ((r >> 1) & 7).
//    A 1-KB DMA instruction fills 8 whole rows; the XOR is applied on the source side (lane -> source chunk).
//  * fragments by the 8-bit transposing LDS read ds_read_b64_tr_b8: a 16-lane group reads a block of 8 rows
//    (pixels = MFMA k) x 16 columns (channels); lane 2q + p supplies the address of row q, columns 8p .. 8p + 7, and
//    lane i receives column i of the 8 rows, row q in byte q (tests/test_wgrad_fp8_gpu.py pins this map on the GPU
//    through imk_probe_ds_read_tr8). Group g takes rows 8g .. 8g + 7 of a 32-row k-step, so ONE read is a lane's 8
//    k-values of a 16x16x32 MFMA, and a 32-lane half reads 16 consecutive rows x 16 B: with the slot XOR above these
//    are 256 distinct bytes over all 64 banks (conflict-free). Both operands use the same rows, so the k order agrees.
//  * MFMA: the fragments are converted to bf16 in registers (exact: one v_cvt_scalef32_pk_bf16_{bf8,fp8} per byte
//    pair) and multiplied on v_mfma_f32_16x16x32_bf16 -- every product is exact in fp32 and the sum is an fp32 sum.
//    v_mfma_f32_16x16x32_bf8_fp8 on the bytes themselves (A = dY e5m2, B = X e4m3; MODE 1) needs no conversion and
//    measured faster, but its sum of 32 products is not an fp32 sum (see MODE below), so it is kept for A/B only. The
//    power-of-two scale is applied to the fp32 accumulators once, before the atomics (exact).
// The accumulator layout is the bf16 one.

#pragma once

#include "conv_wgrad_plan.h"
#include "conv_wgrad_shared.h"

namespace {

typedef int i32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int wg8_swz(int row) { return (row >> 1) & 7; }

// the transposing read as inline assembly: the compiler puts s_waitcnt vmcnt(0) in front of every LDS read that follows
// an LDS-DMA fill in program order (it cannot tell the ring's buffers apart), which drains the prefetched stages; the
// kernel's own counted vmcnt + barrier order the fills against these reads (measured with the builtin read instead,
// same loop: 1.3-1.6 x the time, profiles/fp8_wgrad.md)
__device__ __forceinline__ i32x2 wg8_tr8_asm(uint32_t lds_addr) {
    i32x2 v;
    asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}

// 8 fp8 bytes (one lane's k-values) -> bf16x8, exact (e5m2 / e4m3 values have 3 / 4 significant bits)
template <bool BF8>
__device__ __forceinline__ bf16x8 wg8_to_bf16(i32x2 v) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    // gfx950's v_cvt_scalef32_pk_bf16_{bf8,fp8}: two bytes -> one bf16 pair per instruction (scale 1)
    u32x4 r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        bf16x2 lo, hi;
        if constexpr (BF8) {
            lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(v[h], 1.0f, false);
            hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(v[h], 1.0f, true);
        } else {
            lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[h], 1.0f, false);
            hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v[h], 1.0f, true);
        }
        r[2 * h] = __builtin_bit_cast(uint32_t, lo);
        r[2 * h + 1] = __builtin_bit_cast(uint32_t, hi);
    }
    return __builtin_bit_cast(bf16x8, r);
}

// BR: pixel rows per stage (multiple of 32); NS: ring depth. 2 x 2 waves of 64 x 64 over a 128 x 128 tile.
// MODE 0: fragments converted to bf16 in registers (exact) and multiplied on v_mfma_f32_16x16x32_bf16, whose fp32
// accumulation holds the summation bound of tests/test_wgrad_fp8_gpu.py; 1: v_mfma_f32_16x16x32_bf8_fp8 on the bytes
// (no conversion; its internal sum of 32 products drops low bits of small terms beside large ones -- measured up to
// 2^-11.6 of sum |terms| per MFMA on full-range data, profiles/fp8_wgrad.md; A/B only, never dispatched)
template <int BR, int NS, int MODE>
__global__ __launch_bounds__(256, 2) void wgrad_fp8_kernel(const WgradArgs a, const int* __restrict__ e_dy,
                                                          const int* __restrict__ e_x) {
    constexpr int NW = 4;
    constexpr int SI = BR * 128;           // bytes of one operand per stage
    constexpr int PP = (BR / 8) / NW;      // 1-KB pieces (8 rows) per wave, operand and stage
    static_assert(BR % 32 == 0 && PP >= 1 && PP * NW * 8 == BR, "piece split");
    constexpr int LPS = 2 * PP;            // DMA instructions per wave per stage
    constexpr int NKS = BR / 32;           // MFMA k-steps per stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sD = smem;
    char* sX = smem + NS * SI;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wco = wid & 1, wkc = wid >> 1;
    // (a row's offset in its descriptor: row * ld + chunk * 16)
    const WgradWork w = wgrad_work<128, 128, BR, 1>(a);
    const int mbeg = w.mbeg, mend = w.mend, nst = w.nst;
    if (mbeg >= a.M) return;
    const int ohw = a.OH * a.OW;

    // this lane's DMA slots: piece j = rows 8 j .. 8 j + 7 of the stage; the lane takes row 8 j + (lane >> 3) and
    // source chunk (lane & 7) ^ swz(row)
    uint32_t voffd[PP], rowx[PP], colx[PP];
#pragma unroll
    for (int q = 0; q < PP; ++q) {
        const int r = (wid * PP + q) * 8 + (lane >> 3);
        const uint32_t col = (uint32_t)(((lane & 7) ^ wg8_swz(r)) << 4);
        voffd[q] = (uint32_t)(r * a.Co) + col;
        rowx[q] = (uint32_t)r;
        colx[q] = col;
    }
    const uint32_t dstep = (uint32_t)(BR * a.Co);

    int is = 0;
    auto issue = [&]() {
        if (is >= nst) return;
        const int buf = is % NS;
        char* dD = sD + buf * SI + wid * PP * 1024;
        char* dX = sX + buf * SI + wid * PP * 1024;
        const int mb = mbeg + is * BR;
#pragma unroll
        for (int q = 0; q < PP; ++q) buf_dma16(w.rd, dD + q * 1024, voffd[q] + (uint32_t)is * dstep);
#pragma unroll
        for (int q = 0; q < PP; ++q) {
            const int m = mb + (int)rowx[q];
            uint32_t off = BUF_OOB;
            if (w.dense) {
                if (m < mend) off = (uint32_t)(m - mbeg) * (uint32_t)a.Ci + colx[q];
            } else if (m < mend) {
                const WgradPix px = wgrad_pix((uint32_t)m, (uint32_t)ohw, (uint32_t)a.OW, a.mg_ohw, a.sh_ohw, a.mg_ow,
                                              a.sh_ow, a.stride, w.dh, w.dw);
                if (wgrad_pix_in(px, a.H, a.W))  // (else a padding tap: zeros)
                    off = wgrad_pix_row<uint32_t>(px, (uint32_t)w.img0, a.H, a.W) * (uint32_t)a.Ci + colx[q];
            }
            buf_dma16(w.rx, dX + q * 1024, off);
        }
        ++is;
    };
#pragma unroll
    for (int p = 0; p < NS - 1; ++p) issue();

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // transposed-read addressing: group g = lane >> 4 reads rows 8 g + q (q = (lane >> 1) & 7) of the k-step, columns
    // 16 c + 8 p .. + 7 (p = lane & 1) of chunk c at slot c ^ swz(row); the wave's 64 columns are chunks 4 w .. 4 w + 3
    const int rr = (lane >> 4) * 8 + ((lane >> 1) & 7);
    int offa[4], offb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        offa[i] = rr * 128 + (((wco * 4 + i) ^ wg8_swz(rr)) << 4) + 8 * (lane & 1);
        offb[i] = rr * 128 + (((wkc * 4 + i) ^ wg8_swz(rr)) << 4) + 8 * (lane & 1);
    }

    const uint32_t lds0 = (uint32_t)(size_t)(LDS_PTR(char))smem;
    for (int s = 0; s < nst; ++s) {
        if (is - 1 - s >= NS - 2)
            wait_vm<(NS - 2) * LPS>();
        else
            wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        issue();
        const int buf = s % NS;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            i32x2 rd[4], rx[4];
            const uint32_t ad = lds0 + (uint32_t)(buf * SI + ks * 4096);
#pragma unroll
            for (int i = 0; i < 4; ++i) rd[i] = wg8_tr8_asm(ad + (uint32_t)offa[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) rx[j] = wg8_tr8_asm(ad + (uint32_t)(NS * SI + offb[j]));
            // the eight reads have landed before any conversion / MFMA below takes its operands
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(rd[0]), "+v"(rd[1]), "+v"(rd[2]), "+v"(rd[3]), "+v"(rx[0]), "+v"(rx[1]), "+v"(rx[2]),
                           "+v"(rx[3])
                         :
                         : "memory");
            if constexpr (MODE == 0) {
                bf16x8 fd[4], fx[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fd[i] = wg8_to_bf16<true>(rd[i]);
#pragma unroll
                for (int j = 0; j < 4; ++j) fx[j] = wg8_to_bf16<false>(rx[j]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[i], fx[j], acc[i][j], 0, 0, 0);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(__builtin_bit_cast(long, rd[i]),
                                                                               __builtin_bit_cast(long, rx[j]),
                                                                               acc[i][j], 0, 0, 0);
            }
        }
    }

    wgrad_atomic_tile<true>(a.dW + w.kc0 + wkc * 64, w.co0 + wco * 64, a.KH * a.KW * a.Ci, acc, lane, *e_dy + *e_x);
}

// shapes this kernel covers (host): whole 128-channel tiles of both operands, one image's bytes far below 2^31
bool wgrad_fp8_ok(const WgradArgs& a) {
    if (a.stem || a.xbn) return false;
    if (a.Ci <= 0 || a.Co <= 0 || a.Ci % 128 || a.Co % 128) return false;
    if ((size_t)a.H * a.W * a.Ci * 8 >= (1u << 31) || (size_t)a.OH * a.OW * a.Co * 8 >= (1u << 31)) return false;
    return true;
}

template <int BR, int NS, int MODE>
int launch_wgrad_fp8(WgradArgs a, const int* e_dy, const int* e_x, int splits, hipStream_t st) {
    const int K = a.KH * a.KW * a.Ci;
    const int ntiles = (a.Co / 128) * (K / 128);
    // 512 blocks: one wave of blocks over 256 CUs, two per CU (as launch_wgrad_v3)
    const WgradPlan pl =
        wgrad_plan(a.M, ntiles, BR, 512, splits, (size_t)a.Co, (size_t)a.OH * a.OW, (size_t)a.H * a.W * a.Ci);
    splits = pl.splits;
    a.m_per_split = pl.m_per_split;
    const size_t lds = (size_t)NS * 2 * BR * 128;
    hipLaunchKernelGGL((wgrad_fp8_kernel<BR, NS, MODE>), dim3(ntiles * splits), dim3(256), lds, st, a, e_dy, e_x);
    CONV_COUNTED();
    IMK_CHECK_LAUNCH();
    return 0;
}

// one wave: the byte image img[nbytes] is copied to LDS, lane l reads ds_read_b64_tr_b8 at byte address addr[l]
// (8-byte aligned, addr[l] + 8 <= nbytes <= 4096) and stores its two registers to out[2 l], out[2 l + 1]
__global__ __launch_bounds__(64) void probe_tr8_kernel(const uint8_t* __restrict__ img, int nbytes,
                                                       const int* __restrict__ addr, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char s[4096];
    const int lane = threadIdx.x;
    for (int i = lane; i < 4096; i += 64) s[i] = i < nbytes ? (char)img[i] : (char)0;
    __syncthreads();
    const int ad = addr[lane];  // validated on the host
    const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((LDS_PTR(i32x2))(s + ad));
    out[2 * lane] = (uint32_t)v[0];
    out[2 * lane + 1] = (uint32_t)v[1];
}

}  // namespace
