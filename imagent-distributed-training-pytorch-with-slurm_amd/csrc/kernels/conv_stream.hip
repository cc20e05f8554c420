// Streaming 1x1 convolution for SHORT reductions (K = C in {64, 128, 256}), gfx950.
//
// ResNet bottlenecks spend their 56x56 / 28x28 stages in 1x1 convolutions with
// K = 64 or 128: the expansion conv3 (64 -> 256, 128 -> 512) forward, and the
// dgrad of conv1 (256 -> 64, 512 -> 128: dX[M][256] = dY[M][64] x W) with the
// BN-backward epilogue. These are pure HBM streams (output bytes = 4x input
// bytes) -- the generic tiled kernels (conv_igemm_impl.h) reload the weight
// tile per output tile, keep one 16-KB stage in flight per block and measured
// 2.1 TB/s on them (profiles/r50_b512_v5_*). Same jobs as cuDNN's conv fwd /
// dgrad for those shapes (reference model imagenet.py:312).
//
// Structure (one persistent block = 4 waves per (pixel range, channel slice)):
//  * the block's weight slice [BN][K] lives in LDS for the whole kernel
//    (16-B chunks XOR-swizzled by row -> conflict-free ds_read_b128 A
//    fragments);
//  * each wave walks 16-pixel groups; the pixel operand is the MFMA B
//    fragment, and in NHWC one lane's B fragment (8 consecutive channels of
//    one pixel) is ONE 16-B global load -- no LDS staging at all. D groups
//    are prefetched into registers ahead of use (bytes in flight per CU ~
//    8 waves x D x 2-4 KB);
//  * every global access of the group loop is a raw BUFFER load / store off a wave-uniform base (the group's
//    first row) with per-lane 32-bit offsets; rows past M and groups past the end are out-of-range offsets
//    (loads read zeros, stores are dropped), so the loop has no divergent memory branch. With the former
//    predicated pointer loads the compiler's waitcnt bookkeeping fell back to s_waitcnt vmcnt(0) around them
//    (277 of them in the fused-output kernel), draining the prefetch in every group's epilogue; now the
//    epilogue's own operands (BN-backward x / mask, residual) are issued before the next prefetch and waited
//    for with a counted vmcnt (round 5: <64,256> fused output 870 -> 742 us, <128,128> 508 -> 380 us in-step);
//  * the weight fragments go through a register ring read several MFMAs ahead (sched_group_barrier pins the
//    interleave; left alone the scheduler issued each ds_read right before its MFMA and waited for it);
//  * v_mfma_f32_16x16x32_bf16, weights = A (rows = output channels);
//  * epilogue per group: the 16 x BN bf16 tile goes through a wave-private LDS
//    buffer and comes back as 16-B row chunks, so every global store / read of
//    the epilogue is a coalesced row segment, and each lane always holds the
//    SAME 8 channels -> BatchNorm statistics (forward: sum, sumsq; IG_BNBWD:
//    sum(g*xhat), sum(g) [, sum(g*xhat2)]) accumulate in 16-24 registers over
//    the whole kernel and leave with one lane fold + one atomic per channel
//    and quantity per wave.
// Semantics are those of igemm's plain / IG_ACCUM / IG_BNBWD epilogues.

#include <cstdlib>

#include "conv_epilogue.h"
#include "conv_igemm_impl.h"

namespace {

// MODE 0: plain epilogue (+ optional IG_ACCUM); IG_BNBWD with the ReLU mask
// from the saved output y (1), recomputed from x (2), y + second BN branch x2 (3); 4: the plain epilogue with
// a training block's fused output (IG_RES residual (+ scale), IG_MASKOUT mask bits, IG_Q8OUT e4m3 copy) -- a
// mode of its own so that the registers of those paths never weigh on the plain kernels (eval, forward convs)
// STEM: the 7x7/2 stem as a row-segment gather (C = 4 padded channels, a
// kernel row = 8 taps x 4 channels = 32 K elements, K = KH x 32): one MFMA
// k-step per kernel row, the lane's B fragment = 2 taps x 4 channels = two
// 8-B loads (each predicated on the image border).
// XBN: the pixel operand is relu(x * scale[c] + shift[c]) (a.xbn [2][C]), applied to each B fragment
// in registers right before its MFMAs (8 channels per lane per k-step: 2 KS x 8 constants per lane)
// K2: a second K segment of K2 channels from X2 (same pixels, row pitch K2; the weights' columns [K, K + K2)),
// with IG_BNBWD the Gram-form conv3 dgrad over [g | h2] (bn_gram.hip): `bias` [Nout] is added to the sums
// before the ReLU mask (as the v3 loop's two-segment form)
template <bool STEM, int KT>
constexpr int stream_rp() {  // LDS weight row pitch in 16-B chunks: 16-chunk swizzle groups stay inside the row
    return STEM ? 32 : (KT / 8 <= 16 ? KT / 8 : (KT / 8 + 15) / 16 * 16);
}

// MODE 5 (IG_NEXT1): MODE 4 whose block also computes the NEXT 1x1 conv on the output it stores -- Y2[M][CO2] =
// out[M][BN] x W2^T, the following bottleneck's conv1 -- from the wave-private epilogue tile, with that conv's
// shifted forward statistics (stats2 / shift2): the widest tensor of the block is not read back from HBM. Single
// slice only (BN = Nout: a wave holds every channel of its pixels). W2 [CO2][BN] is a second LDS-resident weight
// image, so two 4-wave blocks no longer fit a CU: NW = 8 waves share both images (one block per CU, the same 8
// waves and 256 VGPRs per wave; stream_nw / stream_co2 below). The second GEMM runs k-steps ascending per
// accumulator on the stored bf16 bits, as conv_stream_kernel<256, 64, 2, 0> does on `out`: Y2 is bit-identical to
// the stand-alone conv
// (the template's parameter list stays as it was: the kernel names are what profiles and tests know them by)
//
// MODES 6 / 7 (IGemmArgs::gt_T): MODE 1 / 3 (mask bits, no x, IG_ACCUM) whose block also accumulates the PREVIOUS
// Gram-form bottleneck's T [Nout][P] += g^T h2 (bn_gram.hip) from the tiles of g it has just stored: g is written,
// final, by this kernel alone, and a separate pass read all of it back a few microseconds later. The stored bits of
// a group go into a second wave-private LDS tile (sG, 256-B rows in the image (b) of cdna_hip_programming.md T10,
// conv_wgrad_v3.h's wg3_swz) next to the group's 16 rows of h2 (sH, buffer-loaded beside the epilogue operands with
// the same out-of-range scheme: rows past M and groups past the end are zeros). Pixels are the MFMA k index of both
// operands, so both are read with the transposing LDS read. A wave-private [128][64] fp32 accumulator does not fit
// (128 registers); instead NW = 8 waves (one block per CU, as MODE 5) each own 128 / 8 = 16 channels x P of the
// slice's T rows (16 registers) and every wave consumes all eight tiles once per round: 128 pixels = 4 k-steps x 4
// fragments = 16 MFMAs per wave and round, as many as the conv itself at K = 64. Two block barriers per round (tiles
// written -> read; read -> next round's writes, which sits after the next group's MFMAs), so every wave of a block
// runs the same number of rounds (groups past the end are all out of range). T leaves once, one atomic per element
// and block. dX, the mask handling and the slab sums are those of modes 1 / 3 bit for bit
constexpr int stream_nw(int mode) { return mode >= 5 ? 8 : 4; }    // waves per block
constexpr int stream_co2(int mode) { return mode == 5 ? 64 : 0; }  // the next conv's output channels
constexpr int stream_gtp(int mode) { return mode >= 6 ? 64 : 0; }  // P of the T modes (the previous block's width)
// h2 tile [16][64] bf16, 128-B rows: 32-B slot s of row r at s ^ gsw(r). A 32-lane half of a transposing read takes
// rows {0..3, 8..11} or {4..7, 12..15} of one 32-B column window: the four rows of either parity then fall into four
// different windows, the two parities into the two halves of the 256-B bank line -- conflict-free
__device__ __forceinline__ int gt_hswz(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 1); }
__device__ __forceinline__ int gt_gswz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }  // image (b), 16-B chunks

// accumulator fragments -> the wave-private swizzled tile (rows of `pitch` bytes): pixel fr, channels i * 16 + 4 fq
// .. + 3 per lane. DS instructions of one wave execute in order: the row-chunk re-reads (epi_read) see these writes,
// and the previous group's reads are complete (their results were consumed) before these writes land.
template <int FN>
__device__ __forceinline__ void frags_to_tile(char* sE, int pitch, int fr, int fq, const f32x4 (&acc)[FN]) {
#pragma unroll
    for (int i = 0; i < FN; ++i)
        *reinterpret_cast<u32x2*>(sE + fr * pitch + epi_swz(fr, (i * 16 + fq * 4) * 2)) =
            u32x2{pack_bf2(acc[i][0], acc[i][1]), pack_bf2(acc[i][2], acc[i][3])};
    __builtin_amdgcn_wave_barrier();
}

// MODE 5's next-conv stage of one group: Y2 rows = (the 16 x BN tile of stored bits in sE) x W2^T. B fragment of k-step
// ks = chunk ks * 4 + fq of pixel row fr; the second output goes through the same wave-private tile (every fragment
// read is complete by then: the accumulators depend on them) as 16 x CO2 bf16, rows of CO2 * 2 bytes, and leaves as
// coalesced 16-B row chunks with its shifted forward statistics (shift2 / s1 / s2 of the lane's chunk lane % (CO2 / 8))
template <int BN, int CO2>
__device__ __forceinline__ void next_conv_stage(const IGemmArgs& a, char* sE, const char* sW2, const int (&aoff2)[4],
                                                int g, int ngroups, int lane, const float (&shift2)[8],
                                                float (&s1)[8], float (&s2)[8]) {
    constexpr int EP = BN * 2, RB2 = BN * 2, FN2 = CO2 / 16, EP2 = CO2 * 2, CH2 = CO2 / 8, PPR2 = 64 / CH2;
    const int fr = lane & 15, fq = lane >> 4;
    bf16x8 fb2[BN / 32];
#pragma unroll
    for (int ks = 0; ks < BN / 32; ++ks) fb2[ks] = __builtin_bit_cast(bf16x8, epi_read(sE, fr, EP, ks * 4 + fq));
    f32x4 acc2[FN2];
#pragma unroll
    for (int i = 0; i < FN2; ++i) acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // MFMA t = (k-step t / FN2, channel fragment t % FN2); W2 fragments through a ring of RR2 registers read RR2 - 1
    // MFMAs ahead, as the main GEMM's (see there for the group barriers)
    constexpr int NT2 = (BN / 32) * FN2, RR2 = 8;
    auto w2frag = [&](int t) {
        return *reinterpret_cast<const bf16x8*>(sW2 + (t % FN2) * 16 * RB2 + aoff2[(t / FN2) & 3] +
                                                ((t / FN2) >> 2) * 256);
    };
    bf16x8 fa2[RR2];
#pragma unroll
    for (int t = 0; t < RR2 - 1; ++t) fa2[t] = w2frag(t);
    __builtin_amdgcn_sched_group_barrier(0x100, RR2 - 1, 0);
#pragma unroll
    for (int t = 0; t < NT2; ++t) {
        if (t + RR2 - 1 < NT2) {
            fa2[(t + RR2 - 1) % RR2] = w2frag(t + RR2 - 1);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        acc2[t % FN2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa2[t % RR2], fb2[t / FN2], acc2[t % FN2], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
    }
    frags_to_tile<FN2>(sE, EP2, fr, fq, acc2);
    const __amdgpu_buffer_rsrc_t ry2 = buf_rsrc(a.Y2 + (size_t)(g < ngroups ? g * 16 : 0) * CO2, true);
#pragma unroll
    for (int q = 0; q < 16 / PPR2; ++q) {
        const int p = q * PPR2 + lane / CH2, c2 = lane % CH2;
        const bool ev2 = g < ngroups && g * 16 + p < a.M;
        const u32x4 t = epi_read(sE, p, EP2, c2);
        __builtin_amdgcn_raw_buffer_store_b128(t, ry2, ev2 ? (uint32_t)(p * CO2 + c2 * 8) * 2 : BUF_OOB, 0, 0);
        if (a.stats2) stat_fwd(t, ev2 ? 1.f : 0.f, shift2, s1, s2);  // shifted sums, as the plain epilogue's
    }
    __builtin_amdgcn_wave_barrier();
}

template <int K, int BN, int D, int MODE, bool STEM = false, bool XBN = false, int K2 = 0>
__global__ __launch_bounds__(stream_nw(MODE) * 64, 2) void conv_stream_kernel(const IGemmArgs a) {
    constexpr int NW = stream_nw(MODE), CO2 = stream_co2(MODE);
    constexpr int KS1 = K / 32;       // k-steps from X
    constexpr int KS = (K + K2) / 32; // MFMA k-steps per group
    constexpr int FN = BN / 16;       // channel fragments
    constexpr int CPR = (K + K2) / 8; // 16-B chunks per weight row
    constexpr int RP = stream_rp<STEM, K + K2>();   // LDS weight row pitch, chunks
    constexpr int RB = RP * 16;                     // ... bytes
    constexpr int SWM = (RP < 16 ? RP : 16) - 1;    // chunk swizzle mask: conflict-free A reads
    constexpr int EP = BN * 2;        // epilogue LDS row pitch (bytes), rows swizzled as the staged epilogue (epi_swz)
    constexpr int CH = BN / 8;        // 16-B output chunks per pixel
    constexpr int PPR = 64 / CH;      // pixels per epilogue read instruction
    constexpr int NR = 16 / PPR;      // epilogue reads per 16-pixel group
    constexpr bool GT = MODE == 6 || MODE == 7;         // + T = g^T h2 (above)
    constexpr int EM = MODE == 6 ? 1 : MODE == 7 ? 3 : MODE;  // the epilogue's mode
    constexpr int P = stream_gtp(MODE);
    constexpr bool bnb = EM >= 1 && EM <= 3, has_y = EM == 1 || EM == 3, has_x2 = EM == 3;
    constexpr bool FO = MODE == 4 || MODE == 5, NX = MODE == 5;
    static_assert(!GT || (BN == 128 && P == 64 && K2 == 0 && !STEM && !XBN), "T modes: 128-channel slices, p = 64");
    constexpr int RB2 = BN * 2;        // W2 row pitch in LDS (bytes): BN / 8 chunks, swizzled in groups of 16
    constexpr int CH2 = NX ? CO2 / 8 : 1;  // 16-B chunks per pixel of the second output
    static_assert(!NX || (K2 == 0 && !STEM && !XBN && BN == 256 && (CO2 == 64 || CO2 == 128)), "next-conv mode");
    static_assert(NX || CO2 == 0, "CO2: next-conv mode only");
    // chunks whose global reads are batched; with the BN-backward epilogue all
    // of a group's reads (x, y | x2, old) are issued before its MFMAs
    constexpr int QB = bnb ? NR : (NR < 4 ? NR : 4);
    static_assert(!bnb || NR <= 4, "BN-backward epilogue: slices of <= 128 channels");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* sW = smem;
    char* sW2 = smem + BN * RB;  // (NX) the next conv's weights [CO2][BN]
    char* sE = smem + BN * RB + CO2 * RB2 + wid * 16 * EP;
    // (GT) every wave's stored tile of g [16][BN] and its rows of h2 [16][P], read by all waves of the block
    char* sG = smem + BN * RB + CO2 * RB2 + NW * 16 * EP;
    char* sH = sG + NW * 16 * EP;

    const int nsl = a.Nout / BN;
    const int G = gridDim.x;  // multiple of nsl (host)
    const int lid = xcd_remap(blockIdx.x, G);
    const int slice = lid % nsl, pb = lid / nsl, npb = G / nsl;
    const int n0 = slice * BN;
    const bool accum = a.flags & IG_ACCUM;

    // weight slice -> LDS: chunk c of row r at slot c ^ (r & SWM)
    for (int idx = tid; idx < BN * CPR; idx += NW * 64) {
        const int r = idx / CPR, c = idx % CPR;
        const u32x4 v = *reinterpret_cast<const u32x4*>(a.Wk + (size_t)(n0 + r) * a.ldb + c * 8);
        *reinterpret_cast<u32x4*>(sW + r * RB + ((c ^ (r & SWM)) * 16)) = v;
    }
    if constexpr (NX) {
        for (int idx = tid; idx < CO2 * (BN / 8); idx += NW * 64) {
            const int r = idx / (BN / 8), c = idx % (BN / 8);
            const u32x4 v = *reinterpret_cast<const u32x4*>(a.W2 + (size_t)r * a.ldb2 + c * 8);
            *reinterpret_cast<u32x4*>(sW2 + r * RB2 + ((c ^ (r & 15)) * 16)) = v;
        }
    }

    // fixed epilogue channel chunk of this lane + the BN constants it needs. (This kernel's main epilogue -- constants,
    // chunk arithmetic, final fold -- stays written out: each of the three, moved onto shared helpers, put a
    // 255 / 256-VGPR instantiation into scratch, profiles/conv_epilogue_refactor.md)
    const int cc = lane % CH;
    const int n = n0 + cc * 8;
    float mean[8], rstd[8], sc[8], sh[8], m2[8], r2[8];
    if (bnb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 mu = *reinterpret_cast<const f32x4*>(a.bnsave + n + 4 * h);
            const f32x4 rs = *reinterpret_cast<const f32x4*>(a.bnsave + a.Nout + n + 4 * h);
            f32x4 g = {0.f, 0.f, 0.f, 0.f}, b = g, mu2 = g, rs2 = g;
            if (!has_y) {
                g = *reinterpret_cast<const f32x4*>(a.bngamma + n + 4 * h);
                b = *reinterpret_cast<const f32x4*>(a.bnbeta + n + 4 * h);
            }
            if (has_x2) {
                mu2 = *reinterpret_cast<const f32x4*>(a.bnsave2 + n + 4 * h);
                rs2 = *reinterpret_cast<const f32x4*>(a.bnsave2 + a.Nout + n + 4 * h);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                mean[4 * h + r] = mu[r];
                rstd[4 * h + r] = rs[r];
                sc[4 * h + r] = g[r] * rs[r];
                sh[4 * h + r] = b[r] - mu[r] * sc[4 * h + r];
                m2[4 * h + r] = mu2[r];
                r2[4 * h + r] = rs2[r];
            }
        }
    }
    // plain epilogue: forward statistics (mean[] holds the shift: previous batch mean, or 0) and the eval
    // forward's folded BatchNorm (IG_AFFINE: a.bias = [scale | shift] -> sc / sh) + ReLU after the accumulate
    const bool affine = !bnb && (a.flags & IG_AFFINE), relu = !bnb && (a.flags & IG_RELU);
    // IG_RES: the residual comes from bnx (training: a Gram-form block's bn3 + shortcut + ReLU in conv3's epilogue,
    // ops/block.py), IG_MASKOUT: the ReLU mask of the stored output as bits (the next block's dgrad epilogue)
    // (bnsave2 non-null with IG_RES: a per-channel scale on the residual, a downsample block's shortcut BN whose
    // shift the caller folded into bias[Nout..])
    const bool resid = FO && (a.flags & IG_RES), maskout = FO && relu && (a.flags & IG_MASKOUT);
    const bool resaff = resid && a.bnsave2;
    // IG_Q8OUT: the e4m3 copy of the stored output (delayed-scaled, amax-tracked) for an fp8 consumer
    const bool q8out = FO && (a.flags & IG_Q8OUT);
    const float q8s = q8out ? ldexpf(1.f, -a.y8exp[0]) : 0.f;
    float m8 = 0.f;
    float rsc[8];
    if (!bnb) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            mean[c] = (a.stats && a.shift) ? a.shift[n + c] : 0.f;
            // (NX: the first output has no statistics; mean / s1 / s2 serve the second output's channel chunk)
            if constexpr (NX) mean[c] = (a.stats2 && a.shift2) ? a.shift2[(lane % CH2) * 8 + c] : 0.f;
            sc[c] = affine ? a.bias[n + c] : 1.f;
            sh[c] = affine ? a.bias[a.Nout + n + c] : 0.f;
            rsc[c] = resaff ? a.bnsave2[n + c] : 1.f;
        }
    }
    float s1[8], s2[8], s3[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) s1[c] = s2[c] = s3[c] = 0.f;
    float gbias[K2 > 0 ? 8 : 1];
    if constexpr (K2 > 0) {
#pragma unroll
        for (int c = 0; c < 8; ++c) gbias[c] = a.bias[n + c];
    }

    const int ohw = a.OH * a.OW;
    const bool dense = a.sA == 1 && a.H == a.OH && a.W == a.OW;  // input row == output pixel
    const int ngroups = (a.M + 15) / 16;
    const int wstride = npb * NW;
    const int w0 = pb * NW + wid;
    const int fr = lane & 15, fq = lane >> 4;

    u32x4 pf[D][KS];
    auto fetch = [&](int d, int g) {
        const int m = g * 16 + fr;
        const bool ok = g < ngroups && m < a.M;
        if constexpr (STEM) {
            int img = 0, oh = 0, ow = 0;
            if (ok) {
                img = m / ohw;
                const int rem = m - img * ohw;
                oh = rem / a.OW;
                ow = rem - oh * a.OW;
            }
            const int kw0 = 2 * fq;
            const int iw = ow * a.sA + a.dw0 + kw0;
            const bool lo_w = ok && kw0 < a.ntw && (unsigned)iw < (unsigned)a.W;
            const bool hi_w = ok && kw0 + 1 < a.ntw && (unsigned)(iw + 1) < (unsigned)a.W;
            const bf16_t* base = a.X + (size_t)img * a.H * a.W * 4;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int ih = oh * a.sA + a.dh0 + ks;
                const bool rok = ks < a.nth && (unsigned)ih < (unsigned)a.H;
                const bf16_t* q = base + ((long)ih * a.W + iw) * 4;
                u32x2 lo = {0u, 0u}, hi = {0u, 0u};
                if (rok && lo_w) lo = *reinterpret_cast<const u32x2*>(q);
                if (rok && hi_w) hi = *reinterpret_cast<const u32x2*>(q + 4);
                pf[d][ks] = u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
            return;
        }
        // branch-free: buffer loads off a wave-uniform base (the group's first input row); rows past M and groups
        // past the end read zeros through an out-of-range offset (no divergent load, so the compiler's vmcnt
        // bookkeeping stays exact and the prefetch stays in flight, see the header)
        const bool gok = g < ngroups;
        const int m0 = gok ? g * 16 : 0;
        size_t row0 = m0;
        if (!dense) {
            const int img = m0 / ohw, rem = m0 - img * ohw;
            const int oh = rem / a.OW, ow = rem - oh * a.OW;
            row0 = ((size_t)img * a.H + oh * a.sA) * a.W + ow * a.sA;
        }
        uint32_t off = BUF_OOB;
        if (ok) {
            size_t row = (size_t)m;
            if (!dense) {
                const int img = m / ohw, rem = m - img * ohw;
                const int oh = rem / a.OW, ow = rem - oh * a.OW;
                row = ((size_t)img * a.H + oh * a.sA) * a.W + ow * a.sA;
            }
            off = (uint32_t)((row - row0) * a.C * 2) + fq * 16;
        }
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(a.X + row0 * a.C, true);
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) pf[d][ks] = buf_ld16(rx, off + ks * 64);
        if constexpr (K2 > 0) {  // (dense rows only: host check)
            const __amdgpu_buffer_rsrc_t rx2 = buf_rsrc(a.X2 + (size_t)m0 * K2, true);
            const uint32_t off2 = ok ? (uint32_t)(fr * K2 * 2 + fq * 16) : BUF_OOB;
#pragma unroll
            for (int ks = KS1; ks < KS; ++ks) pf[d][ks] = buf_ld16(rx2, off2 + (ks - KS1) * 64);
        }
    };
    // epilogue operand addressing of group g
    struct EpiBase {
        __amdgpu_buffer_rsrc_t ry, ro, rbx, rx2o, rym, ry8;
    };
    auto epi_base = [&](int g) {
        const size_t eb0 = (size_t)(g < ngroups ? g * 16 : 0) * a.ldy;
        const bf16_t* ybase = reinterpret_cast<const bf16_t*>(a.Y) + eb0;
        EpiBase e;
        e.ry = buf_rsrc(ybase, true);
        e.ro = buf_rsrc(accum ? ybase : a.bnx + eb0, accum || resid);
        e.rbx = buf_rsrc(a.bnx + eb0, bnb && a.bnx);  // bnx null (mask bits given): x is never read (zeros)
        e.rx2o = buf_rsrc(a.bnx2 + eb0, has_x2);
        e.rym = buf_rsrc(a.bnym + eb0 / 8, has_y || maskout);
        e.ry8 = buf_rsrc(reinterpret_cast<const uint8_t*>(a.Y8) + eb0, q8out);
        return e;
    };
    auto epi_off = [&](int g, int u, bool& ev, uint32_t& o2) {  // row u * PPR + lane / CH of group g, channels n..
        const int pr = u * PPR + lane / CH;
        ev = g < ngroups && g * 16 + pr < a.M;
        o2 = ev ? (uint32_t)(pr * a.ldy + n) * 2 : BUF_OOB;  // bytes from the group's base
    };
    auto oo_off = [&](int g, int u, uint32_t o2) {
        if (accum && (a.flags & IG_ACCUM_SUB2)) {  // dense output grid: only even (oh, ow) accumulate
            const int rem = (g * 16 + u * PPR + lane / CH) % ohw, oh = rem / a.OW;
            if (((oh | (rem - oh * a.OW)) & 1) != 0) return BUF_OOB;
        }
        return o2;
    };
    // EPF: the epilogue's global operands (residual / BN-backward x, mask bits, second-branch x) are prefetched D
    // groups ahead, as the pixel operand is: issued at the start of their own group they left one memory latency
    // exposed per group (<256, 64> fused output at 14x14: 3.5 us per group and wave for 32 MFMAs). Kept where
    // the registers allow (no spill at 256 VGPRs)
    constexpr bool early = bnb || FO;
    constexpr int EPR = FO ? 4 : bnb ? 4 + (has_y ? 1 : 0) + (has_x2 ? 4 : 0) : 0;  // VGPRs per row chunk
    constexpr bool EPF = early && !STEM && !XBN && D * NR * EPR <= (K >= 256 && BN >= 128 ? 16 : 32);
    u32x4 eoo[EPF ? D : 1][NR], exo[EPF ? D : 1][NR], ex2o[EPF ? D : 1][NR];
    uint32_t eyo[EPF ? D : 1][NR];
    auto issue_early = [&](int d, int g) {
        const EpiBase e = epi_base(g);
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            bool ev;
            uint32_t o2;
            epi_off(g, u, ev, o2);
            eoo[d][u] = buf_ld16(e.ro, oo_off(g, u, o2));
            if (bnb) {
                exo[d][u] = buf_ld16(e.rbx, o2);
                if (has_y) eyo[d][u] = __builtin_amdgcn_raw_buffer_load_b8(e.rym, ev ? o2 >> 4 : BUF_OOB, 0, 0);
                if (has_x2) ex2o[d][u] = buf_ld16(e.rx2o, o2);
            }
        }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(d, w0 + d * wstride);
    if constexpr (EPF) {
#pragma unroll
        for (int d = 0; d < D; ++d) issue_early(d, w0 + d * wstride);
    }
    __syncthreads();  // weight slice visible

    int aoff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) aoff[ks] = fr * RB + (((ks * 4 + fq) ^ (fr & SWM)) * 16);
    // W2 A fragments: chunk ks * 4 + fq of row fr at slot (ks * 4 + fq) ^ fr; the swizzle leaves ks / 4 alone, so
    // four offsets (ks % 4) serve the eight k-steps
    int aoff2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) aoff2[j] = fr * RB2 + (((j * 4 + fq) ^ fr) * 16);
    float xsc[XBN ? KS : 1][8], xsh[XBN ? KS : 1][8];  // this lane's channels ks * 32 + fq * 8 + e
    if constexpr (XBN) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            load8(a.xbn, ks * 32 + fq * 8, xsc[ks]);
            load8(a.xbn, a.C + ks * 32 + fq * 8, xsh[ks]);
        }
    }

    // (GT) T accumulators: rows n0 + wid * 16 + fq * 4 + i, columns jf * 16 + fr
    f32x4 tacc[GT ? P / 16 : 1];
#pragma unroll
    for (int jf = 0; jf < (GT ? P / 16 : 1); ++jf) tacc[jf] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ... and the transposing reads' addresses (as conv_wgrad_v3.h): MFMA k-step s covers the tiles of waves 2 s
    // (k 0..3 of each lane) and 2 s + 1 (k 4..7); lane group tg takes rows trow .. of both (a 32-lane half's two
    // blocks 8 rows apart), 8 B at columns 4 tp .. + 3 of this wave's 16 channels / of h2 column fragment jf
    const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int trow = (tg & 1) * 8 + (tg >> 1) * 4 + tq;
    const int goff = trow * EP + (((wid * 2 + (tp >> 1)) ^ gt_gswz(trow)) << 4) + 8 * (tp & 1);
    const int hoff = trow * 2 * P + (gt_hswz(trow) << 5) + 8 * tp;  // fragment jf: ^ (jf << 5), the slot swizzle

    // (GT: the block's waves run the same rounds -- the loop holds block barriers)
    for (int g0 = w0; (GT ? g0 - wid : g0) < ngroups; g0 += D * wstride) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int g = g0 + d * wstride;  // past the end: every access out of range (no divergent exit)
            bf16x8 fb[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                // (XBN: BN apply + ReLU on the operand; rows past M are never stored)
                if constexpr (XBN) fb[ks] = __builtin_bit_cast(bf16x8, xbn_apply(pf[d][ks], xsc[ks], xsh[ks]));
                else fb[ks] = __builtin_bit_cast(bf16x8, pf[d][ks]);
            }
            // the group's epilogue operands: wave-uniform bases at the group's pixel row, per-lane byte offsets
            // (rows past M: out of range, loads read zeros and stores are dropped). Every load of the loop body is
            // unconditional, so the waits stay counted and the prefetch stays in flight
            const EpiBase eb = epi_base(g);
            bool ev[NR];
            uint32_t o2[NR];
            u32x4 oo[NR], xo[NR], x2o[NR];
            uint32_t yo[NR];
#pragma unroll
            for (int u = 0; u < NR; ++u) epi_off(g, u, ev[u], o2[u]);
            auto issue = [&](int u) {  // late / at-group-start form of the epilogue operand loads
                if (early || accum) oo[u] = buf_ld16(eb.ro, oo_off(g, u, o2[u]));
                if (bnb) {
                    // (GT: x is absent by the plan's conditions -- no load of it, and sum(g xhat), which T replaces,
                    // is not formed: row 0 of the slab is left alone)
                    if constexpr (!GT) xo[u] = buf_ld16(eb.rbx, o2[u]);
                    if (has_y) yo[u] = __builtin_amdgcn_raw_buffer_load_b8(eb.rym, ev[u] ? o2[u] >> 4 : BUF_OOB, 0, 0);
                    if (has_x2) x2o[u] = buf_ld16(eb.rx2o, o2[u]);
                }
            };
            if constexpr (EPF) {  // issued D groups ago (below): take them over
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    oo[u] = eoo[d][u];
                    if (bnb) {
                        xo[u] = exo[d][u];
                        if (has_y) yo[u] = eyo[d][u];
                        if (has_x2) x2o[u] = ex2o[d][u];
                    }
                }
            } else if constexpr (early) {
                // the BN-backward (x / mask) and residual reads go out before the MFMAs and BEFORE the next
                // prefetch: waiting for them leaves the prefetch in flight
#pragma unroll
                for (int u = 0; u < NR; ++u) issue(u);
            }
            // (GT) the group's h2 rows, two 16-B chunks per lane (row j * 8 + lane / 8, chunk lane % 8): issued with
            // the epilogue operands, before the next prefetch, unconditional as they are
            u32x4 h2r[GT ? 2 : 1];
            if constexpr (GT) {
                const __amdgpu_buffer_rsrc_t rh = buf_rsrc(a.gt_h2 + (size_t)(g < ngroups ? g * 16 : 0) * P, true);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int hr = j * 8 + (lane >> 3);
                    const bool hv = g < ngroups && g * 16 + hr < a.M;
                    h2r[j] = buf_ld16(rh, hv ? (uint32_t)(hr * P * 2 + (lane & 7) * 16) : BUF_OOB);
                }
            }
            fetch(d, g + D * wstride);
            f32x4 acc[FN];
#pragma unroll
            for (int i = 0; i < FN; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            // (ring loop and tile write of the main GEMM stay written out here: as one helper shared with the second
            // GEMM <128, 128, 2, 4> measured +1.9 % and <256, 128, 2, 4> +1.1 % in-step, profiles/conv_epilogue_refactor.md)
            // weight fragments through a ring of RR registers, read RR - 1 MFMAs ahead of use, MFMA t = (k-step
            // t / FN, channel fragment t % FN) (the group barriers pin the interleave: left to itself the scheduler
            // issued each ds_read right before its MFMA and waited for it, a full LDS latency per MFMA)
            constexpr int NT = KS * FN, RR = NT < 8 ? NT : FN >= 16 && (FO || XBN) ? 3 : (FN >= 16 || EM == 3 ? 4 : 8);
            bf16x8 fa[RR];
#pragma unroll
            for (int t = 0; t < RR - 1; ++t)
                fa[t] = *reinterpret_cast<const bf16x8*>(sW + (t % FN) * 16 * RB + aoff[t / FN]);
            __builtin_amdgcn_sched_group_barrier(0x100, RR - 1, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t + RR - 1 < NT) {
                    const int u = t + RR - 1;
                    fa[u % RR] = *reinterpret_cast<const bf16x8*>(sW + (u % FN) * 16 * RB + aoff[u / FN]);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                acc[t % FN] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t % RR], fb[t / FN], acc[t % FN], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
            }
            // (1) fragments -> wave-private LDS rows (pixel fr, 4 channels per lane).
            // DS instructions of one wave execute in order: the re-reads below see
            // these writes, and the previous group's reads are complete (their
            // results were consumed) before these writes land.
#pragma unroll
            for (int i = 0; i < FN; ++i)
                *reinterpret_cast<u32x2*>(sE + fr * EP + epi_swz(fr, (i * 16 + fq * 4) * 2)) =
                    u32x2{pack_bf2(acc[i][0], acc[i][1]), pack_bf2(acc[i][2], acc[i][3])};
            __builtin_amdgcn_wave_barrier();
            // (GT) every wave has read the previous round's sG / sH tiles: they may be written again
            if constexpr (GT) __syncthreads();
            // (2) coalesced row chunks: pixel q*PPR + lane/CH, channels n .. n+7
#pragma unroll
            for (int q0 = 0; q0 < NR; q0 += QB) {
                if constexpr (!early) {
#pragma unroll
                    for (int u = 0; u < QB; ++u) issue(q0 + u);
                }
#pragma unroll
                for (int u = 0; u < QB; ++u) {
                    const int q = q0 + u;
                    const int p = q * PPR + lane / CH;
                    const u32x4 t = epi_read(sE, p, EP, cc);
                    const float vf = ev[q] ? 1.f : 0.f;  // rows past M: stores dropped, statistics masked
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[2 * k] = lo_bf(t[k]);
                        v[2 * k + 1] = hi_bf(t[k]);
                        if (affine) {
                            v[2 * k] = fmaf(v[2 * k], sc[2 * k], sh[2 * k]);
                            v[2 * k + 1] = fmaf(v[2 * k + 1], sc[2 * k + 1], sh[2 * k + 1]);
                        }
                        if (resaff) {
                            v[2 * k] = fmaf(lo_bf(oo[q][k]), rsc[2 * k], v[2 * k]);
                            v[2 * k + 1] = fmaf(hi_bf(oo[q][k]), rsc[2 * k + 1], v[2 * k + 1]);
                        } else if (accum || resid) {
                            v[2 * k] += lo_bf(oo[q][k]);
                            v[2 * k + 1] += hi_bf(oo[q][k]);
                        }
                        if (relu) {
                            v[2 * k] = fmaxf(v[2 * k], 0.f);
                            v[2 * k + 1] = fmaxf(v[2 * k + 1], 0.f);
                        }
                    }
                    if constexpr (K2 > 0) {
#pragma unroll
                        for (int c = 0; c < 8; ++c) v[c] += gbias[c];
                    }
                    float xv[8];
                    if (bnb) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            xv[2 * k] = GT ? 0.f : lo_bf(xo[q][k]);
                            xv[2 * k + 1] = GT ? 0.f : hi_bf(xo[q][k]);
                        }
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            const bool keep = has_y ? ((yo[q] >> c) & 1u) : (fmaf(xv[c], sc[c], sh[c]) > 0.f);
                            if (!keep) v[c] = 0.f;
                        }
                    }
                    u32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = pack_bf2(v[2 * k], v[2 * k + 1]);
                    __builtin_amdgcn_raw_buffer_store_b128(o, eb.ry, o2[q], 0, 0);
                    if constexpr (NX) epi_write(sE, p, EP, cc, o);  // the stored bits: the next conv's pixel operand
                    if constexpr (GT)  // the stored bits (rows past M: zeros), chunk cc of row p in image (b)
                        *reinterpret_cast<u32x4*>(sG + wid * 16 * EP + p * EP + ((cc ^ gt_gswz(p)) << 4)) =
                            ev[q] ? o : u32x4{0u, 0u, 0u, 0u};
                    if (q8out) {  // quantise the bf16-rounded values the bf16 consumers see
                        float w[8];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            w[2 * k] = lo_bf(o[k]);
                            w[2 * k + 1] = hi_bf(o[k]);
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) m8 = fmaxf(m8, fabsf(w[i]) * vf);
                        __builtin_amdgcn_raw_buffer_store_b64(
                            u32x2{pack4_fp8(w[0] * q8s, w[1] * q8s, w[2] * q8s, w[3] * q8s),
                                  pack4_fp8(w[4] * q8s, w[5] * q8s, w[6] * q8s, w[7] * q8s)},
                            eb.ry8, ev[q] ? o2[q] / 2 : BUF_OOB, 0, 0);
                    }
                    if (maskout) {  // stored bf16 > 0: nonzero, sign clear, not NaN (as bn_fwd's ym)
                        uint32_t b = 0;
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const uint32_t h = (o[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                            b |= (h != 0u && h <= 0x7F80u ? 1u : 0u) << i;
                        }
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)b, eb.rym, ev[q] ? o2[q] / 16 : BUF_OOB, 0, 0);
                    }
                    if (!NX && a.stats) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {  // statistics of the stored (bf16) values
                            v[2 * k] = lo_bf(o[k]) * vf;
                            v[2 * k + 1] = hi_bf(o[k]) * vf;
                        }
                        if (bnb) {
#pragma unroll
                            for (int c = 0; c < 8; ++c) {
                                if constexpr (!GT) s1[c] += v[c] * ((xv[c] - mean[c]) * rstd[c]);
                                s2[c] += v[c];
                            }
                            if (has_x2) {
#pragma unroll
                                for (int c = 0; c < 8; ++c) {
                                    const float x2 = c & 1 ? hi_bf(x2o[q][c >> 1]) : lo_bf(x2o[q][c >> 1]);
                                    s3[c] += v[c] * ((x2 - m2[c]) * r2[c]);
                                }
                            }
                        } else {
#pragma unroll
                            for (int c = 0; c < 8; ++c) {
                                const float d = (v[c] - mean[c]) * vf;
                                s1[c] += d;
                                s2[c] += d * d;
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            if constexpr (NX) {
                // (the epilogue operands' registers are free again: the next group's go out under the second GEMM)
                if constexpr (EPF) issue_early(d, g + D * wstride);
                next_conv_stage<BN, CO2>(a, sE, sW2, aoff2, g, ngroups, lane, mean, s1, s2);
            }
            if constexpr (EPF && !NX) issue_early(d, g + D * wstride);
            if constexpr (GT) {
                static_assert(!GT || !EPF, "T modes: the epilogue operands are issued at the group's start");
                // The T stage of one round. INVARIANT: it holds a block barrier (and another one sits before the tiles
                // are written again), so every wave of the block runs the same number of rounds -- the group loop runs on
                // the block's first group index, and groups past the end are all out of range. (Written out: as a
                // function the three T-mode kernels measured +0.3 .. +1.6 % in-step, profiles/conv_epilogue_refactor.md)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int hr = j * 8 + (lane >> 3);
                    *reinterpret_cast<u32x4*>(sH + wid * 16 * 2 * P + hr * 2 * P +
                                              (((lane & 7) * 16) ^ (gt_hswz(hr) << 5))) = h2r[j];
                }
                __syncthreads();  // the round's NW tiles of g and h2 are complete
                // T rows of this wave += (g tiles)^T (h2 tiles): EXEC is full here (no divergent path in the loop)
#pragma unroll
                for (int s = 0; s < NW / 2; ++s) {
                    const char* gs = sG + 2 * s * 16 * EP;
                    const char* hs = sH + 2 * s * 16 * 2 * P;
                    const bf16x8 fg = tr16_frag(gs, goff, goff + 16 * EP);
#pragma unroll
                    for (int jf = 0; jf < P / 16; ++jf)
                        tacc[jf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            fg, tr16_frag(hs, hoff ^ (jf << 5), (hoff ^ (jf << 5)) + 16 * 2 * P), tacc[jf], 0, 0, 0);
                }
            }
        }
    }
    if constexpr (GT) {  // one atomic per T element and block: the waves own disjoint rows
        float* tp0 = a.gt_T + (size_t)(n0 + wid * 16 + fq * 4) * P + fr;
#pragma unroll
        for (int jf = 0; jf < P / 16; ++jf)
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(tp0 + i * P + jf * 16, tacc[jf][i]);
    }
    if (q8out) {  // one atomic per wave into the 32-slot amax row
        m8 = wave_max(m8);
        if (lane == 0) atomic_max_pos(a.y8amax + (blockIdx.x & 31), m8);
    }
    // fold the lanes that share a channel chunk, one atomic per channel and quantity
    if constexpr (NX) {  // the second output's statistics (the first has none in this mode)
        if (!a.stats2) return;
        float* st2 = stat_slab(a.stats2, 2, CO2) + (lane % CH2) * 8;
        flush_chunk_lanes<CH2>(s1, st2, lane);
        flush_chunk_lanes<CH2>(s2, st2 + CO2, lane);
        return;
    }
    if (!a.stats) return;
    // fold the lanes that share a channel chunk, one atomic per channel and quantity
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int o = CH; o < 64; o <<= 1) {
            s1[c] += __shfl_xor(s1[c], o, 64);
            s2[c] += __shfl_xor(s2[c], o, 64);
            if (has_x2) s3[c] += __shfl_xor(s3[c], o, 64);
        }
    }
    if (lane >= CH) return;
    float* st = stat_slab(a.stats, bnb ? 3 : 2, a.Nout);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if constexpr (!GT) atomicAdd(st + n + c, s1[c]);
        atomicAdd(st + a.Nout + n + c, s2[c]);
        if (has_x2) atomicAdd(st + 2 * a.Nout + n + c, s3[c]);
    }
}

template <int K, int BN, int D, int MODE, bool STEM = false, bool XBN = false, int K2 = 0>
int launch_stream1(const IGemmArgs& a, hipStream_t st) {
    constexpr int NW = stream_nw(MODE), CO2 = stream_co2(MODE);
    constexpr int RP = stream_rp<STEM, K + K2>();
    // weight slice (+ the next conv's [CO2][BN] image) + one 16-pixel epilogue tile per wave
    // (+ with T: the stored tile of g and the h2 rows of every wave)
    constexpr int GP = stream_gtp(MODE);
    const size_t lds = (size_t)BN * RP * 16 + (size_t)CO2 * BN * 2 + NW * 16 * (BN * 2) +
                       (GP ? NW * 16 * (BN * 2 + GP * 2) : 0);
    if (GP && (!a.gt_T || !a.gt_h2 || a.gt_p != GP)) return CONV_RC_UNLISTED;  // (the plan's conditions)
    const auto kern = conv_stream_kernel<K, BN, D, MODE, STEM, XBN, K2>;
    static int resident = 0;
    if (resident == 0) {
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds) != hipSuccess)
            return CONV_RC_LAUNCH;
        resident = resident_blocks(kern, lds, NW * 64);
    }
    const int nsl = a.Nout / BN;
    const int ngroups = (a.M + 15) / 16;
    // enough pixel blocks to fill the chip, but >= D groups per wave
    const int npb = std::max(1, std::min(resident / nsl, (ngroups + NW * D - 1) / (NW * D)));
    hipLaunchKernelGGL(kern, dim3(npb * nsl), dim3(NW * 64), lds, st, a);
    CONV_COUNTED();
    IMK_CHECK_LAUNCH();
    return 0;
}

// The 7x7 / stride-2 stem (C = 4 padded channels -> 64) as a band kernel: a persistent block stages R output rows'
// worth of input rows (2R + 5 rows x the full padded width, 4 channels) in LDS ONCE and builds every B fragment
// from there -- a kernel row's 8 taps x 4 channels of one output pixel are 64 contiguous LDS bytes -- instead of
// gathering two 8-B pieces per tap row per pixel from L1/L2 (each input pixel fed ~12 output pixels: the
// streaming stem ran at 2.0 TB/s, 1.06 ms per call at 1024 img, profiles/r50_b1024_r5_standalone.md). Weights
// (64 x 7 x 32) live in registers (28 A fragments per lane). The next band's rows are loaded into registers
// while the current band computes, then written to the other LDS buffer. Epilogue as the streaming kernel's
// (wave-private swizzled LDS transpose -> coalesced 16-B stores, shifted forward statistics, or the eval
// forward's folded BatchNorm + ReLU).
// Layout: LDS input row pitch SP = 232 pixels x 8 B; input column c at byte (c + 4) * 8 (columns -4 .. -1 and
// W .. W + 3 stay zero: the padding taps and the zero-weight 8th tap read finite zeros).
template <int R>
__global__ __launch_bounds__(256, 2) void stem_band_kernel(const IGemmArgs a, int nbands) {
    constexpr int KH = 7, KS = 7, FN = 4;             // kernel rows (= MFMA k-steps), 64 / 16 channel fragments
    constexpr int PR = 2 * R + KH - 2;                  // staged input rows per band
    constexpr int SP = 232 * 8;                         // LDS row pitch, bytes
    constexpr int BUF = PR * SP;
    constexpr int EP = 64 * 2;                          // epilogue row pitch (64 channels)
    constexpr int W16 = 112;                            // 16-B chunks per input row (224 px x 8 B)
    constexpr int NCH = PR * W16;                       // chunks per band
    constexpr int CPT = (NCH + 255) / 256;              // chunks per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sE = smem + 2 * BUF + (threadIdx.x >> 6) * 16 * EP;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int bpi = (a.OH + R - 1) / R;  // bands per image

    // zero both buffers once (padding columns stay zero: the band loads write columns 0 .. W-1 only)
    for (int e = tid; e < 2 * BUF / 16; e += 256) reinterpret_cast<u32x4*>(smem)[e] = u32x4{0u, 0u, 0u, 0u};
    // weights: A fragment (kernel row ks, channel fragment i) = Wk[i * 16 + fr][ks * 32 + fq * 8 .. + 8]
    bf16x8 wa[KS][FN];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int i = 0; i < FN; ++i)
            wa[ks][i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                                                       a.Wk + (size_t)(i * 16 + fr) * a.ldb + ks * 32 + fq * 8));
    // epilogue constants of this lane's fixed channel chunk
    const int cc = lane & 7, n = cc * 8;
    const bool affine = a.flags & IG_AFFINE, relu = a.flags & IG_RELU;
    float mean[8], sc[8], sh[8], s1[8], s2[8];
    load8(a.stats && a.shift, a.shift, n, mean);
    load8(affine, a.bias, n, sc, 1.f);
    load8(affine, a.bias, a.Nout + n, sh);
#pragma unroll
    for (int c = 0; c < 8; ++c) s1[c] = s2[c] = 0.f;

    u32x4 stage[CPT];
    auto load_band = [&](int band) {  // global -> registers
        const int img = band / bpi, oy0 = (band - img * bpi) * R;
        const int iy0 = 2 * oy0 - 3;
#pragma unroll
        for (int t = 0; t < CPT; ++t) {
            const int e = tid + 256 * t;
            const int r = e / W16, c16 = e - r * W16, iy = iy0 + r;
            const bool ok = e < NCH && (unsigned)iy < (unsigned)a.H;
            stage[t] = ok ? *reinterpret_cast<const u32x4*>(a.X + (((size_t)img * a.H + iy) * a.W) * 4 + c16 * 8)
                          : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto store_band = [&](int buf) {  // registers -> LDS (column 0 at byte 32)
#pragma unroll
        for (int t = 0; t < CPT; ++t) {
            const int e = tid + 256 * t;
            if (e < NCH) {
                const int r = e / W16, c16 = e - r * W16;
                *reinterpret_cast<u32x4*>(smem + buf * BUF + r * SP + 32 + c16 * 16) = stage[t];
            }
        }
    };

    int band = blockIdx.x;
    if (band < nbands) load_band(band);
    __syncthreads();  // (the zero fill)
    if (band < nbands) store_band(0);
    __syncthreads();
    int buf = 0;
    for (; band < nbands; band += gridDim.x) {
        const int nxt = band + gridDim.x;
        if (nxt < nbands) load_band(nxt);  // in flight under this band's MFMAs
        const int img = band / bpi, oy0 = (band - img * bpi) * R;
        const char* sb = smem + buf * BUF;
        const int rows = min(R, a.OH - oy0);
        const int ngroups = rows * (a.OW / 16);
        for (int g = wid; g < ngroups; g += 4) {
            const int ry = g / (a.OW / 16), ox0 = (g - ry * (a.OW / 16)) * 16;
            const int ox = ox0 + fr;
            f32x4 acc[FN];
#pragma unroll
            for (int i = 0; i < FN; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                // taps 2fq, 2fq + 1 of kernel row ks: input row 2 (oy0 + ry) + ks - 3 = staged row 2 ry + ks,
                // columns 2 ox - 3 + 2 fq .. + 1 at byte (2 ox + 1 + 2 fq) * 8
                const char* pb = sb + (2 * ry + ks) * SP + (2 * ox + 1 + 2 * fq) * 8;
                const u32x2 lo = *reinterpret_cast<const u32x2*>(pb);
                const u32x2 hi = *reinterpret_cast<const u32x2*>(pb + 8);
                const bf16x8 fb = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
#pragma unroll
                for (int i = 0; i < FN; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks][i], fb, acc[i], 0, 0, 0);
            }
            // (1) fragments -> wave-private LDS rows
            frags_to_tile<FN>(sE, EP, fr, fq, acc);
            // (2) row chunks: pixel q * 8 + lane / 8, channels n .. n + 7
            const long m0 = ((long)img * a.OH + oy0 + ry) * a.OW + ox0;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int p = q * 8 + (lane >> 3);
                const u32x4 t = epi_read(sE, p, EP, cc);
                float v[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[2 * k] = fmaf(lo_bf(t[k]), sc[2 * k], sh[2 * k]);
                    v[2 * k + 1] = fmaf(hi_bf(t[k]), sc[2 * k + 1], sh[2 * k + 1]);
                    if (relu) {
                        v[2 * k] = fmaxf(v[2 * k], 0.f);
                        v[2 * k + 1] = fmaxf(v[2 * k + 1], 0.f);
                    }
                }
                const u32x4 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
                *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(a.Y) + (m0 + p) * a.ldy + n) = o;
                if (a.stats) {  // (a band holds whole rows: every pixel counts)
                    stat_fwd(o, 1.f, mean, s1, s2);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // buffer buf ^ 1 was last read in the previous band, which every wave finished before the barrier below in
        // that iteration; the barrier orders these stores before the next band's reads
        if (nxt < nbands) store_band(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    if (!a.stats) return;
    float* st = stat_slab(a.stats, 2, a.Nout) + n;
    flush_chunk_lanes<8>(s1, st, lane);
    flush_chunk_lanes<8>(s2, st + a.Nout, lane);
}

template <int R>
int launch_stem_band(const IGemmArgs& a, hipStream_t st) {
    // (R = 4 output rows per band, conv_kernel_lists.h: 2048 img 1,205 us; R = 2 1,391, R = 6 1,344 and R = 8 2,258
    // spill -- the 28 weight fragments held in registers leave no room for a taller band's prefetch)
    const size_t lds = 2 * (size_t)(2 * R + 5) * 232 * 8 + 4 * 16 * 64 * 2;
    static int resident = 0;
    if (resident == 0) resident = resident_blocks(stem_band_kernel<R>, lds);
    const int nbands = a.N * ((a.OH + R - 1) / R);
    hipLaunchKernelGGL((stem_band_kernel<R>), dim3(std::min(nbands, resident)), dim3(256), lds, st, a, nbands);
    CONV_COUNTED();
    IMK_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// (which of them a conv runs: conv_plan.h, stream_plan / stem_band_ok)
int conv_launch_stream(const ConvKernel& k, const IGemmArgs& a, hipStream_t st) {
    if (k.fam == CONV_STEM_BAND) {
#define X(...) CONV_LAUNCH_IF(CONV_STEM_BAND, launch_stem_band, __VA_ARGS__)
        CONV_STEM_BAND_KERNELS(X)
#undef X
    } else {
#define X(...) CONV_LAUNCH_IF(CONV_STREAM, launch_stream1, __VA_ARGS__)
        CONV_STREAM_KERNELS(X)
#undef X
    }
    return CONV_RC_UNLISTED;
}
