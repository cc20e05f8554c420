// Which kernel a forward / data-gradient convolution runs: the one decision function (host, plain C++, no HIP
// include). imk_conv_igemm (conv_igemm.hip) launches what conv_plan() returns; the host runtime exports it as
// imr_conv_plan, so tests/test_conv_plan.py checks it without a GPU against the table recorded from the
// dispatch chain this replaced (tests/data/conv_dispatch_parent.jsonl, profiles/conv_plan_refactor.md).
//
// Tile selection (auto, tile 0):
//  * 64 -> 64 3x3 stride 1: the halo-tiled kernel (conv_halo.hip);
//  * 1x1 with C in {64, 128, 256, 512}: the streaming kernel (conv_stream.hip);
//  * C % 64 == 0 with the staged epilogue (every long-K conv, every fused BN-backward dgrad):
//    the v3 main loop (conv_igemm_v3.h), 256x256 tiles for Nout >= 256 (enough tiles), else 128x128
//    (round-3 A/B at R50 / 1024 img, profiles/r50_b1024_conv_v3.md);
//  * the rest (C % 64 != 0, direct epilogues, Nout <= 64): the LDS-DMA ring / register-staged
//    kernels of conv_igemm_impl.h.
// Explicit tiles (A/B, tests): 1-9 ring / register-staged variants, 17-19 / 27-32 v3 variants, 20-22 the streaming
// kernel's 256 / 128 / 64-channel slices, 23 the streaming row-segment stem (with IG_STEM).
// Measured and removed in round 3 (profiles/r50_b1024_v3_tile_study.md): v3 at 256x128, 128x256, 3-deep,
// and BK-32 4-deep rings, and a ping-pong 256x256 schedule with v3 addressing -- all within 2 % of v3.
// Measured slower and removed in round 3: the phased 256x256 kernel (profiles/
// r50_conv_phased_kernel.md), the ping-pong 256x256 kernel after the 8-phase template (-3.2 %),
// static wave priority for the second half of the waves (neutral).
#pragma once

#include <stddef.h>

#include "conv_args.h"
#include "conv_kernel_lists.h"

// a kernel instantiation: its family and its template arguments in declaration order (bools as 0 / 1, unused 0)
enum ConvFamily { CONV_RS, CONV_DMA, CONV_V3, CONV_DMA_FP8, CONV_V3_FP8, CONV_STREAM, CONV_STEM_BAND, CONV_HALO };
struct ConvKernel {
    int fam, p[10];
};
struct ConvLaunch {
    ConvKernel k;
    int img0, nimg;  // image range of this launch
};
struct ConvPlan {
    int rc, n;
    ConvLaunch part[2];
};

inline bool conv_kernel_is(const ConvKernel& k, int fam, const int (&p)[10]) {
    if (k.fam != fam) return false;
    for (int i = 0; i < 10; ++i)
        if (k.p[i] != p[i]) return false;
    return true;
}

// a family's list entry as a launch: X(...) -> CONV_LAUNCH_IF(family, launcher template, ...) inside a function of
// (const ConvKernel& k, const IGemmArgs& a, hipStream_t st)
#define CONV_LAUNCH_IF(FAM, LAUNCH, ...)                                          \
    {                                                                             \
        const int p_[10] = {__VA_ARGS__};                                         \
        if (conv_kernel_is(k, FAM, p_)) return LAUNCH<__VA_ARGS__>(a, st);        \
    }

// is the kernel one of its family's instantiations (conv_kernel_lists.h)? The launch switches are generated from
// the same lists, so a planned kernel that is not listed fails with CONV_RC_UNLISTED instead of launching
#define CONV_LISTED_(...)                                \
    {                                                    \
        const int p_[10] = {__VA_ARGS__};                \
        if (conv_kernel_is(k, fam_, p_)) return true;    \
    }
inline bool conv_kernel_listed(const ConvKernel& k) {
    int fam_ = CONV_RS;
    CONV_RS_KERNELS(CONV_LISTED_)
    fam_ = CONV_DMA;
    CONV_DMA_KERNELS(CONV_LISTED_)
    fam_ = CONV_V3;
    CONV_V3_KERNELS(CONV_LISTED_)
    fam_ = CONV_DMA_FP8;
    CONV_DMA_FP8_KERNELS(CONV_LISTED_)
    fam_ = CONV_V3_FP8;
    CONV_V3_FP8_KERNELS(CONV_LISTED_)
    fam_ = CONV_STREAM;
    CONV_STREAM_KERNELS(CONV_LISTED_)
    fam_ = CONV_STEM_BAND;
    CONV_STEM_BAND_KERNELS(CONV_LISTED_)
    fam_ = CONV_HALO;
    CONV_HALO_KERNELS(CONV_LISTED_)
    return false;
}
#undef CONV_LISTED_

// ---- return codes (0: launched; > 0: a HIP error from the launch)
constexpr int CONV_RC_LAUNCH = -123;    // a launch-time failure (the streaming kernel's LDS attribute), not a decision
constexpr int CONV_RC_UNLISTED = -124;  // the planned kernel is not in its family's list
inline const char* conv_error_reason(int rc) {
    switch (rc) {
        case 1: return "the operand BatchNorm / two-segment form is off the streaming kernel and no other kernel has it";
        case -100: return "C % 8 != 0: 16-byte chunks must not straddle taps";
        case -101: return "no kernel for this explicit tile";
        case -102: return "IG_STEM needs C == 4, at most 8 taps per row and unit tap steps";
        case -103: return "IG_ACCUM with an fp32 output";
        case -104: return "IG_BNBWD: bf16 output without ReLU, Nout % 8 == 0, ldy == Nout, the BatchNorm's operands, "
                          "a staged epilogue";
        case -105: return "the explicit v3 tile / fp8 path does not cover this shape or epilogue";
        case -106: return "the two-segment (X2) form: not the streaming kernel's shape and not a v3 shape with Nout % 64 == 0";
        case -120: return "the operand BatchNorm (xbn): only the 64 -> 64 3x3 halo kernel and the K = 64 / 128 streaming 1x1";
        case -121: return "IG_RES / IG_MASKOUT / IG_Q8OUT / IG_NEXT1: only the streaming 1x1 kernel has that epilogue";
        case -122: return "IG_NEXT1: only the 64 -> 256 single-slice fused-output form into 64 channels, tile 0";
        case -125: return "gt_T (T = g^T h2 from the dgrad's epilogue): only the accumulating mask-bit BN-backward 1x1 dgrad "
                          "without x on the streaming kernel, K = 64 / 128 into 256 channels, p = 64, tile 0";
        case CONV_RC_LAUNCH: return "setting the kernel's dynamic LDS size failed";
        case CONV_RC_UNLISTED: return "the planned kernel is not instantiated (conv_kernel_lists.h)";
    }
    return "";
}

namespace conv_plan_detail {

constexpr int BK = 64;  // K elements per stage of the bf16 loops (conv_igemm_impl.h)

inline ConvKernel rs(int bm, int bn, int wn, int md, int epi) { return {CONV_RS, {bm, bn, wn, md, epi}}; }
inline ConvKernel dma(int bm, int bn, int wn, int ns, int md, int nw, int epi, int eb = 2, int fb = 0) {
    return {eb == 1 ? CONV_DMA_FP8 : CONV_DMA, {bm, bn, wn, ns, md, nw, epi, eb, fb, 128}};
}
inline ConvKernel v3(int bm, int bn, int wn, int ns, int nw, int rb, int eb = 2, int fb = 0, bool ti = false) {
    return {eb == 1 ? CONV_V3_FP8 : CONV_V3, {bm, bn, wn, ns, nw, rb, eb, fb, ti}};
}
inline ConvKernel stream(int k, int bn, int d, int mode, bool stem = false, bool xbn = false, int k2 = 0) {
    return {CONV_STREAM, {k, bn, d, mode, stem, xbn, k2}};
}
inline ConvKernel halo(int w, int r, int epi) { return {CONV_HALO, {w, r, epi}}; }

inline ConvPlan fail(int rc) { return {rc, 0, {}}; }
inline ConvPlan one(const IGemmArgs& a, const ConvKernel& k) { return {0, 1, {{k, 0, a.N}}}; }
// the first i1 images on `main`, the rest on `tail`
inline ConvPlan two(const IGemmArgs& a, int i1, const ConvKernel& main, const ConvKernel& tail) {
    return {0, 2, {{main, 0, i1}, {tail, i1, a.N - i1}}};
}

// Smallest K (= taps x C) that takes the 256x256 v3 tile (one block per CU); below it the 128x128 tile (two blocks
// per CU) overlaps one block's epilogue with the other's main loop, which is what the epilogue-heavy short-K
// BN-backward dgrads need (A/B at batch 1024: 12,782 img/s with every conv on the big tile, 12,872 at 512)
constexpr int V3_BIG_MIN_K = 512;
// Narrowest output that takes the 256x256 v3 tile: 256 channels (one tile spans the whole output, so every pixel
// row is fetched once; in-step A/B at 2048 img: 16,597 / 16,586 vs 16,469 / 16,488 img/s with 512; isolated
// 256 -> 1024 @14 dgrad 327 vs 365 us, 512 -> 256 @28 fwd 842 vs 895 us)
constexpr int V3_BIG_MIN_N = 256;
// 256x256 tiles of the whole problem at which a one-tile-per-block 256x256 kernel has enough blocks
constexpr long BIG_MIN_TILES = 192;

// Wave-quantisation tail of the one-tile-per-block 256x256 kernels (one block per CU): with T tiles on S CUs the
// last of ceil(T / S) rounds runs T mod S tiles on an otherwise idle chip (R50 at 1024 img: 784 tiles on 256 CUs =
// 3 rounds + 16 tiles for every N = 256 conv at 14x14). When that remainder is at most 30 % of S, a FORWARD conv
// (no fused BN-backward / accumulating epilogue: in backward the weight-gradient side stream already fills the
// idle CUs of the last round) is split at an IMAGE boundary: the first I1 images fill exactly the whole rounds
// with 256x256 tiles, the remaining images run as 128x128 tiles (4x as many blocks, one quarter of the work each)
// right after. Every pixel-indexed operand advances by whole images; the statistics slabs accumulate across both
// launches.
constexpr float TAIL_FRAC = 0.3f;

// images of the main part, or 0 when the conv is not split
inline int tail_split_images(const IGemmArgs& a, int cus) {
    // (re-measured at 2048 img, end of round 5: in-step 16,538 / 16,531 / 16,538 with the split vs 16,491 / 16,487 /
    // 16,495 img/s without, alternating on one box -- kept)
    if (a.N < 2 || (a.flags & (IG_BNBWD | IG_ACCUM))) return 0;
    const long ohw = (long)a.OH * a.OW;
    const long nbn = (a.Nout + 255) / 256;
    const long tiles = ((a.M + 255) / 256) * nbn;
    const long S = cus;
    const long full = tiles / S, rem = tiles - full * S;
    if (full < 1 || rem == 0 || rem > TAIL_FRAC * S) return 0;
    const long mt = full * S / nbn;           // M tiles the whole rounds hold
    const long i1 = mt * 256 / ohw;           // whole images inside them
    return (i1 >= 1 && i1 < a.N) ? (int)i1 : 0;
}

// `big` on the whole conv, or, where the last round of 256x256 tiles would leave most of the chip idle, on the
// images of the whole rounds with `small` on the rest
inline ConvPlan big_or_split(const IGemmArgs& a, int cus, const ConvKernel& big, const ConvKernel& small) {
    const int i1 = tail_split_images(a, cus);
    return i1 > 0 ? two(a, i1, big, small) : one(a, big);
}

// shapes v3 covers: C % 64 == 0 (one tap per stage), taps <= 32, operands < 2^31 bytes, and the staged
// bf16 epilogue (no bias; ReLU only with the eval forward's folded BatchNorm, IG_AFFINE, without statistics)
inline bool v3_ok(const IGemmArgs& a) {
    if (a.C % 64 || a.nth * a.ntw > 32 || a.nth < 1 || a.ntw < 1) return false;
    if (a.flags & (IG_OUT_F32 | IG_STEM | IG_FP8)) return false;
    const bool eval_bn = a.flags & IG_AFFINE;
    if ((a.flags & IG_RELU) && !eval_bn) return false;
    if (eval_bn && (a.stats || (a.flags & IG_BNBWD))) return false;
    const bool bnb_bias = (a.flags & IG_BNBWD) && a.X2;  // the second segment's bias (bn_gram.hip)
    if ((a.bias && !eval_bn && !bnb_bias) || a.xbn || a.Nout % 8 || a.ldy % 8) return false;
    if (a.X2 && (a.C2 % 64 || a.C2 <= 0 || a.nth != 1 || a.ntw != 1 || a.sA != 1 || a.H != a.OH || a.W != a.OW ||
                 a.ldb < a.C + a.C2))
        return false;
    // (X / X2 descriptors are tile-based: any size; one image must stay below 2^31 bytes, the weights too)
    const size_t ib = (size_t)a.H * a.W * a.C * 2 * 4, wb = (size_t)a.Nout * a.ldb * 2;
    return ib < (1ull << 31) && wb < (1ull << 31);
}

// fp8 shapes v3 covers (EB = 1): C % 128 == 0 (one tap per 128-deep stage), the staged bf16 epilogue
// (statistics, fused BN backward, accumulate), no second K segment, scales present
inline bool v3_ok8(const IGemmArgs& a) {
    if (!(a.flags & IG_FP8) || a.C % 128 || a.nth * a.ntw > 32 || a.nth < 1 || a.ntw < 1) return false;
    if (a.flags & (IG_OUT_F32 | IG_STEM | IG_RELU | IG_AFFINE | IG_EPI_DIRECT)) return false;
    if (a.bias || a.xbn || a.X2 || !a.xexp || !a.wexp || a.Nout % 8 || a.ldy % 8) return false;
    const size_t xb = (size_t)a.N * a.H * a.W * a.C, wb = (size_t)a.Nout * a.ldb;
    return xb < (1ull << 31) && wb < (1ull << 31);
}

// ---- the halo-tiled 64 -> 64 3x3 stride-1 kernel (conv_halo.hip), forward and dgrad
inline bool tap_in_halo(int d0, int ds) { return d0 >= -1 && d0 <= 1 && d0 + 2 * ds >= -1 && d0 + 2 * ds <= 1; }

// false: the shape / flags are not the halo kernel's
inline bool halo_plan(const IGemmArgs& a, ConvPlan& p) {
    if (a.flags & (IG_OUT_F32 | IG_STEM | IG_REGSTAGE | IG_FP8 | IG_ACCUM_SUB2)) return false;
    // the eval forward's folded BatchNorm (+ ReLU after the optional accumulate): plain epilogue only
    if ((a.flags & (IG_AFFINE | IG_RELU)) && ((a.flags & IG_BNBWD) || a.stats || a.xbn)) return false;
    if ((a.flags & IG_RELU) && !(a.flags & IG_AFFINE)) return false;
    if ((a.bias && !(a.flags & IG_AFFINE)) || a.C != 64 || a.Nout != 64 || a.ldb < 9 * 64 || a.ldy != 64) return false;
    if (a.nth != 3 || a.ntw != 3 || a.KW != 3 || a.sA != 1 || a.sY != 1 || a.oy != 0 || a.ox != 0) return false;
    if (a.OH != a.H || a.OW != a.W || a.YH != a.H || a.YW != a.W) return false;
    if (!tap_in_halo(a.dh0, a.dhs) || !tap_in_halo(a.dw0, a.dws)) return false;
    if (a.kh0 + 2 * a.khs < 0 || a.kh0 + 2 * a.khs > 2 || a.kh0 < 0 || a.kh0 > 2) return false;
    if (a.kw0 + 2 * a.kws < 0 || a.kw0 + 2 * a.kws > 2 || a.kw0 < 0 || a.kw0 > 2) return false;
    const bool bnb = a.flags & IG_BNBWD;
    if (bnb && a.bnx2 && !a.bnym) return false;  // a second BN branch needs the output's mask bits (c2/c3 hold its constants)
    const int epi = bnb ? (a.bnx2 ? 2 : 1) : 0;  // forward (+ shifted BN statistics), fused BN backward, + second BN branch
    if (a.W == 56 && a.H % 4 == 0) return p = one(a, halo(56, 4, epi)), true;
    if (a.W == 112 && a.H % 2 == 0) return p = one(a, halo(112, 2, epi)), true;
    return false;
}

// ---- the streaming kernels (conv_stream.hip)
// the band stem's shapes: 4-channel 224-wide input, 7x7 / stride 2 / pad 3, 64 channels, 16 | OW, dense bf16 output
inline bool stem_band_ok(const IGemmArgs& a) {
    if (a.flags & (IG_OUT_F32 | IG_FP8 | IG_ACCUM | IG_BNBWD | IG_NOSTREAM | IG_RES | IG_MASKOUT | IG_Q8OUT)) return false;
    if ((a.flags & IG_RELU) && !(a.flags & IG_AFFINE)) return false;
    if ((a.bias && !(a.flags & IG_AFFINE)) || a.xbn || a.X2) return false;
    return a.C == 4 && a.W == 224 && a.nth == 7 && a.ntw == 7 && a.sA == 2 && a.dh0 == -3 && a.dw0 == -3 &&
           a.dhs == 1 && a.dws == 1 && a.Nout == 64 && a.ldb == 7 * 32 && a.ldy == 64 && a.OW % 16 == 0 &&
           2 * (a.OW - 1) - 3 + 8 <= a.W + 3 && a.sY == 1 && a.YH == a.OH && a.YW == a.OW && a.oy == 0 && a.ox == 0;
}

constexpr int IG_FUSED_OUT = IG_RES | IG_MASKOUT | IG_Q8OUT;

// the streaming kernel's MODE: 0 plain epilogue, 4 with a training block's fused output; IG_BNBWD with the ReLU mask
// from the mask bits (1), recomputed from x (2), the bits + the second BN branch (3); -1: no such kernel (a second
// branch without the mask bits)
inline int stream_mode(const IGemmArgs& a) {
    if (!(a.flags & IG_BNBWD)) return (a.flags & IG_FUSED_OUT) ? 4 : 0;
    if (a.bnx2) return a.bnym ? 3 : -1;
    return a.bnym ? 1 : 2;
}

// the <K, BN, D> slice kernel in the mode the arguments ask for; false: that mode does not exist
inline bool stream_slice(const IGemmArgs& a, ConvPlan& p, int k, int bn, int d) {
    const int mode = stream_mode(a);
    return mode >= 0 ? (p = one(a, stream(k, bn, d, mode)), true) : false;
}

// bn: channel-slice width (0 auto: the widest that divides Nout; 64 / 128 / 256 forced, tiles 22 / 21 / 20).
// false: the shape / flags are not the streaming kernel's; true: p holds its kernel, or the error of a form that only
// this kernel has
inline bool stream_plan(const IGemmArgs& a, int bn, ConvPlan& p) {
    const int bn_hint = bn;  // explicit slice width, before the defaults below
    // the eval forward's folded BatchNorm (+ ReLU): plain epilogue, no statistics
    const bool eval_bn = a.flags & IG_AFFINE;
    if ((a.flags & IG_RELU) && !eval_bn) return false;
    if (eval_bn && (a.stats || a.xbn || (a.flags & IG_BNBWD))) return false;
    if ((a.flags & IG_FUSED_OUT) &&
        (!eval_bn || (a.flags & (IG_ACCUM | IG_BNBWD | IG_STEM)) || ((a.flags & IG_RES) && !a.bnx) ||
         ((a.flags & IG_MASKOUT) && (!a.bnym || !(a.flags & IG_RELU))) ||
         ((a.flags & IG_Q8OUT) && (!a.Y8 || !a.y8exp || !a.y8amax))))
        return p = fail(-121), true;
    // IG_NEXT1: the fused-output kernel's single-slice form only (K = 64 into 256 channels on the same pixels, no
    // e4m3 copy), the next conv into 64 channels; anything else is an error, never another kernel
    if (a.flags & IG_NEXT1) {
        // (Co2 = 128, layer 1 into layer 2: a 64-KB W2 image and all 160 KB of a CU's LDS; built and measured, 1.2 ms
        // less stand-alone but in-step within the noise, profiles/ab/next_conv1.txt: not kept)
        if (!(a.flags & (IG_RES | IG_MASKOUT)) ||
            (a.flags & (IG_Q8OUT | IG_OUT_F32 | IG_FP8 | IG_REGSTAGE | IG_NOSTREAM)) || a.stats || a.xbn || a.X2 ||
            a.C != 64 || a.Nout != 256 || (bn != 0 && bn != 256) || !a.W2 || !a.Y2 || a.Co2 != 64 || a.ldb2 < 256 ||
            a.ldb2 % 8 || a.nth != 1 || a.ntw != 1 || a.sA != 1 || a.H != a.OH || a.W != a.OW || a.dh0 != 0 ||
            a.dw0 != 0 || a.kh0 != 0 || a.kw0 != 0 || a.sY != 1 || a.oy != 0 || a.ox != 0 || a.YH != a.OH ||
            a.YW != a.OW || a.ldy != a.Nout || a.ldb < a.C)
            return p = fail(-122), true;
        // D = 1 (2 spills 26 VGPRs); the next group's residual rows are then prefetched too (EPF), issued before
        // the second GEMM
        return p = one(a, stream(64, 256, 1, 5)), true;
    }
    const bool has_bias = a.bias && !eval_bn;
    if (a.X2) {
        // the Gram-form conv3 dgrad of a 64-channel bottleneck (bn_gram.hip): K = [g (256) | h2 (64)] into 64
        // channels with bn2's BN-backward epilogue, weights [64][320] resident in LDS (the 128 x 64 v3 tile
        // re-stages them per tile and ran these HBM streams at ~2.7 TB/s)
        if (!(a.flags & IG_BNBWD) || (a.flags & (IG_ACCUM | IG_FP8 | IG_OUT_F32 | IG_AFFINE | IG_NOSTREAM | IG_RES |
                                                  IG_MASKOUT | IG_Q8OUT)) ||
            a.C != 256 || a.C2 != 64 || a.Nout != 64 || a.ldb != 320 || a.ldy != 64 || !a.bias || a.bnx2 ||
            a.nth != 1 || a.ntw != 1 || a.sA != 1 || a.H != a.OH || a.W != a.OW || a.sY != 1 || a.YH != a.OH ||
            a.YW != a.OW || a.dh0 != 0 || a.dw0 != 0 || a.kh0 != 0 || a.kw0 != 0 || a.oy != 0 || a.ox != 0)
            return false;
        return p = one(a, stream(256, 64, 2, a.bnym ? 1 : 2, false, false, 64)), true;
    }
    if (a.flags & IG_STEM) {  // 7x7 stem, C = 4, K = 7 x 32
        if (a.flags & (IG_OUT_F32 | IG_FP8 | IG_ACCUM | IG_BNBWD | IG_NOSTREAM)) return false;
        if (has_bias || a.C != 4 || a.nth != 7 || a.ntw > 8 || a.ldb != 7 * 32 || a.Nout % 64 || a.ldy != a.Nout ||
            a.sY != 1 || a.YH != a.OH || a.YW != a.OW)
            return false;
        return p = one(a, stream(7 * 32, 64, 2, 0, true)), true;
    }
    if (a.flags & (IG_OUT_F32 | IG_FP8 | IG_REGSTAGE | IG_NOSTREAM)) return false;
    if (a.xbn) {  // BN apply + ReLU on the operand load: K = 64 / 128 plain-epilogue 1x1 convs only
        if ((a.flags & (IG_BNBWD | IG_ACCUM)) || a.bias || a.nth != 1 || a.ntw != 1 || a.sA != 1 ||
            a.H != a.OH || a.W != a.OW || a.sY != 1 || a.YH != a.OH || a.YW != a.OW || a.ldy != a.Nout ||
            a.ldb < a.C || a.dh0 != 0 || a.dw0 != 0)
            return p = fail(-120), true;
        if (a.C == 64 && a.Nout % 256 == 0) return p = one(a, stream(64, 256, 2, 0, false, true)), true;
        if (a.C == 64 && a.Nout % 128 == 0) return p = one(a, stream(64, 128, 3, 0, false, true)), true;
        if (a.C == 128 && a.Nout % 128 == 0) return p = one(a, stream(128, 128, 2, 0, false, true)), true;
        return p = fail(-120), true;
    }
    if (has_bias || a.nth != 1 || a.ntw != 1 || a.dh0 != 0 || a.dw0 != 0 || a.kh0 != 0 || a.kw0 != 0) return false;
    if (a.sY != 1 || a.oy != 0 || a.ox != 0 || a.YH != a.OH || a.YW != a.OW || a.ldy != a.Nout) return false;
    if (a.Nout % 64 != 0 || a.ldb < a.C) return false;
    if ((long)(a.OH - 1) * a.sA >= a.H || (long)(a.OW - 1) * a.sA >= a.W) return false;
    // K = 256 into > 128 channels (bottleneck conv3 / downsample forwards): 64-channel
    // weight slices resident in LDS, the slices of one pixel range on one XCD (the pixels
    // are fetched from HBM once and re-read from that XCD's L2).
    // Only K = 256: at K = 512 the v3 tiles win (conv_bench at 1024 img: 512 -> 2048 @7 fwd 210 -> 179 us,
    // 512 -> 1024 /2 @28 443 -> 375, 2048 -> 512 dgrad 209 -> 152; K = 256 stays here: 256 -> 1024 @14
    // fwd 264 vs 370).
    // 128-channel slices where Nout allows (half the slices re-reading each pixel group, twice the MFMAs per
    // loaded fragment: 256 -> 1024 @14 fwd 277 -> 246 us at 1024 img, round 5); tile 22 forces 64
    if (!(a.flags & IG_BNBWD) && a.C == 256 && a.Nout > 128) {
        if (bn != 64 && a.Nout % 128 == 0) return stream_slice(a, p, 256, 128, 2);
        if (bn != 0 && bn != 64) return false;
        return stream_slice(a, p, 256, 64, 2);
    }
    int maxbn = (a.C == 64 && !(a.flags & IG_BNBWD)) ? 256 : 128;
    if (a.flags & IG_BNBWD) {
        // BN-backward epilogue: every K = 64 / 128 / 256 dgrad, with or without the second BN branch, 128-channel
        // slices. Same-box bench A/B at R50 / 1024 with the ReLU mask as bits (round 3): 73.9 ms/step vs 75.2 with
        // K = 128 on the tiled kernels and 75.0 with the second branch there too; 64-channel slices neutral
        maxbn = 128;
    }
    if (bn == 0) bn = maxbn;
    while (bn > 64 && (bn > maxbn || a.Nout % bn)) bn >>= 1;
    if (a.C == 64) {
        // 256-channel slices: the fused-output / operand-BN variants prefetch 2 groups (3 spill at 256 VGPRs)
        if (bn == 256) return p = one(a, (a.flags & IG_FUSED_OUT) ? stream(64, 256, 2, 4) : stream(64, 256, 3, 0)), true;
        return stream_slice(a, p, 64, bn, 3);
    }
    if (a.C == 128) return stream_slice(a, p, 128, bn, 2);
    // K = 256 BN-backward dgrads into wide outputs (bottleneck conv1 dgrads 256 -> 512 @28, 256 -> 1024 @14): 64-channel
    // weight slices resident in LDS (as the K = 256 forwards) instead of the one-tile-per-block v3 loop, whose
    // 4-stage main loop leaves these epilogue-heavy GEMMs latency-bound (-20 % per call, round 4)
    if (a.C == 256 && (a.flags & IG_BNBWD) && a.Nout > 128) {
        // 128-channel slices (half the slices re-reading each pixel group): in-step A/B at 2048 img 16,622 / 16,663
        // vs 16,530 / 16,522 img/s with 64 (1024 -> 256 @14 dgrad + BN backward 705 -> 488 us, 512 -> 256 @28
        // 1460 -> 1033; at 1024 img round 5 they had measured even); tile 22 forces 64. The second-BN-branch form
        // stays on 64 (at 128 it spills 96 B: in-step 16,604 / 16,651 vs 16,662 / 16,653)
        if (bn_hint != 64 && a.Nout % 128 == 0 && !a.bnx2) return stream_slice(a, p, 256, 128, 2);
        return stream_slice(a, p, 256, 64, 2);
    }
    // K = 256 into <= 128 channels (bottleneck conv1 256 -> 64 / 128): 64-channel
    // slices, plain epilogue or the BN backward without a second branch
    if (a.C == 256 && a.Nout <= 128 && !((a.flags & IG_BNBWD) && a.bnx2)) return stream_slice(a, p, 256, 64, 2);
    return false;
}

// ---- the streaming BN-backward dgrad that also forms T = g^T h2 (conv_args.h gt_T; conv_stream.hip modes 6 / 7): the
// next block's conv1 dgrad, K = 64 / 128 into the 4p = 256 channels of a p = 64 bottleneck (ResNet-50's layer 1 and
// the first block of layer 2), mask bits without x, accumulating. Anything else with gt_T set is the error -125,
// never a kernel that would ignore T
// (p = 128, K = 128 / 256 into 512: not built; p = 256: the K = 256 producers have no registers left)
inline ConvPlan gramt_plan(const IGemmArgs& a, int tile) {
    constexpr int need = IG_BNBWD | IG_ACCUM;
    constexpr int never = IG_OUT_F32 | IG_RELU | IG_STEM | IG_REGSTAGE | IG_EPI_DIRECT | IG_FP8 | IG_BF8X | IG_AFFINE |
                          IG_NOSTREAM | IG_FUSED_OUT | IG_NEXT1;
    if (tile != 0 || (a.flags & need) != need || (a.flags & never) || a.bnx || !a.bnym || !a.gt_h2 || a.gt_p != 64 ||
        a.Nout != 4 * a.gt_p || (a.C != 64 && a.C != 128) || (a.C == 128 && a.bnx2) || a.bias || a.xbn || a.X2 ||
        a.nth != 1 || a.ntw != 1 || a.sA != 1 || a.H != a.OH || a.W != a.OW || a.dh0 != 0 || a.dw0 != 0 ||
        a.kh0 != 0 || a.kw0 != 0 || a.sY != 1 || a.oy != 0 || a.ox != 0 || a.YH != a.OH || a.YW != a.OW ||
        a.ldy != a.Nout || a.ldb < a.C)
        return fail(-125);
    return one(a, a.C == 64 ? stream(64, 128, 3, a.bnx2 ? 7 : 6) : stream(128, 128, 2, 6));
}

// ---- fp8 (conv_igemm_fp8.hip): C % 128 == 0 (every ResNet conv but the 64-channel ones of the first stage) runs the
// v3 LDS-DMA main loop with 1-byte operands (conv_igemm_v3.h, EB = 1): 256x256 tiles for Nout >= 512 with enough
// tiles and K >= 512, 128x128 for Nout >= 128, 128x64 below; explicit tiles 17 / 18 / 19 force those.
// The rest (and explicit tiles 2 / 4 / 8) takes the round-1 ring (igemm_dma_kernel, EB = 1).
inline ConvPlan fp8_plan(const IGemmArgs& a, int tile, long t8, int K) {
    const int fb = (a.flags & IG_BF8X) ? 1 : 0;  // the gathered operand: e4m3 activations / e5m2 gradients
    if (a.C % 16 != 0 || (a.flags & IG_OUT_F32) || a.bias || !a.xexp || !a.wexp) return fail(-105);
    if (!fb && (a.flags & (IG_BNBWD | IG_ACCUM))) return fail(-105);
    if ((tile == 0 || (tile >= 17 && tile <= 19)) && v3_ok8(a) && (tile != 19 || a.Nout % 64 == 0)) {
        if (tile == 0) tile = (a.Nout >= 512 && t8 >= BIG_MIN_TILES && K >= 512) ? 17 : (a.Nout >= 128 ? 18 : 19);
        if (tile == 17) return one(a, v3(256, 256, 2, 2, 8, 128, 1, fb));
        if (tile == 18) return one(a, v3(128, 128, 2, 2, 4, 128, 1, fb));
        return one(a, v3(128, 64, 1, 2, 4, 128, 1, fb));
    }
    if (tile >= 17 && tile <= 19) return fail(-105);
    const int md8 = (a.C % 128) == 0 ? 0 : 1;
    const bool lds_ok = a.Nout % 8 == 0 && a.ldy % 8 == 0 && !(a.flags & (IG_RELU | IG_EPI_DIRECT));
    const bool lds8 = lds_ok && ((a.flags & (IG_EPI_LDS | IG_BNBWD)) || (K + 127) / 128 > 4);
    if ((a.flags & IG_BNBWD) && !lds8) return fail(-104);
    if (tile == 0) tile = (a.Nout >= 256 && t8 >= BIG_MIN_TILES) ? 8 : (a.Nout <= 64 ? 4 : 2);
    const int epi = lds8 ? 2 : 0;
    switch (tile) {
        case 2: return one(a, dma(128, 128, 2, 2, md8, 4, epi, 1, fb));
        case 4: return one(a, dma(128, 64, 1, 3, md8, 4, epi, 1, fb));
        case 8: return one(a, dma(256, 256, 2, 2, md8, 8, epi, 1, fb));
        default: return fail(-101);
    }
}

// ---- the bf16 tiled kernels: the v3 loop, the LDS-DMA ring and the register-staged kernel
// explicit v3 tiles (conv_igemm_v3.h); 19: 256x128; 27 / 28: tap-inner; 29-32: deeper rings (round 6 A/B: the
// 2-deep ring waits vmcnt(0) at every stage, so one stage of MFMA time must cover the fill latency):
// 29 256x256 BK 32 x 4 (3 fills in flight, 128 KB), 30 256x256 BK 32 x 3, 31 128x128 BK 32 x 4 (64 KB,
// two blocks / CU), 32 128x128 BK 64 x 3 (96 KB, one block / CU)
// (a 16-wave 256x256 tile of 64 x 64 waves, round 5: no faster than these on any R50 shape, its staged BN-backward
// epilogue 1.4-1.7x slower from spills at 128 VGPRs -- not kept)
inline bool v3_tile(int tile, ConvKernel& k) {
    switch (tile) {
        case 17: return k = v3(256, 256, 2, 2, 8, 128), true;
        case 18: return k = v3(128, 128, 2, 2, 4, 128), true;
        case 19: return k = v3(256, 128, 2, 2, 8, 128), true;
        case 27: return k = v3(256, 256, 2, 2, 8, 128, 2, 0, true), true;
        case 28: return k = v3(128, 128, 2, 2, 4, 128, 2, 0, true), true;
        case 29: return k = v3(256, 256, 2, 4, 8, 64), true;
        case 30: return k = v3(256, 256, 2, 3, 8, 64), true;
        case 31: return k = v3(128, 128, 2, 4, 4, 64), true;
        case 32: return k = v3(128, 128, 2, 3, 4, 128), true;
    }
    return false;
}

// the LDS-DMA ring's explicit tiles, direct epilogue
inline bool dma_tile(int tile, int md, ConvKernel& k) {
    switch (tile) {
        case 1: return k = dma(256, 64, 1, 2, md, 4, 0), true;
        case 2: return k = dma(128, 128, 2, 2, md, 4, 0), true;
        case 3: return k = dma(64, 128, 4, 3, md, 4, 0), true;
        case 4: return k = dma(128, 64, 1, 3, md, 4, 0), true;
        case 5: return k = dma(128, 128, 2, 3, md, 4, 0), true;
        case 6: return k = dma(256, 128, 2, 3, md, 8, 0), true;  // 144 KiB LDS, 8 waves of 64x64
        case 7: return k = dma(128, 256, 4, 3, md, 8, 0), true;
        case 8: return k = dma(256, 256, 2, 2, md, 8, 0), true;  // 128 KiB LDS, 8 waves of 64x128
        case 9: return k = dma(256, 128, 2, 2, md, 8, 0), true;
    }
    return false;
}

}  // namespace conv_plan_detail

// cus: the device's CU count (the tail split's rounds); v3_deep: IMAGENT_V3_DEEP
inline ConvPlan conv_plan(const IGemmArgs& a, int tile, int cus, bool v3_deep) {
    using namespace conv_plan_detail;
    if (a.M <= 0 || a.Nout <= 0) return fail(0);
    if ((a.flags & IG_ACCUM) && (a.flags & IG_OUT_F32)) return fail(-103);
    if ((a.flags & IG_BNBWD) && ((a.flags & (IG_OUT_F32 | IG_RELU)) || a.Nout % 8 || a.ldy != a.Nout ||
                                 // no x (bn_gram.hip: sum(g xhat) comes from g^T h2): mask bits, staged epilogue
                                 (!a.bnx && (!a.bnym || (a.flags & IG_EPI_DIRECT))) ||
                                 !a.bnsave || !a.stats || (!a.bnym && (!a.bngamma || !a.bnbeta)) ||
                                 (a.bnx2 && !a.bnsave2)))
        return fail(-104);
    if ((a.flags & IG_NEXT1) && ((a.flags & IG_STEM) || a.xbn || a.X2 || tile != 0)) return fail(-122);
    if (a.gt_T) return gramt_plan(a, tile);
    ConvPlan p;
    ConvKernel k;
    if (a.flags & IG_STEM) {  // C == 4 row-segment gather, K = KH x 32
        if (a.C != 4 || a.ntw > 8 || a.dhs != 1 || a.dws != 1) return fail(-102);
        // the band stem (tile 0), else the streaming row-segment stem (tile 0 / 23, A/B), else the register-staged one
        if (tile == 0 && stem_band_ok(a)) return one(a, {CONV_STEM_BAND, {4}});
        if ((tile == 0 || tile == 23) && stream_plan(a, 0, p)) return p;
        return one(a, rs(128, 64, 1, 2, 0));
    }
    if (a.xbn) {  // the operand BN + ReLU: the halo kernel (64 -> 64 3x3) or the streaming 1x1, nothing else
        if (a.flags & (IG_FP8 | IG_OUT_F32 | IG_RELU | IG_AFFINE | IG_STEM | IG_BNBWD | IG_ACCUM)) return fail(-120);
        if (a.nth == 3 && a.ntw == 3) return halo_plan(a, p) ? p : fail(-120);
        return stream_plan(a, 0, p) ? p : fail(1);  // (1 with IG_REGSTAGE / IG_NOSTREAM / X2: as it always was)
    }
    const long t8 = (long)((a.M + 255) / 256) * ((a.Nout + 255) / 256);  // 256x256 tiles of the whole problem
    const int K = a.nth * a.ntw * a.C;
    if (a.X2) {  // two K segments (bn_gram.hip): the streaming kernel for 256 + 64 -> 64, else the v3 loop
        // (the streaming kernel where it takes the shape: 963 vs 1087 us per call in-step for the layer-1 form;
        // tile != 0 forces the v3 loop, tests / A/B)
        if (tile == 0 && stream_plan(a, 0, p)) return p;
        if (!v3_ok(a) || a.Nout % 64) return fail(-106);
        if (a.Nout >= V3_BIG_MIN_N && t8 >= BIG_MIN_TILES) return one(a, v3(256, 256, 2, 2, 8, 128));
        return one(a, a.Nout == 64 ? v3(128, 64, 1, 2, 4, 128) : v3(128, 128, 2, 2, 4, 128));
    }
    if (a.flags & IG_FP8) return fp8_plan(a, tile, t8, K);
    if (a.C % 8 != 0) return fail(-100);  // 16-byte chunks must not straddle taps
    if (tile == 0 && a.C == 64 && a.Nout == 64 && a.nth == 3 && a.ntw == 3 && halo_plan(a, p)) return p;
    const int md = (a.C % BK) == 0 ? 0 : 1;
    // short-K 1x1 convs (K = C = 64 / 128) are HBM streams: weights resident in
    // LDS, pixel fragments straight from HBM (conv_stream.hip); tiles 20/21/22
    // force its 256/128/64-channel slices (A/B testing) and choose as tile 0 where it does not take the conv
    const int slice = tile >= 20 && tile <= 22 ? 256 >> (tile - 20) : 0;
    const bool autotile = tile == 0 || slice != 0;
    if (autotile && a.nth == 1 && a.ntw == 1 && (a.C == 64 || a.C == 128 || a.C == 256 || a.C == 512) &&
        stream_plan(a, slice, p))
        return p;
    if (a.flags & (IG_FUSED_OUT | IG_NEXT1)) return fail(-121);  // only the streaming kernel has that epilogue
    // measured on MI355X (profiles/r50_conv_layers_*): the register-staged
    // pipeline wins for 64-wide output tiles and single-stage (K <= 64) tiles,
    // the LDS-DMA ring for everything with a real K loop
    const bool regstage = (a.flags & IG_REGSTAGE) || (autotile && (a.Nout <= 64 || K <= BK));
    if (autotile) {
        tile = (a.Nout <= 64) ? 4 : 2;
        // 256x256 tiles (8 waves, one block per CU) halve the L2->LDS bytes per
        // MFMA FLOP -- the measured limiter of the 128x128 tile (~70 GB/s per CU
        // of gathered rows, profiles/r50_conv_tiles_*.md) -- but only pay when
        // the output is >= 256 channels wide and there are enough of them to
        // occupy the chip
        if (!regstage && a.Nout >= 256 && t8 >= BIG_MIN_TILES) tile = 8;
    }
    const bool bnb = a.flags & IG_BNBWD;
    // staged epilogue: bf16, no bias; the eval forward's folded BatchNorm (+ ReLU) too
    const bool eval_bn = (a.flags & IG_AFFINE) && !a.stats;
    const bool lds_ok = !(a.flags & IG_OUT_F32) && (!(a.flags & IG_RELU) || eval_bn) && (!a.bias || eval_bn) &&
                        a.Nout % 8 == 0 && a.ldy % 8 == 0;
    // staged epilogue: always with the fused BN backward; otherwise for long-K
    // tiles (non-persistent anyway, +5-10 % measured) -- short-K memory-bound
    // 1x1 convs keep the persistent grid and its epilogue/prefetch overlap
    const bool use_lds = lds_ok && !(a.flags & IG_EPI_DIRECT) &&
                         (bnb || (a.flags & IG_EPI_LDS) || (K + BK - 1) / BK > 4);
    if (v3_tile(tile, k)) return use_lds && v3_ok(a) ? one(a, k) : fail(-105);
    if (autotile && use_lds && md == 0 && a.Nout >= 128 && v3_ok(a)) {
        // forward-type convs (BN statistics or the eval BN affine in the epilogue, no fused BN backward): 32-deep
        // stages with 2-3 fills in flight instead of 64-deep x 2 (whose vmcnt(0) at every stage leaves one stage of
        // MFMA time to cover the fill latency). Round 6, isolated at 2048 img (scripts/runs/ring_ab.sh, tiles 30 / 31
        // vs 17 / 18): forwards 256@14 3x3 554 -> 502 us, 1024 -> 256 @14 346 -> 325, 512@7 3x3 521 -> 491, 256@28
        // 3x3 s2 642 -> 567, 128@28 3x3 721 -> 665, 512 -> 128 @28 570 -> 498; the dgrads (plain or with the fused
        // BN backward) gain nothing (-3 .. +2 %). In-step at 4096 img the isolated gain does NOT carry over:
        // 17,317 / 17,289 img/s with it vs 17,358 / 17,395 without, alternating on one box -- so it stays OFF by
        // default; IMAGENT_V3_DEEP=1 turns it on (A/B), tiles 29-32 remain as tested explicit variants
        const bool fwd_ring = v3_deep && !bnb && (a.stats || (a.flags & IG_AFFINE));
        const ConvKernel big = fwd_ring ? v3(256, 256, 2, 3, 8, 64) : v3(256, 256, 2, 2, 8, 128);
        const ConvKernel small = fwd_ring ? v3(128, 128, 2, 4, 4, 64) : v3(128, 128, 2, 2, 4, 128);
        // (the fused BN-backward dgrads on 128x128 tiles with their epilogue operands prefetched instead: within
        // +-5 % per shape, profiles/r50_b1024_round4_kernel_ab.md -- not taken; again at 2048 img in round 5, isolated
        // 2-7 % faster, in-step 16,584 / 16,576 vs 16,612 / 16,621 img/s)
        if (a.Nout >= V3_BIG_MIN_N && t8 >= BIG_MIN_TILES && K >= V3_BIG_MIN_K) return big_or_split(a, cus, big, small);
        // (256x128 tiles on 8 waves for the 128-channel outputs, tile 19, round 5: forward 3-6 % faster stand-alone,
        // dgrad 6 % and the fused BN-backward dgrads 7-21 % slower, in-step 16,822 / 16,842 vs 17,003 / 16,991 img/s
        // -- not taken, profiles/r50_b2048_r5_v3_256x128.md)
        return one(a, small);
    }
    if (bnb || use_lds) {  // the tiles the auto choice makes, with a fused (1) / staged (2) epilogue
        const int epi = use_lds ? 2 : 1;
        if (regstage || (tile != 2 && tile != 8)) return one(a, tile == 2 ? rs(128, 128, 2, md, epi) : rs(128, 64, 1, md, epi));
        const ConvKernel big = dma(256, 256, 2, 2, md, 8, epi), small = dma(128, 128, 2, 2, md, 4, epi);
        if (tile == 8) return use_lds && autotile ? big_or_split(a, cus, big, small) : one(a, big);
        return one(a, small);
    }
    if (regstage) {
        if (tile == 2) return one(a, rs(128, 128, 2, md, 0));
        return tile == 4 ? one(a, rs(128, 64, 1, md, 0)) : fail(-101);
    }
    return dma_tile(tile, md, k) ? one(a, k) : fail(-101);
}
