// The implicit-GEMM convolutions' argument block and flags (plain C++, no HIP include: the kernels, the host-side
// dispatch plan of conv_plan.h and the host runtime's export of it all read this one definition).
#pragma once

#include <stdint.h>

typedef uint16_t bf16_t;  // storage type (raw bits), as common.h

struct IGemmArgs {
    const bf16_t* X;   // gathered operand, NHWC [N][H][W][C]
    const bf16_t* Wk;  // [Nout][ldb] bf16
    void* Y;           // output NHWC, channel stride ldy
    const float* bias; // [Nout] or null
    float* stats;      // [STAT_SLOTS][2][Nout] (sum, sumsq) slab or null, fp32 atomics
    int N, H, W, C;
    int OH, OW, M;     // row grid, M = N*OH*OW
    int Nout, ldb;
    int sA;
    int nth, ntw, dh0, dhs, dw0, dws, kh0, khs, kw0, kws, KW;
    int YH, YW, sY, oy, ox, ldy;
    int flags;         // IG_* bits
    // IG_BNBWD: the BatchNorm this gradient flows into (all NHWC at the output
    // pixels, channel stride ldy == Nout)
    const bf16_t* bnx;     // BN input x
    // ReLU mask of the BN(+add)+ReLU output as bits (bn.hip bn_fwd ym: byte e/8 of element e, bit
    // e%8 = output > 0; 1/16 of the bytes of re-reading the bf16 output), or null: mask from x
    const uint8_t* bnym;
    const float* bnsave;   // [2][Nout] mean, rstd
    const float* bngamma;  // used with the from-x mask
    const float* bnbeta;
    const bf16_t* bnx2;    // second BN branch input (downsample), or null
    const float* bnsave2;
    // IG_FP8: X and Wk hold e4m3 values x*2^-ex, w*2^-ew; the per-tensor
    // exponents live on the device (delayed scaling, no host sync) and enter
    // the MFMA as E8M0 scales 127 + e
    const int* xexp;
    const int* wexp;
    // forward statistics are SHIFTED sums: sum(v - shift[n]), sum((v - shift[n])^2)
    // with shift = the BN's previous batch mean (null: 0). With shift ~ mean the
    // variance E[(v-s)^2] - E[v-s]^2 has no catastrophic cancellation even when
    // |mean| >> std (imk_bn_stats_finalize turns the slab into mean / variance).
    const float* shift;
    // conv_stream only: the gathered operand is relu(X * xbn[c] + xbn[C + c]) per input channel c --
    // the producing BatchNorm's apply + ReLU done on the consumer's operand load (ops/block.py),
    // so the BN output is never written
    const float* xbn;
    // v3 only: a second K segment -- after the C channels of X, C2 more from X2 (same pixels, row pitch C2;
    // 1x1 stride-1 gathers), the weights' columns [C, C + C2). With IG_BNBWD, `bias` [Nout] is added to
    // the sums before the mask (bn_gram.hip: the bottleneck's bn3 backward folded into conv3's dgrad)
    const bf16_t* X2;
    int C2;
    // IG_Q8OUT (streaming 1x1 only): also the e4m3 copy of the stored bf16 output for fp8 consumers, quantised
    // with 2^-y8exp[0] (delayed scaling, fp8.hip), |y| max into y8amax[blockIdx & 31] (as bn_fwd's y8)
    void* Y8;
    const int* y8exp;
    float* y8amax;
    // IG_NEXT1 (streaming 1x1 fused-output kernel, K = 64 into Nout = 256 only): also the NEXT 1x1 stride-1 conv on
    // the stored output, Y2 [M][Co2] = Y [M][Nout] x W2^T with W2 [Co2][ldb2] (the following bottleneck's conv1),
    // bit-identical to that conv run on Y; its shifted forward statistics go to stats2 [STAT_SLOTS][2][Co2] around
    // shift2 [Co2] (either may be null, as stats / shift)
    const bf16_t* W2;
    bf16_t* Y2;
    float* stats2;
    const float* shift2;
    int Co2, ldb2;
    // gt_T non-null (streaming 1x1 only; IG_BNBWD from the mask bits without x, with IG_ACCUM -- a bottleneck's conv1
    // dgrad finishing the PREVIOUS Gram-form block's output gradient g): the same launch also accumulates
    // gt_T [Nout][gt_p] fp32 += g^T h2 over the stored bf16 bits of g, with gt_h2 [M][gt_p] bf16 that block's conv3
    // input (bn_gram.hip's T, the pass ops/bn_gram.py gram_T otherwise makes over g). A request, not a hint: a shape
    // the kernel does not cover is an error (conv_plan.h -125). Signalled by the pointer, as xbn / X2 are
    const bf16_t* gt_h2;
    float* gt_T;
    int gt_p;
};

#define IG_OUT_F32 1   // fp32 output (else bf16)
#define IG_RELU 2      // ReLU on the output
#define IG_STEM 4      // stem row-segment gather
#define IG_ACCUM 8     // out += result (bf16 out only): fused gradient accumulation
#define IG_REGSTAGE 16 // force the register-staged main loop (A/B testing)
#define IG_BNBWD 32    // epilogue = ReLU mask + BatchNorm-backward reductions (slab [32][3][Nout])
#define IG_EPI_LDS 64  // LDS-staged coalesced epilogue (default for IG_BNBWD)
#define IG_EPI_DIRECT 128  // direct register epilogue even for IG_BNBWD (A/B testing)
#define IG_FP8 256     // fp8 operands on the block-scaled MFMA (conv_igemm_fp8.hip)
#define IG_BF8X 512    // with IG_FP8: the gathered operand X is e5m2 (gradients), Wk e4m3
#define IG_AFFINE 1024 // inference BN folded into the epilogue: out = acc * bias[n] + bias[Nout + n]
#define IG_NOSTREAM 2048  // never the streaming short-K 1x1 kernel (conv_stream.hip; A/B testing)
#define IG_ACCUM_SUB2 4096  // with IG_ACCUM: the old output is valid only at even (y, x) output pixels
                           // (a stride-2 1x1 dgrad wrote only that parity class, no memset); elsewhere 0
#define IG_RES 8192   // (streaming 1x1 only) out = act(affine(acc) + bnx[e]): a residual read from bnx, not from Y
#define IG_Q8OUT 32768  // (streaming 1x1 only) also the e4m3 copy of the output (Y8 / y8exp / y8amax)
#define IG_MASKOUT 16384  // (streaming 1x1 only, with IG_RELU) also write the ReLU mask of the stored output as bits
                          // into bnym (byte e / 8, bit e % 8; bn.hip bn_fwd's `ym` format)
#define IG_NEXT1 65536  // (streaming 1x1 only, with IG_RES / IG_MASKOUT) also the next 1x1 conv of the stored output
                        // (W2 / Y2 / stats2 / shift2 / Co2 / ldb2)
#define STAT_SLOTS 32  // stats slab: [STAT_SLOTS][2][Nout]
