// fp8 (OCP e4m3 / e5m2) implicit-GEMM convolutions on the block-scaled MFMA
// (v_mfma_scale_f32_16x16x128_f8f6f4; kernels in conv_igemm_impl.h, EB = 1):
//  * forward: X = e4m3 activations, Wk = e4m3 weights;
//  * dgrad (IG_BF8X): X = e5m2 upstream gradient, Wk = e4m3 transposed
//    weights, with the same fused epilogues as bf16 (IG_ACCUM residual
//    accumulation, IG_BNBWD BatchNorm-backward reductions).
// Per-tensor power-of-two scales (device ints xexp / wexp) ride in the MFMA's
// E8M0 scale operands.

// Which of them a conv runs: conv_plan.h (fp8_plan).

#include "conv_igemm_impl.h"
#include "conv_igemm_v3.h"

int conv_launch_fp8(const ConvKernel& k, const IGemmArgs& a, hipStream_t st) {
    if (k.fam == CONV_V3_FP8) {
#define X(...) CONV_LAUNCH_IF(CONV_V3_FP8, launch_v3, __VA_ARGS__)
        CONV_V3_FP8_KERNELS(X)
#undef X
    } else {
#define X(...) CONV_LAUNCH_IF(CONV_DMA_FP8, launch_dma, __VA_ARGS__)
        CONV_DMA_FP8_KERNELS(X)
#undef X
    }
    return CONV_RC_UNLISTED;
}
