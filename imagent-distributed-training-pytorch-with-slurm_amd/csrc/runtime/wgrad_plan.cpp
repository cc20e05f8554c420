// The weight-gradient launchers' split-K plan (csrc/kernels/conv_wgrad_plan.h, plain C++) exported from the host
// runtime, so tests/test_wgrad_plan.py checks it -- the 2^31-byte halving above all -- without a GPU.
#include <cstdint>

#include "../kernels/conv_wgrad_plan.h"

extern "C" {

// out[0] = splits, out[1] = m_per_split; -1: an argument out of range. row_bytes 0: no byte limits
int imr_wgrad_plan(int M, int ntiles, int BR, int target, int splits, int64_t row_bytes, int64_t ohw,
                   int64_t img_bytes, int32_t* out) {
    if (M <= 0 || ntiles <= 0 || BR <= 0 || target <= 0 || row_bytes < 0 || ohw <= 0 || img_bytes < 0 || !out) return -1;
    const WgradPlan p = wgrad_plan(M, ntiles, BR, target, splits, (size_t)row_bytes, (size_t)ohw, (size_t)img_bytes);
    out[0] = p.splits;
    out[1] = p.m_per_split;
    return 0;
}

}  // extern "C"
