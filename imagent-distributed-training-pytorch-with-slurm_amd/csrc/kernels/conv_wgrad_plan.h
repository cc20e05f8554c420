// Split-K plan of the weight-gradient launchers (host, plain C++: the runtime library exports it as imr_wgrad_plan
// so tests/test_wgrad_plan.py checks it without a GPU).
#pragma once

#include <algorithm>
#include <cstddef>

struct WgradPlan {
    int splits, m_per_split;
};

// M reduction rows over `splits` blocks per tile (<= 0: as many as bring ntiles x splits to `target` blocks, each at
// least 4 stages of BR rows deep). m_per_split is a multiple of BR -- a split's last stage never reads the next
// split's rows -- and splits is recomputed from it, so no split is empty.
// row_bytes > 0: the kernel addresses a split's dY rows (row_bytes each) and X images (img_bytes each, ohw rows per
// image, up to 2 more touched at the ends) by 32-bit offsets from the split's own base: m_per_split is halved until
// both stay below 2^31 bytes (or one stage is left).
inline WgradPlan wgrad_plan(int M, int ntiles, int BR, int target, int splits, size_t row_bytes = 0, size_t ohw = 1,
                            size_t img_bytes = 0) {
    if (splits <= 0) {
        const int want = (target + ntiles - 1) / ntiles;
        const int maxs = (M + 4 * BR - 1) / (4 * BR);
        splits = std::max(1, std::min(want, maxs));
    }
    int mps = (M + splits - 1) / splits;
    mps = (mps + BR - 1) / BR * BR;
    const size_t lim = (size_t)1 << 31;
    while (row_bytes && mps > BR && ((size_t)mps * row_bytes >= lim || ((size_t)mps / ohw + 2) * img_bytes >= lim))
        mps = (mps / 2 + BR - 1) / BR * BR;
    return {(M + mps - 1) / mps, mps};
}
