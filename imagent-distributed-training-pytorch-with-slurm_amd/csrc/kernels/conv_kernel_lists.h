// Every forward / dgrad conv kernel instantiation, once: X(template arguments in declaration order). The translation
// unit named at each list expands it into its launch switch (the only place the kernels are instantiated);
// conv_plan.h expands all of them into conv_kernel_listed(), which the host test runs over the whole dispatch grid.
// The order of the entries -- and of the sublists in conv_igemm.hip's launch_planned -- is the order the dispatch chain
// first named them in, which is the order the compiler lays the kernels out in: the code objects keep their layout
// (and the ring kernels their PC-relative distance to g_igemm_zero) from before the plan existed. Append new ones.
#pragma once

// igemm_rs_kernel<BM, BN, WN, MODE, EPI> (conv_igemm.hip); MODE 2: the stem's row segments
#define CONV_RS_STEM(X) X(128, 64, 1, 2, 0)
#define CONV_RS_EPI(X, EPI) X(128, 128, 2, 0, EPI) X(128, 128, 2, 1, EPI) X(128, 64, 1, 0, EPI) X(128, 64, 1, 1, EPI)
#define CONV_RS_KERNELS(X) CONV_RS_STEM(X) CONV_RS_EPI(X, 2) CONV_RS_EPI(X, 1) CONV_RS_EPI(X, 0)

// igemm_v3_kernel<BM, BN, WN, NS, NW, RB, EB, FB, TI>, bf16 (conv_igemm.hip)
#define CONV_V3_KERNELS(X)                                                                                    \
    X(256, 256, 2, 2, 8, 128, 2, 0, false) X(128, 64, 1, 2, 4, 128, 2, 0, false) X(128, 128, 2, 2, 4, 128, 2, 0, false) \
    X(256, 128, 2, 2, 8, 128, 2, 0, false) X(256, 256, 2, 2, 8, 128, 2, 0, true) X(256, 256, 2, 4, 8, 64, 2, 0, false) \
    X(256, 256, 2, 3, 8, 64, 2, 0, false) X(128, 128, 2, 4, 4, 64, 2, 0, false) X(128, 128, 2, 3, 4, 128, 2, 0, false) \
    X(128, 128, 2, 2, 4, 128, 2, 0, true)

// igemm_dma_kernel<BM, BN, WN, NS, MODE, NW, EPI, EB, FB, RB>, bf16 (conv_igemm.hip): the auto choice's two tiles with
// the fused (1) / staged (2) epilogue, tiles 1-9 with the direct one
#define CONV_DMA_EPI(X, EPI)                                                                                  \
    X(256, 256, 2, 2, 0, 8, EPI, 2, 0, 128) X(256, 256, 2, 2, 1, 8, EPI, 2, 0, 128)                           \
    X(128, 128, 2, 2, 0, 4, EPI, 2, 0, 128) X(128, 128, 2, 2, 1, 4, EPI, 2, 0, 128)
#define CONV_DMA_TILE_(X, BM, BN, WN, NS, NW) X(BM, BN, WN, NS, 0, NW, 0, 2, 0, 128) X(BM, BN, WN, NS, 1, NW, 0, 2, 0, 128)
#define CONV_DMA_DIRECT(X)                                                                                    \
    CONV_DMA_TILE_(X, 256, 64, 1, 2, 4) CONV_DMA_TILE_(X, 128, 128, 2, 2, 4) CONV_DMA_TILE_(X, 64, 128, 4, 3, 4)  \
    CONV_DMA_TILE_(X, 128, 64, 1, 3, 4) CONV_DMA_TILE_(X, 128, 128, 2, 3, 4) CONV_DMA_TILE_(X, 256, 128, 2, 3, 8) \
    CONV_DMA_TILE_(X, 128, 256, 4, 3, 8) CONV_DMA_TILE_(X, 256, 256, 2, 2, 8) CONV_DMA_TILE_(X, 256, 128, 2, 2, 8)
#define CONV_DMA_KERNELS(X) CONV_DMA_EPI(X, 2) CONV_DMA_EPI(X, 1) CONV_DMA_DIRECT(X)

// fp8 (conv_igemm_fp8.hip), EB = 1, FB 0 e4m3 / 1 e5m2 gathered operand: v3's three tiles, then the ring's three tiles
// with the staged (2) / direct (0) epilogue
#define CONV_V3_FP8_FB_(X, FB)                                                                                \
    X(256, 256, 2, 2, 8, 128, 1, FB, false) X(128, 128, 2, 2, 4, 128, 1, FB, false) X(128, 64, 1, 2, 4, 128, 1, FB, false)
#define CONV_V3_FP8_KERNELS(X) CONV_V3_FP8_FB_(X, 1) CONV_V3_FP8_FB_(X, 0)
#define CONV_DMA_FP8_FB_(X, BM, BN, WN, NS, NW, FB)                                                           \
    X(BM, BN, WN, NS, 0, NW, 2, 1, FB, 128) X(BM, BN, WN, NS, 1, NW, 2, 1, FB, 128)                           \
    X(BM, BN, WN, NS, 0, NW, 0, 1, FB, 128) X(BM, BN, WN, NS, 1, NW, 0, 1, FB, 128)
#define CONV_DMA_FP8_TILE_(X, BM, BN, WN, NS, NW)                                                             \
    CONV_DMA_FP8_FB_(X, BM, BN, WN, NS, NW, 1) CONV_DMA_FP8_FB_(X, BM, BN, WN, NS, NW, 0)
#define CONV_DMA_FP8_KERNELS(X)                                                                               \
    CONV_DMA_FP8_TILE_(X, 128, 128, 2, 2, 4) CONV_DMA_FP8_TILE_(X, 128, 64, 1, 3, 4) CONV_DMA_FP8_TILE_(X, 256, 256, 2, 2, 8)

// conv_stream_kernel<K, BN, D, MODE, STEM, XBN, K2> (conv_stream.hip): the 256-channel slice of K = 64 with the next
// conv1 (mode 5), the two-segment Gram dgrads, the row-segment stem, the operand-BN forms, then the slice kernels:
// fused-output (4) and plain (0), BN backward with a second branch (3), from the mask bits (1), from x (2); last the
// mask-bit dgrads that also form the previous Gram-form block's T = g^T h2 (6 = 1 + T, 7 = 3 + T; p = 64)
#define CONV_STREAM_PLAIN_(X, K, BN, D) X(K, BN, D, 4, false, false, 0) X(K, BN, D, 0, false, false, 0)
#define CONV_STREAM_BNB_(X, K, BN, D) X(K, BN, D, 1, false, false, 0) X(K, BN, D, 2, false, false, 0)
#define CONV_STREAM_ALL_(X, K, BN, D)                                                                         \
    CONV_STREAM_PLAIN_(X, K, BN, D) X(K, BN, D, 3, false, false, 0) CONV_STREAM_BNB_(X, K, BN, D)
#define CONV_STREAM_KERNELS(X)                                                                                \
    X(64, 256, 1, 5, false, false, 0) X(256, 64, 2, 1, false, false, 64) X(256, 64, 2, 2, false, false, 64)   \
    X(7 * 32, 64, 2, 0, true, false, 0)                                                                       \
    X(64, 256, 2, 0, false, true, 0) X(64, 128, 3, 0, false, true, 0) X(128, 128, 2, 0, false, true, 0)       \
    CONV_STREAM_PLAIN_(X, 256, 128, 2) CONV_STREAM_PLAIN_(X, 256, 64, 2)                                      \
    X(64, 256, 2, 4, false, false, 0) X(64, 256, 3, 0, false, false, 0)                                       \
    CONV_STREAM_ALL_(X, 64, 128, 3) CONV_STREAM_ALL_(X, 64, 64, 3) CONV_STREAM_ALL_(X, 128, 128, 2)           \
    CONV_STREAM_ALL_(X, 128, 64, 2)                                                                           \
    CONV_STREAM_BNB_(X, 256, 128, 2) X(256, 64, 2, 3, false, false, 0) CONV_STREAM_BNB_(X, 256, 64, 2)         \
    X(64, 128, 3, 6, false, false, 0) X(64, 128, 3, 7, false, false, 0) X(128, 128, 2, 6, false, false, 0)

// stem_band_kernel<R> (conv_stream.hip)
#define CONV_STEM_BAND_KERNELS(X) X(4)

// halo3x3_kernel<W, R, EPI> (conv_halo.hip)
#define CONV_HALO_KERNELS(X) X(56, 4, 2) X(56, 4, 1) X(56, 4, 0) X(112, 2, 2) X(112, 2, 1) X(112, 2, 0)
