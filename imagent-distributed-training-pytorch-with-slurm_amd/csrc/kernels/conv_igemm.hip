// MFMA implicit-GEMM convolution for gfx950 (MI355X): the bf16 launcher.
// Kernels, layout and design notes: conv_igemm_impl.h; fp8: conv_igemm_fp8.hip.
//
// Which kernel a conv runs is decided in one place, conv_plan() (conv_plan.h: plain C++, checked on the CPU by
// tests/test_conv_plan.py); imk_conv_igemm launches what it returns. Each translation unit instantiates the kernels
// of its own lists (conv_kernel_lists.h) and nothing else: v3 / LDS-DMA ring / register-staged bf16 here, the fp8
// ones in conv_igemm_fp8.hip, streaming and stem band in conv_stream.hip, halo in conv_halo.hip.

#include "conv_igemm_impl.h"
#include "conv_igemm_v3.h"

// the images [i0, i0 + n) of a conv: every pixel-indexed operand advances by whole images
static IGemmArgs image_range(const IGemmArgs& a, int i0, int n) {
    const long xs = (long)a.H * a.W * a.C, ys = (long)a.YH * a.YW * a.ldy;
    IGemmArgs t = a;
    t.N = n;
    t.M = n * a.OH * a.OW;
    t.X = a.X + i0 * xs;
    t.Y = static_cast<bf16_t*>(a.Y) + i0 * ys;  // staged epilogue: bf16 output only
    if (a.bnx) t.bnx = a.bnx + i0 * ys;
    if (a.bnym) t.bnym = a.bnym + i0 * ys / 8;
    if (a.bnx2) t.bnx2 = a.bnx2 + i0 * ys;
    return t;
}

// (the sublists in the order conv_kernel_lists.h explains)
static int launch_planned(const ConvKernel& k, const IGemmArgs& a, hipStream_t st) {
#define RS(...) CONV_LAUNCH_IF(CONV_RS, launch_rs, __VA_ARGS__)
#define V3(...) CONV_LAUNCH_IF(CONV_V3, launch_v3, __VA_ARGS__)
#define DMA(...) CONV_LAUNCH_IF(CONV_DMA, launch_dma, __VA_ARGS__)
    CONV_RS_STEM(RS)
    CONV_V3_KERNELS(V3)
    CONV_RS_EPI(RS, 2) CONV_RS_EPI(RS, 1)
    CONV_DMA_EPI(DMA, 2) CONV_DMA_EPI(DMA, 1)
    CONV_RS_EPI(RS, 0)
    CONV_DMA_DIRECT(DMA)
#undef RS
#undef V3
#undef DMA
    switch (k.fam) {
        case CONV_DMA_FP8:
        case CONV_V3_FP8: return conv_launch_fp8(k, a, st);
        case CONV_STREAM:
        case CONV_STEM_BAND: return conv_launch_stream(k, a, st);
        case CONV_HALO: return conv_launch_halo(k, a, st);
    }
    return CONV_RC_UNLISTED;
}

extern "C" int g_imk_conv_launches = 0;
IMK_EXPORT int imk_conv_launches() { return g_imk_conv_launches; }

IMK_EXPORT int imk_conv_igemm(const IGemmArgs* args, int tile, void* stream) {
    static const bool deep = [] {
        const char* e = getenv("IMAGENT_V3_DEEP");
        return e && atoi(e) != 0;
    }();
    const IGemmArgs& a = *args;
    const ConvPlan p = conv_plan(a, tile, device_cus(), deep);
    if (p.rc != 0) return p.rc;
    for (int i = 0; i < p.n; ++i) {
        const ConvLaunch& l = p.part[i];
        const int r = l.nimg == a.N ? launch_planned(l.k, a, (hipStream_t)stream)
                                    : launch_planned(l.k, image_range(a, l.img0, l.nimg), (hipStream_t)stream);
        if (r != 0) return r;
    }
    return 0;
}

IMK_EXPORT int imk_igemm_args_size() { return (int)sizeof(IGemmArgs); }
