// The forward / dgrad conv dispatch plan (csrc/kernels/conv_plan.h, plain C++) exported from the host runtime, so
// tests/test_conv_plan.py checks its decisions without a GPU, and ops/_lib.py names the IG_* flags and explains the
// conv return codes from the header's own values.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../kernels/conv_plan.h"

// the demangled kernel name prefix a profiler shows, e.g. igemm_v3_kernel<128, 128, 2, 2, 4, 128, 2, 0, false>
static int conv_kernel_name(const ConvKernel& k, char* buf, size_t n) {
    const int* p = k.p;
    const char* const tf[2] = {"false", "true"};
    switch (k.fam) {
        case CONV_RS: return snprintf(buf, n, "igemm_rs_kernel<%d, %d, %d, %d, %d>", p[0], p[1], p[2], p[3], p[4]);
        case CONV_DMA:
        case CONV_DMA_FP8:
            return snprintf(buf, n, "igemm_dma_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d>", p[0], p[1], p[2], p[3],
                            p[4], p[5], p[6], p[7], p[8], p[9]);
        case CONV_V3:
        case CONV_V3_FP8:
            return snprintf(buf, n, "igemm_v3_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %s>", p[0], p[1], p[2], p[3], p[4],
                            p[5], p[6], p[7], tf[p[8] != 0]);
        case CONV_STREAM:
            return snprintf(buf, n, "conv_stream_kernel<%d, %d, %d, %d, %s, %s, %d>", p[0], p[1], p[2], p[3],
                            tf[p[4] != 0], tf[p[5] != 0], p[6]);
        case CONV_STEM_BAND: return snprintf(buf, n, "stem_band_kernel<%d>", p[0]);
        case CONV_HALO: return snprintf(buf, n, "halo3x3_kernel<%d, %d, %d>", p[0], p[1], p[2]);
    }
    return snprintf(buf, n, "?");
}

extern "C" {

constexpr int CONV_PLAN_NAME_BYTES = 96;
constexpr int CONV_PLAN_PART_INTS = 3 + CONV_PLAN_NAME_BYTES / 4;

// out[0] = return code, out[1] = launches (0-2); per launch CONV_PLAN_PART_INTS ints from out[2]: first image, images,
// 1 when the kernel is in its family's list, then the kernel's name (CONV_PLAN_NAME_BYTES bytes, zero-terminated)
int imr_conv_plan(const IGemmArgs* a, int tile, int cus, int deep, int32_t* out) {
    if (!a || !out || cus < 1) return -1;
    const ConvPlan p = conv_plan(*a, tile, cus, deep != 0);
    out[0] = p.rc;
    out[1] = p.n;
    for (int i = 0; i < p.n; ++i) {
        int32_t* o = out + 2 + i * CONV_PLAN_PART_INTS;
        o[0] = p.part[i].img0;
        o[1] = p.part[i].nimg;
        o[2] = conv_kernel_listed(p.part[i].k);
        memset(o + 3, 0, CONV_PLAN_NAME_BYTES);
        conv_kernel_name(p.part[i].k, reinterpret_cast<char*>(o + 3), CONV_PLAN_NAME_BYTES);
    }
    return 0;
}

int imr_conv_plan_out_ints() { return 2 + 2 * CONV_PLAN_PART_INTS; }
int imr_conv_args_size() { return (int)sizeof(IGemmArgs); }
int imr_conv_tail_split_images(const IGemmArgs* a, int cus) { return conv_plan_detail::tail_split_images(*a, cus); }
const char* imr_conv_error_reason(int rc) { return conv_error_reason(rc); }

// the IG_* flags in declared order: name into `name` (32 bytes), value returned; 0 past the last
int imr_conv_flag(int i, char* name) {
#define F(x) {#x, x}
    static const struct {
        const char* name;
        int value;
    } flags[] = {F(IG_OUT_F32), F(IG_RELU), F(IG_STEM), F(IG_ACCUM), F(IG_REGSTAGE), F(IG_BNBWD), F(IG_EPI_LDS),
                 F(IG_EPI_DIRECT), F(IG_FP8), F(IG_BF8X), F(IG_AFFINE), F(IG_NOSTREAM), F(IG_ACCUM_SUB2), F(IG_RES),
                 F(IG_Q8OUT), F(IG_MASKOUT), F(IG_NEXT1)};
#undef F
    if (i < 0 || i >= (int)(sizeof(flags) / sizeof(flags[0]))) return 0;
    strncpy(name, flags[i].name, 31);
    name[31] = 0;
    return flags[i].value;
}

}  // extern "C"
