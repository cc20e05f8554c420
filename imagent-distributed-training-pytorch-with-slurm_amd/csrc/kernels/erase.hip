// Random Erasing (Zhong et al.) of the model input, in place (data/erase.py holds the definition: the draws, the
// noise as integer arithmetic, and the torch backend this kernel is tested against).
//
// x is NHWC [B][H][W][CP], bf16 or fp32, CP 4 or 8, as the normalise kernels leave it. boxes int32 [B][N][4] = (top,
// left, h, w); inside a box channels 0 .. 2 of a pixel become `value` (const) or the pixel's three N(0, 1) values
// (pixel), the pad channels zero -- what the normalise kernels leave there. Nothing outside a box is read or written,
// and nothing inside one is read.
//
// Work follows the erased area, not the batch: the grid is (B N, ER_SPLIT) blocks, block (i, s) owns rows s, s +
// ER_SPLIT, .. of box i, and a block whose box is empty or has no such row returns after four uniform loads. The box
// is block-uniform, so every branch on it is uniform. A box is clipped to the image before use, so no value of it
// writes out of bounds.
//
// Stores are the widest the pixel allows: a pixel of 16 bytes (bf16 CP 8, fp32 CP 4) is one 16-byte store, one of 32
// (fp32 CP 8) two. A pixel of 8 bytes (bf16 CP 4) shares a 16-byte slot with a neighbour: a row of the box is walked
// in aligned slots, a slot with both pixels inside the box is one 16-byte store, and a box that begins or ends at an
// odd pixel has an 8-byte store at that end. Which pixels pair is the parity of the pixel's index in the whole tensor
// (a sample of odd H W shifts it) plus that of the base pointer in 8-byte units.
//
// The noise of pixel q = y W + x of sample b is Philox4x32-10(counter (q, 0, 0, 0), key keys[b]) through Box-Muller
// in fp32 with the precise logf / sinf / cosf: u and v are exact in fp32, the rounded 2 pi v is off by under 6e-7 and
// the radius is at most 5.77, which with a few ulp of the three functions stays under 5e-6 of the float64 value. It
// depends on (key, q) alone, so overlapping boxes of a sample write equal values in any block order.
// Sample offsets are 64-bit (2731 x 224^2 x 8 bf16 passes 2^31 bytes); a pixel's index in its sample fits 32 bits.

#include "common.h"

#include <algorithm>

namespace {

constexpr int ER_THREADS = 256;
constexpr int ER_SPLIT = 4;  // row-interleaved blocks per box

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t r[4]) {
    uint32_t c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
        const uint32_t h1 = __umulhi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// the three channels of pixel q under key (k0, k1)
__device__ __forceinline__ void er_normals(uint32_t q, uint32_t k0, uint32_t k1, float n[3]) {
    uint32_t r[4];
    philox4x32_10(q, k0, k1, r);
    const float u0 = (float)((r[0] >> 8) + 1u) * 0x1p-24f, v0 = (float)(r[1] >> 8) * 0x1p-24f;
    const float u1 = (float)((r[2] >> 8) + 1u) * 0x1p-24f, v1 = (float)(r[3] >> 8) * 0x1p-24f;
    const float rad0 = sqrtf(-2.f * logf(u0)), rad1 = sqrtf(-2.f * logf(u1));
    const float a0 = 6.28318530717958647692f * v0, a1 = 6.28318530717958647692f * v1;
    n[0] = rad0 * cosf(a0);
    n[1] = rad0 * sinf(a0);
    n[2] = rad1 * cosf(a1);
}

// the first 8 bytes (bf16) or 16 bytes (fp32) of a pixel: channels 0 .. 2 and the pad channel 3
template <typename T> struct ErPix;
template <> struct ErPix<bf16_t> {
    typedef u32x2 type;
    static __device__ __forceinline__ type make(const float n[3]) { return type{pack_bf2(n[0], n[1]), pack_bf2(n[2], 0.f)}; }
};
template <> struct ErPix<float> {
    typedef u32x4 type;
    static __device__ __forceinline__ type make(const float n[3]) {
        return type{__float_as_uint(n[0]), __float_as_uint(n[1]), __float_as_uint(n[2]), 0u};
    }
};

template <typename T, int CP, bool PIXEL>
__global__ __launch_bounds__(ER_THREADS) void erase_boxes_kernel(T* __restrict__ x, const int* __restrict__ boxes,
                                                                 const int* __restrict__ keys, int NB, int H, int W,
                                                                 float value, uint32_t odd) {
    typedef typename ErPix<T>::type P;
    constexpr bool PAIRS = CP * sizeof(T) == 8;  // two pixels to a 16-byte slot
    const uint32_t bi = blockIdx.x, part = blockIdx.y;
    const int* bx = boxes + 4 * (size_t)bi;
    const int top = bx[0], left = bx[1], bh = bx[2], bw = bx[3];
    if (bh <= 0 || bw <= 0) return;
    // clipped to the image (the draws never need it)
    const int y0 = max(top, 0), y1 = (int)min((long)top + bh, (long)H);
    const int x0 = max(left, 0), x1 = (int)min((long)left + bw, (long)W);
    if (y1 <= y0 || x1 <= x0) return;
    const uint32_t h = (uint32_t)(y1 - y0), w = (uint32_t)(x1 - x0);
    if (part >= h) return;
    const uint32_t nr = (h - part + ER_SPLIT - 1) / ER_SPLIT;  // rows y0 + part + ER_SPLIT j, j < nr
    const uint32_t b = bi / (uint32_t)NB;
    uint32_t k0 = 0u, k1 = 0u;
    if (PIXEL) k0 = (uint32_t)keys[2 * (size_t)b], k1 = (uint32_t)keys[2 * (size_t)b + 1];
    const size_t pix_b = (size_t)b * (size_t)H * (size_t)W;  // the sample's first pixel in the tensor
    float c[3] = {value, value, value};
    const P cp = ErPix<T>::make(c);
    const uint32_t sl = PAIRS ? w / 2 + 1 : w;  // slots a row can need
    const uint32_t items = nr * sl;             // < 2^31: the launcher checks H W
    for (uint32_t i = threadIdx.x; i < items; i += ER_THREADS) {
        const uint32_t j = i / sl, k = i - j * sl;
        const uint32_t y = (uint32_t)y0 + part + ER_SPLIT * j;
        const uint32_t qrow = y * (uint32_t)W;
        T* row = x + (pix_b + qrow) * CP;
        if (PAIRS) {
            // slot k of the row: pixels px, px + 1 with px's index in the tensor (from the 16-byte boundary) even
            const uint32_t par = (uint32_t)((pix_b + qrow + (uint32_t)x0 + odd) & 1);
            const int px = x0 - (int)par + 2 * (int)k;
            const bool in_a = px >= x0 && px < x1, in_b = px + 1 < x1;
            if (!in_a && !in_b) continue;
            P a = cp, bq = cp;
            if (PIXEL) {
                float n[3];
                if (in_a) { er_normals(qrow + (uint32_t)px, k0, k1, n); a = ErPix<T>::make(n); }
                if (in_b) { er_normals(qrow + (uint32_t)px + 1u, k0, k1, n); bq = ErPix<T>::make(n); }
            }
            if (in_a && in_b) {
                const u32x4 v = {a[0], a[1], bq[0], bq[1]};
                *reinterpret_cast<u32x4*>(row + (size_t)px * CP) = v;
            } else if (in_a) {
                *reinterpret_cast<P*>(row + (size_t)px * CP) = a;
            } else {
                *reinterpret_cast<P*>(row + (size_t)(px + 1) * CP) = bq;
            }
        } else {
            const uint32_t px = (uint32_t)x0 + k;
            P a = cp;
            if (PIXEL) {
                float n[3];
                er_normals(qrow + px, k0, k1, n);
                a = ErPix<T>::make(n);
            }
            T* p = row + (size_t)px * CP;
            if (std::is_same<T, float>::value) {
                *reinterpret_cast<P*>(p) = a;
                if (CP == 8) *reinterpret_cast<u32x4*>(p + 4) = u32x4{0u, 0u, 0u, 0u};
            } else {  // bf16, CP 8: the pixel is one 16-byte store
                const u32x4 v = {a[0], a[1], 0u, 0u};
                *reinterpret_cast<u32x4*>(p) = v;
            }
        }
    }
}

}  // namespace

// Random Erasing in place (erase_boxes_kernel): x bf16 (is_f32 0) or fp32 (1) NHWC [B][H][W][Cp], Cp 4 or 8; boxes
// int32 [B][N][4], keys int32 [B][2] (read in pixel mode only) on the device
IMK_EXPORT int imk_erase_boxes(void* x, const int* boxes, const int* keys, int B, int N, int H, int W, int Cp,
                               int is_f32, int pixel, float value, void* stream) {
    if (B < 0 || N < 1 || H < 1 || W < 1 || !x || !boxes || (pixel && !keys)) return -1;
    if (Cp != 4 && Cp != 8) return -100;
    if ((long)H * W >= (1L << 31)) return -101;  // a pixel's index in its sample: 32 bits
    if ((long)B * N >= (1L << 31)) return -101;
    if (B == 0) return 0;
    const size_t pb = (size_t)Cp * (is_f32 ? 4 : 2);  // a pixel's bytes
    if ((size_t)(uintptr_t)x % (pb < 16 ? pb : 16)) return -100;
    const uint32_t odd = (uint32_t)(((uintptr_t)x >> 3) & 1);
    const dim3 g((uint32_t)((long)B * N), (uint32_t)std::min(H, ER_SPLIT)), bl(ER_THREADS);
#define IMK_ERASE(T, CP, PX)                                                                                      \
    hipLaunchKernelGGL((erase_boxes_kernel<T, CP, PX>), g, bl, 0, (hipStream_t)stream, (T*)x, boxes, keys, N, H, W, \
                       value, odd)
    if (is_f32) {
        if (Cp == 4) { if (pixel) IMK_ERASE(float, 4, true); else IMK_ERASE(float, 4, false); }
        else { if (pixel) IMK_ERASE(float, 8, true); else IMK_ERASE(float, 8, false); }
    } else {
        if (Cp == 4) { if (pixel) IMK_ERASE(bf16_t, 4, true); else IMK_ERASE(bf16_t, 4, false); }
        else { if (pixel) IMK_ERASE(bf16_t, 8, true); else IMK_ERASE(bf16_t, 8, false); }
    }
#undef IMK_ERASE
    IMK_CHECK_LAUNCH();
    return 0;
}
