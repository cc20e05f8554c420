// RandAugment (Cubuk et al.) on the uint8 NHWC batch, ahead of the crop + resize + normalise kernels (data/randaug.py
// holds the definition: the op table, the integer rules and the torch backend these kernels equal bit for bit).
//
// A stage of L layers is L launch pairs over ping-pong buffers: the geometric ops gather, so a layer's input must be
// whole before the layer runs, and nothing is updated in place. Per layer
//   randaug_stats_kernel  the R, G, B and gray histograms of every image whose op needs a statistic of the whole
//                         image (Contrast: the mean gray; AutoContrast: the extremes; Equalize: the CDF) -- LDS
//                         histograms, integer atomics only, so the counts do not depend on the order of arrival;
//   randaug_apply_kernel  one block = one strip of ONE image, so the op is uniform over the block and the branch on
//                         it costs nothing. The sample's row (op, a0 .. a6) of params int32 [B][L][8] is read through
//                         uniform loads.
// No float arithmetic anywhere. An image is H W 3 bytes, which need be no multiple of 4: a lane moves 4 pixels as one
// 12-byte access at whatever alignment the image has (gfx950 global memory takes unaligned dword accesses; 64 lanes
// x 12 B are 768 contiguous bytes), the last 1 .. 3 pixels of an image byte by byte. No access leaves its image's
// H W 3 bytes. Image bases are 64-bit (4096 x 448^2 x 3 bytes are 2.47 GB); offsets inside an image are 32-bit.

#include "common.h"

namespace {

enum RaOp {
    RA_IDENTITY = 0, RA_SHEAR_X, RA_SHEAR_Y, RA_TRANSLATE_X, RA_TRANSLATE_Y, RA_ROTATE, RA_BRIGHTNESS, RA_COLOR,
    RA_CONTRAST, RA_SHARPNESS, RA_POSTERIZE, RA_SOLARIZE, RA_AUTOCONTRAST, RA_EQUALIZE
};

constexpr int RA_THREADS = 256;
constexpr int RA_APPLY_U = 4;    // 4-pixel groups per thread of an apply strip: 4096 pixels, 12 KB in, 12 KB out
constexpr int RA_STATS_U = 16;   // and of a statistics strip: 16384 pixels behind each block's 1024 global atomics

struct Px4 {
    uint32_t w[3];  // 4 RGB pixels: byte j of the 12 is channel j % 3 of pixel j / 3
};

__device__ __forceinline__ uint32_t px_byte(const Px4& p, int j) { return (p.w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

__device__ __forceinline__ uint32_t w_byte(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

__device__ __forceinline__ void px_set(Px4& p, int j, uint32_t v) { p.w[j >> 2] |= (v & 0xFFu) << (8 * (j & 3)); }

// the `np` (1 .. 4) pixels from byte offset `off` of the image at `img`; the bytes of absent pixels read as 0
__device__ __forceinline__ Px4 px_load(const uint8_t* img, uint32_t off, int np) {
    Px4 p = {{0u, 0u, 0u}};
    if (np == 4) {
        __builtin_memcpy(p.w, img + off, 12);
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j)
            if (j < 3 * np) px_set(p, j, img[off + j]);
    }
    return p;
}

__device__ __forceinline__ void px_store(uint8_t* img, uint32_t off, int np, const Px4& p) {
    if (np == 4) {
        __builtin_memcpy(img + off, p.w, 12);
    } else {
#pragma unroll
        for (int j = 0; j < 9; ++j)
            if (j < 3 * np) img[off + j] = (uint8_t)px_byte(p, j);
    }
}

__device__ __forceinline__ int ra_gray(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

__device__ __forceinline__ int ra_clamp8(int v) { return min(max(v, 0), 255); }

// clamp((F v + (256 - F) d + 128) >> 8, 0, 255): F may exceed 256 (the second weight negative), the shift arithmetic.
// Clamped to 16 bits BEFORE the shift, which gives the same value: written as shift-then-clamp, pairs of blends
// compile to gfx950's packing shift (v_ashr_pk_u8_i32), whose result the compiler ORs into the pixel word as if its
// upper half were zero; on the MI355X the upper half kept the bits of the sum, and every negative sum (F > 256)
// set the two bytes above it to 255.
__device__ __forceinline__ int ra_blend(int v, int d, int F) {
    return min(max(F * v + (256 - F) * d + 128, 0), 0xFFFF) >> 8;
}

// the same in 64 bits, for the tables: any F of a params row is defined (data/randaug.py computes in int64)
__device__ __forceinline__ int ra_blend64(int v, long d, long F) {
    const long r = (F * v + (256 - F) * d + 128) >> 8;
    return (int)(r < 0 ? 0 : r > 255 ? 255 : r);
}

__device__ __forceinline__ bool ra_needs_stats(int op) {
    return op == RA_CONTRAST || op == RA_AUTOCONTRAST || op == RA_EQUALIZE;
}

// ------------------------------------------------------------------ statistics
// hist uint32 [B][4][256] (R, G, B, gray), zeroed on the stream ahead of the launch. grid (strips, B).
__global__ __launch_bounds__(RA_THREADS) void randaug_stats_kernel(const uint8_t* __restrict__ src,
                                                                   const int* __restrict__ params,
                                                                   uint32_t* __restrict__ hist, uint32_t npix, int L,
                                                                   int layer) {
    __shared__ uint32_t h[4 * 256];
    const uint32_t b = blockIdx.y;
    const int op = params[((size_t)b * L + layer) * 8];
    if (!ra_needs_stats(op)) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * 256; i += RA_THREADS) h[i] = 0u;
    __syncthreads();
    const uint8_t* img = src + (size_t)b * npix * 3;
    const uint32_t ngroups = (npix + 3) >> 2;
    const uint32_t g0 = blockIdx.x * (uint32_t)(RA_THREADS * RA_STATS_U);
#pragma unroll 2
    for (int u = 0; u < RA_STATS_U; ++u) {
        const uint32_t g = g0 + (uint32_t)u * RA_THREADS + tid;
        if (g >= ngroups) break;
        const int np = (int)min(4u, npix - 4u * g);
        const Px4 p = px_load(img, 12u * g, np);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < np) {
                const int r = px_byte(p, 3 * k), gr = px_byte(p, 3 * k + 1), bl = px_byte(p, 3 * k + 2);
                atomicAdd(&h[r], 1u);
                atomicAdd(&h[256 + gr], 1u);
                atomicAdd(&h[512 + bl], 1u);
                atomicAdd(&h[768 + ra_gray(r, gr, bl)], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = hist + (size_t)b * 1024;
    for (int i = tid; i < 4 * 256; i += RA_THREADS)
        if (h[i]) atomicAdd(&out[i], h[i]);
}

// ------------------------------------------------------------------ apply
// exclusive prefix sum of one value per thread over the block's 256 threads; `ws` 4 words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* ws) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();  // (ws may still be read from the call before)
    if (lane == 63) ws[w] = x;
    __syncthreads();
    uint32_t off = 0;
    for (int i = 0; i < w; ++i) off += ws[i];
    return off + x - v;
}

// the per-channel table of a table op into lut[3][256]; false: the op is no table op. Every thread of the block calls
// it (it holds barriers); thread t forms entry t of each channel.
__device__ __forceinline__ bool ra_build_lut(uint8_t* lut, uint32_t* red, int op, int a0, const uint32_t* __restrict__ hb,
                                             uint32_t npix) {
    const int v = threadIdx.x;  // RA_THREADS == 256: one table entry per thread
    switch (op) {
    case RA_IDENTITY:
    case RA_BRIGHTNESS:
    case RA_POSTERIZE:
    case RA_SOLARIZE: {
        int o = v;
        if (op == RA_BRIGHTNESS) o = ra_blend64(v, 0, a0);
        if (op == RA_POSTERIZE) o = v & a0 & 0xFF;
        if (op == RA_SOLARIZE) o = v >= a0 ? 255 - v : v;
        lut[v] = lut[256 + v] = lut[512 + v] = (uint8_t)o;
        break;
    }
    case RA_CONTRAST: {
        // d = (sum of gray + n / 2) / n from the gray histogram: the sum of v hist[v] in two limbs
        const uint32_t c = hb[768 + v];
        const uint64_t t = (uint64_t)c * (uint32_t)v;
        if (v < 2) red[4 + v] = 0u;
        __syncthreads();
        // 24-bit limbs: 256 terms of at most 24 bits (resp. 2^31 * 255 >> 24 < 2^15) cannot overflow 32 bits
        atomicAdd(&red[4], (uint32_t)(t & 0xFFFFFFu));
        atomicAdd(&red[5], (uint32_t)(t >> 24));
        __syncthreads();
        const uint64_t sum = (uint64_t)red[4] + ((uint64_t)red[5] << 24);
        const long d = (long)((sum + npix / 2) / npix);
        lut[v] = lut[256 + v] = lut[512 + v] = (uint8_t)ra_blend64(v, d, a0);
        break;
    }
    case RA_AUTOCONTRAST: {
        if (v < 3) {
            red[4 + v] = 255u;  // lo
            red[8 + v] = 0u;    // hi
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            if (hb[256 * c + v]) {
                atomicMin(&red[4 + c], (uint32_t)v);
                atomicMax(&red[8 + c], (uint32_t)v);
            }
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            const int lo = (int)red[4 + c], hi = (int)red[8 + c], span = hi - lo;
            int o = v;
            if (span > 0) o = ra_clamp8((max(v - lo, 0) * 255 + span / 2) / span);
            lut[256 * c + v] = (uint8_t)o;
        }
        break;
    }
    case RA_EQUALIZE: {
        if (v < 3) red[8 + v] = 0u;  // the highest non-empty bin
        __syncthreads();
        uint32_t cnt[3];
        for (int c = 0; c < 3; ++c) {
            cnt[c] = hb[256 * c + v];
            if (cnt[c]) atomicMax(&red[8 + c], (uint32_t)v);
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            const uint32_t excl = block_excl_scan(cnt[c], red);
            const uint32_t last = hb[256 * c + red[8 + c]];
            const uint32_t step = (npix - min(last, npix)) / 255u;
            int o = v;
            if (step) o = (int)min(255u, (excl + step / 2) / step);
            lut[256 * c + v] = (uint8_t)o;
        }
        break;
    }
    default:
        return false;
    }
    __syncthreads();
    return true;
}

// pixel (y, x)'s three channels of the sharpness kernel's smoothed image d: (3x3 sum + 4 centre + 6) / 13 inside,
// the pixel itself on the image's border
__device__ __forceinline__ void ra_sharp_px(const uint8_t* img, int H, int W, int y, int x, int F, int out[3]) {
    const uint32_t c = ((uint32_t)y * W + x) * 3u;
    const bool inner = y > 0 && y < H - 1 && x > 0 && x < W - 1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int v = img[c + ch];
        int d = v;
        if (inner) {
            int s = 4 * v + 6;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) s += img[c + ch + (uint32_t)((dy * W + dx) * 3)];
            d = s / 13;
        }
        out[ch] = ra_blend(v, d, F);
    }
}

// grid (strips, B): the block's strip is RA_THREADS * RA_APPLY_U groups of 4 pixels of image blockIdx.y
__global__ __launch_bounds__(RA_THREADS) void randaug_apply_kernel(const uint8_t* __restrict__ src,
                                                                   uint8_t* __restrict__ dst,
                                                                   const int* __restrict__ params,
                                                                   const uint32_t* __restrict__ hist, int H, int W,
                                                                   int L, int layer, int fill) {
    __shared__ uint8_t lut[3 * 256];
    __shared__ uint32_t red[12];
    const uint32_t b = blockIdx.y;
    const int* pr = params + ((size_t)b * L + layer) * 8;
    const int op = pr[0], a0 = pr[1];
    const uint32_t npix = (uint32_t)H * (uint32_t)W;
    const uint8_t* img = src + (size_t)b * npix * 3;
    uint8_t* out = dst + (size_t)b * npix * 3;
    const int tid = threadIdx.x;
    const uint32_t ngroups = (npix + 3) >> 2;
    const uint32_t g0 = blockIdx.x * (uint32_t)(RA_THREADS * RA_APPLY_U);

    if (ra_build_lut(lut, red, op, a0, hist + (size_t)b * 1024, npix)) {
        // byte j of a group is channel j % 3: byte j of word k looks up table (4 k + j) % 3 = (k + j) % 3
#pragma unroll
        for (int u = 0; u < RA_APPLY_U; ++u) {
            const uint32_t g = g0 + (uint32_t)u * RA_THREADS + tid;
            if (g >= ngroups) break;
            const int np = (int)min(4u, npix - 4u * g);
            const Px4 p = px_load(img, 12u * g, np);
            Px4 q = {{0u, 0u, 0u}};
#pragma unroll
            for (int j = 0; j < 12; ++j) px_set(q, j, lut[256 * (j % 3) + px_byte(p, j)]);
            px_store(out, 12u * g, np, q);
        }
        return;
    }

    if (op == RA_COLOR) {
#pragma unroll
        for (int u = 0; u < RA_APPLY_U; ++u) {
            const uint32_t g = g0 + (uint32_t)u * RA_THREADS + tid;
            if (g >= ngroups) break;
            const int np = (int)min(4u, npix - 4u * g);
            const Px4 p = px_load(img, 12u * g, np);
            Px4 q = {{0u, 0u, 0u}};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = px_byte(p, 3 * k), gr = px_byte(p, 3 * k + 1), bl = px_byte(p, 3 * k + 2);
                const int d = ra_gray(r, gr, bl);
                px_set(q, 3 * k, ra_blend(r, d, a0));
                px_set(q, 3 * k + 1, ra_blend(gr, d, a0));
                px_set(q, 3 * k + 2, ra_blend(bl, d, a0));
            }
            px_store(out, 12u * g, np, q);
        }
        return;
    }

    if (op == RA_SHARPNESS) {
        for (int u = 0; u < RA_APPLY_U; ++u) {
            const uint32_t g = g0 + (uint32_t)u * RA_THREADS + tid;
            if (g >= ngroups) break;
            const int np = (int)min(4u, npix - 4u * g);
            const uint32_t p0 = 4u * g;
            const int y = (int)(p0 / (uint32_t)W), x = (int)(p0 - (uint32_t)y * W);
            Px4 q = {{0u, 0u, 0u}};
            if (np == 4 && y > 0 && y < H - 1 && x > 0 && x + 4 < W) {
                // the four pixels and their windows lie inside one row's interior: three 18-byte rows (x - 1 .. x + 4)
                uint32_t rows[3][5] = {};
                const uint32_t c = ((uint32_t)y * W + (x - 1)) * 3u;
                __builtin_memcpy(rows[0], img + c - 3u * W, 18);
                __builtin_memcpy(rows[1], img + c, 18);
                __builtin_memcpy(rows[2], img + c + 3u * W, 18);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int v = (int)w_byte(rows[1], 3 * (k + 1) + ch);
                        int s = 4 * v + 6;
#pragma unroll
                        for (int r = 0; r < 3; ++r)
                            s += (int)(w_byte(rows[r], 3 * k + ch) + w_byte(rows[r], 3 * (k + 1) + ch) +
                                       w_byte(rows[r], 3 * (k + 2) + ch));
                        px_set(q, 3 * k + ch, ra_blend(v, s / 13, a0));
                    }
                }
            } else {
                int yy = y, xx = x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < np) {
                        int o[3];
                        ra_sharp_px(img, H, W, yy, xx, a0, o);
                        px_set(q, 3 * k, o[0]);
                        px_set(q, 3 * k + 1, o[1]);
                        px_set(q, 3 * k + 2, o[2]);
                        if (++xx == W) {
                            xx = 0;
                            ++yy;
                        }
                    }
                }
            }
            px_store(out, 12u * g, np, q);
        }
        return;
    }

    if (op >= RA_SHEAR_X && op <= RA_ROTATE) {
        // the inverse map in doubled, centred pixel units, 16 fraction bits: (a0 .. a5) = (m00 m01 m02 m10 m11 m12)
        const long m00 = pr[1], m01 = pr[2], m02 = pr[3], m10 = pr[4], m11 = pr[5], m12 = pr[6];
        const long cx = m02 + ((long)W << 16), cy = m12 + ((long)H << 16);
        const uint32_t fb = (uint32_t)fill & 0xFFu;
        for (int u = 0; u < RA_APPLY_U; ++u) {
            const uint32_t g = g0 + (uint32_t)u * RA_THREADS + tid;
            if (g >= ngroups) break;
            const int np = (int)min(4u, npix - 4u * g);
            const uint32_t p0 = 4u * g;
            int y = (int)(p0 / (uint32_t)W), x = (int)(p0 - (uint32_t)y * W);
            Px4 q = {{0u, 0u, 0u}};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < np) {
                    const long X = 2L * x - (W - 1), Y = 2L * y - (H - 1);
                    const long sx = (m00 * X + m01 * Y + cx) >> 17, sy = (m10 * X + m11 * Y + cy) >> 17;
                    uint32_t r = fb, gr = fb, bl = fb;
                    if (sx >= 0 && sx < W && sy >= 0 && sy < H) {
                        const uint32_t s = ((uint32_t)sy * W + (uint32_t)sx) * 3u;
                        r = img[s];
                        gr = img[s + 1];
                        bl = img[s + 2];
                    }
                    px_set(q, 3 * k, r);
                    px_set(q, 3 * k + 1, gr);
                    px_set(q, 3 * k + 2, bl);
                    if (++x == W) {
                        x = 0;
                        ++y;
                    }
                }
            }
            px_store(out, 12u * g, np, q);
        }
        return;
    }

    // an op id outside the table: the image as it is
    for (int u = 0; u < RA_APPLY_U; ++u) {
        const uint32_t g = g0 + (uint32_t)u * RA_THREADS + tid;
        if (g >= ngroups) break;
        const int np = (int)min(4u, npix - 4u * g);
        px_store(out, 12u * g, np, px_load(img, 12u * g, np));
    }
}

int ra_check(const void* src, const int* params, int B, int H, int W, int L, int layer) {
    if (B < 0 || H < 1 || W < 1 || L < 1 || layer < 0 || layer >= L || !src || !params) return -1;
    if ((long)H * W * 3 >= (1L << 31)) return -101;  // a byte's offset in its image: 32 bits
    if (B > 65535) return -102;                     // blockIdx.y
    return 0;
}

}  // namespace

// The histograms of layer `layer`'s input: hist uint32 [B][4][256] (R, G, B, gray), cleared here on the stream;
// images whose op of that layer needs no statistic keep zeros. src uint8 [B][H][W][3], params int32 [B][L][8].
IMK_EXPORT int imk_randaug_stats(const void* src, const int* params, void* hist, int B, int H, int W, int L, int layer,
                                 void* stream) {
    const int rc = ra_check(src, params, B, H, W, L, layer);
    if (rc || !hist) return rc ? rc : -1;
    if (B == 0) return 0;
    if (hipMemsetAsync(hist, 0, (size_t)B * 1024 * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return -2;
    const uint32_t npix = (uint32_t)H * W, ngroups = (npix + 3) / 4;
    const uint32_t per = RA_THREADS * RA_STATS_U;
    const dim3 g((ngroups + per - 1) / per, (uint32_t)B), bl(RA_THREADS);
    hipLaunchKernelGGL(randaug_stats_kernel, g, bl, 0, (hipStream_t)stream, (const uint8_t*)src, params,
                       (uint32_t*)hist, npix, L, layer);
    IMK_CHECK_LAUNCH();
    return 0;
}

// One layer: dst = layer `layer` of params applied to src (dst != src, neither overlapping the other), hist as
// imk_randaug_stats left it for this layer and this src, fill the colour (0 .. 255) of pixels an affine op maps from
// outside the image.
IMK_EXPORT int imk_randaug_apply(const void* src, void* dst, const int* params, const void* hist, int B, int H, int W,
                                 int L, int layer, int fill, void* stream) {
    const int rc = ra_check(src, params, B, H, W, L, layer);
    if (rc || !dst || !hist || dst == src) return rc ? rc : -1;
    if (B == 0) return 0;
    const uint32_t npix = (uint32_t)H * W, ngroups = (npix + 3) / 4;
    const uint32_t per = RA_THREADS * RA_APPLY_U;
    const dim3 g((ngroups + per - 1) / per, (uint32_t)B), bl(RA_THREADS);
    hipLaunchKernelGGL(randaug_apply_kernel, g, bl, 0, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, params,
                       (const uint32_t*)hist, H, W, L, layer, fill);
    IMK_CHECK_LAUNCH();
    return 0;
}
