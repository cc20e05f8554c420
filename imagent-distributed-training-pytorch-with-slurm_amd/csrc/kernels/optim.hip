// LARS (layer-wise adaptive rate scaling, You et al. 2017) over the flat
// parameter arena, for the large-batch configuration (BASELINE.json: global
// batch 8192). Two launches per step over a per-tensor descriptor table:
//   1. per-tensor ||w||^2 and ||g||^2 (block reduce, one atomic per block)
//   2. the update, blockIdx.y = tensor:
//        trust = eta * ||w|| / (||g|| + wd * ||w||)   (adapted tensors; 1 else)
//        d = g + wd * w ;  v = mu * v + lr * trust * d ;  w -= v
//      plus the bf16 compute shadow, like the fused SGD kernel (misc.hip).
// BatchNorm weights/biases and the fc bias are conventionally neither decayed
// nor adapted (`adapt` = 0 in their descriptors).

#include "common.h"

struct LarsDesc {
    float* p;
    const float* g;
    float* buf;
    bf16_t* shadow;  // may be null
    long n;
    int adapt;       // 1: LARS trust ratio + weight decay; 0: plain momentum SGD, no decay
    int pad;
};

namespace {

__global__ __launch_bounds__(256) void lars_norms_kernel(const LarsDesc* __restrict__ d, float* __restrict__ norms,
                                                         int T, float gs) {
    const LarsDesc q = d[blockIdx.y];
    float sw = 0.f, sg = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < q.n; i += (long)gridDim.x * 256) {
        const float w = q.p[i], g = q.g[i] * gs;
        sw += w * w;
        sg += g * g;
    }
    __shared__ float red[2][4];
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sw;
        red[1][threadIdx.x >> 6] = sg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(norms + blockIdx.y, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        atomicAdd(norms + T + blockIdx.y, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(256) void lars_update_kernel(const LarsDesc* __restrict__ d,
                                                          const float* __restrict__ norms, int T, float lr,
                                                          float mu, float wd, float eta, float gs, int first) {
    const LarsDesc q = d[blockIdx.y];
    float trust = 1.f, wdt = 0.f;
    if (q.adapt) {
        wdt = wd;
        const float wn = sqrtf(norms[blockIdx.y]), gn = sqrtf(norms[T + blockIdx.y]);
        if (wn > 0.f && gn > 0.f) trust = eta * wn / (gn + wd * wn);
    }
    const float step = lr * trust;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < q.n; i += (long)gridDim.x * 256) {
        const float w = q.p[i];
        const float dd = q.g[i] * gs + wdt * w;
        const float v = first ? step * dd : mu * q.buf[i] + step * dd;
        q.buf[i] = v;
        const float nw = w - v;
        q.p[i] = nw;
        if (q.shadow) q.shadow[i] = f2bf(nw);
    }
}

}  // namespace

// descs: device array of T LarsDesc; norms: device float[2*T] scratch (zeroed here)
IMK_EXPORT int imk_lars_step(const void* descs, int T, long max_n, float* norms, float lr, float mu, float wd,
                             float eta, float gs, int first, void* stream) {
    if (T <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(norms, 0, sizeof(float) * 2 * T, st) != hipSuccess) return -1;
    long bx = (max_n + 1023) / 1024;
    if (bx > 64) bx = 64;
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(lars_norms_kernel, dim3((int)bx, T), dim3(256), 0, st, (const LarsDesc*)descs, norms, T, gs);
    IMK_CHECK_LAUNCH();
    hipLaunchKernelGGL(lars_update_kernel, dim3((int)bx, T), dim3(256), 0, st, (const LarsDesc*)descs,
                       (const float*)norms, T, lr, mu, wd, eta, gs, first);
    IMK_CHECK_LAUNCH();
    return 0;
}

IMK_EXPORT int imk_lars_desc_size() { return (int)sizeof(LarsDesc); }

// ------------------------------------------------------------------------------------------------------------
// The weight average's side of the model buffers (--model-ema, train/ema.py): every float buffer (BatchNorm
// running_mean / running_var) has its average in one flat fp32 side buffer. One launch over a per-tensor
// descriptor table, blockIdx.y = tensor, serves all of them:
//   mode 0 (EMA):   flat[off + i] += omd * (buf[i] - flat[off + i])
//   mode 1 (swap):  buf[i] <-> flat[off + i], in place: the running-statistics and eval-affine descriptor tables
//                   and the cross-rank buffer broadcast hold the buffers' own storage, so no pointer may move.
struct EmaBufDesc {
    float* buf;  // the model's buffer
    long off;    // its offset in the flat side buffer, in floats
    long n;
};

namespace {

template <bool SWAP>
__global__ __launch_bounds__(256) void ema_bufs_kernel(const EmaBufDesc* __restrict__ d, float* __restrict__ flat,
                                                       float omd) {
    const EmaBufDesc q = d[blockIdx.y];
    float* __restrict__ a = flat + q.off;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < q.n; i += (long)gridDim.x * 256) {
        const float b = q.buf[i], e = a[i];
        if constexpr (SWAP) {
            q.buf[i] = e;
            a[i] = b;
        } else {
            a[i] = e + omd * (b - e);
        }
    }
}

}  // namespace

// descs: device array of T EmaBufDesc; flat: the side buffer they index; mode 0: EMA with omd, 1: swap
IMK_EXPORT int imk_ema_bufs(const void* descs, int T, long max_n, float* flat, float omd, int mode, void* stream) {
    if (T <= 0) return 0;
    if (T > 65535 || (mode != 0 && mode != 1)) return -100;
    long bx = (max_n + 255) / 256;
    if (bx > 64) bx = 64;
    if (bx < 1) bx = 1;
    if (mode == 1)
        hipLaunchKernelGGL(ema_bufs_kernel<true>, dim3((int)bx, T), dim3(256), 0, (hipStream_t)stream,
                           (const EmaBufDesc*)descs, flat, omd);
    else
        hipLaunchKernelGGL(ema_bufs_kernel<false>, dim3((int)bx, T), dim3(256), 0, (hipStream_t)stream,
                           (const EmaBufDesc*)descs, flat, omd);
    IMK_CHECK_LAUNCH();
    return 0;
}

IMK_EXPORT int imk_ema_bufdesc_size() { return (int)sizeof(EmaBufDesc); }

// ------------------------------------------------------------------------------------------------------------
// Adam / AdamW (torch.optim.Adam / AdamW math, [torch] optim/adam.py _single_tensor_adam) as ONE launch over the flat
// arena, alignment padding included (all zeros, and 0 / (0 + eps) = 0 keeps it zero), shaped like sgd_kernel
// (misc.hip): f32x4 body, scalar tail, packed bf16 shadow store. Per element, fp32:
//   L2 form (decoupled 0):  g' = g*gs + wd*p          decoupled (1):  g' = g*gs ; p *= lr_wd  (= 1 - lr*wd)
//   m += omb1*(g' - m) ; v = beta2*v + omb2*g'^2 ; p -= step_size * (m / (sqrtf(v)*rbc2 + eps)) ; shadow = bf16(p)
// step_size = lr / (1 - beta1^t), rbc2 = 1 / sqrt(1 - beta2^t), omb = 1 - beta: formed in double on the host and
// rounded once to fp32 (train/optim.py). All four streams are loaded at the top of the iteration (late loads in a
// four-stream kernel: profiles/model_ema.md). g is read only.
namespace {

struct AdamArgs {
    float step_size, rbc2, eps, beta2, omb1, omb2, wd, lr_wd, gs;
    int decoupled;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamArgs& a) {
    float gg = g * a.gs;
    if (a.decoupled) p *= a.lr_wd;
    else gg += a.wd * p;
    m += a.omb1 * (gg - m);
    v = a.beta2 * v + a.omb2 * (gg * gg);
    p -= a.step_size * (m / (sqrtf(v) * a.rbc2 + a.eps));
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16_t* __restrict__ shadow, long n, AdamArgs a) {
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4 + (n % 4 ? 1 : 0); i += (long)gridDim.x * 256) {
        if (i < n4) {
            f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
            const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
            f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
            f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pe = pv[j], me = mv[j], ve = vv[j];
                adam_elem(pe, gv[j], me, ve, a);
                pv[j] = pe;
                mv[j] = me;
                vv[j] = ve;
            }
            reinterpret_cast<f32x4*>(p)[i] = pv;
            reinterpret_cast<f32x4*>(m)[i] = mv;
            reinterpret_cast<f32x4*>(v)[i] = vv;
            if (shadow)
                reinterpret_cast<u32x2*>(shadow)[i] = u32x2{pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3])};
        } else {
            for (long e = n4 * 4; e < n; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam_elem(pe, g[e], me, ve, a);
                p[e] = pe;
                m[e] = me;
                v[e] = ve;
                if (shadow) shadow[e] = f2bf(pe);
            }
        }
    }
}

}  // namespace

// p, g, m, v: flat fp32 arenas of n floats, 16-B aligned; shadow: bf16 [n] or null
IMK_EXPORT int imk_adam_flat(float* p, const float* g, float* m, float* v, void* shadow, long n, float step_size,
                             float rbc2, float eps, float beta2, float omb1, float omb2, float wd, float lr_wd,
                             int decoupled, float gs, void* stream) {
    if (n <= 0) return 0;
    if (!p || !g || !m || !v) return -100;
    const AdamArgs a{step_size, rbc2, eps, beta2, omb1, omb2, wd, lr_wd, gs, decoupled};
    hipLaunchKernelGGL(adam_kernel, dim3(stream_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       (bf16_t*)shadow, n, a);
    IMK_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// LAMB (You et al. 2019; the update of apex FusedLAMB / timm Lamb with the usual no-decay filter) over the flat
// arena: a per-tensor descriptor table and, beside it, a chunk table -- (tensor, first element) per LAMB_CHUNK
// elements, a chunk never spanning two tensors -- so that every block has the same amount of work whatever the
// tensor's size (lars_*_kernel's (<= 64, T) grid gives a 64-element BatchNorm vector as many blocks as a
// 2.36 M-element conv). One block per chunk; every arena slice starts 256-B aligned and LAMB_CHUNK is a multiple of
// 4, so the body is f32x4 everywhere and only a tensor's last chunk has a scalar tail. Per step, no host sync:
//   memset of norms[2T + 1]
//   A (max_grad_norm > 0 only): norms[2T] = sum g^2 over the flat gradient arena
//   B: c = gn > max_grad_norm ? max_grad_norm / gn : 1, gn = gs * sqrtf(norms[2T])  (1 when clipping is off)
//      g' = g*(gs*c) ; m += omb1*(g' - m) ; v = beta2*v + omb2*g'^2 ; r = (m*c1) / (sqrtf(v)*c2 + eps) + wd_i*w
//      norms[i] += sum w^2 ; norms[T + i] += sum r^2      (wave, block, then one atomic pair per block)
//   C: trust = (adapt && wn > 0 && rn > 0) ? wn / rn : 1 ; r recomputed from the stored m, v and w ;
//      w -= (lr*trust)*r ; shadow = bf16(w)
// wd_i = wd for adapted tensors (more than one dimension), 0 for BatchNorm affine parameters and biases, which get
// no trust ratio either. The float-atomic sums make the trust ratios vary in their last bits from run to run, as
// LARS's do. g is read only.
struct LambDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    bf16_t* shadow;  // may be null
    long n;
    int adapt;       // 1: trust ratio + weight decay; 0: neither
    int pad;
};

namespace {

constexpr int LAMB_CHUNK = 4096;       // elements per chunk = per block
constexpr int LAMB_THREADS = 256;
constexpr int LAMB_TRIPS = LAMB_CHUNK / (4 * LAMB_THREADS);
constexpr int LAMB_GNORM_BLOCKS = 2048;  // grid cap of pass A
static_assert(LAMB_CHUNK % (4 * LAMB_THREADS) == 0, "whole f32x4 trips per chunk");

struct LambArgs {
    float lr, beta2, omb1, omb2, c1, c2, eps, wd, max_gn, gs;
};

// block sum of two per-thread values; the total in thread 0
__device__ __forceinline__ void block_sum2(float& a, float& b) {
    __shared__ float red[2][LAMB_THREADS / 64];
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0];
        b = red[1][0];
#pragma unroll
        for (int w = 1; w < LAMB_THREADS / 64; ++w) {
            a += red[0][w];
            b += red[1][w];
        }
    }
}

__global__ __launch_bounds__(LAMB_THREADS) void lamb_gnorm_kernel(const float* __restrict__ g, long n,
                                                                  float* __restrict__ out) {
    const long n4 = n / 4;
    float s = 0.f, unused = 0.f;
    for (long i = (long)blockIdx.x * LAMB_THREADS + threadIdx.x; i < n4 + (n % 4 ? 1 : 0);
         i += (long)gridDim.x * LAMB_THREADS) {
        if (i < n4) {
            const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) s += gv[j] * gv[j];
        } else {
            for (long e = n4 * 4; e < n; ++e) s += g[e] * g[e];
        }
    }
    block_sum2(s, unused);
    if (threadIdx.x == 0) atomicAdd(out, s);
}

__device__ __forceinline__ float lamb_r(float w, float m, float v, float wdt, const LambArgs& a) {
    return (m * a.c1) / (sqrtf(v) * a.c2 + a.eps) + wdt * w;
}

// chunks: nchunks x (tensor, first element), both long
template <bool APPLY>
__global__ __launch_bounds__(LAMB_THREADS) void lamb_kernel(const LambDesc* __restrict__ d,
                                                            const long* __restrict__ chunks,
                                                            float* __restrict__ norms, int T, LambArgs a) {
    const int ti = (int)chunks[2 * (long)blockIdx.x];
    const long first = chunks[2 * (long)blockIdx.x + 1];
    const LambDesc q = d[ti];
    const long left = q.n - first;
    const int len = (int)(left < LAMB_CHUNK ? left : LAMB_CHUNK);  // elements of this chunk
    const int nvec = len / 4, tail = len - nvec * 4;
    const float wdt = q.adapt ? a.wd : 0.f;
    float* __restrict__ P = q.p + first;
    float* __restrict__ M = q.m + first;
    float* __restrict__ V = q.v + first;
    if constexpr (APPLY) {
        float trust = 1.f;
        if (q.adapt) {
            const float wn = sqrtf(norms[ti]), rn = sqrtf(norms[T + ti]);
            if (wn > 0.f && rn > 0.f) trust = wn / rn;
        }
        const float step = a.lr * trust;
        bf16_t* __restrict__ S = q.shadow ? q.shadow + first : nullptr;
        f32x4 pv[LAMB_TRIPS], mv[LAMB_TRIPS], vv[LAMB_TRIPS];
#pragma unroll
        for (int t = 0; t < LAMB_TRIPS; ++t) {
            const int i = t * LAMB_THREADS + threadIdx.x;
            if (i < nvec) {
                pv[t] = reinterpret_cast<f32x4*>(P)[i];
                mv[t] = reinterpret_cast<const f32x4*>(M)[i];
                vv[t] = reinterpret_cast<const f32x4*>(V)[i];
            }
        }
#pragma unroll
        for (int t = 0; t < LAMB_TRIPS; ++t) {
            const int i = t * LAMB_THREADS + threadIdx.x;
            if (i < nvec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) pv[t][j] -= step * lamb_r(pv[t][j], mv[t][j], vv[t][j], wdt, a);
                reinterpret_cast<f32x4*>(P)[i] = pv[t];
                if (S)
                    reinterpret_cast<u32x2*>(S)[i] =
                        u32x2{pack_bf2(pv[t][0], pv[t][1]), pack_bf2(pv[t][2], pv[t][3])};
            }
        }
        if ((int)threadIdx.x < tail) {
            const int e = nvec * 4 + threadIdx.x;
            const float w = P[e], nw = w - step * lamb_r(w, M[e], V[e], wdt, a);
            P[e] = nw;
            if (S) S[e] = f2bf(nw);
        }
    } else {
        float gsc = a.gs;
        if (a.max_gn > 0.f) {
            const float gn = a.gs * sqrtf(norms[2 * T]);
            if (gn > a.max_gn) gsc = a.gs * (a.max_gn / gn);
        }
        const float* __restrict__ G = q.g + first;
        float sw = 0.f, sr = 0.f;
        auto elem = [&](float w, float g, float& m, float& v) {
            const float gg = g * gsc;
            m += a.omb1 * (gg - m);
            v = a.beta2 * v + a.omb2 * (gg * gg);
            const float r = lamb_r(w, m, v, wdt, a);
            sw += w * w;
            sr += r * r;
        };
        f32x4 pv[LAMB_TRIPS], gv[LAMB_TRIPS], mv[LAMB_TRIPS], vv[LAMB_TRIPS];
#pragma unroll
        for (int t = 0; t < LAMB_TRIPS; ++t) {
            const int i = t * LAMB_THREADS + threadIdx.x;
            if (i < nvec) {
                pv[t] = reinterpret_cast<const f32x4*>(P)[i];
                gv[t] = reinterpret_cast<const f32x4*>(G)[i];
                mv[t] = reinterpret_cast<f32x4*>(M)[i];
                vv[t] = reinterpret_cast<f32x4*>(V)[i];
            }
        }
#pragma unroll
        for (int t = 0; t < LAMB_TRIPS; ++t) {
            const int i = t * LAMB_THREADS + threadIdx.x;
            if (i < nvec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float me = mv[t][j], ve = vv[t][j];
                    elem(pv[t][j], gv[t][j], me, ve);
                    mv[t][j] = me;
                    vv[t][j] = ve;
                }
                reinterpret_cast<f32x4*>(M)[i] = mv[t];
                reinterpret_cast<f32x4*>(V)[i] = vv[t];
            }
        }
        if ((int)threadIdx.x < tail) {
            const int e = nvec * 4 + threadIdx.x;
            float me = M[e], ve = V[e];
            elem(P[e], G[e], me, ve);
            M[e] = me;
            V[e] = ve;
        }
        block_sum2(sw, sr);
        if (threadIdx.x == 0) {
            atomicAdd(norms + ti, sw);
            atomicAdd(norms + T + ti, sr);
        }
    }
}

}  // namespace

// descs: device array of T LambDesc; chunks: device long[nchunks][2] = (tensor, first element), LAMB_CHUNK elements
// each but a tensor's last; g_flat / n_flat: the whole gradient arena (pass A); norms: device float[2T + 1] scratch
// (zeroed here; left readable after the step: sum w^2 [T], sum r^2 [T], sum g^2)
IMK_EXPORT int imk_lamb_step(const void* descs, int T, const void* chunks, int nchunks, const float* g_flat,
                             long n_flat, float* norms, float lr, float beta2, float omb1, float omb2, float c1,
                             float c2, float eps, float wd, float max_grad_norm, float gs, void* stream) {
    if (T <= 0 || nchunks <= 0) return 0;
    if (!descs || !chunks || !norms || (max_grad_norm > 0.f && (!g_flat || n_flat <= 0))) return -100;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(norms, 0, sizeof(float) * (2 * (size_t)T + 1), st) != hipSuccess) return -1;
    const LambArgs a{lr, beta2, omb1, omb2, c1, c2, eps, wd, max_grad_norm > 0.f ? max_grad_norm : 0.f, gs};
    if (max_grad_norm > 0.f) {
        long bx = ((n_flat + 3) / 4 + LAMB_THREADS - 1) / LAMB_THREADS;
        if (bx > LAMB_GNORM_BLOCKS) bx = LAMB_GNORM_BLOCKS;
        hipLaunchKernelGGL(lamb_gnorm_kernel, dim3((int)bx), dim3(LAMB_THREADS), 0, st, g_flat, n_flat,
                           norms + 2 * (size_t)T);
        IMK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(lamb_kernel<false>, dim3(nchunks), dim3(LAMB_THREADS), 0, st, (const LambDesc*)descs,
                       (const long*)chunks, norms, T, a);
    IMK_CHECK_LAUNCH();
    hipLaunchKernelGGL(lamb_kernel<true>, dim3(nchunks), dim3(LAMB_THREADS), 0, st, (const LambDesc*)descs,
                       (const long*)chunks, norms, T, a);
    IMK_CHECK_LAUNCH();
    return 0;
}

IMK_EXPORT int imk_lamb_desc_size() { return (int)sizeof(LambDesc); }

// the launch geometry the tests' rounding bounds are computed from: 0 LAMB_CHUNK, 1 threads per block,
// 2 pass A's grid cap, 3 the flat kernels' grid cap (stream_grid)
IMK_EXPORT int imk_optim_const(int which) {
    switch (which) {
        case 0: return LAMB_CHUNK;
        case 1: return LAMB_THREADS;
        case 2: return LAMB_GNORM_BLOCKS;
        case 3: return STREAM_GRID_CAP;
        default: return -1;
    }
}
