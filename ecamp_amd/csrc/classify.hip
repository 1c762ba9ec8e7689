// Linear-probe classification behind the frozen encoder (Fine-tuning/Classification of the reference: models_vit.py:88-95, train.py:148,
// 200-202,423-425): token mean + fc_norm in one pass over the last block's output, and the small-class-count head (1..64 classes) with
// its loss, gradient and weight gradient.  Everything here is f32 arithmetic and DETERMINISTIC: every sum has one fixed order (per-thread
// strides, LDS slices added in index order, partials added in index order), no float atomic, and no workgroup waits for another.
// No grid depends on a row count beyond a cap: the kernels loop over samples / rows.
#include "classify.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// ecamp_pool_norm.  HBM-bound (B = 256, T = 197, D = 768 in 16 bits: 77 MB), so the token range of a sample is spread over `nchunk`
// workgroups -- enough that a small batch still covers the chip -- which leave f32 partial column sums [B, nchunk, D] in the
// workspace; a second, small kernel adds the partials in chunk order, divides, and normalises the row (one workgroup per sample).
// Stage 1 layout: a 256-thread workgroup covers `cw` 16-byte column vectors x `rows_par` token lanes (768 columns of bf16 = 96 vectors
// x 2 lanes); a thread walks its token lane four 16-byte loads at a time, the lanes are added through LDS in lane order.
template <typename T, int VEC>
__global__ __launch_bounds__(POOL_THREADS) void pool_partial_kernel(const T* __restrict__ x, float* __restrict__ part, int64_t B, int Tn, int D,
                                                                    int t0, int t1, int nv, int cw, int rows_par, int nslab, int nchunk,
                                                                    int chunk_len) {
    typedef Vec<T, VEC> V;
    typedef typename V::raw_t raw_t;
    __shared__ __attribute__((aligned(16))) float sh[POOL_THREADS * VEC];
    const int r = threadIdx.x / cw, c = threadIdx.x % cw;
    const int64_t items = B * nchunk * nslab;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int slab = (int)(item % nslab);
        const int chunk = (int)((item / nslab) % nchunk);
        const int64_t b = item / ((int64_t)nslab * nchunk);
        const int cv = slab * cw + c;
        const int ta = t0 + chunk * chunk_len;
        const int tb = ta + chunk_len < t1 ? ta + chunk_len : t1;
        const bool live = r < rows_par && cv < nv;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        if (live) {
            const T* base = x + b * Tn * (int64_t)D + (int64_t)cv * VEC;
            int t = ta + r;
            for (; t + 3 * rows_par < tb; t += 4 * rows_par) {   // four loads in flight per thread
                const raw_t v0 = *reinterpret_cast<const raw_t*>(base + (int64_t)t * D);
                const raw_t v1 = *reinterpret_cast<const raw_t*>(base + (int64_t)(t + rows_par) * D);
                const raw_t v2 = *reinterpret_cast<const raw_t*>(base + (int64_t)(t + 2 * rows_par) * D);
                const raw_t v3 = *reinterpret_cast<const raw_t*>(base + (int64_t)(t + 3 * rows_par) * D);
                V::add(v0, acc); V::add(v1, acc); V::add(v2, acc); V::add(v3, acc);
            }
            for (; t < tb; t += rows_par) V::add(*reinterpret_cast<const raw_t*>(base + (int64_t)t * D), acc);
#pragma unroll
            for (int k = 0; k < VEC; k += 4)
                *reinterpret_cast<float4*>(sh + threadIdx.x * VEC + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
        }
        __syncthreads();
        if (live && r == 0) {   // token lanes 1 .. rows_par-1 onto lane 0, in lane order
            for (int rr = 1; rr < rows_par; ++rr) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += sh[(rr * cw + c) * VEC + k];
            }
            float* dst = part + ((b * nchunk + chunk) * (int64_t)D + (int64_t)cv * VEC);
#pragma unroll
            for (int k = 0; k < VEC; k += 4) *reinterpret_cast<float4*>(dst + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void pool_norm_finish_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ pooled,
                                                               float* __restrict__ feat, int64_t B, int D, int nchunk, float ntok, float eps) {
    __shared__ float sh[4];
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        float* prow = pooled + b * D;
        float s = 0.f;
        for (int d = threadIdx.x; d < D; d += 256) {
            float a = 0.f;
            for (int ch = 0; ch < nchunk; ++ch) a += part[(b * nchunk + ch) * (int64_t)D + d];
            a /= ntok;
            prow[d] = a;   // re-read below by the thread that wrote it
            s += a;
        }
        const float mu = block_sum_256(s, sh) / (float)D;
        float q = 0.f;
        for (int d = threadIdx.x; d < D; d += 256) {
            const float dv = prow[d] - mu;
            q += dv * dv;
        }
        const float rs = rsqrtf(block_sum_256(q, sh) / (float)D + eps);
        for (int d = threadIdx.x; d < D; d += 256) {
            const float xh = (prow[d] - mu) * rs;
            feat[b * D + d] = gamma ? xh * gamma[d] + beta[d] : xh;
        }
    }
}

extern "C" int64_t ecamp_pool_norm_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t t0, int32_t t1, int32_t dtype) {
    if (!pool_shape_ok(B, T, D, t0, t1, dtype)) return 0;
    const PoolPlan p = pool_plan(B, t1 - t0, D, dtype);
    return B * p.nchunk * (int64_t)D * (int64_t)sizeof(float);
}

extern "C" int ecamp_pool_norm(const void* x, const float* gamma, const float* beta, float* pooled, float* feat, int64_t B, int32_t T,
                               int32_t D, int32_t t0, int32_t t1, float eps, void* ws, int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(x && pooled && feat && ws, "pool_norm: null pointer");
    ECAMP_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "pool_norm: null pointer (gamma and beta are given together, or both null for an identity affine)");
    ECAMP_CHECK_ARG(D >= 4 && D % 4 == 0, "pool_norm: D=%d must be a positive multiple of 4", D);
    ECAMP_CHECK_ARG(t0 >= 0 && t0 < t1 && t1 <= T, "pool_norm: token range t0=%d, t1=%d must satisfy 0 <= t0 < t1 <= T=%d", t0, t1, T);
    ECAMP_CHECK_ARG(B >= 1, "pool_norm: B=%lld must be positive", (long long)B);
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "pool_norm: bad dtype %d", dtype);
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const PoolPlan p = pool_plan(B, t1 - t0, D, dtype);
    ECAMP_CHECK_ARG(al16(ws) && al16(pooled) && al16(feat) && (reinterpret_cast<uintptr_t>(x) & (p.vec == 4 && dtype == ECAMP_BF16 ? 7 : 15)) == 0,
                    "pool_norm: x, pooled, feat and ws must be 16-byte aligned");
    const int64_t items = B * p.nchunk * p.nslab;
    const dim3 grid((unsigned)(items < CLS_MAX_GRID ? items : CLS_MAX_GRID)), block(POOL_THREADS);
#define L(T_, V_) hipLaunchKernelGGL((pool_partial_kernel<T_, V_>), grid, block, 0, stream, (const T_*)x, (float*)ws, B, T, D, t0, t1, p.nv, p.cw, \
                                     p.rows_par, p.nslab, p.nchunk, p.chunk_len)
    if (dtype == ECAMP_F32) L(float, 4);
    else if (p.vec == 8) L(bf16_t, 8);
    else L(bf16_t, 4);
#undef L
    ECAMP_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_norm_finish_kernel, dim3((unsigned)(B < CLS_MAX_GRID ? B : CLS_MAX_GRID)), dim3(256), 0, stream, (const float*)ws, gamma,
                       beta, pooled, feat, B, D, p.nchunk, (float)(t1 - t0), eps);
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The head: logits[B, C] = feat[B, D] . W[C, D]^T + b[C] for 1 <= C <= 64 (the datasets have 1..20 classes: N far below an MFMA tile, so
// a plain f32 dot product): one wave per (sample, class), lanes stride over the row in 16-byte vectors, one wave reduction.
__global__ __launch_bounds__(256) void cls_head_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ logits, int64_t B, int C, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t items = B * C;
    const int nv = D / 4;
    for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += (int64_t)gridDim.x * 4) {   // (wave-uniform trip count)
        const int64_t b = it / C;
        const int c = (int)(it % C);
        const float4* f = reinterpret_cast<const float4*>(feat + b * D);
        const float4* w = reinterpret_cast<const float4*>(W + (int64_t)c * D);
        float s = 0.f;
        for (int i = lane; i < nv; i += 64) {
            const float4 a = f[i], v = w[i];
            s += (a.x * v.x + a.y * v.y) + (a.z * v.z + a.w * v.w);
        }
        s = wave_sum(s);
        if (lane == 0) logits[it] = s + bias[c];
    }
}

extern "C" int ecamp_cls_head_fwd(const float* feat, const float* W, const float* bias, float* logits, int64_t B, int32_t C, int32_t D,
                                  hipStream_t stream) {
    ECAMP_CHECK_ARG(feat && W && bias && logits, "cls_head_fwd: null pointer");
    ECAMP_CHECK_ARG(C >= 1 && C <= CLS_MAX_CLASSES, "cls_head_fwd: C=%d must lie in [1, %d]", C, CLS_MAX_CLASSES);
    ECAMP_CHECK_ARG(D >= 4 && D % 4 == 0, "cls_head_fwd: D=%d must be a positive multiple of 4", D);
    ECAMP_CHECK_ARG(B >= 1, "cls_head_fwd: B=%lld must be positive", (long long)B);
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(W)) & 15) == 0, "cls_head_fwd: feat and W must be 16-byte aligned");
    const int64_t blocks = (B * C + 3) / 4;
    hipLaunchKernelGGL(cls_head_fwd_kernel, dim3((unsigned)(blocks < CLS_MAX_GRID ? blocks : CLS_MAX_GRID)), dim3(256), 0, stream, feat, W, bias, logits,
                       B, C, D);
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Loss, gradient of the mean and prediction counts in ONE workgroup: the whole problem is B x C <= a few 10^4 values, and a single
// workgroup gives the ordered sum without a workspace.  A thread owns rows tid, tid + 1024, ...; its partial sums are added by wave
// shuffles, then across the sixteen waves in wave order.
//   kind 0  BCEWithLogitsLoss (train.py:200,423): targets f32 [B, C]; max(x,0) - x y + log1p(exp(-|x|)), mean over B*C;
//           a row is right when every class lies on its target's side of 0 (sigmoid(x) > 0.5 <=> x > 0, train.py:220)
//   kind 1  CrossEntropyLoss (train.py:202,425): targets int64 [B]; row maximum subtracted, mean over B; a row is right when its
//           FIRST maximum is the label (torch.argmax, train.py:222).  A label outside [0, C) reads nothing: the row gets a zero
//           loss and gradient and *bad_label becomes 1.
constexpr int LOSS_THREADS = 1024;

__global__ __launch_bounds__(LOSS_THREADS) void cls_loss_kernel(const float* __restrict__ logits, const void* __restrict__ targets, int kind,
                                                                float* __restrict__ loss, float* __restrict__ dlogits, int64_t* __restrict__ counts,
                                                                int32_t* __restrict__ bad_label, int64_t B, int C) {
    __shared__ float shl[LOSS_THREADS / 64];
    __shared__ int shr[LOSS_THREADS / 64], shb[LOSS_THREADS / 64];
    const float inv = kind == 0 ? 1.0f / ((float)B * (float)C) : 1.0f / (float)B;
    float lsum = 0.f;
    int right = 0, bad = 0;
    for (int64_t b = threadIdx.x; b < B; b += LOSS_THREADS) {
        const float* x = logits + b * C;
        float* g = dlogits + b * C;
        if (kind == 0) {
            const float* y = reinterpret_cast<const float*>(targets) + b * C;
            bool ok = true;
            float rl = 0.f;
            for (int c = 0; c < C; ++c) {
                const float xv = x[c], yv = y[c];
                const float e = expf(-fabsf(xv));
                rl += fmaxf(xv, 0.f) - xv * yv + log1pf(e);
                const float sig = xv >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
                g[c] = (sig - yv) * inv;
                ok = ok && ((xv > 0.f) == (yv > 0.5f));
            }
            lsum += rl;
            right += ok ? 1 : 0;
        } else {
            const int64_t lab = reinterpret_cast<const int64_t*>(targets)[b];
            if (lab < 0 || lab >= C) {
                bad = 1;
                for (int c = 0; c < C; ++c) g[c] = 0.f;
                continue;
            }
            float m = x[0];
            int am = 0;
            for (int c = 1; c < C; ++c) {
                if (x[c] > m) { m = x[c]; am = c; }   // strictly greater: ties go to the lowest index
            }
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += expf(x[c] - m);
            lsum += logf(se) - (x[(int)lab] - m);
            const float rse = 1.0f / se;
            for (int c = 0; c < C; ++c) g[c] = (expf(x[c] - m) * rse - (c == (int)lab ? 1.0f : 0.f)) * inv;
            right += am == (int)lab ? 1 : 0;
        }
    }
    lsum = wave_sum(lsum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        right += __shfl_xor(right, o, 64);
        bad |= __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        shl[threadIdx.x >> 6] = lsum;
        shr[threadIdx.x >> 6] = right;
        shb[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.f;
        int64_t r = 0;
        int any = 0;
        for (int w = 0; w < LOSS_THREADS / 64; ++w) {
            tot += shl[w];
            r += shr[w];
            any |= shb[w];
        }
        loss[0] = tot * inv;
        counts[0] = B;
        counts[1] = r;
        bad_label[0] = any;
    }
}

extern "C" int ecamp_cls_loss(const float* logits, const void* targets, int32_t kind, float* loss, float* dlogits, int64_t* counts,
                              int32_t* bad_label, int64_t B, int32_t C, hipStream_t stream) {
    ECAMP_CHECK_ARG(logits && targets && loss && dlogits && counts && bad_label, "cls_loss: null pointer");
    ECAMP_CHECK_ARG(C >= 1 && C <= CLS_MAX_CLASSES, "cls_loss: C=%d must lie in [1, %d]", C, CLS_MAX_CLASSES);
    ECAMP_CHECK_ARG(kind == 0 || kind == 1, "cls_loss: kind=%d must be 0 (BCE with logits, f32 targets) or 1 (cross entropy, int64 labels)", kind);
    ECAMP_CHECK_ARG(B >= 1 && B < (1ll << 31), "cls_loss: B=%lld must lie in [1, 2^31)", (long long)B);
    hipLaunchKernelGGL(cls_loss_kernel, dim3(1), dim3(LOSS_THREADS), 0, stream, logits, targets, kind, loss, dlogits, counts, bad_label, B, C);
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dW[C, D] = dlogits^T . feat, db[C] = column sums of dlogits, overwriting.  One workgroup per (class, 64-column tile): sixteen
// sample lanes x sixteen 16-byte column vectors; a thread adds samples lane, lane + 16, ... in that order, the lanes are added through
// LDS in lane order -- the summation order over B depends on nothing but B.  The workgroup of a class's first tile also leaves db.
__global__ __launch_bounds__(256) void cls_head_wgrad_kernel(const float* __restrict__ dlogits, const float* __restrict__ feat,
                                                             float* __restrict__ dW, float* __restrict__ db, int64_t B, int C, int D, int ntile) {
    __shared__ float4 sh[256];
    __shared__ float shs[4];
    const int c = blockIdx.x / ntile, tile = blockIdx.x % ntile;
    const int dl = threadIdx.x & 15, bg = threadIdx.x >> 4;
    const int d = tile * 64 + dl * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d < D) {
        for (int64_t b = bg; b < B; b += 16) {
            const float g = dlogits[b * C + c];
            const float4 f = *reinterpret_cast<const float4*>(feat + b * D + d);
            acc.x += g * f.x; acc.y += g * f.y; acc.z += g * f.z; acc.w += g * f.w;
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (bg == 0 && d < D) {
        for (int k = 1; k < 16; ++k) {
            const float4 o = sh[k * 16 + dl];
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
        *reinterpret_cast<float4*>(dW + (int64_t)c * D + d) = acc;
    }
    if (tile == 0) {   // (uniform over the workgroup)
        float s = 0.f;
        for (int64_t b = threadIdx.x; b < B; b += 256) s += dlogits[b * C + c];
        s = block_sum_256(s, shs);
        if (threadIdx.x == 0) db[c] = s;
    }
}

extern "C" int ecamp_cls_head_wgrad(const float* dlogits, const float* feat, float* dW, float* db, int64_t B, int32_t C, int32_t D,
                                    hipStream_t stream) {
    ECAMP_CHECK_ARG(dlogits && feat && dW && db, "cls_head_wgrad: null pointer");
    ECAMP_CHECK_ARG(C >= 1 && C <= CLS_MAX_CLASSES, "cls_head_wgrad: C=%d must lie in [1, %d]", C, CLS_MAX_CLASSES);
    ECAMP_CHECK_ARG(D >= 4 && D % 4 == 0, "cls_head_wgrad: D=%d must be a positive multiple of 4", D);
    ECAMP_CHECK_ARG(B >= 1, "cls_head_wgrad: B=%lld must be positive", (long long)B);
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(dW)) & 15) == 0, "cls_head_wgrad: feat and dW must be 16-byte aligned");
    const int ntile = ceil_div(D, 64);
    hipLaunchKernelGGL(cls_head_wgrad_kernel, dim3((unsigned)(C * ntile)), dim3(256), 0, stream, dlogits, feat, dW, db, B, C, D, ntile);
    ECAMP_LAUNCH_CHECK();
    return 0;
}
