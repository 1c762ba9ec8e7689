// Fine-tuning the encoder behind the classifier (Fine-tuning/Classification of the reference, `--mode Finetune`: train.py:377-384 SGD with
// momentum, :456-461 clip_grad_norm_ + step): the two backward kernels between the loss and the last transformer block
// (ecamp_cls_head_dgrad, ecamp_pool_norm_bwd) and SGD with the global-norm clip over a flat parameter buffer (ecamp_sumsq_grouped,
// ecamp_sgd_grouped), and the stem's batch reduction for a trained pos_embed (ecamp_pos_embed_grad, `--train_pos_embed`).  Conventions as
// classify.hip: f32 arithmetic, every sum in ONE fixed order (per-thread strides, LDS, partials in index order), no float atomic, no
// workgroup waits for another, grids capped with a loop beyond the cap.  All five are HBM-bound: 16-byte accesses, three or four loads
// in flight per thread, enough workgroups for 256 CUs.
#include "classify.h"
#include "group_hyper.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// dfeat[B, D] = dlogits[B, C] . W[C, D]: the data gradient of the head (C <= 64: far below an MFMA tile).  One thread per (sample,
// 16-byte column vector); the C terms are added in class order.
__global__ __launch_bounds__(256) void cls_head_dgrad_kernel(const float* __restrict__ dlogits, const float* __restrict__ W,
                                                             float* __restrict__ dfeat, int64_t B, int C, int D) {
    const int nv = D / 4;
    const int64_t items = B * nv;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int64_t b = it / nv;
        const int v = (int)(it % nv);
        const float* g = dlogits + b * C;
        const float4* w = reinterpret_cast<const float4*>(W) + v;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = 0; c < C; ++c) {
            const float gc = g[c];
            const float4 wv = w[(int64_t)c * nv];
            acc.x += gc * wv.x; acc.y += gc * wv.y; acc.z += gc * wv.z; acc.w += gc * wv.w;
        }
        reinterpret_cast<float4*>(dfeat)[it] = acc;
    }
}

extern "C" int ecamp_cls_head_dgrad(const float* dlogits, const float* W, float* dfeat, int64_t B, int32_t C, int32_t D, hipStream_t stream) {
    ECAMP_CHECK_ARG(dlogits && W && dfeat, "cls_head_dgrad: null pointer");
    ECAMP_CHECK_ARG(C >= 1 && C <= CLS_MAX_CLASSES, "cls_head_dgrad: C=%d must lie in [1, %d]", C, CLS_MAX_CLASSES);
    ECAMP_CHECK_ARG(D >= 4 && D % 4 == 0, "cls_head_dgrad: D=%d must be a positive multiple of 4", D);
    ECAMP_CHECK_ARG(B >= 1, "cls_head_dgrad: B=%lld must be positive", (long long)B);
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(dfeat)) & 15) == 0, "cls_head_dgrad: W and dfeat must be 16-byte aligned");
    hipLaunchKernelGGL(cls_head_dgrad_kernel, flat_grid(B * (D / 4), CLS_MAX_GRID), dim3(256), 0, stream, dlogits, W, dfeat, B, C, D);
    return ecamp_launch_status(__func__);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ecamp_pool_norm_bwd, three launches:
//   1. per sample (one workgroup, looping beyond PNB_ROW_GRID): mean / rstd of pooled[b] again, the LayerNorm backward, and
//      dpooled[b] / (t1 - t0) into the workspace; the workgroup's running sums of dfeat * xhat and dfeat over ITS samples, in sample
//      order, go to its own slab of the workspace (a thread re-reads only what it wrote itself);
//   2. dgamma / dbeta = the slabs added in workgroup order (written, not accumulated);
//   3. the store of dx [B, T, D] -- where the bytes are (77 MB at B = 256 in 16 bits): the rows of a sample are split over workgroups as
//      ecamp_pool_norm splits them, a thread converts its 16-byte column vector once and stores it down its row lane; rows outside
//      [t0, t1) get zeros.  (pool_plan, classify.h: the one split of both directions.)
constexpr int PNB_ROW_GRID = 256;       // workgroups of launch 1 = partial slabs launch 2 adds per column
static int pnb_row_wgs(int64_t B) { return (int)(B < PNB_ROW_GRID ? B : PNB_ROW_GRID); }

// The one place of this file that leaves f32 arithmetic: dpooled = rstd * (g - mean(g) - xhat * mean(g * xhat)) cancels, and an element
// that comes out small carries the f32 rounding of its three terms -- 1e-7 of THEIR size, not of its own -- while the 16-bit dx is held
// to one rounding of the format relative to EACH element.  The row stage is B x D values (0.3 % of the dx bytes), so it runs in f64 and
// rounds once to f32; the sums for dgamma / dbeta stay f32.  f64 also lets ONE pass gather everything the row needs -- sum p, sum p^2,
// sum g, sum g p (variance = E[p^2] - mu^2 and sum g xhat = rstd (sum g p - mu sum g) lose 1e-16 of their terms, not 1e-7) -- so a sample
// costs one block reduction of four values and two sweeps over its row.
__global__ __launch_bounds__(256) void pool_norm_bwd_row_kernel(const float* __restrict__ dfeat, const float* __restrict__ pooled,
                                                                const float* __restrict__ gamma, float* __restrict__ dpool,
                                                                float* __restrict__ part, int64_t B, int D, int ntok, float eps) {
    __shared__ double sh[4][4];
    float* pg = part ? part + (int64_t)blockIdx.x * 2 * D : nullptr;   // this workgroup's slab: [dgamma | dbeta]
    const double rD = 1.0 / (double)D;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const float* prow = pooled + b * D;
        const float* drow = dfeat + b * D;
        double a[4] = {0.0, 0.0, 0.0, 0.0};   // sum p, sum p^2, sum g, sum g p over this thread's columns, in column order
        for (int d = threadIdx.x; d < D; d += 256) {
            const double pv = (double)prow[d];
            const double g = gamma ? (double)drow[d] * (double)gamma[d] : (double)drow[d];
            a[0] += pv; a[1] += pv * pv; a[2] += g; a[3] += g * pv;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
        }
        __syncthreads();   // (the previous sample's reads of sh are done)
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x >> 6] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
        const double mu = a[0] * rD;
        const double var = a[1] * rD - mu * mu;
        const double rs = 1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)eps);
        const double c1 = a[2] * rD;                       // mean of g
        const double c2 = rs * (a[3] - mu * a[2]) * rD;    // mean of g * xhat
        const double scale = rs / (double)ntok;
        const bool first = b == (int64_t)blockIdx.x;
        for (int d = threadIdx.x; d < D; d += 256) {
            const double xh = ((double)prow[d] - mu) * rs;
            const float df = drow[d];
            const double g = gamma ? (double)df * (double)gamma[d] : (double)df;
            dpool[b * D + d] = (float)(scale * (g - c1 - xh * c2));
            if (pg) {
                const float t = df * (float)xh;
                pg[d] = first ? t : pg[d] + t;
                pg[D + d] = first ? df : pg[D + d] + df;
            }
        }
    }
}

// dgamma / dbeta = the slabs of launch 1 added in workgroup order.  One workgroup per 64-column tile: sixteen slab lanes x sixteen 16-byte
// column vectors; a thread adds slabs lane, lane + 16, ... in that order, the lanes are added through LDS in lane order (as
// cls_head_wgrad_kernel adds its samples) -- a thread that walked all 256 slabs alone would spend 256 dependent L2 round trips.
__global__ __launch_bounds__(256) void pool_norm_bwd_affine_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, int D, int nwg) {
    __shared__ float4 shg[256], shb[256];
    const int dl = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int d = blockIdx.x * 64 + dl * 4;
    float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), ab = ag;
    if (d < D) {
        for (int w = lane; w < nwg; w += 16) {
            const float4 g = *reinterpret_cast<const float4*>(part + (int64_t)w * 2 * D + d);
            const float4 c = *reinterpret_cast<const float4*>(part + (int64_t)w * 2 * D + D + d);
            ag.x += g.x; ag.y += g.y; ag.z += g.z; ag.w += g.w;
            ab.x += c.x; ab.y += c.y; ab.z += c.z; ab.w += c.w;
        }
    }
    shg[threadIdx.x] = ag;
    shb[threadIdx.x] = ab;
    __syncthreads();
    if (lane == 0 && d < D) {
        for (int k = 1; k < 16; ++k) {
            const float4 g = shg[k * 16 + dl], c = shb[k * 16 + dl];
            ag.x += g.x; ag.y += g.y; ag.z += g.z; ag.w += g.w;
            ab.x += c.x; ab.y += c.y; ab.z += c.z; ab.w += c.w;
        }
        *reinterpret_cast<float4*>(dgamma + d) = ag;
        *reinterpret_cast<float4*>(dbeta + d) = ab;
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void pool_norm_bwd_store_kernel(const float* __restrict__ dpool, T* __restrict__ dx, int64_t B, int Tn, int D,
                                                                  int t0, int t1, int nv, int cw, int rows_par, int nslab, int nchunk,
                                                                  int chunk_len) {
    typedef Vec<T, VEC> V;
    typedef typename V::raw_t raw_t;
    const int r = threadIdx.x / cw, c = threadIdx.x % cw;
    const int64_t items = B * nchunk * nslab;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int slab = (int)(item % nslab);
        const int chunk = (int)((item / nslab) % nchunk);
        const int64_t b = item / ((int64_t)nslab * nchunk);
        const int cv = slab * cw + c;
        if (r >= rows_par || cv >= nv) continue;
        const int ta = chunk * chunk_len;
        const int tb = ta + chunk_len < Tn ? ta + chunk_len : Tn;
        float v[VEC];
        Vec<float, VEC>::cvt(Vec<float, VEC>::load(dpool + b * D + (int64_t)cv * VEC), v);
        const raw_t val = V::pack(v), zero = V::zero();
        T* base = dx + b * Tn * (int64_t)D + (int64_t)cv * VEC;
        for (int t = ta + r; t < tb; t += rows_par) *reinterpret_cast<raw_t*>(base + (int64_t)t * D) = (t >= t0 && t < t1) ? val : zero;
    }
}

extern "C" int64_t ecamp_pool_norm_bwd_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t t0, int32_t t1, int32_t dtype) {
    if (!pool_shape_ok(B, T, D, t0, t1, dtype)) return 0;
    return (B + 2 * (int64_t)pnb_row_wgs(B)) * D * (int64_t)sizeof(float);   // dpooled [B, D] | slabs [row workgroups, 2, D]
}

extern "C" int ecamp_pool_norm_bwd(const float* dfeat, const float* pooled, const float* gamma, float* dgamma, float* dbeta, void* dx, int64_t B,
                                   int32_t T, int32_t D, int32_t t0, int32_t t1, float eps, void* ws, int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(dfeat && pooled && dx && ws, "pool_norm_bwd: null pointer");
    ECAMP_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "pool_norm_bwd: null pointer (dgamma and dbeta are given together, or both null)");
    ECAMP_CHECK_ARG(D >= 4 && D % 4 == 0, "pool_norm_bwd: D=%d must be a positive multiple of 4", D);
    ECAMP_CHECK_ARG(t0 >= 0 && t0 < t1 && t1 <= T, "pool_norm_bwd: token range t0=%d, t1=%d must satisfy 0 <= t0 < t1 <= T=%d", t0, t1, T);
    ECAMP_CHECK_ARG(B >= 1, "pool_norm_bwd: B=%lld must be positive", (long long)B);
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "pool_norm_bwd: bad dtype %d", dtype);
    const PoolPlan p = pool_plan(B, T, D, dtype);
    const int nrow_wg = pnb_row_wgs(B);
    ECAMP_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(dx) & (p.vec == 4 && dtype == ECAMP_BF16 ? 7 : 15)) == 0 &&
                        ((reinterpret_cast<uintptr_t>(dgamma) | reinterpret_cast<uintptr_t>(dbeta)) & 15) == 0,
                    "pool_norm_bwd: dx, ws, dgamma and dbeta must be 16-byte aligned");
    float* dpool = (float*)ws;
    float* part = dgamma ? dpool + B * D : nullptr;
    hipLaunchKernelGGL(pool_norm_bwd_row_kernel, dim3((unsigned)nrow_wg), dim3(256), 0, stream, dfeat, pooled, gamma, dpool, part, B, D,
                       t1 - t0, eps);
    ECAMP_LAUNCH_CHECK();
    if (dgamma) {
        hipLaunchKernelGGL(pool_norm_bwd_affine_kernel, dim3((unsigned)ceil_div(D, 64)), dim3(256), 0, stream, (const float*)part, dgamma, dbeta, D,
                           nrow_wg);
        ECAMP_LAUNCH_CHECK();
    }
    const int64_t items = B * p.nchunk * p.nslab;
    const dim3 grid((unsigned)(items < CLS_MAX_GRID ? items : CLS_MAX_GRID)), block(256);
#define L(T_, V_) hipLaunchKernelGGL((pool_norm_bwd_store_kernel<T_, V_>), grid, block, 0, stream, (const float*)dpool, (T_*)dx, B, T, D, t0, t1, p.nv, \
                                     p.cw, p.rows_par, p.nslab, p.nchunk, p.chunk_len)
    if (dtype == ECAMP_F32) L(float, 4);
    else if (p.vec == 8) L(bf16_t, 8);
    else L(bf16_t, 4);
#undef L
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ecamp_pos_embed_grad: the three parameter gradients of the stem that are sums of rows of S[t, d] = sum_b dx[b, t, d] -- pos_embed (S
// itself), cls_token (row 0) and the patch embedding's bias (rows 1 .. T-1 added up) -- from ONE pass over dx.  Two launches:
//   1. the stream (where the bytes are: 29 MB at ViT-B, B = 96, in 16 bits).  S is T*D / VEC independent columns of 16-byte vectors; a
//      workgroup takes PEG_CW of them x four batch lanes (one wave each, so a wave's load is 1 KB in one piece), and the batch is cut
//      into `nsplit` ranges over workgroups until 256 CUs have work (peg_plan).  A lane adds its samples b0 + lane, b0 + lane + 4, ... in
//      that order, four loads in flight; the lanes are added through LDS in lane order; the range's partial goes to ws[split][T*D].
//   2. the small one: S = the ranges' partials added in range order, into dpos (row 0 also into dcls) with one 16-byte vector per thread,
//      and the sum of its rows 1 .. T-1 into dbias, 64 token lanes per 16-column tile (pos_embed_grad_apply_kernel).
constexpr int PEG_CW = 64;              // 16-byte column vectors per workgroup of launch 1
constexpr int PEG_LANES = 4;            // batch lanes per workgroup of launch 1
constexpr int PEG_TARGET_WG = 1024;     // as POOL_TARGET_WG: four workgroups per CU before the batch stops being split further
constexpr int PEG_MAX_SPLIT = 16;

struct PegPlan {
    int vec, ntile, nsplit;
    int64_t nv, bchunk;
};

// A function of (B, T, D, dtype) alone, so that the workspace size, both launches and with them every summation order agree.
static PegPlan peg_plan(int64_t B, int T, int D, int dtype) {
    PegPlan p;
    p.vec = dtype == ECAMP_F32 ? 4 : 8;
    p.nv = (int64_t)T * D / p.vec;
    p.ntile = (int)((p.nv + PEG_CW - 1) / PEG_CW);
    int64_t want = (PEG_TARGET_WG + p.ntile - 1) / p.ntile;
    const int64_t most = (B + PEG_LANES * 4 - 1) / (PEG_LANES * 4);   // a lane keeps at least four samples: its loads in flight
    if (want > most) want = most;
    if (want > PEG_MAX_SPLIT) want = PEG_MAX_SPLIT;
    if (want < 1) want = 1;
    p.bchunk = (B + want - 1) / want;
    p.nsplit = (int)((B + p.bchunk - 1) / p.bchunk);
    return p;
}

static bool peg_shape_ok(int64_t B, int32_t T, int32_t D, int32_t dtype) {
    if (dtype != ECAMP_F32 && dtype != ECAMP_BF16) return false;
    return B >= 1 && T >= 2 && D >= 1 && D % (dtype == ECAMP_F32 ? 4 : 8) == 0;
}

template <typename T>
__global__ __launch_bounds__(256) void pos_embed_grad_stream_kernel(const T* __restrict__ dx, float* __restrict__ part, int64_t B, int64_t nv,
                                                                    int ntile, int nsplit, int64_t bchunk) {
    constexpr int VEC = 16 / sizeof(T);   // one 16-byte access: peg_plan's `vec`
    typedef Vec<T, VEC> V;
    typedef typename V::raw_t raw_t;
    __shared__ float sh[PEG_LANES - 1][VEC][PEG_CW];   // [lane][element][column]: a wave writes 64 consecutive floats
    const int c = threadIdx.x & (PEG_CW - 1), lane = threadIdx.x / PEG_CW;
    const int64_t items = (int64_t)ntile * nsplit;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int split = (int)(item / ntile);
        const int64_t cv = (item % ntile) * PEG_CW + c;
        const int64_t b0 = split * bchunk;
        const int64_t b1 = b0 + bchunk < B ? b0 + bchunk : B;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        if (cv < nv) {
            const raw_t* src = reinterpret_cast<const raw_t*>(dx) + cv;   // sample b of this column: src[b * nv]
            int64_t b = b0 + lane;
            for (; b + 3 * PEG_LANES < b1; b += 4 * PEG_LANES) {   // four loads in flight, added in sample order
                raw_t v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = src[(b + k * PEG_LANES) * nv];
#pragma unroll
                for (int k = 0; k < 4; ++k) V::add(v[k], acc);
            }
            for (; b < b1; b += PEG_LANES) V::add(src[b * nv], acc);
        }
        if (lane > 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) sh[lane - 1][k][c] = acc[k];
        }
        __syncthreads();
        if (lane == 0 && cv < nv) {
#pragma unroll
            for (int l = 0; l < PEG_LANES - 1; ++l) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += sh[l][k][c];
            }
            float* dst = part + ((int64_t)split * nv + cv) * VEC;
#pragma unroll
            for (int k = 0; k < VEC; k += 4) *reinterpret_cast<float4*>(dst + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
        }
        __syncthreads();   // (lane 0 has read sh before the next item writes it)
    }
}

// S[t, d .. d + 3] of the float4 at element offset o of the table: the ranges' partials added in range order.
__device__ __forceinline__ float4 peg_table(const float* __restrict__ part, int64_t o, int64_t TD, int nsplit) {
    float4 s = *reinterpret_cast<const float4*>(part + o);
    for (int k = 1; k < nsplit; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(part + k * TD + o);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    return s;
}

__device__ __forceinline__ void peg_add4(float* p, const float4& s) {
    float4 g = *reinterpret_cast<const float4*>(p);
    g.x += s.x; g.y += s.y; g.z += s.z; g.w += s.w;
    *reinterpret_cast<float4*>(p) = g;
}

// Launch 2, two kinds of workgroup in one grid (a single workgroup per 64-column tile walking all tokens took 18 us at T = 197 whatever
// the batch: thirteen dependent trips to L2 per thread, on twelve CUs):
//   [0, npos): dpos += S, one float4 of the table per thread (its first row also into dcls);
//   [npos, npos + nbias): dbias of a PEG_BIAS_COLS-column tile: four 16-byte vectors x 64 token lanes, a lane adds S of the tokens
//     1 + lane, 65 + lane, ... in that order (loads only: the table is read again, from L2), then the lanes are added through LDS in
//     lane order, eight at a time and then the eight sums.
constexpr int PEG_BIAS_COLS = 16;
constexpr int PEG_APPLY_GRID = CLS_MAX_GRID / 2;   // the cap of either kind

__global__ __launch_bounds__(256) void pos_embed_grad_apply_kernel(const float* __restrict__ part, float* __restrict__ dpos,
                                                                   float* __restrict__ dcls, float* __restrict__ dbias, int Tn, int D, int nsplit,
                                                                   int npos, int nbias) {
    __shared__ float4 sh[256];
    const int64_t TD = (int64_t)Tn * D;
    if ((int)blockIdx.x < npos) {
        const int64_t n4 = TD / 4;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)npos * 256) {
            const int64_t o = i * 4;
            const float4 s = peg_table(part, o, TD, nsplit);
            peg_add4(dpos + o, s);
            if (dcls && o < D) peg_add4(dcls + o, s);   // row 0, the cls token (D % 4 == 0: a vector lies in one row)
        }
        return;
    }
    const int dl = threadIdx.x & 3, lane = threadIdx.x >> 2;
    for (int tile = (int)blockIdx.x - npos; tile * PEG_BIAS_COLS < D; tile += nbias) {
        const int d = tile * PEG_BIAS_COLS + dl * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (d < D) {
            for (int t = 1 + lane; t < Tn; t += 64) {   // (the cls row carries no patch: no share of the bias gradient)
                const float4 s = peg_table(part, (int64_t)t * D + d, TD, nsplit);
                a.x += s.x; a.y += s.y; a.z += s.z; a.w += s.w;
            }
        }
        sh[threadIdx.x] = a;
        __syncthreads();
        if (lane < 8) {
            a = sh[lane * 32 + dl];
            for (int k = 1; k < 8; ++k) {
                const float4 v = sh[(lane * 8 + k) * 4 + dl];
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        }
        __syncthreads();
        if (lane < 8) sh[lane * 4 + dl] = a;
        __syncthreads();
        if (lane == 0 && d < D) {
            a = sh[dl];
            for (int k = 1; k < 8; ++k) {
                const float4 v = sh[k * 4 + dl];
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
            peg_add4(dbias + d, a);
        }
        __syncthreads();   // (sh is read before the next tile writes it)
    }
}

extern "C" int64_t ecamp_pos_embed_grad_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t dtype) {
    if (!peg_shape_ok(B, T, D, dtype)) return 0;
    return (int64_t)peg_plan(B, T, D, dtype).nsplit * T * D * (int64_t)sizeof(float);   // partial sums [nsplit, T, D]
}

extern "C" int ecamp_pos_embed_grad(const void* dx, float* dpos, float* dcls, float* dbias, int64_t B, int32_t T, int32_t D, void* ws,
                                    int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(dx && dpos && ws, "pos_embed_grad: null pointer");
    ECAMP_CHECK_ARG((dcls == nullptr) == (dbias == nullptr), "pos_embed_grad: null pointer (dcls and dbias are given together, or both null)");
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "pos_embed_grad: bad dtype %d", dtype);
    ECAMP_CHECK_ARG(B >= 1, "pos_embed_grad: B=%lld must be positive", (long long)B);
    ECAMP_CHECK_ARG(T >= 2, "pos_embed_grad: T=%d must be at least 2 (the cls row and one patch)", T);
    ECAMP_CHECK_ARG(D >= 1 && D % (dtype == ECAMP_F32 ? 4 : 8) == 0, "pos_embed_grad: D=%d must be a positive multiple of %d", D,
                    dtype == ECAMP_F32 ? 4 : 8);
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dpos) | reinterpret_cast<uintptr_t>(dcls) |
                      reinterpret_cast<uintptr_t>(dbias) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
                    "pos_embed_grad: dx, dpos, dcls, dbias and ws must be 16-byte aligned");
    const PegPlan p = peg_plan(B, T, D, dtype);
    const int64_t items = (int64_t)p.ntile * p.nsplit;
    const dim3 grid((unsigned)(items < CLS_MAX_GRID ? items : CLS_MAX_GRID)), block(256);
    const int rc = ECAMP_LAUNCH_TYPED("pos_embed_grad", dtype, [&](auto tag) {
        typedef ECAMP_TAG_T(tag) T;
        hipLaunchKernelGGL(pos_embed_grad_stream_kernel<T>, grid, block, 0, stream, (const T*)dx, (float*)ws, B, p.nv, p.ntile, p.nsplit, p.bchunk);
    });
    if (rc) return rc;
    const int64_t pos_wg = ((int64_t)T * D / 4 + 255) / 256;
    const int npos = (int)(pos_wg < PEG_APPLY_GRID ? pos_wg : PEG_APPLY_GRID);
    const int bias_wg = ceil_div(D, PEG_BIAS_COLS);
    const int nbias = dbias ? (bias_wg < PEG_APPLY_GRID ? bias_wg : PEG_APPLY_GRID) : 0;
    hipLaunchKernelGGL(pos_embed_grad_apply_kernel, dim3((unsigned)(npos + nbias)), dim3(256), 0, stream, (const float*)ws, dpos, dcls, dbias, T, D,
                       p.nsplit, npos, nbias);
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sum(g^2) over the live 64-element blocks (block_group[i] < 8; 255 = frozen / not this optimizer's) of a flat gradient buffer: one f32
// partial per workgroup, NO scalar -- ecamp_sgd_grouped adds the partials itself, so the norm costs no launch of its own and no atomic.
// The grid, and with it every thread's share, is a function of n alone.
constexpr int SUMSQ_MAX_SLOTS = 2048;   // the documented cap: a launch fills at most this many slots (ecamp_sumsq_grouped_slots says how many)

static int sumsq_slots(int64_t n) {
    const int64_t nb = (n / 4 + 1023) / 1024;   // 256 threads x four 16-byte loads in flight
    return (int)(nb < 1 ? 1 : nb > SUMSQ_MAX_SLOTS ? SUMSQ_MAX_SLOTS : nb);
}

__global__ __launch_bounds__(256) void sumsq_grouped_kernel(const float* __restrict__ g, const unsigned char* __restrict__ grp, long n4,
                                                            float* __restrict__ partials) {
    __shared__ float sh[4];
    const long stride = (long)gridDim.x * 256;
    float acc = 0.f;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {   // four loads in flight per thread
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long j = i + k * stride;
            v[k] = grp[j >> 4] < 8 ? reinterpret_cast<const float4*>(g)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
    }
    for (; i < n4; i += stride) {
        if (grp[i >> 4] >= 8) continue;
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        acc += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

extern "C" int64_t ecamp_sumsq_grouped_slots(int64_t n) { return (n < 64 || n % 64 != 0) ? 0 : sumsq_slots(n); }

extern "C" int ecamp_sumsq_grouped(const float* g, const uint8_t* block_group, int64_t n, float* partials, int32_t* npart_out, hipStream_t stream) {
    ECAMP_CHECK_ARG(g && block_group && partials, "sumsq_grouped: null pointer");
    ECAMP_CHECK_ARG(n >= 64 && n % 64 == 0, "sumsq_grouped: n=%lld must be a positive multiple of 64", (long long)n);
    ECAMP_CHECK_ARG((reinterpret_cast<uintptr_t>(g) & 15) == 0, "sumsq_grouped: g must be 16-byte aligned");
    const int nb = sumsq_slots(n);
    hipLaunchKernelGGL(sumsq_grouped_kernel, dim3(nb), dim3(256), 0, stream, g, block_group, (long)(n / 4), partials);
    ECAMP_LAUNCH_CHECK();
    if (npart_out) *npart_out = nb;   // (a HOST int: the slots this launch filled, partials[0 .. nb))
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// torch.optim.SGD (momentum, dampening 0, no Nesterov, coupled weight decay) behind torch.nn.utils.clip_grad_norm_, over a flat buffer
// with ecamp_adamw_grouped's block table.  Every workgroup adds partials[0 .. npart) itself -- a few thousand floats from L2, in one
// order: thread t takes slots t, t + 256, ... in turn, then the 256 sums go through block_sum_256 -- so every workgroup holds the same
// bits of the norm and nothing waits for a reduction launch.  A zero momentum buffer reproduces torch's first step (buf = d).
// (partials_sum_256 is that order, shared with sgd_scale_update_kernel below: the loss scaler's decision and the step see one `s`.)
__device__ __forceinline__ float partials_sum_256(const float* partials, int npart, float* sh) {
    float s = 0.f;
    for (int k = threadIdx.x; k < npart; k += 256) s += partials[k];
    return block_sum_256(s, sh);
}

__global__ __launch_bounds__(256) void sgd_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                          bf16_t* __restrict__ p16, const unsigned char* __restrict__ grp, long n4, GroupHyper hp,
                                                          float momentum, float max_norm, const float* __restrict__ partials, int npart,
                                                          float gscale, const float* __restrict__ ctl, float* __restrict__ norm_out) {
    __shared__ float sh[4];
    if (ctl) {   // as adamw_grouped_kernel: an overflowed step leaves every byte alone
        if (ctl[1] != 0.f) return;
        gscale = ctl[0];
    }
    const float s = partials_sum_256(partials, npart, sh);
    const float norm = sqrtf(s) * gscale;
    const float coef = max_norm > 0.f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    const float gmul = gscale * coef;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const unsigned gi = grp[i >> 4];   // 16 float4 per 64-element block
        if (gi >= 8) continue;
        const float lr = hp.lr[gi], wd = hp.wd[gi];
        float pp[4], gg[4], bb[4];
        ld4<float>(p + i * 4, pp);
        ld4<float>(g + i * 4, gg);
        ld4<float>(buf + i * 4, bb);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = gg[r] * gmul + wd * pp[r];
            bb[r] = momentum * bb[r] + d;
            pp[r] -= lr * bb[r];
        }
        st4<float>(p + i * 4, pp);
        st4<float>(buf + i * 4, bb);
        if (p16) st4<bf16_t>(p16 + i * 4, pp);
    }
}

extern "C" int ecamp_sgd_grouped(float* p, const float* g, float* buf, void* p16, const uint8_t* block_group, int64_t n, int32_t ngroups,
                                 const float* lr_host, const float* wd_host, float momentum, float max_norm, const float* partials, int32_t npart,
                                 float grad_scale, const float* ctl, float* norm_out, hipStream_t stream) {
    ECAMP_CHECK_ARG(p && g && buf && block_group && lr_host && wd_host, "sgd_grouped: null pointer");
    ECAMP_CHECK_ARG(n >= 64 && n % 64 == 0, "sgd_grouped: n=%lld must be a positive multiple of 64", (long long)n);
    ECAMP_CHECK_ARG(ngroups >= 1 && ngroups <= 8, "sgd_grouped: ngroups=%d must lie in [1, 8]", ngroups);
    ECAMP_CHECK_ARG(npart >= 0 && npart <= 2 * SUMSQ_MAX_SLOTS, "sgd_grouped: npart=%d must lie in [0, %d]", npart, 2 * SUMSQ_MAX_SLOTS);
    ECAMP_CHECK_ARG(partials || npart == 0, "sgd_grouped: null pointer (partials) with npart=%d", npart);
    ECAMP_CHECK_ARG(!(max_norm > 0.f) || npart > 0, "sgd_grouped: max_norm=%g needs the partials of ecamp_sumsq_grouped (npart=%d)", (double)max_norm, npart);
    GroupHyper hp;
    for (int i = 0; i < 8; ++i) {
        hp.lr[i] = i < ngroups ? lr_host[i] : 0.f;
        hp.wd[i] = i < ngroups ? wd_host[i] : 0.f;
    }
    const long n4 = n / 4;
    hipLaunchKernelGGL(sgd_grouped_kernel, flat_grid(n4, GROUPED_MAX_GRID), dim3(256), 0, stream, p, g, buf, (bf16_t*)p16, block_group, n4, hp, momentum,
                       max_norm, partials, npart, grad_scale, ctl, norm_out);
    return ecamp_launch_status(__func__);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// apex's LossScaler.update_scale for loss_scale="dynamic" (what `--fp16 --fp16_opt_level O2` puts around the reference's SGD step,
// train.py:398,452-465), decided on the device from the partials ecamp_sumsq_grouped left over the SCALED gradients: one workgroup adds
// them in sgd_grouped_kernel's order (partials_sum_256: the same bits of `s` there and here), thread 0 writes the `ctl` that step reads,
// the norm of the un-scaled gradients and the next state.  state = {scale, clean steps since the last change, steps skipped in total,
// steps skipped in a row}; the counters are f32, exact to 2^24 steps.  window == 0: a static scale.
__global__ __launch_bounds__(256) void sgd_scale_update_kernel(const float* __restrict__ partials, int npart, float* __restrict__ state,
                                                               float* __restrict__ ctl, float* __restrict__ norm_out, float growth, float backoff,
                                                               float window, float max_scale) {
    __shared__ float sh[4];
    const float s = partials_sum_256(partials, npart, sh);
    if (threadIdx.x != 0) return;
    const float scale = state[0], inv = 1.0f / scale;
    const bool found = !(fabsf(s) <= 3.402823466e+38f);   // inf, nan, or finite slots whose sum left f32
    ctl[0] = inv;
    ctl[1] = found ? 1.f : 0.f;
    ctl[2] = 0.f;
    ctl[3] = 0.f;
    if (norm_out) norm_out[0] = sqrtf(s) * inv;             // sgd_grouped_kernel's expression under this ctl; inf / nan on overflow
    if (found) {
        if (window != 0.f) state[0] = scale * backoff;
        state[1] = 0.f;
        state[2] += 1.f;
        state[3] += 1.f;
    } else {
        const float clean = state[1] + 1.f;
        state[3] = 0.f;
        if (clean == window) {
            state[0] = fminf(max_scale, scale * growth);
            state[1] = 0.f;
        } else state[1] = clean;
    }
}

extern "C" int ecamp_sgd_scale_update(const float* partials, int32_t npart, float* state, float* ctl, float* norm_out, float growth, float backoff,
                                      int32_t window, float max_scale, hipStream_t stream) {
    ECAMP_CHECK_ARG(partials && state && ctl, "sgd_scale_update: null pointer");
    ECAMP_CHECK_ARG(npart >= 1 && npart <= 2 * SUMSQ_MAX_SLOTS, "sgd_scale_update: npart=%d must lie in [1, %d]", npart, 2 * SUMSQ_MAX_SLOTS);
    ECAMP_CHECK_ARG(growth >= 1.f, "sgd_scale_update: growth=%g must be at least 1", (double)growth);
    ECAMP_CHECK_ARG(backoff > 0.f && backoff <= 1.f, "sgd_scale_update: backoff=%g must lie in (0, 1]", (double)backoff);
    ECAMP_CHECK_ARG(window >= 0, "sgd_scale_update: window=%d must not be negative (0: a static scale)", window);
    ECAMP_CHECK_ARG(max_scale > 0.f, "sgd_scale_update: max_scale=%g must be positive", (double)max_scale);
    hipLaunchKernelGGL(sgd_scale_update_kernel, dim3(1), dim3(256), 0, stream, partials, npart, state, ctl, norm_out, growth, backoff, (float)window,
                       max_scale);
    return ecamp_launch_status(__func__);
}
