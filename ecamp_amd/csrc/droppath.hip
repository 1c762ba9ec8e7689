// Stochastic depth on the ViT residual stream (timm DropPath with scale_by_keep=True, the `drop_path` of timm's Block; the reference
// builds its fine-tuned ViT with drop_path_rate=0.1, Fine-tuning/Classification/train.py:127): a whole SAMPLE's branch output is dropped
// or scaled by 1 / (1 - p) before it joins the residual,
//     out[b, t, :] = res[b, t, :] + s_b * y[b, t, :],      s_b = dropout_scale(seed, offset, e = b, p, 1 / (1 - p))     (common.h)
// so the kept samples are the kept elements of ecamp_dropout_mask over a [B] tensor under the same (seed, offset).  No mask is stored:
// the backward regenerates s_b.  Both directions are HBM-bound element-wise passes; a sample's rows are contiguous, so the grid is
// (column blocks of one sample) x (samples), both capped with stride loops, and the Philox call is made once per (workgroup, sample),
// never per vector (common.h on what Philox costs).  No atomics: two calls give the same bits.
#include "common.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_MAX_BLOCKS = 4096;   // workgroups per launch, as the other element-wise kernels cap it
constexpr int DP_VEC_PER_THREAD = 4;  // vectors a thread walks per sample when the sample is long enough

// res, out: R [B, nv * VEC]; y: Y [B, nv * VEC].  `out` may be `y` itself (R == Y): a thread reads its vector of y before it writes
// the same bytes, and nobody else touches them -- hence no __restrict__ on y and out.
template <typename R, typename Y, int VEC>
__global__ __launch_bounds__(DP_THREADS) void drop_path_fwd_kernel(const R* __restrict__ res, const Y* y, R* out, int64_t B, int64_t nv, float p,
                                                                   float inv_keep, uint64_t seed, uint64_t offset) {
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float s = dropout_scale(seed, offset, (uint64_t)b, p, inv_keep);   // uniform over the workgroup: once per (workgroup, sample)
        const int64_t base = b * nv;
        if (s == 0.0f) {   // dropped: y is not read
            for (int64_t i = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * DP_THREADS)
                Vec<R, VEC>::copy(res + (base + i) * VEC, out + (base + i) * VEC);   // the residual's BITS
        } else {
            for (int64_t i = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * DP_THREADS) {
                float r[VEC], q[VEC];
                Vec<R, VEC>::get(res + (base + i) * VEC, r);
                Vec<Y, VEC>::get(y + (base + i) * VEC, q);
#pragma unroll
                for (int k = 0; k < VEC; ++k) r[k] = fmaf(s, q[k], r[k]);
                Vec<R, VEC>::put(out + (base + i) * VEC, r);
            }
        }
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(DP_THREADS) void drop_path_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dy, int64_t B, int64_t nv, float p,
                                                                   float inv_keep, uint64_t seed, uint64_t offset) {
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float s = dropout_scale(seed, offset, (uint64_t)b, p, inv_keep);
        const int64_t base = b * nv;
        if (s == 0.0f) {   // dropped: dout is not read, +0 is written
            for (int64_t i = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * DP_THREADS)
                Vec<T, VEC>::store(dy + (base + i) * VEC, Vec<T, VEC>::zero());
        } else {
            for (int64_t i = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * DP_THREADS) {
                float g[VEC];
                Vec<T, VEC>::get(dout + (base + i) * VEC, g);
#pragma unroll
                for (int k = 0; k < VEC; ++k) g[k] *= s;
                Vec<T, VEC>::put(dy + (base + i) * VEC, g);
            }
        }
    }
}

// grid: x over a sample's vectors (DP_VEC_PER_THREAD per thread where the sample is long enough), y over samples; when that is more than
// DP_MAX_BLOCKS workgroups the samples are dealt out in whole rounds, so that every workgroup of a column walks the same number of them
dim3 dp_grid(int64_t B, int64_t nv) {
    int64_t gx = (nv + (int64_t)DP_THREADS * DP_VEC_PER_THREAD - 1) / ((int64_t)DP_THREADS * DP_VEC_PER_THREAD);
    if (gx > DP_MAX_BLOCKS) gx = DP_MAX_BLOCKS;
    int64_t gy = B;
    if (B * gx > DP_MAX_BLOCKS) {
        const int64_t cols = DP_MAX_BLOCKS / gx;          // >= 1
        const int64_t rounds = (B + cols - 1) / cols;
        gy = (B + rounds - 1) / rounds;                   // <= cols
    }
    return dim3((unsigned)gx, (unsigned)gy);
}

bool dp_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

float dp_inv_keep(float p) { return (float)(1.0 / (1.0 - (double)p)); }

}  // namespace

extern "C" int ecamp_drop_path_fwd(const void* res, const void* y, void* out, int64_t B, int32_t T, int32_t D, float p, uint64_t seed,
                                   uint64_t offset, int32_t res_dtype, int32_t y_dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(res && y && out, "drop_path_fwd: null pointer");
    ECAMP_CHECK_ARG(B >= 1 && T >= 1 && D >= 1, "drop_path_fwd: B=%lld, T=%d, D=%d must be positive", (long long)B, T, D);
    ECAMP_CHECK_ARG(D % 4 == 0, "drop_path_fwd: D=%d must be a multiple of 4", D);
    ECAMP_CHECK_ARG(p >= 0.0f && p < 1.0f, "drop_path_fwd: p=%g must lie in [0, 1)", (double)p);
    const bool f32f32 = res_dtype == ECAMP_F32 && y_dtype == ECAMP_F32, h16h16 = res_dtype == ECAMP_BF16 && y_dtype == ECAMP_BF16,
               f32h16 = res_dtype == ECAMP_F32 && y_dtype == ECAMP_BF16;
    ECAMP_CHECK_ARG(f32f32 || h16h16 || f32h16,
                    "drop_path_fwd: bad dtype pair (res %d, y %d): 16-bit with 16-bit, f32 with f32, or an f32 residual with a 16-bit branch", res_dtype,
                    y_dtype);
    const int64_t n = B * (int64_t)T * D;
    const int64_t rbytes = n * (res_dtype == ECAMP_F32 ? 4 : 2), ybytes = n * (y_dtype == ECAMP_F32 ? 4 : 2);
    ECAMP_CHECK_ARG(!dp_overlap(out, rbytes, res, rbytes), "drop_path_fwd: illegal aliasing: out overlaps res (the block's input is kept for the backward)");
    ECAMP_CHECK_ARG(!dp_overlap(out, rbytes, y, ybytes) || (out == y && res_dtype == y_dtype),
                    "drop_path_fwd: illegal aliasing: out may be y itself when their dtypes agree, and may not overlap it otherwise");
    const int vec = (D % 8 == 0 && !f32f32) ? 8 : 4;
    const uintptr_t rmask = (res_dtype == ECAMP_BF16 && vec == 4) ? 7 : 15, ymask = (y_dtype == ECAMP_BF16 && vec == 4) ? 7 : 15;
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(out)) & rmask) == 0 && (reinterpret_cast<uintptr_t>(y) & ymask) == 0,
                    "drop_path_fwd: res, y and out must be aligned to their vector width (16 bytes; 8 for 16-bit data when D %% 8 != 0)");
    const float inv_keep = dp_inv_keep(p);
    const int64_t nv = (int64_t)T * D / vec;
    const dim3 grid = dp_grid(B, nv), block(DP_THREADS);
#define L(R_, Y_, V_) hipLaunchKernelGGL((drop_path_fwd_kernel<R_, Y_, V_>), grid, block, 0, stream, (const R_*)res, (const Y_*)y, (R_*)out, B, nv, p, inv_keep, seed, offset)
    if (f32f32) L(float, float, 4);
    else if (h16h16 && vec == 8) L(bf16_t, bf16_t, 8);
    else if (h16h16) L(bf16_t, bf16_t, 4);
    else if (vec == 8) L(float, bf16_t, 8);
    else L(float, bf16_t, 4);
#undef L
    ECAMP_LAUNCH_CHECK();
    return 0;
}

extern "C" int ecamp_drop_path_bwd(const void* dout, void* dy, int64_t B, int32_t T, int32_t D, float p, uint64_t seed, uint64_t offset,
                                   int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(dout && dy, "drop_path_bwd: null pointer");
    ECAMP_CHECK_ARG(B >= 1 && T >= 1 && D >= 1, "drop_path_bwd: B=%lld, T=%d, D=%d must be positive", (long long)B, T, D);
    ECAMP_CHECK_ARG(D % 4 == 0, "drop_path_bwd: D=%d must be a multiple of 4", D);
    ECAMP_CHECK_ARG(p >= 0.0f && p < 1.0f, "drop_path_bwd: p=%g must lie in [0, 1)", (double)p);
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "drop_path_bwd: bad dtype %d", dtype);
    const int64_t bytes = B * (int64_t)T * D * (dtype == ECAMP_F32 ? 4 : 2);
    ECAMP_CHECK_ARG(!dp_overlap(dy, bytes, dout, bytes), "drop_path_bwd: illegal aliasing: dy overlaps dout (dout is still the residual's gradient)");
    const int vec = (D % 8 == 0 && dtype == ECAMP_BF16) ? 8 : 4;
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dy)) & (vec == 4 && dtype == ECAMP_BF16 ? 7 : 15)) == 0,
                    "drop_path_bwd: dout and dy must be aligned to their vector width (16 bytes; 8 for 16-bit data when D %% 8 != 0)");
    const float inv_keep = dp_inv_keep(p);
    const int64_t nv = (int64_t)T * D / vec;
    const dim3 grid = dp_grid(B, nv), block(DP_THREADS);
#define L(T_, V_) hipLaunchKernelGGL((drop_path_bwd_kernel<T_, V_>), grid, block, 0, stream, (const T_*)dout, (T_*)dy, B, nv, p, inv_keep, seed, offset)
    if (dtype == ECAMP_F32) L(float, 4);
    else if (vec == 8) L(bf16_t, 8);
    else L(bf16_t, 4);
#undef L
    ECAMP_LAUNCH_CHECK();
    return 0;
}
