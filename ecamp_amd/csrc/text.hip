// Report-side HBM-bound kernels:
//   BertEmbeddings: word+position+token-type gather-sum -> LayerNorm(eps 1e-12) -> dropout, and its backward
//   (scatter-add into the f32 embedding-table gradients; the PAD row gets none: nn.Embedding(padding_idx=0));
//   weighted cross-entropy over the 30000-way MLM logits with the gradient written in place.
#include "common.h"

// one workgroup per sequence position s, waves stride over the batch -> the position-table gradient row is
// owned by exactly one workgroup (deterministic, no atomics); token-type / hot special-token / LN-affine
// gradients are reduced per workgroup and flushed with one atomic set.
template <typename T, int IT>
__global__ __launch_bounds__(256) void bert_embed_fwd_kernel(const long* __restrict__ ids, const long* __restrict__ type_ids,
                                                             const float* __restrict__ wword, const float* __restrict__ wpos,
                                                             const float* __restrict__ wtype, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, T* __restrict__ z, T* __restrict__ e,
                                                             float* __restrict__ mean, float* __restrict__ rstd, long B, int S,
                                                             int cols, float eps, float drop_p, uint64_t seed, uint64_t offset) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int nv = cols >> 2;
    const float inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    for (long b = (long)blockIdx.y * 4 + wave; b < B; b += (long)gridDim.y * 4) {
        const long row = b * S + s;
        const long id = ids[row], ty = type_ids[row];
        float v[IT][4];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
                float a[4], p[4], t[4];
                ld4<float>(wword + id * cols + c * 4, a);
                ld4<float>(wtype + ty * cols + c * 4, t);
                ld4<float>(wpos + (long)s * cols + c * 4, p);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[i][r] = rnd<T>((a[r] + t[r]) + p[r]);
                st4<T>(z + row * cols + c * 4, v[i]);
                sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[i][r] = 0.f;
            }
        }
        const float mu = wave_sum(sum) / (float)cols;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float d = v[i][r] - mu;
                    q += d * d;
                }
            }
        }
        const float rs = rsqrtf(wave_sum(q) / (float)cols + eps);
        if (lane == 0) {
            mean[row] = mu;
            rstd[row] = rs;
        }
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
                float4 g = *reinterpret_cast<const float4*>(gamma + c * 4);
                float4 bb = *reinterpret_cast<const float4*>(beta + c * 4);
                float o[4] = {(v[i][0] - mu) * rs * g.x + bb.x, (v[i][1] - mu) * rs * g.y + bb.y,
                              (v[i][2] - mu) * rs * g.z + bb.z, (v[i][3] - mu) * rs * g.w + bb.w};
                if (drop_p > 0.f) {
                    float m[4];
                    dropout_scale4(seed, offset, (uint64_t)(row * nv + c), drop_p, inv_keep, m);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] *= m[r];
                }
                st4<T>(e + row * cols + c * 4, o);
            }
        }
    }
}

template <typename T, int IT>
__global__ __launch_bounds__(256) void bert_embed_bwd_kernel(const T* __restrict__ de, const T* __restrict__ z,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const long* __restrict__ ids,
                                                             const long* __restrict__ type_ids, float* __restrict__ gword,
                                                             float* __restrict__ gpos, float* __restrict__ gtype,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, long B, int S,
                                                             int cols, int pad_id, int hot0, int hot1, float drop_p,
                                                             uint64_t seed, uint64_t offset) {
    extern __shared__ __attribute__((aligned(16))) float sh[];  // [4][cols]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int nv = cols >> 2;
    const float inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    // per-lane column partials: 0 dgamma, 1 dbeta, 2 pos row, 3/4 token types 0/1, 5/6 hot ids
    float acc[7][IT][4];
    float gm[IT][4];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[k][i][r] = 0.f;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        int c = lane + 64 * i;
        if (c < nv) ld4<float>(gamma + c * 4, gm[i]);
        else gm[i][0] = gm[i][1] = gm[i][2] = gm[i][3] = 0.f;
    }
    for (long b = (long)blockIdx.y * 4 + wave; b < B; b += 4 * (long)gridDim.y) {   // gridDim.y workgroups share a position
        const long row = b * S + s;
        const long id = ids[row], ty = type_ids[row];
        const float mu = mean[row], rs = rstd[row];
        float xh[IT][4], g[IT][4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
                float d[4], zz[4];
                ld4<T>(de + row * cols + c * 4, d);
                ld4<T>(z + row * cols + c * 4, zz);
                if (drop_p > 0.f) {
                    float m[4];
                    dropout_scale4(seed, offset, (uint64_t)(row * nv + c), drop_p, inv_keep, m);
#pragma unroll
                    for (int r = 0; r < 4; ++r) d[r] *= m[r];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    xh[i][r] = (zz[r] - mu) * rs;
                    g[i][r] = d[r] * gm[i][r];
                    s1 += g[i][r];
                    s2 += g[i][r] * xh[i][r];
                    acc[0][i][r] += d[r] * xh[i][r];
                    acc[1][i][r] += d[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) xh[i][r] = g[i][r] = 0.f;
            }
        }
        s1 = wave_sum(s1) / (float)cols;
        s2 = wave_sum(s2) / (float)cols;
        // A row of an ordinary token goes to its embedding row by atomics.  Issued from the 16-B-per-lane register layout an atomic instruction
        // touches 4 B in each of 64 chunks 16 B apart (eight 128-B lines a quarter full: 165 us per call at B = 256, the atomic units' line rate);
        // passed through this wave's LDS row first, lane l adds element 64 k + l: two full lines per instruction (round 6).
        const bool scatter = id != hot0 && id != hot1 && id != pad_id;   // wave-uniform (one row per wave)
        float* wrow = sh + wave * cols;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
                float dz4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float dz = rs * (g[i][r] - s1 - xh[i][r] * s2);
                    dz4[r] = dz;
                    acc[2][i][r] += dz;
                    if (ty == 0) acc[3][i][r] += dz; else acc[4][i][r] += dz;
                    if (id == hot0) acc[5][i][r] += dz;
                    else if (id == hot1) acc[6][i][r] += dz;
                }
                if (scatter) *reinterpret_cast<float4*>(wrow + c * 4) = make_float4(dz4[0], dz4[1], dz4[2], dz4[3]);
            }
        }
        if (scatter) {
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS writes have landed (the row is private to the wave)
            __builtin_amdgcn_wave_barrier();
            float* dst = gword + id * cols;
            for (int c = lane; c < cols; c += 64) atomicAdd(dst + c, wrow[c]);
            __builtin_amdgcn_wave_barrier();       // the next row's writes stay behind these reads
        }
    }
    for (int k = 0; k < 7; ++k) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            int c = lane + 64 * i;
            if (c < nv) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = k == 0 ? acc[0][i][r] : k == 1 ? acc[1][i][r] : k == 2 ? acc[2][i][r] : k == 3 ? acc[3][i][r]
                              : k == 4 ? acc[4][i][r] : k == 5 ? acc[5][i][r] : acc[6][i][r];
                    sh[wave * cols + c * 4 + r] = v;
                }
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < cols; c += 256) {
            float t = sh[c] + sh[cols + c] + sh[2 * cols + c] + sh[3 * cols + c];
            if (k == 0) atomicAdd(dgamma + c, t);
            else if (k == 1) atomicAdd(dbeta + c, t);
            else if (k == 2) {
                if (gridDim.y == 1) gpos[(long)s * cols + c] += t;  // this workgroup owns position row s
                else atomicAdd(gpos + (long)s * cols + c, t);
            }
            else if (k == 3) atomicAdd(gtype + c, t);
            else if (k == 4) { if (t != 0.f) atomicAdd(gtype + cols + c, t); }
            else if (k == 5) { if (hot0 != pad_id && t != 0.f) atomicAdd(gword + (long)hot0 * cols + c, t); }
            else { if (hot1 != pad_id && t != 0.f) atomicAdd(gword + (long)hot1 * cols + c, t); }
        }
    }
}

extern "C" int ecamp_bert_embed_fwd(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos,
                                    const float* type, const float* gamma, const float* beta, void* z, void* e, float* mean,
                                    float* rstd, int64_t B, int32_t S, int32_t cols, float eps, float drop_p, uint64_t seed,
                                    uint64_t offset, int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(ids && type_ids && word && pos && type && gamma && beta && z && e && mean && rstd, "bert_embed_fwd: null pointer");
    ECAMP_CHECK_ARG(cols % 4 == 0 && cols <= 1024, "bert_embed_fwd: cols=%d must be a multiple of 4 and <= 1024", cols);
    int gy = (int)((B + 3) / 4);
    if (gy > 16) gy = 16;
    dim3 grid(S, gy), block(256);
    const int it = ceil_div(cols / 4, 64);
#define L(T_, IT_) hipLaunchKernelGGL((bert_embed_fwd_kernel<T_, IT_>), grid, block, 0, stream, (const long*)ids, (const long*)type_ids, word, pos, type, gamma, beta, (T_*)z, (T_*)e, mean, rstd, (long)B, S, cols, eps, drop_p, seed, offset)
    return ECAMP_LAUNCH_TYPED("bert_embed_fwd", dtype, [&](auto tag) {
        typedef ECAMP_TAG_T(tag) T;
        if (it <= 1) L(T, 1); else if (it <= 2) L(T, 2); else if (it <= 3) L(T, 3); else L(T, 4);
    });
#undef L
}

extern "C" int ecamp_bert_embed_bwd(const void* de, const void* z, const float* mean, const float* rstd, const float* gamma,
                                    const int64_t* ids, const int64_t* type_ids, float* gword, float* gpos, float* gtype,
                                    float* dgamma, float* dbeta, int64_t B, int32_t S, int32_t cols, int32_t pad_id,
                                    int32_t hot0, int32_t hot1, float drop_p, uint64_t seed, uint64_t offset, int32_t dtype,
                                    hipStream_t stream) {
    ECAMP_CHECK_ARG(de && z && mean && rstd && gamma && ids && type_ids && gword && gpos && gtype && dgamma && dbeta, "bert_embed_bwd: null pointer");
    ECAMP_CHECK_ARG(cols % 4 == 0 && cols <= 1024, "bert_embed_bwd: cols=%d must be a multiple of 4 and <= 1024", cols);
    // S workgroups alone leave half of the 256 CUs idle at S = 128: split the batch over gridDim.y workgroups per position
    int gy = (int)(B / 32);
    if (gy < 1) gy = 1;
    if (gy > 8) gy = 8;
    dim3 grid(S, gy), block(256);
    size_t shm = (size_t)4 * cols * sizeof(float);
    const int it = ceil_div(cols / 4, 64);
#define L(T_, IT_) hipLaunchKernelGGL((bert_embed_bwd_kernel<T_, IT_>), grid, block, shm, stream, (const T_*)de, (const T_*)z, mean, rstd, gamma, (const long*)ids, (const long*)type_ids, gword, gpos, gtype, dgamma, dbeta, (long)B, S, cols, pad_id, hot0, hot1, drop_p, seed, offset)
    return ECAMP_LAUNCH_TYPED("bert_embed_bwd", dtype, [&](auto tag) {
        typedef ECAMP_TAG_T(tag) T;
        if (it <= 1) L(T, 1); else if (it <= 2) L(T, 2); else if (it <= 3) L(T, 3); else L(T, 4);
    });
#undef L
}

// ---------------------------------------------------------------------------------------------
// weighted cross-entropy (bert_modeling.py:213-217): loss = mean_i( CE(logits_i, label_i) * w_i ) over ALL rows.
// One workgroup per row: pass 1 online max / sum-exp, pass 2 writes d loss / d logits in place:
//   dlogits[i, j] = w_i / M * (softmax_ij - [j == label_i])       loss_sum += w_i * (lse_i - logit[i, label_i])
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_bwd_kernel(T* __restrict__ logits, const long* __restrict__ labels,
                                                         const float* __restrict__ weights, float* __restrict__ loss_sum, int V,
                                                         long ld, float inv_count) {
    __shared__ float shm_[8];
    const long row = blockIdx.x;
    T* x = logits + row * ld;
    const int nv = V >> 2;
    float mx = -INFINITY, sm = 0.f;
    for (int c = threadIdx.x; c < nv; c += 256) {
        float p[4];
        ld4<T>(x + c * 4, p);
        float m4 = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3]));
        if (m4 > mx) {
            sm *= __expf(mx - m4);
            mx = m4;
        }
        sm += __expf(p[0] - mx) + __expf(p[1] - mx) + __expf(p[2] - mx) + __expf(p[3] - mx);
    }
    // block combine of (max, sum)
    float wm = wave_max(mx);
    sm = mx == -INFINITY ? 0.f : sm * __expf(mx - wm);   // a lane (or a whole wave) without elements: exp(-inf + inf) would be NaN
    sm = wave_sum(sm);
    if ((threadIdx.x & 63) == 0) {
        shm_[threadIdx.x >> 6] = wm;
        shm_[4 + (threadIdx.x >> 6)] = sm;
    }
    __syncthreads();
    float gmx = fmaxf(fmaxf(shm_[0], shm_[1]), fmaxf(shm_[2], shm_[3]));
    float gsm = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) gsm += shm_[k] == -INFINITY ? 0.f : shm_[4 + k] * __expf(shm_[k] - gmx);
    // a label outside [0, V) -- CrossEntropyLoss's ignore_index -100 (bert_modeling.py:212) -- contributes no loss and a zero
    // gradient row, and is never used as an index
    const long label = labels[row];
    const bool ign = label < 0 || label >= (long)V;
    const float w = ign ? 0.f : weights[row];
    if (threadIdx.x == 0 && !ign) {
        float lse = gmx + __logf(gsm);
        atomicAdd(loss_sum, w * (lse - to_f<T>(x[label])));
    }
    const float inv = 1.0f / gsm, sc = w * inv_count;
    __syncthreads();
    for (int c = threadIdx.x; c < nv; c += 256) {
        float p[4];
        ld4<T>(x + c * 4, p);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sftm = __expf(p[r] - gmx) * inv;
            p[r] = sc * (sftm - ((long)(c * 4 + r) == label ? 1.0f : 0.0f));
        }
        st4<T>(x + c * 4, p);
    }
}
// bf16 rows of up to 32768 logits: the row is read ONCE into registers (16 B per lane per load) and the gradient is written from them --
// the two-pass kernel above reads every logit twice (2 GB per pass at B*S = 32768, V = 30000).  THREE phases with ONE exp per logit (a
// single pass that evaluates two and rescales a running sum whenever its maximum moves spends ~570 us of VALU time per 1.97 GB of logits
// against the ~500 us a pure read + write of them takes, profiles/r05_vocab_head.txt).  NT threads per row, NG 16-B loads per thread
// (V <= 8 NG NT):
//   1  load the row, maximum                                        -> block maximum
//   2  e = exp(x - max) kept in f32 registers over the loaded row, sum  -> block sum
//   3  d = e * (w / (M sum)), minus w / M at the label, packed, stored over the logits
// Lanes past the row hold -inf: they drop out of the maximum and add exp(-inf) = 0.  Measured directly behind the vocabulary GEMM
// (tools/vocab_head_probe.py, V = 30000): the two-exp single pass 1.33x the time of an in-place multiply over the same bytes, this one with 512
// threads x 8 loads 1.25x, with 1024 x 4 (one row's 120 KB of e spread over all sixteen waves a CU's SIMDs take at 66 registers) 1.20-1.23x;
// forms that keep the row packed and evaluate exp twice (fewer registers, more rows per CU) 1.25-1.33x.
template <int NG, int NT>
__global__ __launch_bounds__(NT) void ce_fwd_bwd_row_kernel(bf16_t* __restrict__ logits, const long* __restrict__ labels,
                                                            const float* __restrict__ weights, float* __restrict__ loss_sum, int V,
                                                            long ld, float inv_count) {
    constexpr int NWV = NT / 64;
    __shared__ float shm_[2 * NWV];
    const long row = blockIdx.x;
    bf16_t* x = logits + row * ld;
    const int nv8 = V >> 3, wave = threadIdx.x >> 6;
    uint4 q[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int c = threadIdx.x + NT * j;
        q[j] = c < nv8 ? *reinterpret_cast<const uint4*>(x + c * 8) : make_uint4(H16_NEG_INF_X2, H16_NEG_INF_X2, H16_NEG_INF_X2, H16_NEG_INF_X2);
    }
    float e[NG][8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[j][2 * r] = h16_lo(w[r]);
            e[j][2 * r + 1] = h16_hi(w[r]);
            mx = fmaxf(mx, fmaxf(e[j][2 * r], e[j][2 * r + 1]));
        }
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) shm_[wave] = mx;
    __syncthreads();
    float gmx = shm_[0];
#pragma unroll
    for (int k = 1; k < NWV; ++k) gmx = fmaxf(gmx, shm_[k]);
    const long label = labels[row];
    const bool ign = label < 0 || label >= (long)V;   // ignore_index (see the generic kernel)
    const float w = ign ? 0.f : weights[row];
    const float xl = (threadIdx.x == 0 && !ign) ? to_f<bf16_t>(x[label]) : 0.f;   // read before anyone overwrites the row (barrier below)
    constexpr float LOG2E = 1.4426950408889634f;
    const float nb = -gmx * LOG2E;
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            e[j][r] = __builtin_amdgcn_exp2f(fmaf(e[j][r], LOG2E, nb));
            sm += e[j][r];
        }
    sm = wave_sum(sm);
    if ((threadIdx.x & 63) == 0) shm_[NWV + wave] = sm;
    __syncthreads();
    float gsm = 0.f;
#pragma unroll
    for (int k = 0; k < NWV; ++k) gsm += shm_[NWV + k];
    if (threadIdx.x == 0 && !ign) atomicAdd(loss_sum, w * (gmx + __logf(gsm) - xl));
    const float sc = w * inv_count, f = sc / gsm;
    const int lg = ign ? -1 : (int)(label >> 3), lr = (int)(label & 7);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int c = threadIdx.x + NT * j;
        if (c < nv8) {
            float g[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) g[r] = e[j][r] * f;
            if (c == lg) {
#pragma unroll
                for (int r = 0; r < 8; ++r) g[r] -= r == lr ? sc : 0.f;
            }
            uint4 o;
            o.x = pack_bf16x2(g[0], g[1]); o.y = pack_bf16x2(g[2], g[3]); o.z = pack_bf16x2(g[4], g[5]); o.w = pack_bf16x2(g[6], g[7]);
            *reinterpret_cast<uint4*>(x + c * 8) = o;
        }
    }
}
extern "C" int ecamp_ce_fwd_bwd(void* logits, const int64_t* labels, const float* weights, float* loss_sum, int64_t M, int32_t V,
                                int64_t ld, float inv_count, int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(logits && labels && weights && loss_sum, "ce_fwd_bwd: null pointer");
    ECAMP_CHECK_ARG(V > 0 && V % 4 == 0 && ld % 4 == 0 && ld >= V, "ce_fwd_bwd: V=%d and ld=%ld must be multiples of 4 (ld >= V > 0)", V, (long)ld);
    ECAMP_CHECK_ARG(M >= 0 && M <= 0x7fffffffLL, "ce_fwd_bwd: M=%ld rows do not fit one launch", (long)M);
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "ce_fwd_bwd: dtype %d", dtype);
    if (M == 0) return 0;
    dim3 grid((unsigned)M), block(256);
    if (dtype == ECAMP_BF16 && V % 8 == 0 && ld % 8 == 0 && V <= 32768 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0) {
#define CE_ROW(NG_, NT_) hipLaunchKernelGGL((ce_fwd_bwd_row_kernel<NG_, NT_>), grid, dim3(NT_), 0, stream, (bf16_t*)logits, (const long*)labels, weights, loss_sum, V, (long)ld, inv_count)
        if (V <= 4096) CE_ROW(1, 512); else if (V <= 8192) CE_ROW(2, 512); else if (V <= 16384) CE_ROW(4, 512); else CE_ROW(4, 1024);
#undef CE_ROW
        ECAMP_LAUNCH_CHECK();
        return 0;
    }
    if (dtype == ECAMP_F32) hipLaunchKernelGGL(ce_fwd_bwd_kernel<float>, grid, block, 0, stream, (float*)logits, (const long*)labels, weights, loss_sum, V, (long)ld, inv_count);
    else hipLaunchKernelGGL(ce_fwd_bwd_kernel<bf16_t>, grid, block, 0, stream, (bf16_t*)logits, (const long*)labels, weights, loss_sum, V, (long)ld, inv_count);
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Held-out evaluation of the MLM head: the same weighted cross-entropy WITHOUT its gradient, plus what a validation pass reports --
// how many rows were scored and whether the label ranks first / within the first five.  Read-only on the logits, one workgroup per row:
//   label outside [0, V) (ignore_index -100): the workgroup returns after reading the label -- the row's logits are never touched
//   xl = logit[label]      loss_sum += w (logsumexp(row) - xl)      rank = #{ j : logit[j] > xl }  (strictly: a label tied with the
//   maximum is correct)    counts[0] += 1    counts[1] += rank == 0    counts[2] += rank < 5       (64-bit integer atomics: exact)
// Against ecamp_ce_fwd_bwd: no write of [M, V], and at the reference's masking rate only the ~15 % of rows that carry a label are read.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void ce_eval_flush(float* loss_sum, unsigned long long* counts, float loss, int rank) {
    atomicAdd(loss_sum, loss);
    atomicAdd(counts, 1ull);
    if (rank == 0) atomicAdd(counts + 1, 1ull);
    if (rank < 5) atomicAdd(counts + 2, 1ull);
}
// 16-bit rows of up to 32768 logits, the row held in registers as in ce_fwd_bwd_row_kernel (NT threads, NG 16-B loads per thread, lanes
// past the row hold -inf): maximum and the strictly-greater count from the registers, then ONE exp2 per logit for the sum.
template <int NG, int NT>
__global__ __launch_bounds__(NT) void ce_eval_row_kernel(const bf16_t* __restrict__ logits, const long* __restrict__ labels,
                                                         const float* __restrict__ weights, float* __restrict__ loss_sum,
                                                         unsigned long long* __restrict__ counts, int V, long ld) {
    constexpr int NWV = NT / 64;
    __shared__ float shm_[2 * NWV];
    __shared__ int shc_[NWV];
    const long row = blockIdx.x;
    const long label = labels[row];
    if (label < 0 || label >= (long)V) return;   // uniform over the workgroup, ahead of every barrier
    const bf16_t* x = logits + row * ld;
    const int nv8 = V >> 3, wave = threadIdx.x >> 6;
    uint4 q[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int c = threadIdx.x + NT * j;
        q[j] = c < nv8 ? *reinterpret_cast<const uint4*>(x + c * 8) : make_uint4(H16_NEG_INF_X2, H16_NEG_INF_X2, H16_NEG_INF_X2, H16_NEG_INF_X2);
    }
    const float xl = to_f<bf16_t>(x[label]);   // one address for the whole wave: a single broadcast load
    float mx = -INFINITY;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = h16_lo(w[r]), b = h16_hi(w[r]);
            mx = fmaxf(mx, fmaxf(a, b));
            cnt += (a > xl ? 1 : 0) + (b > xl ? 1 : 0);
        }
    }
    mx = wave_max(mx);
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) {
        shm_[wave] = mx;
        shc_[wave] = cnt;
    }
    __syncthreads();
    float gmx = shm_[0];
#pragma unroll
    for (int k = 1; k < NWV; ++k) gmx = fmaxf(gmx, shm_[k]);
    constexpr float LOG2E = 1.4426950408889634f;
    const float nb = -gmx * LOG2E;
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
            sm += __builtin_amdgcn_exp2f(fmaf(h16_lo(w[r]), LOG2E, nb)) + __builtin_amdgcn_exp2f(fmaf(h16_hi(w[r]), LOG2E, nb));
    }
    sm = wave_sum(sm);
    if ((threadIdx.x & 63) == 0) shm_[NWV + wave] = sm;
    __syncthreads();
    if (threadIdx.x == 0) {
        float gsm = 0.f;
        int rank = 0;
#pragma unroll
        for (int k = 0; k < NWV; ++k) {
            gsm += shm_[NWV + k];
            rank += shc_[k];
        }
        ce_eval_flush(loss_sum, counts, weights[row] * (gmx + __logf(gsm) - xl), rank);
    }
}
// everything else (f32; 16-bit rows the kernel above refuses: V > 32768, V % 8 != 0, a base that is not 16-B aligned): one pass with a
// running (maximum, sum) per lane as in ce_fwd_bwd_kernel -- the label's logit is known before the pass, so the count rides along.
template <typename T>
__global__ __launch_bounds__(256) void ce_eval_kernel(const T* __restrict__ logits, const long* __restrict__ labels,
                                                      const float* __restrict__ weights, float* __restrict__ loss_sum,
                                                      unsigned long long* __restrict__ counts, int V, long ld) {
    __shared__ float shm_[8];
    __shared__ int shc_[4];
    const long row = blockIdx.x;
    const long label = labels[row];
    if (label < 0 || label >= (long)V) return;
    const T* x = logits + row * ld;
    const int nv = V >> 2;
    const float xl = to_f<T>(x[label]);
    float mx = -INFINITY, sm = 0.f;
    int cnt = 0;
    for (int c = threadIdx.x; c < nv; c += 256) {
        float p[4];
        ld4<T>(x + c * 4, p);
        const float m4 = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3]));
        if (m4 > mx) {
            sm *= __expf(mx - m4);
            mx = m4;
        }
        sm += __expf(p[0] - mx) + __expf(p[1] - mx) + __expf(p[2] - mx) + __expf(p[3] - mx);
        cnt += (p[0] > xl ? 1 : 0) + (p[1] > xl ? 1 : 0) + (p[2] > xl ? 1 : 0) + (p[3] > xl ? 1 : 0);
    }
    const float wm = wave_max(mx);
    sm = mx == -INFINITY ? 0.f : sm * __expf(mx - wm);   // a lane (or a whole wave) without elements: exp(-inf + inf) would be NaN
    sm = wave_sum(sm);
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) {
        shm_[threadIdx.x >> 6] = wm;
        shm_[4 + (threadIdx.x >> 6)] = sm;
        shc_[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float gmx = fmaxf(fmaxf(shm_[0], shm_[1]), fmaxf(shm_[2], shm_[3]));
        float gsm = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) gsm += shm_[k] == -INFINITY ? 0.f : shm_[4 + k] * __expf(shm_[k] - gmx);
        ce_eval_flush(loss_sum, counts, weights[row] * (gmx + __logf(gsm) - xl), shc_[0] + shc_[1] + shc_[2] + shc_[3]);
    }
}
extern "C" int ecamp_ce_eval(const void* logits, const int64_t* labels, const float* weights, float* loss_sum, int64_t* counts, int64_t M,
                             int32_t V, int64_t ld, int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(logits && labels && weights && loss_sum && counts, "ce_eval: null pointer");
    ECAMP_CHECK_ARG(V > 0 && V % 4 == 0 && ld % 4 == 0 && ld >= V, "ce_eval: V=%d and ld=%ld must be multiples of 4 (ld >= V > 0)", V, (long)ld);
    ECAMP_CHECK_ARG(M >= 0 && M <= 0x7fffffffLL, "ce_eval: M=%ld rows do not fit one launch", (long)M);
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "ce_eval: dtype %d", dtype);
    if (M == 0) return 0;
    dim3 grid((unsigned)M);
    unsigned long long* cn = reinterpret_cast<unsigned long long*>(counts);
    if (dtype == ECAMP_BF16 && V % 8 == 0 && ld % 8 == 0 && V <= 32768 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0) {
#define CE_EVAL(NG_, NT_) hipLaunchKernelGGL((ce_eval_row_kernel<NG_, NT_>), grid, dim3(NT_), 0, stream, (const bf16_t*)logits, (const long*)labels, weights, loss_sum, cn, V, (long)ld)
        if (V <= 4096) CE_EVAL(1, 512); else if (V <= 8192) CE_EVAL(2, 512); else if (V <= 16384) CE_EVAL(4, 512); else CE_EVAL(4, 1024);
#undef CE_EVAL
    } else if (dtype == ECAMP_F32) {
        hipLaunchKernelGGL(ce_eval_kernel<float>, grid, dim3(256), 0, stream, (const float*)logits, (const long*)labels, weights, loss_sum, cn, V, (long)ld);
    } else {
        hipLaunchKernelGGL(ce_eval_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)logits, (const long*)labels, weights, loss_sum, cn, V, (long)ld);
    }
    ECAMP_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Row compaction in front of the evaluation head: a held-out pass scores 15-30 % of the B*S positions (the [MASK]ed ones), and the
// transform, the 30000-way decoder and ce_eval need only those rows.  Row m is SCORED iff 0 <= labels[m] < V and (ids == NULL or
// ids[m] == mask_id); the scored rows of x (with label, weight and source index) move to the front of the outputs in increasing m,
// output rows [count, cap) are padding (zeros, label -100, weight 0, index -1) and nothing at or beyond row `cap` is written.
// Deterministic and order-preserving without atomics and without one workgroup waiting for another: three launches over segments of
// COMPACT_SEG rows --
//   1  compact_count_kernel   counts[s]  = scored rows of segment s (one ballot + popcount per wave)
//   2  compact_sums_kernel    sums[u]    = sum of the COMPACT_SUP counts of super-segment u (64-bit: M reaches 2^31 - 1)
//   3  compact_gather_kernel  workgroup s < nseg: base = sums before its super-segment + counts before it inside it, then its scored
//                             rows move in 16-byte pieces, consecutive lanes on consecutive pieces of one row;
//                             workgroups from nseg on: the padding, in pieces of 64 output rows; the first of them writes count_out
// ws: int32 counts[nseg] (padded to 16 bytes), int64 sums[nsup].
// ---------------------------------------------------------------------------------------------
constexpr int COMPACT_SEG = 256, COMPACT_SUP = 1024, COMPACT_FILL = 64;
__device__ __forceinline__ long wave_sum_l(long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block sum for blockDim.x == 256; `sh` holds 4 longs.  All threads get the sum.
__device__ __forceinline__ long block_sum_l_256(long v, long* sh) {
    v = wave_sum_l(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ bool compact_scored(const long* __restrict__ labels, const long* __restrict__ ids, long mask_id, long m, long M, int V) {
    if (m >= M) return false;
    const long label = labels[m];
    return label >= 0 && label < (long)V && (ids == nullptr || ids[m] == mask_id);
}
__global__ __launch_bounds__(256) void compact_count_kernel(const long* __restrict__ labels, const long* __restrict__ ids, long mask_id,
                                                            long M, int V, int* __restrict__ counts) {
    __shared__ int shc_[4];
    const long m = (long)blockIdx.x * COMPACT_SEG + threadIdx.x;
    const unsigned long long b = __ballot(compact_scored(labels, ids, mask_id, m, M, V));
    if ((threadIdx.x & 63) == 0) shc_[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = shc_[0] + shc_[1] + shc_[2] + shc_[3];
}
__global__ __launch_bounds__(256) void compact_sums_kernel(const int* __restrict__ counts, long nseg, long* __restrict__ sums) {
    __shared__ long shl_[4];
    const long s0 = (long)blockIdx.x * COMPACT_SUP;
    long v = 0;
    for (int k = threadIdx.x; k < COMPACT_SUP; k += 256)
        if (s0 + k < nseg) v += counts[s0 + k];
    v = block_sum_l_256(v, shl_);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}
// 16-byte pieces [0, n * nchunk) of n rows over 256 threads: thread t starts at piece t and advances by 256, kept as (row, piece in row)
// so that no index is formed that a long row could overflow
struct CompactCursor {
    int r, c, dr, dc;
    __device__ __forceinline__ CompactCursor(int nchunk) : r(threadIdx.x / nchunk), c(threadIdx.x % nchunk), dr(256 / nchunk), dc(256 % nchunk) {}
    __device__ __forceinline__ void next(int nchunk) {
        r += dr;
        c += dc;
        if (c >= nchunk) {
            c -= nchunk;
            ++r;
        }
    }
};
__global__ __launch_bounds__(256) void compact_gather_kernel(const char* __restrict__ x, long row_bytes_in, const long* __restrict__ labels,
                                                             const float* __restrict__ weights, const long* __restrict__ ids, long mask_id,
                                                             long M, int V, int nchunk, long cap, long nseg, long nsup,
                                                             const int* __restrict__ counts, const long* __restrict__ sums,
                                                             char* __restrict__ x_out, long* __restrict__ labels_out,
                                                             float* __restrict__ weights_out, int* __restrict__ rows_out,
                                                             long* __restrict__ count_out) {
    __shared__ long shl_[4];
    __shared__ int shc_[4];
    __shared__ int src_[COMPACT_SEG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row_bytes = (long)nchunk * 16;
    if ((long)blockIdx.x >= nseg) {
        // padding: the total is the sum of every super-segment
        long v = 0;
        for (long u = threadIdx.x; u < nsup; u += 256) v += sums[u];
        const long count = block_sum_l_256(v, shl_);
        if ((long)blockIdx.x == nseg && threadIdx.x == 0) count_out[0] = count;
        const long nfill = (cap + COMPACT_FILL - 1) / COMPACT_FILL;
        for (long j = (long)blockIdx.x - nseg; j < nfill; j += (long)gridDim.x - nseg) {
            const long first = j * COMPACT_FILL;
            const long lo = count > first ? count : first, hi = first + COMPACT_FILL < cap ? first + COMPACT_FILL : cap;
            if (lo >= hi) continue;
            const int n = (int)(hi - lo);
            if ((int)threadIdx.x < n) {
                labels_out[lo + threadIdx.x] = -100;
                weights_out[lo + threadIdx.x] = 0.f;
                rows_out[lo + threadIdx.x] = -1;
            }
            for (CompactCursor p(nchunk); p.r < n; p.next(nchunk))
                *reinterpret_cast<uint4*>(x_out + (lo + p.r) * row_bytes + (long)p.c * 16) = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }
    const long seg = blockIdx.x, sup = seg / COMPACT_SUP;
    long v = 0;
    for (long u = threadIdx.x; u < sup; u += 256) v += sums[u];
    for (long s = sup * COMPACT_SUP + threadIdx.x; s < seg; s += 256) v += counts[s];
    const long base = block_sum_l_256(v, shl_);
    if (base >= cap) return;   // uniform over the workgroup: every row of this segment lies beyond the capacity
    const long m = seg * COMPACT_SEG + threadIdx.x;
    const bool scored = compact_scored(labels, ids, mask_id, m, M, V);
    const unsigned long long b = __ballot(scored);
    if (lane == 0) shc_[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));   // scored rows in front of this one: in its wave, then in the waves before it
    for (int k = 0; k < wave; ++k) before += shc_[k];
    const int total = shc_[0] + shc_[1] + shc_[2] + shc_[3];
    const int n = base + total <= cap ? total : (int)(cap - base);   // rows of this segment that fit
    if (scored && before < n) {
        src_[before] = threadIdx.x;
        labels_out[base + before] = labels[m];
        weights_out[base + before] = weights[m];
        rows_out[base + before] = (int)m;
    }
    __syncthreads();
    for (CompactCursor p(nchunk); p.r < n; p.next(nchunk)) {
        const long from = seg * COMPACT_SEG + src_[p.r];
        *reinterpret_cast<uint4*>(x_out + (base + p.r) * row_bytes + (long)p.c * 16) =
            *reinterpret_cast<const uint4*>(x + from * row_bytes_in + (long)p.c * 16);
    }
}
static void compact_layout(int64_t M, int64_t* nseg, int64_t* nsup, int64_t* counts_bytes) {
    *nseg = (M + COMPACT_SEG - 1) / COMPACT_SEG;
    *nsup = (*nseg + COMPACT_SUP - 1) / COMPACT_SUP;
    if (*nsup < 1) *nsup = 1;
    *counts_bytes = (*nseg * 4 + 15) / 16 * 16;
}
extern "C" int64_t ecamp_compact_rows_workspace_bytes(int64_t M) {
    if (M < 0 || M > 0x7fffffffLL) return ecamp_set_error(-1, "compact_rows_workspace_bytes: M=%ld outside [0, 2^31 - 1]", (long)M);
    int64_t nseg, nsup, cb;
    compact_layout(M, &nseg, &nsup, &cb);
    return cb + nsup * 8;
}
extern "C" int ecamp_compact_rows(const void* x, int64_t ldx, const int64_t* labels, const float* weights, const int64_t* ids,
                                  int64_t mask_id, int64_t M, int32_t cols, int32_t V, int64_t cap, void* x_out, int64_t* labels_out,
                                  float* weights_out, int32_t* rows_out, int64_t* count_out, void* ws, int32_t dtype, hipStream_t stream) {
    ECAMP_CHECK_ARG(x && labels && weights && x_out && labels_out && weights_out && rows_out && count_out && ws, "compact_rows: null pointer");
    ECAMP_CHECK_ARG(dtype == ECAMP_F32 || dtype == ECAMP_BF16, "compact_rows: dtype %d", dtype);
    ECAMP_CHECK_ARG(M >= 0 && M <= 0x7fffffffLL && cap >= 0 && cap <= 0x7fffffffLL, "compact_rows: M=%ld, cap=%ld outside [0, 2^31 - 1]", (long)M, (long)cap);
    ECAMP_CHECK_ARG(cols > 0 && V > 0 && ldx >= cols, "compact_rows: cols=%d, V=%d, ldx=%ld (ldx >= cols > 0, V > 0)", cols, V, (long)ldx);
    const int64_t es = dtype == ECAMP_F32 ? 4 : 2;
    ECAMP_CHECK_ARG((cols * es) % 16 == 0 && (ldx * es) % 16 == 0, "compact_rows: cols=%d, ldx=%ld of %d-byte elements: a row and the row stride must be multiples of 16 bytes", cols, (long)ldx, (int)es);
    ECAMP_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_out) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0, "compact_rows: x, x_out and ws must be 16-byte aligned");
    int64_t nseg, nsup, cb;
    compact_layout(M, &nseg, &nsup, &cb);
    int* counts = reinterpret_cast<int*>(ws);
    long* sums = reinterpret_cast<long*>(reinterpret_cast<char*>(ws) + cb);
    if (nseg > 0) {
        hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nseg), dim3(256), 0, stream, (const long*)labels, (const long*)ids, (long)mask_id, (long)M, V, counts);
        ECAMP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(compact_sums_kernel, dim3((unsigned)nsup), dim3(256), 0, stream, counts, (long)nseg, sums);
    ECAMP_LAUNCH_CHECK();
    int64_t nfill = (cap + COMPACT_FILL - 1) / COMPACT_FILL;   // padding workgroups stride over the 64-row pieces: the grid stays below 2^32 threads
    nfill = nfill < 1 ? 1 : nfill > 4096 ? 4096 : nfill;        // (at least one: the first of them also writes count_out)
    hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)(nseg + nfill)), dim3(256), 0, stream, (const char*)x, (long)(ldx * es), (const long*)labels,
                       weights, (const long*)ids, (long)mask_id, (long)M, V, (int)(cols * es / 16), (long)cap, (long)nseg, (long)nsup, counts, sums,
                       (char*)x_out, (long*)labels_out, weights_out, (int*)rows_out, (long*)count_out);
    ECAMP_LAUNCH_CHECK();
    return 0;
}
