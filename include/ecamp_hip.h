/* libecamp_hip.so -- C ABI of the MI355X-native ECAMP pre-training hot path.
 *
 * The reference (ToniChopp/ECAMP) is 100 % Python: it has NO native interface to mirror.
 * Each entry point below therefore cites the reference *Python call site* whose ATen/cuDNN/cuBLAS kernels it
 * replaces (paths relative to ECAMP/Pre-training/).  Conventions:
 *   - raw device pointers + explicit sizes / element strides; dtype enum 0 = f32, 1 = bf16 (storage of activations);
 *     parameters, LayerNorm statistics, losses and all parameter gradients are always f32
 *   - every call only ENQUEUES work on `stream` (never synchronises, never allocates, never frees)
 *   - returns 0 on success, <0 on argument errors, >0 = hipError_t; message via ecamp_last_error() (thread-local)
 *   - parameter-gradient outputs ACCUMULATE (+=) into the caller's f32 buffers (gradient accumulation,
 *     main_pretrain.py:147-153); activation-gradient outputs are overwritten
 *   - dropout is a Philox4x32-7 stream keyed by (seed, offset, element index >> 3; one 16-bit draw per element): backward regenerates the mask
 */
#ifndef ECAMP_HIP_H
#define ECAMP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ecampStream_t; /* == hipStream_t */

#define ECAMP_F32 0
#define ECAMP_BF16 1

/* Bumped whenever an exported signature changes (2: ecamp_wgrad_group gained table_bytes, ecamp_gemm_fp8 its q8_* arguments;
 * 3: round 5 -- ecamp_dropout_mask, ecamp_prof_dump, ecamp_fp8_roll's amax history and margin; 4: round 6 -- ecamp_adamw_grouped's
 * `ctl`, ecamp_loss_scale_update, ecamp_half_format, the resample entry points; 5: the f32 residual stream -- ecamp_gemm_res32,
 * ecamp_layernorm_fwd_x32, ecamp_layernorm_bwd_z32, ecamp_assemble_tokens_x32, ecamp_unshuffle_fwd_x32).  ecamp_abi_version()
 * returns the value the library was BUILT with; a consumer compares it with the header it was compiled against -- the Python binding
 * (ecamp_amd/_lib.py) refuses a library of another version, which is what protects an A/B of two builds (ECAMP_LIB, tools/ab_lib.sh)
 * from calling an older build with a newer argument list.  ecamp_ce_eval -- and later ecamp_drop_path_fwd / ecamp_drop_path_bwd, ecamp_pos_embed_grad,
 * ecamp_resample_boxes_u8 (+ its workspace function), ecamp_im2col_u8, ecamp_resample_boxes_rgb_u8, ecamp_layernorm_layout and
 * ecamp_resample_shard_u8 -- were
 * ADDED at version 5 without touching an existing signature: a build that lacks them is refused by the binding all the same, which
 * resolves every declared symbol when it loads. */
#define ECAMP_ABI_VERSION 5
int ecamp_abi_version(void);
const char* ecamp_last_error(void);
/* The 16-bit activation format of THIS build -- what dtype code ECAMP_BF16 (1) stores.  0: bfloat16 (libecamp_hip.so, the benchmarked
 * mode).  1: IEEE half (libecamp_hip_f16.so: the same sources compiled with -DECAMP_HALF_F16), the format the reference's
 * torch.cuda.amp.autocast() computes its linear layers and attention products in (main_pretrain.py:139, engine_pretrain.py:44); it is
 * run with dynamic loss scaling (util/misc.py:251-271).  Accumulation, LayerNorm / softmax statistics, losses, parameters and their
 * gradients are f32 in both.  The e4m3 forward (ecamp_gemm_fp8 and its producers) exists in the bfloat16 build only. */
int ecamp_half_format(void);

/* ---- dense contractions -------------------------------------------------------------------------------------
 * C[M,N] (+)= epi( alpha * (alpha_dev ? *alpha_dev : 1) * sum_k opA[m,k] opB[k,n] ); a_kc/b_kc = operand is contiguous along the contraction.
 * Replaces every nn.Linear / Conv2d-as-GEMM on the path: timm PatchEmbed.proj (model_ecamp.py:60,220), Block
 * qkv/proj/fc1/fc2 (:66-68,80-82,233-234,254-255), decoder_embed/pred (:74,85,242,259), bert_mlp (:99,268), HF
 * Bert* dense layers (bert_modeling.py:113-131, context_fusion.py:32-72), MLM decoder (bert_modeling.py:209), and
 * their autograd dgrad/wgrad.  Epilogue: +bias[n]; save pre-activation; exact-erf GELU; *gelu'(gmul[m,n]);
 * +residual[m,n].  act: 0 none; 1 GELU (pre_out, if given, receives the pre-activation; gmul holds a pre-activation and the
 * result is multiplied by gelu'(gmul)); 2 (bf16 only) GELU with the SAVED DERIVATIVE: pre_out receives gelu'(pre-activation)
 * and, in the data-gradient call, gmul holds that derivative and multiplies the result as it is -- torch's GeluBackward
 * (nn.GELU at timm Mlp.act / HF BertIntermediate.intermediate_act_fn) without erf / exp in the backward pass, at the price of
 * one more bf16 rounding of the derivative.  out_f32/accumulate: f32 output added into C (weight gradients).  split_k > 1: the contraction is cut
 * into slabs written to `splitk_ws` (split_k*M*N floats) and combined by a deterministic reduce kernel (no atomics).
 * rowsum (optional, f32 [M]): rowsum[m] += alpha * sum_k opA[m,k] -- the bias gradient, computed inside the wgrad GEMM from the
 * M-side fragments it already holds (v_dot2c_f32_bf16 sums placed between the MFMAs) instead of a separate pass over dY. */
int ecamp_gemm(const void* A, const void* B, void* C, int64_t M, int64_t N, int64_t K, int a_kc, int64_t lda, int b_kc,
               int64_t ldb, int64_t ldc, const float* bias, const void* residual, int64_t ldr, void* pre_out, int64_t ldp,
               const void* gmul, int64_t ldg, int act, float alpha, const float* alpha_dev, int dtype, int out_f32, int accumulate,
               int split_k, float* splitk_ws, float* rowsum, ecampStream_t stream);
/* The f32 residual stream (ECAMP(f32_residual=True); the stream autocast leaves in f32: an f32 x plus a half branch promotes to f32 at timm
 * Block `x = x + attn(norm1(x))` / `x = x + mlp(norm2(x))`, model_ecamp.py:233-234,254-255): C f32 [M, ldc] = A B^T + bias[n] + residual
 * (f32 [M, ldr]); A [M, lda] and B [N, ldb] 16-bit (dtype 1), both contraction-contiguous -- the forward form of ecamp_gemm with its
 * residual epilogue, the sum formed from the f32 accumulator and never rounded to 16 bits.  Same kernels as ecamp_gemm (the persistent
 * ones where their legality holds, counted by ecamp_gemm_q8_launches / ecamp_gemm_q16_launches); residual and C 16-B aligned. */
int ecamp_gemm_res32(const void* A, const void* B, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                     const float* bias, const float* residual, int64_t ldr, int dtype, ecampStream_t stream);
/* Split count the library recommends for ecamp_gemm(M, N, K, ...) with an f32 accumulated output (the weight-gradient call of
 * torch.autograd for nn.Linear, e.g. timm Mlp.fc1 at model_ecamp.py:233): it depends on which kernel the shape selects
 * (128^2 tiles, or the persistent 256^2 kernel whose work items should fill whole rounds of the chip).  Pure host arithmetic. */
int ecamp_gemm_suggest_split(int64_t M, int64_t N, int64_t K, int a_kc, int b_kc, int dtype);
/* Grouped weight gradients (no reference counterpart: the reference's autograd issues one addmm per nn.Linear; timm Block at
 * model_ecamp.py:66-68,233-234, BertLayer at bert_layers.py): gw[p] [n_out[p], k_in[p]] (f32, contiguous) (+)= alpha * dy[p]^T x[p] and
 * gb[p] [n_out[p]] (f32, may be null) += alpha * column sums of dy[p], for the 1-4 linear layers of one block that share the row count
 * `rows` of dy[p] [rows, n_out[p]] / x[p] [rows, k_in[p]] (bf16, row-contiguous), as ONE persistent launch + one reduce.
 * accumulate[p] = 0 overwrites gw[p].  ws: ecamp_wgrad_group_workspace_bytes(...) bytes.  workgroups: 0 = three quarters of the CUs
 * (what is left runs whatever is queued beside it), otherwise at most one per CU.  ecamp_wgrad_group_supported == 0: issue per-layer ecamp_gemm calls.
 * table: DEVICE copy (32-byte aligned) of the group's item table -- pure host arithmetic on (shapes, has_bias, rows, workgroup count)
 * that ecamp_wgrad_group_table writes into HOST memory of ecamp_wgrad_group_table_bytes(...) bytes; the caller uploads it once per
 * shape set and keeps it (the library never allocates and never synchronises: the call is two kernel launches, capturable into a
 * HIP graph).  ecamp_wgrad_group_workgroups(w) = the workgroup count the launch uses for argument w (part of the table's identity).
 * table_bytes = what ecamp_wgrad_group_table returned for that image: a table built for another plan (the CU reserve or the workgroup
 * count changed in between) is refused instead of read at the wrong offsets. */
int ecamp_wgrad_group_supported(int32_t n, const int64_t* n_out, const int64_t* k_in, int64_t rows);
int64_t ecamp_wgrad_group_workspace_bytes(int32_t n, const int64_t* n_out, const int64_t* k_in, int64_t rows);
int64_t ecamp_wgrad_group_table_bytes(int32_t n, const int64_t* n_out, const int64_t* k_in, int64_t rows);
int64_t ecamp_wgrad_group_table(int32_t n, const int64_t* n_out, const int64_t* k_in, const int32_t* has_bias, int64_t rows,
                                int32_t workgroups, void* host_table);
int ecamp_wgrad_group_workgroups(int32_t workgroups);
int ecamp_wgrad_group(int32_t n, const void* const* dy, const void* const* x, float* const* gw, float* const* gb, const int64_t* n_out,
                      const int64_t* k_in, int64_t rows, float alpha, const float* alpha_dev, const int32_t* accumulate, float* ws,
                      const void* table, int64_t table_bytes, int32_t workgroups, ecampStream_t stream);
/* Workspace sizes (bytes) the caller allocates and passes in -- the library never allocates:
 *   ecamp_gemm_workspace_bytes      `splitk_ws` of ecamp_gemm for this split count (0 when split_k <= 1)
 *   ecamp_attn_bwd_workspace_bytes  `delta_ws` of ecamp_attn_bwd (one f32 per query row)
 *   ecamp_sr_bwd_workspace_bytes    `gw_ws` of ecamp_sr_bwd (168 f32, zeroed by the caller) */
int64_t ecamp_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int32_t split_k);
int64_t ecamp_attn_bwd_workspace_bytes(int32_t B, int32_t H, int32_t Tq);
int64_t ecamp_sr_bwd_workspace_bytes(void);
/* Process-wide switches with no reference counterpart (the "p8_" prefix is historical: the persistent one-workgroup-per-CU GEMM).
 * One table holds them all (csrc/core.hip g_opts; INTEGRATION.md "Library options" lists every row, the environment-only ones
 * included).  Where a switch has an environment variable it is read once, at first use, and a value set here wins over it.
 * Returns 0, or -1 (ecamp_last_error) for a null or unknown name.  The option names:
 * "p8_wgrad" (default 1): 0 keeps weight-gradient GEMMs off the persistent kernel.  "p8_wgrad_reserve_cus" (default 0): launch the
 * backward-pass forms of that kernel with this many fewer workgroups than CUs -- set by the data-parallel wrapper, whose all-reduce
 * kernels share the CUs during backward.  "q8_bwd_grid" (default 0 = one workgroup per CU; env ECAMP_Q8_BWD_GRID): n > 0 launches the
 * data-gradient form on min(output tiles, n) workgroups -- with n past the tile count every workgroup computes ONE tile and the
 * hardware dispatcher deals the tiles to whichever CUs the communication kernels leave free (+0.15 ms per step alone on a GPU);
 * set by the data-parallel wrapper as well; n <= 0 back to the environment. */
int ecamp_set_option(const char* name, int32_t value);
/* "q8_mode" (env ECAMP_GEMM_Q8): -1 automatic (default), 0 never, 2 whenever its alignment / size conditions hold -- the
 * persistent 256x256x64 kernel (csrc/gemm_q8.h) that serves the forward, data-gradient and weight-gradient forms.  Any other value
 * means -1; once this option has been set the environment variable is no longer consulted.
 * "q16_mode" (env ECAMP_Q16): the four-wave v_mfma_f32_16x16x32_bf16 kernel (csrc/gemm_q16.h; forward and data-gradient forms
 * with a plain / bias / residual epilogue, 256 x 256 or 256 x 192 tiles).  0 never; 1 (default) where the 192-column tile removes idle
 * last-round time -- the model's 768-wide outputs; 2 every eligible call; 3 as 2 whatever the size (tests); any other value back to
 * the environment.
 * "q16_wgrad" (env ECAMP_Q16_WGRAD): the weight-gradient form of that kernel (both operands strided; per-layer and grouped launches).
 * 0 never; 1 (default) every grouped launch and the per-layer launches the size rule selects whose output is at least 256 x 256 --
 * nothing while "q16_mode" is 0; 2 wherever legal, whatever the size (lab, tests); any other value back to the environment.
 * "attn_head" (env ECAMP_ATTN_HEAD): 1 (default) one workgroup per (batch, head) with everything resident in LDS for sequences
 * that fit (<= 256 tokens here), 0 the 64-row streaming kernels for every length, negative back to the environment's choice */

/* ---- fp8 forward (BASELINE.json configs[4]: "fp8 MFMA forward (bf16 grads) for QKV/MLP GEMMs"; no reference counterpart -- the
 * reference runs these nn.Linear layers under torch.cuda.amp, main_pretrain.py:138).  Per-tensor scaling, OCP e4m3:
 *   ecamp_amax      out[0] = max(out[0], max|x|)               (caller zeroes out[0]; n % 4 == 0)
 *   ecamp_quant_fp8 scale_out[0] = max(amax[0], tiny) / 448;  q[i] = e4m3(clamp(x[i] / scale, +-448))   (one byte per element)
 *   ecamp_gemm_fp8  C[M,N] (bf16) = act((A8[M,K] . B8[N,K]^T) * scale_a[0] * scale_b[0] + bias) (+ residual); act 0 none, 1 exact GELU, 2 exact GELU with gelu'(pre-activation) saved to pre_out (see ecamp_gemm),
 *                   with the bf16 pre-activation saved to pre_out -- the forward of timm Attention.qkv / proj and Mlp.fc1 / fc2
 *                   (call sites model_ecamp.py:233-234, 254-255).  K, lda, ldb multiples of 16 bytes.  f32 accumulation with unit block
 *                   scales: v_mfma_scale_f32_32x32x64_f8f6f4 in the persistent 256 x 256 x 128 kernel (csrc/gemm_q8.h, F8; every shape of
 *                   the model at B >= 64), v_mfma_scale_f32_16x16x128_f8f6f4 in the 128^2 kernel that serves small / unaligned shapes. */
int ecamp_amax(const void* x, float* out, int64_t n, int32_t dtype, ecampStream_t stream);
/* Delayed per-tensor scaling (round 4): a GEMM input site owns scale[0] (f32: what its producer quantises with and ecamp_gemm_fp8
 * dequantises with during this optimizer step) and 16 amax slots 32 floats apart (512 floats per site; what this step's producers saw).
 *   ecamp_quant_fp8_delayed  q[i] = e4m3(clamp(x[i] / scale[0], +-448)); amax_slots[(workgroup & 15) * 32] = max(., |x|)  -- one pass
 *   ecamp_fp8_roll           per site i < n: a = max over its slots; slots = 0; if a > 0: hist[i][hist_pos % hist_len] = a (hist nullable);
 *                            scale[i] = margin * max(a, hist[i][...]) / 448   (once per optimizer step).  hist = NULL, margin = 1: exact
 *                            current scaling (the weights).  Activation sites: the largest maximum of the last hist_len fed steps times a
 *                            margin, so that an activation that grows from one step to the next does not saturate at +-448
 *   ecamp_layernorm_fwd_q8   ecamp_layernorm_fwd that also writes the e4m3 copy of y (same conventions): the quantisation folded into
 *                            the producer of the GEMM input (nn.LayerNorm sites model_ecamp.py:69,84,235,256; BertSelfOutput / BertOutput) */
int ecamp_quant_fp8_delayed(const void* x, const float* scale, void* q, float* amax_slots, int64_t n, int32_t dtype, ecampStream_t stream);
int ecamp_fp8_roll(float* amax_slots, float* scale, int32_t n, float* hist, int32_t hist_len, int32_t hist_pos, float margin, ecampStream_t stream);
/* The e4m3 copies of all weights of a flat bf16 arena in two launches per optimizer step (exact per-matrix scaling): items = DEVICE table
 * of int32[4] {first element (multiple of 4), count (multiple of 4, <= 65536), scale id, 0}, one workgroup each.  pass 0: the item's
 * max|w| into the amax slots of its scale id; (ecamp_fp8_roll); pass 1: w8[i] = e4m3(clamp(w[i] / scales[id], +-448)). */
int ecamp_fp8_weights(const void* w_bf16, void* w8, const int32_t* items, int32_t nitems, float* amax_slots, const float* scales,
                      int32_t pass, ecampStream_t stream);
int ecamp_layernorm_fwd_q8(const void* x, const void* residual, void* z_out, const float* gamma, const float* beta, void* y, float* mean,
                           float* rstd, int64_t rows, int32_t cols, float eps, float drop_p, uint64_t seed, uint64_t offset, void* q8,
                           const float* q8_scale, float* q8_amax_slots, int32_t dtype, ecampStream_t stream);
int ecamp_quant_fp8(const void* x, const float* amax, void* q, float* scale_out, int64_t n, int32_t dtype, ecampStream_t stream);
int ecamp_gemm_fp8(const void* A8, const void* B8, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                   const float* scale_a, const float* scale_b, const float* bias, const void* residual, int64_t ldr, void* pre_out,
                   int64_t ldp, int act, void* q8_out, const float* q8_scale, float* q8_amax_slots, ecampStream_t stream);
/* q8_out (nullable; needs act = 1 or 2, pre_out, no residual, ldc = N): also leave the e4m3 copy of C for the NEXT dense layer (timm Mlp.fc2 /
 * BertOutput.dense behind the GELU), quantised with that layer's input scale q8_scale[0], and max|C| in its amax slots -- the fp8
 * forward's quantisation folded into the epilogue that produces the activation (ecamp_quant_fp8_delayed's conventions). */

/* ---- LayerNorm (nn.LayerNorm eps 1e-6: model_ecamp.py:69,84,235,256 + timm Block norms; HF LN eps 1e-12:
 * BertSelfOutput/BertOutput/BertEmbeddings/transform).  y = LN(z), z = dropout(x) + residual (both optional). */
int ecamp_layernorm_fwd(const void* x, const void* residual, void* z_out, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, int64_t rows, int32_t cols, float eps, float drop_p, uint64_t seed,
                        uint64_t offset, int32_t dtype, ecampStream_t stream);
int ecamp_layernorm_bwd(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                        const void* dres_in, void* dz, void* dx_drop, float* dgamma, float* dbeta, int64_t rows, int32_t cols,
                        float drop_p, uint64_t seed, uint64_t offset, int32_t dtype, ecampStream_t stream);
/* The LayerNorms of the f32 residual stream (timm Block norm1 / norm2, `norm`, `decoder_norm`: model_ecamp.py:69,84,233-235,254-256 --
 * under autocast nn.LayerNorm runs in f32 on the f32 stream): x / z f32 [rows, cols]; y, dy, dres_in (nullable) and dz 16-bit (dtype 1).
 * No residual or dropout fusion; otherwise ecamp_layernorm_fwd / ecamp_layernorm_bwd. */
int ecamp_layernorm_fwd_x32(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows,
                            int32_t cols, float eps, int32_t dtype, ecampStream_t stream);
int ecamp_layernorm_bwd_z32(const void* dy, const float* z, const float* mean, const float* rstd, const float* gamma, const void* dres_in,
                            void* dz, float* dgamma, float* dbeta, int64_t rows, int32_t cols, int32_t dtype, ecampStream_t stream);
/* Which layout a LayerNorm call gets (no reference counterpart; host arithmetic, nothing is launched): out = int32[6] {elements per lane
 * access, accesses per lane and row, waves per workgroup, gamma in registers (1) or in LDS (0), dynamic LDS bytes, most workgroups
 * launched (0: no cap)} for (backward?, 16-bit rows? -- the f32-stream entries count as 16-bit --, cols, every row pointer on a 16-byte
 * boundary?, the value of ECAMP_LN_BWD).  Added at version 5 without touching an existing signature. */
int ecamp_layernorm_layout(int32_t backward, int32_t rows16, int32_t cols, int32_t al16, int32_t opt_bwd, int32_t* out);

/* ---- attention (timm Attention.forward: softmax(q k^T * hd^-1/2) v; HF BertSelfAttention 4.42.4 incl. the
 * cross-attention mode of context_fusion.py:45-53).  strides = {batch, token, head} in elements, head_dim contiguous.
 * key_mask: int32 [B,Tk], nonzero = attend (the additive finfo.min mask of bert_modeling.py:92), or NULL.
 * drop_mask (optional, ecamp_attn_mask_bytes(...) bytes): the dropout keep-mask of the probabilities as bits, written by the forward
 * call and read by the backward call that is given the same buffer -- the Philox stream is then evaluated once per score instead of
 * three times (forward, dQ pass, dK/dV pass).  NULL (or a size of 0: shapes the bit form does not serve): the backward pass
 * regenerates the mask from (seed, offset); both forms give bit-identical results. */
int64_t ecamp_attn_mask_bytes(int32_t B, int32_t H, int32_t Tq, int32_t Tk, int32_t hd, int32_t dtype);
int ecamp_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int32_t* key_mask, int32_t B,
                   int32_t H, int32_t Tq, int32_t Tk, int32_t hd, const int64_t* q_strides, const int64_t* k_strides,
                   const int64_t* v_strides, const int64_t* o_strides, float scale, float drop_p, uint64_t seed, uint64_t offset,
                   int32_t dtype, void* drop_mask, ecampStream_t stream);
int ecamp_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   float* delta_ws, void* dq, void* dk, void* dv, const int32_t* key_mask, int32_t B, int32_t H, int32_t Tq,
                   int32_t Tk, int32_t hd, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                   const int64_t* o_strides, const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides,
                   const int64_t* dv_strides, float scale, float drop_p, uint64_t seed, uint64_t offset, int32_t dtype,
                   const void* drop_mask, ecampStream_t stream);
/* Attention probabilities softmax(scale * q k^T + mask), f32 [B,H,Tq,Tk] (Tk <= 1024): the tensor the reference's Visualization
 * model returns from the fusion layer's cross-attention (Visualization/module/context_fusion.py:45-57,
 * Visualization/module/model_ecamp.py:308-319).  Evaluation only. */
int ecamp_attn_probs(const void* q, const void* k, const int32_t* key_mask, float* probs, int32_t B, int32_t H, int32_t Tq, int32_t Tk,
                     int32_t hd, const int64_t* q_strides, const int64_t* k_strides, float scale, int32_t dtype, ecampStream_t stream);

/* ---- elementwise / reductions ---- */
int ecamp_add(const void* a, const void* b, void* y, int64_t n, int32_t dtype, ecampStream_t stream);
int ecamp_gelu_bwd(const void* dy, const void* pre, void* dx, int64_t n, int32_t dtype, ecampStream_t stream);
int ecamp_cast(const void* src, void* dst, int64_t n, int32_t src_dtype, int32_t dst_dtype, ecampStream_t stream);
/* y = x * alpha * (alpha_dev ? *alpha_dev : 1) in f32 arithmetic; x == y allowed (autograd's scaling of a gradient tensor by an upstream
 * scalar, bert_modeling.py:213-217 -> loss.backward()) */
int ecamp_scale(const void* x, void* y, int64_t n, float alpha, const float* alpha_dev, int32_t dtype, ecampStream_t stream);
int ecamp_zero(void* p, int64_t bytes, ecampStream_t stream);
/* out[n] += alpha * sum over rows m (optionally only rows with lo <= m % period < hi) of X[m*ld+n]: bias grads,
 * cls-token grad (model_ecamp.py:228-230). */
int ecamp_colsum(const void* X, int64_t ld, int64_t M, int64_t N, float alpha, const float* alpha_dev, int32_t period, int32_t lo, int32_t hi,
                 float* out, int32_t dtype, ecampStream_t stream);
int ecamp_bcast_add(const void* x, const void* g, void* y, int64_t B, int32_t S, int32_t H, int32_t dtype,
                    ecampStream_t stream); /* context_fusion.py:55 */
int ecamp_seq_sum(const void* x, void* out, int64_t B, int32_t S, int32_t H, int32_t s0, int32_t s1, float scale, int32_t dtype,
                  ecampStream_t stream); /* model_ecamp.py:269 gap token; grad of the broadcast */
int ecamp_seq_bcast(const void* g, void* y, int64_t B, int32_t S, int32_t H, int32_t s0, int32_t s1, float scale, int32_t mode,
                    int32_t dtype, ecampStream_t stream);
int ecamp_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, ecampStream_t stream); /* model_ecamp.py:177 */

/* ---- image side ---- */
int ecamp_bicubic_resize(const float* src, float* dst, int64_t planes, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                         ecampStream_t stream); /* model_ecamp.py:318 */
/* The same resize from the dataset's grayscale crop as uint8 [B,Hs,Ws] (pretrain_datasets.py:47-52: Grayscale(3) + ToTensor +
 * Normalize with ONE mean / std, i.e. three identical channels): dst f32 [B,3,Hd,Wd] = resize(lut[src]), the three planes written
 * from one evaluation.  lut: 256 f32 on the device, lut[u] = ((float)u / 255 - mean) / std in f32 arithmetic (ToTensor + Normalize
 * per byte value), which makes the result bit for bit what ecamp_bicubic_resize gives on the f32 [B,3,Hs,Ws] image for the exact 2x
 * ratio of the hot path and for Hs == Hd (the normalised image itself).  One byte per pixel crosses PCIe and is read instead of twelve. */
int ecamp_bicubic_resize_u8(const uint8_t* src, float* dst, int64_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd, const float* lut,
                            ecampStream_t stream);
int ecamp_mask_indices(const float* noise, int64_t B, int32_t L, int32_t len_keep, int32_t* ids_restore, int32_t* ids_keep,
                       float* mask, ecampStream_t stream); /* model_ecamp.py:168-193 */
int ecamp_im2col_gather(const float* imgs, const int32_t* ids_keep, void* out, int64_t B, int32_t Lk, int32_t C, int32_t R,
                        int32_t p, int32_t dtype, ecampStream_t stream); /* model_ecamp.py:220 + :185 */
int ecamp_assemble_tokens(void* x, const float* cls, const float* pos, const int32_t* ids_keep, int64_t B, int32_t Lk, int32_t D,
                          int32_t dtype, ecampStream_t stream); /* model_ecamp.py:222,228-230 */
/* ecamp_assemble_tokens into a separate f32 out [B, Lk+1, D] from the 16-bit (dtype 1) patch embedding x: the f32 residual stream's first
 * value, autocast's half conv output + f32 pos_embed (model_ecamp.py:222,228-230) */
int ecamp_assemble_tokens_x32(const void* x, float* out, const float* cls, const float* pos, const int32_t* ids_keep, int64_t B, int32_t Lk,
                              int32_t D, int32_t dtype, ecampStream_t stream);
/* The dataset's image transform on the device (pretrain_datasets.py:47-52,113-115: RandomResizedCrop(448, bicubic) + RandomHorizontalFlip +
 * Grayscale): B crops of a pre-decoded uint8 grayscale radiograph -> dst uint8 [B, out, out], equal BYTE FOR BYTE to
 * PIL's img.crop(box).resize((out, out), BICUBIC) (+ FLIP_LEFT_RIGHT, convert('L')) on the same pixels -- Pillow's two-pass antialiased
 * resample (Resample.c: double-precision coefficients -> 22-bit fixed point, uint8 intermediate) restated in csrc/augment.hip.
 * src: the crops' bytes back to back (each h x w, contiguous); table int64 [B, 6] on the device = {byte offset in src, h, w, flip (0/1),
 * first row of the sample in the intermediate (prefix sum of h), 0}; kmax >= the tap count of the batch's largest scale factor
 * (2 * ceil(2 * max(1, size / out)) + 1); tmp_rows = sum of h; max_h = largest h; ws from ecamp_resample_crops_workspace_bytes;
 * err_flag: int32 on the device, set to 1 if a sample needs more than kmax taps (the result is then undefined).  B <= 65535, out <= 512.
 * The four resample entry points share one launch path and one workspace layout; the boxes forms add a table copy at its end. */
int64_t ecamp_resample_crops_workspace_bytes(int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows);
int ecamp_resample_crops_u8(const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows,
                            int32_t max_h, void* ws, int64_t ws_bytes, int32_t* err_flag, ecampStream_t stream);
/* The classification transforms on the device (Fine-tuning/Classification/utils/data_utils.py:20-34: RandomResizedCrop((s, s)) + flip,
 * and Resize(int) + CenterCrop((s, s)), Pillow BILINEAR): the same two-pass resample with a filter argument (0: BILINEAR, 1: BICUBIC) and,
 * per axis, `full` -- the size the axis is resized to -- and `shift` -- where the `out` output pixels start in the resized axis; an output
 * pixel outside [0, full) is 0 (CenterCrop's zero padding).  table int64 [B, 10] on the device = {byte offset in src, h, w, flip (0/1), first
 * intermediate row, full_w, shift_w, full_h, shift_h, 0}; a training crop is full = out, shift = 0.  kmax >= 2 * ceil(support *
 * max(1, size / full)) + 1 of every sample and axis (support 1 bilinear, 2 bicubic); the other arguments as ecamp_resample_crops_u8, ws
 * from ecamp_resample_boxes_workspace_bytes.  Filter 1 with full = out, shift = 0 gives the bytes of ecamp_resample_crops_u8. */
int64_t ecamp_resample_boxes_workspace_bytes(int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows);
int ecamp_resample_boxes_u8(const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows,
                            int32_t max_h, int32_t filter, void* ws, int64_t ws_bytes, int32_t* err_flag, ecampStream_t stream);
/* ecamp_resample_boxes_u8 for batches that may hold COLOUR sources (the same call sites, data_utils.py:20-34, on the colour-fundus tasks:
 * Pillow resamples an RGB image band by band with an L image's coefficients and uint8 intermediate, and Grayscale -- convert("L"),
 * L = (19595 R + 38470 G + 7471 B + 2^15) >> 16 -- follows the resize).  Same arguments; the last table column is the sample's plane
 * count c: 3 = three planes R, G, B of h x w bytes back to back at the byte offset, which own 3 h rows of the intermediate from the
 * sample's first row (plane p at + p h) and are folded to luma behind the vertical pass; any other value = one plane, the row's meaning
 * in ecamp_resample_boxes_u8, and that function's byte.  tmp_rows = sum of c * h, max_h = largest c * h; ws from
 * ecamp_resample_boxes_workspace_bytes; both filters; the same argument checks and err_flag. */
int ecamp_resample_boxes_rgb_u8(const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows,
                                int32_t max_h, int32_t filter, void* ws, int64_t ws_bytes, int32_t* err_flag, ecampStream_t stream);
/* ecamp_resample_boxes_rgb_u8 on a shard that STAYS in device memory: `shard` is the whole uploaded file of `shard_bytes` bytes and every
 * box is read where it lies in its stored image -- no box is copied.  table int64 [B, 12] on the device = the stride-10 row of
 * ecamp_resample_boxes_rgb_u8 (column 9: the plane count c) + {pitch, plane_pitch}: pitch = bytes between two rows of the stored image (its
 * width W), plane_pitch = bytes between two of its planes (H * W); `off` = byte offset in `shard` of the box's first pixel in plane 0 (image
 * offset + y0 * W + x0), row r of plane p of the box starts at off + p * plane_pitch + r * pitch.  Everything else as
 * ecamp_resample_boxes_rgb_u8 (both filters, full / shift, flip, the luma fold, tmp_rows / max_h counting c * h, kmax, B <= 65535,
 * out <= 512, ws from ecamp_resample_boxes_workspace_bytes); with pitch = w, plane_pitch = h * w and a packed source: that function's bytes.
 * Every row is checked on the device before a byte is read: h > 0, w > 0, pitch >= w, off >= 0, plane_pitch >= 0 and
 * off + (c - 1) * plane_pitch + (h - 1) * pitch + w <= shard_bytes.  A row that fails reads nothing, its sample is all zeros, and 2 is ORed
 * into err_flag (1 keeps its meaning: more than kmax taps).  Added at version 5 without touching an existing signature. */
int ecamp_resample_shard_u8(const uint8_t* shard, int64_t shard_bytes, const int64_t* table, uint8_t* dst, int64_t B, int32_t out,
                            int32_t kmax, int64_t tmp_rows, int32_t max_h, int32_t filter, void* ws, int64_t ws_bytes,
                            int32_t* err_flag, ecampStream_t stream);
/* ecamp_im2col_gather straight from a uint8 grayscale image [B, R, R] at the model's own size: out [B * (Lk + 1), 3 * p * p] (f32 or the
 * build's 16-bit format), the cls row zero, the three channel slabs the same values lut[byte] -- bit for bit ecamp_im2col_gather on
 * lut[img] expanded to three planes (lut as in ecamp_bicubic_resize_u8, built from the caller's mean / std). */
int ecamp_im2col_u8(const uint8_t* img, const float* lut, const int32_t* ids_keep, void* out, int64_t B, int32_t Lk, int32_t R, int32_t p,
                    int32_t dtype, ecampStream_t stream);
int ecamp_unshuffle_fwd(const void* y, const int32_t* ids_restore, const float* mask_token, const float* dpos, void* xd, int64_t B,
                        int32_t L, int32_t Lk, int32_t D, int32_t dtype, ecampStream_t stream); /* model_ecamp.py:245-251 */
/* ecamp_unshuffle_fwd with an f32 xd from the 16-bit (dtype 1) y: the decoder's f32 residual stream (autocast promotes the cat of the half
 * decoder_embed output with the f32 mask tokens, + the f32 decoder_pos_embed: model_ecamp.py:245-251) */
int ecamp_unshuffle_fwd_x32(const void* y, const int32_t* ids_restore, const float* mask_token, const float* dpos, float* xd, int64_t B,
                            int32_t L, int32_t Lk, int32_t D, int32_t dtype, ecampStream_t stream);
int ecamp_unshuffle_bwd(const void* dxd, const int32_t* ids_restore, const int32_t* ids_keep, void* dy, float* dmask_token,
                        int64_t B, int32_t L, int32_t Lk, int32_t D, int32_t dtype, ecampStream_t stream);
int ecamp_unpatchify_mim(const void* pred, const float* imgs, const float* mask, float* pred_img, float* loss_sum, int64_t B,
                         int32_t R, int32_t p, int32_t dtype, ecampStream_t stream); /* model_ecamp.py:153-165,288-298 */
int ecamp_img_loss_bwd(const float* pred_img, const float* imgs, const float* mask, const float* dsr, const float* gm_gs,
                       void* dpred, int64_t B, int32_t R, int32_t p, int32_t dtype, ecampStream_t stream);
int ecamp_sr_fwd(const float* pred_img, const void* big, const float* big_lut, const int64_t* column,
                 const int64_t* row, const float* w1, const float* b1, const float* w2, const float* b2, float* loss_sum, int64_t B,
                 int32_t R, int32_t super_patch, int32_t window, int32_t mode,
                 ecampStream_t stream); /* model_ecamp.py:28-46,196-215,291-299; fused, LDS-resident.
                 mode 0: f32 VALU stencils (parity); mode 1: bf16 matrix cores (4x4x4 MFMA per tap), f32 accumulate / skip / loss.
                 big: the loss target, f32 [B,3,2R,2R] (big_lut = NULL) or the uint8 crop [B,2R,2R] normalised on the fly through
                 big_lut[256] (see ecamp_bicubic_resize_u8; same bits as the f32 image) */
/* The SR head's output image itself, f32 [B,3,2R,2R] = super_res(pred_img) (model_ecamp.py:28-46,285): never materialised by the
 * training step (ecamp_sr_fwd folds it into the loss); for parity checks against the reference's activation and visualisation. */
int ecamp_sr_image(const float* pred_img, const float* w1, const float* b1, const float* w2, const float* b2, float* sr, int64_t B,
                   int32_t R, ecampStream_t stream);
int ecamp_sr_bwd(const float* pred_img, const void* big, const float* big_lut, const int64_t* column,
                 const int64_t* row, const float* w1, const float* b1, const float* w2, const float* b2, float* dsr, float* gw_ws,
                 int64_t B, int32_t R, int32_t super_patch, int32_t window, int32_t mode, ecampStream_t stream);
int ecamp_scaled_accum(const float* ws, float* grad, const float* scale_dev, int32_t idx, int32_t n, ecampStream_t stream);

/* ---- report side ---- */
int ecamp_bert_embed_fwd(const int64_t* ids, const int64_t* type_ids, const float* word, const float* pos, const float* type,
                         const float* gamma, const float* beta, void* z, void* e, float* mean, float* rstd, int64_t B, int32_t S,
                         int32_t cols, float eps, float drop_p, uint64_t seed, uint64_t offset, int32_t dtype,
                         ecampStream_t stream); /* HF BertEmbeddings, bert_modeling.py:113 */
int ecamp_bert_embed_bwd(const void* de, const void* z, const float* mean, const float* rstd, const float* gamma, const int64_t* ids,
                         const int64_t* type_ids, float* gword, float* gpos, float* gtype, float* dgamma, float* dbeta, int64_t B,
                         int32_t S, int32_t cols, int32_t pad_id, int32_t hot0, int32_t hot1, float drop_p, uint64_t seed,
                         uint64_t offset, int32_t dtype, ecampStream_t stream);
/* Weighted cross-entropy of the MLM head with its gradient written over the logits (bert_modeling.py:213-217).  `logits` [M, V], row
 * stride ld, f32 or the build's 16-bit format; ld >= V > 0, V and ld multiples of 4, 0 <= M <= 2^31 - 1 (anything else, a null pointer
 * or another dtype code is refused before any launch; M == 0 returns 0 without one).  Per row, with w = weights[i] and a label in
 * [0, V):  loss_sum += w * (logsumexp(row) - logit[label])  and  logits[i, j] = inv_count * w * (softmax_ij - [j == label]);  a row
 * whose label lies outside [0, V) (ignore_index -100) adds nothing and gets a row of zeros.  Columns [V, ld) are never written.
 * inv_count = gain / M: the caller divides loss_sum by M and the gain out of the upstream gradient.  Logits must be finite. */
int ecamp_ce_fwd_bwd(void* logits, const int64_t* labels, const float* weights, float* loss_sum, int64_t M, int32_t V, int64_t ld,
                     float inv_count, int32_t dtype, ecampStream_t stream);
/* Held-out evaluation of the same head (no reference counterpart: the reference has no validation loop).  Read-only on `logits`
 * [M, V] (row stride ld; V and ld multiples of 4).  A row whose label lies outside [0, V) (ignore_index -100) is skipped without a
 * read of its logits; for every other row, with xl = logit[label] and rank = #{ j : logit[j] > xl } (strictly greater: a label tied
 * with the maximum ranks first):  loss_sum += w * (logsumexp(row) - xl) -- the quantity ecamp_ce_fwd_bwd accumulates; the caller
 * divides by M --, counts[0] += 1, counts[1] += rank == 0, counts[2] += rank < 5.  counts is int64[3] (integer atomics: exact);
 * the caller zeroes loss_sum and counts. */
int ecamp_ce_eval(const void* logits, const int64_t* labels, const float* weights, float* loss_sum, int64_t* counts, int64_t M,
                  int32_t V, int64_t ld, int32_t dtype, ecampStream_t stream);
/* Row compaction in front of that head (no reference counterpart): a held-out pass scores a fraction of the B*S positions, and the
 * head needs those rows only.  Row m of x [M, cols] (row stride ldx; f32 or the build's 16-bit format) is SCORED iff
 * 0 <= labels[m] < V and (ids == NULL or ids[m] == mask_id).  The scored rows are written in increasing order of m -- the row to
 * x_out [cap, cols] (contiguous), its label, its weight and rows_out[i] = m; output rows [count, cap) are padding: zeros, label -100,
 * weight 0, rows_out -1 (the head and ecamp_ce_eval run over them unchanged).  count_out[0] receives the true number of scored rows
 * even where it exceeds cap; nothing is written at or beyond row cap.  Deterministic: counts per segment, sums of counts, a gather
 * in which every workgroup derives its own offset -- no atomics, no workgroup waits for another.  A row and the row stride must be
 * multiples of 16 bytes, x / x_out / ws 16-byte aligned; M and cap at most 2^31 - 1.  ws: ecamp_compact_rows_workspace_bytes(M)
 * bytes of device memory, scratch (added at version 5 like ecamp_ce_eval: no existing signature changes). */
int64_t ecamp_compact_rows_workspace_bytes(int64_t M);
int ecamp_compact_rows(const void* x, int64_t ldx, const int64_t* labels, const float* weights, const int64_t* ids, int64_t mask_id,
                       int64_t M, int32_t cols, int32_t V, int64_t cap, void* x_out, int64_t* labels_out, float* weights_out,
                       int32_t* rows_out, int64_t* count_out, void* ws, int32_t dtype, ecampStream_t stream);

/* ---- linear-probe classification behind the frozen encoder (ECAMP/Fine-tuning/Classification; csrc/classify.hip).  Added at version 5
 * like ecamp_ce_eval: no existing signature changes.  All arithmetic f32; every sum has one fixed order (no float atomics, no workgroup
 * waits for another), so two calls on the same input give the same bits; no grid grows with B beyond a cap (the kernels loop).  A null
 * pointer, C outside [1, 64], D % 4 != 0 or t0 >= t1 is refused before the device is touched. ---- */
/* x [B, T, D] (the build's 16-bit format, dtype 1, or f32, dtype 0: the f32 residual stream) -> pooled f32 [B, D] = mean over tokens
 * t0 <= t < t1 (t0 = 1: `x[:, 1:, :].mean(dim=1)`, models_vit.py:92) and feat f32 [B, D] = LayerNorm(pooled) with f32 gamma / beta and
 * eps (`self.fc_norm(x)`, models_vit.py:93); gamma == beta == NULL: identity affine.  One pass over x with f32 means, where
 * ecamp_seq_sum + ecamp_layernorm_fwd round the mean to 16 bits in between.  x, pooled, feat and ws 16-byte aligned;
 * ws: ecamp_pool_norm_workspace_bytes(...) bytes of device memory, scratch (f32 partial sums of the token chunks). */
int64_t ecamp_pool_norm_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t t0, int32_t t1, int32_t dtype);
int ecamp_pool_norm(const void* x, const float* gamma, const float* beta, float* pooled, float* feat, int64_t B, int32_t T, int32_t D,
                    int32_t t0, int32_t t1, float eps, void* ws, int32_t dtype, ecampStream_t stream);
/* logits f32 [B, C] = feat [B, D] . W [C, D]^T + bias [C], all f32, 1 <= C <= 64 (`self.head(x)` of timm's VisionTransformer.forward,
 * call site train.py:441; the datasets have 1..20 classes, shapes the MFMA GEMMs refuse). */
int ecamp_cls_head_fwd(const float* feat, const float* W, const float* bias, float* logits, int64_t B, int32_t C, int32_t D,
                       ecampStream_t stream);
/* kind 0: targets f32 [B, C], BCEWithLogitsLoss, mean over B*C (train.py:200,423) as max(x,0) - x y + log1p(exp(-|x|));
 * kind 1: targets int64 [B], CrossEntropyLoss, mean over B (train.py:202,425) with the row maximum subtracted.
 * loss f32 [1]; dlogits f32 [B, C] = gradient of that mean; counts int64 [2] = {rows seen, rows predicted right}: kind 1, the first
 * maximum is the label (torch.argmax, train.py:222); kind 0, every class on its target's side of 0 (train.py:220).  bad_label int32 [1]
 * on the device: 1 if a kind-1 label lies outside [0, C) (that row reads no logit and gets a zero loss and gradient), else 0 -- the
 * caller reads it where it synchronises anyway.  Meant for a head's batch -- B up to a few thousand rows, B * C a few 10^4 values: the
 * kernel is ONE 1024-thread workgroup (the ordered sum needs no workspace that way) in which a thread walks whole rows, so its time
 * grows linearly with B / 1024 on a single CU; larger B is accepted (below 2^31) and correct, but not what it is built for. */
int ecamp_cls_loss(const float* logits, const void* targets, int32_t kind, float* loss, float* dlogits, int64_t* counts,
                   int32_t* bad_label, int64_t B, int32_t C, ecampStream_t stream);
/* dW [C, D] = dlogits^T . feat and db [C] = column sums of dlogits, f32, overwriting (the head's share of `loss.backward()`,
 * train.py:454); the summation order over B is fixed. */
int ecamp_cls_head_wgrad(const float* dlogits, const float* feat, float* dW, float* db, int64_t B, int32_t C, int32_t D,
                         ecampStream_t stream);

/* ---- optimizer side ---- */
/* optimizer.zero_grad() (main_pretrain.py:169) without touching the weight matrices: zero the 64-element blocks of the gradient arena
 * whose flag byte is non-zero (n = arena length, a multiple of 64).  The weight-gradient GEMMs of the next backward pass overwrite
 * their outputs (ecamp_gemm accumulate = 0) instead of adding to a zeroed buffer. */
int ecamp_zero_blocks(float* g, const uint8_t* block_flags, int64_t n, ecampStream_t stream);
int ecamp_sumsq(const float* x, int64_t n, float* out, ecampStream_t stream); /* util/misc.py:280-292 */
int ecamp_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2,
                float eps, float weight_decay, int64_t step, float grad_scale,
                ecampStream_t stream); /* torch.optim.AdamW, main_pretrain.py:254 */

int ecamp_adamw_grouped(float* p, const float* g, float* m, float* v, void* p_bf16, const uint8_t* block_group, int64_t n,
                        int32_t ngroups, const float* lr_host, const float* wd_host, float beta1, float beta2, float eps,
                        int64_t step, float grad_scale, float* grad_sumsq, const float* ctl,
                        ecampStream_t stream); /* whole-arena AdamW with timm's decay/no-decay groups, main_pretrain.py:253-254;
                                                * grad_sumsq (nullable, caller-zeroed): += sum of (g * grad_scale)^2 over the updated
                                                * elements -- the global gradient norm of util/misc.py:280-292 without a second pass;
                                                * ctl (nullable, device f32[4] written by ecamp_loss_scale_update): {grad_scale, skip, bias
                                                * corrections} read on the DEVICE instead of `step` / `grad_scale` -- a skipped step writes nothing */
/* GradScaler's unscale_ + step + update (util/misc.py:262-269: `self._scaler.unscale_`, `.step(optimizer)`, `.update()`) decided on the
 * device, so the training loop never waits for the overflow flag: sumsq = sum(g^2) over the scaled gradients (ecamp_sumsq);
 * state f32[4] = {scale, growth tracker, skipped steps, unused}; opt_step f32[1] = optimizer steps actually taken (bias corrections);
 * ctl f32[4] = output for ecamp_adamw_grouped; norm_out (nullable) = sqrt(sumsq) / scale. */
int ecamp_loss_scale_update(const float* sumsq, float* state, float* opt_step, float* ctl, float* norm_out, float growth_factor,
                            float backoff_factor, int32_t growth_interval, float beta1, float beta2, ecampStream_t stream);

/* ---- fine-tuning the encoder behind the classifier (`--mode Finetune` of ECAMP/Fine-tuning/Classification; csrc/finetune.hip).  Added at
 * version 5: no existing signature changes.  Conventions as the linear-probe kernels above: f32 arithmetic, every sum in one fixed order
 * (no float atomics, no workgroup waits for another: two calls on the same input give the same bits), grids capped with a loop beyond
 * the cap; a null pointer, C outside [1, 64], D % 4 != 0, t0 >= t1 or n % 64 != 0 is refused before the device is touched. ---- */
/* dfeat f32 [B, D] = dlogits [B, C] . W [C, D]: the head's data gradient (the share of `loss.backward()` that leaves the head towards
 * the encoder), 1 <= C <= 64, D % 4 == 0; W and dfeat 16-byte aligned. */
int ecamp_cls_head_dgrad(const float* dlogits, const float* W, float* dfeat, int64_t B, int32_t C, int32_t D, ecampStream_t stream);
/* Backward of ecamp_pool_norm.  dfeat f32 [B, D]; pooled f32 [B, D] as ecamp_pool_norm returned it (mean and rstd are computed again
 * from it); gamma f32 [D] or NULL (identity affine).  dgamma / dbeta f32 [D] (given together, or both NULL): WRITTEN, not accumulated,
 * from per-workgroup partial sums in the workspace added in workgroup order.  dx [B, T, D] in `dtype` (0: f32, 1: the build's 16-bit
 * format): dx[b, t, :] = dpooled[b] / (t1 - t0) for t0 <= t < t1 and 0 for every other token (the cls row).  dx, ws, dgamma and dbeta 16-byte aligned;
 * ws: ecamp_pool_norm_bwd_workspace_bytes(...) bytes of device memory, scratch. */
int64_t ecamp_pool_norm_bwd_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t t0, int32_t t1, int32_t dtype);
int ecamp_pool_norm_bwd(const float* dfeat, const float* pooled, const float* gamma, float* dgamma, float* dbeta, void* dx, int64_t B,
                        int32_t T, int32_t D, int32_t t0, int32_t t1, float eps, void* ws, int32_t dtype, ecampStream_t stream);
/* sum(g^2) over the 64-element blocks of g [n] whose block_group byte is below 8 (ecamp_adamw_grouped's table; 255 = skipped), as ONE f32
 * partial PER WORKGROUP in partials[0 .. slots): no scalar is produced, ecamp_sgd_grouped adds the partials itself.
 * slots = ecamp_sumsq_grouped_slots(n) <= 2048 (a function of n alone; 0 for an n the launch refuses); *npart_out (a HOST int, nullable)
 * receives the same number.  Two launches may fill disjoint ranges of one partials buffer (an arena and a tail buffer).  n % 64 == 0. */
int64_t ecamp_sumsq_grouped_slots(int64_t n);
int ecamp_sumsq_grouped(const float* g, const uint8_t* block_group, int64_t n, float* partials, int32_t* npart_out, ecampStream_t stream);
/* torch.optim.SGD (momentum, dampening 0, no Nesterov, weight decay added to the gradient; train.py:377-384) behind
 * torch.nn.utils.clip_grad_norm_(max_norm) (train.py:458), over a flat buffer with ecamp_adamw_grouped's block table and per-group
 * lr / weight decay.  Every workgroup adds partials[0 .. npart) (device, ecamp_sumsq_grouped; npart <= 4096) in one fixed order, then
 *   norm = sqrt(sum) * grad_scale;   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1
 *   d = g * grad_scale * coef + wd * p;   buf = momentum * buf + d;   p -= lr * buf
 * per element of a live block (a zero `buf` reproduces torch's first step); p16 (nullable): the 16-bit shadow, refreshed.  Blocks of
 * group 255 are neither read nor written.  norm_out (nullable, device f32[1]) receives `norm`.  ctl (nullable, device f32[4] as
 * ecamp_loss_scale_update writes it): ctl[0] replaces grad_scale, ctl[1] != 0 leaves every byte alone.  n % 64 == 0. */
int ecamp_sgd_grouped(float* p, const float* g, float* buf, void* p16, const uint8_t* block_group, int64_t n, int32_t ngroups,
                      const float* lr_host, const float* wd_host, float momentum, float max_norm, const float* partials, int32_t npart,
                      float grad_scale, const float* ctl, float* norm_out, ecampStream_t stream);
/* Dynamic loss scaling around ecamp_sgd_grouped, decided on the device (IEEE-half fine-tuning: what apex's `--fp16 --fp16_opt_level O2`
 * puts around the reference's step, train.py:398,452-465).  ONE workgroup adds partials[0 .. npart) -- the slots ecamp_sumsq_grouped
 * filled over the SCALED gradients, 1 <= npart <= 4096 -- in exactly ecamp_sgd_grouped's order, so both hold the same bits of the sum s.
 *   found = !(|s| <= FLT_MAX)            (inf, nan, or finite slots whose sum leaves f32)
 *   ctl[0..4) = {1 / scale, found, 0, 0}  (what ecamp_sgd_grouped reads: a found step leaves every byte alone)
 *   norm_out[0] = sqrt(s) / scale        (nullable; the norm of the un-scaled gradients, computed as sqrt(s) * ctl[0] like the step's own
 *                                         norm_out and bit-equal to it; inf / nan when found)
 * state f32[4] = {scale, clean steps since the last change, steps skipped in total, steps skipped in a row} then moves as apex's
 * LossScaler.update_scale does for loss_scale="dynamic":
 *   found:      scale *= backoff; clean = 0; both skipped counters += 1
 *   otherwise:  clean += 1; skipped in a row = 0; when clean == window: scale = min(max_scale, scale * growth), clean = 0
 * (apex: growth 2, backoff 0.5, window 2000, max_scale 2^24, no floor; the reference starts at 2^20).  window == 0 is a STATIC scale: it
 * never changes (no backoff either; the counters still move), and a non-finite step is still skipped -- apex's static mode would step into the NaNs instead.  The counters are f32,
 * exact to 2^24 steps.  The host reads nothing.  Refused before the device is touched: a null partials, state or ctl, npart outside
 * [1, 4096], growth < 1, backoff outside (0, 1], window < 0, max_scale <= 0. */
int ecamp_sgd_scale_update(const float* partials, int32_t npart, float* state, float* ctl, float* norm_out, float growth, float backoff,
                           int32_t window, float max_scale, ecampStream_t stream);
/* The stem's parameter gradients that are sums of rows of one table (`--train_pos_embed`: timm's pos_embed is a trained parameter,
 * Fine-tuning/Classification/train.py:377-380).  dx [B, T, D] contiguous, the gradient at the stem's output, in `dtype` (0: f32, 1: the
 * build's 16-bit format).  With S[t, d] = sum_b dx[b, t, d], formed ONCE by this call:
 *   dpos[t, d] += S[t, d]                     dpos f32 [T, D]: pos_embed
 *   dcls[d]    += S[0, d]                     dcls f32 [D]:    cls_token
 *   dbias[d]   += sum_{t = 1 .. T-1} S[t, d]  dbias f32 [D]:   patch_embed.proj.bias (the cls row carries no patch)
 * The outputs ACCUMULATE (parameter gradients in the arena, zeroed by zero_grad).  dcls and dbias are given together, or both NULL (only
 * dpos is then touched).  One pass over dx, every sum in one fixed order that is a function of (B, T, D, dtype) alone: no atomics, two
 * calls on equal inputs give equal bits.  B >= 1, T >= 2, D a positive multiple of 8 (16 bits) or 4 (f32); dx, dpos, dcls, dbias and ws
 * 16-byte aligned.  ws: ecamp_pos_embed_grad_workspace_bytes(...) bytes of device memory, scratch (0 for a shape the launch refuses). */
int64_t ecamp_pos_embed_grad_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t dtype);
int ecamp_pos_embed_grad(const void* dx, float* dpos, float* dcls, float* dbias, int64_t B, int32_t T, int32_t D, void* ws, int32_t dtype,
                         ecampStream_t stream);
/* Stochastic depth on the ViT residual stream: timm's DropPath(scale_by_keep=True) inside timm's Block, which the reference fine-tunes
 * with drop_path_rate=0.1 (Fine-tuning/Classification/train.py:127; rates linear over the blocks, timm vision_transformer.py).
 *   out[b, t, :] = res[b, t, :] + s_b * y[b, t, :],   s_b = 0 or 1 / (1 - p)
 * res, y, out [B*T, D] contiguous rows.  Sample b is kept iff element b of the library's dropout convention under (seed, offset) is: the
 * kept set is ecamp_dropout_mask(keep, B, p, seed, offset).  No mask is stored; ecamp_drop_path_bwd regenerates it.  Dtype pairs
 * (res_dtype, y_dtype): (1, 1) the 16-bit modes, (0, 0) the f32 parity mode, (0, 1) the f32 residual stream with a 16-bit branch; `out`
 * has res's dtype.  f32 arithmetic, one rounding to the output format.  `out` may be `y` itself when the dtypes agree, and may overlap
 * neither res nor (otherwise) y.  A dropped sample's y is not read and its output rows are res's bits.  D % 4 == 0 (16-byte accesses
 * when D % 8 == 0 in 16 bits or D % 4 == 0 in f32, else 8-byte ones; pointers aligned accordingly), 0 <= p < 1.  Deterministic. */
int ecamp_drop_path_fwd(const void* res, const void* y, void* out, int64_t B, int32_t T, int32_t D, float p, uint64_t seed, uint64_t offset,
                        int32_t res_dtype, int32_t y_dtype, ecampStream_t stream);
/* Its backward with respect to y: dy[b, t, :] = s_b * dout[b, t, :] in `dtype` (the gradient stream's format: 1, or 0 in the f32 mode);
 * the gradient of res is dout itself.  dy may not overlap dout.  A dropped sample's dout is not read and exact +0 is written. */
int ecamp_drop_path_bwd(const void* dout, void* dy, int64_t B, int32_t T, int32_t D, float p, uint64_t seed, uint64_t offset, int32_t dtype,
                        ecampStream_t stream);

/* ---- optional in-process timing (bench.py roofline): HIP-event pairs around every GEMM / attention launch ---- */
int ecamp_prof_enable(int on);
int ecamp_prof_collect(int category, double* total_ms, double* total_work, int64_t* count); /* 0 gemm bf16, 1 gemm f32, 2 attention, 3 gemm fp8; <0 clears */
/* event pairs the timing facility currently holds: bounded (a pool of 4096 pairs whose finished records are folded into running
 * totals), however many steps run under `main_pretrain.py --profile` */
int64_t ecamp_prof_live_events(void);

/* ---- development ABI: NOT part of the drop-in boundary.  A C consumer sees these only with -DECAMP_DEV_ABI; the library always
 * exports them and the Python binding (which parses this header) binds them for tests/ and tools/ only.  No reference counterpart.
 *   ecamp_dev_spin              `blocks` workgroups spinning for `cycles` shader clocks on `stream` (tools/hog_probe.py: a stand-in
 *                               for a communication kernel sharing the GPU with the training step)
 *   ecamp_gemm_q8_launches      GEMM calls routed to the persistent 256x256x64 kernel so far (tests assert that it really ran)
 *   ecamp_wgrad_group_launches  grouped weight-gradient launches issued so far (tests assert that the grouped path really ran)
 *   ecamp_gemm_f8_q8_launches   ecamp_gemm_fp8 calls routed to the persistent 256 x 256 x 128 e4m3 kernel so far
 *   ecamp_attn_head_launches    launches of the head-resident bf16 attention kernels (one workgroup per (batch, head)) so far
 *   ecamp_dropout_mask          keep[e] = 1 iff element e of a tensor survives dropout(p) under (seed, offset): the Philox mask every kernel
 *                               of this library regenerates (attention probabilities: e = ((b*H + h)*Tq + i)*Tk + j; LayerNorm / embedding
 *                               dropout: e = row*cols + col), as bytes -- lets the tests and the oracle replay the reference's dropout
 *                               sites (context_fusion.py:28-57, bert_modeling.py:113,131) under the SAME masks in plain PyTorch */
#ifdef ECAMP_DEV_ABI
int ecamp_dropout_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, uint64_t offset, ecampStream_t stream);
int ecamp_dev_spin(int32_t blocks, int32_t threads, int64_t cycles, ecampStream_t stream);
int64_t ecamp_gemm_q8_launches(void);
int64_t ecamp_wgrad_group_launches(void);
int64_t ecamp_gemm_f8_q8_launches(void);
int64_t ecamp_gemm_q16_launches(void);   /* GEMM calls routed to the four-wave 16x16x32 kernel (csrc/gemm_q16.h) so far */
int64_t ecamp_attn_head_launches(void);
/* per-tag totals of the profiled launches, "<tag> <n> <ms> <flop>" lines.  GEMM tags: name:form:e<epi>:M:N:K:<w tile | s split> (per form,
 * epilogue and shape).  Attention tags say which kernel family served the call:
 *   attn:<head|resident|stream|long|f32>:<f|b>:<hd>:<Tq>:<Tk>:k<KCH>F<FLAGS>b<bits>w<waves>
 * f / b = forward / backward call; KCH = the 64-key chunks the kernel is instantiated on (0: more than 256 keys, -: the family has
 * none); FLAGS = key mask or dropout; bits = the saved dropout bits are written (f) or read (b); waves per workgroup. */
int64_t ecamp_prof_dump(char* buf, int64_t cap);
#endif

#ifdef __cplusplus
}
#endif
#endif
