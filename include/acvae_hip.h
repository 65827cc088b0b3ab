/* acvae_hip.h — C ABI of libacvae_hip.so: the MI355X (gfx950) kernels behind AC-VAE's training hot path.
 *
 * The reference (XinMing0411/AC-VAE) is pure Python on torch.nn and has NO FFI / operator API of its own
 * (SURVEY.md F1, §8(b)); this ABI is therefore build-defined.  Each entry point names the reference
 * computation it replaces (file:line relative to the reference root).  The Python host side
 * (the acvae_amd package) mirrors the reference's module classes and calls these through ctypes; see
 * INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless its name ends in _host.
 *   - the caller owns every buffer, workspaces included; the library never allocates or frees device
 *     memory (no hipMalloc / hipFree anywhere in csrc/; tests/test_abi_cpu.py greps for it).
 *   - Mutable state inside the library, ALL of it:
 *       (1) a per-THREAD, per-device pool of 64 HIP events used for the fork / join edges of the two-stream calls
 *           (thread_local: concurrent calls from different host threads share nothing, so every entry point is
 *           re-entrant across threads and streams);
 *       (2) the opt-in timing ring (acvae_prof_*, mutex-guarded, empty unless enabled);
 *       (3) one slot per DEVICE for the persistent launches (csrc/decode_persist.hip), mutex-guarded: the HIP event that
 *           chains a device's persistent launches behind each other, the device's CU count, which kernels had their
 *           dynamic-LDS limit raised there, and the status pointer registered with acvae_persist_status_register.
 *     There are no process-global behaviour switches: what used to be acvae_set_decode_persist / _decode_defer /
 *     _attn_split are per-call `flags` (ACVAE_FLAG_*).  The library reads ONE environment variable, once per process into
 *     a static constant (never written afterwards): ACVAE_CONV_WINO (encoder.hip: 0 = implicit-GEMM convolutions), the
 *     A/B switch the benchmark and the tests still use.
 *   - Workspaces (`saved`, `scratch`, `ws`), sized by the `*_bytes` function named beside each entry:
 *       (1) the declared size is exact: a call touches no byte outside [ptr, ptr + declared bytes);
 *       (2) the contents on entry are arbitrary (whatever the allocator last held there): every ticket, arrival counter and
 *           accumulator inside a workspace is zeroed by the call itself.  The caller zeroes ONLY: the first 1024 bytes of
 *           acvae_attn_fwd's workspace, once; the tickets of the reducers' test entries called with reset_tickets = 0 (an
 *           earlier call with reset_tickets = 1 does it); the status words of acvae_persist_status_register;
 *       (3) a workspace below the declared size is ACVAE_EWORKSPACE before any HIP call, and nothing is touched.  Where one
 *           function sizes one buffer for two entries it returns the larger need: acvae_decode_scratch_bytes - the forward
 *           and the backward both refuse anything below it; acvae_step_scratch_bytes - acvae_prior_step_fwd is not told H
 *           and A and refuses what is below its own (E, E, E) layout, acvae_decoder_step_fwd what is below its (E, H, A) one.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and nothing synchronises.
 *   - return 0 on success, a negative ACVAE_E* code for bad arguments, or a positive hipError_t.
 *   - fp32 everywhere ("dtype f32"), token ids / lengths int64 (as torch.long).
 *   - "ld*" are leading dimensions in ELEMENTS; rows are addressed as base + row*ld.
 */
#ifndef ACVAE_HIP_H
#define ACVAE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ACVAE_ABI_VERSION 3
int acvae_abi_version(void);

/* Per-call option bits (`flags`, the last argument of the entry points that take them; 0 = defaults). */
#define ACVAE_FLAG_NO_PERSIST 1          /* decode / posterior: the per-step launches instead of the persistent kernels */
#define ACVAE_FLAG_DEFER_PARAM_GRADS 2   /* acvae_decode_bwd: parameter gradients trail on aux_stream (see there) */
#define ACVAE_FLAG_NO_ATTN_SPLIT 4       /* acvae_attn_fwd: never the split-over-frames form */
#define ACVAE_FLAG_ROLLOUT_GRAD 16       /* acvae_decode_fwd_sampled with caps == NULL / acvae_decode_bwd: a differentiable rollout (see there) */
#define ACVAE_FLAG_TEST_STALL 8          /* test aid: a persistent launch is queued one workgroup short with a short spin
                                            bound, so that its roles give up as they would if part of the grid were not
                                            resident; exercises the abort -> NaN -> status path below */

/* Persistent launches (the teacher-forced decode loop and the posterior BiGRU, forward and backward: one launch each whose
 * workgroups hand results to each other and therefore must ALL be resident).  The library (1) takes that path only when the
 * occupancy calculator says the whole grid fits the current device, (2) chains a device's persistent launches behind each
 * other so that two never share the chip, and (3) bounds every wait: a launch that still cannot finish (another PROCESS
 * holds the CUs) gives up, a one-workgroup tail kernel behind it overwrites its outputs with NaN and sets status words
 * the caller registered for the device:
 *   status_words_host: 8 uint32 in page-locked, device-visible host memory owned by the caller (hipHostMalloc /
 *   torch pin_memory), zeroed by the caller; word k (0 decode fwd, 1 decode bwd, 2 posterior fwd, 3 posterior bwd) and word 4
 *   ("any") become 1.  The caller reads them at a point where the stream has drained (acvae_amd: TrainStep's in-flight event,
 *   Hybrid_VAEModel.check_persistent_launches) and raises.  NULL unregisters.  Without a registered pointer only the NaNs tell. */
int acvae_persist_status_register(int device, void* status_words_host);

/* ---------------------------------------------------------------------------------------------
 * Generic dense products on fp32 MFMA (v_mfma_f32_32x32x2_f32).  Replace torch.nn.Linear /
 * F.linear call sites of the path (models/attn_model.py:32, models/decoder.py:198,
 * models/text_encoder.py:192,255, models/vae_model.py:726) and their autograd backward.
 *   NT: C[M,N] = A[M,K] . B[N,K]^T (+ bias[N]) (+ C if accumulate)
 *   TN: C[M,N] = sum_k A[K,M]^T . B[K,N]   (weight gradients: dW = dY^T . X)
 * ------------------------------------------------------------------------------------------- */
int acvae_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, float* C,
                  int64_t ldc, int M, int N, int K, int accumulate, void* stream);
int acvae_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N,
                  int K, int accumulate, float* slab_ws, int64_t slab_ws_bytes, void* stream);
int64_t acvae_gemm_tn_workspace_bytes(int M, int N, int K);
/* out[c] = sum_r x[r,c] of a contiguous [rows, cols] matrix (bias gradients); deterministic (fixed-order fp64 combine) */
int64_t acvae_colsum_workspace_bytes(int cols);
int acvae_colsum(const float* x, int rows, int cols, float* out, void* ws, int64_t ws_bytes, void* stream);

/* The cross-workgroup reductions of the composite drivers, as C entry points for the tests (the drivers reach them only at
 * their own shapes).  Each hands partial results from workgroup to workgroup: the last to arrive at a ticket sums them and
 * resets the ticket.  reset_tickets = 1 zeroes the workspace's tickets first, as a composite call does at its entry;
 * 0 relies on every earlier reducer on that workspace having left its ticket at zero.  The *_plan queries are host
 * arithmetic and come from the functions the dispatchers use.
 *   acvae_gemm_nt_dual_ws  C = A1 . B1^T (+ A2 . B2^T if A2) (+ bias) (+ C): the NT product with the split-K workspace of
 *                          acvae_gemm_nt_splitk_workspace_bytes() (ws = NULL: no split, as acvae_gemm_nt);
 *                          acvae_gemm_nt_split_plan: 0 = the 128-row tile kernel, else its split count S (1: no split);
 *                          K2 > 0 means the dual form
 *   acvae_gemm_nt_pair_c   two independent NT products of M <= 64 rows in one launch (no split)
 *   acvae_gemm_tn_fused_c  acvae_gemm_tn with the slab sum in the same launch: ws = tickets | slabs of
 *                          acvae_gemm_tn_fused_workspace_bytes (0: one slice); acvae_gemm_tn_fused_plan: the slices it
 *                          launches with ws_bytes of workspace (1: it falls back to acvae_gemm_tn without one)
 *   acvae_gemm_tn_group_c  up to 8 such products in ONE launch, each bit for bit what its own acvae_gemm_tn_fused_c call
 *                          gives (accumulate = 0): A / B / C host tables of device pointers, lda / ldb / ldc / M / N / K host
 *                          arrays.  Only products of the 128 x 128 vector tile: M > 64, M and N multiples of 4, A and B 16-B
 *                          aligned, lda and ldb multiples of 4 (anything else, a NULL, n outside [1, 8]: ACVAE_EINVAL).  All
 *                          jobs are live at once: ws = tickets | the slabs of EVERY sliced job,
 *                          acvae_gemm_tn_group_workspace_bytes (0: no job is sliced; -1: bad shapes, or more sliced tiles
 *                          than tickets); a smaller ws is ACVAE_EWORKSPACE.  All refusals come before any HIP call.
 *   acvae_colsum_batch     up to 6 column sums (as acvae_colsum) in one launch: x / out / out_b are host tables of device
 *                          pointers (out_b or its entries may be NULL), P / width host int arrays; ws: tickets | group
 *                          sums, acvae_colsum_batch_workspace_bytes for one launch;  acvae_colsum_batch_plan: 1 = one
 *                          launch, 0 = one launch per job (one job, more than 128 column blocks, or a smaller ws) */
int64_t acvae_gemm_nt_splitk_workspace_bytes(void);
int acvae_gemm_nt_split_plan(int M, int N, int K1, int K2, int with_ws);
int acvae_gemm_nt_dual_ws(const float* A1, int64_t lda1, const float* B1, int64_t ldb1, int K1, const float* A2,
                          int64_t lda2, const float* B2, int64_t ldb2, int K2, const float* bias, float* C, int64_t ldc,
                          int M, int N, int accumulate, float* ws, int64_t ws_bytes, int reset_tickets, void* stream);
int acvae_gemm_nt_pair_c(const float* A0, int64_t lda0, const float* B0, int64_t ldb0, int K0, const float* bias0, float* C0,
                         int64_t ldc0, int N0, int acc0, const float* A1, int64_t lda1, const float* B1, int64_t ldb1, int K1,
                         const float* bias1, float* C1, int64_t ldc1, int N1, int acc1, int M, void* stream);
int64_t acvae_gemm_tn_fused_workspace_bytes(int M, int N, int K);
int acvae_gemm_tn_fused_plan(int M, int N, int K, int64_t ws_bytes);
int acvae_gemm_tn_fused_c(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N,
                          int K, int accumulate, float* ws, int64_t ws_bytes, int reset_tickets, void* stream);
int64_t acvae_gemm_tn_group_workspace_bytes(int n, const int* M, const int* N, const int* K);
int acvae_gemm_tn_group_c(int n, const void* const* A, const int64_t* lda, const void* const* B, const int64_t* ldb,
                          const void* const* C, const int64_t* ldc, const int* M, const int* N, const int* K, void* ws,
                          int64_t ws_bytes, int reset_tickets, void* stream);
int64_t acvae_colsum_batch_workspace_bytes(int n, const int* P, const int* width);
int acvae_colsum_batch_plan(int n, const int* P, const int* width, int64_t ws_bytes);
int acvae_colsum_batch(int n, const void* const* x, const int* P, const int* width, const void* const* out,
                       const void* const* out_b, void* ws, int64_t ws_bytes, int reset_tickets, void* stream);
/* out[c,r] = in[r,c] */
int acvae_transpose(const float* in, int64_t ld_in, float* out, int64_t ld_out, int rows, int cols, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A3  Seq2SeqAttention.forward  models/attn_model.py:20-46, with the loop-invariant half of
 * h2attn hoisted:  encproj[n,s,:] = W[:, hs_dec:] . h_enc[n,s] + b  (once per batch),
 * qproj[row,:] = W[:, :hs_dec] . h_dec[row]  (per query).  Query row (n,j), n<N, j<Tq lives at
 * base + n*stride_n + j*stride_j for qproj / ctx / weights (lets a decode step address column t of
 * batch-major [N,Tc,.] buffers).  score = v . tanh(qproj + encproj), positions s >= lens[n] get
 * -1e10 before the softmax (attn_model.py:41), ctx = sum_s w_s h_enc[n,s].
 * ------------------------------------------------------------------------------------------- */
/* acvae_attn_fwd with N * Tq <= 128 query rows and S > 16 splits the frames of a row over workgroups (one decode step of the
 * step API / beam search / sampled decode; results equal to the one-workgroup form up to the summation order of the softmax
 * denominator and the context) - when the caller hands over `ws` of acvae_attn_fwd_workspace_bytes (0: the shape never
 * splits).  Its first 1024 bytes are arrival counters: ZERO them once (hipMemsetAsync) before the first call; every call
 * leaves them zero, so stream-ordered calls may reuse the workspace; calls that can run side by side need one each.
 * ws == NULL or ACVAE_FLAG_NO_ATTN_SPLIT: the one-workgroup form. */
int64_t acvae_attn_fwd_workspace_bytes(int N, int Tq, int S, int A, int E);
int acvae_attn_fwd(const float* qproj, int64_t q_sn, int64_t q_sj, const float* encproj, const float* enc,
                   const int64_t* lens, const float* v, float* ctx, int64_t c_sn, int64_t c_sj, float* weights,
                   int64_t w_sn, int64_t w_sj, int N, int Tq, int S, int A, int E, void* ws, int64_t ws_bytes, void* stream,
                   int flags);
/* Test aid: y[i] = the tanh the attention kernels evaluate (hardware exp2 / rcp form, absolute error <= 2.5e-7 (measured 2.1e-7); a library built
 * with -DACVAE_EXACT_TANH uses tanhf instead, for parity debugging). */
int acvae_tanh_att(const float* x, float* y, int64_t n, void* stream);
/* Backward of the above for upstream dctx (attention weights carry no gradient on this path).
 * dencproj [N,S,A] and denc [N,S,E] are ACCUMULATED into (+=); dv_part [N,A] is accumulated into;
 * dqproj rows are written.  `ws`: scratch of acvae_attn_bwd_workspace_bytes(N,Tq,S,A). */
int64_t acvae_attn_bwd_workspace_bytes(int N, int Tq, int S, int A);
int acvae_attn_bwd(const float* dctx, int64_t dc_sn, int64_t dc_sj, const float* qproj, int64_t q_sn, int64_t q_sj,
                   const float* encproj, const float* enc, const int64_t* lens, const float* v,
                   const float* weights, int64_t w_sn, int64_t w_sj, float* dqproj, int64_t dq_sn, int64_t dq_sj,
                   float* dencproj, float* denc, float* dv_part, float* ws, int64_t ws_bytes, int N, int Tq, int S,
                   int A, int E, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reparameterisation  z = eps * exp(.5*logvar) + mu   models/text_encoder.py:196-197,259-262.
 * `ml` holds [rows, 2E] = [mu | logvar] (the Linear output, split at half: text_encoder.py:257-258).
 * Writes mean/log/z (each row stride ld_out) and, if z2 != NULL, a second copy of z (row stride ld_z2).
 * ------------------------------------------------------------------------------------------- */
int acvae_reparam_fwd(const float* ml, int64_t ld_ml, const float* eps, int64_t ld_eps, float* mean, float* logv,
                      float* z, int64_t ld_out, float* z2, int64_t ld_z2, int rows, int E, void* stream);
/* dml[:, :E] = dz + dmean_ext ; dml[:, E:] = dz*eps*.5*exp(.5*logvar) + dlog_ext  (ext terms may be NULL) */
int acvae_reparam_bwd(const float* dz, int64_t ld_dz, const float* dmean_ext, const float* dlog_ext, int64_t ld_ext,
                      const float* logv, int64_t ld_lv, const float* eps, int64_t ld_eps, float* dml, int64_t ld_dml,
                      int rows, int E, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A9  Normal_kl_loss.forward  utils/train_util.py:259-266:  sum over E, mean over ALL rows (unmasked, F8).
 * Inputs are [rows,E] contiguous.  `partials` is a scratch of acvae_kl_partials(rows,E) floats.
 * ------------------------------------------------------------------------------------------- */
int64_t acvae_kl_partials(int64_t n_elem);
int acvae_gauss_kl_fwd(const float* mu1, const float* lv1, const float* mu2, const float* lv2, float* partials,
                       float* out_scalar, int64_t rows, int E, void* stream);
/* grad_out: device scalar (dLoss/dKL).  Any of the four outputs may be NULL. */
int acvae_gauss_kl_bwd(const float* mu1, const float* lv1, const float* mu2, const float* lv2, const float* grad_out,
                       float* dmu1, float* dlv1, float* dmu2, float* dlv2, int64_t rows, int E, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A6  CaptionModel.sample_next_word (greedy)  models/word_model.py:173-207  and
 * A8  LabelSmoothingLoss.forward  utils/train_util.py:243-251 / torch CrossEntropyLoss (runner :222-227)
 * A13 masked CrossEntropyLoss / LabelSmoothingLoss  losses/loss.py:18-70
 * One pass over logits [N,T,V] (row (n,t) at logits + n*ld_n + t*ld_t) producing per-row
 * argmax (first maximum), max log-prob and log-sum-exp; the CE kernels reuse the row stats.
 * A row (n,t) is valid iff t < lens1[n] (lens1 = cap_lens-1; NULL = all valid).
 * ------------------------------------------------------------------------------------------- */
int acvae_row_logsoftmax_argmax(const float* logits, int64_t ld_n, int64_t ld_t, int64_t* argmax, float* max_logprob,
                                float* lse, int64_t o_sn, int64_t o_st, int N, int T, int V, void* stream);
/* The non-greedy branches of sample_next_word (models/word_model.py:188-203) for rows (n,t) of logits as above.
 *   ACVAE_SAMPLE_GUMBEL      w = argmax_c (log_softmax(logits)_c + g_c) / temp, g = -log(-log(U+1e-20)+1e-20) with
 *                            U = torch.rand(N,V) drawn by the caller on the CPU generator (:189-191);
 *   ACVAE_SAMPLE_MULTINOMIAL w = torch.multinomial(exp(log_softmax(logits) / temp), 1) = argmax_c p_c / q_c with
 *                            q = empty(N,V).exponential_(1), which is how ATen draws one sample per row; the caller
 *                            draws q the same way.
 * noise row (n,t) at noise + n*nz_sn + t*nz_st (V floats: g or q).  Writes w (int64) and log_softmax(logits)[w]
 * (the reference's "probs") at w_out / logprob_out + n*o_sn + t*o_st.  First maximum wins (torch.max). */
#define ACVAE_SAMPLE_GREEDY 0
#define ACVAE_SAMPLE_GUMBEL 1
#define ACVAE_SAMPLE_MULTINOMIAL 2
/* n floats of sampling noise generated on the device (counter-based Philox, element i from (seed, i)): Gumbel noise for
 * ACVAE_SAMPLE_GUMBEL, Exp(1) draws for ACVAE_SAMPLE_MULTINOMIAL - what the caller otherwise draws on the CPU generator
 * (models/word_model.py:188-203).  Same distributions, another random stream: the opt-in fast mode of method="sample" /
 * "gumbel"; the CPU-generator mode stays the parity default. */
int acvae_sample_noise(float* noise, int64_t n, int method, uint64_t seed, void* stream);
int acvae_sample_next_word(const float* logits, int64_t ld_n, int64_t ld_t, const float* noise, int64_t nz_sn,
                           int64_t nz_st, int method, float temp, int64_t* w_out, float* logprob_out, int64_t o_sn,
                           int64_t o_st, int N, int T, int V, void* stream);
/* The same draw restricted to a prefix of the row's words: top-k and nucleus (top-p) sampling.  No counterpart in the
 * reference.  Per row of V logits x:
 *   order      x descending, equal values by lower index (a stable sort on -x);
 *   pi         the distribution the method samples from: softmax(x / temp) for ACVAE_SAMPLE_MULTINOMIAL; softmax(x) for
 *              ACVAE_SAMPLE_GUMBEL, where `temp` divides every score (lp + g) / temp alike and so moves no argmax - in the
 *              reference's Gumbel branch temp has no effect on the word, and it has none on the nucleus here;
 *   top_k      >= 0, 0 = off: keep the first min(top_k, V) words of the order;
 *   top_p      in (0, 1], exactly 1 = off: keep the word at rank r iff the mass of the ranks before it is < top_p (the
 *              shortest prefix whose mass reaches top_p; rank 0 is always kept).  The masses are fp32 sums in a fixed
 *              order (bit-reproducible), so against exact arithmetic the cut may sit a few words off where the prefix
 *              mass passes top_p within ~1e-5;
 *   both       the shorter of the two prefixes.
 * w is the first-index argmax over the kept words of acvae_sample_next_word's score, with the same noise: one value per
 * word of the row is consumed, kept or not, so a seeded run uses the same random stream with and without truncation.
 * logprob_out stays log_softmax(x)[w] of the FULL row (the reference's sampled_logprobs), which is NOT the log-probability
 * of w under the truncated distribution.  kept_out (may be NULL): int32, the size of the kept prefix, strided by
 * o_sn / o_st as the other outputs.  With both knobs off this is acvae_sample_next_word bit for bit, and kept = V.
 * -inf logits are words of mass 0; a row with a NaN terminates and touches nothing out of range, its word is unspecified.
 * No workspace.  ACVAE_EINVAL for top_k < 0, top_p outside (0, 1] or NaN, and for what acvae_sample_next_word refuses. */
int acvae_sample_next_word_truncated(const float* logits, int64_t ld_n, int64_t ld_t, const float* noise, int64_t nz_sn,
                                     int64_t nz_st, int method, float temp, int64_t* w_out, float* logprob_out,
                                     int64_t o_sn, int64_t o_st, int N, int T, int V, int top_k, float top_p,
                                     int32_t* kept_out, void* stream);
/* reduction: 0 none (writes loss_rows only), 1 mean over valid rows, 2 sum.  loss_rows [N,T] (0 at invalid rows).
 * V >= 2: a one-word vocabulary has no s / (V - 1) and no gradient; V = 1 is ACVAE_EINVAL, forward and backward, for any
 * smoothing.  lens1 may be NULL (every row valid), hold 0 (no valid row in the clip) or exceed T (counted as T). */
int acvae_ls_ce_fwd(const float* logits, int64_t ld_n, int64_t ld_t, const int64_t* targets, int64_t tg_sn,
                    const int64_t* lens1, const float* lse, float smoothing, int reduction, float* loss_rows,
                    float* out_scalar, int N, int T, int V, void* stream);
/* dlogits [N,T,V] contiguous rows (ld_n, ld_t as logits); grad_out device scalar; grad_rows optional [N,T]
 * (reduction none).  Invalid rows get zeros. */
int acvae_ls_ce_bwd(const float* logits, int64_t ld_n, int64_t ld_t, const int64_t* targets, int64_t tg_sn,
                    const int64_t* lens1, const float* lse, float smoothing, int reduction, const float* grad_out,
                    const float* grad_rows, float* dlogits, int N, int T, int V, void* stream);
/* Self-critical sequence training, utils/train_util.py:398-409 (scst_Loss / Nscst_Loss; models/seq_train_model.py:57-65):
 *   loss = mean_n sum_t -sampled_logprobs[n,t] * reward[n] * mask[n,t],  mask[n,0] = 1, mask[n,t] = seqs[n,t-1] != end_idx.
 * acvae_scst_loss_fwd writes coef[n,t] = -reward[n] * mask[n,t] / N (= d loss / d sampled_logprobs) and the device scalar
 * loss = sum(coef * sampled_logprobs), summed in a fixed order (one workgroup, no atomics: bit-reproducible); entries whose
 * coef is 0 are not read into the sum.  All of [N,Tc] contiguous, reward [N] f32, seqs i64.  The library's rollout runs
 * every step, and rows that have finished hold end_idx, so steps behind a row's <end> count as finished.
 * acvae_logprob_bwd: d_logits[r,v] = coef[r] * ((v == seqs[r]) - exp(logits[r,v] - lse[r])) over `rows` rows of V floats,
 * row stride ld (>= V) for logits and d_logits alike; lse / seqs / coef [rows].  lse is NOT recomputed: pass the forward's
 * own, which acvae_decode_fwd_sampled keeps in `saved` at byte offset acvae_decode_saved_lse_offset(dims) as f32 [N,Tc]
 * (or acvae_row_logsoftmax_argmax's).  A row whose coef is 0 is written as zeros and its logits are not read.  One read
 * and one write of the rows, 16-byte accesses when V and ld are multiples of 4 and both bases are 16-B aligned. */
int acvae_scst_loss_fwd(const float* sampled_logprobs, const int64_t* seqs, const float* reward, int end_idx, float* coef,
                        float* loss, int N, int Tc, void* stream);
int acvae_logprob_bwd(const float* logits, int64_t ld, const float* lse, const int64_t* seqs, const float* coef,
                      float* d_logits, int64_t rows, int V, void* stream);
/* The SCST reward on the device: CIDEr-D of the rollouts' token rows against reference tables prepared on the host
 * (acvae_amd/cider.py).  Replaces utils/score_util.py:5-96 (compute_batch_score / compur_batch_score_samplen: words to the
 * host, strings, pycocoevalcap's dictionary scorer) and the reward lines of models/seq_train_model.py:47-65 and
 * utils/train_util.py:315-321.  All arithmetic is float64 and every sum has a fixed order (bit-reproducible).
 *
 * An n-gram of k <= 4 token ids w_0..w_{k-1} is the 64-bit key sum_j (w_j + 1) << (16 j); ids outside [0, 65534) match
 * nothing.  Tables (device, the caller's):
 *   idf_keys / idf_vals [n_idf]   ascending keys of the batch's in-vocabulary reference n-grams and their idf; a key
 *                                 not found has idf = log_d (ln of the number of documents)
 *   ref_keys / ref_w [n_entries]  per reference r the slice [ref_off[r], ref_off[r+1]) of ascending keys and
 *                                 tf * idf weights; ref_norm [n_refs, 4] its norm per order (over ALL its n-grams, the
 *                                 out-of-vocabulary ones included), ref_len [n_refs] its number of bigrams
 *   doc_ref [n_docs + 1]          the references of document d are [doc_ref[d], doc_ref[d+1])
 *   row_doc / row_src [n]         per row its document and the row whose words score it (rows sharing a key)
 *   len_factor [n_len]            exp(-delta^2 / (2 sigma^2)) for |delta| = 0 .. n_len - 1 (clamped to the last entry)
 * acvae_ciderd_scores: token rows i64 seqs0 [n, max_length] and, with n_sets == 2, seqs1 [n, max_length] (row stride ld
 * for both) -> score [n_sets * n]; row s * n + i is scored by the words of row row_src[i] of set s.  A row is cleaned as
 * the reference's sentence conversion does it: start_idx skipped wherever it stands, cut at the first end_idx.  One
 * wavefront per row.  Every index read from a table is clamped to its table, so a bad table cannot reach outside one.
 * A NULL pointer, n <= 0, n_sets not 1 or 2, max_length outside [1, ACVAE_CIDER_MAX_LENGTH], ld < max_length, n_docs <= 0,
 * n_refs <= 0, n_len <= 0, or a negative n_idf / n_entries (0 is fine: their arrays are then not read) -> ACVAE_EINVAL
 * before any launch.
 * acvae_ciderd_reward: sample_n <= 1: reward[i] = score[i] - score[n + i] (sampled - greedy, score [2 n]); sample_n >= 2:
 * rows clip-major, reward[i] = score[i] - (sum of the clip's scores - score[i]) / (sample_n - 1) (score [n], n a
 * multiple of sample_n or ACVAE_EINVAL); formed in float64 and rounded once to f32 reward [n]; reward_mean (optional
 * device double) gets the mean of the float64 rewards.  One workgroup. */
#define ACVAE_CIDER_MAX_LENGTH 64
int acvae_ciderd_scores(const int64_t* seqs0, const int64_t* seqs1, int64_t ld, int n, int n_sets, int max_length,
                        int start_idx, int end_idx, const uint64_t* idf_keys, const double* idf_vals, int n_idf,
                        double log_d, const uint64_t* ref_keys, const double* ref_w, int n_entries, const int* ref_off,
                        const double* ref_norm, const int* ref_len, int n_refs, const int* doc_ref, int n_docs,
                        const int* row_doc, const int* row_src, const double* len_factor, int n_len, double* score,
                        void* stream);
int acvae_ciderd_reward(const double* score, int n, int sample_n, float* reward, double* reward_mean, void* stream);
/* Consensus (minimum-Bayes-risk) reranking of a clip's sampled captions: CIDEr-D of every candidate with the clip's OTHER
 * candidates as its references, and the candidate that agrees most with the rest (csrc/consensus.hip, acvae_amd/consensus.py).
 * Token rows i64 seqs [n, max_length] (row stride ld), clip-major: the candidates of clip b are rows b * sample_n + j,
 * j = 0 .. sample_n - 1.  A row is cleaned as acvae_ciderd_scores cleans it (start_idx skipped wherever it stands, cut at the
 * first end_idx); n-grams of orders 1..4 with the key format above; ids outside [0, 65534) count as one unknown word that
 * no table holds.  idf_keys / idf_vals [n_idf]: ascending keys and idf of a CORPUS (not of the batch: a clip's result does
 * not depend on what else is in the launch); a key not found has idf = log_d; n_idf == 0 is fine (the arrays are then not
 * read), and with log_d = 1 every n-gram weighs 1.  len_factor [n_len] as above.  float64:
 *   v_i(g) = count_i(g) idf(g);  norm_k(i) = sqrt(sum_g v_i(g)^2);  len(i) = the number of bigrams of candidate i
 *   sim_k(i, j) = sum_{g in i} min(v_i(g), v_j(g)) v_j(g), / (norm_k(i) norm_k(j)) if both are non-zero, * len_factor[|len i - len j|]
 *   score[b * sample_n + i] = 10 mean_k (1 / (sample_n - 1)) sum_{j != i} sim_k(i, j);  an empty candidate scores 0
 *   best[b] = the lowest index among the maxima of the clip's scores;  picked[b, :] (optional, i64 [n / sample_n,
 *   max_length], dense) = row b * sample_n + best[b]
 * Every sum has a fixed order (n-grams in order of first appearance, j ascending, orders ((s0 + s1) + s2) + s3): two runs
 * are bit-equal.  No atomics, no transcendental function.  One launch: one workgroup per clip, one wavefront per candidate,
 * all of a clip's vectors in dynamic LDS, 3888 bytes per candidate (62208 bytes at sample_n = 16, inside the 64 KB a launch
 * may ask for without more ado; no workspace).  Limits: 2 <= sample_n <= ACVAE_CONSENSUS_MAX_SAMPLES (the wavefronts of one
 * workgroup), max_length <= ACVAE_CONSENSUS_MAX_LENGTH (one lane per word).  Every index is formed from the launch geometry
 * or clamped.  A NULL seqs / len_factor / score / best, sample_n outside that range, n not a positive multiple of sample_n,
 * max_length outside [1, 64], ld < max_length, n_len <= 0, a negative n_idf, or n_idf > 0 with a NULL table -> ACVAE_EINVAL
 * before any launch. */
#define ACVAE_CONSENSUS_MAX_LENGTH 64
#define ACVAE_CONSENSUS_MAX_SAMPLES 16
int acvae_consensus_scores(const int64_t* seqs, int64_t ld, int n, int sample_n, int max_length, int start_idx, int end_idx,
                           const uint64_t* idf_keys, const double* idf_vals, int n_idf, double log_d,
                           const double* len_factor, int n_len, double* score, int64_t* best, int64_t* picked, void* stream);
/* Diversity of a clip's N captions: the integer statistics behind Div-n, mBLEU and the vocabulary size (csrc/diversity.hip,
 * acvae_amd/diversity.py evaluates the formulas on the host).  Token rows i64 seqs [n, max_length] (row stride ld), clip-major
 * as above, cleaned as acvae_consensus_scores cleans them (start_idx skipped wherever it stands, cut at the first end_idx;
 * what stands behind the first end_idx is never interpreted).  A kept id outside [0, V) is one shared out-of-range word.
 * With h_i the cleaned candidate i, L_i its length and c_i(g) the count of n-gram g in it (orders k = 1..4), the record of
 * clip b is ACVAE_DIVERSITY_HEAD + ACVAE_DIVERSITY_PER_CANDIDATE * sample_n int32 at record[b * that]:
 *   [0]            words = sum_i L_i
 *   [1 + k']       distinct_k = the number of different order-k n-grams over all candidates, k' = k - 1 = 0..3
 *   [5 + 6 i]      testlen = L_i
 *   [5 + 6 i + 1]  reflen = the L_j, j != i, that minimises (|L_j - L_i|, L_j) lexicographically (BLEU's "closest")
 *   [5 + 6 i + 2 + k']  correct_k = sum over the different order-k n-grams g of h_i of min(c_i(g), max_{j != i} c_j(g))
 * (guess_k = max(0, L_i - k + 1) follows from testlen.)  seen [V + 1] int32: the plain value 1 is stored at every kept word,
 * slot V for the out-of-range word; the kernel never clears it, so it accumulates over launches (the caller zeroes it once).
 * Integers only: no atomics, no workspace, no scratch; identical racing stores into `seen` are the only sharing between
 * workgroups, so the result does not depend on launch order.  One launch: one workgroup per clip, one wavefront per
 * candidate, static LDS.  Every index is formed from the launch geometry or clamped.  A NULL seqs / record / seen, sample_n
 * outside [2, ACVAE_CONSENSUS_MAX_SAMPLES], n not a positive multiple of sample_n, max_length outside [1, 64], ld < max_length
 * or V outside [1, 65534] -> ACVAE_EINVAL before any launch. */
#define ACVAE_DIVERSITY_HEAD 5
#define ACVAE_DIVERSITY_PER_CANDIDATE 6
int acvae_diversity_stats(const int64_t* seqs, int64_t ld, int n, int sample_n, int max_length, int start_idx, int end_idx,
                          int V, int* record, int* seen, void* stream);
/* Captions against their references: the integer statistics behind BLEU-1..4 and ROUGE-L (csrc/accuracy.hip;
 * acvae_amd/accuracy.py evaluates the formulas on the host).  Token rows i64 seqs [n, max_length] (row stride ld), clip-major:
 * row r belongs to clip r / sample_n, 1 <= sample_n <= ACVAE_CONSENSUS_MAX_SAMPLES.  A row is cleaned as
 * acvae_diversity_stats cleans it (start_idx skipped wherever it stands, cut at the first end_idx; what stands behind the
 * first end_idx is never interpreted).  The references: ref_words [n_words] int32, the words of all references one after the
 * other, a vocabulary id or, for a word outside the vocabulary, any value outside [0, V) (the sentinel; -1 by convention);
 * ref_off [n_refs + 1]: the words of reference j are ref_words[ref_off[j] .. ref_off[j + 1]); clip_ref [n_clips + 1]: the
 * references of clip b are clip_ref[b] .. clip_ref[b + 1] - 1.  A reference has at least one word and may have any number.
 * Matching: a candidate word outside [0, V) matches no reference word, a reference word outside [0, V) matches no candidate
 * word, and two n-grams match only if every word matches.  With h the cleaned row, L its length, R its clip's references
 * and c_s(g) the count of n-gram g in sentence s, the record of row r is ACVAE_ACCURACY_RECORD int32 at record[9 r]:
 *   [0]        testlen = L
 *   [1]        reflen = the len(r), r in R, that minimises (|len(r) - L|, len(r))  ("closest"; ties go to the shorter)
 *   [2 + k']   correct_k = sum over the distinct order-k n-grams g of h of min(c_h(g), max_{r in R} c_r(g)), k' = k - 1 = 0..3
 *   [6]        lcs_p = max_{r in R} LCS(h, r), the length of the longest common subsequence
 *   [7], [8]   lcs_r, len_r = the pair (LCS(h, r), len(r)) with the largest quotient, compared by integer
 *              cross-multiplication; ties go to the earlier reference
 * A clip without references gets reflen = lcs_p = lcs_r = len_r = 0 and correct_k = 0.
 * Integers only: no atomics, no workspace, no scratch, two runs are bit-equal.  One launch, one wavefront per row; the
 * references are streamed 64 words per step, so their number and their lengths are not bounded by the kernel.  Every index
 * is formed from the launch geometry or clamped to its array: offsets that are not monotone or not in range give empty
 * references, never a read outside ref_words [n_words], ref_off [n_refs + 1] or clip_ref [n_clips + 1].  A NULL pointer,
 * sample_n outside [1, ACVAE_CONSENSUS_MAX_SAMPLES], n not a positive multiple of sample_n, max_length outside [1, 64],
 * ld < max_length, V outside [1, 65534], n_clips != n / sample_n, a negative n_words or n_refs, or n_words above 2^30 (the
 * kernel's word indices are int32) -> ACVAE_EINVAL before any launch. */
#define ACVAE_ACCURACY_RECORD 9
int acvae_accuracy_stats(const int64_t* seqs, int64_t ld, int n, int sample_n, int max_length, int start_idx, int end_idx,
                         int V, const int* ref_words, int n_words, const int* ref_off, int n_refs, const int* clip_ref,
                         int n_clips, int* record, void* stream);
/* mean((a-b)^2) over n elements and its backward (runner :317, nn.MSELoss). */
int acvae_mse_fwd(const float* a, const float* b, float* partials, float* out_scalar, int64_t n, void* stream);
int acvae_mse_bwd(const float* a, const float* b, const float* grad_out, float* da, float* db, int64_t n, void* stream);
/* A10 loss assembly, runners/pytorch_runner_vae.py:315-320: loss = ce + w_kl * kl (+ w_mse * mse; mse may be NULL) on device
 * scalars, and its gradient (g, g * w_kl, g * w_mse) - one launch each instead of a chain of scalar tensor kernels. */
int acvae_loss_combine_fwd(const float* ce, const float* kl, const float* mse, float w_kl, float w_mse, float* out, void* stream);
int acvae_loss_combine_bwd(const float* grad_out, float w_kl, float w_mse, float* g_ce, float* g_kl, float* g_mse, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A1  Cnn10.forward  models/encoder.py:672-707 (ConvBlock :606-649) and its backward.
 * feats f32 [N,T,F=64] -> audio_embeds f32 [N,S,512] (S = T/16), audio_embeds_pooled f32 [N,512].
 * `params` / `grads`: pointer tables in the reference's state-dict order for the encoder:
 *   bn0.{weight,bias,running_mean,running_var,num_batches_tracked},
 *   conv_block{1..4}.{conv1.weight, conv2.weight, bn1.{w,b,rm,rv,nbt}, bn2.{w,b,rm,rv,nbt}},
 *   embed_pooled.{weight,bias}                                   (55 entries; weights in OIHW).
 * training != 0: BatchNorm uses batch statistics and updates the running buffers (momentum 0.1,
 * unbiased variance) and dropout (p_block after every block, p_fc around embed_pooled) is applied,
 * drawn from Philox(seed) unless `masks` supplies the 6 (Cnn14_16k: 8) keep-masks explicitly (uint8, the reference's
 * NCHW / [N,512] order: parity tests).  `saved` (acvae_encoder_saved_bytes) carries activations from
 * fwd to bwd; `scratch` (acvae_encoder_scratch_bytes) is free between calls.  Gradients are WRITTEN
 * (not accumulated) for every conv / bn weight and bias; embed_pooled receives none (its output is
 * not consumed on this path, models/vae_model.py:821).
 * `arch` selects the PANNs encoder: ACVAE_ARCH_CNN10 (above) or ACVAE_ARCH_CNN14_16K (SURVEY §8(f) N4,
 * models/encoder.py:871-964): conv_block{1..6} up to 2048 channels, the sixth block pooled (1,1), S = T/32,
 * audio_embeds [N,S,2048], the pooled head is fc1 (2048x2048); its table has 79 entries (…, conv_block6.*, fc1.{w,b})
 * and 8 dropout sites.  acvae_encoder_nparams / acvae_encoder_out_dims report the table length and (S, C).
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_ENC_NPARAMS 55          /* Cnn10 */
#define ACVAE_ARCH_CNN10 0
#define ACVAE_ARCH_CNN14_16K 1
/* ACVAE_ARCH_RESNET38 (models/encoder.py:1169-1234, the PANNs ResNet38): bn0, conv_block1 = ConvBlock(1, 64) pooled 2x2,
 * 16 residual basic blocks (layers [3, 4, 6, 3] at 64 / 128 / 256 / 512 channels; the first block of layers 2-4 pools its
 * input 2x2 and has a downsample AvgPool2d(2) + conv1x1 + BatchNorm2d), avg_pool2d(2), conv_block_after1 =
 * ConvBlock(512, 2048) pooled (1, 1), the fc1 head: S = T/32, audio_embeds [N,S,2048].  fp32 only: ACVAE_ENC_BF16, T < 32
 * or F != 64 with this arch is ACVAE_EINVAL before any launch.  Its table has 241 entries, the reference's state-dict order:
 *   [0..4]    bn0.*                       [5] conv_block1.conv1.weight  [6] conv_block1.conv2.weight
 *   [7..11]   conv_block1.bn1.*           [12..16] conv_block1.bn2.*
 *   from 17, per block resnet.layerL.i in order: conv1.weight, bn1.* (5), conv2.weight, bn2.* (5) and, in layer2.0 /
 *             layer3.0 / layer4.0, downsample.1.weight [C][Cin][1][1], downsample.2.* (5): 12 or 18 entries
 *   [227] conv_block_after1.conv1.weight [228] .conv2.weight [229..233] .bn1.* [234..238] .bn2.*  [239, 240] fc1.{weight,bias}
 * 21 dropout sites (masks in this order, NCHW / [N,2048]): 0 after conv_block1 (p_block), 1..16 inside block k = site-1
 * after relu(bn1) (p = p_block / 2: the reference's 0.1 beside its 0.2), 17 after the pool behind the resnet (p_block), 18
 * after conv_block_after1 (p_block), 19 and 20 around fc1 (p_fc).
 * 36 ReLU sites (acvae_encoder_relu_mask): 0, 1 conv_block1 bn1 / bn2; 2+2k block k's relu(bn1), 3+2k block k's residual
 * relu(bn2(..) + identity) (decision: out > 0); 34, 35 conv_block_after1 bn1 / bn2.
 * acvae_encoder_bwd_hooked calls block_done ONCE, with block = 0, when the gradients of conv_block_after1 (47.2 M of the
 * encoder's 72.7 M parameters) are queued. */
#define ACVAE_ARCH_RESNET38 2
/* OR-ed into `arch`: BASELINE configs[2] "bf16 forward / fp32 loss".  The conv stack's activations (raw conv outputs,
 * pooled tensors, their gradients) and the repacked conv weights are STORED in bf16 and the 3x3 convolutions run on
 * v_mfma_f32_32x32x16_bf16; accumulation, BatchNorm statistics (taken from the rounded tensor that is stored), parameter
 * gradients, parameters and every output of these calls (audio_embeds, pooled) stay fp32.  Same tables, same dropout
 * streams; saved / scratch sizes roughly halve (ask acvae_encoder_saved_bytes / _scratch_bytes with the flag set). */
#define ACVAE_ENC_BF16 256
int acvae_encoder_nparams(int arch);
int acvae_encoder_out_dims(int arch, int T, int* S, int* C);
int64_t acvae_encoder_saved_bytes(int arch, int N, int T, int F);
int64_t acvae_encoder_scratch_bytes(int arch, int N, int T, int F);
int acvae_encoder_fwd(const void* const* params, const float* feats, float* audio_embeds, float* pooled,
                      void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes, int arch, int N, int T,
                      int F, int training, float p_block, float p_fc, uint64_t seed, const uint8_t* const* masks,
                      void* stream);
/* `training` must be the value the forward that filled `saved` was called with: 0 = evaluation-mode BatchNorm
 * (running statistics, no dropout; dY = scale * g, fine-tuning with frozen statistics and the data-parallel
 * equivalence test), != 0 = batch statistics. */
int acvae_encoder_bwd(const void* const* params, void* const* grads, const float* feats,
                      const float* d_audio_embeds, void* saved, int64_t saved_bytes, void* scratch,
                      int64_t scratch_bytes, int arch, int N, int T, int F, int training, float p_block, uint64_t seed,
                      const uint8_t* const* masks, void* stream);
/* Test aid: the ReLU decisions (y * scale + shift > 0, as the backward kernels evaluate them) of BN+ReLU site `site`
 * (0 .. 2*blocks-1: ConvBlock site/2 + 1, bn1 then bn2) read from the `saved` buffer of a forward call, written as uint8
 * [N,C,H,W] - the reference's layout.  A checker evaluates the reference under exactly these decisions instead of
 * tolerating mask bits that two fp32 summation orders put on different sides of zero. */
int acvae_encoder_relu_mask(const void* saved, int64_t saved_bytes, int arch, int N, int T, int F, int site,
                            uint8_t* mask_nchw, void* stream);
/* The same with a host callback: `block_done`, if not NULL, is a `void (*)(int block, void* user)` (passed as void*)
 * that is called on the calling thread right after the kernels producing ALL parameter gradients of ConvBlock `block`
 * (conv1 / conv2 / bn1 / bn2; blocks run nb .. 1) have been queued on `stream`: a data-parallel caller starts the
 * all-reduce of that block's gradient bucket there, behind `stream`, while the shallower blocks still run. */
int acvae_encoder_bwd_hooked(const void* const* params, void* const* grads, const float* feats,
                             const float* d_audio_embeds, void* saved, int64_t saved_bytes, void* scratch,
                             int64_t scratch_bytes, int arch, int N, int T, int F, int training, float p_block,
                             uint64_t seed, const uint8_t* const* masks, void* stream, void* block_done, void* user);

/* ---------------------------------------------------------------------------------------------
 * The encoder's kernels one by one (conv3x3[_bn], bn_mel, bn pieces): the same launchers
 * acvae_encoder_fwd / _bwd sequence, each callable - and tested - alone.  Activations are NHWC
 * [N][H][W][C] fp32 (the reference is NCHW: torch.nn.Conv2d(.., (3,3), (1,1), (1,1), bias=False),
 * models/encoder.py:612-622, 633-649), weights OIHW as in the state dict.  `ws`: scratch of
 * acvae_conv3x3_workspace_bytes / acvae_bn_workspace_bytes for the same dims, 16-byte aligned.
 *   acvae_conv3x3_fwd   Y = conv3x3(act(X), W), act = relu(x * in_scale[ci] + in_shift[ci]) (the PREVIOUS layer's fused
 *                       BatchNorm+ReLU) or the identity when in_scale == NULL.  If bn_out != NULL it also returns THIS
 *                       layer's BatchNorm as [4][Cout] = scale | shift | mean | invstd (y_bn = Y*scale + shift) from the
 *                       batch statistics (training != 0: running buffers updated, momentum 0.1, unbiased variance) or
 *                       from the running buffers (training == 0).  Cin == 1 is the stack's first convolution:
 *                       in_scale / in_shift are then bn0's per-MEL affine [W] (required), W = 64, Cout = 64.
 *   acvae_conv3x3_dgrad dX = conv3x3(dY, flipped / transposed W)           (Cin >= 32)
 *   acvae_conv3x3_wgrad dW[co][ci][tap] = sum_p dY[p][co] * act(X)[p + tap][ci]      (Cin >= 4; Cin == 1: below)
 *   acvae_conv1_first_bwd  first convolution: dW1 [64][1][3][3] and bn0's dgamma / dbeta [64] (x [N,T,64] features,
 *                       bn0 = [4][64] from acvae_bn_mel_fwd).
 *   acvae_bn_mel_fwd    bn0 (BatchNorm2d(64) over the MEL axis, models/encoder.py:655, 679-681) statistics of x [rows,64]
 *                       -> bn_out [4][64]; the normalised tensor is never written: the first convolution applies it.
 *   acvae_bn_relu_pool_fwd  P = dropout(avg_pool2x2(relu(Y*scale + shift)))  (pool != 0) or dropout(relu(..)) (pool == 0:
 *                       ConvBlock pool_size (1,1)); bn = [4][C] as above; dropout p_drop with Philox(seed, site) or an
 *                       explicit keep mask (NCHW order), p_drop = 0 disables.
 *                       The draw, wherever an entry takes (p_drop, seed, site, keep_mask) and keep_mask == NULL - forward
 *                       and backward recompute it, they never store it: element e of the site's STORED output (flat index
 *                       in NHWC order of the pooled / output tensor; n*C + c for the encoders' two head sites) takes
 *                       word e & 3 of r = Philox4x32-10(key = (lo32(seed), hi32(seed)),
 *                       counter = (lo32(e >> 2), hi32(e >> 2), site, 0x5eed5eed)) and is kept iff
 *                       (float)(word >> 8) * 2^-24 >= p_drop, evaluated in fp32; kept elements are multiplied by
 *                       1.0f / (1.0f - p_drop).  tests/philox_ref.py restates it on the host and
 *                       tests/test_dropout_philox_gpu.py holds every kernel that draws to it bit for bit.
 *   acvae_bn_relu_bwd   backward of relu(bn(Y)) for upstream dO: upstream 0 = dO [N,H,W,C] as is, 1 = dO [N,H/2,W/2,C]
 *                       through dropout + 2x2 average pool, 2 = through dropout only.  Writes dgamma, dbeta [C] and dY.
 *                       training == 0: evaluation-mode BatchNorm (dY = scale * g).
 * ------------------------------------------------------------------------------------------- */
int64_t acvae_conv3x3_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int acvae_conv3x3_fwd(const float* X, const float* W_oihw, const float* in_scale, const float* in_shift, float* Y,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, int training, float* bn_out, void* ws, int64_t ws_bytes, int N, int H,
                      int W, int Cin, int Cout, void* stream);
int acvae_conv3x3_dgrad(const float* dY, const float* W_oihw, float* dX, void* ws, int64_t ws_bytes, int N, int H, int W,
                        int Cin, int Cout, void* stream);
int acvae_conv3x3_wgrad(const float* dY, const float* X, const float* in_scale, const float* in_shift, float* dW_oihw,
                        void* ws, int64_t ws_bytes, int N, int H, int W, int Cin, int Cout, void* stream);
int acvae_conv1_first_bwd(const float* x, const float* bn0, const float* W1_oihw, const float* dY, float* dW1,
                          float* dgamma0, float* dbeta0, void* ws, int64_t ws_bytes, int N, int T, int F, void* stream);
/* acvae_conv1_first_bwd with the backward of the BatchNorm + ReLU that follows the first convolution (bn1) folded in:
 * dO [N,T,64,64] is the gradient at bn1's ReLU output, Y1 the convolution's output, bn1 = [4][64] its bn_out.  Returns
 * bn1's dgamma1 / dbeta1 and the outputs acvae_conv1_first_bwd gives for the dY of acvae_bn_relu_bwd (upstream 0, same
 * training flag), bit for bit, without writing that dY.  The workspace must cover acvae_conv3x3_workspace_bytes(N, T, F, 1,
 * 64) + acvae_bn_workspace_bytes(N, T, F, 64). */
int acvae_conv1_first_bwd_bn(const float* x, const float* bn0, const float* W1_oihw, const float* Y1, const float* dO,
                             const float* bn1, float* dgamma1, float* dbeta1, float* dW1, float* dgamma0, float* dbeta0,
                             void* ws, int64_t ws_bytes, int N, int T, int F, int training, void* stream);
/* Winograd F(2x2,3x3) forms of the forward convolution and the data gradient (conv_wino.hip): same contracts, fp32
 * throughout, 2.25x fewer matrix-pipe flops; results differ from the implicit-GEMM forms by fp32 rounding only.
 * W a power of two in 4..64, Cin % 16 == 0, Cout % 64 == 0 (dgrad: the roles of Cin / Cout swap), otherwise
 * ACVAE_EUNSUPPORTED.  Same workspace. */
int acvae_conv3x3_fwd_wino(const float* X, const float* W_oihw, const float* in_scale, const float* in_shift, float* Y,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, int training, float* bn_out, void* ws, int64_t ws_bytes, int N,
                           int H, int W, int Cin, int Cout, void* stream);
int acvae_conv3x3_dgrad_wino(const float* dY, const float* W_oihw, float* dX, void* ws, int64_t ws_bytes, int N, int H,
                             int W, int Cin, int Cout, void* stream);
/* The data gradient of a convolution whose INPUT was relu(batchnorm(Yprev)) - the second convolution of a ConvBlock
 * (models/encoder.py:631-641) - with the first pass of that BatchNorm + ReLU's backward inside: besides dX it returns
 * sum_g[Cin] = sum over pixels of g and sum_gy[Cin] = sum of g * (Yprev - mean) * invstd, g = dX where Yprev * scale + shift > 0.
 * bn_prev = [4][Cin]: scale | shift | mean | invstd (the bn_out of the layer that made Yprev).  The workspace must cover
 * acvae_conv3x3_workspace_bytes for (Cin, Cout) and for (Cout, Cin). */
int acvae_conv3x3_dgrad_bnred_wino(const float* dY, const float* W_oihw, float* dX, const float* Yprev, const float* bn_prev,
                                   float* sum_g, float* sum_gy, void* ws, int64_t ws_bytes, int N, int H, int W, int Cin,
                                   int Cout, void* stream);
/* weight gradient in the same form (Cin % 64 == 0, Cout % 64 == 0): 16 GEMMs over the tiles, split over workgroups into
 * fp32 slabs that are summed in fixed order (in double) and folded through G^T . G. */
int acvae_conv3x3_wgrad_wino(const float* dY, const float* X, const float* in_scale, const float* in_shift, float* dW_oihw,
                             void* ws, int64_t ws_bytes, int N, int H, int W, int Cin, int Cout, void* stream);
/* bf16-storage forms of the three convolutions (acvae_encoder_* with ACVAE_ENC_BF16): X / dY / dX / Y are bf16 NHWC
 * (uint16 bit patterns, round-to-nearest-even), weights OIHW fp32 (rounded to bf16 inside), dW fp32.  Cin % 64 == 0.
 * acvae_conv3x3_fwd_bf16 returns this layer's BatchNorm in bn_out exactly like the fp32 form, from the statistics of the
 * ROUNDED output.  Same workspace size as the fp32 forms. */
int acvae_conv3x3_fwd_bf16(const void* X, const float* W_oihw, const float* in_scale, const float* in_shift, void* Y,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, int training, float* bn_out, void* ws, int64_t ws_bytes, int N,
                           int H, int W, int Cin, int Cout, void* stream);
int acvae_conv3x3_dgrad_bf16(const void* dY, const float* W_oihw, void* dX, void* ws, int64_t ws_bytes, int N, int H, int W,
                             int Cin, int Cout, void* stream);
int acvae_conv3x3_wgrad_bf16(const void* dY, const void* X, const float* in_scale, const float* in_shift, float* dW_oihw,
                             void* ws, int64_t ws_bytes, int N, int H, int W, int Cin, int Cout, void* stream);
int64_t acvae_bn_workspace_bytes(int N, int H, int W, int C);
/* bf16-storage forms of the first convolution and of the BatchNorm pieces, as the bf16 encoder runs them: same contracts
 * as the fp32 forms, Y / P / dO / dY bf16 NHWC, fp32 arithmetic inside, bf16 outputs rounded to nearest even.
 *   acvae_conv1_first_fwd_bf16  acvae_conv3x3_fwd with Cin == 1 (x fp32 [N,T,64] features, in_scale / in_shift bn0's
 *                       affine [64]) writing a bf16 Y; bn_out from the statistics of the ROUNDED Y.
 *   acvae_conv1_first_bwd_bf16  acvae_conv1_first_bwd for a bf16 dY. */
int acvae_conv1_first_fwd_bf16(const float* x, const float* in_scale, const float* in_shift, const float* W1_oihw, void* Y,
                               const float* gamma, const float* beta, float* running_mean, float* running_var,
                               int64_t* num_batches_tracked, int training, float* bn_out, void* ws, int64_t ws_bytes, int N,
                               int T, int F, void* stream);
int acvae_conv1_first_bwd_bf16(const float* x, const float* bn0, const float* W1_oihw, const void* dY, float* dW1,
                               float* dgamma0, float* dbeta0, void* ws, int64_t ws_bytes, int N, int T, int F, void* stream);
int acvae_bn_relu_pool_fwd_bf16(const void* Y, const float* bn, void* P, int N, int H, int W, int C, int pool, float p_drop,
                                uint64_t seed, int site, const uint8_t* keep_mask, void* stream);
int acvae_bn_relu_bwd_bf16(const void* Y, const void* dO, int upstream, const float* bn, float* dgamma, float* dbeta,
                           void* dY, void* ws, int64_t ws_bytes, int N, int H, int W, int C, int training, float p_drop,
                           uint64_t seed, int site, const uint8_t* keep_mask, void* stream);
/* The ResNet38 kernels one by one (resnet.hip), NHWC fp32; bn* = [4][C] scale | shift | mean | invstd as above.
 *   acvae_res_join_fwd   out = relu(y2*bn2.scale + bn2.shift + (yd ? yd*bnd.scale + bnd.shift : x))   (yd == NULL: identity x)
 *   acvae_res_join_bwd   g = dO * (out > 0) -> G; dbeta2 = sum g, dgamma2 = sum g*yhat2 (and the same for bnd where yd != NULL,
 *                        yhat = (y - mean) * invstd); dy2 / dyd = BatchNorm backward of g (training != 0: batch statistics)
 *   acvae_conv1x1_fwd    Y[m][co] = sum_ci X[m][ci] W[co][ci]; partials (optional) [acvae_conv1x1_partials_rows][2][Cout] =
 *                        per 64-pixel tile sum y | sum y^2 (Cin % 16 == 0, Cout % 64 == 0)
 *   acvae_conv1x1_dgrad  dX (+)= dY . W      acvae_conv1x1_wgrad  dW[co][ci] = sum_m dY[m][co] X[m][ci] (fixed-order slab sum)
 *   acvae_avg_pool2_fwd  P = dropout(avg_pool2x2(X)) (floors odd H / W; p_drop = 0: none; mask: explicit NCHW keep-mask)
 *   acvae_avg_pool2_bwd  dX = upsample(dP * dropout) / 4 (pool != 0; 0 behind the last full window) or dP * dropout (pool == 0),
 *                        plus add (if not NULL); dX is [N,H,W,C] */
int acvae_res_join_fwd(const float* y2, const float* bn2, const float* yd, const float* bnd, const float* x, float* out, int N,
                       int H, int W, int C, void* stream);
int64_t acvae_res_join_bwd_workspace_bytes(int N, int H, int W, int C);
int acvae_res_join_bwd(const float* dO, const float* out, const float* y2, const float* bn2, const float* yd, const float* bnd,
                       float* G, float* dy2, float* dyd, float* dgamma2, float* dbeta2, float* dgammad, float* dbetad,
                       int training, void* ws, int64_t ws_bytes, int N, int H, int W, int C, void* stream);
int acvae_conv1x1_partials_rows(int N, int H, int W);
int acvae_conv1x1_fwd(const float* X, const float* W_oi, float* Y, float* partials, int N, int H, int W, int Cin, int Cout,
                      void* stream);
int acvae_conv1x1_dgrad(const float* dY, const float* W_oi, float* dX, int accumulate, int N, int H, int W, int Cin, int Cout,
                        void* stream);
int64_t acvae_conv1x1_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int acvae_conv1x1_wgrad(const float* dY, const float* X, float* dW_oi, void* ws, int64_t ws_bytes, int N, int H, int W, int Cin,
                        int Cout, void* stream);
int acvae_avg_pool2_fwd(const float* X, float* P, int N, int H, int W, int C, float p_drop, uint64_t seed, int site,
                        const uint8_t* mask, void* stream);
int acvae_avg_pool2_bwd(const float* dP, const float* add, float* dX, int N, int H, int W, int C, int pool, float p_drop,
                        uint64_t seed, int site, const uint8_t* mask, void* stream);
int acvae_bn_mel_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, int training, float* bn_out, void* ws, int64_t ws_bytes, int64_t rows,
                     int F, void* stream);
int acvae_bn_relu_pool_fwd(const float* Y, const float* bn, float* P, int N, int H, int W, int C, int pool, float p_drop,
                           uint64_t seed, int site, const uint8_t* keep_mask, void* stream);
int acvae_bn_relu_bwd(const float* Y, const float* dO, int upstream, const float* bn, float* dgamma, float* dbeta,
                      float* dY, void* ws, int64_t ws_bytes, int N, int H, int W, int C, int training, float p_drop,
                      uint64_t seed, int site, const uint8_t* keep_mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The recurrent cells one by one (gru_step, lstm_step, bigru_seq), torch.nn.GRU / LSTM
 * semantics and weight layout (gate order r|z|n and i|f|g|o):
 *   acvae_gru_step   one step of the decoder's GRU, models/decoder.py:39-44, 190: x [N,I], h [N,H] -> h_out [N,H]
 *   acvae_lstm_step  one step of the prior's LSTM, models/text_encoder.py:229-235, 254: (h, c) -> (h_out, c_out)
 *   acvae_bigru_seq  the posterior's packed bidirectional GRU, models/text_encoder.py:189-191: X [N,Tc,E] (batch-major),
 *                    lens [N] int64 (rows stop at their length; padded outputs are zero, pad_packed_sequence),
 *                    w = {w_ih, w_hh, b_ih, b_hh, then the same four of the reverse direction}, hidden [N,Tc,2H].
 * `ws`: scratch of acvae_rnn_workspace_bytes(N, Tc (1 for the single steps), I, H).
 * ------------------------------------------------------------------------------------------- */
int64_t acvae_rnn_workspace_bytes(int N, int Tc, int I, int H);
int acvae_gru_step(const float* x, const float* h, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, float* h_out, void* ws, int64_t ws_bytes, int N, int I, int H, void* stream);
int acvae_lstm_step(const float* x, const float* h, const float* c, const float* w_ih, const float* w_hh,
                    const float* b_ih, const float* b_hh, float* h_out, float* c_out, void* ws, int64_t ws_bytes, int N,
                    int I, int H, void* stream);
int acvae_bigru_seq(const float* X, const int64_t* lens, const void* const* w, float* hidden, void* ws, int64_t ws_bytes,
                    int N, int Tc, int E, int H, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Text side of the path.  `params` / `grads` are pointer tables in the reference's state-dict order
 * after the encoder (ACVAE_TEXT_NPARAMS entries; ln.* may be NULL when absent):
 *   decoder.{word_embeddings.weight, model.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0},
 *            classifier.{weight,bias}, attn.{v, h2attn.weight, h2attn.bias}},
 *   qnet.{word_embedding.weight, network.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0,
 *         *_reverse x4}, token_mean_log.{weight,bias}},
 *   pnet.{word_embedding.weight, word_attn.{v, h2attn.weight, h2attn.bias},
 *         network.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0}, mean_log_out.{weight,bias}},
 *   mean_log_out.{weight,bias}, ln.{weight,bias}.
 * All [N,Tc,*] tensors are batch-major and contiguous like the reference's outputs.
 * Gradients are WRITTEN (not accumulated).
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_TEXT_NPARAMS 35

/* A2  PosteriorRNN_hybrid.forward  models/text_encoder.py:182-216.  caps: int64 token ids [N, >=Tc]
 * (row stride ld_caps), lens1 = cap_lens-1 (device int64), Tc = max(lens1); eps_q [N,Tc,E] is the
 * torch.randn draw of :196 (made on the host, F9).  Packed-sequence semantics: a row stops at its
 * length, padded outputs are zero (so q_means/q_logs there equal the Linear bias). */
int64_t acvae_posterior_saved_bytes(int N, int Tc, int E, int Hq, int V);
int64_t acvae_posterior_scratch_bytes(int N, int Tc, int E, int Hq, int V);
int acvae_posterior_fwd(const void* const* params, const int64_t* caps, int64_t ld_caps, const int64_t* lens1,
                        const float* eps_q, float* q_means, float* q_logs, float* q_z, float* q_means_utt,
                        void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes, int N, int Tc, int E,
                        int Hq, int V, void* stream, int flags);
int acvae_posterior_bwd(const void* const* params, void* const* grads, const int64_t* lens1, const float* eps_q,
                        const float* q_logs, const float* d_q_means, const float* d_q_logs, const float* d_q_z,
                        const float* d_q_means_utt, void* saved, int64_t saved_bytes, void* scratch,
                        int64_t scratch_bytes, int N, int Tc, int E, int Hq, int V, void* stream, int flags);

/* A2 with stacked layers: PosteriorRNN_hybrid(num_layers = num_layers >= 1), i.e. nn.GRU(E, Hq, num_layers, bidirectional=True,
 * dropout=p).  Layer 0 is the one-layer posterior above (its eight tensors come from `params`); layer k >= 1 runs the same
 * packed BiGRU over the [N,Tc,2Hq] output [fw | bw] of layer k-1 instead of the embedded words, from a zero hidden state.
 * token_mean_log, the reparameterisation and q_means_utt (mean_with_lens + max_with_lens) read the TOP layer only.
 *   upper / upper_grads: 8 (num_layers - 1) entries; for k = 1 .. num_layers-1 torch's order
 *     network.{weight_ih_lk [3Hq][2Hq], weight_hh_lk [3Hq][Hq], bias_ih_lk, bias_hh_lk} then the same four of _lk_reverse
 *     (NULL tables when num_layers == 1).  Gradients are WRITTEN.
 *   keep: uint8 [num_layers-1][N][Tc][2Hq] (nonzero = kept), the inter-layer dropout of nn.GRU in training mode: the output of
 *     layer k < num_layers-1 is multiplied by keep[k] * keep_scale (keep_scale = 1/(1-p) as torch forms it in fp32) before
 *     layer k+1 reads it; the backward applies the same mask.  NULL = no dropout (eval mode, p = 0).  Entries at padded
 *     positions (t >= lens1[n]) are never read by a recurrence.  A mask needs num_layers > 1.
 * The same call with num_layers = 1 is acvae_posterior_fwd / _bwd (which are this code path, bit for bit).  num_layers is at
 * most 16.  The saved buffer of the forward holds every layer's outputs and cell saves; the backward reads it, and the
 * same upper table, keep mask and keep_scale must be passed to both. */
int64_t acvae_posterior_stack_saved_bytes(int N, int Tc, int E, int Hq, int V, int num_layers);
int64_t acvae_posterior_stack_scratch_bytes(int N, int Tc, int E, int Hq, int V, int num_layers);
int acvae_posterior_stack_fwd(const void* const* params, const void* const* upper, int num_layers, const uint8_t* keep,
                              float keep_scale, const int64_t* caps, int64_t ld_caps, const int64_t* lens1,
                              const float* eps_q, float* q_means, float* q_logs, float* q_z, float* q_means_utt,
                              void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes, int N, int Tc,
                              int E, int Hq, int V, void* stream, int flags);
int acvae_posterior_stack_bwd(const void* const* params, void* const* grads, const void* const* upper,
                              void* const* upper_grads, int num_layers, const uint8_t* keep, float keep_scale,
                              const int64_t* lens1, const float* eps_q, const float* q_logs, const float* d_q_means,
                              const float* d_q_logs, const float* d_q_z, const float* d_q_means_utt, void* saved,
                              int64_t saved_bytes, void* scratch, int64_t scratch_bytes, int N, int Tc, int E, int Hq,
                              int V, void* stream, int flags);

/* The teacher-forced decode loop (all words known, no step feeds the prior's z to the decoder: acvae_decode_fwd with every
 * ss flag set and every dis flag clear) runs as ONE persistent launch (csrc/decode_persist.hip) when N <= 32, S <= 512,
 * E is a power of two in 32..2048, H, A are multiples of 32 and the whole grid fits the device at once; its results are
 * bit-identical to the per-step path.  The posterior's packed BiGRU (acvae_posterior_fwd / _bwd) runs the same way - one
 * launch per pass for both directions - when N <= 32 and Hq is a multiple of 32 up to 512.  ACVAE_FLAG_NO_PERSIST forces the
 * per-step paths (A/B, parity tests).  Replaces nothing in the reference (scheduling only). */

/* A4+A5+A6+A7 (+A12 when caps == NULL): the step-by-step decode of Hybrid_VAEModel
 * models/vae_model.py:700-730,792-869 with PriorRNN (text_encoder.py:247-268),
 * VAERNNBahdanauAttnDecoder (decoder.py:175-203) and greedy sample_next_word (word_model.py:173-207).
 *   mem_in [N,S,Eenc] audio_embeds (projected by ln when Eenc != E), mem_lens [N] (= feat_lens//16),
 *   caps/ld_caps/lens1 as above (NULL caps = inference: words come from the previous argmax, z from
 *   the prior, finished rows emit <end>),  q_z [N,Tc,E] posterior samples,
 *   eps_p [Tc,N,E] the per-step torch.randn draws of text_encoder.py:259,
 *   ss_flags_host[t] != 0: step t is teacher-forced (random.random() < ss_ratio, vae_model.py:826),
 *   dis_flags_host[t] != 0: step t feeds the PRIOR's z to the decoder (torch.rand(1) <= dis_ratio, :805).
 * Outputs: logits [N,Tc,V], outputs [N,Tc,H], seqs i64 [N,Tc], sampled_logprobs [N,Tc],
 *   attn_w [N,Tc,S] (the reference's attn_weights transposed), p_means/p_logs/p_z [N,Tc,E],
 *   p_means_utt [N,2E] (training only), final states h [N,H], (hp, cp) [N,E].
 * aux_stream (may be NULL): a second HIP stream of the same device.  With teacher forcing the prior's recurrence
 *   (embedding -> attention -> LSTM -> z_t) and the decoder's (attention -> GRU) are two independent chains of ~10 us
 *   kernels unless a step feeds the prior's z to the decoder; given a second stream the call forks after the hoisted
 *   GEMMs, runs the prior chain there and joins before it returns, so on return all work is ordered on `stream`. */
int64_t acvae_decode_saved_bytes(int N, int Tc, int S, int E, int H, int A, int V, int Eenc);
int64_t acvae_decode_scratch_bytes(int N, int Tc, int S, int E, int H, int A, int V, int Eenc);
/* byte offset inside `saved` of the rows' log-sum-exp, f32 [N,Tc], written by every decode forward (-1: bad dims) */
int64_t acvae_decode_saved_lse_offset(int N, int Tc, int S, int E, int H, int A, int V, int Eenc);
int acvae_decode_fwd(const void* const* params, const float* mem_in, const int64_t* mem_lens, const int64_t* caps,
                     int64_t ld_caps, const int64_t* lens1, const float* q_z, const float* eps_p,
                     const int* ss_flags_host, const int* dis_flags_host, float* logits, float* outputs, int64_t* seqs,
                     float* sampled_logprobs, float* attn_w, float* p_means, float* p_logs, float* p_z,
                     float* p_means_utt, float* h_final, float* hp_final, float* cp_final, void* saved,
                     int64_t saved_bytes, void* scratch, int64_t scratch_bytes, int N, int Tc, int S, int E, int H,
                     int A, int V, int Eenc, int start_idx, int end_idx, void* stream, void* aux_stream, int flags);
/* The same with sample_next_word's method (models/word_model.py:173-207) chosen by the caller: ACVAE_SAMPLE_GREEDY
 * (= acvae_decode_fwd), or GUMBEL / MULTINOMIAL with `temp` and `sample_noise` [Tc,N,V] (see acvae_sample_next_word; the
 * per-step draws of the reference in step order).  seqs / sampled_logprobs then hold the sampled words; with
 * scheduled sampling or in inference the sampled word of step t-1 is the input of step t (vae_model.py:829-832).
 * emb_keep (may be NULL): keep mask uint8 [Tc,N,E] of the decoder's word-embedding nn.Dropout(emb_drop_p)
 * (models/decoder.py:33,184), drawn by the host on the CPU generator after each step's prior noise; kept rows are
 * scaled by 1/(1-p).  The same mask and p go to acvae_decode_bwd. */
int acvae_decode_fwd_sampled(const void* const* params, const float* mem_in, const int64_t* mem_lens,
                             const int64_t* caps, int64_t ld_caps, const int64_t* lens1, const float* q_z,
                             const float* eps_p, const int* ss_flags_host, const int* dis_flags_host, float* logits,
                             float* outputs, int64_t* seqs, float* sampled_logprobs, float* attn_w, float* p_means,
                             float* p_logs, float* p_z, float* p_means_utt, float* h_final, float* hp_final,
                             float* cp_final, void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes,
                             int N, int Tc, int S, int E, int H, int A, int V, int Eenc, int start_idx, int end_idx,
                             void* stream, void* aux_stream, int sample_method, float temp, const float* sample_noise,
                             const uint8_t* emb_keep, float emb_drop_p, int flags);
/* The same with every sampled step drawn by acvae_sample_next_word_truncated(top_k, top_p) (see there); `kept` (may be
 * NULL): int32 [N,Tc], the size of the kept prefix of every row and step.  acvae_decode_fwd_sampled is the
 * (0, 1.0f, NULL) case of this call: with both knobs off the untruncated kernel runs and `kept` is not written.
 * ACVAE_EINVAL, before anything is launched: top_k < 0; top_p outside (0, 1] or NaN; truncation (top_k > 0 or
 * top_p < 1) together with ACVAE_SAMPLE_GREEDY, or together with ACVAE_FLAG_ROLLOUT_GRAD - sampled_logprobs is the
 * log-probability under the full distribution, not the one sampled from, so it is not what a policy gradient needs. */
int acvae_decode_fwd_truncated(const void* const* params, const float* mem_in, const int64_t* mem_lens,
                               const int64_t* caps, int64_t ld_caps, const int64_t* lens1, const float* q_z,
                               const float* eps_p, const int* ss_flags_host, const int* dis_flags_host, float* logits,
                               float* outputs, int64_t* seqs, float* sampled_logprobs, float* attn_w, float* p_means,
                               float* p_logs, float* p_z, float* p_means_utt, float* h_final, float* hp_final,
                               float* cp_final, void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes,
                               int N, int Tc, int S, int E, int H, int A, int V, int Eenc, int start_idx, int end_idx,
                               void* stream, void* aux_stream, int sample_method, float temp, const float* sample_noise,
                               const uint8_t* emb_keep, float emb_drop_p, int flags, int top_k, float top_p,
                               int32_t* kept);
/* Backward for upstream gradients of logits / outputs / p_means / p_logs / p_z / p_means_utt (each may be
 * NULL).  Writes every decoder / pnet / mean_log_out / ln gradient, d_mem_in [N,S,Eenc] and d_q_z [N,Tc,E].
 * Stream contract: d_mem_in and d_q_z are ordered on `stream` when the call returns.  With ACVAE_FLAG_DEFER_PARAM_GRADS, when
 * acvae_decode_bwd_defers says 1 for the same flags / streams (a second stream is given and no step fed the prior's z to the
 * decoder), everything else - the parameter gradients - is queued on `aux_stream` behind
 * the call, so that it runs beside whatever `stream` does next (the posterior's and the encoder's backward; with the persistent
 * BPTT launch the seven weight gradients that need only its outputs go out earlier, as one grouped launch on `stream` while
 * it waits for `aux_stream`'s share of the memory gradient): the caller joins
 * aux_stream before those gradients are read on another stream, and keeps saved / scratch / outputs / mem_in / the upstream
 * gradients untouched until aux_stream has drained (mem_in: without an ln projection the products read it in place).  Without the flag (0) everything is ordered on `stream` on return.  Hybrid_VAEModel, which joins
 * the second stream at the end of the backward pass, passes it unless ACVAE_DECODE_DEFER=0 (-0.07 ms per step on the
 * reference configuration). */
/* Differentiable rollout.  acvae_decode_fwd_sampled with caps == NULL and ACVAE_FLAG_ROLLOUT_GRAD keeps in `saved` what the
 * backward reads, as the training form does (the transposed weights; the fed words and the finished-row state are kept by
 * every rollout).  acvae_decode_bwd with the same flag accepts that `saved`: lens1, dis_flags_host and d_q_z may be NULL,
 * d_p_means_utt must be NULL (a rollout has no utterance head; grads[mean_log_out.*] may be NULL and is left alone), every
 * step feeds the prior's z to the decoder (never deferred, never persistent), and the sampled words are constants.
 * Without the flag both calls behave as before: no transposes in a rollout, ACVAE_EINVAL for a backward without lens1. */
int acvae_decode_bwd_defers(const int* dis_flags_host, int Tc, void* stream, void* aux_stream, int flags);
int acvae_decode_bwd(const void* const* params, void* const* grads, const float* mem_in, const int64_t* mem_lens,
                     const int64_t* lens1, const float* eps_p, const int* dis_flags_host, const float* outputs,
                     const float* attn_w, const float* p_logs, const float* d_logits, const float* d_outputs_ext,
                     const float* d_p_means, const float* d_p_logs, const float* d_p_z, const float* d_p_means_utt,
                     float* d_mem_in, float* d_q_z, void* saved, int64_t saved_bytes, void* scratch,
                     int64_t scratch_bytes, int N, int Tc, int S, int E, int H, int A, int V, int Eenc, void* stream,
                     void* aux_stream, const uint8_t* emb_keep, float emb_drop_p, int flags);
/* float caption ids (collate pads with torch.zeros -> float32, caption_dataset.py:293) -> int64 */
int acvae_caps_to_long(const float* caps, int64_t* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A10  runners/pytorch_runner_vae.py:321-324: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step over
 * one flat fp32 buffer.  acvae_grad_norm writes ||grad_scale * g||_2 to a device scalar (grad_scale = 1/world
 * after a SUM all-reduce); acvae_adam_step applies coef = min(1, max_grad_norm / (norm + 1e-6)) (skipped when
 * total_norm is NULL or max_grad_norm <= 0) and the bias-corrected Adam update in one pass.
 * ------------------------------------------------------------------------------------------- */
int64_t acvae_grad_norm_partials(void);
int acvae_grad_norm(const float* grads, int64_t n, float grad_scale, float* partials, float* out_norm, void* stream);
int acvae_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                    float max_grad_norm, const float* total_norm, void* stream);
/* The other optimisers of conf["optimizer"] (runners/pytorch_runner_vae.py:219), same clip contract as
 * acvae_adam_step: coef = grad_scale * min(1, max_grad_norm / (*total_norm + 1e-6)), the clip skipped when total_norm
 * is NULL or max_grad_norm <= 0; no host synchronisation.  Elementwise in the operation order of torch.optim.<X>
 * (foreach=False).  Every pointer 16-B aligned (ACVAE_EALIGN otherwise); NULL / n <= 0 / step <= 0 -> ACVAE_EINVAL.
 * acvae_adamw_step: torch.optim.Adam (decoupled = 0: weight_decay * p folded into the gradient) or AdamW (decoupled = 1:
 *   p *= 1 - lr * weight_decay first); amsgrad = 1 keeps max_exp_avg_sq (may be NULL otherwise) and divides by its root.
 *   The hyperparameters are double (torch's are Python floats): 1 - beta, lr / bias correction, 1 - lr * weight_decay
 *   are formed in double on the host and rounded to float once, as torch's scalars reach its fp32 kernels.
 * acvae_sgd_step: torch.optim.SGD.  momentum_buffer may be NULL when momentum == 0; first = 1 on a parameter's first
 *   update sets the buffer to the (clipped, decayed) gradient itself, later ones apply buf = momentum*buf + (1-dampening)*g.
 *   nesterov needs momentum != 0 and dampening == 0 (ACVAE_EINVAL otherwise). */
int acvae_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                     int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                     int amsgrad, int64_t step, float grad_scale, float max_grad_norm, const float* total_norm,
                     void* stream);
int acvae_sgd_step(float* params, const float* grads, float* momentum_buffer, int64_t n, double lr, double momentum,
                   double dampening, double weight_decay, int nesterov, int first, float grad_scale, float max_grad_norm,
                   const float* total_norm, void* stream);
/* Gradient accumulation and the exponential moving average of the weights (TrainStep(accum_steps=, ema_decay=)): one
 * streaming pass each over flat fp32 buffers, grid-stride under ACVAE_FLAT_BLOCKS_CAP blocks of 256 threads with four
 * elements per thread and trip.  Every element is stored once; no atomics, no workspace, no host synchronisation.
 * Both: a NULL pointer, n <= 0, or [dst, dst + n) and [src, src + n) sharing a byte -> ACVAE_EINVAL; a base that is not
 * 16-B aligned -> ACVAE_EALIGN; both before any launch.
 * acvae_grad_accumulate: first != 0: acc[i] = grads[i], and acc is not read (whatever it held, NaN included, reaches
 *   nothing); first == 0: acc[i] = acc[i] + grads[i], one IEEE fp32 addition per element.  The norm of the accumulated
 *   gradient is acvae_grad_norm on acc, the mean over k micro-steps a grad_scale of 1 / k there and in the update.
 * acvae_ema_step: ema[i] = lerp(ema[i], params[i], w), w = (float)(1.0 - decay), by torch's rule (w < 0.5 ?
 *   ema + w * (params - ema) : params - (params - ema) * (1 - w)), the one torch.optim.swa_utils.get_ema_multi_avg_fn
 *   applies.  decay outside [0, 1] or NaN -> ACVAE_EINVAL.  ema == params gives ema back, decay == 1 leaves ema as it
 *   is, decay == 0 copies params. */
#define ACVAE_FLAT_BLOCKS_CAP 2048
int acvae_grad_accumulate(float* acc, const float* grads, int64_t n, int first, void* stream);
int acvae_ema_step(float* ema, const float* params, int64_t n, double decay, void* stream);
/* Parameter groups (TrainStep(param_groups=)): the norm and the update over the same flat buffers with up to
 * ACVAE_OPT_MAX_GROUPS sets of hyperparameters.  The host cuts every segment (a run of adjacent parameters of one group that
 * have a gradient and, for SGD, share the `first` flag) into chunks of at most acvae_opt_chunk_elems() elements; every
 * parameter's slice is padded to 4 elements, so chunks count float4s.  `chunks` is a DEVICE table int32 [n_chunks, 3]:
 *   [start / 4, length / 4, group | ACVAE_OPT_CHUNK_FIRST if this is the first SGD update of the chunk's parameters]
 * built once and reused; the hyperparameters are HOST arrays of n_groups doubles and travel by value in the kernel argument
 * (no host-to-device copy, no synchronisation).  A workgroup owns whole chunks (b, b + grid, ...), so its group is uniform.
 * A chunk with start < 0, length <= 0, group >= n_groups or unknown bits in its third word is skipped (the norm counts it as
 * zero); a length above the chunk size is cut to it and, in the steps, a range that leaves [0, n) is cut at n: a bad table
 * is never followed out of the buffers it was made for.  Elements no chunk covers are neither read nor written.
 * acvae_grad_norm_groups: partials[c] = the fp32 sum of squares of chunk c (one launch), then one finishing launch adds
 *   them in float64 in a fixed order that depends on n_chunks alone: each of 256 threads adds a contiguous run of chunks in
 *   ascending order into one sum per group, thread 0 adds the threads' sums in ascending order, then the groups in ascending
 *   order.  group_norms[k] = grad_scale * sqrt(sum of group k), total_norm[0] = grad_scale * sqrt(sum of all).  No atomics,
 *   every output stored once, nothing depends on what partials held: bit-reproducible.  A NaN / inf stays in its group
 *   and in the total.
 * acvae_adamw_groups_step / acvae_sgd_groups_step: acvae_adamw_step / acvae_sgd_step with per-group lr, betas, eps,
 *   weight_decay (SGD: lr, momentum, weight_decay); decoupled, amsgrad, nesterov and dampening are common to all groups.
 *   Every derived scalar is formed in double per group and rounded once, and the element arithmetic is the one-group
 *   entries' own, so a chunk comes out bit for bit as the one-group entry over its range would leave it.  SGD's momentum
 *   is zero in all groups (momentum_buffer may be NULL) or in none (ACVAE_EINVAL for a mix).
 * All three: a NULL pointer, n_groups outside 1..ACVAE_OPT_MAX_GROUPS, n_chunks <= 0 (steps: n <= 0, step <= 0) ->
 * ACVAE_EINVAL; a buffer or the table not 16-B aligned -> ACVAE_EALIGN; both before any launch. */
#define ACVAE_OPT_MAX_GROUPS 8
#define ACVAE_OPT_CHUNK_FIRST 256
int64_t acvae_opt_chunk_elems(void);
int acvae_grad_norm_groups(const float* grads, const int* chunks, int n_chunks, int n_groups, float grad_scale,
                           float* partials, float* group_norms, float* total_norm, void* stream);
int acvae_adamw_groups_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                            int64_t n, const int* chunks, int n_chunks, int n_groups, const double* lr,
                            const double* beta1, const double* beta2, const double* eps, const double* weight_decay,
                            int decoupled, int amsgrad, int64_t step, float grad_scale, float max_grad_norm,
                            const float* total_norm, void* stream);
int acvae_sgd_groups_step(float* params, const float* grads, float* momentum_buffer, int64_t n, const int* chunks,
                          int n_chunks, int n_groups, const double* lr, const double* momentum,
                          const double* weight_decay, double dampening, int nesterov, float grad_scale,
                          float max_grad_norm, const float* total_norm, void* stream);
/* The non-finite guard (TrainStep(nonfinite="skip")): whether an update is applied is decided on the device, from the norm
 * that lives there, and everything that moves the training state reads that decision.  A skipped update leaves every
 * buffer bit for bit as it was.  The RECORD is caller-owned device memory of ACVAE_GUARD_RECORD_BYTES bytes, 16-B aligned,
 * zeroed by the caller before the first use; only the entries below write it.  Layout (byte offset, type):
 *     0  int64  applied        updates applied so far: the `step` of Adam's bias correction
 *     8  int64  skipped        updates skipped so far
 *    16  int64  streak         consecutive skips up to and including the last decision (0 after an applied update)
 *    24  int64  ema_updates    updates the weight average has seen (ema_warmup's t)
 *    32  int32  ok             the last decision: 1 apply, 0 skip
 *    36  int32  window_bad     OR of the witnesses since the last decision
 *    40  float  step_size[8]   per group, (float)(lr / (1 - beta1^applied)), formed in double at the last applied decision
 *    72  float  bc2_sqrt[8]    per group, (float)sqrt(1 - beta2^applied)
 *   104  float  ema_w          (float)(1 - decay) of the last applied decision
 *   108  int32  reserved
 * acvae_guard_witness: one workgroup; window_bad |= (*loss is NaN / +-inf) | (any of buf[0 .. n_buf) is NaN / +-inf).
 *   loss (a device fp32 scalar) may be NULL (not looked at); buf == NULL with n_buf == 0 is legal (n_buf < 0, or a NULL
 *   buf with n_buf > 0 -> ACVAE_EINVAL); buf 16-B aligned.  Finite values, +-0, denormals and +-FLT_MAX set nothing.
 * acvae_guard_decide: one wavefront.  ok = isfinite(total_norm[0]) && !window_bad; ok: applied += 1, streak = 0; else
 *   skipped += 1, streak += 1; window_bad = 0 either way.  When ok and kind == 0 (Adam / AdamW), for every group k
 *   step_size[k] = (float)(lr[k] / (1 - pow(beta1[k], t))) and bc2_sqrt[k] = (float)sqrt(1 - pow(beta2[k], t)) with
 *   t = applied after the increment, in double, rounded once: the scalars acvae_adamw_groups_step forms on the host for
 *   step = t.  kind == 1 (SGD) forms none (beta1 / beta2 may be NULL).  When ok and 0 <= ema_decay <= 1:
 *   ema_w = (float)(1 - d), d = ema_warmup ? min(ema_decay, (1 + u) / (10 + u)) : ema_decay with u = ema_updates, in
 *   double, then ema_updates += 1; ema_decay < 0 means "no average" and leaves both alone.  lr / beta1 / beta2 are HOST
 *   arrays of n_groups doubles and travel by value in the kernel argument.  kind outside {0, 1}, n_groups outside
 *   1..ACVAE_OPT_MAX_GROUPS, ema_decay > 1 or NaN, a NULL record / total_norm / lr (kind 0: beta1 / beta2) -> ACVAE_EINVAL.
 * acvae_adamw_groups_step_guarded / acvae_sgd_groups_step_guarded: the grouped steps without `step`: every workgroup
 *   reads ok once and returns before touching anything when it is 0; otherwise a chunk takes step_size / bc2_sqrt of its
 *   group from the record (Adam) and runs the unguarded kernel's arithmetic: with ok == 1 every buffer comes out bit for
 *   bit as acvae_adamw_groups_step(step = applied) / acvae_sgd_groups_step leaves it.  SGD: momentum must be 0 in every
 *   group (the first-update flag of the momentum buffer is the host's and cannot follow a device decision; ACVAE_EINVAL).
 * acvae_ema_step_guarded: acvae_ema_step with w = ema_w of the record; nothing is touched when ok == 0.
 * acvae_guard_restore: ok == 0: dst[0 .. n) = snapshot[0 .. n); ok == 1: neither is read or written.
 * Both: NULL, n <= 0 or overlapping ranges -> ACVAE_EINVAL.  All six: a buffer or the record not 16-B aligned -> ACVAE_EALIGN;
 * every refusal before any launch; no host synchronisation, no atomics, every word stored by one thread. */
#define ACVAE_GUARD_RECORD_BYTES 112
typedef struct acvae_guard_record {
  int64_t applied, skipped, streak, ema_updates;
  int32_t ok, window_bad;
  float step_size[8], bc2_sqrt[8];
  float ema_w;
  int32_t reserved;
} acvae_guard_record;
int acvae_guard_witness(const float* loss, const float* buf, int64_t n_buf, acvae_guard_record* record, void* stream);
int acvae_guard_decide(acvae_guard_record* record, const float* total_norm, int kind, int n_groups, const double* lr,
                       const double* beta1, const double* beta2, double ema_decay, int ema_warmup, void* stream);
int acvae_adamw_groups_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                    float* max_exp_avg_sq, int64_t n, const int* chunks, int n_chunks, int n_groups,
                                    const double* lr, const double* beta1, const double* beta2, const double* eps,
                                    const double* weight_decay, int decoupled, int amsgrad, float grad_scale,
                                    float max_grad_norm, const float* total_norm, const acvae_guard_record* record,
                                    void* stream);
int acvae_sgd_groups_step_guarded(float* params, const float* grads, int64_t n, const int* chunks, int n_chunks,
                                  int n_groups, const double* lr, const double* weight_decay, float grad_scale,
                                  float max_grad_norm, const float* total_norm, const acvae_guard_record* record,
                                  void* stream);
int acvae_ema_step_guarded(float* ema, const float* params, int64_t n, const acvae_guard_record* record, void* stream);
int acvae_guard_restore(float* dst, const float* snapshot, int64_t n, const acvae_guard_record* record, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-time augmentation, datasets/augment.py:time_roll + spec_augment's time_mask / freq_mask (:30-65), on the
 * uploaded batch in [N, T, F] (F % 4 == 0, `in` / `out` 16-B aligned or ACVAE_EALIGN, `out` never aliases `in`).
 * The random draws are the host's (acvae_amd/augment.py); `params` is an int32 table [N, K], K = ACVAE_AUG_TABLE_WIDTH,
 * one row per clip:
 *   [shift, n_time, n_freq, time masks (start, end) x ACVAE_AUG_MAX_MASKS, freq masks (start, end) x ACVAE_AUG_MAX_MASKS]
 * Per clip n of length L = lens[n] (clamped to [0, T]): output row i < L = input row (i - shift) mod L (np.roll); then
 * each mask in table order (the time masks [start, end) x all F, then the freq masks all L x [start, end)) overwrites its
 * region with the mean over all L * F cells of the clip as it stands just before that mask (fixed-order fp64 sums, the
 * mean rounded to fp32: bit-reproducible).  Rows >= L are copied unchanged.  Every index is clamped to the clip, so a bad
 * table cannot reach outside it.  One workgroup per clip, no workspace.  N <= 0, T <= 0, F % 4 != 0, F > ACVAE_AUG_MAX_F,
 * T * F > INT32_MAX, a NULL pointer or K != ACVAE_AUG_TABLE_WIDTH -> ACVAE_EINVAL before any HIP call.
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_AUG_MAX_MASKS 8
#define ACVAE_AUG_TABLE_WIDTH 35        /* 3 + 2 * 2 * ACVAE_AUG_MAX_MASKS */
#define ACVAE_AUG_MAX_F 1024            /* mel bins per frame */
int acvae_spec_augment(const float* in, float* out, const int* lens, const int* params, int N, int T, int F, int K,
                       void* stream);

/* The same with datasets/augment.py:random_crop in front, for clips that exist only on the device (features formed there
 * from waveforms): `in` [N, T, F] holds the uncropped clips of src_lens[n] rows, `out` [N, To, F] (To <= T, never
 * aliasing `in`) the cropped, rolled and masked ones.  `table` is int32 [N, K], K = ACVAE_AUG_WINDOW_TABLE_WIDTH, one
 * row per clip:
 *   [the ACVAE_AUG_TABLE_WIDTH columns above, out_len, n_windows, (start, shift, length) x ACVAE_AUG_MAX_WINDOWS]
 * The windows are the crops that fired, in the order they were applied: `length` is the clip's length in front of the
 * crop, `shift` the roll pending in front of it, and the crop keeps rows [start, start + size) of the rolled clip
 * (circularly), `size` being the next window's `length`, or out_len behind the last one.  Row i < out_len of the clip the
 * first ACVAE_AUG_TABLE_WIDTH columns apply to is input row j, from j = i and, for the windows from last to first,
 * j = (start + j - shift) mod length; the roll and the masks then act on that clip of L = out_len rows exactly as above:
 * the same arithmetic in the same order, so the result equals acvae_spec_augment on the host-cropped clip bit for bit.
 * Rows >= out_len of `out` are written as zeros, which is what collate_fn pads with.  Each window's length is clamped
 * into [1, the size in front of it], start into the window's clip, out_len into [0, min(last size, To)]: a bad table
 * cannot reach outside the clip.  One workgroup per clip, no workspace.  N <= 0, T <= 0, To <= 0, To > T, F % 4 != 0,
 * F > ACVAE_AUG_MAX_F, T * F > INT32_MAX, a NULL pointer or K != ACVAE_AUG_WINDOW_TABLE_WIDTH -> ACVAE_EINVAL before any
 * HIP call; `in` / `out` not 16-B aligned -> ACVAE_EALIGN. */
#define ACVAE_AUG_MAX_WINDOWS 4
#define ACVAE_AUG_WINDOW_TABLE_WIDTH 49 /* ACVAE_AUG_TABLE_WIDTH + 2 + 3 * ACVAE_AUG_MAX_WINDOWS */
int acvae_augment_window(const float* in, float* out, const int* src_lens, const int* table, int N, int T, int To, int F,
                         int K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Log-mel front end: waveforms -> the [T, n_mels] features every encoder of the package starts from (the PANNs front end,
 * models/encoder.py:877-885: torchlibrosa's Spectrogram then LogmelFilterBank), one fused kernel, no workspace.
 * For clip n of L = wave_lens[n] samples, with n = n_fft, h = hop, nb = n/2 + 1:
 *   padding  reflect, n/2 samples on both sides of the clip's OWN length: index i < 0 -> -i, i >= L -> 2(L-1) - i;
 *   frames   Tn = 1 + L / h frames, frame t = padded samples t*h .. t*h + n - 1;
 *   power    P[t, f] = (sum_k x_t[k] w[k] cos(2 pi k f / n))^2 + (sum_k x_t[k] w[k] sin(2 pi k f / n))^2, f = 0 .. n/2,
 *            w the periodic Hann window;
 *   output   out[t, m] = 10 log10(max(sum_f P[t, f] W[f, m], amin)) - db_offset, db_offset = 10 log10(max(amin, ref)).
 * Rows t >= Tn of `out` (and of `spec`) are written as zeros, which is what collate_fn pads features with; nothing is
 * written outside [N, T, .].
 *
 * Operands (the caller owns them all; the tables are built in float64 on the host and rounded once to fp32,
 * acvae_amd/frontend.py):
 *   wave      [N, wave_stride] samples, fp32, or int16 PCM when wave_is_i16 (scaled by 1/32768 on load, exact in fp32);
 *   wave_lens int32 [N] on the device.  The kernel cannot refuse a bad length, so it clamps: a length above wave_stride
 *             counts as wave_stride, a clip shorter than n/2 + 1 has no frames (all its rows are zeros).  The caller checks
 *             wave_lens[n] >= n/2 + 1 on the host;
 *   basis     the windowed DFT matrix, n_fft * n_fft floats, 16-B aligned, in the order the kernel stages it:
 *             [n_fft/128 frequency chunks][n_fft/32 K-steps][128 columns][32 k].  Column c < 64 of chunk q is the real part of
 *             bin f = 64 q + c: w[k] cos(2 pi k f / n); column 64 + c its imaginary part -w[k] sin(2 pi k f / n) - except
 *             column 64 of chunk 0 (the imaginary part of bin 0, identically zero), which holds the real part of the Nyquist
 *             bin n/2, w[k] cos(pi k) (whose imaginary part is zero as well): n/2 + 1 bins in exactly n columns;
 *   melw      [nb, n_mels] mel weights, row-major.  Row n/2 (the Nyquist bin) is added on the vector unit in the epilogue,
 *             after the matrix-pipe sum over the other bins; LogMel's own weights there are zero (fmax <= sr/2);
 *   out       f32 [N, T, n_mels];  spec: f32 [N, T, nb] power spectrogram, or NULL (then it never leaves the registers).
 * A workgroup owns ACVAE_LOGMEL_FRAME_TILE consecutive frames of one clip.  Per frequency chunk it runs the DFT as a GEMM
 * on v_mfma_f32_32x32x2_f32 (exact fp32): the frame matrix is never materialised - every K-step's [frames x 32] piece is
 * gathered from the waveform into LDS with the reflect rule applied - squares and adds re / im in registers, multiplies the
 * power tile by `melw` on the matrix pipe through LDS and keeps the mel sums in registers until the single store of `out`.
 * The summation order is fixed and there are no atomics: bit-reproducible, and `spec` = NULL gives the same `out`.
 * Limits (ACVAE_EINVAL before any HIP call): n_fft in {256, 512, 1024, 2048}; 1 <= hop <= n_fft; n_mels a multiple of 4 in
 * [4, 128]; N, T >= 1; T = 1 + max_len / hop for the longest clip, of which (T - 1) * hop <= wave_stride is checked;
 * n_fft/2 + 1 <= wave_stride <= 2^30; N * T * nb < 2^31; amin > 0; wave_is_i16 0 or 1; a NULL pointer other than
 * `spec`.  `basis` not 16-B aligned -> ACVAE_EALIGN.
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_LOGMEL_FRAME_TILE 64
int acvae_logmel_fwd(const void* wave, int wave_is_i16, int64_t wave_stride, const int* wave_lens, const float* basis,
                     const float* melw, float* out, float* spec, int N, int T, int n_fft, int hop, int n_mels, float amin,
                     float db_offset, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sample-rate conversion in front of the log-mel front end: band-limited interpolation with a Kaiser-windowed sinc
 * (the closed form behind librosa / resampy's "kaiser_best" and "kaiser_fast" settings; their interpolated tables and
 * soxr are NOT reproduced bit for bit), one kernel, no workspace.  Rates orig -> new, g = gcd, U = new / g, D = orig / g,
 * c = rolloff * min(1, U / D), Z zero crossings:
 *   kernel   g(tau) = c sinc(c tau) I0(beta sqrt(1 - (c tau / Z)^2)) / I0(beta) for |c tau| < Z, else 0 (tau in input samples);
 *   output   y[m] = sum_n x[n] g(m D / U - n), x zero outside [0, L);  L_out = ceil(L U / D) outputs for a clip of L samples.
 * Columns L_out .. out_stride - 1 of a clip's row of `out` are written as zeros; nothing is written outside
 * [N, out_stride].
 *
 * The kernel runs it as the product Y[j, i] = sum_k X[j, k] H[k, i] with m = j U + i (block j, phase i < U),
 * X[j, k] = x[j D + k - W] and H[k, i] = g(i D / U - (k - W)), W = ceil(Z / c) + 1, on v_mfma_f32_32x32x2_f32 (exact fp32);
 * X is never materialised - every K-step's [blocks x 32] piece is gathered from the waveform into LDS with the zero rule
 * applied.  U and D need not be coprime: for a small U the host groups s blocks into one (U' = s U >= 32, D' = s D) and
 * hands in U', D'; the kernel knows nothing of s.
 *
 * Operands (the caller owns them all; the tables are built in float64 on the host and rounded once to fp32,
 * acvae_amd/frontend.py):
 *   wave       [N, wave_stride] samples, fp32, or int16 PCM when wave_is_i16 (scaled by 1/32768 on load, exact in fp32);
 *   wave_lens  int32 [N] on the device.  The kernel cannot refuse a bad length, so it clamps it to [0, wave_stride];
 *   bank       the filter table compacted per tile of 32 phases, 16-B aligned:
 *              [ceil(U / 32) phase tiles][ksteps K-steps][32 phases][32 k] floats.  Entry (t, s, p, q) is
 *              H[first_k(t) + 32 s + q, 32 t + p]; phases >= U, K-steps behind the tile's own and rows outside H are zeros;
 *   bank_index int32 [ceil(U / 32), 2] on the device: per phase tile its first k and its number of K-steps (clamped to
 *              [0, ksteps] by the kernel).  A tile's taps are non-zero only over a band of about 2 Z / c + 31 D / U values
 *              of k, and the kernel visits only the K-steps of that band;
 *   out        f32 [N, out_stride], out_stride >= the longest L_out the caller wants to keep (outputs behind out_stride
 *              are dropped).
 * A workgroup owns ACVAE_RESAMPLE_BLOCK_TILE consecutive blocks of one clip times one phase tile.  The summation order is
 * fixed, there are no atomics and every output is stored once: bit-reproducible.
 * Limits (ACVAE_EINVAL before any HIP call): U, D in [1, ACVAE_RESAMPLE_MAX_RATIO] and U != D; W >= 1 and the taps per
 * output 2 W <= ACVAE_RESAMPLE_MAX_TAPS; ksteps in [1, ACVAE_RESAMPLE_MAX_KSTEPS]; N >= 1; 1 <= wave_stride <= 2^30;
 * out_stride >= 1 and N * out_stride < 2^31; wave_is_i16 0 or 1; a NULL pointer.  `bank` not 16-B aligned -> ACVAE_EALIGN.
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_RESAMPLE_BLOCK_TILE 64
#define ACVAE_RESAMPLE_MAX_RATIO 1024
#define ACVAE_RESAMPLE_MAX_TAPS 2048
#define ACVAE_RESAMPLE_MAX_KSTEPS 98    /* (MAX_TAPS + MAX_RATIO) / 32 + 2: the widest band of a phase tile */
int acvae_resample_fwd(const void* wave, int wave_is_i16, int64_t wave_stride, const int* wave_lens, const float* bank,
                       const int* bank_index, float* out, int64_t out_stride, int N, int U, int D, int W, int ksteps,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rows of a [*, R] matrix gathered by an index, and the adjoint: rows folded into the row they came from.  The training
 * step with several captions per clip (Hybrid_VAEModel.forward(..., clip_index=)) runs the encoder once over the B clips
 * and gathers its memory [B, R = S * C] into the N caption rows; the backward folds the N rows' gradients into the B clips'.
 *   acvae_rows_gather: dst[r, :] = src[index[r], :] for r < N.  src [B, R], index int64 [N] (device memory), dst [N, R].
 *                      A row whose index lies outside [0, B) is written as zeros (nothing outside src is read).
 *   acvae_rows_fold:   dst[c, :] = 0 + src[rows[offsets[c]], :] + src[rows[offsets[c] + 1], :] + ... for c < B, plain fp32
 *                      additions in exactly that order.  src [N, R], dst [B, R]; offsets int32 [B + 1] / rows int32 [N] are the
 *                      CSR lists of each clip's rows, built by the caller on the host (ascending within a clip for the
 *                      adjoint of the gather).  A clip without rows gets zeros.  No atomics and one owner per output
 *                      element: bit-reproducible.  A row number outside [0, N) contributes zero.
 * Memory-bound: one thread per 16-byte chunk of a row / clip, no workspace, no state.  NULL pointers, B < 1, N < 1, R < 4 or
 * R % 4 != 0 -> ACVAE_EINVAL; src / dst not 16-byte aligned -> ACVAE_EALIGN; both before any HIP call.
 * ------------------------------------------------------------------------------------------- */
int acvae_rows_gather(const float* src, const int64_t* index, float* dst, int B, int N, int64_t R, void* stream);
int acvae_rows_fold(const float* src, const int* offsets, const int* rows, float* dst, int B, int N, int64_t R,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Opt-in kernel timing (bench.py's live roofline figure): while enabled, the conv launches are bracketed
 * by HIP events on their stream; acvae_prof_read waits for them and returns the summed duration and the
 * launch count of a tag, then clears it.  Tags: 0 = conv3x3 implicit GEMM (forward + data gradient),
 * 1 = conv3x3 weight gradient.  This ring is the only mutable state in the library and exists only
 * while enabled.  total_ms_host / launches_host are HOST pointers.
 * ------------------------------------------------------------------------------------------- */
int acvae_prof_enable(int enable);
int acvae_prof_pause(int paused);   /* stop / resume marking, keeping what was recorded (sampled measurement) */
int acvae_prof_read(int tag, double* total_ms_host, int64_t* launches_host);

/* ---------------------------------------------------------------------------------------------
 * Single decode steps (inference, no gradients): the per-call API of the reference's sub-modules,
 *   PriorRNN.forward(word, enc_mem, hiddens_state, last_z, lens)            models/text_encoder.py:247-268
 *   VAERNNBahdanauAttnDecoder.forward(word=, state=, enc_mem=, enc_mem_lens=, z=)   models/decoder.py:175-203
 * as used by the validation beam search (models/vae_model.py:896-995).  encproj_* may be NULL
 * (computed into scratch) or the result of acvae_attn_precompute (hoisted out of the step loop).  word int64 [N].
 * acvae_logprob_add / acvae_topk_flat are the beam bookkeeping of vae_model.py:909-916 (log_softmax + running beam
 * score; flat top-k over beam*V with idx / V and idx % V).
 * The widths are free of each other: E (embeddings, memory, the prior's LSTM), H (the decoder GRU), A (its attention); the
 * searches below take them per member likewise.  acvae_step_scratch_bytes sizes ONE buffer for both step entries.
 * ------------------------------------------------------------------------------------------- */
int64_t acvae_step_scratch_bytes(int N, int S, int E, int H, int A, int V);
int acvae_attn_precompute(const void* const* params, int which, const float* mem, float* encproj, int N, int S, int E,
                          int H, int A, void* stream);
int acvae_prior_step_fwd(const void* const* params, const int64_t* word, const float* mem, const int64_t* mem_lens,
                         const float* encproj_p, const float* h_prev, const float* c_prev, const float* last_z,
                         const float* eps, float* mean, float* logv, float* z, float* h_out, float* c_out, float* attw,
                         void* scratch, int64_t scratch_bytes, int N, int S, int E, int V, void* stream);
int acvae_decoder_step_fwd(const void* const* params, const int64_t* word, const float* h_prev, const float* mem,
                           const int64_t* mem_lens, const float* encproj_d, const float* z, float* logits, float* h_out,
                           float* attw, float* rnn_input, void* scratch, int64_t scratch_bytes, int N, int S, int E,
                           int H, int A, int V, void* stream);
int acvae_logprob_add(const float* logits, int64_t ld, const float* lse, const float* prev, float* out, int N, int V,
                      void* stream);
int acvae_topk_flat(const float* x, int64_t n, int k, int V, float* vals, int64_t* idx, int64_t* row, int64_t* col,
                    void* stream);
/* All clips of a batch at once: group g searches x[g * group_stride .. + n) (n = beam*V scores of one clip, or V: only
 * its first beam row), outputs [groups][k]; `row` comes back as group * row_base + idx / V, i.e. as an index into the
 * batch's beam rows when row_base = beam. */
int acvae_topk_flat_batched(const float* x, int64_t n, int64_t group_stride, int k, int V, float* vals, int64_t* idx,
                            int64_t* row, int64_t* col, int groups, int row_base, void* stream);
/* Validation beam search as one call: Hybrid_VAEModel.beam_search, models/vae_model.py:896-995, for
 * all N clips at once.  mem [N,S,E] (after the optional `ln` projection), mem_lens [N], eps [max_length][N*beam][E]
 * (the N(0,1) draws of PriorRNN.forward, text_encoder.py:259, step-major), start_idx = vocabulary index of <start>.
 * Outputs, as the reference keeps them (beam 0 of each clip, :990-995): seqs int64 [N,max_length],
 * attn_weights [N,S,max_length].  No host synchronisation; scratch of acvae_beam_search_scratch_bytes().
 * This is the M = 1 beam case of acvae_ensemble_search (below: one driver, one acvae_ensemble_mix launch per step forms the
 * scores) plus beam 0's attention-weight history.  Refused before any launch: a dimension <= 0 (ACVAE_EINVAL);
 * N * beam > 2^20 (ACVAE_EUNSUPPORTED, -1 from the bytes function); a NULL pointer, start_idx outside [0, V), or
 * beam > 16 (acvae_topk_flat_batched's limit) (ACVAE_EINVAL); scratch below the bytes function (ACVAE_EWORKSPACE). */
int64_t acvae_beam_search_scratch_bytes(int N, int beam, int max_length, int S, int E, int H, int A, int V);
int acvae_beam_search(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                      int64_t start_idx, int64_t* seqs, float* attn_weights, void* scratch, int64_t scratch_bytes, int N,
                      int beam, int max_length, int S, int E, int H, int A, int V, void* stream);
/* Diverse beam search, models/word_model.py:344-348 with add_diversity :298-312: per beam row
 *   out[n,c] = log_softmax(log_softmax(logits[n]) / temperature)[c] - diversity_lambda * counts[c] + prev[n]
 * counts (may be NULL: first group) = how often the earlier groups chose word c at this local step: one vector [V] for
 * all rows (rows_per_count = 0) or one per clip, [N / rows_per_count][V]; prev [N] (may be NULL) the running beam
 * log-probabilities. */
int acvae_dbs_scores(const float* logits, int64_t ld, float temperature, const float* counts, float diversity_lambda,
                     const float* prev, float* out, int N, int V, int rows_per_count, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble decoding: BaseRunner.ensemble / _ensemble_batch / _ensemble_batch_beam_search,
 * runners/base_runner.py:397-694, with several trained models at once: at every step the members' word probabilities
 * are averaged and the word is picked from the average (:616-618 greedy, :675-686 beam).
 *
 * acvae_ensemble_mix, one launch per step (in the place of M x (acvae_row_logsoftmax_argmax + acvae_logprob_add) and a
 * mixing pass):
 *   out[r,c] = log( (1/M) * sum_m softmax(logits_m[r])[c] ) + prev[r]
 * logits / ld: HOST arrays of M device pointers and leading dimensions (member m's row r at logits[m] + r * ld[m],
 * ld[m] >= V), 1 <= M <= ACVAE_ENSEMBLE_MAX; prev [R] may be NULL (0).  out (row stride ld_out >= V) may be NULL when only
 * the selection is wanted; argmax / best (either may be NULL; element r at r * o_stride): the first maximum column of
 * out[r] and its value, what the greedy search picks (:618).  Arithmetic: lse_m as acvae_row_logsoftmax_argmax forms it,
 * lp_m = logits_m - lse_m, a = max_m lp_m, s = sum_m expf(lp_m - a) in member order, out = (a + logf(s / M)) + prev; hence
 * M = 1 is bit-equal to acvae_row_logsoftmax_argmax + acvae_logprob_add, and M copies of one matrix are bit-equal to M = 1.
 *
 * acvae_ensemble_search, the whole search as one call, on Hybrid_VAEModel's step (prior step -> z -> decoder step,
 * models/vae_model.py:896-995; the reference's ensemble code never runs the prior).  HOST arrays of M entries describe
 * the members: params[m] the member's text parameter table (ACVAE_TEXT_NPARAMS pointers), mem[m] [N,S[m],E[m]] (after the
 * member's `ln`), mem_lens[m] int64 [N], eps[m] [max_length][N*beam][E[m]] (step-major, as acvae_beam_search), and the
 * dimensions S / E / H / A.  V, start_idx and end_idx are shared; all members are fed the same word.
 *   greedy != 0 (beam must be 1): the mixture's argmax; a row that has produced end_idx keeps emitting and feeding it, all
 *     max_length steps run (no host read-back): seqs as :584, 622-630 leave it.  logprobs f32 [N,max_length]: the
 *     mixture's log-probability of the step's argmax.
 *   greedy == 0: beam search, flat top-k over beam * V per clip at every step, t = 0 included (as acvae_beam_search: the
 *     rows of a clip differ in z), beam 0 traced back.  logprobs f32 [N]: beam 0's final score.  With M = 1 this is
 *     acvae_beam_search (the same driver) without the attention-weight history: the same seqs bit for bit.
 * seqs int64 [N,max_length].  Refused before any launch: M outside [1, ACVAE_ENSEMBLE_MAX], a NULL entry,
 * beam > 64, greedy with beam != 1, start_idx / end_idx outside [0, V) (ACVAE_EINVAL); N * beam > 2^20, or beam > 16
 * without greedy (acvae_topk_flat_batched's limit) (ACVAE_EUNSUPPORTED); scratch below
 * acvae_ensemble_search_scratch_bytes() (ACVAE_EWORKSPACE).  One stream, no host synchronisation.
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_ENSEMBLE_MAX 8
int acvae_ensemble_mix(const float* const* logits, const int64_t* ld, int M, const float* prev, float* out, int64_t ld_out,
                       int64_t* argmax, float* best, int64_t o_stride, int R, int V, void* stream);
int64_t acvae_ensemble_search_scratch_bytes(int M, int N, int beam, int max_length, const int* S, const int* E,
                                            const int* H, const int* A, int V);
int acvae_ensemble_search(const void* const* const* params, const float* const* mem, const int64_t* const* mem_lens,
                          const float* const* eps, const int* S, const int* E, const int* H, const int* A, int M,
                          int64_t start_idx, int64_t end_idx, int greedy, int64_t* seqs, float* logprobs, void* scratch,
                          int64_t scratch_bytes, int N, int beam, int max_length, int V, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble rollouts: sample_n sampled (or greedy) captions per clip from the mixture.  No counterpart in the reference.
 *
 * acvae_ensemble_mix_sample, one launch per sampled step: the mixture's log-probabilities v[r,c] exactly as
 * acvae_ensemble_mix forms them with prev = NULL, scored by acvae_sample_next_word's rule on the caller's noise row
 * (noise + r * ld_noise, ld_noise >= V):
 *   ACVAE_SAMPLE_GUMBEL       w = argmax_c (v_c + g_c) / temp
 *   ACVAE_SAMPLE_MULTINOMIAL  w = argmax_c expf(v_c / temp) / q_c
 * first maximum wins; a row whose scores are all NaN gets a word in [0, V).  `temp` acts on the MIXTURE: the members are
 * mixed at temperature 1 and v is divided by temp, not the members' logits before the mixing.  Then the greedy search's
 * bookkeeping of step t: a row with t > 0 and seqs[r * ld_seqs + t - 1] == end_idx gets end_idx; seqs[r * ld_seqs + t]
 * and word[r] (the word fed to the next step) receive the word, logprobs[r * ld_logprobs + t] = v[r, w] of the CHOSEN
 * word w (untempered; also for a row that is held at end_idx).  out (row stride ld_out >= V) may be NULL: the mixed row
 * then never reaches memory.  ACVAE_EINVAL before any launch: what acvae_ensemble_mix refuses of logits / ld / M / R / V,
 * a method other than the two, temp not finite or <= 0, noise / seqs / logprobs / word NULL, t < 0, ld_seqs or
 * ld_logprobs <= t, ld_noise < V, out with ld_out < V.  No workspace, no atomics.
 *
 * acvae_ensemble_rollout, the whole rollout as one call: acvae_ensemble_search's driver with the pick chosen by `method`.
 * Rows R = N * sample_n, row n * sample_n + j is rollout j of clip n; the rows of a clip share its memory.  Members as for
 * acvae_ensemble_search, with eps[m] [max_length][R][E[m]].  Every step: the members' steps on the shared word, the
 * constraints (off: 1.0f, 0, 0, NULL, 0) on every member's logits with the seqs row as the history, then
 *   ACVAE_SAMPLE_GREEDY       acvae_ensemble_mix's argmax and the bookkeeping launch (sample_n = 1: acvae_ensemble_search's
 *                             greedy call bit for bit); noise may be NULL, top_k must be 0 and top_p 1;
 *   GUMBEL / MULTINOMIAL      top_k == 0 and top_p == 1: one acvae_ensemble_mix_sample launch on noise[t] (noise
 *                             [max_length][R][V], as acvae_sample_noise draws it); otherwise acvae_ensemble_mix writes
 *                             the mixed row, acvae_sample_next_word_truncated(top_k, top_p) draws from it (the row is a
 *                             normalised log-probability row already) and the bookkeeping launch follows.
 * A row that has produced end_idx keeps emitting and feeding it; all max_length steps run, nothing is read back.
 * seqs int64 [R,max_length], logprobs f32 [R,max_length]: the mixture's log-probability of each chosen word.
 * Refused before any launch: M outside [1, ACVAE_ENSEMBLE_MAX], a NULL entry, sample_n < 1, a method outside the three,
 * temp not finite or <= 0, a sampling method with noise NULL, top_k < 0, top_p outside (0, 1], truncation with
 * ACVAE_SAMPLE_GREEDY, start_idx / end_idx outside [0, V), what the constrained entries refuse (ACVAE_EINVAL);
 * N * sample_n > 2^20 (ACVAE_EUNSUPPORTED); scratch below acvae_ensemble_rollout_scratch_bytes() (ACVAE_EWORKSPACE).
 * ------------------------------------------------------------------------------------------- */
int acvae_ensemble_mix_sample(const float* const* logits, const int64_t* ld, int M, const float* noise, int64_t ld_noise,
                              int method, float temp, float* out, int64_t ld_out, int64_t* seqs, int64_t ld_seqs,
                              float* logprobs, int64_t ld_logprobs, int64_t* word, int64_t end_idx, int t, int R, int V,
                              void* stream);
int64_t acvae_ensemble_rollout_scratch_bytes(int M, int N, int sample_n, int max_length, const int* S, const int* E,
                                             const int* H, const int* A, int V);
int acvae_ensemble_rollout(const void* const* const* params, const float* const* mem, const int64_t* const* mem_lens,
                           const float* const* eps, const int* S, const int* E, const int* H, const int* A, int M,
                           int64_t start_idx, int64_t end_idx, int method, float temp, int top_k, float top_p,
                           const float* noise, int64_t* seqs, float* logprobs, void* scratch, int64_t scratch_bytes, int N,
                           int sample_n, int max_length, int V, void* stream, float repetition_penalty,
                           int no_repeat_ngram_size, int min_length, const int* suppress_host, int n_suppress);

/* ---------------------------------------------------------------------------------------------
 * Constrained decoding on the device: four controls on a row's logits x at step t, applied inside every decoding loop in
 * front of the selection.  No counterpart in the reference.  h[0..t) is the row's history: the words it has emitted so
 * far, <start> not among them.  All are off by default, and with all four off every entry below runs exactly the launches
 * of its unconstrained base.
 *   repetition_penalty theta (off: 1.0f)  for every DISTINCT word w of h: x[w] <- x[w] / theta if x[w] > 0, else
 *                                         x[w] * theta; fp32, once per distinct word; theta finite and > 0;
 *   no_repeat_ngram_size n   (off: 0)     n >= 1 and t >= n - 1: for every i in [n - 1, t) with
 *                                         h[i-n+1 .. i) == h[t-n+1 .. t), ban h[i]: no n-gram of the finished caption
 *                                         occurs twice; n = 1 bans every word of h;
 *   min_length m             (off: 0)     ban end_idx at steps t < m; 0 <= m <= max_length;
 *   suppress_host, n_suppress (off: 0)    ban these ids at every step: a HOST array (may be NULL when n_suppress is 0) of
 *                                         at most ACVAE_SUPPRESS_MAX ids in [0, V), copied into the kernel arguments.
 * A ban writes -inf.  The penalty is applied first and a ban wins over it.  The edited row is the row everything
 * downstream sees: argmax, sampling (top_k / top_p truncate the constrained row), mixing and the flat top-k; the logits a
 * decode forward returns hold the constrained rows and sampled_logprobs is log_softmax of the constrained row at the
 * chosen word.  Finished rows keep emitting end_idx: the drivers' overrides come after the selection.  A history word
 * outside [0, V) is skipped.
 *
 * acvae_constrain_logits: the kernel alone, in place on R rows (row r at logits + r * ld, ld >= V; its history at
 * hist + r * hist_ld, int64, hist_ld >= t; hist may be NULL when t is 0).  One wavefront per row, O(t + n_suppress) logits
 * touched, no workspace.  With everything off it launches nothing and returns ACVAE_OK.
 *
 * acvae_decode_fwd_constrained: acvae_decode_fwd_truncated (which is its all-off case) with the controls; the history
 * of a row is its `seqs` row, the kernel runs between the classifier and the log-softmax of every step.
 * acvae_beam_search_constrained / acvae_ensemble_search_constrained: acvae_beam_search (which has no end_idx of its own, so
 * it is added) / acvae_ensemble_search with the controls on every member's logits in front of the mixing.  The greedy
 * history is the `seqs` row; the beam search keeps a word history per row that follows its parent every step (one more job
 * of the state gather), which needs the scratch of the *_constrained_scratch_bytes functions (the base sizes suffice when
 * every control is off).
 *
 * ACVAE_EINVAL, before anything is launched: theta not finite or <= 0; n < 0; m < 0 or (drivers) m > max_length;
 * n_suppress outside [0, ACVAE_SUPPRESS_MAX]; an id outside [0, V); n_suppress > 0 with a NULL list; and with a control on:
 * end_idx outside [0, V); V <= n_suppress + max_length + beam (beam = 1 for the decode forward; a row must keep a word, and
 * a clip `beam` finite scores); in the decode forward, caps != NULL (a teacher-forced row has no history of its own) or
 * ACVAE_FLAG_ROLLOUT_GRAD (the backward does not know the penalty's factor).
 * Out of scope: diverse beam search (acvae_dbs_search takes no controls), constraints in differentiable rollouts and in the
 * training forward, per-row settings.  (Finishing beams on end_idx and length-normalised scores: the *_finishing entries.)
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_SUPPRESS_MAX 64
int acvae_constrain_logits(float* logits, int64_t ld, const int64_t* hist, int64_t hist_ld, int t, int R, int V,
                           int end_idx, float repetition_penalty, int no_repeat_ngram_size, int min_length,
                           const int* suppress_host, int n_suppress, void* stream);
int acvae_decode_fwd_constrained(const void* const* params, const float* mem_in, const int64_t* mem_lens,
                                 const int64_t* caps, int64_t ld_caps, const int64_t* lens1, const float* q_z,
                                 const float* eps_p, const int* ss_flags_host, const int* dis_flags_host, float* logits,
                                 float* outputs, int64_t* seqs, float* sampled_logprobs, float* attn_w, float* p_means,
                                 float* p_logs, float* p_z, float* p_means_utt, float* h_final, float* hp_final,
                                 float* cp_final, void* saved, int64_t saved_bytes, void* scratch, int64_t scratch_bytes,
                                 int N, int Tc, int S, int E, int H, int A, int V, int Eenc, int start_idx, int end_idx,
                                 void* stream, void* aux_stream, int sample_method, float temp, const float* sample_noise,
                                 const uint8_t* emb_keep, float emb_drop_p, int flags, int top_k, float top_p,
                                 int32_t* kept, float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                 const int* suppress_host, int n_suppress);
int64_t acvae_beam_search_constrained_scratch_bytes(int N, int beam, int max_length, int S, int E, int H, int A, int V);
int acvae_beam_search_constrained(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                                  int64_t start_idx, int64_t* seqs, float* attn_weights, void* scratch,
                                  int64_t scratch_bytes, int N, int beam, int max_length, int S, int E, int H, int A, int V,
                                  void* stream, int64_t end_idx, float repetition_penalty, int no_repeat_ngram_size,
                                  int min_length, const int* suppress_host, int n_suppress);
int64_t acvae_ensemble_search_constrained_scratch_bytes(int M, int N, int beam, int max_length, const int* S, const int* E,
                                                        const int* H, const int* A, int V);
int acvae_ensemble_search_constrained(const void* const* const* params, const float* const* mem,
                                      const int64_t* const* mem_lens, const float* const* eps, const int* S, const int* E,
                                      const int* H, const int* A, int M, int64_t start_idx, int64_t end_idx, int greedy,
                                      int64_t* seqs, float* logprobs, void* scratch, int64_t scratch_bytes, int N, int beam,
                                      int max_length, int V, void* stream, float repetition_penalty,
                                      int no_repeat_ngram_size, int min_length, const int* suppress_host, int n_suppress);

/* ---------------------------------------------------------------------------------------------
 * Finishing beam search: hypotheses end at end_idx, are scored by length and reported as an n-best list.  The rule is the
 * one of the reference's diverse beam search (models/word_model.py:371-383: record a hypothesis when it emits <end> or at
 * the last step, score logprob / length, take it out of the beam), which its beam_search never applies (done_beams is
 * sorted and never filled).  Opt-in: the entries above are the same driver with finishing off and run what they ran.
 *
 * Definition.  Rows r = n * beam + j of clip n.  Step t forms scores[r,v] = c[r] + logmix_t[r,v] (acvae_ensemble_mix,
 * after the constraints) and the flat top-k over the clip's beam * V scores (acvae_topk_flat_batched: sorted descending,
 * ties to the lower flat index, t = 0 included) gives row r its cumulative score c_t[r], parent p_t[r] and word w_t[r].
 * Then, per row (acvae_beam_retire):
 *   1. r is alive iff c_t[r] > -inf;
 *   2. f_t[r] = c_t[r] if r is alive and (w_t[r] == end_idx or t == max_length - 1), else -inf      (the record);
 *   3. if w_t[r] == end_idx: c_t[r] <- -inf                                                        (the row is retired).
 * All children of a retired row score -inf at the next step (acvae_ensemble_mix with prev = -inf writes -inf into every
 * column, banned ones included; never NaN) and lose to every alive candidate; where a clip has fewer than `beam` alive
 * candidates the top-k takes such children: dead rows, never recorded.  (The reference's logprob_table[is_end] -= 1000
 * with -inf in the place of -1000.)  After the last step, per clip (acvae_beam_finish):
 *   candidates  every (t, j) with f_t[n * beam + j] > -inf;
 *   score       s = f_t / norm[t], ONE IEEE fp32 division, norm[t] = (float)pow((double)(t + 1), length_penalty) formed
 *               on the host (length_norm_host, [max_length], every entry finite and > 0; all ones = raw scores);
 *   order       s descending, then t ascending, then j ascending; the first `nbest` are returned;
 *   words       the parents traced back from (t, r) to step 0; positions behind t hold end_idx; length t + 1;
 *   missing     fewer than nbest candidates (only when bans leave a clip fewer than `beam` finite continuations): rows of
 *               end_idx with score and log-probability -inf and length 0.
 * The search itself is unchanged: same t = 0 rule, same noise, all max_length steps run, retired and dead rows keep being
 * stepped, no host read-back.  Finishing adds one acvae_beam_retire launch per step and replaces the final trace by
 * acvae_beam_finish; the norm table travels in kernel arguments (64 entries per launch) into the scratch.
 *
 * Outputs: nbest_seqs int64 [N,nbest,T], nbest_scores f32 [N,nbest] (s), nbest_logprobs f32 [N,nbest] (the raw f),
 * nbest_lengths int32 [N,nbest]; seqs [N,T] = hypothesis 0; acvae_beam_search_finishing: attn_weights [N,S,T] = hypothesis
 * 0's weights, zeros in the columns behind its length; acvae_ensemble_search_finishing: logprobs [N] = hypothesis 0's raw
 * log-probability.  Scratch of the *_finishing_scratch_bytes functions (never below the *_constrained ones).
 *
 * Refused before any launch, beside what the *_constrained entries refuse: nbest outside [1, beam], a NULL output, a NULL
 * norm table or an entry that is not finite and positive, end_idx outside [0, V), greedy != 0 in the ensemble entry
 * (ACVAE_EINVAL); scratch below the bytes function (ACVAE_EWORKSPACE).
 *
 * The kernels alone, on caller-built histories (device pointers unless named _host):
 *   acvae_beam_retire  c [R] in place, word int64 [R], f [R] out; last != 0 at the last step.
 *   acvae_beam_finish  parent / word int64, element (t, r) at [t * hist_stride + r], hist_stride >= R = N * beam; f [T][R];
 *                      attw [T][R][S] with attw_out [N,S,T], both or neither NULL (S is then ignored); seqs [N,T] and
 *                      logprobs [N] may be NULL; norm_dev: T floats of device workspace the table is written to.  A parent
 *                      outside [0, R) is clamped into it.  beam <= 16, T >= 1.
 * Out of scope: early exit once every clip has finished (needs a read-back), compacting retired rows out of the step
 * kernels, diverse beam search, consensus reranking of the n-best list, per-row settings, GNMT's ((5 + len) / 6)^alpha,
 * a coverage penalty.
 * ------------------------------------------------------------------------------------------- */
int acvae_beam_retire(float* c, const int64_t* word, float* f, int64_t end_idx, int last, int R, void* stream);
int acvae_beam_finish(const int64_t* parent, const int64_t* word, int64_t hist_stride, const float* f,
                      const float* length_norm_host, float* norm_dev, const float* attw, int64_t* seqs, float* logprobs,
                      float* attw_out, int64_t* nbest_seqs, float* nbest_scores, float* nbest_logprobs, int* nbest_lengths,
                      int N, int beam, int T, int S, int nbest, int64_t end_idx, void* stream);
int64_t acvae_beam_search_finishing_scratch_bytes(int N, int beam, int max_length, int S, int E, int H, int A, int V);
int acvae_beam_search_finishing(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                                int64_t start_idx, int64_t* seqs, float* attn_weights, void* scratch, int64_t scratch_bytes,
                                int N, int beam, int max_length, int S, int E, int H, int A, int V, void* stream,
                                int64_t end_idx, float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                const int* suppress_host, int n_suppress, const float* length_norm_host, int nbest,
                                int64_t* nbest_seqs, float* nbest_scores, float* nbest_logprobs, int* nbest_lengths);
int64_t acvae_ensemble_search_finishing_scratch_bytes(int M, int N, int beam, int max_length, const int* S, const int* E,
                                                      const int* H, const int* A, int V);
int acvae_ensemble_search_finishing(const void* const* const* params, const float* const* mem,
                                    const int64_t* const* mem_lens, const float* const* eps, const int* S, const int* E,
                                    const int* H, const int* A, int M, int64_t start_idx, int64_t end_idx, int greedy,
                                    int64_t* seqs, float* logprobs, void* scratch, int64_t scratch_bytes, int N, int beam,
                                    int max_length, int V, void* stream, float repetition_penalty, int no_repeat_ngram_size,
                                    int min_length, const int* suppress_host, int n_suppress,
                                    const float* length_norm_host, int nbest, int64_t* nbest_seqs, float* nbest_scores,
                                    float* nbest_logprobs, int* nbest_lengths);

/* ---------------------------------------------------------------------------------------------
 * Diverse beam search as one call: CaptionModel.diverse_beam_search (models/word_model.py:297-394) on Hybrid_VAEModel's
 * step, for all N clips at once, one model (acvae_dbs_search) or M members (acvae_ensemble_dbs_search; one driver, the
 * former is its M = 1 case).  No host synchronisation, no read-back; bit-identical in tokens and scores to the loop over
 * the step API, acvae_dbs_scores and acvae_topk_flat_batched that it replaces.
 *
 * Definition.  G groups of bdash beams per clip, R = N * bdash rows per group, row r = n * bdash + b of clip n,
 * T = max_length.  The schedule is the list of pairs (t, g), t = 0 .. T + G - 2, g = 0 .. G - 1, with 0 <= lt = t - g <= T - 1,
 * in that order; pair k of the n_steps = T * G reads the noise eps[k] [R][E].  Step (t, g):
 *   inputs   lt = 0: the word is start_idx, every state zero; else the word chosen at the group's previous local step and
 *            the states (decoder hidden [H]; the prior's h, c and last_z [E]) of the row's parent at that step;
 *   step     prior step, then decoder step, on the group's R rows (the launches of acvae_beam_search's driver);
 *   scores   score[r,c] = log_softmax(log_softmax(logits[r]) / temperature)[c] - diversity_lambda * count_n[c] + prev_g[r],
 *            count_n[c] = the number of beams of the groups e < g of clip n whose CURRENT history holds word c at column lt:
 *            group e's beams after its latest local step min(lt + g - e, T - 1), traced through the parents since.
 *            prev_g = the group's running scores, zero at lt = 0.  Bit for bit acvae_dbs_scores on the dense counts;
 *   top-k    per clip the flat top-bdash over bdash * V scores (lt = 0: over the first row's V), acvae_topk_flat_batched:
 *            value c, parent and word per row;
 *   record   a row is recorded iff its word is end_idx or lt = T - 1, with c as it is; then its running score becomes
 *            c - 1000.0f.  A retired row keeps being expanded and is recorded again whenever it emits end_idx again.
 * After the last step, per clip and group: the records ranked by (double)c / (double)(lt + 1) (IEEE fp64), descending,
 * ties in the order of recording (lt, then beam, ascending); the first bdash are kept.  Output rows per clip: with
 * group_nbest != 0 the groups' kept records in group order (rows = G * bdash), else each group's best (rows = G).
 * seqs int64 [N,rows,T]: the record's lt + 1 words through its parents, then end_idx; scores f64 [N,rows];
 * lengths int32 [N,rows].
 *
 * Ensembles: every member steps on the shared word with its own states and noise (eps[m] [n_steps][R][E[m]]); one
 * acvae_ensemble_mix launch (prev = NULL) forms log(mean_m softmax(logits_m)) per row, which takes the logits' place in
 * `scores`.  With M = 1 the mix is skipped: acvae_ensemble_dbs_search is acvae_dbs_search bit for bit.
 *
 * Refused before any launch: a dimension <= 0, a NULL pointer, start_idx / end_idx outside [0, V), temperature not finite
 * and > 0, diversity_lambda not finite, M outside [1, ACVAE_ENSEMBLE_MAX] (ACVAE_EINVAL); bdash > 16 (the top-k's limit),
 * G > 16 (the penalty list holds (G - 1) * bdash <= 240 words) or N * bdash > 2^20 (ACVAE_EUNSUPPORTED, -1 from the bytes
 * functions); scratch below the bytes function (ACVAE_EWORKSPACE).  The declared size is exact and the scratch may hold
 * anything on entry.
 *
 * The kernels alone, on caller-built tables (int32 [G][T][R], element (e, s, r) at [(e * T + s) * R + r]):
 *   acvae_dbs_scores_sparse  acvae_dbs_scores for group g at local step lt with the penalty read from the tables of the
 *                            groups e < g (parent_tab / word_tab may be NULL when g is 0); N clips, rows R = N * bdash;
 *                            logits row stride ld, prev [R] may be NULL, out [R][V].  A parent outside [0, R) is clamped
 *                            into it, a word outside [0, V) is skipped.
 *   acvae_dbs_advance        behind a top-k: c [R] in place (retired where recorded), parent / word int64 [R] in,
 *                            parent_out / word_out int32 [R] and rec_out f32 [R] (c, or NaN for "none") out; last != 0 at
 *                            lt = T - 1.
 *   acvae_dbs_finish         rec f32 [G][T][R]; outputs as above.
 * Out of scope: one batch of G * R rows per time step (other launch shapes, other bits), the decoding constraints,
 * truncation and reranking, an early exit, attention-weight histories.
 * ------------------------------------------------------------------------------------------- */
int acvae_dbs_scores_sparse(const float* logits, int64_t ld, float temperature, float diversity_lambda, const float* prev,
                            float* out, const int* parent_tab, const int* word_tab, int N, int bdash, int T, int V, int G,
                            int g, int lt, void* stream);
int acvae_dbs_advance(float* c, const int64_t* parent, const int64_t* word, int* parent_out, int* word_out, float* rec_out,
                      int64_t end_idx, int last, int R, void* stream);
int acvae_dbs_finish(const int* parent_tab, const int* word_tab, const float* rec, int64_t* seqs, double* scores,
                     int* lengths, int N, int G, int bdash, int T, int group_nbest, int64_t end_idx, void* stream);
int64_t acvae_dbs_search_scratch_bytes(int N, int G, int bdash, int T, int S, int E, int H, int A, int V);
int acvae_dbs_search(const void* const* params, const float* mem, const int64_t* mem_lens, const float* eps,
                     int64_t start_idx, int64_t end_idx, int N, int G, int bdash, int T, int S, int E, int H, int A, int V,
                     float temperature, float diversity_lambda, int group_nbest, int64_t* seqs, double* scores,
                     int* lengths, void* scratch, int64_t scratch_bytes, void* stream);
int64_t acvae_ensemble_dbs_search_scratch_bytes(int M, int N, int G, int bdash, int T, const int* S, const int* E,
                                                const int* H, const int* A, int V);
int acvae_ensemble_dbs_search(const void* const* const* params, const float* const* mem, const int64_t* const* mem_lens,
                              const float* const* eps, const int* S, const int* E, const int* H, const int* A, int M,
                              int64_t start_idx, int64_t end_idx, int N, int G, int bdash, int T, int V, float temperature,
                              float diversity_lambda, int group_nbest, int64_t* seqs, double* scores, int* lengths,
                              void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring GIVEN captions: per-step log-probability, rank and KL of a teacher-forced forward's outputs, and their per-row
 * sums (csrc/likelihood.hip; acvae_amd/likelihood.py is the front).  No counterpart in the reference, whose only
 * loss-shaped number is the label-smoothed batch scalar with its KL averaged over padded positions too (F8).
 *
 * acvae_caption_terms: one pass over R rows of T steps.  logits f32, row (r, t) at logits + r*ld_n + t*ld_t (V floats, as
 * acvae_ls_ce_fwd takes them); targets int64, (r, t) at targets + r*tg_sn + t; lens1 int64 [R], NULL = every cell valid,
 * 0 allowed, a value > T counts as T.  q_means / q_logs / p_means / p_logs f32 [R, T, E] contiguous (mu1, logvar1 of the
 * posterior; mu2, logvar2 of the prior); if any of the four is NULL no KL is requested, E is not used and `kl` may be NULL
 * (it is written as zeros if it is not).  A cell (r, t) is valid iff t < lens1[r].  Outputs [R, T] contiguous:
 *   logprob f32  x[tgt] - logsumexp(x) over the row's V logits x.  The row is read once: a running maximum and a sum
 *                of exp(x - maximum) per lane, merged against the row's maximum, so the log-sum-exp is max-subtracted
 *                throughout and is not taken from a precomputed lse.  A logit of -inf is a word of mass 0.  A row
 *                without a defined value - nothing but -inf, a +inf logit, a NaN logit anywhere in it (told by its
 *                bits) - gives NaN.
 *   rank    i32  #{v : x[v] > x[tgt]} + #{v < tgt : x[v] == x[tgt]}: the target's position under the first-maximum rule of
 *                acvae_row_logsoftmax_argmax / torch.max, so rank == 0 iff the greedy decode emits the target.  Comparisons
 *                of the fp32 inputs only: exact.  NaN logits compare with nothing and so count for nothing; a target
 *                whose own logit is NaN gets INT32_MAX (no top-1 / top-5 hit).  In a row of nothing but -inf every
 *                word ties: the rank is the target's index.
 *   kl      f32  sum over e < E of Normal_kl_loss's term (utils/train_util.py:259-266)
 *                lv2/2 - lv1/2 + (exp(lv1) + (mu1 - mu2)^2) / (2 exp(lv2)) - 1/2  in a fixed order.  The terms and their
 *                sum are evaluated in float64 (a term is what is left of summands that cancel) and the cell is rounded
 *                to fp32 once, at the store.
 * An invalid cell is written as exact zeros in all three outputs and none of its inputs is read.  A valid cell whose
 * target lies outside [0, V) is written as logprob = NaN, rank = INT32_MAX (its kl is the cell's own); the row is read,
 * nothing outside it is.  Every output element is stored exactly once; no atomics, no hand-off between workgroups, no
 * workspace; every sum has a fixed order (bit-reproducible).  One workgroup per cell: its work is V + 4E elements.  16-byte
 * loads of the logits when the base is 16-byte aligned and ld_n and ld_t are multiples of 4 (a V that is not has a scalar
 * tail), of the Gaussians when E is a multiple of 4 and the four bases are aligned; scalar loads otherwise.
 * ACVAE_EINVAL before any launch: logits / targets / logprob / rank NULL, R or T < 1, V < 2, E < 0, a negative stride,
 * R * T >= 2^31, or a KL requested with E < 1 or kl NULL.
 *
 * acvae_caption_sums: per row r over its valid cells t < min(max(lens1[r], 0), T) (lens1 NULL: T), t ascending, in float64:
 *   nll[r] = sum_t -(double)logprob[r,t]      kl_sum[r] = sum_t (double)kl[r,t]   (kl NULL: 0)
 *   tokens[r] = the number of valid cells      hit1[r] / hit5[r] = #{t : rank[r,t] < 1} / #{t : rank[r,t] < 5}   (int32)
 * One lane per row, serial over t: bit-equal to a host loop over the same cells; no transcendental function.
 * ------------------------------------------------------------------------------------------- */
int acvae_caption_terms(const float* logits, int64_t ld_n, int64_t ld_t, const int64_t* targets, int64_t tg_sn,
                        const int64_t* lens1, const float* q_means, const float* q_logs, const float* p_means,
                        const float* p_logs, float* logprob, int32_t* rank, float* kl, int R, int T, int V, int E,
                        void* stream);
int acvae_caption_sums(const float* logprob, const int32_t* rank, const float* kl, const int64_t* lens1, double* nll,
                       double* kl_sum, int32_t* tokens, int32_t* hit1, int32_t* hit5, int R, int T, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The variational term of the training objective: KL over a chosen set of cells, free bits, per-dimension and per-step
 * diagnostics (csrc/kl_objective.hip; acvae_amd/train_util.py: KLObjective is the front).  acvae_gauss_kl_fwd / bwd above
 * stay the reference's Normal_kl_loss, which averages over padded positions too (F8); the reference has no masked form in
 * use and no free bits.
 *
 * mu_q / lv_q / mu_p / lv_p f32 [R, T, E] contiguous (posterior mean and log-variance, prior mean and log-variance).
 * lens1 int64 [R] (cap_lens - 1) or NULL.  Per element
 *   k[r,t,e] = lv_p/2 - lv_q/2 + (exp(lv_q) + (mu_q - mu_p)^2) / (2 exp(lv_p)) - 1/2
 * evaluated in FLOAT64 (as acvae_caption_terms' kl; exactly 0 where q == p bit for bit).  The cell set S and divisor D:
 *   lens1 NULL:  every (r, t), and D must be R * T;
 *   lens1 given: the cells with t < lens1[r] (0 allowed, a value > T counts as T), and D is the caller's sum of those
 *                counts, 1 <= D <= R * T: the host knows the lengths, so nothing is read back.
 * With m_e = (1/D) sum_{c in S} k[c,e] and s_c = sum_e k[c,e]:
 *   free_bits == 0:                 kl = sum_e m_e                      (over_cell only chooses what gates_open counts)
 *   free_bits != 0, over_cell == 0: kl = sum_e max(m_e, lam)            gates u8 [E]:     m_e > lam
 *   free_bits != 0, over_cell != 0: kl = (1/D) sum_{c in S} max(s_c, lam)   gates u8 [R * T]: c in S and s_c > lam
 * The gate is strict (a tie is closed); a NaN m_e or s_c makes kl NaN and its gate closed.  lam >= 0 and finite.
 * Outputs, all written by the forward and none read back: kl f32 [1]; kl_raw f32 [1] = sum_e m_e whatever the free bits;
 * kl_dims f32 [E] = m_e; kl_steps f32 [T] = the mean of s_c over the rows r with (r, t) in S, 0 for a step with none;
 * gates_open i32 [1] = the number of open gates (free_bits == 0: E, or the number of cells of S if over_cell); gates as
 * above (free_bits == 0: not written, may be NULL).
 * Cells outside S are not read: a NaN or inf there changes nothing, forward or backward.
 * Three launches in stream order (slab partials; per-dimension and per-step finish; scalar); all sums in float64 in a
 * fixed order: the cells of a slab of ACVAE_KL_OBJECTIVE_SLAB consecutive cells, then the slabs ascending; a cell's
 * columns in groups of four per lane, then the lanes' butterfly.  No atomics, no hand-off inside a launch, every output
 * element stored once, bit-reproducible.  `scratch` holds acvae_kl_objective_scratch_bytes(R, T, E) bytes (8-byte aligned,
 * ACVAE_EALIGN otherwise); every word that is read was written by the same call, so its contents on entry do not matter.
 * 16-byte loads when E % 4 == 0 and the four bases are 16-byte aligned, scalar loads otherwise with the same order of
 * additions (the same bits); any E >= 1.
 * ACVAE_EINVAL before any launch: a NULL input or output (gates with free bits), R, T or E < 1, R * T >= 2^31, D outside
 * [1, R * T] or != R * T without lens1, lam negative, NaN or inf with free bits.  Then ACVAE_EWORKSPACE for a scratch that
 * is too small, also before any HIP call.
 *
 * acvae_kl_objective_bwd: one elementwise launch.  With g = grad_out[0] / D (fp32, as acvae_gauss_kl_bwd with D for rows)
 *   dmu_q = g d / v_p   dlv_q = g (-1/2 + v_q / (2 v_p))   dmu_p = -g d / v_p   dlv_p = g (1/2 - (v_q + d^2) / (2 v_p))
 * (d = mu_q - mu_p, v = exp(lv)) where the cell is in S and its gate is open (gates NULL: no free bits; over_cell says
 * whether gates is per cell or per dimension); exact zeros elsewhere, without reading the inputs of a cell that is outside S
 * or closed.  Any of the four outputs may be NULL (all four: nothing is launched).  lens1 and D as in the forward.
 * ------------------------------------------------------------------------------------------- */
#define ACVAE_KL_OBJECTIVE_SLAB 8
int64_t acvae_kl_objective_scratch_bytes(int R, int T, int E);
int acvae_kl_objective_fwd(const float* mu_q, const float* lv_q, const float* mu_p, const float* lv_p,
                           const int64_t* lens1, int64_t D, int free_bits, int over_cell, double lam, float* kl,
                           float* kl_raw, float* kl_dims, float* kl_steps, int32_t* gates_open, uint8_t* gates,
                           void* scratch, int64_t scratch_bytes, int R, int T, int E, void* stream);
int acvae_kl_objective_bwd(const float* mu_q, const float* lv_q, const float* mu_p, const float* lv_p,
                           const int64_t* lens1, int64_t D, int over_cell, const uint8_t* gates, const float* grad_out,
                           float* dmu_q, float* dlv_q, float* dmu_p, float* dlv_p, int R, int T, int E, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACVAE_HIP_H */
