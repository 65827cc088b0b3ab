// Ensemble decoding, the mixing rule of BaseRunner._ensemble_batch / _ensemble_batch_beam_search
// (runners/base_runner.py:616-618, 675-680): at every step the members' word probabilities are averaged and the word is
// picked from the average.  One launch per step over the M members' logits [R, V]:
//
//   out[r, c] = log( (1/M) * sum_m softmax(logits_m[r])[c] ) + prev[r]
//
// and, optionally, the first-maximum column of out[r] and its value (what the greedy search needs: no top-k launch).
//
// One workgroup of 256 threads per row.  The arithmetic is fixed so that two identities hold exactly:
//   - a member's row statistic lse_m = max + logf(sum expf(x - max)) is formed as row_stats_kernel (losses.hip) forms it:
//     the same thread stride (256), the same in-thread order, the same wave butterfly and the same order over the waves.
//     That kernel sums expf(x - max) against the row's final maximum, so the maximum is a pass of its own here too (a
//     running maximum with a rescaled sum rounds differently and would break the identity).  lp_m = x - lse_m is then
//     bit-equal to what acvae_logprob_add forms from acvae_row_logsoftmax_argmax's lse;
//   - the mixture is a + logf(s / M), a = max_m lp_m, s = sum_m expf(lp_m - a) with the members added in index order, and
//     prev is added last.  M = 1: s = expf(0) = 1, logf(1 / 1) = 0, out = lp + prev, the two-kernel route bit for bit.
//     M copies of one matrix: every term is expf(0) = 1, s = M exactly, s / M = 1: bit-equal to M = 1.
// The row is read three times (maximum, sum, scores), M * V * 4 bytes each, the second and third time from L2 (100 KB at
// M = 5, V = 5000); HBM sees M * R * V * 4 bytes in and R * V * 4 out.  The member pointers travel by value in a bounded
// job table (job_table.h).
// ensemble_mix_sample_kernel, further down, is the same three passes with a sampled pick and the rollout's bookkeeping.
#include <math.h>
#include "common.h"
#include "job_table.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int MIX_THREADS = 256;       // row_stats_kernel's EW_THREADS: the identity above needs the same stride
constexpr int MIX_WAVES = MIX_THREADS / 64;

struct MixJob { const float* logits; long ld; };
using MixTable = acvae::JobTable<MixJob, ACVAE_ENSEMBLE_MAX>;

// Passes 1 and 2 of both kernels: every member's lse_m of row x[m][0..V), in row_stats_kernel's order.  red: M * MIX_WAVES
// floats of LDS; every thread of the workgroup calls it and gets every lse_m.
template <int M>
__device__ __forceinline__ void member_lse(const float* (&x)[M], int V, float* red, float (&lse)[M]) {
  const int w = threadIdx.x >> 6;
  // ---- pass 1: the members' row maxima
  float mx[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float v = -INFINITY;
    for (int c = threadIdx.x; c < V; c += MIX_THREADS) v = fmaxf(v, x[m][c]);
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[m * MIX_WAVES + w] = v;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float t = red[m * MIX_WAVES];
    for (int i = 1; i < MIX_WAVES; ++i) t = fmaxf(t, red[m * MIX_WAVES + i]);
    mx[m] = t;
  }
  __syncthreads();

  // ---- pass 2: sum expf(x - max) in row_stats_kernel's order (in-thread stride, wave butterfly, waves 0..3 from 0.f)
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float s = 0.f;
    for (int c = threadIdx.x; c < V; c += MIX_THREADS) s += expf(x[m][c] - mx[m]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[m * MIX_WAVES + w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float t = 0.f;
    for (int i = 0; i < MIX_WAVES; ++i) t += red[m * MIX_WAVES + i];
    lse[m] = mx[m] + logf(t);
  }
}

// Pass 3 of both kernels, one column: the mixture's log-probability a + logf(s / M) of word c.
template <int M>
__device__ __forceinline__ float mix_value(const float* (&x)[M], const float (&lse)[M], int c) {
  float lp[M];
  float a = -INFINITY;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    lp[m] = x[m][c] - lse[m];
    a = fmaxf(a, lp[m]);
  }
  if (!(a > -INFINITY)) return a;                        // every member at -inf: the mixture is -inf, not inf - inf
  float s = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m) s += expf(lp[m] - a);
  return a + logf(s / (float)M);
}

template <int M>
__global__ __launch_bounds__(MIX_THREADS) void ensemble_mix_kernel(MixTable tab, const float* __restrict__ prev,
                                                                   float* __restrict__ out, long ld_out,
                                                                   int64_t* __restrict__ argmax, float* __restrict__ best,
                                                                   long o_stride, int V) {
  __shared__ float red[M * MIX_WAVES];
  __shared__ float redv[MIX_WAVES];
  __shared__ int redi[MIX_WAVES];
  const long r = blockIdx.x;
  const int w = threadIdx.x >> 6;
  const float* x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = tab.job[m].logits + r * tab.job[m].ld;
  float lse[M];
  member_lse<M>(x, V, red, lse);

  // ---- pass 3: the mixture's scores, and their first maximum
  const float pv = prev ? prev[r] : 0.f;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < V; c += MIX_THREADS) {
    const float v = mix_value<M>(x, lse, c) + pv;
    if (out) out[r * ld_out + c] = v;
    if (v > bv) { bv = v; bi = c; }                      // strict '>': the first maximum within the thread's stride
  }
  if (!argmax && !best) return;                          // uniform over the block
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { redv[w] = bv; redi[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < MIX_WAVES; ++i)
      if (redv[i] > bv || (redv[i] == bv && redi[i] < bi)) { bv = redv[i]; bi = redi[i]; }
    if (argmax) argmax[r * o_stride] = bi;
    if (best) best[r * o_stride] = bv;
  }
}

// The sampled word from the mixture, one launch per step of a rollout (acvae_ensemble_rollout): passes 1 and 2 are
// member_lse, pass 3 forms v_c = mix_value (no prev) and scores it by sample_rows_kernel's rule (losses.hip) on the caller's
// noise row z:
//   ACVAE_SAMPLE_GUMBEL       (v_c + z_c) / temp          z: Gumbel noise
//   ACVAE_SAMPLE_MULTINOMIAL  expf(v_c / temp) / z_c      z ~ Exp(1)
// THE TEMPERATURE ACTS ON THE MIXTURE: the members are mixed at temperature 1 and the mixture's log-probabilities are
// divided by temp (softmax(v / temp) is the distribution "sample" draws from), not the members' logits before the mixing.
// First-maximum argmax with sample_rows_kernel's reductions (a thread's first column is taken whatever its score, a NaN
// included; the butterfly and the waves prefer the larger score, then the lower index); a row whose scores are all NaN gets
// a word clamped into the row.  Thread 0 then does greedy_pick_kernel's bookkeeping (search.hip): a row whose previous
// word is end_idx keeps end_idx; seqs[r, t], the word fed to the next step, and logprobs[r, t] = v of the chosen word
// (untempered; recomputed by thread 0 with pass 3's own arithmetic, so it is the bits `out` holds there).
// The mixed row reaches HBM only through the optional `out`.  No atomics, no workspace, no hand-off between workgroups;
// every sum is formed in a fixed order.
// Resources (hipcc's remarks), M = 1 / 2 / 5 / 8: 25 / 25 / 36 / 40 VGPRs, 48 / 64 / 112 / 160 bytes of LDS, no scratch
// in any.
template <int M>
__global__ __launch_bounds__(MIX_THREADS) void ensemble_mix_sample_kernel(
    MixTable tab, const float* __restrict__ noise, long ld_nz, int method, float temp, float* __restrict__ out, long ld_out,
    int64_t* __restrict__ seqs, long ld_seqs, float* __restrict__ logprobs, long ld_lp, int64_t* __restrict__ word,
    int64_t end_idx, int t, int V) {
  __shared__ float red[M * MIX_WAVES];
  __shared__ float redv[MIX_WAVES];
  __shared__ int redi[MIX_WAVES];
  const long r = blockIdx.x;
  const int w = threadIdx.x >> 6;
  const float* x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = tab.job[m].logits + r * tab.job[m].ld;
  const float* z = noise + r * ld_nz;
  float lse[M];
  member_lse<M>(x, V, red, lse);

  // ---- pass 3: the mixture's log-probabilities, their scores and the first maximum of those
  float bs = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < V; c += MIX_THREADS) {
    const float v = mix_value<M>(x, lse, c);
    if (out) out[r * ld_out + c] = v;
    const float sc = method == ACVAE_SAMPLE_GUMBEL ? (v + z[c]) / temp : expf(v / temp) / z[c];
    if (sc > bs || bi == 0x7fffffff) { bs = sc; bi = c; }   // strict '>': first maximum within the stride
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { redv[w] = bs; redi[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < MIX_WAVES; ++i)
      if (redv[i] > bs || (redv[i] == bs && redi[i] < bi)) { bs = redv[i]; bi = redi[i]; }
    if (bi < 0 || bi >= V) bi = 0;                        // every score NaN: sample_rows_kernel's clamp
    int64_t wd = bi;
    if (t > 0 && seqs[r * ld_seqs + t - 1] == end_idx) wd = end_idx;   // a finished row keeps end_idx
    seqs[r * ld_seqs + t] = wd;
    logprobs[r * ld_lp + t] = mix_value<M>(x, lse, bi);
    word[r] = wd;
  }
}

// The member table of both entries, ACVAE_EINVAL for what cannot be one.
int mix_table(const float* const* logits, const int64_t* ld, int M, int V, MixTable& tab) {
  if (!logits || !ld || M < 1 || M > ACVAE_ENSEMBLE_MAX) return ACVAE_EINVAL;
  for (int m = 0; m < M; ++m) {
    if (!logits[m] || ld[m] < V) return ACVAE_EINVAL;
    tab.add({logits[m], (long)ld[m]});
  }
  return tab.ok() ? ACVAE_OK : ACVAE_EINVAL;
}

// kernel<M> for the call's M (the table holds 1 .. ACVAE_ENSEMBLE_MAX members)
#define ACVAE_MIX_DISPATCH(kernel, M, R, st, ...)                                                                      \
  switch (M) {                                                                                                         \
    case 1: hipLaunchKernelGGL(kernel<1>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    case 2: hipLaunchKernelGGL(kernel<2>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    case 3: hipLaunchKernelGGL(kernel<3>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    case 4: hipLaunchKernelGGL(kernel<4>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    case 5: hipLaunchKernelGGL(kernel<5>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    case 6: hipLaunchKernelGGL(kernel<6>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    case 7: hipLaunchKernelGGL(kernel<7>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;          \
    default: hipLaunchKernelGGL(kernel<8>, dim3((unsigned)(R)), dim3(MIX_THREADS), 0, st, __VA_ARGS__); break;         \
  }
}  // namespace

extern "C" int acvae_ensemble_mix(const float* const* logits, const int64_t* ld, int M, const float* prev, float* out,
                                  int64_t ld_out, int64_t* argmax, float* best, int64_t o_stride, int R, int V,
                                  void* stream) {
  if (R <= 0 || V <= 0) return ACVAE_EINVAL;
  if (!out && !argmax && !best) return ACVAE_EINVAL;
  if ((out && ld_out < V) || ((argmax || best) && o_stride < 1)) return ACVAE_EINVAL;
  MixTable tab;
  ACVAE_TRY(mix_table(logits, ld, M, V, tab));
  ACVAE_MIX_DISPATCH(ensemble_mix_kernel, M, R, (hipStream_t)stream, tab, prev, out, (long)ld_out, argmax, best,
                     (long)o_stride, V);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_ensemble_mix_sample(const float* const* logits, const int64_t* ld, int M, const float* noise,
                                         int64_t ld_noise, int method, float temp, float* out, int64_t ld_out,
                                         int64_t* seqs, int64_t ld_seqs, float* logprobs, int64_t ld_logprobs, int64_t* word,
                                         int64_t end_idx, int t, int R, int V, void* stream) {
  if (R <= 0 || V <= 0 || t < 0) return ACVAE_EINVAL;
  if (method != ACVAE_SAMPLE_GUMBEL && method != ACVAE_SAMPLE_MULTINOMIAL) return ACVAE_EINVAL;
  if (!isfinite(temp) || !(temp > 0.f)) return ACVAE_EINVAL;
  if (!noise || ld_noise < V || (out && ld_out < V)) return ACVAE_EINVAL;
  if (!seqs || !logprobs || !word || ld_seqs <= t || ld_logprobs <= t) return ACVAE_EINVAL;
  MixTable tab;
  ACVAE_TRY(mix_table(logits, ld, M, V, tab));
  ACVAE_MIX_DISPATCH(ensemble_mix_sample_kernel, M, R, (hipStream_t)stream, tab, noise, (long)ld_noise, method, temp, out,
                     (long)ld_out, seqs, (long)ld_seqs, logprobs, (long)ld_logprobs, word, end_idx, t, V);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
