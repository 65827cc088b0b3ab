// Constrained decoding: edits a row's logits at step t, in place, in front of the selection (argmax / sampling / ensemble
// mixing / flat top-k).  No counterpart in the reference.  h[0..t) is the row's history, the words it has emitted so far
// (<start> is not part of it):
//
//   repetition_penalty theta  for every DISTINCT word w of h: x[w] <- x[w] / theta if x[w] > 0, else x[w] * theta (fp32);
//   no_repeat_ngram_size n    n >= 1, t >= n - 1: for every i in [n - 1, t) with h[i-n+1 .. i) == h[t-n+1 .. t), ban h[i]
//                             (no n-gram of the caption occurs twice; n = 1 bans every word of h);
//   min_length m              ban end_idx at steps t < m;
//   suppress                  ban the listed ids at every step.
//
// A ban writes -inf.  The penalty comes first and a ban wins over it.
//
// One wavefront per row, CON_WAVES rows per workgroup.  Lanes take history positions, 64 at a time.  A row costs
// O(t * n / 64) comparisons per lane for the n-gram test and touches at most t + n_suppress + 1 logits, never the whole
// row.  The penalty must hit a word once however often it occurs: the lane at position i applies it only if no earlier
// position holds the same word, a scan of h[0..i) from the L1-resident history (t^2 / 2 comparisons per row, at most
// t - 1 in one lane below 64 steps: 29 at t = 30; the one part that is not O(t * n)).  Penalty stores and ban stores may
// target one address from different lanes, so the two phases are separated by a workgroup barrier and nothing depends on
// the order of the lanes; the bans of one phase all store the same value.  No atomics, no workspace, no LDS, no scratch.  Every word read from the history is range-checked before
// it addresses a logit, and one outside [0, V) is skipped.  The suppress list travels by value in the kernel arguments.
#include "constrain.h"

namespace {
constexpr int CON_WAVES = 4;
struct SuppressList { int n; int id[ACVAE_SUPPRESS_MAX]; };

__global__ __launch_bounds__(CON_WAVES * 64) void constrain_logits_kernel(
    float* __restrict__ logits, long ld, const int64_t* __restrict__ hist, long hist_ld, int t, int R, int V, int end_idx,
    float theta, int ngram, int min_len, SuppressList sup) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * CON_WAVES + (threadIdx.x >> 6);
  const bool live = r < R;                               // (no early return: every wavefront reaches the barrier)
  float* x = logits + (live ? r : 0) * ld;
  const int64_t* h = hist + (live ? r : 0) * hist_ld;

  // ---- phase 1: the penalty, once per distinct word (the lane of its first occurrence)
  if (live && theta != 1.f)
    for (int i = lane; i < t; i += 64) {
      const int64_t w = h[i];
      if (w < 0 || w >= V) continue;
      bool first = true;
      for (int j = 0; j < i && first; ++j) first = h[j] != w;
      if (first) {
        const float v = x[w];
        x[w] = v > 0.f ? v / theta : v * theta;
      }
    }
  __syncthreads();

  // ---- phase 2: the bans
  if (!live) return;
  if (t < min_len && lane == 0) x[end_idx] = -INFINITY;
  if (lane < sup.n) x[sup.id[lane]] = -INFINITY;          // (n <= 64 = ACVAE_SUPPRESS_MAX: one word per lane)
  if (ngram >= 1 && t >= ngram - 1)
    for (int i = ngram - 1 + lane; i < t; i += 64) {
      bool same = true;
      for (int k = 1; k < ngram && same; ++k) same = h[i - k] == h[t - k];
      const int64_t w = h[i];
      if (same && w >= 0 && w < V) x[w] = -INFINITY;
    }
}
}  // namespace

namespace acvae {
int constrain_rows(float* logits, long ld, const int64_t* hist, long hist_ld, int t, int R, int V, int end_idx,
                   const Constraints& c, hipStream_t st) {
  if (!c.on()) return ACVAE_OK;
  static_assert(ACVAE_SUPPRESS_MAX <= 64, "one suppressed word per lane");
  SuppressList sup;
  sup.n = c.n_suppress;
  for (int i = 0; i < ACVAE_SUPPRESS_MAX; ++i) sup.id[i] = i < c.n_suppress ? c.suppress[i] : 0;
  hipLaunchKernelGGL(constrain_logits_kernel, dim3((unsigned)cdiv(R, CON_WAVES)), dim3(CON_WAVES * 64), 0, st, logits, ld,
                     hist, hist_ld, t, R, V, end_idx, c.repetition_penalty, c.no_repeat_ngram_size, c.min_length, sup);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
}  // namespace acvae

extern "C" int acvae_constrain_logits(float* logits, int64_t ld, const int64_t* hist, int64_t hist_ld, int t, int R, int V,
                                      int end_idx, float repetition_penalty, int no_repeat_ngram_size, int min_length,
                                      const int* suppress_host, int n_suppress, void* stream) {
  acvae::Constraints c;
  c.repetition_penalty = repetition_penalty; c.no_repeat_ngram_size = no_repeat_ngram_size; c.min_length = min_length;
  c.suppress = suppress_host; c.n_suppress = n_suppress;
  if (R <= 0 || V <= 0 || t < 0) return ACVAE_EINVAL;
  ACVAE_TRY(acvae::constraints_check(c, V));
  if (!c.on()) return ACVAE_OK;
  if (!logits || ld < V || end_idx < 0 || end_idx >= V) return ACVAE_EINVAL;
  if (t > 0 && (!hist || hist_ld < t)) return ACVAE_EINVAL;
  return acvae::constrain_rows(logits, ld, hist, hist_ld, t, R, V, end_idx, c, (hipStream_t)stream);
}
