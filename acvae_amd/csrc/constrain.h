// Constrained decoding: the controls every decoding loop applies to a row's logits in front of its selection
// (constrain.hip has the kernel and the definitions).  Host side only: the drivers validate once, before their first launch,
// and then enqueue one launch per step and member.
#pragma once
#include <math.h>
#include "common.h"
#include "../../include/acvae_hip.h"

namespace acvae {

// The four controls as the C entries receive them; `suppress` is a HOST array.
struct Constraints {
  float repetition_penalty = 1.f;
  int no_repeat_ngram_size = 0;
  int min_length = 0;
  const int* suppress = nullptr;
  int n_suppress = 0;
  bool on() const { return repetition_penalty != 1.f || no_repeat_ngram_size > 0 || min_length > 0 || n_suppress > 0; }
};

// Values alone (what acvae_constrain_logits refuses).
inline int constraints_check(const Constraints& c, int V) {
  if (!isfinite(c.repetition_penalty) || !(c.repetition_penalty > 0.f)) return ACVAE_EINVAL;
  if (c.no_repeat_ngram_size < 0 || c.min_length < 0) return ACVAE_EINVAL;
  if (c.n_suppress < 0 || c.n_suppress > ACVAE_SUPPRESS_MAX || (c.n_suppress > 0 && !c.suppress)) return ACVAE_EINVAL;
  for (int i = 0; i < c.n_suppress; ++i)
    if (c.suppress[i] < 0 || c.suppress[i] >= V) return ACVAE_EINVAL;
  return ACVAE_OK;
}

// A decoding loop of max_length steps over `beam` rows per clip.  With a control on, a row must keep a word: a step bans at
// most n_suppress + t + 1 words of a row (the list, one word per history position, end_idx), and the flat top-k needs
// `beam` finite scores per clip.
inline int constraints_check_loop(const Constraints& c, int V, int end_idx, int max_length, int beam) {
  ACVAE_TRY(constraints_check(c, V));
  if (!c.on()) return ACVAE_OK;
  if (c.min_length > max_length || end_idx < 0 || end_idx >= V) return ACVAE_EINVAL;
  if ((long)V <= (long)c.n_suppress + max_length + beam) return ACVAE_EINVAL;
  return ACVAE_OK;
}

// One launch over R rows (none when nothing is on); the arguments have passed constraints_check.
int constrain_rows(float* logits, long ld, const int64_t* hist, long hist_ld, int t, int R, int V, int end_idx,
                   const Constraints& c, hipStream_t st);

}  // namespace acvae
