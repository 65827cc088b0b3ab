// The index arithmetic and the rules of the one-call diverse beam search (include/acvae_hip.h has the definition), shared by
// its kernels (dbs_scores_sparse_kernel in losses.hip; dbs_advance_kernel and dbs_finish_kernel in search.hip) and by a
// plain C++ build: nothing here needs HIP, tests/test_dbs_device_cpu.py compiles it with the host compiler alone.
// Tables are int32 / fp32 [G][T][R]: element (e, s, r) = local step s of group e, row r = n * bdash + b.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ACVAE_DBS_HD __host__ __device__ inline
#else
#define ACVAE_DBS_HD inline
#endif

namespace acvae {
namespace dbs {

ACVAE_DBS_HD long at(int e, int s, long r, int T, int R) { return ((long)e * T + s) * R + r; }
// a parent outside [0, R) is clamped into it (the driver's come from the top-k and are in range)
ACVAE_DBS_HD long clamp_row(long p, int R) { return p < 0 ? 0 : (p >= R ? R - 1 : p); }
// the latest local step group e < g has run when group g is at local step lt
ACVAE_DBS_HD int latest_step(int lt, int g, int e, int T) {
  const int le = lt + g - e;
  return le < T - 1 ? le : T - 1;
}
// the word that row r of group e, as it stands after its latest step, holds at column lt: through every parent since
ACVAE_DBS_HD int column_word(const int* par_tab, const int* word_tab, int e, int g, int lt, long r, int T, int R) {
  for (int s = latest_step(lt, g, e, T); s > lt; --s) r = clamp_row(par_tab[at(e, s, r, T, R)], R);
  return word_tab[at(e, lt, r, T, R)];
}
// how often list[i] occurs among list[0 .. L), and whether i is its first occurrence
ACVAE_DBS_HD int multiplicity(const int* list, int L, int i, bool* first) {
  const int c = list[i];
  int mult = 0;
  bool f = true;
  for (int j = 0; j < L; ++j) {
    const bool same = list[j] == c;
    mult += same ? 1 : 0;
    f = f && !(same && j < i);
  }
  *first = f;
  return mult;
}

// record and retire: a row is recorded iff it emitted end_idx or this is the last step; "none" is a NaN
ACVAE_DBS_HD bool recorded(int64_t word, int64_t end_idx, int last) { return last != 0 || word == end_idx; }
ACVAE_DBS_HD float no_record() { return __builtin_nanf(""); }
ACVAE_DBS_HD bool is_record(float f) { return f == f; }
ACVAE_DBS_HD float retired(float c) { return c - 1000.0f; }

// ranking: key c / (lt + 1) in IEEE fp64, descending, ties to the lower candidate index i = lt * bdash + b
ACVAE_DBS_HD double key(float c, int lt) { return (double)c / (double)(lt + 1); }
ACVAE_DBS_HD bool better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }
ACVAE_DBS_HD int cand_step(int i, int bdash) { return i / bdash; }
ACVAE_DBS_HD long cand_row(int i, int bdash, int n) { return (long)n * bdash + (i - (i / bdash) * bdash); }
ACVAE_DBS_HD long out_row(int n, int g, int q, int G, int keep) { return ((long)n * G + g) * keep + q; }

// the words of the record made by row r at step t0 of group g (t0 < 0: none), then end_idx up to T
ACVAE_DBS_HD void trace(const int* par_tab, const int* word_tab, int g, int t0, long r, int T, int R, int64_t end_idx,
                        int64_t* row) {
  for (int t = T - 1; t > t0; --t) row[t] = end_idx;
  for (int t = t0; t >= 0; --t) {
    const long a = at(g, t, r, T, R);
    row[t] = word_tab[a];
    r = clamp_row(par_tab[a], R);
  }
}

}  // namespace dbs
}  // namespace acvae
