// CIDEr-D of the SCST rollouts on the device (the reward of self-critical training without a host round trip).
// The reference side - document frequencies, idf, the references' tf-idf weights, norms and lengths, the length-penalty
// table - is prepared on the host per batch (acvae_amd/cider.py); what depends on the sampled words is per row: at most
// 4 * 64 n-grams against a few reference vectors.
//
// One wavefront per row.  Lane i owns the n-grams that start at word i, one per order.  An n-gram that occurs several
// times in the row is summed once, by the lane of its first occurrence, with its count; the other lanes contribute an
// exact 0.  Every sum over n-grams is then formed by one lane per order walking the positions in order, so the terms
// are added in the order of first appearance: a fixed order (bit-reproducible), and the order in which a dictionary-based
// scorer walks its n-grams.  float64 throughout; the length penalty comes from the host's table, so no transcendental
// function is evaluated here.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int MAXL = ACVAE_CIDER_MAX_LENGTH;
constexpr int NORD = 4;
static_assert(MAXL == 64, "one lane per word of a row");

struct CiderTables {
  const uint64_t* idf_keys; const double* idf_vals; int n_idf; double log_d;
  const uint64_t* ref_keys; const double* ref_w; int n_entries;
  const int* ref_off; const double* ref_norm; const int* ref_len; int n_refs;
  const int* doc_ref; int n_docs;
  const int* row_doc; const int* row_src;
  const double* len_factor; int n_len;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Where the four keys k[] lie in the ascending, duplicate-free keys[lo, hi): at[j] = index or -1 (on[j] false: not searched).
// The four bisections run in lockstep with one trip count, so that their loads are in flight together: the tables were just
// uploaded, every probe is a miss of the L2, and a row's time is the number of dependent probes.
__device__ __forceinline__ void find_keys4(const uint64_t* __restrict__ keys, int lo0, int hi0, const uint64_t (&k)[NORD],
                                           const bool (&on)[NORD], int (&at)[NORD]) {
  int lo[NORD], hi[NORD];
#pragma unroll
  for (int j = 0; j < NORD; ++j) { lo[j] = lo0; hi[j] = on[j] ? hi0 : lo0; at[j] = -1; }
  for (int span = hi0 - lo0; span > 0; span >>= 1) {          // floor(log2 n) + 1 trips: what a bisection of n needs
    int mid[NORD];
    uint64_t v[NORD];
#pragma unroll
    for (int j = 0; j < NORD; ++j) {
      mid[j] = (lo[j] + hi[j]) >> 1;
      v[j] = keys[lo[j] < hi[j] ? mid[j] : lo0];               // always an index inside [lo0, hi0)
    }
#pragma unroll
    for (int j = 0; j < NORD; ++j)
      if (lo[j] < hi[j]) {
        if (v[j] == k[j]) at[j] = mid[j];
        if (v[j] < k[j]) lo[j] = mid[j] + 1; else hi[j] = mid[j];
      }
  }
}

__global__ __launch_bounds__(64) void ciderd_scores_kernel(const int64_t* __restrict__ seqs0, const int64_t* __restrict__ seqs1,
                                                          int64_t ld, int n, int max_length, int start_idx, int end_idx,
                                                          CiderTables t, double* __restrict__ score) {
  __shared__ int words[MAXL];                 // the cleaned row, id + 1 (0xFFFF: an id no table holds)
  __shared__ uint64_t keys[NORD][MAXL];
  __shared__ double term[NORD][MAXL];
  __shared__ double hnorm[NORD];
  __shared__ double part[NORD];
  const int lane = threadIdx.x;
  const int set = blockIdx.x / n, i = blockIdx.x - set * n;
  const int src = clampi(t.row_src[i], 0, n - 1);
  const int doc = clampi(t.row_doc[i], 0, t.n_docs - 1);
  const int64_t* row = (set == 0 ? seqs0 : seqs1) + (int64_t)src * ld;

  // 1. clean the row: lanes past max_length count as <end>
  const int64_t tok = lane < max_length ? row[lane] : (int64_t)end_idx;
  const unsigned long long endm = __ballot(tok == (int64_t)end_idx);
  const int first_end = endm ? __ffsll(endm) - 1 : MAXL;
  const bool keep = lane < first_end && tok != (int64_t)start_idx;
  const unsigned long long km = __ballot(keep);
  const int L = __popcll(km);
  if (keep) words[__popcll(km & ((1ull << lane) - 1ull))] = (tok >= 0 && tok < 65534) ? (int)tok + 1 : 0xFFFF;
  __syncthreads();

  // 2. the n-grams that start at this lane's word
  uint64_t key[NORD];
  bool lead[NORD];
  double vh[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) {
    uint64_t kk = 0;
    if (lane + k < L)
      for (int j = 0; j <= k; ++j) kk |= (uint64_t)words[lane + j] << (16 * j);
    key[k] = kk;                              // 0 where the row has no n-gram of this order here: no real key is 0
    keys[k][lane] = kk;
  }
  __syncthreads();

  // 3.-5. counts within the row, idf, the hypothesis' norms
  int cnt[NORD], at[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) {
    const int nk = L - k;                     // number of n-grams of order k + 1 (<= 0: none)
    int c = 0;
    bool first = lane < nk;
    for (int p = 0; p < nk; ++p) {
      const bool same = keys[k][p] == key[k];
      c += same ? 1 : 0;
      if (same && p < lane) first = false;
    }
    cnt[k] = c;
    lead[k] = first;
  }
  find_keys4(t.idf_keys, 0, t.n_idf, key, lead, at);
#pragma unroll
  for (int k = 0; k < NORD; ++k) {
    const double idf = at[k] >= 0 ? t.idf_vals[at[k]] : t.log_d;
    vh[k] = (double)cnt[k] * idf;
    term[k][lane] = lead[k] ? vh[k] * vh[k] : 0.0;
  }
  __syncthreads();
  if (lane < NORD) {
    double s = 0.0;
    for (int p = 0; p < L - lane; ++p) s += term[lane][p];
    hnorm[lane] = sqrt(s);
  }
  __syncthreads();

  // 6. the references of the row's document
  const int r0 = clampi(t.doc_ref[doc], 0, t.n_refs);
  const int r1 = clampi(t.doc_ref[doc + 1], r0, t.n_refs);
  const int len_h = L > 1 ? L - 1 : 0;        // the number of bigrams
  double acc = 0.0;                           // lanes 0..3: sum over the references of sim_k
  for (int r = r0; r < r1; ++r) {
    const int e0 = clampi(t.ref_off[r], 0, t.n_entries);
    const int e1 = clampi(t.ref_off[r + 1], e0, t.n_entries);
    find_keys4(t.ref_keys, e0, e1, key, lead, at);
#pragma unroll
    for (int k = 0; k < NORD; ++k) {
      const double vr = at[k] >= 0 ? t.ref_w[at[k]] : 0.0;     // an n-gram the reference does not hold: min(v, 0) * 0
      term[k][lane] = fmin(vh[k], vr) * vr;
    }
    __syncthreads();
    if (lane < NORD) {
      double s = 0.0;
      for (int p = 0; p < L - lane; ++p) s += term[lane][p];
      const double nh = hnorm[lane], nr = t.ref_norm[(int64_t)r * NORD + lane];
      if (nh != 0.0 && nr != 0.0) s /= nh * nr;
      const int d = len_h - t.ref_len[r];
      s *= t.len_factor[clampi(d < 0 ? -d : d, 0, t.n_len - 1)];
      acc += s;
    }
    __syncthreads();
  }

  // 7. mean over the orders, mean over the references, times 10
  if (lane < NORD) part[lane] = acc;
  __syncthreads();
  if (lane == 0) {
    const double m = (((part[0] + part[1]) + part[2]) + part[3]) / (double)NORD;
    score[blockIdx.x] = r1 > r0 ? m / (double)(r1 - r0) * 10.0 : 0.0;
  }
}

constexpr int RW_THREADS = 256;

__global__ __launch_bounds__(RW_THREADS) void ciderd_reward_kernel(const double* __restrict__ score, int n, int sample_n,
                                                                   float* __restrict__ reward, double* __restrict__ reward_mean) {
  __shared__ double red[RW_THREADS / 64];
  double mine = 0.0;
  for (int i = threadIdx.x; i < n; i += RW_THREADS) {
    double rw;
    if (sample_n <= 1) {
      rw = score[i] - score[n + i];
    } else {
      const int base = (i / sample_n) * sample_n;
      double s = 0.0;
      for (int j = 0; j < sample_n; ++j) s += score[base + j];
      const double me = score[i];
      rw = me - (s - me) / (double)(sample_n - 1);
    }
    reward[i] = (float)rw;
    mine += rw;
  }
  mine = wave_sum_d(mine);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0 && reward_mean) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < RW_THREADS / 64; ++w) tot += red[w];
    *reward_mean = tot / (double)n;
  }
}
}  // namespace

extern "C" int acvae_ciderd_scores(const int64_t* seqs0, const int64_t* seqs1, int64_t ld, int n, int n_sets, int max_length,
                                   int start_idx, int end_idx, const uint64_t* idf_keys, const double* idf_vals, int n_idf,
                                   double log_d, const uint64_t* ref_keys, const double* ref_w, int n_entries,
                                   const int* ref_off, const double* ref_norm, const int* ref_len, int n_refs,
                                   const int* doc_ref, int n_docs, const int* row_doc, const int* row_src,
                                   const double* len_factor, int n_len, double* score, void* stream) {
  if (!seqs0 || n <= 0 || (n_sets != 1 && n_sets != 2) || (n_sets == 2 && !seqs1) || (int64_t)n * n_sets > INT32_MAX)
    return ACVAE_EINVAL;
  if (max_length < 1 || max_length > ACVAE_CIDER_MAX_LENGTH || ld < max_length) return ACVAE_EINVAL;
  if (n_idf < 0 || (n_idf > 0 && (!idf_keys || !idf_vals)) || n_entries < 0 || (n_entries > 0 && (!ref_keys || !ref_w)))
    return ACVAE_EINVAL;
  if (!ref_off || !ref_norm || !ref_len || n_refs <= 0 || !doc_ref || n_docs <= 0 || !row_doc || !row_src || !len_factor ||
      n_len <= 0 || !score)
    return ACVAE_EINVAL;
  const CiderTables t{idf_keys, idf_vals, n_idf, log_d, ref_keys, ref_w, n_entries, ref_off, ref_norm, ref_len, n_refs,
                      doc_ref, n_docs, row_doc, row_src, len_factor, n_len};
  hipLaunchKernelGGL(ciderd_scores_kernel, dim3(n * n_sets), dim3(64), 0, (hipStream_t)stream, seqs0, seqs1, ld, n, max_length,
                     start_idx, end_idx, t, score);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_ciderd_reward(const double* score, int n, int sample_n, float* reward, double* reward_mean, void* stream) {
  if (!score || !reward || n <= 0 || (sample_n >= 2 && n % sample_n != 0)) return ACVAE_EINVAL;
  hipLaunchKernelGGL(ciderd_reward_kernel, dim3(1), dim3(RW_THREADS), 0, (hipStream_t)stream, score, n, sample_n, reward,
                     reward_mean);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
