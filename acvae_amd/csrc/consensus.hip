// Consensus (minimum-Bayes-risk) reranking of a clip's sampled captions under CIDEr-D, on the device: every candidate
// is scored with the clip's OTHER candidates as its references, and the best one is picked.  Unlike csrc/cider.hip, whose
// reference side is prepared on the host, the "references" here are the other rows of the same launch; the only table
// is a corpus-level (key, idf) array the caller uploads once (acvae_amd/consensus.py), which may be empty.
//
// One workgroup per clip, one wavefront per candidate, lane p = the n-grams that start at word p (one per order).
//   1. each wavefront cleans its row and writes to LDS, per word position, the packed four-word key (from which the key
//      of every order at that position is a mask away) and per order the weight count * idf (at EVERY position of an
//      n-gram, so that a match at any of them yields the weight), then its norms and its length;
//   2. after a barrier it walks the other candidates' positions in LDS: lane p looks its n-grams up among candidate j's,
//      forms min(v_i, v_j) * v_j at the position of the n-gram's first occurrence (an exact 0 elsewhere), and one lane per
//      order adds the positions up in order: the order of first appearance, j ascending, orders ((s0 + s1) + s2) + s3;
//   3. wavefront 0 takes the first maximum of the workgroup's scores and copies the picked row.
// float64 throughout, no atomics, no transcendental function (the length penalty is the host's table).  The sums over
// positions go through a [2][64] float64 buffer, two orders at a time, which keeps a candidate at 3888 bytes of LDS and
// sixteen candidates inside 64 KB of dynamic LDS.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int MAXL = ACVAE_CONSENSUS_MAX_LENGTH;
constexpr int MAXN = ACVAE_CONSENSUS_MAX_SAMPLES;
constexpr int NORD = 4;
static_assert(MAXL == 64, "one lane per word of a row");

struct Cand {                                 // one candidate's share of the dynamic LDS
  uint64_t key4[MAXL];                        // words p .. p+3 packed (id + 1) << 16 j; a word past the end is 0
  double w[NORD][MAXL];                       // count * idf of the order-k n-gram at position p (0 where there is none)
  double term[2][MAXL];                       // the terms of two orders, summed by lanes 0 and 1
  double norm[NORD];
  double score;
  int len, L;                                 // number of bigrams, number of words
  int words[MAXL];                            // the cleaned row, id + 1 (0xFFFF: an id outside [0, 65534))
};
static_assert(sizeof(Cand) % 16 == 0, "every candidate's slice of the dynamic LDS starts 16-byte aligned");
static_assert(sizeof(Cand) * MAXN <= 65536, "sixteen candidates fit the 64 KB a launch may ask for");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint64_t order_mask(int k) { return k == 3 ? ~0ull : (1ull << (16 * (k + 1))) - 1ull; }

// Where the four keys k[] lie in the ascending, duplicate-free keys[0, n): at[j] = index or -1 (on[j] false: not searched).
// The four bisections run in lockstep with one trip count, so that their loads are in flight together.
__device__ __forceinline__ void find_idf4(const uint64_t* __restrict__ keys, int n, const uint64_t (&k)[NORD],
                                          const bool (&on)[NORD], int (&at)[NORD]) {
  int lo[NORD], hi[NORD];
#pragma unroll
  for (int j = 0; j < NORD; ++j) { lo[j] = 0; hi[j] = on[j] ? n : 0; at[j] = -1; }
  for (int span = n; span > 0; span >>= 1) {                   // floor(log2 n) + 1 trips: what a bisection of n needs
    int mid[NORD];
    uint64_t v[NORD];
#pragma unroll
    for (int j = 0; j < NORD; ++j) {
      mid[j] = (lo[j] + hi[j]) >> 1;
      v[j] = keys[lo[j] < hi[j] ? mid[j] : 0];                  // always an index inside [0, n)
    }
#pragma unroll
    for (int j = 0; j < NORD; ++j)
      if (lo[j] < hi[j]) {
        if (v[j] == k[j]) at[j] = mid[j];
        if (v[j] < k[j]) lo[j] = mid[j] + 1; else hi[j] = mid[j];
      }
  }
}

// The sum of term[lane][0 .. L) in position order, by lanes 0 and 1.  Every position of the row was written and those past
// an order's last n-gram hold an exact 0, so the walk goes in chunks of eight whose loads are in flight together; the
// additions stay one chain in position order.
__device__ __forceinline__ double walk(const double (&term)[2][MAXL], int lane, int L) {
  double s = 0.0;
  if (lane < 2)
    for (int p0 = 0; p0 < L; p0 += 8) {      // (L <= 64 = 8 * 8: p0 + 7 stays inside the row)
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = term[lane][p0 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += x[u];
    }
  return s;
}

__global__ __launch_bounds__(64 * MAXN) void consensus_scores_kernel(
    const int64_t* __restrict__ seqs, int64_t ld, int sample_n, int max_length, int start_idx, int end_idx,
    const uint64_t* __restrict__ idf_keys, const double* __restrict__ idf_vals, int n_idf, double log_d,
    const double* __restrict__ len_factor, int n_len, double* __restrict__ score, int64_t* __restrict__ best,
    int64_t* __restrict__ picked) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Cand* cand = reinterpret_cast<Cand*>(smem);
  const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;    // the launch has exactly sample_n wavefronts
  const int64_t clip = blockIdx.x;
  Cand& me = cand[i];
  const int64_t* row = seqs + (clip * sample_n + i) * ld;

  // 1. clean the row: lanes past max_length count as <end>
  const int64_t tok = lane < max_length ? row[lane] : (int64_t)end_idx;
  const unsigned long long endm = __ballot(tok == (int64_t)end_idx);
  const int first_end = endm ? __ffsll(endm) - 1 : MAXL;
  const bool keep = lane < first_end && tok != (int64_t)start_idx;
  const unsigned long long km = __ballot(keep);
  const int L = __popcll(km);
  if (keep) me.words[__popcll(km & ((1ull << lane) - 1ull))] = (tok >= 0 && tok < 65534) ? (int)tok + 1 : 0xFFFF;
  __syncthreads();

  // 2. the n-grams that start at this lane's word
  uint64_t k4 = 0;
#pragma unroll
  for (int j = 0; j < NORD; ++j)
    if (lane + j < L) k4 |= (uint64_t)me.words[lane + j] << (16 * j);
  me.key4[lane] = k4;
  uint64_t key[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) key[k] = lane + k < L ? (k4 & order_mask(k)) : 0;     // no real key is 0
  __syncthreads();

  // 3. counts within the row (an n-gram is summed by the lane of its first occurrence), idf, weights
  int cnt[NORD], at[NORD];
  bool lead[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) { cnt[k] = 0; lead[k] = lane + k < L; }
  for (int p0 = 0; p0 < L; p0 += 4) {        // in chunks of four loads; a position past the row holds 0 and matches nothing
    uint64_t kp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) kp[u] = me.key4[p0 + u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < NORD; ++k) {        // (masked to order k, kp holds a zero field unless p + k < L: no match)
        const bool same = key[k] != 0 && (kp[u] & order_mask(k)) == key[k];
        cnt[k] += same ? 1 : 0;
        if (same && p0 + u < lane) lead[k] = false;
      }
  }
  bool valid[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) valid[k] = key[k] != 0;
  find_idf4(idf_keys, n_idf, key, valid, at);                  // every position of an n-gram carries its weight: a match at
  double v[NORD];                                              // any of them then yields it
#pragma unroll
  for (int k = 0; k < NORD; ++k) {
    const double idf = at[k] >= 0 ? idf_vals[at[k]] : log_d;
    v[k] = (double)cnt[k] * idf;
    me.w[k][lane] = valid[k] ? v[k] : 0.0;
  }

  // 4. the candidate's norms and length
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) me.term[kk][lane] = lead[2 * half + kk] ? v[2 * half + kk] * v[2 * half + kk] : 0.0;
    __syncthreads();
    const double s = walk(me.term, lane, L);
    if (lane < 2) me.norm[2 * half + lane] = sqrt(s);
    __syncthreads();
  }
  if (lane == 0) { me.len = L > 1 ? L - 1 : 0; me.L = L; }
  __syncthreads();

  // 5. the other candidates, j ascending (every wavefront makes sample_n - 1 trips: the barriers below are uniform)
  double acc[2] = {0.0, 0.0};                 // lanes 0 and 1: sum over j of sim_k, k = lane and k = 2 + lane
  for (int jj = 0; jj < sample_n - 1; ++jj) {
    const int j = jj + (jj >= i ? 1 : 0);
    const Cand& o = cand[j];
    const int Lj = clampi(o.L, 0, MAXL);
#pragma unroll
    for (int k = 0; k < NORD; ++k) at[k] = -1;
    for (int q0 = 0; q0 < Lj; q0 += 4) {
      uint64_t kq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) kq[u] = o.key4[q0 + u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < NORD; ++k)                          // (a lane without an n-gram of this order, key 0, may "match" a
          if ((kq[u] & order_mask(k)) == key[k]) at[k] = q0 + u;   // position past j's end: it is no lead and adds nothing)
    }
    double t[NORD];
#pragma unroll
    for (int k = 0; k < NORD; ++k) {
      const double vr = at[k] >= 0 ? o.w[k][at[k]] : 0.0;       // an n-gram candidate j does not hold: min(v, 0) * 0
      t[k] = lead[k] ? fmin(v[k], vr) * vr : 0.0;
    }
    const int d = me.len - o.len;
    const double pen = len_factor[clampi(d < 0 ? -d : d, 0, n_len - 1)];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      me.term[0][lane] = t[2 * half];
      me.term[1][lane] = t[2 * half + 1];
      __syncthreads();
      double s = walk(me.term, lane, L);
      if (lane < 2) {
        const double nh = me.norm[2 * half + lane], nr = o.norm[2 * half + lane];
        if (nh != 0.0 && nr != 0.0) s /= nh * nr;
        acc[half] += s * pen;
      }
      __syncthreads();
    }
  }

  // 6. mean over the orders, mean over the other candidates, times 10
  if (lane < 2) { me.term[0][lane] = acc[0]; me.term[0][2 + lane] = acc[1]; }
  __syncthreads();
  if (lane == 0) {
    const double m = (((me.term[0][0] + me.term[0][1]) + me.term[0][2]) + me.term[0][3]) / (double)NORD;
    const double sc = L > 0 ? m / (double)(sample_n - 1) * 10.0 : 0.0;
    me.score = sc;
    score[clip * sample_n + i] = sc;
  }
  __syncthreads();

  // 7. the first maximum and its row
  if (i == 0) {
    int b = 0;
    double top = cand[0].score;
    for (int j = 1; j < sample_n; ++j) {
      const double s = cand[j].score;
      if (s > top) { top = s; b = j; }
    }
    if (lane == 0) best[clip] = b;
    if (picked && lane < max_length) picked[clip * max_length + lane] = seqs[(clip * sample_n + b) * ld + lane];
  }
}
}  // namespace

extern "C" int acvae_consensus_scores(const int64_t* seqs, int64_t ld, int n, int sample_n, int max_length, int start_idx,
                                      int end_idx, const uint64_t* idf_keys, const double* idf_vals, int n_idf, double log_d,
                                      const double* len_factor, int n_len, double* score, int64_t* best, int64_t* picked,
                                      void* stream) {
  if (!seqs || !len_factor || !score || !best) return ACVAE_EINVAL;
  if (sample_n < 2 || sample_n > ACVAE_CONSENSUS_MAX_SAMPLES || n <= 0 || n % sample_n != 0) return ACVAE_EINVAL;
  if (max_length < 1 || max_length > ACVAE_CONSENSUS_MAX_LENGTH || ld < max_length || n_len <= 0) return ACVAE_EINVAL;
  if (n_idf < 0 || (n_idf > 0 && (!idf_keys || !idf_vals))) return ACVAE_EINVAL;
  hipLaunchKernelGGL(consensus_scores_kernel, dim3(n / sample_n), dim3(64 * sample_n), sizeof(Cand) * (size_t)sample_n,
                     (hipStream_t)stream, seqs, ld, sample_n, max_length, start_idx, end_idx, idf_keys, idf_vals, n_idf, log_d,
                     len_factor, n_len, score, best, picked);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
