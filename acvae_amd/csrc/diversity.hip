// Diversity of a clip's N captions on the device: the integer statistics behind Div-n, mBLEU and the vocabulary size
// (include/acvae_hip.h has the record's layout, acvae_amd/diversity.py the formulas).  The data layout and the cleaning rule
// are those of csrc/consensus.hip, the arithmetic is counting.
//
// One workgroup per clip, one wavefront per candidate, lane p = the n-grams that start at word p (one per order).
//   1. each wavefront cleans its row, marks its words in `seen` and writes to LDS, per word position, the packed four-word
//      key (from which the key of every order at that position is a mask away), and its length;
//   2. after a barrier lane p counts its n-grams within its own row (it contributes only where p is the n-gram's first
//      occurrence) and within every other candidate's row (every lane reads the same LDS address: a broadcast), keeps the
//      maximum of those counts, and notes whether a candidate j < i holds the n-gram (then it is not the clip's first);
//   3. the clipped counts of the four orders, each at most 64 per row, travel through one butterfly packed 8 bits apiece;
//      the clip-first n-grams are ballots; wavefront 0 adds the candidates' numbers up through LDS and writes the head.
// Integers only, no atomics, no scratch; 12.6 KB of static LDS.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int MAXL = ACVAE_CONSENSUS_MAX_LENGTH;
constexpr int MAXN = ACVAE_CONSENSUS_MAX_SAMPLES;
constexpr int NORD = 4;
constexpr int HEAD = ACVAE_DIVERSITY_HEAD, PER = ACVAE_DIVERSITY_PER_CANDIDATE;
static_assert(MAXL == 64, "one lane per word of a row");
static_assert(HEAD == 1 + NORD && PER == 2 + NORD, "the record's layout");

struct Cand {                                 // one candidate's share of the LDS
  uint64_t key4[MAXL];                        // words p .. p+3 packed (id + 1) << 16 j; a word past the end is 0
  int words[MAXL];                            // the cleaned row, id + 1 (0xFFFF: an id outside [0, V))
  int L;                                      // number of words
  int first[NORD];                            // the order-k n-grams of this candidate that no earlier candidate holds
  int pad[3];
};
static_assert(sizeof(Cand) % 16 == 0, "every candidate's slice starts 16-byte aligned");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint64_t order_mask(int k) { return k == 3 ? ~0ull : (1ull << (16 * (k + 1))) - 1ull; }

__global__ __launch_bounds__(64 * MAXN) void diversity_stats_kernel(
    const int64_t* __restrict__ seqs, int64_t ld, int sample_n, int max_length, int start_idx, int end_idx, int V,
    int* __restrict__ record, int* __restrict__ seen) {
  __shared__ __attribute__((aligned(16))) Cand cand[MAXN];
  const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;    // the launch has exactly sample_n <= MAXN wavefronts
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
  if (keep) {
    const bool inside = tok >= 0 && tok < (int64_t)V;         // (V <= 65534: id + 1 fits 16 bits below 0xFFFF)
    me.words[__popcll(km & ((1ull << lane) - 1ull))] = inside ? (int)tok + 1 : 0xFFFF;
    seen[inside ? (int)tok : V] = 1;
  }
  if (lane == 0) me.L = L;
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

  // 3. counts within the row; an n-gram contributes at the lane of its first occurrence
  int cnt[NORD];
  bool lead[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) { cnt[k] = 0; lead[k] = key[k] != 0; }
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

  // 4. the other candidates, j ascending: the maximum of their counts, and whether an earlier one holds the n-gram
  int most[NORD];
  bool first[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) { most[k] = 0; first[k] = lead[k]; }
  int reflen = 0, refgap = 2 * MAXL;
  for (int jj = 0; jj < sample_n - 1; ++jj) {
    const int j = jj + (jj >= i ? 1 : 0);
    const Cand& o = cand[j];
    const int Lj = clampi(o.L, 0, MAXL);
    const int gap = Lj > L ? Lj - L : L - Lj;
    if (gap < refgap || (gap == refgap && Lj < reflen)) { refgap = gap; reflen = Lj; }
    int c[NORD];
#pragma unroll
    for (int k = 0; k < NORD; ++k) c[k] = 0;
    for (int q0 = 0; q0 < Lj; q0 += 4) {
      uint64_t kq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) kq[u] = o.key4[q0 + u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < NORD; ++k) c[k] += (key[k] != 0 && (kq[u] & order_mask(k)) == key[k]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < NORD; ++k) {
      most[k] = c[k] > most[k] ? c[k] : most[k];
      if (j < i && c[k] > 0) first[k] = false;
    }
  }

  // 5. wavefront sums: the clipped counts packed 8 bits per order (a row has at most 64 n-grams of an order), the
  //    clip-first n-grams as ballots
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < NORD; ++k) packed |= (unsigned)(lead[k] ? (cnt[k] < most[k] ? cnt[k] : most[k]) : 0) << (8 * k);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
  int nfirst[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) nfirst[k] = __popcll(__ballot(first[k]));
  if (lane == 0) {
    int* out = record + clip * (HEAD + PER * sample_n) + HEAD + PER * i;
    out[0] = L;
    out[1] = reflen;
#pragma unroll
    for (int k = 0; k < NORD; ++k) { out[2 + k] = (int)((packed >> (8 * k)) & 0xFFu); me.first[k] = nfirst[k]; }
  }
  __syncthreads();

  // 6. the clip's head: words and the distinct n-grams of every order
  if (i == 0 && lane <= NORD) {
    int s = 0;
    for (int j = 0; j < sample_n; ++j) s += lane == 0 ? clampi(cand[j].L, 0, MAXL) : cand[j].first[lane - 1];
    record[clip * (HEAD + PER * sample_n) + lane] = s;
  }
}
}  // namespace

extern "C" int acvae_diversity_stats(const int64_t* seqs, int64_t ld, int n, int sample_n, int max_length, int start_idx,
                                     int end_idx, int V, int* record, int* seen, void* stream) {
  if (!seqs || !record || !seen) return ACVAE_EINVAL;
  if (sample_n < 2 || sample_n > ACVAE_CONSENSUS_MAX_SAMPLES || n <= 0 || n % sample_n != 0) return ACVAE_EINVAL;
  if (max_length < 1 || max_length > ACVAE_CONSENSUS_MAX_LENGTH || ld < max_length) return ACVAE_EINVAL;
  if (V < 1 || V > 65534) return ACVAE_EINVAL;
  hipLaunchKernelGGL(diversity_stats_kernel, dim3(n / sample_n), dim3(64 * sample_n), 0, (hipStream_t)stream, seqs, ld,
                     sample_n, max_length, start_idx, end_idx, V, record, seen);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
