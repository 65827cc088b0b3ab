// Captions against their references on the device: the integer statistics behind BLEU-1..4 and ROUGE-L
// (include/acvae_hip.h has the record's layout, acvae_amd/accuracy.py the formulas).  The cleaning rule and the key format are
// those of csrc/diversity.hip; the references are real ones: ragged, any number per clip, of any length, with words
// outside the vocabulary.
//
// One workgroup = one wavefront = one token row; lane p = the candidate n-grams that start at word p (one per order).
//   1. the wavefront cleans its row into LDS (id + 1; 0xFFFF for an id outside [0, V)) and forms, per word position, the
//      packed four-word key; an n-gram that holds 0xFFFF gets the key 0, which matches nothing;
//   2. lane p counts its n-grams within the row (it contributes only where p is the n-gram's first occurrence);
//   3. the clip's references are streamed, 64 words per step: one coalesced load (the next step's words are in flight while
//      this step's are used), their four-word keys formed in registers from the neighbouring lanes, and per reference word
//      one broadcast of its key to all lanes, which count their matches per order.  A reference word outside the vocabulary
//      is 0xFFFF, which no surviving candidate key holds.  The same broadcast word advances the bit-parallel LCS, whose
//      state is one 64-bit word per wavefront (bit p = candidate word p): V = (V + (V & M)) | (V & ~M) with M the ballot of
//      the lanes whose word equals the reference word; the LCS is the number of zero bits among the low L.  Lengths, the
//      LCS and the closest reference length are wave-uniform and stay on the scalar unit;
//   4. the clipped counts of the four orders, each at most 64 per row, travel through one butterfly packed 8 bits apiece.
// Integers only, no atomics, no workspace; nothing is staged in HBM.  Every index is formed from the launch geometry or
// clamped to its array: offsets that are not monotone or not in range give empty references, never a read outside.
// Resource use (gfx950, the build's kernel-resource-usage remarks): 36 VGPRs, 76 SGPRs, no AGPRs, 816 bytes of static LDS,
// scratch 0, no spills, occupancy 8 waves per SIMD.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int MAXL = ACVAE_CONSENSUS_MAX_LENGTH;
constexpr int NORD = 4;
constexpr int REC = ACVAE_ACCURACY_RECORD;
static_assert(MAXL == 64, "one lane per word of a row, one bit per word of the LCS state");
static_assert(REC == 5 + NORD, "the record's layout");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint64_t order_mask(int k) { return k == 3 ? ~0ull : (1ull << (16 * (k + 1))) - 1ull; }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(64) void accuracy_stats_kernel(
    const int64_t* __restrict__ seqs, int64_t ld, int sample_n, int max_length, int start_idx, int end_idx, int V,
    const int* __restrict__ ref_words, int n_words, const int* __restrict__ ref_off, int n_refs,
    const int* __restrict__ clip_ref, int* __restrict__ record) {
  __shared__ int words[MAXL + NORD];            // the cleaned row, id + 1 (0xFFFF: outside [0, V)); 0 past its end
  __shared__ uint64_t key4[MAXL + 4];           // words p .. p+3 packed (id + 1) << 16 j; 0 where the n-gram cannot match
  const int lane = threadIdx.x;                 // the launch has exactly 64 threads per workgroup
  const int64_t r = blockIdx.x;
  const int64_t clip = r / sample_n;
  const int64_t* row = seqs + r * ld;

  // 1. clean the row: lanes past max_length count as <end>
  const int64_t tok = lane < max_length ? row[lane] : (int64_t)end_idx;
  const unsigned long long endm = __ballot(tok == (int64_t)end_idx);
  const int first_end = endm ? __ffsll(endm) - 1 : MAXL;
  const bool keep = lane < first_end && tok != (int64_t)start_idx;
  const unsigned long long km = __ballot(keep);
  const int L = __popcll(km);
  words[lane] = 0;
  if (lane < NORD) { words[MAXL + lane] = 0; key4[MAXL + lane] = 0; }
  __syncthreads();
  if (keep) {
    const bool inside = tok >= 0 && tok < (int64_t)V;         // (V <= 65534: id + 1 fits 16 bits below 0xFFFF)
    words[__popcll(km & ((1ull << lane) - 1ull))] = inside ? (int)tok + 1 : 0xFFFF;
  }
  __syncthreads();

  // 2. the n-grams that start at this lane's word; one that holds an out-of-range word is disqualified
  const int mine = words[lane];
  const int cw = mine == 0xFFFF ? 0 : mine;                   // for the LCS: 0 equals no reference word
  uint64_t k4 = 0;
  bool bad = false;
  uint64_t key[NORD];
#pragma unroll
  for (int j = 0; j < NORD; ++j) {
    const int w = words[lane + j];
    k4 |= (uint64_t)w << (16 * j);
    bad = bad || w == 0xFFFF;
    key[j] = (lane + j < L && !bad) ? k4 : 0;                 // (k4 so far is the key of order j; no real key is 0)
  }
  key4[lane] = k4;
  __syncthreads();

  // 3. counts within the row; an n-gram contributes at the lane of its first occurrence
  int cnt[NORD];
  bool lead[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) { cnt[k] = 0; lead[k] = key[k] != 0; }
  for (int p0 = 0; p0 < L; p0 += 4) {          // in chunks of four loads; a position past the row holds 0 and matches nothing
    uint64_t kp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) kp[u] = key4[p0 + u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < NORD; ++k) {
        const bool same = key[k] != 0 && (kp[u] & order_mask(k)) == key[k];
        cnt[k] += same ? 1 : 0;
        if (same && p0 + u < lane) lead[k] = false;
      }
  }

  // 4. the references of the clip, streamed
  const int j_lo = uniform(clampi(clip_ref[clip], 0, n_refs));
  const int j_hi = uniform(clampi(clip_ref[clip + 1], 0, n_refs));
  int most[NORD];
#pragma unroll
  for (int k = 0; k < NORD; ++k) most[k] = 0;
  int reflen = 0, refgap = 0x7fffffff, lcs_p = 0, lcs_r = 0, len_r = 0;
  const unsigned long long lowL = L >= 64 ? ~0ull : (1ull << L) - 1ull;
  for (int j = j_lo; j < j_hi; ++j) {
    const int lo = uniform(clampi(ref_off[j], 0, n_words));
    const int hi = uniform(clampi(ref_off[j + 1], 0, n_words));
    const int len = hi > lo ? hi - lo : 0;
    const int gap = len > L ? len - L : L - len;
    if (gap < refgap || (gap == refgap && len < reflen)) { refgap = gap; reflen = len; }
    int c[NORD];
#pragma unroll
    for (int k = 0; k < NORD; ++k) c[k] = 0;
    unsigned long long Vb = ~0ull;
    int nxt = 0;
    if (lane < len) { const int w = ref_words[lo + lane]; nxt = (w >= 0 && w < V) ? w + 1 : 0xFFFF; }
    for (int base = 0; base < len; base += 64) {
      const int cur = nxt;
      nxt = 0;
      if (base + 64 + lane < len) { const int w = ref_words[lo + base + 64 + lane]; nxt = (w >= 0 && w < V) ? w + 1 : 0xFFFF; }
      uint64_t rk4 = (uint64_t)cur;             // the four-word key of reference position base + lane (0 past the end)
#pragma unroll
      for (int jj = 1; jj < NORD; ++jj) {
        const int src = (lane + jj) & 63;
        const int a = __shfl(cur, src, 64), b = __shfl(nxt, src, 64);
        rk4 |= (uint64_t)(lane + jj < 64 ? a : b) << (16 * jj);
      }
      const unsigned rk_lo = (unsigned)rk4, rk_hi = (unsigned)(rk4 >> 32);
      const int m = len - base < 64 ? len - base : 64;
      for (int u = 0; u < m; ++u) {
        const uint64_t rk = (uint64_t)(unsigned)__builtin_amdgcn_readlane((int)rk_lo, u) |
                            ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)rk_hi, u) << 32);
#pragma unroll
        for (int k = 0; k < NORD; ++k) c[k] += (key[k] != 0 && (rk & order_mask(k)) == key[k]) ? 1 : 0;
        const unsigned long long M = __ballot(cw == (int)(rk & 0xFFFFull)) & lowL;     // (cw == 0 equals no reference word)
        Vb = (Vb + (Vb & M)) | (Vb & ~M);
      }
    }
#pragma unroll
    for (int k = 0; k < NORD; ++k) most[k] = c[k] > most[k] ? c[k] : most[k];
    const int lcs = __popcll(~Vb & lowL);
    lcs_p = lcs > lcs_p ? lcs : lcs_p;
    // the recall pair: the largest LCS / len by cross-multiplication (both factors < 2^31), ties to the earlier reference
    if (j == j_lo || (int64_t)lcs * len_r > (int64_t)lcs_r * len) { lcs_r = lcs; len_r = len; }
  }

  // 5. the clipped counts packed 8 bits per order (a row has at most 64 n-grams of an order)
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < NORD; ++k) packed |= (unsigned)(lead[k] ? (cnt[k] < most[k] ? cnt[k] : most[k]) : 0) << (8 * k);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
  if (lane == 0) {
    int* out = record + r * REC;
    out[0] = L;
    out[1] = reflen;
#pragma unroll
    for (int k = 0; k < NORD; ++k) out[2 + k] = (int)((packed >> (8 * k)) & 0xFFu);
    out[6] = lcs_p;
    out[7] = lcs_r;
    out[8] = len_r;
  }
}
}  // namespace

extern "C" int acvae_accuracy_stats(const int64_t* seqs, int64_t ld, int n, int sample_n, int max_length, int start_idx,
                                    int end_idx, int V, const int* ref_words, int n_words, const int* ref_off, int n_refs,
                                    const int* clip_ref, int n_clips, int* record, void* stream) {
  if (!seqs || !ref_words || !ref_off || !clip_ref || !record) return ACVAE_EINVAL;
  if (sample_n < 1 || sample_n > ACVAE_CONSENSUS_MAX_SAMPLES || n <= 0 || n % sample_n != 0) return ACVAE_EINVAL;
  if (max_length < 1 || max_length > ACVAE_CONSENSUS_MAX_LENGTH || ld < max_length) return ACVAE_EINVAL;
  if (V < 1 || V > 65534) return ACVAE_EINVAL;
  if (n_words < 0 || n_words > (1 << 30) || n_refs < 0 || n_clips != n / sample_n) return ACVAE_EINVAL;
  hipLaunchKernelGGL(accuracy_stats_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, seqs, ld, sample_n, max_length,
                     start_idx, end_idx, V, ref_words, n_words, ref_off, n_refs, clip_ref, record);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
