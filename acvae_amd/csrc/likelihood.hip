// Scoring given captions on the device: per-step log-probability, rank and KL of teacher-forced outputs, and their per-row
// sums (include/acvae_hip.h has the definitions, acvae_amd/likelihood.py the front).
//
// acvae_caption_terms - the mapping and why.  The work is a row reduction per cell (r, t): V logits (20 KB at V = 5000) and
// 4 x E floats of the two Gaussians (8 KB at E = 512), read once, three numbers out; R * T * V * 4 bytes in all (67 MB at
// 160 x 21 x 5000), so the kernel is bound by memory traffic and what matters is the number of 16-byte loads in flight.
//   One WORKGROUP of 256 lanes per cell, as the neighbouring row kernels of csrc/losses.hip.  A wavefront per cell would
//   save the two barriers, but a row is 20 iterations of 1 KB per wavefront and the evaluation batches are small: at
//   R = 32 there are 672 cells, less than one wavefront for each of the chip's 1024 SIMDs, and nothing would hide the
//   latency of a row's serial loads.  A workgroup per cell puts 4 wavefronts on each row (2688 at R = 32, 13440 at R = 160)
//   and every lane's share of the row is at most five 16-byte loads at V = 5000, issued four at a time before any is used.
//   The work of a workgroup is V + 4 E elements whatever R and T are.
//   The row is read ONCE: each lane keeps a running maximum and a sum of exp(x - maximum) that is rescaled when the maximum
//   moves (one extra exp per group of four elements); the lanes' pairs are merged against the workgroup's maximum, so the
//   log-sum-exp is max-subtracted throughout.  The target's logit is one broadcast load in front of the pass; the two
//   counters of the rank compare every element with it as it goes by.
//   No atomics, no workspace, no scratch; 112 bytes of LDS for the two reductions.  Every sum has a fixed order: a lane's
//   elements ascending, the lanes of a wavefront through the xor butterfly, the wavefronts ascending.
#include <limits.h>

#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int CT = 256;                    // lanes per cell
constexpr int NW = CT / 64;

struct RowAcc {                            // one lane's share of a row
  float m, s;                              // running maximum, sum of exp(x - m) (0 while m is -inf)
  int gt, eq;                              // elements above the target's logit; elements equal to it in front of the target
  int nan;                                 // NaN elements, told by their bits (a row that holds one has no log-probability)
};

__device__ __forceinline__ int is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u ? 1 : 0; }

__device__ __forceinline__ void take1(RowAcc& a, float v, int idx, float xt, int tg) {
  a.gt += v > xt ? 1 : 0;
  a.eq += (v == xt && idx < tg) ? 1 : 0;
  a.nan += is_nan_bits(v);
  if (v > a.m) {                           // (m = -inf: s is 0 and stays 0 under the rescale)
    a.s = a.s * expf(a.m - v) + 1.f;
    a.m = v;
  } else if (v != -INFINITY) {             // a word of mass 0 adds nothing (and -inf - -inf has no value)
    a.s += expf(v - a.m);
  }
}

__device__ __forceinline__ void take4(RowAcc& a, float4 v, int idx, float xt, int tg) {
  a.gt += (v.x > xt ? 1 : 0) + (v.y > xt ? 1 : 0) + (v.z > xt ? 1 : 0) + (v.w > xt ? 1 : 0);
  a.eq += ((v.x == xt && idx < tg) ? 1 : 0) + ((v.y == xt && idx + 1 < tg) ? 1 : 0) + ((v.z == xt && idx + 2 < tg) ? 1 : 0) +
          ((v.w == xt && idx + 3 < tg) ? 1 : 0);
  a.nan += is_nan_bits(v.x) + is_nan_bits(v.y) + is_nan_bits(v.z) + is_nan_bits(v.w);
  const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
  const float mn = fmaxf(a.m, m4);
  if (mn == -INFINITY) return;             // nothing but words of mass 0 so far
  if (mn > a.m) { a.s *= expf(a.m - mn); a.m = mn; }
  a.s += expf(v.x - mn) + expf(v.y - mn) + expf(v.z - mn) + expf(v.w - mn);
}

// Normal_kl_loss's term (csrc/losses.hip: kl_elem), evaluated in float64: a term is typically a few hundredths, left over
// from summands of magnitude 1/2 that cancel, so in fp32 each of the E terms would carry a rounding of that magnitude,
// more than the Gaussians themselves do (profiles/r19_likelihood.txt, section 4).  The cell is rounded to fp32 once, at the
// store.  2 E exponentials per cell beside the V of the row: not what the kernel's time is made of.
__device__ __forceinline__ double kl_term(float mu1, float lv1, float mu2, float lv2) {
  const double d = (double)mu1 - (double)mu2;
  return (double)lv2 * .5 - (double)lv1 * .5 + (exp((double)lv1) + d * d) / (2. * exp((double)lv2)) - .5;
}

__global__ __launch_bounds__(CT) void caption_terms_kernel(
    const float* __restrict__ logits, long ld_n, long ld_t, const int64_t* __restrict__ targets, long tg_sn,
    const int64_t* __restrict__ lens1, const float* __restrict__ q_means, const float* __restrict__ q_logs,
    const float* __restrict__ p_means, const float* __restrict__ p_logs, float* __restrict__ logprob,
    int32_t* __restrict__ rank, float* __restrict__ kl, int T, int V, int E, int vec_v, int vec_e) {
  __shared__ double red_k[NW];
  __shared__ float red_m[NW], red_s[NW];
  __shared__ int red_gt[NW], red_eq[NW], red_nan[NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long cell = blockIdx.x;
  const long r = cell / T;
  const int t = (int)(cell % T);
  const bool want_kl = q_means != nullptr;              // (the host passes all four or none)
  if (lens1 && (int64_t)t >= lens1[r]) {                // an invalid cell: exact zeros, nothing is read
    if (tid == 0) {
      logprob[cell] = 0.f;
      rank[cell] = 0;
      if (kl) kl[cell] = 0.f;
    }
    return;
  }
  const float* x = logits + r * ld_n + t * ld_t;
  const int64_t tg64 = targets[r * tg_sn + t];
  const bool inside = tg64 >= 0 && tg64 < (int64_t)V;
  const int tg = inside ? (int)tg64 : 0;                // a target outside [0, V) reads x[0]; its outputs are overwritten
  const float xt = x[tg];

  RowAcc a = {-INFINITY, 0.f, 0, 0, 0};
  if (vec_v) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const int n4 = V >> 2;
    int c = tid;
    for (; c + 3 * CT < n4; c += 4 * CT) {              // four loads in flight per lane
      const float4 v0 = x4[c], v1 = x4[c + CT], v2 = x4[c + 2 * CT], v3 = x4[c + 3 * CT];
      take4(a, v0, 4 * c, xt, tg);
      take4(a, v1, 4 * (c + CT), xt, tg);
      take4(a, v2, 4 * (c + 2 * CT), xt, tg);
      take4(a, v3, 4 * (c + 3 * CT), xt, tg);
    }
    for (; c < n4; c += CT) take4(a, x4[c], 4 * c, xt, tg);
    for (int i = (n4 << 2) + tid; i < V; i += CT) take1(a, x[i], i, xt, tg);
  } else {
    for (int i = tid; i < V; i += CT) take1(a, x[i], i, xt, tg);
  }

  double k = 0.0;
  if (want_kl) {
    const long o = cell * (long)E;
    if (vec_e) {
      const float4 *m1 = reinterpret_cast<const float4*>(q_means + o), *l1 = reinterpret_cast<const float4*>(q_logs + o);
      const float4 *m2 = reinterpret_cast<const float4*>(p_means + o), *l2 = reinterpret_cast<const float4*>(p_logs + o);
      for (int c = tid; c < (E >> 2); c += CT) {
        const float4 a1 = m1[c], b1 = l1[c], a2 = m2[c], b2 = l2[c];
        k += kl_term(a1.x, b1.x, a2.x, b2.x) + kl_term(a1.y, b1.y, a2.y, b2.y) + kl_term(a1.z, b1.z, a2.z, b2.z) +
             kl_term(a1.w, b1.w, a2.w, b2.w);
      }
    } else {
      for (int i = tid; i < E; i += CT) k += kl_term(q_means[o + i], q_logs[o + i], p_means[o + i], p_logs[o + i]);
    }
  }

  // the workgroup's maximum first, then every lane's sum against it
  const float wm = wave_max(a.m);
  if (lane == 0) red_m[w] = wm;
  __syncthreads();
  float M = red_m[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) M = fmaxf(M, red_m[i]);
  float s = a.m == -INFINITY ? 0.f : a.s * expf(a.m - M);
  s = wave_sum(s);
  k = wave_sum_d(k);
  int gt = a.gt, eq = a.eq, nn = a.nan;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    gt += __shfl_xor(gt, o, 64);
    eq += __shfl_xor(eq, o, 64);
    nn += __shfl_xor(nn, o, 64);
  }
  if (lane == 0) { red_s[w] = s; red_k[w] = k; red_gt[w] = gt; red_eq[w] = eq; red_nan[w] = nn; }
  __syncthreads();
  if (tid == 0) {
    float S = 0.f;
    double K = 0.0;
    int G = 0, Q = 0, N = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { S += red_s[i]; K += red_k[i]; G += red_gt[i]; Q += red_eq[i]; N += red_nan[i]; }
    logprob[cell] = inside && N == 0 ? (xt - M) - logf(S) : __int_as_float(0x7fc00000);
    rank[cell] = inside && xt == xt ? G + Q : INT_MAX;   // (a NaN target logit compares with nothing: no hit)
    if (kl) kl[cell] = want_kl ? (float)K : 0.f;
  }
}

// One lane per row: the sums run over t ascending in float64, exactly as a host loop over the same cells would.
__global__ __launch_bounds__(64) void caption_sums_kernel(const float* __restrict__ logprob, const int32_t* __restrict__ rank,
                                                          const float* __restrict__ kl, const int64_t* __restrict__ lens1,
                                                          double* __restrict__ nll, double* __restrict__ kl_sum,
                                                          int32_t* __restrict__ tokens, int32_t* __restrict__ hit1,
                                                          int32_t* __restrict__ hit5, int R, int T) {
  const long r = blockIdx.x * 64L + threadIdx.x;
  if (r >= R) return;
  int64_t n = lens1 ? lens1[r] : (int64_t)T;
  n = n < 0 ? 0 : (n > T ? T : n);
  double a = 0.0, b = 0.0;
  int h1 = 0, h5 = 0;
  for (int t = 0; t < (int)n; ++t) {
    const long o = r * T + t;
    a += -(double)logprob[o];
    if (kl) b += (double)kl[o];
    const int k = rank[o];
    h1 += k < 1 ? 1 : 0;
    h5 += k < 5 ? 1 : 0;
  }
  nll[r] = a;
  kl_sum[r] = b;
  tokens[r] = (int)n;
  hit1[r] = h1;
  hit5[r] = h5;
}
}  // namespace

extern "C" int acvae_caption_terms(const float* logits, int64_t ld_n, int64_t ld_t, const int64_t* targets, int64_t tg_sn,
                                   const int64_t* lens1, const float* q_means, const float* q_logs, const float* p_means,
                                   const float* p_logs, float* logprob, int32_t* rank, float* kl, int R, int T, int V, int E,
                                   void* stream) {
  if (!logits || !targets || !logprob || !rank) return ACVAE_EINVAL;
  if (R <= 0 || T <= 0 || V < 2 || E < 0 || (int64_t)R * T > INT_MAX) return ACVAE_EINVAL;
  if (ld_n < 0 || ld_t < 0 || tg_sn < 0) return ACVAE_EINVAL;
  const bool want_kl = q_means && q_logs && p_means && p_logs;
  if (want_kl && (E < 1 || !kl)) return ACVAE_EINVAL;
  const int vec_v = aligned16(logits) && ld_n % 4 == 0 && ld_t % 4 == 0;
  const int vec_e = want_kl && E % 4 == 0 && aligned16(q_means) && aligned16(q_logs) && aligned16(p_means) && aligned16(p_logs);
  hipLaunchKernelGGL(caption_terms_kernel, dim3(R * T), dim3(CT), 0, (hipStream_t)stream, logits, ld_n, ld_t, targets, tg_sn,
                     lens1, want_kl ? q_means : nullptr, q_logs, p_means, p_logs, logprob, rank, kl, T, V, E, vec_v, vec_e);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_caption_sums(const float* logprob, const int32_t* rank, const float* kl, const int64_t* lens1, double* nll,
                                  double* kl_sum, int32_t* tokens, int32_t* hit1, int32_t* hit5, int R, int T, void* stream) {
  if (!logprob || !rank || !nll || !kl_sum || !tokens || !hit1 || !hit5) return ACVAE_EINVAL;
  if (R <= 0 || T <= 0 || (int64_t)R * T > INT_MAX) return ACVAE_EINVAL;
  hipLaunchKernelGGL(caption_sums_kernel, dim3(cdiv(R, 64)), dim3(64), 0, (hipStream_t)stream, logprob, rank, kl, lens1, nll,
                     kl_sum, tokens, hit1, hit5, R, T);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
