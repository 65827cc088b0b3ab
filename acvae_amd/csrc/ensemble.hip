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
#include "common.h"
#include "job_table.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int MIX_THREADS = 256;       // row_stats_kernel's EW_THREADS: the identity above needs the same stride
constexpr int MIX_WAVES = MIX_THREADS / 64;

struct MixJob { const float* logits; long ld; };
using MixTable = acvae::JobTable<MixJob, ACVAE_ENSEMBLE_MAX>;

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
  float lse[M];
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

  // ---- pass 3: the mixture's scores, and their first maximum
  const float pv = prev ? prev[r] : 0.f;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < V; c += MIX_THREADS) {
    float lp[M];
    float a = -INFINITY;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      lp[m] = x[m][c] - lse[m];
      a = fmaxf(a, lp[m]);
    }
    float v = a;                                         // every member at -inf: the mixture is -inf, not inf - inf
    if (a > -INFINITY) {
      float s = 0.f;
#pragma unroll
      for (int m = 0; m < M; ++m) s += expf(lp[m] - a);
      v = a + logf(s / (float)M);
    }
    v = v + pv;
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

template <int M>
void launch_mix(const MixTable& tab, const float* prev, float* out, long ld_out, int64_t* argmax, float* best, long o_stride,
                int R, int V, hipStream_t st) {
  hipLaunchKernelGGL(ensemble_mix_kernel<M>, dim3((unsigned)R), dim3(MIX_THREADS), 0, st, tab, prev, out, ld_out, argmax, best,
                     o_stride, V);
}
}  // namespace

extern "C" int acvae_ensemble_mix(const float* const* logits, const int64_t* ld, int M, const float* prev, float* out,
                                  int64_t ld_out, int64_t* argmax, float* best, int64_t o_stride, int R, int V,
                                  void* stream) {
  if (!logits || !ld || M < 1 || M > ACVAE_ENSEMBLE_MAX || R <= 0 || V <= 0) return ACVAE_EINVAL;
  if (!out && !argmax && !best) return ACVAE_EINVAL;
  if ((out && ld_out < V) || ((argmax || best) && o_stride < 1)) return ACVAE_EINVAL;
  MixTable tab;
  for (int m = 0; m < M; ++m) {
    if (!logits[m] || ld[m] < V) return ACVAE_EINVAL;
    tab.add({logits[m], (long)ld[m]});
  }
  if (!tab.ok()) return ACVAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  switch (M) {
    case 1: launch_mix<1>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    case 2: launch_mix<2>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    case 3: launch_mix<3>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    case 4: launch_mix<4>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    case 5: launch_mix<5>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    case 6: launch_mix<6>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    case 7: launch_mix<7>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
    default: launch_mix<8>(tab, prev, out, ld_out, argmax, best, o_stride, R, V, st); break;
  }
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
