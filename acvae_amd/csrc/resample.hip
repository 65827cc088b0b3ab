// Band-limited sample-rate conversion (include/acvae_hip.h, acvae_resample_fwd): y[m] = sum_n x[n] g(m D / U - n), one
// kernel.  With m = j U + i (block j, phase i < U) the output of a clip is the product Y[j, i] = sum_k X[j, k] H[k, i] of
// the frame matrix X[j, k] = x[j D + k - W] (hop D, zero outside the clip) and the filter table H, on the exact-fp32 matrix
// pipe with the operand maps and the LDS row pitch of mfma_tile.h - the structure of the log-mel front end (frontend.hip)
// with another table and a zero rule in place of the reflect rule.  X exists only as the [64 x 32] piece of the current
// K-step in LDS, gathered from the waveform (coalesced along k).
//
// Workgroup = 256 threads = 4 wavefronts, BT = 64 consecutive blocks of one clip times ONE tile of 32 phases.  A phase
// tile has non-zero taps only over a band of k; the host stores just that band per tile (`bank`, its first k and its
// number of K-steps in `bank_index`), and the workgroup visits only those K-steps.  One tile per workgroup because the
// bands of neighbouring tiles are different windows of k: sharing a staged frame piece among them would mean staging the
// union of their bands, which is the work the band structure saves.  The four wavefronts are 2 (blocks) x 2 (halves of the
// K-step): wave (wm, wk) multiplies blocks wm*32.. by the k groups 16 wk .. 16 wk + 15 of every K-step; at the end the
// wk = 1 partial tiles go through LDS and wave (wm, 0) stores partial(wk = 0) + partial(wk = 1).
// LDS: two-stage ring of 9 KB (frames) + 4.5 KB (table) = 27 KB.
// Summation order is fixed: K-steps ascending inside each half, mfma_tile.h's k pairs inside a K-step, then the two
// halves.  No atomics.  Bit-reproducible.
#include "mfma_tile.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int BT = ACVAE_RESAMPLE_BLOCK_TILE;
constexpr int PT = 32;                    // phases per tile = one MFMA tile
constexpr int BK = mfma::BK;              // 32
constexpr int LD = mfma::LDS_LD;          // 36
constexpr int TH = 256;
static_assert(BT == 64 && BK == 32, "the wave grid and the loaders below are written for a 64 x 32 frame piece");
static_assert(2 * 16 * 64 <= BT * LD, "the two partial tiles live in one frame buffer");

struct alignas(16) Smem {
  float a[2][BT * LD];                    // frames [block][k]; after the last K-step a[0] carries the wk = 1 partials
  float b[2][PT * LD];                    // table [phase][k]
};

__device__ __forceinline__ float sample(const float* p) { return *p; }
__device__ __forceinline__ float sample(const short* p) { return (float)*p * (1.0f / 32768.0f); }

template <class S>
__global__ __launch_bounds__(TH, 2) void resample_kernel(const S* __restrict__ wave, long stride,
                                                         const int* __restrict__ lens, const float* __restrict__ bank,
                                                         const int* __restrict__ index, float* __restrict__ out,
                                                         long out_stride, int U, int D, int W, int ksteps, int ptiles,
                                                         int btiles) {
  __shared__ Smem sm;
  const int pt = blockIdx.x % ptiles;
  const int bt = (blockIdx.x / ptiles) % btiles, n = blockIdx.x / ptiles / btiles;
  const int j0 = bt * BT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wk = w & 1, li = lane & 31, lh = lane >> 5;
  int L = lens[n];
  L = L < 0 ? 0 : L;
  L = L < (int)stride ? L : (int)stride;
  long Lout = ((long)L * U + D - 1) / D;  // ceil(L U / D) outputs; behind them the row is zeros
  Lout = Lout < out_stride ? Lout : out_stride;
  float* outn = out + (long)n * out_stride;

  if ((long)j0 * U >= Lout) {             // the whole tile is padding (uniform over the workgroup)
    for (int e = tid; e < BT * PT; e += TH) {
      const int i = pt * PT + (e & 31);
      const long m = (long)(j0 + (e >> 5)) * U + i;
      if (i < U && m < out_stride) outn[m] = 0.f;
    }
    return;
  }

  const S* wv = wave + (long)n * stride;
  const int kfirst = index[2 * pt];
  int nk = index[2 * pt + 1];             // the table is the caller's: never step outside this tile's part of `bank`
  nk = nk < 0 ? 0 : (nk < ksteps ? nk : ksteps);
  const float* bankt = bank + (long)pt * ksteps * (PT * BK);
  const int ak = tid & 31, arow = tid >> 5;             // frame loader: column k, blocks arow + 8 j
  const int brow = tid >> 3, bc4 = (tid & 7) * 4;       // table loader: float4 column of phase brow

  S va[8];
  unsigned amask;
  float4 vb;
  // issue: addresses (always legal) and loads only; stash: masks and conversion, just before the LDS stores
  auto issue = [&](int it) {
    const int k = kfirst + it * BK + ak - W;
    amask = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int jb = j0 + arow + 8 * j;
      const bool live = (long)jb * U < Lout;            // a block with outputs: then jb D < L + D, inside 32 bits
      long s = (long)(live ? jb : 0) * D + k;
      const bool ok = live && s >= 0 && s < L;          // x is zero outside [0, L)
      s = ok ? s : 0;
      va[j] = wv[s];
      amask |= (ok ? 1u : 0u) << j;
    }
    vb = *reinterpret_cast<const float4*>(bankt + (long)it * (PT * BK) + brow * BK + bc4);
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      sm.a[buf][(arow + 8 * j) * LD + ak] = ((amask >> j) & 1u) ? sample(&va[j]) : 0.f;
    *reinterpret_cast<float4*>(&sm.b[buf][brow * LD + bc4]) = vb;
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  if (nk > 0) {
    issue(0);
    stash(0);
  }
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int cur = it & 1;
    if (it + 1 < nk) issue(it + 1);
    const float* As = sm.a[cur] + (wm * 32 + li) * LD + 4 * lh + 16 * wk;
    const float* Bs = sm.b[cur] + li * LD + 4 * lh + 16 * wk;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const float4 af = *reinterpret_cast<const float4*>(As + 8 * g);
      const float4 bf = *reinterpret_cast<const float4*>(Bs + 8 * g);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc, 0, 0, 0);
    }
    if (it + 1 < nk) stash(cur ^ 1);
    __syncthreads();                      // everyone is done reading ring slot `cur`; slot cur^1 is complete
  }

  // ---- the two halves of the K-steps meet: partial(wk = 1) -> LDS -> wave (wm, 0), which stores every output once
  float* red = sm.a[0] + wm * (16 * 64);
  if (wk == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[r * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wk == 1) return;
  const int i = pt * PT + li;
  if (i >= U) return;                     // a zero column behind the last phase
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    const long m = (long)(j0 + row) * U + i;
    if (m < out_stride) outn[m] = m < Lout ? acc[r] + red[r * 64 + lane] : 0.f;
  }
}
}  // namespace

extern "C" int acvae_resample_fwd(const void* wave, int wave_is_i16, int64_t wave_stride, const int* wave_lens,
                                  const float* bank, const int* bank_index, float* out, int64_t out_stride, int N, int U,
                                  int D, int W, int ksteps, void* stream) {
  if (!wave || !wave_lens || !bank || !bank_index || !out || N <= 0 || (wave_is_i16 != 0 && wave_is_i16 != 1))
    return ACVAE_EINVAL;
  if (U < 1 || U > ACVAE_RESAMPLE_MAX_RATIO || D < 1 || D > ACVAE_RESAMPLE_MAX_RATIO || U == D) return ACVAE_EINVAL;
  if (W < 1 || 2 * (int64_t)W > ACVAE_RESAMPLE_MAX_TAPS) return ACVAE_EINVAL;
  if (ksteps < 1 || ksteps > ACVAE_RESAMPLE_MAX_KSTEPS) return ACVAE_EINVAL;
  if (wave_stride < 1 || wave_stride > ((int64_t)1 << 30) || out_stride < 1) return ACVAE_EINVAL;
  if ((int64_t)N * out_stride >= ((int64_t)1 << 31)) return ACVAE_EINVAL;
  const int ptiles = (U + PT - 1) / PT;
  const int64_t blocks = (out_stride + U - 1) / U;
  const int64_t btiles = (blocks + BT - 1) / BT;
  if ((int64_t)N * btiles * ptiles >= ((int64_t)1 << 31)) return ACVAE_EINVAL;
  if (!aligned16(bank)) return ACVAE_EALIGN;
  const dim3 grid((unsigned)(N * btiles * ptiles)), block(TH);
  if (wave_is_i16)
    hipLaunchKernelGGL(resample_kernel<short>, grid, block, 0, (hipStream_t)stream, (const short*)wave, (long)wave_stride,
                       wave_lens, bank, bank_index, out, (long)out_stride, U, D, W, ksteps, ptiles, (int)btiles);
  else
    hipLaunchKernelGGL(resample_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)wave, (long)wave_stride,
                       wave_lens, bank, bank_index, out, (long)out_stride, U, D, W, ksteps, ptiles, (int)btiles);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
