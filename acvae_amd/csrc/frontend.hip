// Log-mel front end (include/acvae_hip.h, acvae_logmel_fwd): waveform -> reflect-padded frames -> windowed DFT -> power
// -> mel -> dB, one kernel.  The DFT is a GEMM [frames x n_fft] . [n_fft x n_fft] on the exact-fp32 matrix pipe with the
// operand maps and the LDS row pitch of mfma_tile.h; its left operand, the frame matrix, exists only as the [64 x 32] piece
// of the current K-step in LDS, gathered from the waveform (coalesced along k, reflect rule at the clip's two ends).
//
// Workgroup = 256 threads = 4 wavefronts as 2 (frames) x 2 (frequencies), FT = 64 frames of one clip.  For each chunk of
// 64 frequencies (128 basis columns: 64 real, 64 imaginary) wave (wm, wn) accumulates the real and the imaginary 32 x 32
// tile of frames wm*32.. and bins wn*32.., so re and im of a cell meet in one lane; after the chunk's last K-step it squares
// and adds them, writes the power tile into LDS (over the basis buffer it has just consumed) and adds its product with the
// chunk's 64 rows of the mel weights (fragments straight from global / L2) to the mel accumulators, which stay in registers
// to the end: wave (wm, wn) owns frames wm*32.. and the mel columns of tiles wn and wn + 2.  The Nyquist bin travels in the
// column of bin 0's (zero) imaginary part; its mel term is added on the vector unit in the final epilogue.
// LDS: two-stage ring of 18 KB (frames) + 36 KB (basis) = 54 KB, the same for every hop -> two workgroups per CU.
// Summation order is fixed: K-steps ascending; inside a 32-wide K-step the MFMAs take the k pairs (8g + e, 8g + 4 + e) for
// g = 0..3, e = 0..3 (mfma_tile.h's permutation of the summation index, not ascending k); chunks ascending in the mel sum.
// Bit-reproducible.
#include "mfma_tile.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int FT = ACVAE_LOGMEL_FRAME_TILE;
constexpr int FC = 64;                    // frequencies per chunk
constexpr int BK = mfma::BK;              // 32
constexpr int LD = mfma::LDS_LD;          // 36: conflict-free ds_read_b128 over 16 consecutive rows
constexpr int PLD = FC + 4;               // row pitch of the power tile (68 = 4 mod 64: the same property)
constexpr int TH = 256;
static_assert(FT == 64 && BK == 32, "the wave grid and the loaders below are written for a 64 x 32 frame piece");
static_assert(FT * PLD <= 2 * FC * LD, "the power tile lives in one basis buffer");

struct alignas(16) Smem {
  float a[2][FT * LD];                    // frames [row][k]
  float b[2][2 * FC * LD];                // basis [column][k]; the consumed one doubles as the power tile [row][PLD]
  float nyq[FT];                          // power of the Nyquist bin per frame
};

__device__ __forceinline__ float sample(const float* p, int i) { return p[i]; }
__device__ __forceinline__ float sample(const short* p, int i) { return (float)p[i] * (1.0f / 32768.0f); }

template <class S>
__global__ __launch_bounds__(TH, 2) void logmel_kernel(const S* __restrict__ wave, long stride,
                                                       const int* __restrict__ lens, const float* __restrict__ basis,
                                                       const float* __restrict__ melw, float* __restrict__ out,
                                                       float* __restrict__ spec, int T, int n_fft, int hop, int n_mels,
                                                       float amin, float db_offset, int tiles) {
  __shared__ Smem sm;
  const int n = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * FT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1, li = lane & 31, lh = lane >> 5;
  const int half = n_fft >> 1, nb = half + 1;
  int L = lens[n];
  L = L < (int)stride ? L : (int)stride;
  int Tn = L >= nb ? 1 + L / hop : 0;     // frames of this clip; a clip too short to reflect has none
  Tn = Tn < T ? Tn : T;
  float* outn = out + (long)n * T * n_mels;
  float* specn = spec ? spec + (long)n * T * nb : nullptr;

  if (t0 >= Tn) {                         // the whole tile is padding (uniform over the workgroup)
    const int rows = (T - t0) < FT ? (T - t0) : FT;
    for (int i = tid; i < rows * n_mels; i += TH) outn[(long)t0 * n_mels + i] = 0.f;
    if (specn)
      for (int i = tid; i < rows * nb; i += TH) specn[(long)t0 * nb + i] = 0.f;
    return;
  }

  const S* wv = wave + (long)n * stride;
  const int nk = n_fft / BK, nchunks = half / FC, total = nk * nchunks;
  const int ak = tid & 31, arow = tid >> 5;             // frame loader: column k, rows arow + 8 j
  const int brow = tid >> 3, bc4 = (tid & 7) * 4;       // basis loader: float4 column, rows brow + 32 j

  S va[8];
  unsigned amask;
  float4 vb[4];
  // issue: addresses (always legal) and loads only; stash: masks and conversion, just before the LDS stores
  auto issue = [&](int it) {
    const int k0 = (it % nk) * BK;
    amask = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = t0 + arow + 8 * j;
      int s = t * hop + k0 + ak - half;
      s = s < 0 ? -s : s;
      s = s >= L ? 2 * (L - 1) - s : s;
      const bool ok = t < Tn;
      s = (ok && s >= 0 && s < L) ? s : 0;              // (a valid frame never needs the clamp: L >= n_fft/2 + 1)
      va[j] = wv[s];
      amask |= (ok ? 1u : 0u) << j;
    }
    const float* bp = basis + (long)it * (2 * FC * BK);  // chunk-major, K-step inside: exactly the iteration order
#pragma unroll
    for (int j = 0; j < 4; ++j) vb[j] = *reinterpret_cast<const float4*>(bp + (brow + 32 * j) * BK + bc4);
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      sm.a[buf][(arow + 8 * j) * LD + ak] = ((amask >> j) & 1u) ? sample(&va[j], 0) : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(&sm.b[buf][(brow + 32 * j) * LD + bc4]) = vb[j];
  };

  f32x16 re, im, macc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; macc[0][r] = 0.f; macc[1][r] = 0.f; }

  issue(0);
  stash(0);
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    if (it + 1 < total) issue(it + 1);
    const float* As = sm.a[cur] + (wm * 32 + li) * LD + 4 * lh;
    const float* Br = sm.b[cur] + (wn * 32 + li) * LD + 4 * lh;
    const float* Bi = Br + FC * LD;
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) {
      const float4 af = *reinterpret_cast<const float4*>(As + 8 * g);
      const float4 br = *reinterpret_cast<const float4*>(Br + 8 * g);
      const float4 bi = *reinterpret_cast<const float4*>(Bi + 8 * g);
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, br.x, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bi.x, im, 0, 0, 0);
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, br.y, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bi.y, im, 0, 0, 0);
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, br.z, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bi.z, im, 0, 0, 0);
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, br.w, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bi.w, im, 0, 0, 0);
    }
    if (it + 1 < total) stash(cur ^ 1);
    __syncthreads();                      // everyone is done reading ring slot `cur`; slot cur^1 is complete
    if ((it + 1) % nk != 0) continue;

    // ---- end of a frequency chunk: power tile -> LDS (slot `cur`'s basis buffer) -> mel accumulators
    const int q = it / nk;
    float* P = sm.b[cur];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int t = t0 + row;
      float p = re[r] * re[r] + im[r] * im[r];
      if (q == 0 && wn == 0 && li == 0) {   // bin 0 has no imaginary part: that column carried the Nyquist bin
        const float pn = im[r] * im[r];
        p = re[r] * re[r];
        sm.nyq[row] = pn;
        if (specn && t < T) specn[(long)t * nb + half] = pn;
      }
      P[row * PLD + wn * 32 + li] = p;
      if (specn && t < T) specn[(long)t * nb + q * FC + wn * 32 + li] = p;   // frames >= Tn were staged as zeros: p = 0
      re[r] = 0.f;
      im[r] = 0.f;
    }
    __syncthreads();
    const float* Ps = P + (wm * 32 + li) * PLD + 4 * lh;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = (wn + 2 * c) * 32 + li;
      if ((wn + 2 * c) * 32 >= n_mels) continue;          // uniform over the wave
      const bool cok = col < n_mels;
      const float* wp = melw + (long)(q * FC + 4 * lh) * n_mels + (cok ? col : 0);
      float bw[32];
#pragma unroll
      for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) bw[4 * g + e] = wp[(long)(8 * g + e) * n_mels];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float4 pf = *reinterpret_cast<const float4*>(Ps + 8 * g);
        macc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf.x, cok ? bw[4 * g + 0] : 0.f, macc[c], 0, 0, 0);
        macc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf.y, cok ? bw[4 * g + 1] : 0.f, macc[c], 0, 0, 0);
        macc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf.z, cok ? bw[4 * g + 2] : 0.f, macc[c], 0, 0, 0);
        macc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf.w, cok ? bw[4 * g + 3] : 0.f, macc[c], 0, 0, 0);
      }
    }
    __syncthreads();                      // the next K-step's stash overwrites the power tile
  }

  // ---- final epilogue: Nyquist term, dB, the single store of `out`
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int col = (wn + 2 * c) * 32 + li;
    if (col >= n_mels) continue;
    const float wny = melw[(long)half * n_mels + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int t = t0 + row;
      if (t >= T) continue;
      const float m = macc[c][r] + sm.nyq[row] * wny;
      outn[(long)t * n_mels + col] = t < Tn ? 10.f * log10f(fmaxf(m, amin)) - db_offset : 0.f;
    }
  }
}
}  // namespace

extern "C" int acvae_logmel_fwd(const void* wave, int wave_is_i16, int64_t wave_stride, const int* wave_lens,
                                const float* basis, const float* melw, float* out, float* spec, int N, int T, int n_fft,
                                int hop, int n_mels, float amin, float db_offset, void* stream) {
  if (!wave || !wave_lens || !basis || !melw || !out || N <= 0 || T <= 0 || (wave_is_i16 != 0 && wave_is_i16 != 1))
    return ACVAE_EINVAL;
  if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048) return ACVAE_EINVAL;
  if (hop < 1 || hop > n_fft || n_mels < 4 || n_mels > 128 || (n_mels & 3) != 0) return ACVAE_EINVAL;
  if (!(amin > 0.f) || !(amin <= 3.0e38f) || !(db_offset == db_offset)) return ACVAE_EINVAL;
  const int nb = n_fft / 2 + 1;
  if (wave_stride < nb || wave_stride > ((int64_t)1 << 30) || (int64_t)(T - 1) * hop > wave_stride) return ACVAE_EINVAL;
  if ((int64_t)N * T * nb >= ((int64_t)1 << 31)) return ACVAE_EINVAL;
  const int tiles = (T + FT - 1) / FT;
  if ((int64_t)N * tiles >= ((int64_t)1 << 31)) return ACVAE_EINVAL;
  if (!aligned16(basis)) return ACVAE_EALIGN;
  const dim3 grid((unsigned)(N * tiles)), block(TH);
  if (wave_is_i16)
    hipLaunchKernelGGL(logmel_kernel<short>, grid, block, 0, (hipStream_t)stream, (const short*)wave, (long)wave_stride,
                       wave_lens, basis, melw, out, spec, T, n_fft, hop, n_mels, amin, db_offset, tiles);
  else
    hipLaunchKernelGGL(logmel_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)wave, (long)wave_stride,
                       wave_lens, basis, melw, out, spec, T, n_fft, hop, n_mels, amin, db_offset, tiles);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
