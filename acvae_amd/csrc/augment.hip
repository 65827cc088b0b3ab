// Training-time augmentation on the uploaded batch: datasets/augment.py time_roll (np.roll along time) followed by
// spec_augment's time masks and frequency masks, each mask filled with the mean of the clip as it stands just before it.
// The random draws are made on the host (acvae_amd/augment.py); this kernel applies the table they produced.
//
// One workgroup per clip, no workspace and no cross-workgroup hand-off.  The fill of mask k needs the clip's sum just
// before it, S_k; instead of materialising the clip after every mask, the kernel keeps
//     S_{k+1} = S_k - (current sum over region k) + |region k| * fill_k
// where the current value of a cell in region k is the fill of the latest earlier mask that covers it, else the rolled
// input.  Every pass reads only `in`, never what the kernel wrote.  Sums are fp64 in a fixed order (per-thread strided
// partials, butterfly, then waves in order): bit-reproducible run to run.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int TH = 1024;
constexpr int NW = TH / 64;
constexpr int MAXM = 2 * ACVAE_AUG_MAX_MASKS;
constexpr int U = 8;                     // loads in flight per lane: one workgroup streams a whole clip, so the
                                         // passes are latency-bound unless each lane issues several loads at once

struct Masks {                           // one clip's masks after clamping: time masks [0, nt), freq masks [nt, m)
  int r0[MAXM], r1[MAXM], c0[MAXM], c1[MAXM];
  float fill[MAXM];
  int nt, m;
  // colm[j]: the latest frequency mask processed so far that covers column j, or -1 (no search per cell)
  alignas(4) signed char colm[ACVAE_AUG_MAX_F];
};

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();                       // `red` may still be read by the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += red[w];
  return t;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// Input row of output row i under the roll by s (0 <= i < L, 0 <= s < L).
__device__ __forceinline__ int src_row(int i, int s, int L) { return i >= s ? i - s : i - s + L; }

// Latest time mask with index < kend that covers row i, or -1.  A fixed-length loop without early exit: its LDS reads
// issue together instead of one dependent read per mask.
__device__ __forceinline__ int time_cover(const Masks& M, int i, int kend) {
  int best = -1;
#pragma unroll
  for (int m = 0; m < ACVAE_AUG_MAX_MASKS; ++m)
    if (m < kend && M.r0[m] <= i && i < M.r1[m]) best = m;
  return best;
}

__global__ __launch_bounds__(TH) void spec_augment_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          const int* __restrict__ lens, const int* __restrict__ params,
                                                          int T, int F) {
  __shared__ Masks M;
  __shared__ double red[NW];
  __shared__ double S;
  __shared__ int L_s, shift_s;
  const int n = blockIdx.x;
  const int F4 = F >> 2;
  const long base = (long)n * T * F;
  const float4* in4 = reinterpret_cast<const float4*>(in + base);
  float4* out4 = reinterpret_cast<float4*>(out + base);

  if (threadIdx.x == 0) {
    const int* row = params + (long)n * ACVAE_AUG_TABLE_WIDTH;
    const int L = clampi(lens[n], 0, T);
    int s = 0;
    if (L > 0) {
      s = row[0] % L;
      if (s < 0) s += L;
    }
    const int nt = L > 0 ? clampi(row[1], 0, ACVAE_AUG_MAX_MASKS) : 0;
    const int nf = L > 0 ? clampi(row[2], 0, ACVAE_AUG_MAX_MASKS) : 0;
    for (int k = 0; k < nt; ++k) {
      const int a = clampi(row[3 + 2 * k], 0, L);
      M.r0[k] = a; M.r1[k] = clampi(row[4 + 2 * k], a, L); M.c0[k] = 0; M.c1[k] = F;
    }
    for (int k = 0; k < nf; ++k) {
      const int* f = row + 3 + 2 * ACVAE_AUG_MAX_MASKS + 2 * k;
      const int a = clampi(f[0], 0, F);
      M.r0[nt + k] = 0; M.r1[nt + k] = L; M.c0[nt + k] = a; M.c1[nt + k] = clampi(f[1], a, F);
    }
    for (int k = nt + nf; k < MAXM; ++k) { M.r0[k] = M.r1[k] = M.c0[k] = M.c1[k] = 0; }
    M.nt = nt; M.m = nt + nf;
    L_s = L; shift_s = s;
  }
  for (int j = threadIdx.x; j < F; j += TH) M.colm[j] = -1;
  __syncthreads();
  const int L = L_s, s = shift_s, nm = M.m, nt = M.nt;
  const int n4 = L * F4;            // in-clip indices are int: T * F < 2^31

  if (nm > 0) {
    // pass 1: the clip's sum (the roll does not change it)
    double acc = 0.0;
    for (int q0 = threadIdx.x; q0 < n4; q0 += U * TH) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {                  // loads first, from in-bounds addresses: U in flight per lane
        const int q = q0 + u * TH;
        v[u] = in4[q < n4 ? q : q0];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (q0 + u * TH < n4) acc += (double)v[u].x + (double)v[u].y + (double)v[u].z + (double)v[u].w;
    }
    acc = block_sum_d(acc, red);
    if (threadIdx.x == 0) S = acc;
    __syncthreads();

    const double cells = (double)L * F;
    for (int k = 0; k < nm; ++k) {
      const float fill = (float)(S / cells);          // every thread reads S before thread 0 may update it below
      const int r0 = M.r0[k], c0 = M.c0[k], w = M.c1[k] - c0;
      const int rows = M.r1[k] - r0;
      double r = 0.0;
      if (k < nt) {                                    // time mask: whole rows, earlier time masks only
        const int cnt = rows * F4;
        for (int q0 = threadIdx.x; q0 < cnt; q0 += U * TH) {
          float4 v[U];
          int i[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int q = q0 + u * TH < cnt ? q0 + u * TH : q0;
            i[u] = r0 + q / F4;
            v[u] = in4[src_row(i[u], s, L) * F4 + q % F4];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (q0 + u * TH >= cnt) break;
            const int m = time_cover(M, i[u], k);
            if (m >= 0) {
              const double f = (double)M.fill[m];
              r += f + f + f + f;
            } else {
              r += (double)v[u].x + (double)v[u].y + (double)v[u].z + (double)v[u].w;
            }
          }
        }
      } else {                                         // freq mask: columns [c0, c0 + w) of every row
        const int cnt = rows * w;
        const float* inr = in + base;
        for (int q0 = threadIdx.x; q0 < cnt; q0 += U * TH) {
          float v[U];
          int i[U], j[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int q = q0 + u * TH < cnt ? q0 + u * TH : q0;
            i[u] = r0 + q / w;
            j[u] = c0 + q % w;
            v[u] = inr[src_row(i[u], s, L) * F + j[u]];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (q0 + u * TH >= cnt) break;
            int m = M.colm[j[u]];
            if (m < 0) m = time_cover(M, i[u], nt);
            r += m >= 0 ? (double)M.fill[m] : (double)v[u];
          }
        }
      }
      r = block_sum_d(r, red);                         // (its barriers: every lane is done reading colm)
      if (k >= nt)
        for (int j = c0 + threadIdx.x; j < c0 + w; j += TH) M.colm[j] = (signed char)k;
      if (threadIdx.x == 0) {
        M.fill[k] = fill;
        S = S - r + (double)(rows * w) * (double)fill;
      }
      __syncthreads();
    }
  }

  // pass 2: rolled rows with the final fills
  for (int q0 = threadIdx.x; q0 < n4; q0 += U * TH) {
    float4 v[U];
    int row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * TH < n4 ? q0 + u * TH : q0;
      row[u] = q / F4;
      v[u] = in4[src_row(row[u], s, L) * F4 + q % F4];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * TH;
      if (q >= n4) break;
      if (nm > 0) {
        const int tm = time_cover(M, row[u], nt);
        const int cm = *reinterpret_cast<const int*>(&M.colm[4 * (q % F4)]);   // 4 columns' int8 entries
        float* e = reinterpret_cast<float*>(&v[u]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int m = (signed char)(cm >> (8 * c));
          if (m < 0) m = tm;
          if (m >= 0) e[c] = M.fill[m];
        }
      }
      out4[q] = v[u];
    }
  }
  // rows >= L: copied unchanged
  const int t4 = T * F4;
  for (int q0 = n4 + threadIdx.x; q0 < t4; q0 += U * TH) {
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * TH;
      v[u] = in4[q < t4 ? q : q0];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * TH;
      if (q < t4) out4[q] = v[u];
    }
  }
}
}  // namespace

extern "C" int acvae_spec_augment(const float* in, float* out, const int* lens, const int* params, int N, int T, int F,
                                  int K, void* stream) {
  if (!in || !out || !lens || !params || N <= 0 || T <= 0 || F <= 0 || (F & 3) != 0 || F > ACVAE_AUG_MAX_F ||
      (int64_t)T * F > INT32_MAX || K != ACVAE_AUG_TABLE_WIDTH)
    return ACVAE_EINVAL;
  if (!aligned16(in) || !aligned16(out)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(spec_augment_kernel, dim3(N), dim3(TH), 0, (hipStream_t)stream, in, out, lens, params, T, F);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
