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
//
// acvae_augment_window is the same body with a crop in front: the clip the rolls and masks see is a chain of (circular)
// windows cut out of a longer input clip, as Augment.draw_shape planned them.  Only the row a cell is read from changes:
// every pass walks the cells of the OUTPUT clip in the order spec_augment_kernel walks them, so the sums - and with them
// the fills - are bit for bit those of acvae_spec_augment run on the host-cropped clip.
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

// The crops of one clip, last first: row j of the clip behind a window is row (j + add) mod len of the clip in front of
// it, add = (start - shift) mod len.  j < len holds at every step (each window is no longer than the clip it is cut
// from), so one conditional subtraction is the modulo.  Unused steps are add = 0, len = INT32_MAX: no-ops; a clip
// without crops (n == 0, the same for the whole workgroup) skips them.
struct Windows {
  int add[ACVAE_AUG_MAX_WINDOWS], len[ACVAE_AUG_MAX_WINDOWS];
  int n;
};
template <bool WIN>
__device__ __forceinline__ int win_row(int j, const Windows& W) {
  if (WIN && W.n > 0) {
#pragma unroll
    for (int w = 0; w < ACVAE_AUG_MAX_WINDOWS; ++w) {
      j += W.add[w];
      if (j >= W.len[w]) j -= W.len[w];
    }
  }
  return j;
}

// Latest time mask with index < kend that covers row i, or -1.  A fixed-length loop without early exit: its LDS reads
// issue together instead of one dependent read per mask.
__device__ __forceinline__ int time_cover(const Masks& M, int i, int kend) {
  int best = -1;
#pragma unroll
  for (int m = 0; m < ACVAE_AUG_MAX_MASKS; ++m)
    if (m < kend && M.r0[m] <= i && i < M.r1[m]) best = m;
  return best;
}

// The body of both kernels.  WIN = false: acvae_spec_augment (`lens` the clips' lengths, To == T, rows >= L copied).
// WIN = true: acvae_augment_window (`lens` the lengths of the input clips, rows of K = ACVAE_AUG_WINDOW_TABLE_WIDTH
// entries, the output clip To rows long, rows >= L zeros).
template <bool WIN>
__device__ __forceinline__ void augment_body(const float* __restrict__ in, float* __restrict__ out,
                                             const int* __restrict__ lens, const int* __restrict__ params, int T, int To,
                                             int F) {
  __shared__ Masks M;
  __shared__ double red[NW];
  __shared__ double S;
  __shared__ int L_s, shift_s;
  __shared__ Windows W_s;
  const int n = blockIdx.x;
  const int F4 = F >> 2;
  const long base = (long)n * T * F;
  const float4* in4 = reinterpret_cast<const float4*>(in + base);
  float4* out4 = reinterpret_cast<float4*>(out + (WIN ? (long)n * To * F : base));

  if (threadIdx.x == 0) {
    const int* row = params + (long)n * (WIN ? ACVAE_AUG_WINDOW_TABLE_WIDTH : ACVAE_AUG_TABLE_WIDTH);
    int L = clampi(lens[n], 0, T);
    if (WIN) {                                   // the crops: each length clamped into [1, the size in front of it]
      const int* win = row + ACVAE_AUG_TABLE_WIDTH + 2;
      const int nw = L > 0 ? clampi(row[ACVAE_AUG_TABLE_WIDTH + 1], 0, ACVAE_AUG_MAX_WINDOWS) : 0;
      for (int w = 0; w < ACVAE_AUG_MAX_WINDOWS; ++w) {
        const int k = nw - 1 - w;                // stored last window first, the order win_row applies them in
        int add = 0, len = INT32_MAX;
        if (w < nw) {
          len = L = clampi(win[3 * w + 2], 1, L);
          add = (clampi(win[3 * w], 0, len - 1) - win[3 * w + 1] % len) % len;
          if (add < 0) add += len;
          W_s.add[k] = add; W_s.len[k] = len;
        } else {
          W_s.add[w] = add; W_s.len[w] = len;
        }
      }
      W_s.n = nw;
      L = clampi(row[ACVAE_AUG_TABLE_WIDTH], 0, L < To ? L : To);
    }
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
  Windows W;
  if (WIN) {
    W = W_s;
    W.n = __builtin_amdgcn_readfirstlane(W.n);
  }

  if (nm > 0) {
    // pass 1: the clip's sum (the roll does not change it)
    double acc = 0.0;
    for (int q0 = threadIdx.x; q0 < n4; q0 += U * TH) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {                  // loads first, from in-bounds addresses: U in flight per lane
        const int q = q0 + u * TH < n4 ? q0 + u * TH : q0;
        v[u] = in4[WIN && W.n > 0 ? win_row<WIN>(q / F4, W) * F4 + q % F4 : q];
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
            v[u] = in4[win_row<WIN>(src_row(i[u], s, L), W) * F4 + q % F4];
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
            v[u] = inr[win_row<WIN>(src_row(i[u], s, L), W) * F + j[u]];
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
      v[u] = in4[win_row<WIN>(src_row(row[u], s, L), W) * F4 + q % F4];
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
  if (WIN) {                         // rows >= L of the output clip: zeros, what collate_fn pads with
    const int t4 = To * F4;
    for (int q = n4 + threadIdx.x; q < t4; q += TH) out4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
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

__global__ __launch_bounds__(TH) void spec_augment_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          const int* __restrict__ lens, const int* __restrict__ params,
                                                          int T, int F) {
  augment_body<false>(in, out, lens, params, T, T, F);
}

__global__ __launch_bounds__(TH) void augment_window_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const int* __restrict__ src_lens,
                                                            const int* __restrict__ table, int T, int To, int F) {
  augment_body<true>(in, out, src_lens, table, T, To, F);
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

extern "C" int acvae_augment_window(const float* in, float* out, const int* src_lens, const int* table, int N, int T,
                                    int To, int F, int K, void* stream) {
  if (!in || !out || !src_lens || !table || N <= 0 || T <= 0 || To <= 0 || To > T || F <= 0 || (F & 3) != 0 ||
      F > ACVAE_AUG_MAX_F || (int64_t)T * F > INT32_MAX || K != ACVAE_AUG_WINDOW_TABLE_WIDTH)
    return ACVAE_EINVAL;
  if (!aligned16(in) || !aligned16(out)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(augment_window_kernel, dim3(N), dim3(TH), 0, (hipStream_t)stream, in, out, src_lens, table, T, To, F);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
