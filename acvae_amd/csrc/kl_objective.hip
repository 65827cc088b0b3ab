// The variational term of the training objective with its controls: KL over the valid cells only, free bits per latent
// dimension or per cell, and the per-dimension / per-step diagnostics (include/acvae_hip.h has the definitions,
// acvae_amd/train_util.py: KLObjective the front).  acvae_gauss_kl_fwd / bwd (csrc/losses.hip) stay what the reference's
// Normal_kl_loss is; nothing here touches them.
//
// The mapping and why.  The inputs are four f32 [R, T, E] tensors, 5.5 MB at 32 x 21 x 512 and 27.5 MB at 160 x 21 x 512,
// read once; two families of sums are wanted from the same terms k[c, e]: over the cells c of S for every dimension e
// (m_e, E of them) and over e for every cell (s_c, R * T of them).
//   kl_obj_slab_kernel   one workgroup of 4 wavefronts per slab of ACVAE_KL_OBJECTIVE_SLAB = 8 cells, wavefront w the cells
//                        2w, 2w + 1 of the slab, its lanes along E in 16-byte pieces.  A lane keeps the running sum of each of
//                        its two cells (-> s_c by one butterfly over the wavefront at the end) and, per pass of 256 columns,
//                        the sum of its four columns over the two cells; the four wavefronts' column sums meet in 8 KB of
//                        LDS and are added in wavefront order: one float64 per slab and column goes to the scratch.
//                        84 workgroups at R = 32, 420 at R = 160: a slab is small so that the small batch still reaches a
//                        third of the CUs; the slab partials are R * T * E bytes, 1/16 of what was read.
//   kl_obj_finish_kernel one lane per dimension: the slabs' partials in slab order -> m_e, its gate, kl_dims; and one lane
//                        per step t: s_c over the rows that hold step t, r ascending -> kl_steps.
//   kl_obj_scalar_kernel one workgroup: sum_e m_e (kl_raw), the clamped sum over dimensions or over cells, the open gates.
// Three plain launches in stream order; no atomics, no hand-off inside a launch; every sum is float64 in a fixed order, so
// two runs agree bit for bit, and every scratch word that is read was written by the same call.
// The terms are evaluated in float64, as csrc/likelihood.hip: kl_term and for its reason (a term is what is left of
// summands of magnitude 1/2 that cancel); 2 E float64 exponentials per cell make kl_obj_slab_kernel bound by the vector
// unit rather than by its 16-byte loads, at a size where the launch costs more than either (profiles/r20_kl_objective.txt).
// Where q == p bit for bit the term is exactly 0: lv/2 - lv/2 = 0, exp(lv) / (2 exp(lv)) = 1/2 exactly (the doubling is
// exact), 0 + 1/2 - 1/2 = 0; the build has no FMA contraction (-ffp-contract=off) to undo that.
// Cells outside S are never read, forward or backward: a NaN there cannot reach anything.
//   kl_obj_bwd_kernel    elementwise, 16 bytes per lane and tensor: g * gate / D times the four derivatives of kl_bwd_kernel
//                        (csrc/losses.hip) in fp32, zeros where the gate is closed or the cell lies outside S.
// build.resource_usage():  kl_obj_slab_kernel<true> 74 VGPRs, <false> 76 VGPRs, 8192 B LDS, 6 waves / SIMD;  kl_obj_finish_kernel
// 20 VGPRs, no LDS;  kl_obj_scalar_kernel 24 VGPRs, 96 B LDS;  kl_obj_bwd_kernel<true> 48 VGPRs, <false> 21 VGPRs, no LDS;  no scratch
// memory in any of them.
#include <limits.h>

#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int KT = 256;                    // lanes per workgroup
constexpr int KW = KT / 64;
constexpr int CPW = ACVAE_KL_OBJECTIVE_SLAB / KW;      // cells per wavefront
static_assert(CPW * KW == ACVAE_KL_OBJECTIVE_SLAB, "a slab is a whole number of cells per wavefront");

__device__ __forceinline__ double klo_term(float mu1, float lv1, float mu2, float lv2) {
  const double d = (double)mu1 - (double)mu2;
  return (double)lv2 * .5 - (double)lv1 * .5 + (exp((double)lv1) + d * d) / (2. * exp((double)lv2)) - .5;
}

// max(v, lam) that keeps a NaN v (the gate, v > lam, is closed for it)
__device__ __forceinline__ double klo_clamp(double v, double lam) { return v <= lam ? lam : v; }

__device__ __forceinline__ bool klo_in_set(const int64_t* __restrict__ lens1, long cell, int T) {
  return !lens1 || (int64_t)(cell % T) < lens1[cell / T];
}

template <bool VEC>
__global__ __launch_bounds__(KT) void kl_obj_slab_kernel(const float* __restrict__ mu_q, const float* __restrict__ lv_q,
                                                         const float* __restrict__ mu_p, const float* __restrict__ lv_p,
                                                         const int64_t* __restrict__ lens1, double lam, int cell_gates,
                                                         double* __restrict__ dim_part, double* __restrict__ cell_sum,
                                                         uint8_t* __restrict__ gates, int C, int T, int E) {
  __shared__ double red[KW][KT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long first = (long)blockIdx.x * ACVAE_KL_OBJECTIVE_SLAB + w * CPW;
  bool in[CPW];
  double cs[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    in[i] = first + i < C && klo_in_set(lens1, first + i, T);
    cs[i] = 0.0;
  }
  // A lane owns four consecutive columns per pass of 256, whichever way they are loaded: the scalar path adds the same
  // numbers in the same order as the 16-byte one (a column past E counts as an exact 0).
  const int units = (E + 3) >> 2;
  for (int u0 = 0; u0 < units; u0 += 64) {  // (the trip count is the workgroup's: the barriers below are reached by all)
    const int u = u0 + lane;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    if (u < units) {
#pragma unroll
      for (int i = 0; i < CPW; ++i) {
        if (!in[i]) continue;
        const long o = (first + i) * (long)E + 4 * u;
        double k0, k1 = 0.0, k2 = 0.0, k3 = 0.0;
        if constexpr (VEC) {
          const float4 a = load4(mu_q + o), b = load4(lv_q + o), p = load4(mu_p + o), q = load4(lv_p + o);
          k0 = klo_term(a.x, b.x, p.x, q.x); k1 = klo_term(a.y, b.y, p.y, q.y);
          k2 = klo_term(a.z, b.z, p.z, q.z); k3 = klo_term(a.w, b.w, p.w, q.w);
        } else {
          const int left = E - 4 * u;       // >= 1
          k0 = klo_term(mu_q[o], lv_q[o], mu_p[o], lv_p[o]);
          if (left > 1) k1 = klo_term(mu_q[o + 1], lv_q[o + 1], mu_p[o + 1], lv_p[o + 1]);
          if (left > 2) k2 = klo_term(mu_q[o + 2], lv_q[o + 2], mu_p[o + 2], lv_p[o + 2]);
          if (left > 3) k3 = klo_term(mu_q[o + 3], lv_q[o + 3], mu_p[o + 3], lv_p[o + 3]);
        }
        c0 += k0; c1 += k1; c2 += k2; c3 += k3;
        cs[i] += (k0 + k1) + (k2 + k3);
      }
    }
    red[w][lane * 4] = c0; red[w][lane * 4 + 1] = c1; red[w][lane * 4 + 2] = c2; red[w][lane * 4 + 3] = c3;
    __syncthreads();
    const int col = u0 * 4 + tid;           // the pass holds 256 columns
    if (col < E) {
      double t = red[0][tid];
#pragma unroll
      for (int i = 1; i < KW; ++i) t += red[i][tid];
      dim_part[(long)blockIdx.x * E + col] = t;
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const double s = wave_sum_d(cs[i]);
    if (lane == 0 && first + i < C) {
      cell_sum[first + i] = in[i] ? s : 0.0;
      if (cell_gates) gates[first + i] = in[i] && s > lam ? 1 : 0;
    }
  }
}

// blocks [0, nbe): one lane per dimension;  blocks [nbe, nbe + nbt): one lane per step
__global__ __launch_bounds__(64) void kl_obj_finish_kernel(const double* __restrict__ dim_part, const double* __restrict__ cell_sum,
                                                           const int64_t* __restrict__ lens1, double inv_d, double lam,
                                                           int dim_gates, double* __restrict__ dim_mean,
                                                           float* __restrict__ kl_dims, float* __restrict__ kl_steps,
                                                           uint8_t* __restrict__ gates, int nslab, int nbe, int R, int T, int E) {
  if ((int)blockIdx.x < nbe) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    double acc = 0.0;
    int s = 0;
    for (; s + 3 < nslab; s += 4) {         // four loads in flight; the order of the additions is the slabs'
      const double p0 = dim_part[(long)s * E + e], p1 = dim_part[(long)(s + 1) * E + e];
      const double p2 = dim_part[(long)(s + 2) * E + e], p3 = dim_part[(long)(s + 3) * E + e];
      acc += p0; acc += p1; acc += p2; acc += p3;
    }
    for (; s < nslab; ++s) acc += dim_part[(long)s * E + e];
    const double m = acc * inv_d;
    dim_mean[e] = m;
    kl_dims[e] = (float)m;
    if (dim_gates) gates[e] = m > lam ? 1 : 0;
    return;
  }
  const int t = (blockIdx.x - nbe) * 64 + threadIdx.x;
  if (t >= T) return;
  double acc = 0.0;
  int n = 0;
  for (int r = 0; r < R; ++r) {
    if (lens1 && (int64_t)t >= lens1[r]) continue;
    acc += cell_sum[(long)r * T + t];
    ++n;
  }
  kl_steps[t] = n ? (float)(acc / (double)n) : 0.f;
}

__global__ __launch_bounds__(KT) void kl_obj_scalar_kernel(const double* __restrict__ dim_mean, const double* __restrict__ cell_sum,
                                                           const int64_t* __restrict__ lens1, double inv_d, double lam,
                                                           int free_bits, int over_cell, float* __restrict__ kl,
                                                           float* __restrict__ kl_raw, int32_t* __restrict__ gates_open,
                                                           int C, int T, int E) {
  __shared__ double red_r[KW], red_v[KW];
  __shared__ int red_n[KW], red_c[KW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double raw = 0.0, val = 0.0;
  int open = 0, cells = 0;
  for (int e = tid; e < E; e += KT) {
    const double m = dim_mean[e];
    raw += m;
    if (free_bits && !over_cell) {
      val += klo_clamp(m, lam);
      open += m > lam ? 1 : 0;
    }
  }
  if (over_cell) {
    for (int c = tid; c < C; c += KT) {
      if (!klo_in_set(lens1, c, T)) continue;
      ++cells;
      if (free_bits) {
        const double s = cell_sum[c];
        val += klo_clamp(s, lam);
        open += s > lam ? 1 : 0;
      }
    }
  }
  raw = wave_sum_d(raw);
  val = wave_sum_d(val);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    open += __shfl_xor(open, o, 64);
    cells += __shfl_xor(cells, o, 64);
  }
  if (lane == 0) { red_r[w] = raw; red_v[w] = val; red_n[w] = open; red_c[w] = cells; }
  __syncthreads();
  if (tid == 0) {
    double Rw = 0.0, V = 0.0;
    int N = 0, Cn = 0;
#pragma unroll
    for (int i = 0; i < KW; ++i) { Rw += red_r[i]; V += red_v[i]; N += red_n[i]; Cn += red_c[i]; }
    kl_raw[0] = (float)Rw;
    kl[0] = !free_bits ? (float)Rw : over_cell ? (float)(V * inv_d) : (float)V;
    gates_open[0] = free_bits ? N : over_cell ? Cn : E;
  }
}

template <bool VEC>
__global__ __launch_bounds__(KT) void kl_obj_bwd_kernel(const float* __restrict__ mu_q, const float* __restrict__ lv_q,
                                                        const float* __restrict__ mu_p, const float* __restrict__ lv_p,
                                                        const int64_t* __restrict__ lens1, const uint8_t* __restrict__ gates,
                                                        int over_cell, const float* __restrict__ grad_out, float inv_d,
                                                        float* __restrict__ dmu_q, float* __restrict__ dlv_q,
                                                        float* __restrict__ dmu_p, float* __restrict__ dlv_p, int T, int E,
                                                        long units) {
  constexpr int PER = VEC ? 4 : 1;
  const float g = grad_out[0] * inv_d;
  const int upc = E / PER;                  // units per cell
  for (long i = blockIdx.x * (long)KT + threadIdx.x; i < units; i += (long)gridDim.x * KT) {
    const long cell = i / upc;
    const int e0 = (int)(i % upc) * PER;
    const bool in = klo_in_set(lens1, cell, T);
    float a[PER], b[PER], c[PER], d[PER];   // dmu_q, dlv_q, dmu_p, dlv_p
#pragma unroll
    for (int j = 0; j < PER; ++j) a[j] = b[j] = c[j] = d[j] = 0.f;
    const bool cell_open = in && (!gates || !over_cell || gates[cell]);
    if (cell_open) {                        // (a closed cell is not read)
      const long o = cell * (long)E + e0;
      float m1[PER], l1[PER], m2[PER], l2[PER];
      if constexpr (VEC) {
        const float4 x = load4(mu_q + o), y = load4(lv_q + o), z = load4(mu_p + o), v = load4(lv_p + o);
        m1[0] = x.x; m1[1] = x.y; m1[2] = x.z; m1[3] = x.w;
        l1[0] = y.x; l1[1] = y.y; l1[2] = y.z; l1[3] = y.w;
        m2[0] = z.x; m2[1] = z.y; m2[2] = z.z; m2[3] = z.w;
        l2[0] = v.x; l2[1] = v.y; l2[2] = v.z; l2[3] = v.w;
      } else {
        m1[0] = mu_q[o]; l1[0] = lv_q[o]; m2[0] = mu_p[o]; l2[0] = lv_p[o];
      }
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (gates && !over_cell && !gates[e0 + j]) continue;
        const float df = m1[j] - m2[j];
        const float v1 = expf(l1[j]), iv2 = 1.f / expf(l2[j]);
        a[j] = g * df * iv2;
        c[j] = -g * df * iv2;
        b[j] = g * (-.5f + .5f * v1 * iv2);
        d[j] = g * (.5f - .5f * (v1 + df * df) * iv2);
      }
    }
    const long o = cell * (long)E + e0;
    if constexpr (VEC) {
      if (dmu_q) store4(dmu_q + o, make_float4(a[0], a[1], a[2], a[3]));
      if (dlv_q) store4(dlv_q + o, make_float4(b[0], b[1], b[2], b[3]));
      if (dmu_p) store4(dmu_p + o, make_float4(c[0], c[1], c[2], c[3]));
      if (dlv_p) store4(dlv_p + o, make_float4(d[0], d[1], d[2], d[3]));
    } else {
      if (dmu_q) dmu_q[o] = a[0];
      if (dlv_q) dlv_q[o] = b[0];
      if (dmu_p) dmu_p[o] = c[0];
      if (dlv_p) dlv_p[o] = d[0];
    }
  }
}

inline int64_t klo_slabs(int64_t C) { return (C + ACVAE_KL_OBJECTIVE_SLAB - 1) / ACVAE_KL_OBJECTIVE_SLAB; }

inline bool klo_dims_ok(int R, int T, int E) { return R > 0 && T > 0 && E > 0 && (int64_t)R * T <= INT_MAX; }
}  // namespace

extern "C" int64_t acvae_kl_objective_scratch_bytes(int R, int T, int E) {
  if (!klo_dims_ok(R, T, E)) return 0;
  const int64_t C = (int64_t)R * T;
  return 8 * (klo_slabs(C) * E + C + E);    // float64: slab partials [slabs, E], cell sums [R * T], m_e [E]
}

extern "C" int acvae_kl_objective_fwd(const float* mu_q, const float* lv_q, const float* mu_p, const float* lv_p,
                                      const int64_t* lens1, int64_t D, int free_bits, int over_cell, double lam, float* kl,
                                      float* kl_raw, float* kl_dims, float* kl_steps, int32_t* gates_open, uint8_t* gates,
                                      void* scratch, int64_t scratch_bytes, int R, int T, int E, void* stream) {
  if (!mu_q || !lv_q || !mu_p || !lv_p || !kl || !kl_raw || !kl_dims || !kl_steps || !gates_open || !scratch) return ACVAE_EINVAL;
  if (!klo_dims_ok(R, T, E)) return ACVAE_EINVAL;
  const int64_t C = (int64_t)R * T;
  if (D < 1 || D > C || (!lens1 && D != C)) return ACVAE_EINVAL;
  free_bits = free_bits != 0;
  over_cell = over_cell != 0;
  if (free_bits && (!gates || !(lam >= 0.0) || !(lam <= 1.79e308))) return ACVAE_EINVAL;    // (a NaN lam fails both)
  if (scratch_bytes < acvae_kl_objective_scratch_bytes(R, T, E)) return ACVAE_EWORKSPACE;
  if (reinterpret_cast<uintptr_t>(scratch) & 7u) return ACVAE_EALIGN;
  const int nslab = (int)klo_slabs(C);
  double* dim_part = static_cast<double*>(scratch);
  double* cell_sum = dim_part + (int64_t)nslab * E;
  double* dim_mean = cell_sum + C;
  const double inv_d = 1.0 / (double)D;
  const bool vec = E % 4 == 0 && aligned16(mu_q) && aligned16(lv_q) && aligned16(mu_p) && aligned16(lv_p);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(kl_obj_slab_kernel<true>, dim3(nslab), dim3(KT), 0, st, mu_q, lv_q, mu_p, lv_p, lens1, lam,
                       free_bits && over_cell, dim_part, cell_sum, gates, (int)C, T, E);
  else
    hipLaunchKernelGGL(kl_obj_slab_kernel<false>, dim3(nslab), dim3(KT), 0, st, mu_q, lv_q, mu_p, lv_p, lens1, lam,
                       free_bits && over_cell, dim_part, cell_sum, gates, (int)C, T, E);
  const int nbe = cdiv(E, 64), nbt = cdiv(T, 64);
  hipLaunchKernelGGL(kl_obj_finish_kernel, dim3(nbe + nbt), dim3(64), 0, st, dim_part, cell_sum, lens1, inv_d, lam,
                     free_bits && !over_cell, dim_mean, kl_dims, kl_steps, gates, nslab, nbe, R, T, E);
  hipLaunchKernelGGL(kl_obj_scalar_kernel, dim3(1), dim3(KT), 0, st, dim_mean, cell_sum, lens1, inv_d, lam, free_bits,
                     over_cell, kl, kl_raw, gates_open, (int)C, T, E);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_kl_objective_bwd(const float* mu_q, const float* lv_q, const float* mu_p, const float* lv_p,
                                      const int64_t* lens1, int64_t D, int over_cell, const uint8_t* gates,
                                      const float* grad_out, float* dmu_q, float* dlv_q, float* dmu_p, float* dlv_p, int R,
                                      int T, int E, void* stream) {
  if (!mu_q || !lv_q || !mu_p || !lv_p || !grad_out) return ACVAE_EINVAL;
  if (!klo_dims_ok(R, T, E)) return ACVAE_EINVAL;
  const int64_t C = (int64_t)R * T;
  if (D < 1 || D > C || (!lens1 && D != C)) return ACVAE_EINVAL;
  if (!dmu_q && !dlv_q && !dmu_p && !dlv_p) return ACVAE_OK;
  const bool vec = E % 4 == 0 && aligned16(mu_q) && aligned16(lv_q) && aligned16(mu_p) && aligned16(lv_p) &&
                   aligned16(dmu_q) && aligned16(dlv_q) && aligned16(dmu_p) && aligned16(dlv_p);
  const float inv_d = (float)(1.0 / (double)D);
  const long units = C * (long)(vec ? E / 4 : E);
  const int grid = (int)((units + KT - 1) / KT < 65535 * 4 ? (units + KT - 1) / KT : 65535 * 4);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(kl_obj_bwd_kernel<true>, dim3(grid), dim3(KT), 0, st, mu_q, lv_q, mu_p, lv_p, lens1, gates,
                       over_cell != 0, grad_out, inv_d, dmu_q, dlv_q, dmu_p, dlv_p, T, E, units);
  else
    hipLaunchKernelGGL(kl_obj_bwd_kernel<false>, dim3(grid), dim3(KT), 0, st, mu_q, lv_q, mu_p, lv_p, lens1, gates,
                       over_cell != 0, grad_out, inv_d, dmu_q, dlv_q, dmu_p, dlv_p, T, E, units);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
