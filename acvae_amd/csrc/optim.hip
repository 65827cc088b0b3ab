// A10: global-norm gradient clipping + Adam over ONE flat fp32 parameter/gradient buffer.
// Reference: runners/pytorch_runner_vae.py:321-324 (loss.backward -> clip_grad_norm_(max_grad_norm) ->
// optimizer.step with torch.optim.Adam).  HBM-bound streaming kernels: the norm is one read of the gradients
// (two-level fixed-order reduction, fp64 combine: deterministic), the update is one pass that reads p,g,m,v and
// writes p,m,v (28 B/param), with the clip coefficient taken from the device-side norm so no host sync is needed.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int TH = 256;
constexpr int NORM_BLOCKS = 1024;

__global__ __launch_bounds__(TH) void sqsum_kernel(const float* __restrict__ g, long n, float* __restrict__ partials) {
  __shared__ float red[16];
  float acc = 0.f;
  const long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (long i = blockIdx.x * (long)TH + threadIdx.x; i < n4; i += (long)gridDim.x * TH) {
    const float4 v = g4[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += TH) acc += g[i] * g[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
// norm = scale * sqrt(sum partials)
__global__ void norm_final_kernel(const float* __restrict__ partials, int n, float scale, float* __restrict__ out) {
  __shared__ double redd[16];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)partials[i];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) redd[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += redd[i];
    out[0] = (float)(sqrt(t) * (double)scale);
  }
}

__global__ __launch_bounds__(TH) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                  float beta1, float beta2, float eps, float weight_decay,
                                                  float bc1, float bc2_sqrt, float grad_scale, float max_norm,
                                                  const float* __restrict__ total_norm) {
  // clip_grad_norm_: coef = clamp(max_norm / (total_norm + 1e-6), max=1)
  float coef = grad_scale;
  if (total_norm && max_norm > 0.f) {
    float c = max_norm / (total_norm[0] + 1e-6f);
    coef *= c < 1.f ? c : 1.f;
  }
  const float step_size = lr / bc1;
  for (long i = blockIdx.x * (long)TH + threadIdx.x; i < n; i += (long)gridDim.x * TH) {
    float gi = g[i] * coef;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] = pi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
  }
}
}  // namespace

extern "C" int64_t acvae_grad_norm_partials(void) { return NORM_BLOCKS; }

extern "C" int acvae_grad_norm(const float* grads, int64_t n, float grad_scale, float* partials, float* out_norm,
                               void* stream) {
  if (!grads || !partials || !out_norm || n <= 0) return ACVAE_EINVAL;
  if (!aligned16(grads)) return ACVAE_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  long nb = (n / 4 + TH - 1) / TH;
  if (nb < 1) nb = 1;
  if (nb > NORM_BLOCKS) nb = NORM_BLOCKS;
  hipLaunchKernelGGL(sqsum_kernel, dim3((int)nb), dim3(TH), 0, st, grads, (long)n, partials);
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(256), 0, st, partials, (int)nb, grad_scale, out_norm);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                               float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                               float grad_scale, float max_grad_norm, const float* total_norm, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return ACVAE_EINVAL;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long nb = (n + TH - 1) / TH;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(adam_kernel, dim3((int)nb), dim3(TH), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq,
                     (long)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale,
                     max_grad_norm, total_norm);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// AdamW / amsgrad / SGD over the same flat buffer (the reference takes its optimiser from conf["optimizer"],
// runners/pytorch_runner_vae.py:219).  One streaming kernel body, the optimiser kind a template parameter; every
// element follows the operation order of torch.optim.<X>(foreach=False), so the result agrees with torch to fp32
// elementwise rounding.  float4 main loop, scalar tail in block 0 (as sqsum_kernel).  Bytes per parameter:
// Adam/AdamW 28 (+8 amsgrad), SGD 12 (+4 reading the momentum buffer, +4 writing it).
namespace {
enum OptKind { OPT_ADAM = 0, OPT_SGD = 1 };

struct OptArgs {
  float* p; const float* g; float* s0; float* s1; float* s2;   // Adam: exp_avg, exp_avg_sq, max_exp_avg_sq; SGD: buf
  long n;
  float lr, a, b, c, d, wd, decay;       // Adam: a = 1-beta1, b = beta2, c = 1-beta2, d = eps; SGD: a = momentum, b = 1-dampening
  float step_size, bc2_sqrt;             // Adam: lr / bc1, sqrt(bc2)
  int flags;                             // OPT_F_*
  float grad_scale, max_norm;
  const float* total_norm;
};
constexpr int OPT_F_DECOUPLED = 1, OPT_F_NESTEROV = 2, OPT_F_FIRST = 4;

// torch's lerp: weight < 0.5 ? a + w*(b-a) : b - (b-a)*(1-w)
__device__ __forceinline__ float lerp_t(float a, float b, float w) {
  return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w);
}

// One element; STATE = amsgrad (Adam) / momentum != 0 (SGD).  Only the state that the kind uses is touched.
template <int KIND, bool STATE>
__device__ __forceinline__ void opt_elem(const OptArgs& A, float coef, float& p, float g, float& s0, float& s1, float& s2) {
  g *= coef;
  if (KIND == OPT_ADAM) {
    if (A.wd != 0.f) {
      if (A.flags & OPT_F_DECOUPLED) p *= A.decay;     // param.mul_(1 - lr*wd)
      else g += A.wd * p;                              // grad.add(param, alpha=wd)
    }
    s0 = lerp_t(s0, g, A.a);                           // exp_avg.lerp_(grad, 1-beta1)
    s1 = s1 * A.b + A.c * (g * g);                     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1-beta2)
    float v = s1;
    if (STATE) { s2 = fmaxf(s2, s1); v = s2; }         // torch.maximum(max_exp_avg_sq, exp_avg_sq)
    const float denom = sqrtf(v) / A.bc2_sqrt + A.d;
    p = p + (-A.step_size) * (s0 / denom);             // addcdiv_(exp_avg, denom, value=-step_size)
  } else {
    if (A.wd != 0.f) g += A.wd * p;
    if (STATE) {
      s0 = (A.flags & OPT_F_FIRST) ? g : s0 * A.a + A.b * g;
      g = (A.flags & OPT_F_NESTEROV) ? g + A.a * s0 : s0;
    }
    p = p + (-A.lr) * g;
  }
}

template <int KIND, bool STATE>
__global__ __launch_bounds__(TH) void opt_kernel(OptArgs A) {
  float coef = A.grad_scale;                           // clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max=1)
  if (A.total_norm && A.max_norm > 0.f) {
    float c = A.max_norm / (A.total_norm[0] + 1e-6f);
    coef *= c < 1.f ? c : 1.f;
  }
  constexpr bool ADAM = KIND == OPT_ADAM;
  // which state arrays are read / written (SGD's first step writes the buffer without reading it)
  const bool r0 = ADAM || (STATE && !(A.flags & OPT_F_FIRST));
  const bool w0 = ADAM || STATE;
  const bool u1 = ADAM, u2 = ADAM && STATE;
  const long n4 = A.n >> 2;
  float4* p4 = reinterpret_cast<float4*>(A.p);
  const float4* g4 = reinterpret_cast<const float4*>(A.g);
  float4* s04 = reinterpret_cast<float4*>(A.s0);
  float4* s14 = reinterpret_cast<float4*>(A.s1);
  float4* s24 = reinterpret_cast<float4*>(A.s2);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long i = blockIdx.x * (long)TH + threadIdx.x; i < n4; i += (long)gridDim.x * TH) {
    float4 p = p4[i];
    const float4 g = g4[i];
    float4 s0 = r0 ? s04[i] : z, s1 = u1 ? s14[i] : z, s2 = u2 ? s24[i] : z;
    opt_elem<KIND, STATE>(A, coef, p.x, g.x, s0.x, s1.x, s2.x);
    opt_elem<KIND, STATE>(A, coef, p.y, g.y, s0.y, s1.y, s2.y);
    opt_elem<KIND, STATE>(A, coef, p.z, g.z, s0.z, s1.z, s2.z);
    opt_elem<KIND, STATE>(A, coef, p.w, g.w, s0.w, s1.w, s2.w);
    p4[i] = p;
    if (w0) s04[i] = s0;
    if (u1) s14[i] = s1;
    if (u2) s24[i] = s2;
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < A.n; i += TH) {
      float p = A.p[i], s0 = r0 ? A.s0[i] : 0.f, s1 = u1 ? A.s1[i] : 0.f, s2 = u2 ? A.s2[i] : 0.f;
      opt_elem<KIND, STATE>(A, coef, p, A.g[i], s0, s1, s2);
      A.p[i] = p;
      if (w0) A.s0[i] = s0;
      if (u1) A.s1[i] = s1;
      if (u2) A.s2[i] = s2;
    }
}

bool aligned_or_null(const void* p) { return !p || aligned16(p); }

int launch_opt(int kind, bool state, const OptArgs& A, void* stream) {
  long nb = (A.n / 4 + TH - 1) / TH;
  if (nb < 1) nb = 1;
  if (nb > 4096) nb = 4096;
  hipStream_t st = (hipStream_t)stream;
  if (kind == OPT_ADAM) {
    if (state) hipLaunchKernelGGL((opt_kernel<OPT_ADAM, true>), dim3((int)nb), dim3(TH), 0, st, A);
    else hipLaunchKernelGGL((opt_kernel<OPT_ADAM, false>), dim3((int)nb), dim3(TH), 0, st, A);
  } else {
    if (state) hipLaunchKernelGGL((opt_kernel<OPT_SGD, true>), dim3((int)nb), dim3(TH), 0, st, A);
    else hipLaunchKernelGGL((opt_kernel<OPT_SGD, false>), dim3((int)nb), dim3(TH), 0, st, A);
  }
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
}  // namespace

extern "C" int acvae_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                float* max_exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int decoupled, int amsgrad, int64_t step, float grad_scale,
                                float max_grad_norm, const float* total_norm, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || (amsgrad && !max_exp_avg_sq) || n <= 0 || step <= 0)
    return ACVAE_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
      (amsgrad && !aligned16(max_exp_avg_sq)))
    return ACVAE_EALIGN;
  // hyperparameters arrive in double and every derived scalar is formed in double, then rounded once, as torch's Python
  // scalars reach its fp32 kernels (1 - beta2 from a float 0.999f would be off by 1.3e-5 relative)
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  OptArgs A{};
  A.p = params; A.g = grads; A.s0 = exp_avg; A.s1 = exp_avg_sq; A.s2 = amsgrad ? max_exp_avg_sq : nullptr;
  A.n = (long)n; A.lr = (float)lr;
  A.a = (float)(1.0 - beta1); A.b = (float)beta2; A.c = (float)(1.0 - beta2); A.d = (float)eps;
  A.wd = (float)weight_decay; A.decay = (float)(1.0 - lr * weight_decay);
  A.step_size = (float)(lr / bc1); A.bc2_sqrt = (float)sqrt(bc2);
  A.flags = decoupled ? OPT_F_DECOUPLED : 0;
  A.grad_scale = grad_scale; A.max_norm = max_grad_norm; A.total_norm = total_norm;
  return launch_opt(OPT_ADAM, amsgrad != 0, A, stream);
}

extern "C" int acvae_sgd_step(float* params, const float* grads, float* momentum_buffer, int64_t n, double lr,
                              double momentum, double dampening, double weight_decay, int nesterov, int first,
                              float grad_scale, float max_grad_norm, const float* total_norm, void* stream) {
  const bool mom = momentum != 0.0;
  if (!params || !grads || (mom && !momentum_buffer) || n <= 0) return ACVAE_EINVAL;
  if (nesterov && (!mom || dampening != 0.0)) return ACVAE_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned_or_null(mom ? momentum_buffer : nullptr)) return ACVAE_EALIGN;
  OptArgs A{};
  A.p = params; A.g = grads; A.s0 = mom ? momentum_buffer : nullptr;
  A.n = (long)n; A.lr = (float)lr;
  A.a = (float)momentum; A.b = (float)(1.0 - dampening); A.wd = (float)weight_decay;
  A.flags = (nesterov ? OPT_F_NESTEROV : 0) | (first ? OPT_F_FIRST : 0);
  A.grad_scale = grad_scale; A.max_norm = max_grad_norm; A.total_norm = total_norm;
  return launch_opt(OPT_SGD, mom, A, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Gradient accumulation and the weight EMA of TrainStep(accum_steps=, ema_decay=): two more streaming passes over the flat
// buffers.  float4 main loop, scalar tail in block 0 (as sqsum_kernel), grid-stride under ACVAE_FLAT_BLOCKS_CAP blocks
// (256 CUs x 8 blocks).  Every element is stored once; no atomics, no workspace.  Bytes per element: accumulate 12
// (8 with first: acc is not read), EMA 12.
// kernel-resource-usage (gfx950, -O3): accumulate_kernel<true> 12 VGPRs / 24 SGPRs, accumulate_kernel<false> 18 / 26,
// ema_kernel 26 / 30; no scratch, no LDS, occupancy 8 waves per SIMD for all three.
namespace {
constexpr int FLAT_BLOCKS = ACVAE_FLAT_BLOCKS_CAP;

template <bool FIRST>
__global__ __launch_bounds__(TH) void accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n) {
  const long n4 = n >> 2;
  float4* a4 = reinterpret_cast<float4*>(acc);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (long i = blockIdx.x * (long)TH + threadIdx.x; i < n4; i += (long)gridDim.x * TH) {
    float4 v = g4[i];
    if (!FIRST) {
      const float4 a = a4[i];
      v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w;
    }
    a4[i] = v;
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += TH) acc[i] = FIRST ? g[i] : acc[i] + g[i];
}

__device__ __forceinline__ void ema_body(float* __restrict__ ema, const float* __restrict__ p, long n, float w) {
  const long n4 = n >> 2;
  float4* e4 = reinterpret_cast<float4*>(ema);
  const float4* p4 = reinterpret_cast<const float4*>(p);
  for (long i = blockIdx.x * (long)TH + threadIdx.x; i < n4; i += (long)gridDim.x * TH) {
    float4 e = e4[i];
    const float4 v = p4[i];
    e.x = lerp_t(e.x, v.x, w); e.y = lerp_t(e.y, v.y, w); e.z = lerp_t(e.z, v.z, w); e.w = lerp_t(e.w, v.w, w);
    e4[i] = e;
  }
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += TH) ema[i] = lerp_t(ema[i], p[i], w);
}

__global__ __launch_bounds__(TH) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float w) {
  ema_body(ema, p, n, w);
}

// [a, a + n) and [b, b + n) floats share a byte
bool ranges_overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  const uintptr_t bytes = (uintptr_t)n * sizeof(float);
  return x < y ? y - x < bytes : x - y < bytes;
}

int flat_blocks(int64_t n) {
  long nb = (n / 4 + TH - 1) / TH;
  if (nb < 1) nb = 1;
  if (nb > FLAT_BLOCKS) nb = FLAT_BLOCKS;
  return (int)nb;
}
}  // namespace

extern "C" int acvae_grad_accumulate(float* acc, const float* grads, int64_t n, int first, void* stream) {
  if (!acc || !grads || n <= 0 || ranges_overlap(acc, grads, n)) return ACVAE_EINVAL;
  if (!aligned16(acc) || !aligned16(grads)) return ACVAE_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (first) hipLaunchKernelGGL(accumulate_kernel<true>, dim3(flat_blocks(n)), dim3(TH), 0, st, acc, grads, (long)n);
  else hipLaunchKernelGGL(accumulate_kernel<false>, dim3(flat_blocks(n)), dim3(TH), 0, st, acc, grads, (long)n);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_ema_step(float* ema, const float* params, int64_t n, double decay, void* stream) {
  if (!ema || !params || n <= 0 || !(decay >= 0.0 && decay <= 1.0) || ranges_overlap(ema, params, n)) return ACVAE_EINVAL;
  if (!aligned16(ema) || !aligned16(params)) return ACVAE_EALIGN;
  // 1 - decay is formed in double and rounded once, as the optimisers' 1 - beta
  hipLaunchKernelGGL(ema_kernel, dim3(flat_blocks(n)), dim3(TH), 0, (hipStream_t)stream, ema, params, (long)n,
                     (float)(1.0 - decay));
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Parameter groups (TrainStep(param_groups=)): the norm and the update with up to ACVAE_OPT_MAX_GROUPS sets of
// hyperparameters.  The host cuts the flat range into chunks of at most OPT_CHUNK elements that never leave a group
// (include/acvae_hip.h has the table's layout); a workgroup walks chunks b, b + grid, ..., so everything it reads from the
// table and from the per-group hyperparameters is uniform and sits in scalar registers.  The table (12 B per chunk) is
// on the device; the hyperparameters, which change every step, are a by-value kernel argument like OptArgs.  The element
// arithmetic is opt_elem itself and the derived scalars are formed as acvae_adamw_step / acvae_sgd_step form them, so a
// chunk comes out bit for bit as the one-group kernel over its range would leave it.  Every slice is a multiple of four
// elements: no scalar tail.  A chunk that does not fit (negative start, no length, group >= n_groups, unknown bits) is
// skipped, a length above OPT_CHUNK or an end behind n is cut: a bad table is never followed.
// kernel-resource-usage (gfx950, -O3), VGPRs / SGPRs / LDS bytes: sqsum_chunks_kernel 20 / 44 / 64, norm_groups_final_kernel
// 48 / 24 / 16448, opt_groups_kernel<Adam, amsgrad> 45 / 68 / 0, <Adam> 39 / 64 / 0, <SGD, momentum> 32 / 58 / 0, <SGD> 22 / 41 / 0;
// no scratch, occupancy 8 waves per SIMD for all six.
#include "job_table.h"
// The chunk size, by measurement at 28.6 M elements (profiles/r22_param_groups.txt; -DACVAE_OPT_CHUNK=C builds a candidate):
// 4096 and 8192 make the finishing launch of the norm walk 7000 / 3500 table rows (20 / 12 us against 6), 32768 leaves 890
// workgroups for 256 CUs and both streaming kernels lose 14 - 20 %; 16384 holds all three to the one-group kernels' times.
#ifndef ACVAE_OPT_CHUNK
#define ACVAE_OPT_CHUNK 16384
#endif
namespace {
constexpr int OPT_CHUNK = ACVAE_OPT_CHUNK;                 // elements; a multiple of 4 * TH keeps every trip of a full chunk full
constexpr int OPT_CHUNK4 = OPT_CHUNK / 4;
constexpr int GROUP_BLOCKS = 4096;                         // as launch_opt
static_assert(OPT_CHUNK % 4 == 0 && OPT_CHUNK > 0, "chunks count float4s");

struct GroupHyper {                                        // OptArgs' per-group part, same meaning of every field
  float lr, a, b, c, d, wd, decay, step_size, bc2_sqrt;
};
struct GroupedArgs {
  float* p; const float* g; float* s0; float* s1; float* s2;
  long n;
  const int* chunks;
  int n_chunks, n_groups;
  int flags;                                               // OPT_F_DECOUPLED | OPT_F_NESTEROV; OPT_F_FIRST comes from the chunk
  float grad_scale, max_norm;
  const float* total_norm;
  const acvae_guard_record* guard;                         // the guarded entries' record (GUARD instantiations only)
  acvae::JobTable<GroupHyper, ACVAE_OPT_MAX_GROUPS> hyper;
};

// chunk c of the table -> [a, e) in float4s and the group; false: skip it.  Uniform over the workgroup.
__device__ __forceinline__ bool read_chunk(const int* __restrict__ chunks, int c, int n_groups, long n4, long& a, long& e,
                                           int& group, bool& first) {
  const int start = chunks[3 * c], len = chunks[3 * c + 1], tag = chunks[3 * c + 2];
  group = tag & (ACVAE_OPT_CHUNK_FIRST - 1);
  first = (tag & ACVAE_OPT_CHUNK_FIRST) != 0;
  if (start < 0 || len <= 0 || tag < 0 || (tag & ~(2 * ACVAE_OPT_CHUNK_FIRST - 1)) || group >= n_groups) return false;
  a = start;
  e = a + (len < OPT_CHUNK4 ? len : OPT_CHUNK4);
  if (e > n4) e = n4;
  return a < e;
}

__global__ __launch_bounds__(TH) void sqsum_chunks_kernel(const float* __restrict__ g, const int* __restrict__ chunks,
                                                          int n_chunks, int n_groups, float* __restrict__ partials) {
  __shared__ float red[16];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    long a = 0, e = 0;
    int group;
    bool first;
    float acc = 0.f;
    // (the norm has no n: the table's own bounds are all there is, the length still cut to a chunk)
    if (read_chunk(chunks, c, n_groups, 0x7fffffffL + OPT_CHUNK4, a, e, group, first))
      for (long i = a + threadIdx.x; i < e; i += TH) {
        const float4 v = g4[i];
        acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partials[c] = acc;               // a skipped chunk stores its zero: nothing of partials is read unset
  }
}

// One workgroup.  Thread t adds chunks [t * per, (t + 1) * per) in ascending order into one float64 sum per group (a
// select, not a product: a NaN stays in its group), thread 0 adds the threads' sums in ascending order and then the groups.
__global__ __launch_bounds__(TH) void norm_groups_final_kernel(const float* __restrict__ partials,
                                                               const int* __restrict__ chunks, int n_chunks, int n_groups,
                                                               float scale, float* __restrict__ group_norms,
                                                               float* __restrict__ total_norm) {
  __shared__ double sums[ACVAE_OPT_MAX_GROUPS][TH + 1];
  double acc[ACVAE_OPT_MAX_GROUPS];
#pragma unroll
  for (int k = 0; k < ACVAE_OPT_MAX_GROUPS; ++k) acc[k] = 0.0;
  const int per = (n_chunks + TH - 1) / TH;
  const int c0 = threadIdx.x * per, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
  for (int c = c0; c < c1; ++c) {
    const int tag = chunks[3 * c + 2];
    const int group = tag & (ACVAE_OPT_CHUNK_FIRST - 1);
    const double v = (double)partials[c];
    if (tag >= 0 && group < n_groups) {
#pragma unroll
      for (int k = 0; k < ACVAE_OPT_MAX_GROUPS; ++k) acc[k] += group == k ? v : 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < ACVAE_OPT_MAX_GROUPS; ++k) sums[k][threadIdx.x] = acc[k];
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < ACVAE_OPT_MAX_GROUPS)
    for (int i = 0; i < TH; ++i) t += sums[threadIdx.x][i];
  __syncthreads();
  if (threadIdx.x < ACVAE_OPT_MAX_GROUPS) sums[threadIdx.x][0] = t;
  __syncthreads();
  if (threadIdx.x < n_groups) group_norms[threadIdx.x] = (float)(sqrt(t) * (double)scale);
  if (threadIdx.x == 0) {
    double all = 0.0;
    for (int k = 0; k < n_groups; ++k) all += sums[k][0];
    total_norm[0] = (float)(sqrt(all) * (double)scale);
  }
}

// GUARD: the non-finite guard's form (further down).  The workgroup reads the record's decision once (uniform) and leaves
// before it has touched anything when the update is skipped; otherwise Adam's step_size / bc2_sqrt are the record's, formed
// on the device from its own count of applied updates.  Without GUARD the kernel is what it was.
template <int KIND, bool STATE, bool GUARD = false>
__global__ __launch_bounds__(TH) void opt_groups_kernel(GroupedArgs G) {
  if (GUARD && G.guard->ok == 0) return;
  float coef = G.grad_scale;                               // as opt_kernel
  if (G.total_norm && G.max_norm > 0.f) {
    float c = G.max_norm / (G.total_norm[0] + 1e-6f);
    coef *= c < 1.f ? c : 1.f;
  }
  constexpr bool ADAM = KIND == OPT_ADAM;
  const bool w0 = ADAM || STATE;
  const bool u1 = ADAM, u2 = ADAM && STATE;
  const long n4 = G.n >> 2;
  float4* p4 = reinterpret_cast<float4*>(G.p);
  const float4* g4 = reinterpret_cast<const float4*>(G.g);
  float4* s04 = reinterpret_cast<float4*>(G.s0);
  float4* s14 = reinterpret_cast<float4*>(G.s1);
  float4* s24 = reinterpret_cast<float4*>(G.s2);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = blockIdx.x; c < G.n_chunks; c += gridDim.x) {
    long a, e;
    int group;
    bool first;
    if (!read_chunk(G.chunks, c, G.n_groups, n4, a, e, group, first)) continue;
    const GroupHyper& h = G.hyper.job[group];
    OptArgs A{};
    A.lr = h.lr; A.a = h.a; A.b = h.b; A.c = h.c; A.d = h.d; A.wd = h.wd; A.decay = h.decay;
    A.step_size = h.step_size; A.bc2_sqrt = h.bc2_sqrt;
    if (GUARD && ADAM) { A.step_size = G.guard->step_size[group]; A.bc2_sqrt = G.guard->bc2_sqrt[group]; }
    A.flags = G.flags | (first ? OPT_F_FIRST : 0);
    const bool r0 = ADAM || (STATE && !first);
    for (long i = a + threadIdx.x; i < e; i += TH) {
      float4 p = p4[i];
      const float4 g = g4[i];
      float4 s0 = r0 ? s04[i] : z, s1 = u1 ? s14[i] : z, s2 = u2 ? s24[i] : z;
      opt_elem<KIND, STATE>(A, coef, p.x, g.x, s0.x, s1.x, s2.x);
      opt_elem<KIND, STATE>(A, coef, p.y, g.y, s0.y, s1.y, s2.y);
      opt_elem<KIND, STATE>(A, coef, p.z, g.z, s0.z, s1.z, s2.z);
      opt_elem<KIND, STATE>(A, coef, p.w, g.w, s0.w, s1.w, s2.w);
      p4[i] = p;
      if (w0) s04[i] = s0;
      if (u1) s14[i] = s1;
      if (u2) s24[i] = s2;
    }
  }
}

int group_blocks(int n_chunks) { return n_chunks < GROUP_BLOCKS ? n_chunks : GROUP_BLOCKS; }

int launch_opt_groups(int kind, bool state, const GroupedArgs& G, void* stream) {
  const dim3 grid(group_blocks(G.n_chunks)), block(TH);
  hipStream_t st = (hipStream_t)stream;
  if (G.guard) {                                           // (SGD with a momentum buffer has no guarded form)
    if (kind == OPT_ADAM && state) hipLaunchKernelGGL((opt_groups_kernel<OPT_ADAM, true, true>), grid, block, 0, st, G);
    else if (kind == OPT_ADAM) hipLaunchKernelGGL((opt_groups_kernel<OPT_ADAM, false, true>), grid, block, 0, st, G);
    else hipLaunchKernelGGL((opt_groups_kernel<OPT_SGD, false, true>), grid, block, 0, st, G);
  } else if (kind == OPT_ADAM) {
    if (state) hipLaunchKernelGGL((opt_groups_kernel<OPT_ADAM, true>), grid, block, 0, st, G);
    else hipLaunchKernelGGL((opt_groups_kernel<OPT_ADAM, false>), grid, block, 0, st, G);
  } else {
    if (state) hipLaunchKernelGGL((opt_groups_kernel<OPT_SGD, true>), grid, block, 0, st, G);
    else hipLaunchKernelGGL((opt_groups_kernel<OPT_SGD, false>), grid, block, 0, st, G);
  }
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

bool groups_ok(int n_groups, int n_chunks) { return n_groups >= 1 && n_groups <= ACVAE_OPT_MAX_GROUPS && n_chunks > 0; }
}  // namespace

extern "C" int64_t acvae_opt_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int acvae_grad_norm_groups(const float* grads, const int* chunks, int n_chunks, int n_groups, float grad_scale,
                                      float* partials, float* group_norms, float* total_norm, void* stream) {
  if (!grads || !chunks || !partials || !group_norms || !total_norm || !groups_ok(n_groups, n_chunks)) return ACVAE_EINVAL;
  if (!aligned16(grads) || !aligned16(chunks)) return ACVAE_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sqsum_chunks_kernel, dim3(group_blocks(n_chunks)), dim3(TH), 0, st, grads, chunks, n_chunks, n_groups,
                     partials);
  hipLaunchKernelGGL(norm_groups_final_kernel, dim3(1), dim3(TH), 0, st, partials, chunks, n_chunks, n_groups, grad_scale,
                     group_norms, total_norm);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_adamw_groups_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                       float* max_exp_avg_sq, int64_t n, const int* chunks, int n_chunks, int n_groups,
                                       const double* lr, const double* beta1, const double* beta2, const double* eps,
                                       const double* weight_decay, int decoupled, int amsgrad, int64_t step,
                                       float grad_scale, float max_grad_norm, const float* total_norm, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || (amsgrad && !max_exp_avg_sq) || !chunks || !lr || !beta1 || !beta2 ||
      !eps || !weight_decay || n <= 0 || step <= 0 || !groups_ok(n_groups, n_chunks))
    return ACVAE_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
      (amsgrad && !aligned16(max_exp_avg_sq)) || !aligned16(chunks))
    return ACVAE_EALIGN;
  GroupedArgs G{};
  G.p = params; G.g = grads; G.s0 = exp_avg; G.s1 = exp_avg_sq; G.s2 = amsgrad ? max_exp_avg_sq : nullptr;
  G.n = (long)n; G.chunks = chunks; G.n_chunks = n_chunks; G.n_groups = n_groups;
  G.flags = decoupled ? OPT_F_DECOUPLED : 0;
  G.grad_scale = grad_scale; G.max_norm = max_grad_norm; G.total_norm = total_norm;
  for (int k = 0; k < n_groups; ++k) {                     // every derived scalar in double, rounded once (acvae_adamw_step)
    const double bc1 = 1.0 - pow(beta1[k], (double)step);
    const double bc2 = 1.0 - pow(beta2[k], (double)step);
    GroupHyper h{};
    h.lr = (float)lr[k];
    h.a = (float)(1.0 - beta1[k]); h.b = (float)beta2[k]; h.c = (float)(1.0 - beta2[k]); h.d = (float)eps[k];
    h.wd = (float)weight_decay[k]; h.decay = (float)(1.0 - lr[k] * weight_decay[k]);
    h.step_size = (float)(lr[k] / bc1); h.bc2_sqrt = (float)sqrt(bc2);
    G.hyper.add(h);
  }
  return launch_opt_groups(OPT_ADAM, amsgrad != 0, G, stream);
}

extern "C" int acvae_sgd_groups_step(float* params, const float* grads, float* momentum_buffer, int64_t n,
                                     const int* chunks, int n_chunks, int n_groups, const double* lr,
                                     const double* momentum, const double* weight_decay, double dampening, int nesterov,
                                     float grad_scale, float max_grad_norm, const float* total_norm, void* stream) {
  if (!params || !grads || !chunks || !lr || !momentum || !weight_decay || n <= 0 || !groups_ok(n_groups, n_chunks))
    return ACVAE_EINVAL;
  int with_mom = 0;
  for (int k = 0; k < n_groups; ++k) with_mom += momentum[k] != 0.0;
  if (with_mom != 0 && with_mom != n_groups) return ACVAE_EINVAL;     // the state exists for all groups or for none
  const bool mom = with_mom != 0;
  if ((mom && !momentum_buffer) || (nesterov && (!mom || dampening != 0.0))) return ACVAE_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned_or_null(mom ? momentum_buffer : nullptr) || !aligned16(chunks))
    return ACVAE_EALIGN;
  GroupedArgs G{};
  G.p = params; G.g = grads; G.s0 = mom ? momentum_buffer : nullptr;
  G.n = (long)n; G.chunks = chunks; G.n_chunks = n_chunks; G.n_groups = n_groups;
  G.flags = nesterov ? OPT_F_NESTEROV : 0;
  G.grad_scale = grad_scale; G.max_norm = max_grad_norm; G.total_norm = total_norm;
  for (int k = 0; k < n_groups; ++k) {
    GroupHyper h{};
    h.lr = (float)lr[k]; h.a = (float)momentum[k]; h.b = (float)(1.0 - dampening); h.wd = (float)weight_decay[k];
    G.hyper.add(h);
  }
  return launch_opt_groups(OPT_SGD, mom, G, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The non-finite guard (TrainStep(nonfinite="skip")): the decision whether an update is applied is formed on the device,
// where the norm lives, and kept in a caller-owned record (include/acvae_hip.h has its layout).  Three single-workgroup
// launches (witness, decide, and a restore that returns at once on an applied update) and guarded forms of the grouped
// update and the EMA that return before touching anything when the record says skip.  Every word of the record is stored by
// one thread with a vector store; no atomics.  Non-finite is a test of the exponent bits, so no floating-point mode bears
// on it.
// kernel-resource-usage (gfx950, -O3), VGPRs / SGPRs / LDS bytes: guard_witness_kernel 24 / 38 / 16, guard_decide_kernel
// 36 / 85 / 0, ema_guarded_kernel 26 / 28 / 0 (ema_kernel: 26 / 28 / 0), guard_restore_kernel 12 / 24 / 0,
// opt_groups_kernel<Adam, amsgrad, GUARD> 47 / 68 / 0, <Adam, GUARD> 40 / 62 / 0, <SGD, GUARD> 22 / 41 / 0; the four
// instantiations without GUARD keep the figures above.  No scratch, occupancy 8 waves per SIMD for all seven.
namespace {
__device__ __forceinline__ int nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(TH) void guard_witness_kernel(const float* __restrict__ loss, const float* __restrict__ buf,
                                                           long n, acvae_guard_record* __restrict__ rec) {
  __shared__ int bad_of_wave[TH / 64];
  int bad = 0;
  const long n4 = n >> 2;
  const float4* b4 = reinterpret_cast<const float4*>(buf);
  for (long i = threadIdx.x; i < n4; i += TH) {
    const float4 v = b4[i];
    bad |= nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
  }
  for (long i = (n4 << 2) + threadIdx.x; i < n; i += TH) bad |= nonfinite_bits(buf[i]);
  if (threadIdx.x == 0 && loss) bad |= nonfinite_bits(loss[0]);
  bad = __any(bad) ? 1 : 0;
  if ((threadIdx.x & 63) == 0) bad_of_wave[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    int any = 0;
    for (int w = 0; w < TH / 64; ++w) any |= bad_of_wave[w];
    if (any) rec->window_bad = 1;                          // an OR: a clean call leaves the flag as it found it
  }
}

struct DecideArgs {
  double lr[ACVAE_OPT_MAX_GROUPS], beta1[ACVAE_OPT_MAX_GROUPS], beta2[ACVAE_OPT_MAX_GROUPS];
  double ema_decay;
  int kind, n_groups, ema_warmup;
};

// One wavefront.  Every lane reads the record, the barrier puts those loads in front of every store, lane k < n_groups
// forms group k's scalars and lane 0 moves the counters.
__global__ __launch_bounds__(64) void guard_decide_kernel(acvae_guard_record* rec, const float* __restrict__ total_norm,
                                                          DecideArgs D) {
  const long applied = rec->applied, skipped = rec->skipped, streak = rec->streak, ema_updates = rec->ema_updates;
  const int window_bad = rec->window_bad;
  const int ok = !nonfinite_bits(total_norm[0]) && window_bad == 0;
  __syncthreads();
  const int lane = threadIdx.x;
  if (ok && D.kind == OPT_ADAM && lane < D.n_groups) {
    const double t = (double)(applied + 1);
    // (a select per group, not an index into the by-value arrays: they stay in scalar registers, no scratch)
    double lr = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll
    for (int k = 0; k < ACVAE_OPT_MAX_GROUPS; ++k)
      if (lane == k) { lr = D.lr[k]; b1 = D.beta1[k]; b2 = D.beta2[k]; }
    const double bc1 = 1.0 - pow(b1, t);
    const double bc2 = 1.0 - pow(b2, t);
    rec->step_size[lane] = (float)(lr / bc1);
    rec->bc2_sqrt[lane] = (float)sqrt(bc2);
  }
  if (lane == 0) {
    if (ok) {
      rec->applied = applied + 1;
      rec->streak = 0;
      if (D.ema_decay >= 0.0) {
        const double u = (double)ema_updates;
        const double warm = (1.0 + u) / (10.0 + u);
        const double d = D.ema_warmup && warm < D.ema_decay ? warm : D.ema_decay;
        rec->ema_w = (float)(1.0 - d);
        rec->ema_updates = ema_updates + 1;
      }
    } else {
      rec->skipped = skipped + 1;
      rec->streak = streak + 1;
    }
    rec->ok = ok;
    rec->window_bad = 0;
  }
}

__global__ __launch_bounds__(TH) void ema_guarded_kernel(float* __restrict__ ema, const float* __restrict__ p, long n,
                                                         const acvae_guard_record* __restrict__ rec) {
  if (rec->ok == 0) return;
  ema_body(ema, p, n, rec->ema_w);
}

__global__ __launch_bounds__(TH) void guard_restore_kernel(float* __restrict__ dst, const float* __restrict__ snap, long n,
                                                           const acvae_guard_record* __restrict__ rec) {
  if (rec->ok != 0) return;
  const long n4 = n >> 2;
  float4* d4 = reinterpret_cast<float4*>(dst);
  const float4* s4 = reinterpret_cast<const float4*>(snap);
  for (long i = blockIdx.x * (long)TH + threadIdx.x; i < n4; i += (long)gridDim.x * TH) d4[i] = s4[i];
  if (blockIdx.x == 0)
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += TH) dst[i] = snap[i];
}
}  // namespace

extern "C" int acvae_guard_witness(const float* loss, const float* buf, int64_t n_buf, acvae_guard_record* record,
                                   void* stream) {
  if (!record || n_buf < 0 || (!buf && n_buf > 0)) return ACVAE_EINVAL;
  if (!aligned16(record) || !aligned_or_null(buf)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(guard_witness_kernel, dim3(1), dim3(TH), 0, (hipStream_t)stream, loss, buf, buf ? (long)n_buf : 0L,
                     record);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_guard_decide(acvae_guard_record* record, const float* total_norm, int kind, int n_groups,
                                  const double* lr, const double* beta1, const double* beta2, double ema_decay,
                                  int ema_warmup, void* stream) {
  if (!record || !total_norm || !lr || (kind != OPT_ADAM && kind != OPT_SGD) || (kind == OPT_ADAM && (!beta1 || !beta2)) ||
      n_groups < 1 || n_groups > ACVAE_OPT_MAX_GROUPS || !(ema_decay <= 1.0))
    return ACVAE_EINVAL;
  if (!aligned16(record)) return ACVAE_EALIGN;
  DecideArgs D{};
  for (int k = 0; k < n_groups; ++k) {
    D.lr[k] = lr[k];
    if (kind == OPT_ADAM) { D.beta1[k] = beta1[k]; D.beta2[k] = beta2[k]; }
  }
  D.ema_decay = ema_decay; D.kind = kind; D.n_groups = n_groups; D.ema_warmup = ema_warmup != 0;
  hipLaunchKernelGGL(guard_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, record, total_norm, D);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_adamw_groups_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                               float* max_exp_avg_sq, int64_t n, const int* chunks, int n_chunks,
                                               int n_groups, const double* lr, const double* beta1, const double* beta2,
                                               const double* eps, const double* weight_decay, int decoupled, int amsgrad,
                                               float grad_scale, float max_grad_norm, const float* total_norm,
                                               const acvae_guard_record* record, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || (amsgrad && !max_exp_avg_sq) || !chunks || !lr || !beta1 || !beta2 ||
      !eps || !weight_decay || !record || n <= 0 || !groups_ok(n_groups, n_chunks))
    return ACVAE_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
      (amsgrad && !aligned16(max_exp_avg_sq)) || !aligned16(chunks) || !aligned16(record))
    return ACVAE_EALIGN;
  GroupedArgs G{};
  G.p = params; G.g = grads; G.s0 = exp_avg; G.s1 = exp_avg_sq; G.s2 = amsgrad ? max_exp_avg_sq : nullptr;
  G.n = (long)n; G.chunks = chunks; G.n_chunks = n_chunks; G.n_groups = n_groups;
  G.flags = decoupled ? OPT_F_DECOUPLED : 0;
  G.grad_scale = grad_scale; G.max_norm = max_grad_norm; G.total_norm = total_norm; G.guard = record;
  for (int k = 0; k < n_groups; ++k) {                     // as acvae_adamw_groups_step; step_size / bc2_sqrt are the record's
    GroupHyper h{};
    h.lr = (float)lr[k];
    h.a = (float)(1.0 - beta1[k]); h.b = (float)beta2[k]; h.c = (float)(1.0 - beta2[k]); h.d = (float)eps[k];
    h.wd = (float)weight_decay[k]; h.decay = (float)(1.0 - lr[k] * weight_decay[k]);
    G.hyper.add(h);
  }
  return launch_opt_groups(OPT_ADAM, amsgrad != 0, G, stream);
}

extern "C" int acvae_sgd_groups_step_guarded(float* params, const float* grads, int64_t n, const int* chunks, int n_chunks,
                                             int n_groups, const double* lr, const double* weight_decay, float grad_scale,
                                             float max_grad_norm, const float* total_norm,
                                             const acvae_guard_record* record, void* stream) {
  if (!params || !grads || !chunks || !lr || !weight_decay || !record || n <= 0 || !groups_ok(n_groups, n_chunks))
    return ACVAE_EINVAL;
  if (!aligned16(params) || !aligned16(grads) || !aligned16(chunks) || !aligned16(record)) return ACVAE_EALIGN;
  GroupedArgs G{};
  G.p = params; G.g = grads;
  G.n = (long)n; G.chunks = chunks; G.n_chunks = n_chunks; G.n_groups = n_groups;
  G.grad_scale = grad_scale; G.max_norm = max_grad_norm; G.total_norm = total_norm; G.guard = record;
  for (int k = 0; k < n_groups; ++k) {                     // as acvae_sgd_groups_step with momentum 0 (b is not read)
    GroupHyper h{};
    h.lr = (float)lr[k]; h.b = 1.f; h.wd = (float)weight_decay[k];
    G.hyper.add(h);
  }
  return launch_opt_groups(OPT_SGD, false, G, stream);
}

extern "C" int acvae_ema_step_guarded(float* ema, const float* params, int64_t n, const acvae_guard_record* record,
                                      void* stream) {
  if (!ema || !params || !record || n <= 0 || ranges_overlap(ema, params, n)) return ACVAE_EINVAL;
  if (!aligned16(ema) || !aligned16(params) || !aligned16(record)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(ema_guarded_kernel, dim3(flat_blocks(n)), dim3(TH), 0, (hipStream_t)stream, ema, params, (long)n,
                     record);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_guard_restore(float* dst, const float* snapshot, int64_t n, const acvae_guard_record* record,
                                   void* stream) {
  if (!dst || !snapshot || !record || n <= 0 || ranges_overlap(dst, snapshot, n)) return ACVAE_EINVAL;
  if (!aligned16(dst) || !aligned16(snapshot) || !aligned16(record)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(guard_restore_kernel, dim3(flat_blocks(n)), dim3(TH), 0, (hipStream_t)stream, dst, snapshot, (long)n,
                     record);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
