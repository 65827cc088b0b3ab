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

__global__ __launch_bounds__(TH) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float w) {
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
