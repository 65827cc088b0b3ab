// The per-element arithmetic of the BatchNorm + ReLU backward's apply pass, shared by the standalone apply kernels (conv.hip)
// and by the consumers that apply it while they gather their operand (conv1_first_bwd_kernel).  One expression in one place:
// the library is built with -ffp-contract=off, so it gives the same bits wherever it runs.
#pragma once
#include <hip/hip_runtime.h>

// the six per-channel constants of four consecutive channels: scale, shift, mean, invstd and a = sum_g / n, b = sum_gy / n
// (n = pixels of the batch; 0 for evaluation-mode BatchNorm, whose statistics do not depend on the batch)
struct BnBwdQuad { float4 sc, sh, mu, is, a, b; };

__device__ __forceinline__ BnBwdQuad bn_bwd_quad(const float* __restrict__ scale, const float* __restrict__ shift,
                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                 const float* __restrict__ sum_g, const float* __restrict__ sum_gy, int c,
                                                 float invn) {
  BnBwdQuad k;
  k.sc = *reinterpret_cast<const float4*>(scale + c); k.sh = *reinterpret_cast<const float4*>(shift + c);
  k.mu = *reinterpret_cast<const float4*>(mean + c); k.is = *reinterpret_cast<const float4*>(invstd + c);
  k.a = *reinterpret_cast<const float4*>(sum_g + c); k.b = *reinterpret_cast<const float4*>(sum_gy + c);
  k.a.x *= invn; k.a.y *= invn; k.a.z *= invn; k.a.w *= invn;
  k.b.x *= invn; k.b.y *= invn; k.b.z *= invn; k.b.w *= invn;
  return k;
}

// dZ = sc * (g - a - yhat * b), g = the upstream gradient where y * sc + sh > 0 (the ReLU passed it), else 0
__device__ __forceinline__ float bn_bwd_dz1(float y, float g, float sc, float sh, float mu, float is, float a, float b) {
  if (y * sc + sh <= 0.f) g = 0.f;
  return sc * (g - a - ((y - mu) * is) * b);
}
__device__ __forceinline__ float4 bn_bwd_dz(float4 y, float4 g, const BnBwdQuad& k) {
  return make_float4(bn_bwd_dz1(y.x, g.x, k.sc.x, k.sh.x, k.mu.x, k.is.x, k.a.x, k.b.x),
                     bn_bwd_dz1(y.y, g.y, k.sc.y, k.sh.y, k.mu.y, k.is.y, k.a.y, k.b.y),
                     bn_bwd_dz1(y.z, g.z, k.sc.z, k.sh.z, k.mu.z, k.is.z, k.a.z, k.b.z),
                     bn_bwd_dz1(y.w, g.w, k.sc.w, k.sh.w, k.mu.w, k.is.w, k.a.w, k.b.w));
}

// 1/n of the batch statistics (0: evaluation mode)
__host__ __device__ inline float bn_bwd_invn(int N, int H, int W, bool batch_stats) {
  return batch_stats ? 1.0f / (float)((long)N * H * W) : 0.f;
}

// everything a consumer needs to apply it to its operand: the saved BatchNorm input Y, its constants and the sums that the
// backward's reduction left in the parameter-gradient buffers (sum_g = d beta, sum_gy = d gamma)
struct BnBwdApply {
  const float* Y;
  const float* scale; const float* shift; const float* mean; const float* invstd;
  const float* sum_g; const float* sum_gy;
  float invn;
};
