// Internal C++ launcher API of resnet.hip: the kernels the ResNet38 encoder adds to those of conv.hip (residual join,
// 1x1 downsample convolution, 2x2 average pool of raw activations).  Activations NHWC fp32, M = N*H*W pixels.
#pragma once
#include "conv.h"

namespace acvae {
// out = relu(y2*s2 + b2 + (yd ? yd*sd + bd : x))   (bn2, the downsample's BatchNorm, the identity; C % 4 == 0)
int res_join_fwd(const float* y2, const float* s2, const float* b2, const float* yd, const float* sd, const float* bd,
                 const float* x, float* out, long M, int C, hipStream_t st);
// Residual join backward, reduction pass: g = dO * (out > 0) is written to G and reduced into partial rows
// part2 = [rows][2][C] (sum g | sum g*yhat2) and, where yd != nullptr, partd = [rows][2][C] (sum g | sum g*yhatd);
// yhat = (y - mean) * invstd.  rows = res_join_rows(M, C); C in {4 .. 1024}, 1024 % C == 0.
int res_join_rows(long M, int C);
int res_join_bwd_reduce(const float* dO, const float* out, const float* y2, const float* m2, const float* i2, const float* yd,
                        const float* md, const float* id, float* G, float* part2, float* partd, long M, int C, hipStream_t st);
// ... apply pass: dy = scale * (g - sum_g * invn - yhat * sum_gy * invn) for bn2 and (yd != nullptr) the downsample BN
// (invn = 1/M with batch statistics, 0 in evaluation mode)
int res_join_bwd_apply(const float* G, const float* y2, const float* s2, const float* m2, const float* i2, const float* sg2,
                       const float* sgy2, float* dy2, const float* yd, const float* sd, const float* md, const float* id,
                       const float* sgd, const float* sgyd, float* dyd, long M, int C, float invn, hipStream_t st);
// 1x1 convolution (bias-free): Y[m][co] = sum_ci X[m][ci] * W[co][ci]; partials (optional) = [conv1x1_rows(M)][2][Cout]
// sum y | sum y^2 (bn_finalize's input).  Cin % 16 == 0, Cout % 64 == 0.
int conv1x1_rows(long M);
int conv1x1_fwd(const float* X, const float* W, float* Y, float* partials, long M, int Cin, int Cout, hipStream_t st);
// dX[m][ci] (+)= sum_co dY[m][co] * W[co][ci]     (accumulate != 0: added to dX in place)
int conv1x1_dgrad(const float* dY, const float* W, float* dX, long M, int Cin, int Cout, int accumulate, hipStream_t st);
// dW[co][ci] = sum_m dY[m][co] * X[m][ci]: per-slice slabs, then a fixed-order sum over the slices
long conv1x1_wgrad_slab_floats(long M, int Cin, int Cout);
int conv1x1_wgrad(const float* dY, const float* X, float* dW, float* slab, long M, int Cin, int Cout, hipStream_t st);
// P[n,ho,wo,c] = dropout(avg_pool2x2(X)) (floors odd H / W; drop.p == 0: no dropout)
int avg_pool2(const float* X, float* P, int N, int H, int W, int C, DropoutSpec drop, hipStream_t st);
// pool: dX[n,h,w,c] = dP[n,h/2,w/2,c] * dropout * 0.25 (0 behind the last full window); !pool: dX = dP * dropout;
// plus add[n,h,w,c] where add != nullptr.  dX has the shape [N,H,W,C] in both cases.
int avg_pool2_bwd(const float* dP, const float* add, float* dX, int N, int H, int W, int C, int pool, DropoutSpec drop,
                  hipStream_t st);
// out_nchw[n,c,h,w] = x[n,h,w,c] > 0   (the residual ReLU's decisions, test aid)
int positive_mask(const float* x, uint8_t* out_nchw, int N, int H, int W, int C, hipStream_t st);
}  // namespace acvae
