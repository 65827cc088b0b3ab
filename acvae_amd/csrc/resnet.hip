// Kernels of the ResNet38 encoder (reference models/encoder.py:1014-1036 _ResnetBasicBlock, :1096-1167 _ResNet) that
// conv.hip does not have: the residual join (bn2 + identity / downsample BN + ReLU) forward and backward, the 1x1
// downsample convolution with its gradients, and the 2x2 average pool of raw activations.  fp32 throughout, NHWC,
// every reduction in a fixed order (no float atomics): bit-reproducible run to run.
#include "resnet.h"
#include "../../include/acvae_hip.h"

namespace {

inline int grid_of(long n) {
  long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// dropout multiplier (0 or 1/(1-p)) of the 4 channels c..c+3 at (n, h, w) of a [N,H,W,C] tensor whose quad index is idx4:
// the same draw as conv.hip's (Philox(seed, idx4, site), one word per channel) or an explicit keep-mask in NCHW order
__device__ __forceinline__ float4 drop_mul4(const DropoutSpec& d, long idx4, int n, int h, int w, int c, int H, int W, int C) {
  if (d.p <= 0.f) return make_float4(1.f, 1.f, 1.f, 1.f);
  const float k = 1.0f / (1.0f - d.p);
  if (d.mask) {
    const long b = (((long)n * C + c) * H + h) * W + w, cs = (long)H * W;
    return make_float4(d.mask[b] ? k : 0.f, d.mask[b + cs] ? k : 0.f, d.mask[b + 2 * cs] ? k : 0.f, d.mask[b + 3 * cs] ? k : 0.f);
  }
  const uint4 r = philox4x32(d.seed, (uint64_t)idx4, d.site);
  const float u = 1.0f / 16777216.0f;
  return make_float4((float)(r.x >> 8) * u >= d.p ? k : 0.f, (float)(r.y >> 8) * u >= d.p ? k : 0.f,
                     (float)(r.z >> 8) * u >= d.p ? k : 0.f, (float)(r.w >> 8) * u >= d.p ? k : 0.f);
}

// ------------------------------------------------------------------ residual join
__global__ __launch_bounds__(256) void res_join_fwd_kernel(const float* __restrict__ y2, const float* __restrict__ s2,
                                                           const float* __restrict__ b2, const float* __restrict__ yd,
                                                           const float* __restrict__ sd, const float* __restrict__ bd,
                                                           const float* __restrict__ x, float* __restrict__ out, long total,
                                                           int C4) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int c = (int)(i % C4) * 4;
    const float4 a = load4(y2 + 4 * i), sa = load4(s2 + c), ba = load4(b2 + c);
    float4 id;
    if (yd) {
      const float4 v = load4(yd + 4 * i), sv = load4(sd + c), bv = load4(bd + c);
      id = make_float4(v.x * sv.x + bv.x, v.y * sv.y + bv.y, v.z * sv.z + bv.z, v.w * sv.w + bv.w);
    } else {
      id = load4(x + 4 * i);
    }
    float4 o;
    o.x = fmaxf((a.x * sa.x + ba.x) + id.x, 0.f); o.y = fmaxf((a.y * sa.y + ba.y) + id.y, 0.f);
    o.z = fmaxf((a.z * sa.z + ba.z) + id.z, 0.f); o.w = fmaxf((a.w * sa.w + ba.w) + id.w, 0.f);
    store4(out + 4 * i, o);
  }
}

constexpr int RJ_PIX_PER_LANE = 32;
// Block = 256 threads = (C/4 channel quads) x (1024/C pixel lanes), each lane RJ_PIX_PER_LANE pixels; the lanes' sums are
// added in lane order.
__global__ __launch_bounds__(256) void res_join_bwd_reduce_kernel(const float* __restrict__ dO, const float* __restrict__ out,
                                                                  const float* __restrict__ y2, const float* __restrict__ m2,
                                                                  const float* __restrict__ i2, const float* __restrict__ yd,
                                                                  const float* __restrict__ md, const float* __restrict__ id,
                                                                  float* __restrict__ G, float* __restrict__ part2,
                                                                  float* __restrict__ partd, long M, int C) {
  __shared__ float red[12][256];
  const int C4 = C / 4, npl = 256 / C4;
  const int cq = threadIdx.x % C4, pl = threadIdx.x / C4;
  const int c = cq * 4;
  const long ppb = (long)npl * RJ_PIX_PER_LANE;
  const long p0 = (long)blockIdx.x * ppb;
  float s[4] = {0, 0, 0, 0}, q2[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};
  const float4 mu2 = load4(m2 + c), is2 = load4(i2 + c);
  float4 mud = make_float4(0.f, 0.f, 0.f, 0.f), isd = mud;
  if (yd) { mud = load4(md + c); isd = load4(id + c); }
  for (long p = p0 + pl; p < p0 + ppb && p < M; p += npl) {
    const long e = p * C + c;
    float4 g = load4(dO + e);
    const float4 o = load4(out + e);
    if (o.x <= 0.f) g.x = 0.f;
    if (o.y <= 0.f) g.y = 0.f;
    if (o.z <= 0.f) g.z = 0.f;
    if (o.w <= 0.f) g.w = 0.f;
    store4(G + e, g);
    const float4 y = load4(y2 + e);
    s[0] += g.x; s[1] += g.y; s[2] += g.z; s[3] += g.w;
    q2[0] += g.x * ((y.x - mu2.x) * is2.x); q2[1] += g.y * ((y.y - mu2.y) * is2.y);
    q2[2] += g.z * ((y.z - mu2.z) * is2.z); q2[3] += g.w * ((y.w - mu2.w) * is2.w);
    if (yd) {
      const float4 v = load4(yd + e);
      qd[0] += g.x * ((v.x - mud.x) * isd.x); qd[1] += g.y * ((v.y - mud.y) * isd.y);
      qd[2] += g.z * ((v.z - mud.z) * isd.z); qd[3] += g.w * ((v.w - mud.w) * isd.w);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[k][threadIdx.x] = s[k]; red[4 + k][threadIdx.x] = q2[k]; red[8 + k][threadIdx.x] = qd[k];
  }
  __syncthreads();
  if (threadIdx.x < C4) {
    float a[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < npl; ++j)
#pragma unroll
      for (int k = 0; k < 12; ++k) a[k] += red[k][j * C4 + threadIdx.x];
    float* o2 = part2 + (long)blockIdx.x * 2 * C;
#pragma unroll
    for (int k = 0; k < 4; ++k) { o2[c + k] = a[k]; o2[C + c + k] = a[4 + k]; }
    if (yd) {
      float* od = partd + (long)blockIdx.x * 2 * C;
#pragma unroll
      for (int k = 0; k < 4; ++k) { od[c + k] = a[k]; od[C + c + k] = a[8 + k]; }
    }
  }
}

__device__ __forceinline__ float4 bn_dy4(float4 g, float4 y, float4 sc, float4 mu, float4 is, float4 a, float4 b) {
  float4 o;
  o.x = sc.x * (g.x - a.x - ((y.x - mu.x) * is.x) * b.x);
  o.y = sc.y * (g.y - a.y - ((y.y - mu.y) * is.y) * b.y);
  o.z = sc.z * (g.z - a.z - ((y.z - mu.z) * is.z) * b.z);
  o.w = sc.w * (g.w - a.w - ((y.w - mu.w) * is.w) * b.w);
  return o;
}
__device__ __forceinline__ float4 scale4(float4 v, float k) { return make_float4(v.x * k, v.y * k, v.z * k, v.w * k); }

__global__ __launch_bounds__(256) void res_join_bwd_apply_kernel(
    const float* __restrict__ G, const float* __restrict__ y2, const float* __restrict__ s2, const float* __restrict__ m2,
    const float* __restrict__ i2, const float* __restrict__ sg2, const float* __restrict__ sgy2, float* __restrict__ dy2,
    const float* __restrict__ yd, const float* __restrict__ sd, const float* __restrict__ md, const float* __restrict__ id,
    const float* __restrict__ sgd, const float* __restrict__ sgyd, float* __restrict__ dyd, long total, int C4, float invn) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int c = (int)(i % C4) * 4;
    const float4 g = load4(G + 4 * i);
    store4(dy2 + 4 * i, bn_dy4(g, load4(y2 + 4 * i), load4(s2 + c), load4(m2 + c), load4(i2 + c), scale4(load4(sg2 + c), invn),
                               scale4(load4(sgy2 + c), invn)));
    if (yd)
      store4(dyd + 4 * i, bn_dy4(g, load4(yd + 4 * i), load4(sd + c), load4(md + c), load4(id + c), scale4(load4(sgd + c), invn),
                                 scale4(load4(sgyd + c), invn)));
  }
}

// ------------------------------------------------------------------ 1x1 convolution
// C[m][n] = (acc ? C[m][n] : 0) + sum_k A[m][k] * B(n, k), B(n, k) = TB ? Bm[k*Nn + n] : Bm[n*K + k].
// Tile 64 rows x 64 columns, K in steps of 16 through LDS; thread (tr, tc) = 4 rows x 4 columns.  Exact fp32 FMAs on the
// VALU: the downsamples are 6.3 of the 1500 GFLOP of a B=32, T=1000 forward, too few to pay for an MFMA tile layout.
// partials: per 64-row tile, sum y | sum y^2 of its rows for each column, tile-row sums added in a fixed order.
constexpr int G1_BM = 64, G1_BN = 64, G1_BK = 16;
template <bool TB>
__global__ __launch_bounds__(256) void conv1x1_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                      float* __restrict__ Cm, float* __restrict__ partials, long M, int K, int Nn,
                                                      int acc) {
  __shared__ float As[G1_BK][G1_BM + 4];
  __shared__ float Bs[G1_BK][G1_BN + 4];
  __shared__ float red[2][16][G1_BN];
  const int t = threadIdx.x, tr = t / 16, tc = t % 16;
  const long m0 = (long)blockIdx.x * G1_BM;
  const int n0 = blockIdx.y * G1_BN;
  float r[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += G1_BK) {
    {
      const int row = t / 4, k4 = (t % 4) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + row < M) v = load4(A + (m0 + row) * K + k0 + k4);
      As[k4][row] = v.x; As[k4 + 1][row] = v.y; As[k4 + 2][row] = v.z; As[k4 + 3][row] = v.w;
      if (TB) {
        const int k = t / 16, n4 = (t % 16) * 4;
        const float4 b = load4(Bm + (long)(k0 + k) * Nn + n0 + n4);
        Bs[k][n4] = b.x; Bs[k][n4 + 1] = b.y; Bs[k][n4 + 2] = b.z; Bs[k][n4 + 3] = b.w;
      } else {
        const int n = t / 4;
        const float4 b = load4(Bm + (long)(n0 + n) * K + k0 + k4);
        Bs[k4][n] = b.x; Bs[k4 + 1][n] = b.y; Bs[k4 + 2][n] = b.z; Bs[k4 + 3][n] = b.w;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < G1_BK; ++kk) {
      const float4 a = *reinterpret_cast<const float4*>(&As[kk][4 * tr]);
      const float4 b = *reinterpret_cast<const float4*>(&Bs[kk][4 * tc]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r[i][j] = fmaf(av[i], bv[j], r[i][j]);
    }
    __syncthreads();
  }
  float s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long m = m0 + 4 * tr + i;
    if (m < M) {
      float* c = Cm + m * Nn + n0 + 4 * tc;
      float4 o = make_float4(r[i][0], r[i][1], r[i][2], r[i][3]);
      if (acc) {
        const float4 p = load4(c);
        o = make_float4(p.x + o.x, p.y + o.y, p.z + o.z, p.w + o.w);
      }
      store4(c, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j] += r[i][j]; q[j] += r[i][j] * r[i][j]; }
    }
  }
  if (!partials) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[0][tr][4 * tc + j] = s[j]; red[1][tr][4 * tc + j] = q[j]; }
  __syncthreads();
  if (t < G1_BN) {
    float a = 0.f, b = 0.f;
    for (int i = 0; i < 16; ++i) { a += red[0][i][t]; b += red[1][i][t]; }
    float* o = partials + (long)blockIdx.x * 2 * Nn;
    o[n0 + t] = a;
    o[Nn + n0 + t] = b;
  }
}

// slab[z][co][ci] = sum over the rows of slice z of dY[m][co] * X[m][ci]; tile 64 co x 64 ci, rows 16 at a time
__global__ __launch_bounds__(256) void conv1x1_wgrad_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                            float* __restrict__ slab, long M, int Cin, int Cout, long rows) {
  __shared__ float Ds[G1_BK][G1_BM + 4];
  __shared__ float Xs[G1_BK][G1_BN + 4];
  const int t = threadIdx.x, tr = t / 16, tc = t % 16;
  const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
  const long mb = (long)blockIdx.z * rows;
  const long me = mb + rows < M ? mb + rows : M;
  float r[4][4] = {};
  for (long m = mb; m < me; m += G1_BK) {
    {
      const int k = t / 16, c4 = (t % 16) * 4;
      float4 d = make_float4(0.f, 0.f, 0.f, 0.f), x = d;
      if (m + k < me) { d = load4(dY + (m + k) * Cout + co0 + c4); x = load4(X + (m + k) * Cin + ci0 + c4); }
      *reinterpret_cast<float4*>(&Ds[k][c4]) = d;
      *reinterpret_cast<float4*>(&Xs[k][c4]) = x;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < G1_BK; ++kk) {
      const float4 a = *reinterpret_cast<const float4*>(&Ds[kk][4 * tr]);
      const float4 b = *reinterpret_cast<const float4*>(&Xs[kk][4 * tc]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r[i][j] = fmaf(av[i], bv[j], r[i][j]);
    }
    __syncthreads();
  }
  float* o = slab + (long)blockIdx.z * Cout * Cin;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    store4(o + (long)(co0 + 4 * tr + i) * Cin + ci0 + 4 * tc, make_float4(r[i][0], r[i][1], r[i][2], r[i][3]));
}

__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ slab, int nz, long n, float* __restrict__ out) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    float a = 0.f;
    for (int z = 0; z < nz; ++z) a += slab[(long)z * n + i];
    out[i] = a;
  }
}

// ------------------------------------------------------------------ 2x2 average pool of raw activations
__global__ __launch_bounds__(256) void avg_pool2_kernel(const float* __restrict__ X, float* __restrict__ P, int N, int H, int W,
                                                        int C, DropoutSpec drop) {
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const long total = (long)N * Ho * Wo * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int c4 = (int)(i % C4);
    long r = i / C4;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const float* x = X + ((((long)n * H + 2 * ho) * W + 2 * wo) * C + c4 * 4);
    const float4 a = load4(x), b = load4(x + C), c = load4(x + (long)W * C), d = load4(x + (long)W * C + C);
    const float4 m = drop_mul4(drop, i, n, ho, wo, c4 * 4, Ho, Wo, C);
    float4 o;       // F.avg_pool2d (sum / 4) then F.dropout
    o.x = ((a.x + b.x + c.x + d.x) * 0.25f) * m.x; o.y = ((a.y + b.y + c.y + d.y) * 0.25f) * m.y;
    o.z = ((a.z + b.z + c.z + d.z) * 0.25f) * m.z; o.w = ((a.w + b.w + c.w + d.w) * 0.25f) * m.w;
    store4(P + 4 * i, o);
  }
}

__global__ __launch_bounds__(256) void avg_pool2_bwd_kernel(const float* __restrict__ dP, const float* __restrict__ add,
                                                            float* __restrict__ dX, int N, int H, int W, int C, int pool,
                                                            DropoutSpec drop) {
  const int C4 = C / 4, Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const long total = (long)N * H * W * C4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int c4 = (int)(i % C4);
    long r = i / C4;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H);
    const int n = (int)(r / H);
    const int ho = pool ? h >> 1 : h, wo = pool ? w >> 1 : w;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ho < Ho && wo < Wo) {
      const long j = (((long)n * Ho + ho) * Wo + wo) * C4 + c4;
      const float4 m = drop_mul4(drop, j, n, ho, wo, c4 * 4, Ho, Wo, C);
      const float k = pool ? 0.25f : 1.f;
      v = load4(dP + 4 * j);
      v = make_float4((v.x * m.x) * k, (v.y * m.y) * k, (v.z * m.z) * k, (v.w * m.w) * k);
    }
    if (add) {
      const float4 a = load4(add + 4 * i);
      v = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
    }
    store4(dX + 4 * i, v);
  }
}

__global__ void positive_mask_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int N, int H, int W, int C) {
  const long total = (long)N * H * W * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long r = i / C;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H);
    const int n = (int)(r / H);
    out[(((long)n * C + c) * H + h) * W + w] = x[i] > 0.f ? 1 : 0;
  }
}

}  // namespace

namespace acvae {

int res_join_fwd(const float* y2, const float* s2, const float* b2, const float* yd, const float* sd, const float* bd,
                 const float* x, float* out, long M, int C, hipStream_t st) {
  if (!y2 || !s2 || !b2 || !out || (yd ? !sd || !bd : !x) || M <= 0 || C <= 0 || C % 4) return ACVAE_EINVAL;
  const long total = M * (C / 4);
  hipLaunchKernelGGL(res_join_fwd_kernel, dim3(grid_of(total)), dim3(256), 0, st, y2, s2, b2, yd, sd, bd, x, out, total, C / 4);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

static bool rj_channels_ok(int C) { return C >= 4 && C <= 1024 && C % 4 == 0 && 1024 % C == 0; }
int res_join_rows(long M, int C) {
  if (!rj_channels_ok(C)) return 0;
  return cdiv(M, (long)(256 / (C / 4)) * RJ_PIX_PER_LANE);
}
int res_join_bwd_reduce(const float* dO, const float* out, const float* y2, const float* m2, const float* i2, const float* yd,
                        const float* md, const float* id, float* G, float* part2, float* partd, long M, int C, hipStream_t st) {
  if (!rj_channels_ok(C) || M <= 0) return ACVAE_EUNSUPPORTED;
  if (!dO || !out || !y2 || !m2 || !i2 || !G || !part2 || (yd && (!md || !id || !partd))) return ACVAE_EINVAL;
  hipLaunchKernelGGL(res_join_bwd_reduce_kernel, dim3(res_join_rows(M, C)), dim3(256), 0, st, dO, out, y2, m2, i2, yd, md, id, G,
                     part2, partd, M, C);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
int res_join_bwd_apply(const float* G, const float* y2, const float* s2, const float* m2, const float* i2, const float* sg2,
                       const float* sgy2, float* dy2, const float* yd, const float* sd, const float* md, const float* id,
                       const float* sgd, const float* sgyd, float* dyd, long M, int C, float invn, hipStream_t st) {
  if (M <= 0 || C <= 0 || C % 4) return ACVAE_EINVAL;
  if (!G || !y2 || !s2 || !m2 || !i2 || !sg2 || !sgy2 || !dy2 || (yd && (!sd || !md || !id || !sgd || !sgyd || !dyd)))
    return ACVAE_EINVAL;
  const long total = M * (C / 4);
  hipLaunchKernelGGL(res_join_bwd_apply_kernel, dim3(grid_of(total)), dim3(256), 0, st, G, y2, s2, m2, i2, sg2, sgy2, dy2, yd, sd,
                     md, id, sgd, sgyd, dyd, total, C / 4, invn);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

int conv1x1_rows(long M) { return cdiv(M, G1_BM); }
int conv1x1_fwd(const float* X, const float* W, float* Y, float* partials, long M, int Cin, int Cout, hipStream_t st) {
  if (!X || !W || !Y || M <= 0) return ACVAE_EINVAL;
  if (Cin % G1_BK || Cout % G1_BN || (long)cdiv(M, G1_BM) > 0x7fffffffL) return ACVAE_EUNSUPPORTED;
  if (!aligned16(X) || !aligned16(W) || !aligned16(Y)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(conv1x1_kernel<false>, dim3(cdiv(M, G1_BM), Cout / G1_BN), dim3(256), 0, st, X, W, Y, partials, M, Cin, Cout,
                     0);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
int conv1x1_dgrad(const float* dY, const float* W, float* dX, long M, int Cin, int Cout, int accumulate, hipStream_t st) {
  if (!dY || !W || !dX || M <= 0) return ACVAE_EINVAL;
  if (Cout % G1_BK || Cin % G1_BN) return ACVAE_EUNSUPPORTED;
  if (!aligned16(dY) || !aligned16(W) || !aligned16(dX)) return ACVAE_EALIGN;
  hipLaunchKernelGGL(conv1x1_kernel<true>, dim3(cdiv(M, G1_BM), Cin / G1_BN), dim3(256), 0, st, dY, W, dX, (float*)nullptr, M,
                     Cout, Cin, accumulate ? 1 : 0);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
// rows per slice: a multiple of 16, at least 256, at most 256 slices
static long wg1_rows(long M) {
  long r = cdiv(cdiv(M, 256), 16) * 16L;
  if (r < 256) r = 256;
  return r;
}
static int wg1_slices(long M) { return cdiv(M, wg1_rows(M)); }
long conv1x1_wgrad_slab_floats(long M, int Cin, int Cout) { return (long)wg1_slices(M) * Cin * Cout; }
int conv1x1_wgrad(const float* dY, const float* X, float* dW, float* slab, long M, int Cin, int Cout, hipStream_t st) {
  if (!dY || !X || !dW || !slab || M <= 0) return ACVAE_EINVAL;
  if (Cin % 64 || Cout % 64) return ACVAE_EUNSUPPORTED;
  if (!aligned16(dY) || !aligned16(X) || !aligned16(slab)) return ACVAE_EALIGN;
  const int nz = wg1_slices(M);
  hipLaunchKernelGGL(conv1x1_wgrad_kernel, dim3(Cin / 64, Cout / 64, nz), dim3(256), 0, st, dY, X, slab, M, Cin, Cout,
                     wg1_rows(M));
  ACVAE_LAUNCH_CHECK();
  const long n = (long)Cin * Cout;
  hipLaunchKernelGGL(slab_sum_kernel, dim3(grid_of(n)), dim3(256), 0, st, slab, nz, n, dW);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

int avg_pool2(const float* X, float* P, int N, int H, int W, int C, DropoutSpec drop, hipStream_t st) {
  if (!X || !P || N <= 0 || H < 2 || W < 2 || C <= 0 || C % 4) return ACVAE_EINVAL;
  const long total = (long)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(avg_pool2_kernel, dim3(grid_of(total)), dim3(256), 0, st, X, P, N, H, W, C, drop);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
int avg_pool2_bwd(const float* dP, const float* add, float* dX, int N, int H, int W, int C, int pool, DropoutSpec drop,
                  hipStream_t st) {
  if (!dP || !dX || N <= 0 || H < 1 || W < 1 || C <= 0 || C % 4 || (pool && (H < 2 || W < 2))) return ACVAE_EINVAL;
  const long total = (long)N * H * W * (C / 4);
  hipLaunchKernelGGL(avg_pool2_bwd_kernel, dim3(grid_of(total)), dim3(256), 0, st, dP, add, dX, N, H, W, C, pool ? 1 : 0, drop);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
int positive_mask(const float* x, uint8_t* out_nchw, int N, int H, int W, int C, hipStream_t st) {
  if (!x || !out_nchw || N <= 0 || H <= 0 || W <= 0 || C <= 0) return ACVAE_EINVAL;
  hipLaunchKernelGGL(positive_mask_kernel, dim3(grid_of((long)N * H * W * C)), dim3(256), 0, st, x, out_nchw, N, H, W, C);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

}  // namespace acvae

// =============================================================================================
// per-op C ABI (include/acvae_hip.h): each kernel alone, for the tests against fp64
// =============================================================================================
namespace {
inline DropoutSpec drop_of(float p, uint64_t seed, int site, const uint8_t* mask) {
  DropoutSpec d;
  d.p = p; d.mask = mask; d.seed = seed; d.site = (uint32_t)site;
  return d;
}
}  // namespace

extern "C" int acvae_res_join_fwd(const float* y2, const float* bn2, const float* yd, const float* bnd, const float* x,
                                  float* out, int N, int H, int W, int C, void* stream) {
  if (!bn2 || (yd && !bnd)) return ACVAE_EINVAL;
  return acvae::res_join_fwd(y2, bn2, bn2 + C, yd, yd ? bnd : nullptr, yd ? bnd + C : nullptr, x, out, (long)N * H * W, C,
                             (hipStream_t)stream);
}
extern "C" int64_t acvae_res_join_bwd_workspace_bytes(int N, int H, int W, int C) {
  const long rows = acvae::res_join_rows((long)N * H * W, C);
  if (rows <= 0) return -1;
  return (int64_t)(2 * rows * 2L * C + 2 * acvae::colsum_scratch_doubles(2 * C) + 64) * 4;
}
extern "C" int acvae_res_join_bwd(const float* dO, const float* out, const float* y2, const float* bn2, const float* yd,
                                  const float* bnd, float* G, float* dy2, float* dyd, float* dgamma2, float* dbeta2,
                                  float* dgammad, float* dbetad, int training, void* ws, int64_t ws_bytes, int N, int H, int W,
                                  int C, void* stream) {
  const int64_t need = acvae_res_join_bwd_workspace_bytes(N, H, W, C);
  if (need < 0) return ACVAE_EUNSUPPORTED;
  if (!ws || !bn2 || !dgamma2 || !dbeta2 || (yd && (!bnd || !dgammad || !dbetad))) return ACVAE_EINVAL;
  if (ws_bytes < need) return ACVAE_EWORKSPACE;
  if (!aligned16(ws)) return ACVAE_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)N * H * W;
  const int rows = acvae::res_join_rows(M, C);
  double* dpart = (double*)ws;
  float* part2 = (float*)ws + 2 * acvae::colsum_scratch_doubles(2 * C) + 64;
  float* partd = part2 + rows * 2L * C;
  ACVAE_TRY(acvae::colsum_tickets_reset(dpart, st));
  const float* bd = yd ? bnd : nullptr;
  ACVAE_TRY(acvae::res_join_bwd_reduce(dO, out, y2, bn2 + 2 * C, bn2 + 3 * C, yd, bd ? bd + 2 * C : nullptr,
                                       bd ? bd + 3 * C : nullptr, G, part2, partd, M, C, st));
  ACVAE_TRY(acvae::colsum2(part2, rows, 2 * C, dpart, dbeta2, dgamma2, C, st));
  if (yd) ACVAE_TRY(acvae::colsum2(partd, rows, 2 * C, dpart, dbetad, dgammad, C, st));
  return acvae::res_join_bwd_apply(G, y2, bn2, bn2 + 2 * C, bn2 + 3 * C, dbeta2, dgamma2, dy2, yd, bd, bd ? bd + 2 * C : nullptr,
                                   bd ? bd + 3 * C : nullptr, dbetad, dgammad, dyd, M, C, training ? 1.0f / (float)M : 0.f, st);
}
extern "C" int acvae_conv1x1_partials_rows(int N, int H, int W) { return acvae::conv1x1_rows((long)N * H * W); }
extern "C" int acvae_conv1x1_fwd(const float* X, const float* W_oi, float* Y, float* partials, int N, int H, int W, int Cin,
                                 int Cout, void* stream) {
  return acvae::conv1x1_fwd(X, W_oi, Y, partials, (long)N * H * W, Cin, Cout, (hipStream_t)stream);
}
extern "C" int acvae_conv1x1_dgrad(const float* dY, const float* W_oi, float* dX, int accumulate, int N, int H, int W, int Cin,
                                   int Cout, void* stream) {
  return acvae::conv1x1_dgrad(dY, W_oi, dX, (long)N * H * W, Cin, Cout, accumulate, (hipStream_t)stream);
}
extern "C" int64_t acvae_conv1x1_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
  return (int64_t)acvae::conv1x1_wgrad_slab_floats((long)N * H * W, Cin, Cout) * 4;
}
extern "C" int acvae_conv1x1_wgrad(const float* dY, const float* X, float* dW_oi, void* ws, int64_t ws_bytes, int N, int H, int W,
                                   int Cin, int Cout, void* stream) {
  if (ws_bytes < acvae_conv1x1_wgrad_workspace_bytes(N, H, W, Cin, Cout)) return ACVAE_EWORKSPACE;
  return acvae::conv1x1_wgrad(dY, X, dW_oi, (float*)ws, (long)N * H * W, Cin, Cout, (hipStream_t)stream);
}
extern "C" int acvae_avg_pool2_fwd(const float* X, float* P, int N, int H, int W, int C, float p_drop, uint64_t seed, int site,
                                   const uint8_t* mask, void* stream) {
  return acvae::avg_pool2(X, P, N, H, W, C, drop_of(p_drop, seed, site, mask), (hipStream_t)stream);
}
extern "C" int acvae_avg_pool2_bwd(const float* dP, const float* add, float* dX, int N, int H, int W, int C, int pool,
                                   float p_drop, uint64_t seed, int site, const uint8_t* mask, void* stream) {
  return acvae::avg_pool2_bwd(dP, add, dX, N, H, W, C, pool, drop_of(p_drop, seed, site, mask), (hipStream_t)stream);
}
