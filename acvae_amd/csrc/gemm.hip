// Dense fp32 products on MFMA for the Linear layers of the path (attention projections, recurrent
// input/hidden projections, mean/log-variance heads, vocabulary classifier) and their gradients.
// Replaces torch.nn.Linear / F.linear at models/attn_model.py:32, models/decoder.py:198,
// models/text_encoder.py:192,255, models/vae_model.py:726 and the GEMMs inside nn.GRU / nn.LSTM.
#include <cstdint>
#include <cstdlib>
#include "mfma_tile.h"
#include "../../include/acvae_hip.h"
#include "conv.h"

namespace {
using namespace mfma;

template <int BN, bool VEC4>
__global__ __launch_bounds__(nt_threads<128>(), 2) void gemm_nt_kernel(const float* __restrict__ A, long lda,
                                                                     const float* __restrict__ B, long ldb,
                                                                     const float* __restrict__ bias,
                                                                     float* __restrict__ C, long ldc, int M, int N,
                                                                     int K, int accumulate) {
  __shared__ NtSmem<128, BN> sm;
  PlainLoader<VEC4, 4> al{A, lda, M, K};
  PlainLoader<VEC4, BN / 32> bl{B, ldb, N, K};
  PlainEpilogue ep{C, ldc, bias, accumulate};
  int bm, bn;
  xcd_tile(gridDim.x, gridDim.y, bm, bn);
  nt_block<128, BN>(al, bl, M, N, K, bm, bn, ep, sm);
}

template <int WM, int WN, bool VEC4>
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(const float* __restrict__ A, long lda,
                                                         const float* __restrict__ B, long ldb, float* __restrict__ C,
                                                         long ldc, int M, int N, int K, int k_per, int accumulate,
                                                         long slab_stride) {
  __shared__ TnSmem<WM, WN> sm;
  PlainKMajorLoader<VEC4> al{A, lda, M, K}, bl{B, ldb, N, K};
  const int kb = blockIdx.z * k_per;
  const int ke = min(K, kb + k_per);
  float* out = C + (long)blockIdx.z * slab_stride;
  tn_block<WM, WN>(al, bl, M, N, kb, ke, blockIdx.x, blockIdx.y, out, ldc, accumulate, sm);
}

// C[m][n] (+)= sum_z slab[z][m][n]   (fixed order: deterministic)
__global__ void slab_reduce_kernel(const float* __restrict__ slab, long slab_stride, int nsplit, float* __restrict__ C,
                                   long ldc, int M, int N, int accumulate) {
  const long total = (long)M * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / N), n = (int)(i % N);
    float acc = 0.f;
    for (int z = 0; z < nsplit; ++z) acc += slab[z * slab_stride + i];
    float* p = C + (long)m * ldc + n;
    *p = accumulate ? *p + acc : acc;
  }
}

// gemm_tn with the slab sum inside (the composite calls' form: 12 launches of slab_reduce_kernel per step): every K-slice
// writes its partial tile to its slab and takes a ticket of the TILE; the block that draws the last one sums the tile's slices
// IN SLICE ORDER - the arithmetic of slab_reduce_kernel, bit for bit - into C.  Hand-off without fences: the partial tile is
// stored write-through (sc1), drained (vmcnt(0)) in front of the barrier and the ticket, and read back with sc1 loads.  (With
// __threadfence() around the ticket - a write-back and an invalidate of the XCD's whole L2 per workgroup - the Winograd weight
// gradient running beside these products on the first stream lost 18 %: 0.55 -> 0.65 ms per launch, +0.8 ms per step.)
// Tickets: one word per output tile, zeroed once per composite call, reset by the reducer.
// One workgroup's share of such a product: slice z (of nsplit) of tile (bx, by), `tk` the tile's ticket
template <int WM, int WN, bool VEC4>
__device__ __forceinline__ void tn_fused_tile(const float* __restrict__ A, long lda, const float* __restrict__ B, long ldb,
                                              float* __restrict__ slab, float* __restrict__ C, long ldc, int M, int N, int K,
                                              int k_per, int accumulate, long slab_stride, unsigned* __restrict__ tk, int bx,
                                              int by, int z, int nsplit, TnSmem<WM, WN>& sm, int& s_last) {
  PlainKMajorLoader<VEC4> al{A, lda, M, K}, bl{B, ldb, N, K};
  const int kb = z * k_per;
  const int ke = min(K, kb + k_per);
  tn_block<WM, WN, true>(al, bl, M, N, kb, ke, bx, by, slab + (long)z * slab_stride, (long)N, 0, sm);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == (unsigned)nsplit - 1 ? 1 : 0;
    if (s_last) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  constexpr int TM = WM * 64, TN = WN * 64;
  const int m0 = bx * TM, n0 = by * TN;
  for (int i = threadIdx.x; i < TM * TN; i += 256) {
    const int m = m0 + i / TN, n = n0 + i % TN;
    if (m >= M || n >= N) continue;
    const long e = (long)m * N + n;
    float acc = 0.f;
    for (int z0 = 0; z0 < nsplit; z0 += 8) {          // eight loads in flight; the additions stay in slice order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = z0 + u < nsplit ? __hip_atomic_load(slab + (z0 + u) * slab_stride + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (z0 + u < nsplit) acc += v[u];
    }
    float* p = C + (long)m * ldc + n;
    *p = accumulate ? *p + acc : acc;
  }
}

template <int WM, int WN, bool VEC4>
__global__ __launch_bounds__(256, 2) void gemm_tn_fused_kernel(const float* __restrict__ A, long lda, const float* __restrict__ B,
                                                               long ldb, float* __restrict__ slab, float* __restrict__ C, long ldc,
                                                               int M, int N, int K, int k_per, int accumulate, long slab_stride,
                                                               unsigned* __restrict__ tickets) {
  __shared__ TnSmem<WM, WN> sm;
  __shared__ int s_last;
  tn_fused_tile<WM, WN, VEC4>(A, lda, B, ldb, slab, C, ldc, M, N, K, k_per, accumulate, slab_stride,
                              tickets + blockIdx.y * gridDim.x + blockIdx.x, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.z, sm,
                              s_last);
}

// Several of these products in ONE launch (conv.h: TnGroup).  A block finds its job from the flat block index and its place
// in the job's own grid (tile column fastest, then tile row, then slice); a sliced job then runs gemm_tn_fused_kernel's body on
// its own slabs and tickets, a job of one slice gemm_tn_kernel's, straight into C: each result is its own launch's, bit for bit.
__global__ __launch_bounds__(256, 2) void gemm_tn_group_kernel(TnGroup g, float* __restrict__ slabs,
                                                               unsigned* __restrict__ tickets) {
  __shared__ TnSmem<2, 2> sm;
  __shared__ int s_last;
  const int l = g.find((int)blockIdx.x);
  const TnJob& j = g.job[l];
  const int t = blockIdx.x - g.start[l];
  const int bx = t % j.gx, by = t / j.gx % j.gy, z = t / (j.gx * j.gy);
  if (j.slices == 1) {
    PlainKMajorLoader<true> al{j.A, j.lda, j.M, j.K}, bl{j.B, j.ldb, j.N, j.K};
    tn_block<2, 2>(al, bl, j.M, j.N, 0, j.K, bx, by, j.C, j.ldc, 0, sm);
    return;
  }
  tn_fused_tile<2, 2, true>(j.A, j.lda, j.B, j.ldb, slabs + j.slab0, j.C, j.ldc, j.M, j.N, j.K, j.k_per, 0, (long)j.M * j.N,
                            tickets + j.tk0 + by * j.gx + bx, bx, by, z, j.slices, sm, s_last);
}

// gridDim.z = S K-slices per output tile.  S == 1: the block owns the tile.  S > 1: every slice writes its partial
// tile to a slab and takes a ticket; the block that draws the last ticket sums the S slabs IN SLICE ORDER (so the
// result does not depend on which block was last: deterministic) and runs the epilogue.  Hand-off = the agent-scope
// release/acquire counter recipe of cdna_hip_programming.md §6 Guideline 16; the counter is reset by the reducer
// (and zeroed once per composite call by the host: acvae_skinny_ws_reset).
constexpr int SK_MAX_TILES = 1024;
template <bool VEC4>
__global__ __launch_bounds__(SK_THREADS) void gemm_skinny_kernel(const float* __restrict__ A1, long lda1,
                                                                 const float* __restrict__ B1, long ldb1, int K1,
                                                                 const float* __restrict__ A2, long lda2,
                                                                 const float* __restrict__ B2, long ldb2, int K2,
                                                                 const float* __restrict__ bias, float* __restrict__ C,
                                                                 long ldc, int M, int N, int accumulate,
                                                                 float* __restrict__ slabs, unsigned* __restrict__ cnt) {
  __shared__ float red[SK_WAVES][32][33];
  __shared__ int s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  const int S = gridDim.z, z = blockIdx.z;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // K-groups (of 8) are dealt round-robin to the S*8 (slice, wave) pairs
  sk_accumulate<VEC4>(acc, A1, lda1, B1, ldb1, M, N, K1, m0, n0, z * SK_WAVES + wave, S * SK_WAVES, li, lh);
  if (A2) sk_accumulate<VEC4>(acc, A2, lda2, B2, ldb2, M, N, K2, m0, n0, z * SK_WAVES + wave, S * SK_WAVES, li, lh);
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * lh][li] = acc[r];
  __syncthreads();
  const int tile = blockIdx.y * gridDim.x + blockIdx.x;
  float* my = slabs + ((long)tile * S + z) * 1024;
  // Split-K hand-off without fences (round 4; an agent release fence writes back the XCD's whole L2 and the acquire
  // invalidates the CU's L1 - measured on the column-sum kernel: 6-10 us per launch): the partial tile is stored write-through
  // (8-byte agent-scope atomic stores, `sc1`), every wave drains its stores, ONE lane takes the ticket behind the barrier, and
  // the block whose ticket came last reads all S partial tiles with agent-scope loads (`sc1`: never from its L1) - the first
  // row of MI355X_MICROARCH.md's table of hand-offs measured with `sc1` loads in place of the acquire.
  if (S > 1) {
    {
      const int e = threadIdx.x * 2;                 // SK_THREADS = 512: one pair of neighbours per thread
      float v0 = 0.f, v1 = 0.f;
#pragma unroll
      for (int w = 0; w < SK_WAVES; ++w) { v0 += red[w][e >> 5][e & 31]; v1 += red[w][e >> 5][(e & 31) + 1]; }
      const unsigned long long bits = (unsigned long long)__float_as_uint(v0) | ((unsigned long long)__float_as_uint(v1) << 32);
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(my + e), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned t = __hip_atomic_fetch_add(&cnt[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = (t == (unsigned)(S - 1));
      if (last) __hip_atomic_store(&cnt[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    // the S partial tiles in slice order, eight loads in flight
    const float* base = slabs + (long)tile * S * 1024;
    const int e = threadIdx.x * 2;
    float v0 = 0.f, v1 = 0.f;
    for (int q0 = 0; q0 < S; q0 += 8) {
      unsigned long long b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        b[u] = q0 + u < S ? __hip_atomic_load(reinterpret_cast<const unsigned long long*>(base + (long)(q0 + u) * 1024 + e),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (q0 + u < S) { v0 += __uint_as_float((unsigned)b[u]); v1 += __uint_as_float((unsigned)(b[u] >> 32)); }
    }
    const int mm = e >> 5, m = m0 + mm;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int n = n0 + (e & 31) + k;
      if (m < M && n < N) {
        float v = k ? v1 : v0;
        if (bias) v += bias[n];
        float* p = C + (long)m * ldc + n;
        if (accumulate) v += *p;
        *p = v;
      }
    }
    return;
  }
  for (int e = threadIdx.x; e < 1024; e += SK_THREADS) {
    const int mm = e >> 5, nn = e & 31;
    const int m = m0 + mm, n = n0 + nn;
    if (m < M && n < N) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < SK_WAVES; ++w) v += red[w][mm][nn];
      if (bias) v += bias[n];
      float* p = C + (long)m * ldc + n;
      if (accumulate) v += *p;
      *p = v;
    }
  }
}

__global__ void transpose_kernel(const float* __restrict__ in, long ld_in, float* __restrict__ out, long ld_out,
                                 int rows, int cols) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + threadIdx.x;
    tile[j][threadIdx.x] = (r < rows && c < cols) ? in[(long)r * ld_in + c] : 0.f;
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + threadIdx.x;
    if (r < rows && c < cols) out[(long)c * ld_out + r] = tile[threadIdx.x][j];
  }
}

__global__ void transpose_batch_kernel(TransposeBatch b) {
  __shared__ float tile[32][33];
  const int m = b.find((int)blockIdx.x);
  const TransposeJob& job = b.job[m];
  const int t = blockIdx.x - b.start[m];
  const int tcols = (job.cols + 31) / 32;
  const int c0 = (t % tcols) * 32, r0 = (t / tcols) * 32;
  const float* in = job.in;
  float* out = job.out;
  const int rows = job.rows, cols = job.cols;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + threadIdx.x;
    tile[j][threadIdx.x] = (r < rows && c < cols) ? in[(long)r * job.ld_in + c] : 0.f;
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + threadIdx.x;
    if (r < rows && c < cols) out[(long)c * job.ld_out + r] = tile[threadIdx.x][j];
  }
}

inline bool vec_ok(const float* p, int64_t ld, int k) { return aligned16(p) && (ld & 3) == 0 && (k & 3) == 0; }

}  // namespace

int acvae_transpose_batch(TransposeBatch& b, hipStream_t st) {
  if (!b.ok()) return ACVAE_EINVAL;
  if (b.n <= 0) return ACVAE_OK;
  for (int m = 0; m < b.n; ++m) {
    const TransposeJob& j = b.job[m];
    if (!j.in || !j.out || j.rows <= 0 || j.cols <= 0) return ACVAE_EINVAL;
  }
  const int tiles = b.seal([](const TransposeJob& j) { return cdiv(j.cols, 32) * cdiv(j.rows, 32); });
  hipLaunchKernelGGL(transpose_batch_kernel, dim3(tiles), dim3(32, 8), 0, st, b);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// Internal C++ entry (also used by the composite encoder/decoder drivers).
long acvae_skinny_ws_floats() { return SK_MAX_TILES + (long)SK_MAX_TILES * 1024; }
long acvae_skinny_ticket_words() { return SK_MAX_TILES; }
int acvae_skinny_ws_reset(float* ws, hipStream_t st) {   // zero the ticket counters (first SK_MAX_TILES words)
  return hipMemsetAsync(ws, 0, SK_MAX_TILES * sizeof(unsigned), st) == hipSuccess ? ACVAE_OK : (int)hipGetLastError();
}

namespace {
// Two independent skinny products in ONE launch (no split-K): the x-tiles of the first, then those of the second.  For
// the serial decode steps, where two short-K products hang off the same input (h . W_att^T and h . W_hh^T in the decoder
// step): each kernel on such a chain lasts 7-20 us - its own load latency, not its work - so running the two side by
// side takes one kernel's time instead of two.  Each tile runs exactly the arithmetic of gemm_skinny_kernel with
// gridDim.z = 1 (long-K products gain more from the split-K path and stay separate).
struct SkProblem {
  const float* A; long lda;
  const float* B; long ldb;
  int K;
  const float* bias;
  float* C; long ldc;
  int N, accumulate;
};
template <bool VEC4>
__global__ __launch_bounds__(SK_THREADS) void gemm_skinny_pair_kernel(SkProblem p0, SkProblem p1, int nx0, int M) {
  __shared__ float red[SK_WAVES][32][33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const bool second = (int)blockIdx.x >= nx0;
  const SkProblem& p = second ? p1 : p0;
  const int n0 = ((int)blockIdx.x - (second ? nx0 : 0)) * 32, m0 = blockIdx.y * 32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  sk_accumulate<VEC4>(acc, p.A, p.lda, p.B, p.ldb, M, p.N, p.K, m0, n0, wave, SK_WAVES, li, lh);
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * lh][li] = acc[r];
  __syncthreads();
  for (int e = threadIdx.x; e < 1024; e += SK_THREADS) {
    const int mm = e >> 5, nn = e & 31;
    const int m = m0 + mm, n = n0 + nn;
    if (m < M && n < p.N) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < SK_WAVES; ++w) v += red[w][mm][nn];
      if (p.bias) v += p.bias[n];
      float* o = p.C + (long)m * p.ldc + n;
      if (p.accumulate) v += *o;
      *o = v;
    }
  }
}
}  // namespace

int acvae_gemm_nt_pair(const float* A0, int64_t lda0, const float* B0, int64_t ldb0, int K0, const float* bias0, float* C0,
                       int64_t ldc0, int N0, int acc0, const float* A1, int64_t lda1, const float* B1, int64_t ldb1, int K1,
                       const float* bias1, float* C1, int64_t ldc1, int N1, int acc1, int M, hipStream_t st) {
  if (!A0 || !B0 || !C0 || !A1 || !B1 || !C1 || M <= 0 || M > 64 || N0 <= 0 || N1 <= 0 || K0 <= 0 || K1 <= 0)
    return ACVAE_EINVAL;
  const bool vec = vec_ok(A0, lda0, K0) && vec_ok(B0, ldb0, K0) && vec_ok(A1, lda1, K1) && vec_ok(B1, ldb1, K1);
  const SkProblem p0{A0, lda0, B0, ldb0, K0, bias0, C0, ldc0, N0, acc0}, p1{A1, lda1, B1, ldb1, K1, bias1, C1, ldc1, N1, acc1};
  const int nx0 = cdiv(N0, 32);
  dim3 grid(nx0 + cdiv(N1, 32), cdiv(M, 32));
  if (vec) hipLaunchKernelGGL(gemm_skinny_pair_kernel<true>, grid, dim3(SK_THREADS), 0, st, p0, p1, nx0, M);
  else hipLaunchKernelGGL(gemm_skinny_pair_kernel<false>, grid, dim3(SK_THREADS), 0, st, p0, p1, nx0, M);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// The skinny dispatcher's plan: 0 = the 128-row tile kernel, else the split count S of the 32x32-tile kernel (1 = no split).
// The dispatcher and the plan query (acvae_gemm_nt_split_plan) both call it.
static int skinny_plan(int M, int N, int Ktot, bool dual, bool have_ws) {
  // The 128-row tile kernel needs >= ~100 workgroups to fill the chip; mid-sized products (M = N*Tc = 672 rows
  // against 512..2048 columns) would launch 24-96 of them and run 100-140 us, so they take the 32x32-tile kernel too.
  const long big_blocks = (long)cdiv(M, 128) * cdiv(N, N <= 64 ? 64 : 128);
  if (!(M <= 64 || dual || (big_blocks < 100 && M <= 4096))) return 0;
  const int tiles = cdiv(N, 32) * cdiv(M, 32);
  // split K over more workgroups when there are few tiles and K is long (the serial decode/BPTT steps)
  int S = 1;
  // Only the long-K, few-tile products of the BPTT steps gain: the release/acquire hand-off costs a few us
  // (measured: 48 tiles x K=512 went 6.8 -> 9.8 us with S=2, 16 tiles x K=2048 went 25 -> 13.7 us with S=8).
  if (have_ws && tiles <= 16 && Ktot >= 1024) {
    S = 128 / tiles;
    const int maxs = Ktot / 256;       // keep >= 256 k per slice
    if (S > maxs) S = maxs;
    if (S > 8) S = 8;
    if (S < 1) S = 1;
    if ((long)tiles * S > SK_MAX_TILES) S = 1;
  }
  return S;
}

int acvae_gemm_nt_dual(const float* A1, int64_t lda1, const float* B1, int64_t ldb1, int K1, const float* A2,
                       int64_t lda2, const float* B2, int64_t ldb2, int K2, const float* bias, float* C, int64_t ldc,
                       int M, int N, int accumulate, hipStream_t st, float* skws) {
  if (!A1 || !B1 || !C || M <= 0 || N <= 0 || K1 <= 0) return ACVAE_EINVAL;
  if (A2 && (!B2 || K2 <= 0)) return ACVAE_EINVAL;
  bool vec = vec_ok(A1, lda1, K1) && vec_ok(B1, ldb1, K1);
  if (A2) vec = vec && vec_ok(A2, lda2, K2) && vec_ok(B2, ldb2, K2);
  const int S = skinny_plan(M, N, K1 + (A2 ? K2 : 0), A2 != nullptr, skws != nullptr);
  if (S > 0) {
    dim3 grid(cdiv(N, 32), cdiv(M, 32), S);
    unsigned* cnt = (unsigned*)skws;
    float* slabs = skws ? skws + SK_MAX_TILES : nullptr;
    if (vec)
      hipLaunchKernelGGL(gemm_skinny_kernel<true>, grid, dim3(SK_THREADS), 0, st, A1, lda1, B1, ldb1, K1, A2, lda2, B2,
                         ldb2, K2, bias, C, ldc, M, N, accumulate, slabs, cnt);
    else
      hipLaunchKernelGGL(gemm_skinny_kernel<false>, grid, dim3(SK_THREADS), 0, st, A1, lda1, B1, ldb1, K1, A2, lda2,
                         B2, ldb2, K2, bias, C, ldc, M, N, accumulate, slabs, cnt);
    ACVAE_LAUNCH_CHECK();
    return ACVAE_OK;
  }
  const bool bn64 = (N <= 64);
  dim3 grid(cdiv(M, 128), cdiv(N, bn64 ? 64 : 128));
#define LAUNCH_NT(BN_, V_)                                                                                     \
  hipLaunchKernelGGL((gemm_nt_kernel<BN_, V_>), grid, dim3(nt_threads<128>()), 0, st, A1, lda1, B1, ldb1, bias, C, ldc, M, \
                     N, K1, accumulate)
  if (bn64) { if (vec) LAUNCH_NT(64, true); else LAUNCH_NT(64, false); }
  else      { if (vec) LAUNCH_NT(128, true); else LAUNCH_NT(128, false); }
#undef LAUNCH_NT
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, float* C,
                             int64_t ldc, int M, int N, int K, int accumulate, void* stream) {
  return acvae_gemm_nt_dual(A, lda, B, ldb, K, nullptr, 0, nullptr, 0, 0, bias, C, ldc, M, N, accumulate,
                            (hipStream_t)stream, nullptr);
}

static int tn_splits(int M, int N, int K) {
  const long tiles = (long)cdiv(M, 128) * cdiv(N, 128);
  // one round of workgroups (256 CUs, two blocks per CU would fit): these products run on the second stream beside the
  // MFMA-bound encoder backward, where more slices only mean more slab traffic (347 MB per step with the earlier target of
  // 1024 workgroups, 139 MB now) and a reduce launch for the three largest products that no longer need one
  int s = (int)(256 / (tiles > 0 ? tiles : 1));
  const int maxs = cdiv(K, 4 * BKT);  // at least 64 k per slice
  if (s > maxs) s = maxs;
  if (s < 1) s = 1;
  if (s > 256) s = 256;
  return s;
}

extern "C" int64_t acvae_gemm_tn_workspace_bytes(int M, int N, int K) {
  const int s = tn_splits(M, N, K);
  return s > 1 ? (int64_t)s * M * N * (int64_t)sizeof(float) : 0;
}

extern "C" int acvae_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
                             int N, int K, int accumulate, float* slab_ws, int64_t slab_ws_bytes, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return ACVAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int s = tn_splits(M, N, K);
  if (s > 1 && (!slab_ws || slab_ws_bytes < (int64_t)s * M * N * (int64_t)sizeof(float))) s = 1;
  int k_per = cdiv(cdiv(K, s), BKT) * BKT;
  s = cdiv(K, k_per);
  const bool vec = aligned16(A) && aligned16(B) && (lda & 3) == 0 && (ldb & 3) == 0 && (M & 3) == 0 && (N & 3) == 0;
  const bool narrow = (M <= 64);
  dim3 grid(cdiv(M, narrow ? 64 : 128), cdiv(N, narrow ? 256 : 128), s);
  float* out = s > 1 ? slab_ws : C;
  const long out_ld = s > 1 ? N : ldc;
  const long slab_stride = s > 1 ? (long)M * N : 0;
  const int acc_k = s > 1 ? 0 : accumulate;
#define LAUNCH_TN(WM_, WN_, V_)                                                                              \
  hipLaunchKernelGGL((gemm_tn_kernel<WM_, WN_, V_>), grid, dim3(256), 0, st, A, lda, B, ldb, out, out_ld, M, N, K, \
                     k_per, acc_k, slab_stride)
  if (narrow) { if (vec) LAUNCH_TN(1, 4, true); else LAUNCH_TN(1, 4, false); }
  else        { if (vec) LAUNCH_TN(2, 2, true); else LAUNCH_TN(2, 2, false); }
#undef LAUNCH_TN
  if (s > 1) {
    const long total = (long)M * N;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)),
                       dim3(256), 0, st, slab_ws, slab_stride, s, C, ldc, M, N, accumulate);
  }
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// The fused TN call's plan: the K-slices it launches (k_per k each); 1 = it falls back to acvae_gemm_tn without a workspace
// (one slice, or a workspace too small for the slabs, or more tiles than tickets).  The call and the plan query
// (acvae_gemm_tn_fused_plan) both use it.
static int tn_fused_slices(int M, int N, int K, bool have_ws, int64_t ws_bytes, int* k_per_out) {
  int s = tn_splits(M, N, K);
  const bool narrow = (M <= 64);
  const long tiles = (long)cdiv(M, narrow ? 64 : 128) * cdiv(N, narrow ? 256 : 128);
  if (s > 1 && (!have_ws || ws_bytes < (int64_t)TN_TICKETS * 4 + (int64_t)s * M * N * (int64_t)sizeof(float) ||
                tiles > TN_TICKETS))
    return 1;
  const int k_per = cdiv(cdiv(K, s), BKT) * BKT;
  s = cdiv(K, k_per);
  if (k_per_out) *k_per_out = k_per;
  return s;
}

// ws = [TN_TICKETS words of tickets (zeroed once per composite call) | slabs]
int acvae_gemm_tn_fused(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
                        int accumulate, float* ws, int64_t ws_bytes, hipStream_t st) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return ACVAE_EINVAL;
  int k_per = 0;
  const int s = tn_fused_slices(M, N, K, ws != nullptr, ws_bytes, &k_per);
  if (s <= 1) return acvae_gemm_tn(A, lda, B, ldb, C, ldc, M, N, K, accumulate, nullptr, 0, st);  // one slice per tile, no workspace
  const bool narrow = (M <= 64);
  dim3 grid(cdiv(M, narrow ? 64 : 128), cdiv(N, narrow ? 256 : 128), s);
  const bool vec = aligned16(A) && aligned16(B) && (lda & 3) == 0 && (ldb & 3) == 0 && (M & 3) == 0 && (N & 3) == 0;
  unsigned* tickets = reinterpret_cast<unsigned*>(ws);
  float* slab = ws + TN_TICKETS;
#define LAUNCH_TNF(WM_, WN_, V_)                                                                                        \
  hipLaunchKernelGGL((gemm_tn_fused_kernel<WM_, WN_, V_>), grid, dim3(256), 0, st, A, lda, B, ldb, slab, C, ldc, M, N, K, k_per, \
                     accumulate, (long)M * N, tickets)
  if (narrow) { if (vec) LAUNCH_TNF(1, 4, true); else LAUNCH_TNF(1, 4, false); }
  else        { if (vec) LAUNCH_TNF(2, 2, true); else LAUNCH_TNF(2, 2, false); }
#undef LAUNCH_TNF
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

bool acvae_gemm_tn_group_add(TnGroup& g, const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N,
                             int K) {
  if (!A || !B || !C || M <= 64 || N <= 0 || K <= 0) return false;                                       // (M <= 64: the 64 x 256 tile)
  if (!aligned16(A) || !aligned16(B) || (lda & 3) || (ldb & 3) || (M & 3) || (N & 3)) return false;      // the scalar loader
  g.add({A, lda, B, ldb, C, ldc, M, N, K, 0, 0, 0, 0, 0, 0});
  return true;
}

long acvae_gemm_tn_group_plan(TnGroup& g) {
  if (!g.ok()) return -1;
  long slab = 0;
  int tk = 0;
  for (int l = 0; l < g.n; ++l) {
    TnJob& j = g.job[l];
    j.k_per = 0;
    j.slices = tn_fused_slices(j.M, j.N, j.K, true, INT64_MAX, &j.k_per);   // the job's own call, given the workspace it asks for
    j.gx = cdiv(j.M, 128);
    j.gy = cdiv(j.N, 128);
    j.slab0 = 0;
    j.tk0 = 0;
    if (j.slices > 1) {
      j.slab0 = slab;
      slab += (long)j.slices * j.M * j.N;
      j.tk0 = tk;
      tk += j.gx * j.gy;
    }
  }
  if (tk > TN_TICKETS) return -1;
  g.seal([](const TnJob& j) { return j.gx * j.gy * j.slices; });
  return slab;
}

int acvae_gemm_tn_group(TnGroup& g, float* ws, int64_t ws_bytes, hipStream_t st) {
  if (!g.ok()) return ACVAE_EINVAL;
  if (g.n <= 0) return ACVAE_OK;
  const long slab = acvae_gemm_tn_group_plan(g);
  if (slab < 0 || (slab > 0 && (!ws || ws_bytes < ((int64_t)TN_TICKETS + slab) * (int64_t)sizeof(float)))) return ACVAE_EWORKSPACE;
  hipLaunchKernelGGL(gemm_tn_group_kernel, dim3(g.start[g.n]), dim3(256), 0, st, g, ws + TN_TICKETS,
                     reinterpret_cast<unsigned*>(ws));
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_transpose(const float* in, int64_t ld_in, float* out, int64_t ld_out, int rows, int cols,
                               void* stream) {
  if (!in || !out || rows <= 0 || cols <= 0) return ACVAE_EINVAL;
  hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(cols, 32), cdiv(rows, 32)), dim3(32, 8), 0, (hipStream_t)stream, in,
                     ld_in, out, ld_out, rows, cols);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

// ---- C entry points of the internal forms above, for tests: the composite drivers reach them only at their own shapes.
// reset_tickets = 1 zeroes the workspace's tickets in front of the launch (a composite driver's entry); 0 relies on every
// earlier reducer having left its ticket at zero.
extern "C" int64_t acvae_gemm_nt_splitk_workspace_bytes(void) { return acvae_skinny_ws_floats() * (int64_t)sizeof(float); }
extern "C" int acvae_gemm_nt_split_plan(int M, int N, int K1, int K2, int with_ws) {
  if (M <= 0 || N <= 0 || K1 <= 0 || K2 < 0) return ACVAE_EINVAL;
  return skinny_plan(M, N, K1 + K2, K2 > 0, with_ws != 0);
}
extern "C" int acvae_gemm_nt_dual_ws(const float* A1, int64_t lda1, const float* B1, int64_t ldb1, int K1, const float* A2,
                                     int64_t lda2, const float* B2, int64_t ldb2, int K2, const float* bias, float* C,
                                     int64_t ldc, int M, int N, int accumulate, float* ws, int64_t ws_bytes, int reset_tickets,
                                     void* stream) {
  if (!A1 || !B1 || !C || M <= 0 || N <= 0 || K1 <= 0 || (A2 && (!B2 || K2 <= 0))) return ACVAE_EINVAL;
  if (ws && ws_bytes < acvae_gemm_nt_splitk_workspace_bytes()) return ACVAE_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (ws && reset_tickets) ACVAE_TRY(acvae_skinny_ws_reset(ws, st));
  return acvae_gemm_nt_dual(A1, lda1, B1, ldb1, K1, A2, lda2, B2, ldb2, K2, bias, C, ldc, M, N, accumulate, st, ws);
}
extern "C" int acvae_gemm_nt_pair_c(const float* A0, int64_t lda0, const float* B0, int64_t ldb0, int K0, const float* bias0,
                                    float* C0, int64_t ldc0, int N0, int acc0, const float* A1, int64_t lda1, const float* B1,
                                    int64_t ldb1, int K1, const float* bias1, float* C1, int64_t ldc1, int N1, int acc1, int M,
                                    void* stream) {
  return acvae_gemm_nt_pair(A0, lda0, B0, ldb0, K0, bias0, C0, ldc0, N0, acc0, A1, lda1, B1, ldb1, K1, bias1, C1, ldc1, N1,
                            acc1, M, (hipStream_t)stream);
}
extern "C" int64_t acvae_gemm_tn_fused_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return -1;
  const int s = tn_splits(M, N, K);
  return s > 1 ? (int64_t)TN_TICKETS * 4 + (int64_t)s * M * N * (int64_t)sizeof(float) : 0;
}
extern "C" int acvae_gemm_tn_fused_plan(int M, int N, int K, int64_t ws_bytes) {
  if (M <= 0 || N <= 0 || K <= 0) return ACVAE_EINVAL;
  return tn_fused_slices(M, N, K, ws_bytes > 0, ws_bytes, nullptr);
}
extern "C" int acvae_gemm_tn_fused_c(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
                                     int N, int K, int accumulate, float* ws, int64_t ws_bytes, int reset_tickets,
                                     void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return ACVAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (ws && reset_tickets && ws_bytes >= (int64_t)TN_TICKETS * 4)
    if (hipMemsetAsync(ws, 0, TN_TICKETS * sizeof(unsigned), st) != hipSuccess) return (int)hipGetLastError();
  return acvae_gemm_tn_fused(A, lda, B, ldb, C, ldc, M, N, K, accumulate, ws, ws_bytes, st);
}

// the grouped form: n jobs as host arrays (A / B / C: device pointers); ws = tickets | the slabs of every sliced job
static int tn_group_shapes(int n, const int* M, const int* N, const int* K, TnGroup& g) {
  if (n <= 0 || n > TnGroup::capacity || !M || !N || !K) return ACVAE_EINVAL;
  const float* none = reinterpret_cast<const float*>(16);       // (a placeholder that passes the checks: never dereferenced)
  for (int l = 0; l < n; ++l)
    if (!acvae_gemm_tn_group_add(g, none, 4, none, 4, const_cast<float*>(none), 4, M[l], N[l], K[l])) return ACVAE_EINVAL;
  return ACVAE_OK;
}
extern "C" int64_t acvae_gemm_tn_group_workspace_bytes(int n, const int* M, const int* N, const int* K) {
  TnGroup g;
  if (tn_group_shapes(n, M, N, K, g) != ACVAE_OK) return -1;
  const long slab = acvae_gemm_tn_group_plan(g);
  if (slab < 0) return -1;
  return slab > 0 ? ((int64_t)TN_TICKETS + slab) * (int64_t)sizeof(float) : 0;
}
extern "C" int acvae_gemm_tn_group_c(int n, const void* const* A, const int64_t* lda, const void* const* B, const int64_t* ldb,
                                     const void* const* C, const int64_t* ldc, const int* M, const int* N, const int* K, void* ws,
                                     int64_t ws_bytes, int reset_tickets, void* stream) {
  TnGroup g;
  if (n <= 0 || n > TnGroup::capacity || !A || !lda || !B || !ldb || !C || !ldc || !M || !N || !K) return ACVAE_EINVAL;
  for (int l = 0; l < n; ++l)
    if (ldc[l] < N[l] || lda[l] < M[l] || ldb[l] < N[l] ||
        !acvae_gemm_tn_group_add(g, (const float*)A[l], lda[l], (const float*)B[l], ldb[l], (float*)C[l], ldc[l], M[l], N[l], K[l]))
      return ACVAE_EINVAL;
  const long slab = acvae_gemm_tn_group_plan(g);
  if (slab < 0 || (slab > 0 && (!ws || ws_bytes < ((int64_t)TN_TICKETS + slab) * (int64_t)sizeof(float)))) return ACVAE_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (ws && reset_tickets && ws_bytes >= (int64_t)TN_TICKETS * 4)
    if (hipMemsetAsync(ws, 0, TN_TICKETS * sizeof(unsigned), st) != hipSuccess) return (int)hipGetLastError();
  return acvae_gemm_tn_group(g, (float*)ws, ws_bytes, st);
}
