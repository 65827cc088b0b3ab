// Row gather and its adjoint, the ordered row fold: what lets one encoder pass serve all captions of a clip in the
// training step (Hybrid_VAEModel.forward(..., clip_index=)).  The encoder memory of B clips, R = S * C floats per clip, is
// gathered into the N caption rows on the way forward; on the way back the N rows' memory gradients are folded into their
// clips'.
//
// Both are pure data movement (the fold adds k rows per clip), so they are laid out for the memory system alone: one
// thread per float4 column chunk of a row (gather) or clip (fold), 16-byte loads and stores, consecutive lanes on
// consecutive chunks, a grid over (rows or clips) x chunk blocks.  The row numbers are uniform per workgroup.  The fold
// uses no atomics: a clip's chunk is owned by one thread, which adds the clip's rows in the order of the CSR list, so the
// sum is defined exactly and is bit-reproducible.
#include "common.h"
#include "../../include/acvae_hip.h"

namespace {
constexpr int ROWS_THREADS = 256;

__global__ __launch_bounds__(ROWS_THREADS) void rows_gather_kernel(const float* __restrict__ src, const int64_t* __restrict__ index,
                                                                   float* __restrict__ dst, int B, int chunks, int chunk_blocks) {
  const int row = blockIdx.x / chunk_blocks;
  const int chunk = (blockIdx.x - row * chunk_blocks) * ROWS_THREADS + threadIdx.x;
  if (chunk >= chunks) return;
  const int64_t clip = index[row];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (clip >= 0 && clip < B) v = load4(src + ((size_t)clip * chunks + chunk) * 4);      // a bad index reads nothing
  store4(dst + ((size_t)row * chunks + chunk) * 4, v);
}

__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
// chunk `chunk` of row r; a row number outside [0, N) contributes an exact zero instead of a read outside src
__device__ __forceinline__ float4 row_chunk(const float* __restrict__ src, int r, int N, int chunks, int chunk) {
  return (r >= 0 && r < N) ? load4(src + ((size_t)r * chunks + chunk) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(ROWS_THREADS) void rows_fold_kernel(const float* __restrict__ src, const int* __restrict__ offsets,
                                                                 const int* __restrict__ rows, float* __restrict__ dst, int N,
                                                                 int chunks, int chunk_blocks) {
  const int clip = blockIdx.x / chunk_blocks;
  const int chunk = (blockIdx.x - clip * chunk_blocks) * ROWS_THREADS + threadIdx.x;
  if (chunk >= chunks) return;
  const int lo = max(offsets[clip], 0), hi = min(offsets[clip + 1], N);      // `rows` holds N entries
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int j = lo;
  for (; j + 4 <= hi; j += 4) {            // four loads in flight, added in list order
    const float4 a = row_chunk(src, rows[j], N, chunks, chunk), b = row_chunk(src, rows[j + 1], N, chunks, chunk);
    const float4 c = row_chunk(src, rows[j + 2], N, chunks, chunk), d = row_chunk(src, rows[j + 3], N, chunks, chunk);
    add4(acc, a); add4(acc, b); add4(acc, c); add4(acc, d);
  }
  for (; j < hi; ++j) add4(acc, row_chunk(src, rows[j], N, chunks, chunk));
  store4(dst + ((size_t)clip * chunks + chunk) * 4, acc);
}

// blocks of the (rows x chunk blocks) grid, or -1 where it does not fit a launch
inline int64_t grid_blocks(int rows, int chunk_blocks) {
  const int64_t n = (int64_t)rows * chunk_blocks;
  return n > INT32_MAX ? -1 : n;
}
}  // namespace

extern "C" int acvae_rows_gather(const float* src, const int64_t* index, float* dst, int B, int N, int64_t R, void* stream) {
  if (!src || !index || !dst || B < 1 || N < 1 || R < 4 || R % 4 != 0 || R / 4 > INT32_MAX) return ACVAE_EINVAL;
  if (!aligned16(src) || !aligned16(dst)) return ACVAE_EALIGN;
  const int chunks = (int)(R / 4), chunk_blocks = cdiv(chunks, ROWS_THREADS);
  const int64_t blocks = grid_blocks(N, chunk_blocks);
  if (blocks < 0) return ACVAE_EINVAL;
  hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)blocks), dim3(ROWS_THREADS), 0, (hipStream_t)stream, src, index, dst, B,
                     chunks, chunk_blocks);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}

extern "C" int acvae_rows_fold(const float* src, const int* offsets, const int* rows, float* dst, int B, int N, int64_t R,
                               void* stream) {
  if (!src || !offsets || !rows || !dst || B < 1 || N < 1 || R < 4 || R % 4 != 0 || R / 4 > INT32_MAX) return ACVAE_EINVAL;
  if (!aligned16(src) || !aligned16(dst)) return ACVAE_EALIGN;
  const int chunks = (int)(R / 4), chunk_blocks = cdiv(chunks, ROWS_THREADS);
  const int64_t blocks = grid_blocks(B, chunk_blocks);
  if (blocks < 0) return ACVAE_EINVAL;
  hipLaunchKernelGGL(rows_fold_kernel, dim3((unsigned)blocks), dim3(ROWS_THREADS), 0, (hipStream_t)stream, src, offsets, rows, dst,
                     N, chunks, chunk_blocks);
  ACVAE_LAUNCH_CHECK();
  return ACVAE_OK;
}
