// Idioms shared by the memory-bound kernels: the grid of a grid-stride pass, the per-dtype
// launch, the two-level sum (wave shuffle -> LDS -> one fp32 partial per block, then one block
// over the partials in float64; no atomics, so the same call gives the same bits) and the
// 16-byte grid-stride loop with its scalar tail.
#pragma once
#include "rdn_common.h"

#define RDN_STREAM ((hipStream_t)stream)

// blocks of a grid-stride pass over n items at per_block items per block, 1 .. cap
static inline int grid_for(int64_t n, int per_block, int cap = 8192) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

// most blocks of a partial-sum launch (rdn_reduce_workspace_size: two floats per block)
constexpr int kRedBlocks = 1024;

// the launch statement once, with T = bf16 or float by the dtype code of the C ABI
// (variadic: the commas of <<<...>>> split the statement into macro arguments)
#define RDN_LAUNCH_T(dtype, ...)                              \
  do {                                                        \
    if ((dtype) == RDN_BF16) { using T = bf16; __VA_ARGS__; } \
    else { using T = float; __VA_ARGS__; }                    \
  } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block step of K sums in a 256-thread block: after it sh[k][0..3] hold the four wave sums
// of v[k], for thread 0 to combine (the callers associate them differently, and fp32
// rounds differently for it, so the combination is theirs).
template <int K>
__device__ __forceinline__ void block_wave_sums(float (&v)[K], float (&sh)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
}
__device__ __forceinline__ void block_wave_sums(float v, float (&sh)[4]) {
  float a[1] = {v};
  block_wave_sums<1>(a, reinterpret_cast<float(&)[1][4]>(sh));
}

// Final pass of one 256-thread block over nb partials of K interleaved sums (part[K*i + k]):
// thread t adds slots t, t + 256, ... in float64, then a shared-memory tree with offsets
// 128 .. 1.  tot[] gets the K totals; true on thread 0, the one that writes the result.
template <int K, typename P>
__device__ __forceinline__ bool final_sums(const P* __restrict__ part, int nb, double (&tot)[K]) {
  __shared__ double sh[K][256];
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += part[(int64_t)K * i + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) tot[k] = sh[k][0];
  return threadIdx.x == 0;
}

// the K means of nb fp32 partials: out[k] = total k / count (anonymous namespace: a copy
// per translation unit, as every kernel of the library)
namespace {
template <int K>
__global__ __launch_bounds__(256) void mean_final_kernel(const float* __restrict__ part, int nb, double count,
                                                         float* __restrict__ out) {
  double tot[K];
  if (final_sums(part, nb, tot)) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = (float)(tot[k] / count);
  }
}
}  // namespace

// Grid-stride pass over n floats: unit(i) for each of the first n4 16-byte units, then
// elem(i) for the elements behind them.  tid / stride: the grid-stride geometry, read in
// the __global__ function itself (why: the note at adam_loop, optim.hip).
template <typename Unit, typename Elem>
__device__ __forceinline__ void vec4_loop(int64_t n, int64_t n4, int64_t tid, int64_t stride, Unit unit, Elem elem) {
  for (int64_t i = tid; i < n4; i += stride) unit(i);
  for (int64_t i = n4 * 4 + tid; i < n; i += stride) elem(i);
}

// The host half: n4 is count / 4 when every pointer is 16-byte aligned, else 0 (a view at
// an odd element offset); items is grid_for's argument (the units, or else the elements).
struct Vec4Plan {
  int64_t n4, items;
};
template <typename... P>
static inline Vec4Plan vec4_plan(int64_t count, const P*... ptrs) {
  const bool aligned = ((... | (uintptr_t)ptrs) & 15) == 0;
  const int64_t n4 = aligned ? count / 4 : 0;
  return {n4, aligned ? n4 + 3 : count};
}
