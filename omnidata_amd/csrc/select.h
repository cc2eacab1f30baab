// select.h -- what refocus.hip, midas_loss.hip and vnl_loss.hip share: order-preserving fp32 keys, the single-rank 8-bit radix
// select step, fixed-order fp64 sums, and the host-side shape limits and block split.
//
// This header holds integer code and fp64 additions only: nothing a floating-point contraction could fuse.  It therefore
// carries NO `#pragma clang fp contract` (midas_loss.hip and vnl_loss.hip switch contraction off for their whole unit,
// refocus.hip only inside its *_rn helpers; a pragma leaking out of here would change refocus's bits).  Keep it that way: a
// multiplication next to an addition does not belong here.
//
// The select: NPASS passes, most significant digit first.  Pass q histograms digit q of the keys whose higher digits equal
// the prefix selected so far; every block of pass q >= 1 derives that prefix itself from pass q - 1's histogram
// (select_state -> resolve: an inclusive scan, exactly one bin holds the rank) and block 0 records it.  After the last
// pass the prefix is the key of the rank-th smallest value and the rank left is its position among the keys equal to it.
// Integer counts only, so the result does not depend on the order of the atomics that built the histograms.
// refocus.hip's multi-rank select (up to 64 ranks per pass) answers a different question and takes only the keys from here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace dptx {

constexpr int BINS = 256;  // 8-bit digits, 4 passes
constexpr int NPASS = 4;

// ---------------------------------------------------------------- host: shape limits, grids, launch check
constexpr int MAX_SIDE = 8192;
constexpr int64_t MAX_HW = 1ll << 24;
constexpr int MAX_GRID_Y = 65535;

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

inline bool launch_ok() { return hipGetLastError() == hipSuccess; }

// grid.y of the kernels that stride over the batch
inline int grid_y(int B) { return B < MAX_GRID_Y ? B : MAX_GRID_Y; }

// `total` items over at most `max_blocks` blocks of at least `per` items each, evenly -> nblk blocks of per_block items
inline void split(int64_t total, int64_t per, int64_t max_blocks, int64_t& nblk, int64_t& per_block) {
  nblk = std::min<int64_t>((total + per - 1) / per, max_blocks);
  per_block = (total + nblk - 1) / nblk;
}

// ---------------------------------------------------------------- device
// order-preserving keys; -0.0 and +0.0 are one key (that of +0.0)
__device__ __forceinline__ uint32_t f2key(float f) {
  uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// inclusive scan, in place, of NA rows of BINS LDS counters by a block of BINS threads (thread t owns column t; the caller
// has written the rows and need not have synchronised)
template <int NA>
__device__ __forceinline__ void block_scan256(uint32_t (*sc)[BINS]) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int off = 1; off < BINS; off <<= 1) {
    uint32_t v[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) v[a] = t >= off ? sc[a][t - off] : 0u;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NA; ++a) sc[a][t] += v[a];
    __syncthreads();
  }
}

// The digit of one pass of the rank-th key (among the keys with the prefix selected before that pass) of NA arrays at once:
// inclusive scan of the pass's histograms.  pre / rank: in = state before the pass, out = state after it (prefix << 8 |
// digit, rank left).  An array without keys (!has) keeps prefix << 8 and rank 0.
template <int NA>
__device__ __forceinline__ void resolve(const uint32_t* __restrict__ h /*[NA][BINS]*/, uint32_t (*sc)[BINS] /*LDS [NA]*/,
                                        uint32_t* res /*LDS [2 NA]*/, const bool (&has)[NA], uint32_t (&pre)[NA],
                                        uint32_t (&rank)[NA]) {
  const int t = threadIdx.x;
  uint32_t hv[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    hv[a] = h[a * BINS + t];
    sc[a][t] = hv[a];
  }
  if (t < NA) {
    res[2 * t] = pre[t] << 8;
    res[2 * t + 1] = 0;
  }
  block_scan256<NA>(sc);
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const uint32_t inc = sc[a][t], ex = inc - hv[a];
    if (has[a] && ex <= rank[a] && rank[a] < inc) {  // exactly one bin holds the rank
      res[2 * a] = (pre[a] << 8) | (uint32_t)t;
      res[2 * a + 1] = rank[a] - ex;
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    pre[a] = res[2 * a];
    rank[a] = res[2 * a + 1];
  }
  __syncthreads();
}

// The select state before pass q (1 <= q <= NPASS), derived from pass q - 1's histogram; block 0 records it.
// hist [NPASS][NA][BINS] and state [NPASS + 1][NA][2] (prefix, rank left) are those of one select (one image);
// rank0: the rank looked for, read only at q == 1.
template <int NA>
__device__ __forceinline__ void select_state(const uint32_t* __restrict__ hist, uint32_t* state, int q, uint32_t (*sc)[BINS],
                                             uint32_t* res, const bool (&has)[NA], const uint32_t (&rank0)[NA], uint32_t (&pre)[NA],
                                             uint32_t (&rank)[NA]) {
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    pre[a] = q == 1 ? 0u : state[((q - 1) * NA + a) * 2];
    rank[a] = q == 1 ? rank0[a] : state[((q - 1) * NA + a) * 2 + 1];
  }
  resolve<NA>(hist + (q - 1) * NA * BINS, sc, res, has, pre, rank);
  if (blockIdx.x == 0 && threadIdx.x < NA) {
    state[(q * NA + threadIdx.x) * 2] = pre[threadIdx.x];
    state[(q * NA + threadIdx.x) * 2 + 1] = rank[threadIdx.x];
  }
}

// sum of v over the wave in a fixed order (a __shfl_down tree); the total is in lane 0
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sums of NS fp64 values over the block (256 threads) in a fixed order -> dst[0 .. NS)
template <int NS>
__device__ __forceinline__ void block_sum(double (&v)[NS], double* red /*LDS [4][NS]*/, double* dst) {
  const int t = threadIdx.x;
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = wave_sum(v[s]);
  if ((t & 63) == 0)
#pragma unroll
    for (int s = 0; s < NS; ++s) red[(t >> 6) * NS + s] = v[s];
  __syncthreads();
  if (t < NS) dst[t] = ((red[t] + red[NS + t]) + red[2 * NS + t]) + red[3 * NS + t];
  __syncthreads();
}

}  // namespace dptx
