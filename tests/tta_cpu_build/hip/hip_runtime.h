// A stand-in for <hip/hip_runtime.h> that lets tests/test_tta_cpu_build.py compile csrc/tta.hip for the HOST: qualifiers vanish,
// __shared__ is a static array, a launch runs the blocks and their threads one after the other.  Good for kernels whose threads
// do not exchange data (the fp32 output of the TTA merge); with the uint8 output, whose rows go through LDS behind a
// __syncthreads(), only the addresses are meaningful (AddressSanitizer watches them), not the values.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)
struct dim3 { unsigned x, y, z; dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {} };
static dim3 threadIdx, blockIdx, blockDim;
using std::min; using std::max;
inline void __syncthreads() {}
typedef void* hipStream_t;
enum { hipSuccess = 0 };
inline int hipGetLastError() { return 0; }
#define hipLaunchKernelGGL(k, grid, block, shmem, st, ...) do { dim3 g_ = grid, b_ = block; blockDim = b_; \
  for (unsigned bx = 0; bx < g_.x; ++bx) for (unsigned tx = 0; tx < b_.x; ++tx) { blockIdx = dim3(bx); threadIdx = dim3(tx); k(__VA_ARGS__); } } while (0)
