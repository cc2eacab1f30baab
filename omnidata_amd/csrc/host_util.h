// host_util.h -- small host-side helpers shared by the two engines (engine.hip, unet_engine.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dptx {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline uint16_t f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                            // RNE
  return (uint16_t)(u >> 16);
}
// RNE in integer arithmetic: the bits of a `(_Float16)f` cast for every input that is not a NaN, and NaN -> NaN (checked over
// all 2^32 bit patterns).  Not the cast itself: inlined behind a double -> float conversion (the standardised convolution
// weights of pack_host) it packed other bits.
inline uint16_t f32_to_fp16(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (x >= 0x477ff000u) {  // >= 65520 rounds to inf
    return (uint16_t)(sign | 0x7c00u);
  }
  if (x < 0x38800000u) {  // subnormal half (|f| < 2^-14)
    if (x < 0x33000000u) return (uint16_t)sign;  // < 2^-25 -> 0
    const int e = (int)(x >> 23);                // biased exponent
    uint32_t m = (x & 0x7fffffu) | 0x800000u;    // 24-bit significand
    const int shift = 126 - e;                   // 14..24: result = m >> shift with RNE (units of 2^-24)
    const uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u);
    const uint32_t half = 1u << (shift - 1);
    uint32_t r = q;
    if (rem > half || (rem == half && (q & 1u))) r++;
    return (uint16_t)(sign | r);
  }
  uint32_t r = x - 0x38000000u;  // rebias exponent (127-15)<<23
  const uint32_t rem = r & 0x1fffu;
  r >>= 13;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
  return (uint16_t)(sign | r);
}

// Makes a handle's device current for the duration of a C entry point and restores the caller's device afterwards (a process
// that drives several GPUs keeps its own current device; torch.cuda.current_device() is not switched behind its back).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace dptx
