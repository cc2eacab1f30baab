// unet.hip -- kernels of the version-1 UNet (6 down / 6 up blocks, GroupNorm(8) behind every convolution): the small-channel
// 3x3 convolution on MFMA with the GroupNorm records in its epilogue, GroupNorm(8) statistics / apply (+ 2x2 max-pool, + the
// final 1x1 convolution), bilinear x2 (align_corners=False) into a channel slice, and the first layer's im2col.  NHWC 16-bit
// activations, fp32 arithmetic.  The op-level entry points (dptx_op_unet_*) are at the end.
#include <hip/hip_runtime.h>

#include "../../include/dptx.h"
#include "kernels.h"
#include "unet.h"

namespace dptx {

// ------------------------------------------------------------------------------------------------ small-channel 3x3 conv
// Block = 4 waves, tile = 8 rows x 32 columns of output pixels of one image; wave w owns rows 2w, 2w+1.
// LDS: the tile with its one-pixel halo for all Cin ([rows][cols][Cin + 8] halves: the 8-half pad spreads the 16-byte
// fragment reads of neighbouring pixels over the banks) and the layer's weights ([32 NB][taps*Cin + 8]).
// MFMA 32x32x16: M = 32 output channels (A = weights, lane: channel lane%32, k = 8*(lane/32)..+7), N = 32 pixels of one row
// (B = activations, lane: pixel lane%32, the same 8 k), k-block = (tap, 16 channels).  A lane ends up with 4 consecutive
// channels of one pixel per accumulator quad: 8-byte NHWC stores.
template <int CIN, int TAPS, int COUT>
struct UConvCfg {
  static constexpr int HALO = TAPS == 9 ? 1 : 0;
  static constexpr int ROWS = UNET_TILE_H + 2 * HALO, COLS = UNET_TILE_W + 2 * HALO;
  static constexpr int PS = CIN + 8;            // halves per staged pixel
  static constexpr int NB = COUT > 32 ? COUT / 32 : 1;
  static constexpr int WROWS = NB * 32;         // rows >= COUT are zero
  static constexpr int WS = TAPS * CIN + 8;     // halves per weight row
  static constexpr int QN = COUT >= 32 ? 4 : COUT / 8;  // accumulator quads (of 8 channels) that hold real channels
  static constexpr size_t TILE_BYTES = (size_t)ROWS * COLS * PS * 2;
  static constexpr size_t W_BYTES = (size_t)WROWS * WS * 2;
  static constexpr size_t RED_BYTES = (size_t)4 * NB * 16 * 2 * 4;  // [wave][channel pair][sum, sq]
  static constexpr size_t SMEM = TILE_BYTES + W_BYTES + RED_BYTES;
};

template <int DT, int CIN, int TAPS, int COUT>
__global__ __launch_bounds__(256) void unet_conv_small_kernel(UnetConvParams p) {
  using Cfg = UConvCfg<CIN, TAPS, COUT>;
  constexpr int HALO = Cfg::HALO, ROWS = Cfg::ROWS, COLS = Cfg::COLS, PS = Cfg::PS, NB = Cfg::NB, WS = Cfg::WS, QN = Cfg::QN;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* ts = (uint16_t*)smem;
  uint16_t* ws = (uint16_t*)(smem + Cfg::TILE_BYTES);
  float* red = (float*)(smem + Cfg::TILE_BYTES + Cfg::W_BYTES);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
  const int tiles_x = (p.W + UNET_TILE_W - 1) / UNET_TILE_W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, b = blockIdx.y;
  const int oy0 = ty * UNET_TILE_H, ox0 = tx * UNET_TILE_W;

  // ---- stage the tile (+ halo): 16-byte chunks of 8 channels; outside the image: zero (never the neighbouring image)
  {
    constexpr int CPP = CIN / 8;  // chunks per pixel
    const uint16_t* X = (const uint16_t*)p.X;
    for (int i = tid; i < ROWS * COLS * CPP; i += 256) {
      const int pix = i / CPP, ch = i - pix * CPP;
      const int r = pix / COLS, c = pix - r * COLS;
      const int gy = oy0 + r - HALO, gx = ox0 + c - HALO;
      u32x4_t v = {0u, 0u, 0u, 0u};
      if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W)
        v = *(const u32x4_t*)(X + (((long long)b * p.H + gy) * p.W + gx) * p.x_pix_stride + p.x_off + ch * 8);
      *(u32x4_t*)(ts + pix * PS + ch * 8) = v;
    }
    constexpr int CPR = TAPS * CIN / 8;  // chunks per weight row
    const uint16_t* Wt = (const uint16_t*)p.Wt;
    for (int i = tid; i < Cfg::WROWS * CPR; i += 256) {
      const int o = i / CPR, ch = i - o * CPR;
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (o < COUT) v = *(const u32x4_t*)(Wt + (long long)o * (TAPS * CIN) + ch * 8);
      *(u32x4_t*)(ws + o * WS + ch * 8) = v;
    }
  }
  __syncthreads();

  f32x16_t acc[2][NB];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[r][n][e] = 0.f;

#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap) {
    const int ky = TAPS == 9 ? tap / 3 : 0, kx = TAPS == 9 ? tap - 3 * (tap / 3) : 0;
#pragma unroll
    for (int cb = 0; cb < CIN / 16; ++cb) {
      const int kc = cb * 16 + lh * 8;
      u32x4_t a[NB], bv[2];
#pragma unroll
      for (int n = 0; n < NB; ++n) a[n] = *(const u32x4_t*)(ws + (n * 32 + lr) * WS + tap * CIN + kc);
#pragma unroll
      for (int r = 0; r < 2; ++r) bv[r] = *(const u32x4_t*)(ts + ((2 * wave + r + ky) * COLS + lr + kx) * PS + kc);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[r][n] = T16<DT>::mfma32(a[n], bv[r], acc[r][n]);
    }
  }

  // ---- epilogue: + bias, 16-bit store, GroupNorm(8) records of the stored (rounded) values
  uint16_t* Y = (uint16_t*)p.Y;
  const int gx = ox0 + lr;
  float s1[NB][QN][2], s2[NB][QN][2];
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int q = 0; q < QN; ++q) { s1[n][q][0] = s1[n][q][1] = 0.f; s2[n][q][0] = s2[n][q][1] = 0.f; }
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      const int ch = n * 32 + q * 8 + lh * 4;
      const float4 bq = *(const float4*)(p.bias + ch);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int gy = oy0 + 2 * wave + r;
        if (gy < p.H && gx < p.W) {
          const float v0 = acc[r][n][4 * q + 0] + bq.x, v1 = acc[r][n][4 * q + 1] + bq.y;
          const float v2 = acc[r][n][4 * q + 2] + bq.z, v3 = acc[r][n][4 * q + 3] + bq.w;
          uint2 o;
          o.x = T16<DT>::pack2(v0, v1);
          o.y = T16<DT>::pack2(v2, v3);
          *(uint2*)(Y + (((long long)b * p.H + gy) * p.W + gx) * COUT + ch) = o;
          // statistics of the STORED values: what the apply pass normalises, and an fp16 overflow shows up in the sums
          const float r0 = T16<DT>::tof((uint16_t)(o.x & 0xffffu)), r1 = T16<DT>::tof((uint16_t)(o.x >> 16));
          const float r2 = T16<DT>::tof((uint16_t)(o.y & 0xffffu)), r3 = T16<DT>::tof((uint16_t)(o.y >> 16));
          s1[n][q][0] += r0 + r1; s2[n][q][0] += r0 * r0 + r1 * r1;
          s1[n][q][1] += r2 + r3; s2[n][q][1] += r2 * r2 + r3 * r3;
        }
      }
    }
  if (p.gn_part == nullptr) return;
  // the 32 pixels of a row sit in the 32 lanes of one half-wave: butterfly inside the half, fixed order
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int q = 0; q < QN; ++q)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float a = s1[n][q][h], c = s2[n][q][h];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
        if (lr == 0) {
          const int pair = n * 16 + q * 4 + lh * 2 + h;  // channel / 2
          red[(wave * NB * 16 + pair) * 2 + 0] = a;
          red[(wave * NB * 16 + pair) * 2 + 1] = c;
        }
      }
  __syncthreads();
  if (tid < 8) {
    constexpr int PPG = COUT / 16;  // channel pairs per group
    float a = 0.f, c = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int j = 0; j < PPG; ++j) {
        a += red[(w * NB * 16 + tid * PPG + j) * 2 + 0];
        c += red[(w * NB * 16 + tid * PPG + j) * 2 + 1];
      }
    float2* out = (float2*)p.gn_part + ((long long)b * gridDim.x + blockIdx.x) * 8 + tid;
    *out = make_float2(a, c);
  }
}

bool unet_conv_small_supported(int Cin, int Cout, int taps) {
  if (taps == 1) return Cin == 32 && Cout == 16;
  if (taps != 9) return false;
  return (Cin == 16 && (Cout == 16 || Cout == 32)) || (Cin == 32 && (Cout == 32 || Cout == 64)) || (Cin == 48 && Cout == 16) ||
         (Cin == 96 && Cout == 32);
}

template <int DT, int CIN, int TAPS, int COUT>
static hipError_t launch_conv_cfg(const UnetConvParams& p, hipStream_t stream) {
  auto k = unet_conv_small_kernel<DT, CIN, TAPS, COUT>;
  constexpr size_t smem = UConvCfg<CIN, TAPS, COUT>::SMEM;
  static_assert(smem <= 160 * 1024, "tile + weights fit the CU's LDS");
  ensure_dyn_smem((const void*)k, smem);
  hipLaunchKernelGGL(k, dim3(unet_conv_tiles(p.H, p.W), p.B), dim3(256), smem, stream, p);
  return hipGetLastError();
}

template <int DT>
static hipError_t launch_conv_dt(const UnetConvParams& p, hipStream_t stream) {
  if (p.taps == 1) return launch_conv_cfg<DT, 32, 1, 16>(p, stream);
  if (p.Cin == 16 && p.Cout == 16) return launch_conv_cfg<DT, 16, 9, 16>(p, stream);
  if (p.Cin == 16 && p.Cout == 32) return launch_conv_cfg<DT, 16, 9, 32>(p, stream);
  if (p.Cin == 32 && p.Cout == 32) return launch_conv_cfg<DT, 32, 9, 32>(p, stream);
  if (p.Cin == 32 && p.Cout == 64) return launch_conv_cfg<DT, 32, 9, 64>(p, stream);
  if (p.Cin == 48 && p.Cout == 16) return launch_conv_cfg<DT, 48, 9, 16>(p, stream);
  if (p.Cin == 96 && p.Cout == 32) return launch_conv_cfg<DT, 96, 9, 32>(p, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_unet_conv_small(int mode, const UnetConvParams& p, hipStream_t stream) {
  if (!unet_conv_small_supported(p.Cin, p.Cout, p.taps) || p.B <= 0 || p.H <= 0 || p.W <= 0 || p.x_pix_stride % 8 != 0 ||
      p.x_off % 8 != 0 || p.x_off < 0 || p.x_off + p.Cin > p.x_pix_stride || p.B > 65535)
    return hipErrorInvalidValue;
  if (mode == MODE_BF16) return launch_conv_dt<DT_BF16>(p, stream);
  if (mode == MODE_FP16) return launch_conv_dt<DT_FP16>(p, stream);
  return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------ first layer: im2col
template <int DT>
__global__ __launch_bounds__(256) void unet_im2col3_kernel(const void* __restrict__ x, int io, uint16_t* __restrict__ P, int H, int W) {
  const int pix = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (pix >= H * W) return;
  const int y = pix / W, xx = pix - y * W;
  float v[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) v[k] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int gy = y + ky - 1, gx = xx + kx - 1;
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[(ky * 3 + kx) * 3 + c] = io_load(x, (((long long)b * 3 + c) * H + gy) * W + gx, io);
      }
    }
  uint16_t* dst = P + ((long long)b * H * W + pix) * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) *(uint4*)(dst + 8 * j) = pack8<DT>(v + 8 * j);
}

hipError_t launch_unet_im2col3(int mode, const void* x, int io, void* P, int B, int H, int W, hipStream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || io < 0 || io > 2) return hipErrorInvalidValue;
  dim3 grid((H * W + 255) / 256, B);
  if (mode == MODE_BF16) hipLaunchKernelGGL(unet_im2col3_kernel<DT_BF16>, grid, dim3(256), 0, stream, x, io, (uint16_t*)P, H, W);
  else if (mode == MODE_FP16) hipLaunchKernelGGL(unet_im2col3_kernel<DT_FP16>, grid, dim3(256), 0, stream, x, io, (uint16_t*)P, H, W);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ GroupNorm(8)
// statistics of a dense tensor: a thread owns 8 consecutive channels (4 channel pairs; a pair never straddles a group: C / 8 is
// even) of every px_par-th pixel of the block's chunk; the block then adds the pair sums of every group in a fixed order
constexpr int UNET_GN_ITERS = 16;
static inline int unet_gn_pxpar(int C) { return 256 / (C / 8); }
int unet_gn_chunks(int HW, int C) {
  const int chunk = unet_gn_pxpar(C) * UNET_GN_ITERS;
  return (HW + chunk - 1) / chunk;
}

template <int DT>
__global__ __launch_bounds__(256) void unet_gn_stats_kernel(const uint16_t* __restrict__ X, float2* __restrict__ partial, int HW, int C) {
  __shared__ float2 sred[256 * 4];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int TP = C >> 3, px_par = 256 / TP;
  const int slot = tid / TP, tc = tid - slot * TP;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (slot < px_par) {
    const int p0 = blockIdx.x * px_par * UNET_GN_ITERS;
    for (int it = 0; it < UNET_GN_ITERS; ++it) {
      const int pix = p0 + it * px_par + slot;
      if (pix < HW) {
        float f[8];
        unpack8<DT>(*(const uint4*)(X + ((long long)b * HW + pix) * C + tc * 8), f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s1[j] += f[2 * j] + f[2 * j + 1];
          s2[j] += f[2 * j] * f[2 * j] + f[2 * j + 1] * f[2 * j + 1];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sred[tid * 4 + j] = make_float2(s1[j], s2[j]);
  __syncthreads();
  if (tid < 8) {
    const int ppg = C >> 4;  // channel pairs per group
    float a = 0.f, c = 0.f;
    for (int s = 0; s < px_par; ++s)
      for (int j = 0; j < ppg; ++j) {
        const int pair = tid * ppg + j;  // channel / 2 -> thread pair / 4 of the slot, its pair % 4
        const float2 v = sred[(s * TP + (pair >> 2)) * 4 + (pair & 3)];
        a += v.x; c += v.y;
      }
    partial[((long long)b * gridDim.x + blockIdx.x) * 8 + tid] = make_float2(a, c);
  }
}

hipError_t launch_unet_gn_stats(int mode, const void* X, float* partial, int B, int HW, int C, hipStream_t stream) {
  if (C < 16 || C > 1024 || C % 16 != 0 || B <= 0 || HW <= 0 || B > 65535) return hipErrorInvalidValue;
  dim3 grid(unet_gn_chunks(HW, C), B);
  if (mode == MODE_BF16) hipLaunchKernelGGL(unet_gn_stats_kernel<DT_BF16>, grid, dim3(256), 0, stream, (const uint16_t*)X, (float2*)partial, HW, C);
  else if (mode == MODE_FP16) hipLaunchKernelGGL(unet_gn_stats_kernel<DT_FP16>, grid, dim3(256), 0, stream, (const uint16_t*)X, (float2*)partial, HW, C);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// one block per image, one wave per group: the records in double, lane-strided and then a butterfly (a fixed order)
__global__ __launch_bounds__(512) void unet_gn_finalize_kernel(const float2* __restrict__ partial, int nrec, float2* __restrict__ stats,
                                                               double inv_n, float eps, unsigned* __restrict__ flag) {
  const int b = blockIdx.x, g = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double s = 0.0, q = 0.0;
  for (int r = lane; r < nrec; r += 64) {
    const float2 v = partial[((long long)b * nrec + r) * 8 + g];
    s += (double)v.x; q += (double)v.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
  if (lane == 0) {
    const double mean = s * inv_n;
    double var = q * inv_n - mean * mean;
    if (!(var > 0.0)) var = 0.0;  // also a NaN: the flag below reports it
    stats[b * 8 + g] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)eps)));
    const float sf = (float)s, qf = (float)q;
    if (flag != nullptr && !(fabsf(sf) <= 3.0e38f && fabsf(qf) <= 3.0e38f)) atomicOr(flag, 1u);
  }
}

hipError_t launch_unet_gn_finalize(const float* partial, int nrec, float* stats, int B, int HW, int C, float eps, unsigned* flag,
                                   hipStream_t stream) {
  if (B <= 0 || nrec <= 0 || C % 8 != 0) return hipErrorInvalidValue;
  const double inv_n = 1.0 / ((double)HW * (double)(C / 8));
  hipLaunchKernelGGL(unet_gn_finalize_kernel, dim3(B), dim3(512), 0, stream, (const float2*)partial, nrec, (float2*)stats, inv_n, eps, flag);
  return hipGetLastError();
}

// scale / shift of a thread's 8 channels: y = x * a + c with a = rstd * gamma, c = beta - mean * a
__device__ __forceinline__ void unet_gn_coeffs(const float2* stats, const float* gamma, const float* beta, int b, int ch0, int cpg,
                                               float* a, float* c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float2 st = stats[b * 8 + (ch0 + j) / cpg];
    a[j] = st.y * gamma[ch0 + j];
    c[j] = __fmaf_rn(-st.x, a[j], beta[ch0 + j]);
  }
}

// a thread owns 8 channels of a 2x2 quad of pixels: relu(gn(x)) of the four, and their maximum for the pooled copy
template <int DT>
__global__ __launch_bounds__(256) void unet_gn_apply_kernel(UnetGnApply p) {
  const int TP = p.C >> 3, b = blockIdx.y;
  const int qw = (p.W + 1) >> 1, qh = (p.H + 1) >> 1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)qw * qh * TP) return;
  const int quad = (int)(i / TP), tc = (int)(i - (long long)quad * TP);
  const int qy = quad / qw, qx = quad - qy * qw;
  float a[8], c[8];
  unet_gn_coeffs((const float2*)p.stats, p.gamma, p.beta, b, tc * 8, p.C >> 3, a, c);
  const uint16_t* X = (const uint16_t*)p.X;
  uint16_t* Y = (uint16_t*)p.Y;
  float m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = 0.f;  // ReLU'd values are >= 0
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int y = 2 * qy + dy, x = 2 * qx + dx;
      if (y < p.H && x < p.W) {
        const long long pix = ((long long)b * p.H + y) * p.W + x;
        float f[8];
        unpack8<DT>(*(const uint4*)(X + pix * p.C + tc * 8), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f[j] = fmaxf(__fmaf_rn(f[j], a[j], c[j]), 0.f);
          m[j] = fmaxf(m[j], f[j]);
        }
        if (Y != nullptr) *(uint4*)(Y + pix * p.y_pix_stride + p.y_off + tc * 8) = pack8<DT>(f);
      }
    }
  if (p.P != nullptr)
    *(uint4*)((uint16_t*)p.P + (((long long)b * (p.H >> 1) + qy) * (p.W >> 1) + qx) * p.p_pix_stride + p.p_off + tc * 8) = pack8<DT>(m);
}

hipError_t launch_unet_gn_apply(int mode, const UnetGnApply& p, hipStream_t stream) {
  if (p.C < 16 || p.C > 1024 || p.C % 16 != 0 || p.B <= 0 || p.H <= 0 || p.W <= 0 || p.B > 65535) return hipErrorInvalidValue;
  if (p.Y == nullptr && p.P == nullptr) return hipErrorInvalidValue;
  if (p.Y != nullptr && (p.y_pix_stride % 8 != 0 || p.y_off % 8 != 0 || p.y_off < 0 || p.y_off + p.C > p.y_pix_stride)) return hipErrorInvalidValue;
  if (p.P != nullptr && (p.H % 2 != 0 || p.W % 2 != 0 || p.p_pix_stride % 8 != 0 || p.p_off % 8 != 0 || p.p_off < 0 ||
                         p.p_off + p.C > p.p_pix_stride))
    return hipErrorInvalidValue;
  const long long n = (long long)((p.W + 1) / 2) * ((p.H + 1) / 2) * (p.C / 8);
  dim3 grid((unsigned)((n + 255) / 256), p.B);
  if (mode == MODE_BF16) hipLaunchKernelGGL(unet_gn_apply_kernel<DT_BF16>, grid, dim3(256), 0, stream, p);
  else if (mode == MODE_FP16) hipLaunchKernelGGL(unet_gn_apply_kernel<DT_FP16>, grid, dim3(256), 0, stream, p);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// last_bn + ReLU + last_conv2: a thread owns one pixel's 16 channels; the normalised values stay in fp32
template <int DT>
__global__ __launch_bounds__(256) void unet_gn_head_kernel(const uint16_t* __restrict__ X, const float2* __restrict__ stats,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ y, int HW, int OC) {
  const int pix = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (pix >= HW) return;
  float f[16];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float a[8], c[8];
    unet_gn_coeffs(stats, gamma, beta, b, h * 8, 2, a, c);
    unpack8<DT>(*(const uint4*)(X + ((long long)b * HW + pix) * 16 + h * 8), f + h * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[h * 8 + j] = fmaxf(__fmaf_rn(f[h * 8 + j], a[j], c[j]), 0.f);
  }
  for (int o = 0; o < OC; ++o) {
    float s = bias[o];
#pragma unroll
    for (int j = 0; j < 16; ++j) s = __fmaf_rn(w[o * 16 + j], f[j], s);
    y[((long long)b * OC + o) * HW + pix] = s;
  }
}

hipError_t launch_unet_gn_head(int mode, const void* X, const float* stats, const float* gamma, const float* beta, const float* w,
                               const float* b, float* y, int B, int HW, int OC, hipStream_t stream) {
  if (B <= 0 || HW <= 0 || OC < 1 || OC > 4 || B > 65535) return hipErrorInvalidValue;
  dim3 grid((HW + 255) / 256, B);
  if (mode == MODE_BF16)
    hipLaunchKernelGGL(unet_gn_head_kernel<DT_BF16>, grid, dim3(256), 0, stream, (const uint16_t*)X, (const float2*)stats, gamma, beta, w, b, y, HW, OC);
  else if (mode == MODE_FP16)
    hipLaunchKernelGGL(unet_gn_head_kernel<DT_FP16>, grid, dim3(256), 0, stream, (const uint16_t*)X, (const float2*)stats, gamma, beta, w, b, y, HW, OC);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ bilinear x2, align_corners=False
// source index (o + 0.5) / 2 - 0.5 clamped at 0 (torch): weights 0.25 / 0.75, neighbours clamped at the edge
template <int DT>
__global__ __launch_bounds__(256) void unet_upsample2x_kernel(const uint16_t* __restrict__ X, uint16_t* __restrict__ Y, int H, int W,
                                                              int C, int y_pix_stride, int y_off) {
  const int TP = C >> 3, b = blockIdx.y, Ho = 2 * H, Wo = 2 * W;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Ho * Wo * TP) return;
  const int pix = (int)(i / TP), tc = (int)(i - (long long)pix * TP);
  const int oy = pix / Wo, ox = pix - oy * Wo;
  const float sy = fmaxf(0.5f * (float)oy - 0.25f, 0.f), sx = fmaxf(0.5f * (float)ox - 0.25f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float ly1 = sy - (float)y0, lx1 = sx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const uint16_t* xb = X + (long long)b * H * W * C + tc * 8;
  float f00[8], f01[8], f10[8], f11[8], o[8];
  unpack8<DT>(*(const uint4*)(xb + ((long long)y0 * W + x0) * C), f00);
  unpack8<DT>(*(const uint4*)(xb + ((long long)y0 * W + x1) * C), f01);
  unpack8<DT>(*(const uint4*)(xb + ((long long)y1 * W + x0) * C), f10);
  unpack8<DT>(*(const uint4*)(xb + ((long long)y1 * W + x1) * C), f11);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = bilerp(f00[j], f01[j], f10[j], f11[j], lx0, lx1, ly0, ly1);
  *(uint4*)(Y + ((long long)b * Ho * Wo + pix) * y_pix_stride + y_off + tc * 8) = pack8<DT>(o);
}

hipError_t launch_unet_upsample2x(int mode, const void* X, void* Y, int B, int H, int W, int C, int y_pix_stride, int y_off,
                                  hipStream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || y_pix_stride % 8 != 0 || y_off % 8 != 0 || y_off < 0 ||
      y_off + C > y_pix_stride || B > 65535)
    return hipErrorInvalidValue;
  const long long n = 4ll * H * W * (C / 8);
  dim3 grid((unsigned)((n + 255) / 256), B);
  if (mode == MODE_BF16)
    hipLaunchKernelGGL(unet_upsample2x_kernel<DT_BF16>, grid, dim3(256), 0, stream, (const uint16_t*)X, (uint16_t*)Y, H, W, C, y_pix_stride, y_off);
  else if (mode == MODE_FP16)
    hipLaunchKernelGGL(unet_upsample2x_kernel<DT_FP16>, grid, dim3(256), 0, stream, (const uint16_t*)X, (uint16_t*)Y, H, W, C, y_pix_stride, y_off);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace dptx

// ------------------------------------------------------------------------------------------------ op-level entry points
using namespace dptx;

extern "C" {

static int urc(hipError_t r) { return r == hipSuccess ? DPTX_OK : (r == hipErrorInvalidValue ? DPTX_E_INVALID : DPTX_E_HIP); }

// Cin == 3: X is the caller's NCHW image [B,3,H,W] of element type io
static int op_conv3x3(int32_t dtype, const void* X, int32_t io, int32_t x_pix_stride, int32_t x_off, const void* Wt, const float* bias,
                      void* Y, float* gn_part, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* scratch, void* stream) {
  UnetConvParams p{};
  p.Wt = Wt; p.bias = bias; p.Y = Y; p.gn_part = gn_part; p.B = B; p.H = H; p.W = W; p.Cout = Cout;
  if (Cin == 3) {  // scratch: B*H*W*32 16-bit elements; Wt [Cout][32], k = (ky*3+kx)*3 + c
    if (scratch == nullptr) return DPTX_E_INVALID;
    const hipError_t r = launch_unet_im2col3(dtype, X, io, scratch, B, H, W, (hipStream_t)stream);
    if (r != hipSuccess) return urc(r);
    p.X = scratch; p.Cin = 32; p.taps = 1; p.x_pix_stride = 32; p.x_off = 0;
  } else {
    p.X = X; p.Cin = Cin; p.taps = 9; p.x_pix_stride = x_pix_stride; p.x_off = x_off;
  }
  return urc(launch_unet_conv_small(dtype, p, (hipStream_t)stream));
}

int dptx_op_unet_conv3x3(int32_t dtype, const void* X, int32_t x_pix_stride, int32_t x_off, const void* Wt, const float* bias, void* Y,
                         float* gn_part, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* scratch, void* stream) {
  return op_conv3x3(dtype, X, DPTX_IO_FP32, x_pix_stride, x_off, Wt, bias, Y, gn_part, B, H, W, Cin, Cout, scratch, stream);
}

// the first layer (Cin = 3) on a caller image of element type io: im2col, then the 1-tap product
int dptx_op_unet_conv3x3_io(int32_t dtype, const void* x, int32_t io, const void* Wt, const float* bias, void* Y, float* gn_part,
                            int32_t B, int32_t H, int32_t W, int32_t Cout, void* scratch, void* stream) {
  if (io != DPTX_IO_FP32 && io != DPTX_IO_BF16 && io != DPTX_IO_FP16) return DPTX_E_INVALID;
  return op_conv3x3(dtype, x, io, 0, 0, Wt, bias, Y, gn_part, B, H, W, 3, Cout, scratch, stream);
}

// a GEMM-path convolution exactly as Fwd::conv (unet_engine.hip) launches it: gemm_params_unet_conv, plain bias epilogue
int dptx_op_unet_conv_gemm(int32_t dtype, const void* X, int32_t x_pix_stride, int32_t x_off, int64_t x_bytes, const void* Wt,
                           const float* bias, void* Y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stream) {
  if (dtype != DPTX_DTYPE_BF16 && dtype != DPTX_DTYPE_FP16) return DPTX_E_INVALID;
  if (X == nullptr || Wt == nullptr || Y == nullptr || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return DPTX_E_INVALID;
  if (x_pix_stride % 8 != 0 || x_off % 8 != 0 || x_off < 0 || x_off + Cin > x_pix_stride) return DPTX_E_INVALID;
  if ((long long)B * H * W >= (1ll << 31) || x_bytes < (long long)B * H * W * x_pix_stride * 2) return DPTX_E_INVALID;
  GemmParams p;
  gemm_params_unet_conv(p, B, H, W, Cin, Cout, x_pix_stride, x_off, (long long)x_bytes);
  p.A = X; p.W = Wt; p.C = Y; p.bias = bias;
  return urc(launch_gemm(dtype, p, (hipStream_t)stream));
}

// last_bn + ReLU + last_conv2 with the caller's (mean, rstd) table
int dptx_op_unet_gn_head(int32_t dtype, const void* X, const float* stats, const float* gamma, const float* beta, const float* w,
                         const float* bias, float* y, int32_t B, int32_t HW, int32_t OC, void* stream) {
  if (X == nullptr || stats == nullptr || gamma == nullptr || beta == nullptr || w == nullptr || bias == nullptr || y == nullptr)
    return DPTX_E_INVALID;
  return urc(launch_unet_gn_head(dtype, X, stats, gamma, beta, w, bias, y, B, HW, OC, (hipStream_t)stream));
}

int32_t dptx_op_unet_conv_records(int32_t H, int32_t W) { return unet_conv_tiles(H, W); }

// statistics pass + finalize + apply: Y (full size, channel slice) and / or P (2x2 max-pooled, channel slice); scratch_f32 holds
// the records and the (mean, rstd) table: B * (dptx_op_unet_gn_records(H*W, C) * 16 + 16) floats
int32_t dptx_op_unet_gn_records(int32_t HW, int32_t C) { return (C >= 16 && C % 16 == 0 && C <= 1024) ? unet_gn_chunks(HW, C) : 0; }

int dptx_op_unet_groupnorm(int32_t dtype, const void* X, const float* gamma, const float* beta, void* Y, int32_t y_pix_stride,
                           int32_t y_off, void* P, int32_t p_pix_stride, int32_t p_off, int32_t B, int32_t H, int32_t W, int32_t C,
                           float eps, void* scratch_f32, void* stream) {
  if (scratch_f32 == nullptr || C < 16 || C % 16 != 0 || C > 1024) return DPTX_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const int nrec = unet_gn_chunks(H * W, C);
  float* part = (float*)scratch_f32;
  float* stats = part + (size_t)B * nrec * 16;
  hipError_t r = launch_unet_gn_stats(dtype, X, part, B, H * W, C, st);
  if (r != hipSuccess) return urc(r);
  r = launch_unet_gn_finalize(part, nrec, stats, B, H * W, C, eps, nullptr, st);
  if (r != hipSuccess) return urc(r);
  UnetGnApply a{};
  a.X = X; a.stats = stats; a.gamma = gamma; a.beta = beta; a.Y = Y; a.y_pix_stride = y_pix_stride; a.y_off = y_off;
  a.P = P; a.p_pix_stride = p_pix_stride; a.p_off = p_off; a.B = B; a.H = H; a.W = W; a.C = C;
  return urc(launch_unet_gn_apply(dtype, a, st));
}

int dptx_op_unet_upsample2x(int32_t dtype, const void* X, void* Y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t y_pix_stride,
                            int32_t y_off, void* stream) {
  return urc(launch_unet_upsample2x(dtype, X, Y, B, H, W, C, y_pix_stride, y_off, (hipStream_t)stream));
}

}  // extern "C"
