// stem.hip -- fused 7x7 stride-2 TF-SAME stem convolution of the ResNetV2 hybrid backbone
// (timm StdConv2dSame 3->64; vit.py:128-131 reaches it through patch_embed.backbone).
//
// x NCHW fp32 (or bf16 / fp16: DPTX_IO_*) [B,3,H,W]  ->  y NHWC 16-bit [B,H/2,W/2,64]   (raw conv output; GroupNorm+ReLU+MaxPool follow)
//
// No im2col buffer: a block owns 4 output rows x 64 output columns.  Its 13 x 133 x 3 input patch is converted to
// 16-bit once and kept in LDS (10.6 KB); the implicit-GEMM K axis is ordered (c, ky, kx) with kx padded 7 -> 8, so
// that one MFMA operand chunk (8 consecutive k) is 8 CONSECUTIVE input columns of one (channel, row) -- 16
// contiguous, 4-byte-aligned bytes of the patch, fetched with four conflict-free ds_read_b32 (neighbouring output
// pixels are 4 bytes apart).  K = 3*7*8 = 168, padded to 176 = 11 MFMA k-steps; the weight matrix [64][176]
// (22.5 KB, zero in the padded taps) is read straight from L1/L2.  v_mfma_f32_32x32x16: wave w computes output row
// w of the block (64 pixels x 64 channels).  Replaces im2col (453 MB written + read per 32 images) + a K=192 GEMM.
#include "common.h"
#include "kernels.h"

#include <type_traits>

namespace dptx {

constexpr int STEM_KP = 176;       // packed K of the stem weight rows
constexpr int ST_ROWS = 13, ST_PITCH = 136;  // patch rows, patch row pitch (elements)
constexpr int ST_PATCH = 3 * ST_ROWS * ST_PITCH;  // elements per plane

template <int DT, int PL>
__global__ __launch_bounds__(256, 2) void stem_conv_kernel(const void* __restrict__ x, int io, const uint16_t* __restrict__ Wt,
                                                           uint16_t* __restrict__ y, int H, int W, int pad_t, int pad_l,
                                                           long long act_plane, long long w_plane) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* patch = (uint16_t*)smem;  // [PL][3][13][136]
  const int Ho = H >> 1, Wo = W >> 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int tiles_x = (Wo + 63) / 64;   // the last column tile may be partial (W any multiple of 8)
  const int ox0 = (blockIdx.x % tiles_x) * 64, oy0 = (blockIdx.x / tiles_x) * 4, b = blockIdx.y;
  const int iy0 = 2 * oy0 - pad_t, ix0 = 2 * ox0 - pad_l;

  // ---- input patch -> LDS (zero outside the image and in the pitch padding).  A wave owns one (channel, row) line of the
  // patch per pass and moves it as column PAIRS: the patch starts at an even column (ix0 = 128 k - pad_l, pad_l = 2) and W is
  // even, so a pair is either inside the image or outside it -- one 8-byte (fp32) / 4-byte (16-bit) load and one ds_write_b32
  // per pair instead of two scalar loads, two conversions and four integer divisions per element
  const long long xb = (long long)b * 3 * H * W;  // element offset of image b (x is fp32, bf16 or fp16: `io`)
  for (int rc = wave; rc < 3 * ST_ROWS; rc += 4) {
    const int c = rc / ST_ROWS, r = rc - c * ST_ROWS;
    const int iy = iy0 + r;
    const bool rowok = (unsigned)iy < (unsigned)H;
    const long long rowoff = xb + ((long long)c * H + iy) * W;
    for (int cp = lane; cp < ST_PITCH / 2; cp += 64) {
      const int col = 2 * cp, ix = ix0 + col;
      float v0 = 0.f, v1 = 0.f;
      if (rowok && col < 134 && (unsigned)ix < (unsigned)W) {
        if (io == IO_FP32) {
          const float2 t = *(const float2*)((const float*)x + rowoff + ix);
          v0 = t.x; v1 = t.y;
        } else {
          const uint32_t t = *(const uint32_t*)((const uint16_t*)x + rowoff + ix);
          v0 = io == IO_BF16 ? T16<DT_BF16>::tof((uint16_t)(t & 0xffffu)) : T16<DT_FP16>::tof((uint16_t)(t & 0xffffu));
          v1 = io == IO_BF16 ? T16<DT_BF16>::tof((uint16_t)(t >> 16)) : T16<DT_FP16>::tof((uint16_t)(t >> 16));
        }
      }
      const uint32_t hi = T16<DT>::pack2(v0, v1);
      *(uint32_t*)(patch + rc * ST_PITCH + col) = hi;
      if (PL == 2)
        *(uint32_t*)(patch + ST_PATCH + rc * ST_PITCH + col) =
            T16<DT>::pack2(v0 - T16<DT>::tof((uint16_t)(hi & 0xffffu)), v1 - T16<DT>::tof((uint16_t)(hi >> 16)));
    }
  }
  __syncthreads();

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int ks = 0; ks < STEM_KP / 16; ++ks) {
    const int q = 2 * ks + lh;                 // k chunk 0..21; chunk 21 is all-zero weights
    const int qq = q < 21 ? q : 0;
    const int c = qq / 7, ky = qq - c * 7;
    u32x4_t af[2], al[2], bf[2], bl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int cx = i * 32 + lr;              // output column inside the block
      const uint32_t* src = (const uint32_t*)(patch + ((c * ST_ROWS + 2 * wave + ky) * ST_PITCH + 2 * cx));
      af[i] = u32x4_t{src[0], src[1], src[2], src[3]};
      if (PL == 2) {
        const uint32_t* sl = src + ST_PATCH / 2;
        al[i] = u32x4_t{sl[0], sl[1], sl[2], sl[3]};
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint16_t* wp = Wt + (long long)(j * 32 + lr) * STEM_KP + q * 8;
      bf[j] = *(const u32x4_t*)wp;
      if (PL == 2) bl[j] = *(const u32x4_t*)(wp + w_plane);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (PL == 2) {
          acc[i][j] = T16<DT>::mfma32(al[i], bf[j], acc[i][j]);
          acc[i][j] = T16<DT>::mfma32(af[i], bl[j], acc[i][j]);
        }
        acc[i][j] = T16<DT>::mfma32(af[i], bf[j], acc[i][j]);
      }
  }

  // ---- epilogue: accumulators -> LDS [256 pixels][64 ch] fp32 -> coalesced NHWC rows (128 B per pixel)
  __syncthreads();
  float* ct = (float*)smem;
  constexpr int CT_PITCH = 68;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pl_ = wave * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;  // pixel = (row wave, column)
        ct[pl_ * CT_PITCH + j * 32 + lr] = acc[i][j][r];
      }
  __syncthreads();
  const int cn = tid & 7;
#pragma unroll 2
  for (int p = tid >> 3; p < 256; p += 32) {
    const int r = p >> 6, c = p & 63;
    float v[8];
    const float4 a0 = *(const float4*)(ct + p * CT_PITCH + cn * 8), a1 = *(const float4*)(ct + p * CT_PITCH + cn * 8 + 4);
    v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w; v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
    if (ox0 + c < Wo) store8f<DT, PL>(y + (((long long)b * Ho + oy0 + r) * Wo + ox0 + c) * 64 + cn * 8, act_plane, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The one-plane form the forward runs (bf16 / fp16): the same tile, patch, K layout and MFMA order per accumulator, so the
// same bits, with what kept stem_conv_kernel at two blocks per CU and its phases serial taken out:
// * LDS is the patch plus 4 x 2.3 KB of wave-private packed 16-bit staging (the idiom of conv1x1_stream_kernel: rounding in
//   registers with T16::pack2 -- store8f's conversion --, neighbouring channels paired across lanes, 16 pixels x 64 channels
//   per pass, read back as 16-byte row pieces): 19.8 KB, no block barrier after the MFMAs, and 128 VGPRs -- four blocks per CU.
// * The weight fragments of a wave's first 32 output channels (11 k-steps x 16 B per lane) are fetched ahead of the patch
//   fill, those of the second 32 into the same registers as the first are consumed: no k-step waits for a load issued in it.
//   The accumulators of the two channel halves are independent, each runs k-steps 0..10 in ascending order from zero.
// * The patch fill is fully unrolled, every load of a thread in flight before the first ds_write, and moves 4 columns per
//   load (16 bytes of an fp32 image): the patch starts at ix0 = 128 k - 2, so columns 2..133 are 33 aligned quads of the
//   image row and columns 0..1 one pair; W % 4 == 0, so a quad is inside the image or outside it.  Same zero-fill rule.
//   The pitch padding (columns 134, 135) is never read by a fragment and is left as it is.
constexpr int STW_STG_PITCH = 144;                  // bytes per staged pixel: 64 channels x 2 + 16
constexpr int STW_STG_WAVE = 16 * STW_STG_PITCH;    // 16 pixels per pass
constexpr int STW_LDS = ST_PATCH * 2 + 4 * STW_STG_WAVE;
constexpr int STW_QUADS = 3 * ST_ROWS * 33;         // aligned 4-column pieces of the patch
constexpr int STW_PASSES = (STW_QUADS + 255) / 256;
static_assert(ST_PATCH * 2 % 16 == 0, "the staging behind the patch is read in 16-byte pieces");

// raw 4-column / 2-column pieces of an image row as loaded (converted only when they are written to LDS: fewer live registers)
template <int IO> struct StwRaw { typedef uint2 Q; typedef uint32_t P; };
template <> struct StwRaw<IO_FP32> { typedef float4 Q; typedef float2 P; };
template <int DT, int IO>
__device__ __forceinline__ void stw_pack4(const typename StwRaw<IO>::Q& t, uint32_t* d) {
  if constexpr (IO == IO_FP32) {
    d[0] = T16<DT>::pack2(t.x, t.y);
    d[1] = T16<DT>::pack2(t.z, t.w);
  } else {
    constexpr int S = IO == IO_BF16 ? DT_BF16 : DT_FP16;
    d[0] = T16<DT>::pack2(T16<S>::tof((uint16_t)(t.x & 0xffffu)), T16<S>::tof((uint16_t)(t.x >> 16)));
    d[1] = T16<DT>::pack2(T16<S>::tof((uint16_t)(t.y & 0xffffu)), T16<S>::tof((uint16_t)(t.y >> 16)));
  }
}
template <int DT, int IO>
__device__ __forceinline__ uint32_t stw_pack2(const typename StwRaw<IO>::P& t) {
  if constexpr (IO == IO_FP32) {
    return T16<DT>::pack2(t.x, t.y);
  } else {
    constexpr int S = IO == IO_BF16 ? DT_BF16 : DT_FP16;
    return T16<DT>::pack2(T16<S>::tof((uint16_t)(t & 0xffffu)), T16<S>::tof((uint16_t)(t >> 16)));
  }
}

template <int DT, int IO>
__global__ __launch_bounds__(256, 4) void stem_conv_kernel_wp(const void* __restrict__ x, const uint16_t* __restrict__ Wt,
                                                              uint16_t* __restrict__ y, int H, int W, int pad_t, int pad_l) {
  __shared__ __attribute__((aligned(16))) char smem[STW_LDS];
  uint16_t* patch = (uint16_t*)smem;  // [3][13][136]
  const int Ho = H >> 1, Wo = W >> 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int tiles_x = (Wo + 63) / 64;
  const int ox0 = (blockIdx.x % tiles_x) * 64, oy0 = (blockIdx.x / tiles_x) * 4, b = blockIdx.y;
  const int iy0 = 2 * oy0 - pad_t, ix0 = 2 * ox0 - pad_l;

  // ---- input patch -> LDS.  Every load is unconditional (a piece outside the image reads the image's first bytes and is
  // replaced by zeros), so that none of them waits for another
  const uint16_t* wp = Wt + lr * STEM_KP + lh * 8;
  u32x4_t bw[STEM_KP / 16];
  constexpr int STW_EARLY = 8;  // k-steps whose fragments are fetched under the patch fill (all 11 leave it too few registers)
  {
    typedef typename StwRaw<IO>::Q RawQ;
    typedef typename StwRaw<IO>::P RawP;
    typedef typename std::conditional<IO == IO_FP32, float, uint16_t>::type Elem;
    const Elem* xe = (const Elem*)x + (long long)b * 3 * H * W;  // 3 H W < 2^31 (launch_stem_conv): 32-bit offsets below
    RawQ q[STW_PASSES];
    RawP pr;
#pragma unroll
    for (int p = 0; p < STW_PASSES; ++p) {
      const int u = tid + 256 * p;
      const int line = u / 33, col = 2 + 4 * (u - line * 33);
      const int c = line / ST_ROWS, iy = iy0 + line - c * ST_ROWS, ix = ix0 + col;
      const bool ok = u < STW_QUADS && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      q[p] = *(const RawQ*)(xe + (ok ? (c * H + iy) * W + ix : 0));
      if (!ok) q[p] = RawQ{};  // all-zero bits are 0.f in every input type
    }
    {
      const int line = tid < 3 * ST_ROWS ? tid : 0;
      const int c = line / ST_ROWS, iy = iy0 + line - c * ST_ROWS;
      const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix0 < (unsigned)W;
      pr = *(const RawP*)(xe + (ok ? (c * H + iy) * W + ix0 : 0));
      if (!ok) pr = RawP{};
    }
    // ---- weight fragments of output channels lr (k chunk 2 ks + lh); chunk 21 is all-zero weights, as stored.  Issued
    // behind the patch loads: they are still in flight while the patch is converted and written
#pragma unroll
    for (int ks = 0; ks < STW_EARLY; ++ks) bw[ks] = *(const u32x4_t*)(wp + ks * 16);
#pragma unroll
    for (int p = 0; p < STW_PASSES; ++p) {
      const int u = tid + 256 * p;
      const int line = u / 33, col = 2 + 4 * (u - line * 33);
      if (u < STW_QUADS) stw_pack4<DT, IO>(q[p], (uint32_t*)(patch + line * ST_PITCH + col));
    }
    if (tid < 3 * ST_ROWS) *(uint32_t*)(patch + tid * ST_PITCH) = stw_pack2<DT, IO>(pr);
  }
  __syncthreads();  // the only block barrier
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = STW_EARLY; ks < STEM_KP / 16; ++ks) bw[ks] = *(const u32x4_t*)(wp + ks * 16);  // consumed 8 k-steps on

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto a_frag = [&](int ks, int i) {
    const int qk = 2 * ks + lh;
    const int qq = qk < 21 ? qk : 0;
    const int c = qq / 7, ky = qq - c * 7;
    const uint32_t* src = (const uint32_t*)(patch + ((c * ST_ROWS + 2 * wave + ky) * ST_PITCH + 2 * (i * 32 + lr)));
    return u32x4_t{src[0], src[1], src[2], src[3]};
  };
  // channels lr: k-steps 0..10.  The fragments of channels 32 + lr follow into the registers just consumed -- the first
  // STW_REFILL of them here, the rest under the second loop (all 11 at once would not leave room for 64 accumulators)
  constexpr int KS = STEM_KP / 16, STW_REFILL = 8;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const u32x4_t a0 = a_frag(ks, 0), a1 = a_frag(ks, 1);
    acc[0][0] = T16<DT>::mfma32(a0, bw[ks], acc[0][0]);
    acc[1][0] = T16<DT>::mfma32(a1, bw[ks], acc[1][0]);
    if (ks < STW_REFILL) bw[ks] = *(const u32x4_t*)(wp + 32 * STEM_KP + ks * 16);
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const u32x4_t a0 = a_frag(ks, 0), a1 = a_frag(ks, 1);
    const u32x4_t w = bw[ks < STW_REFILL ? ks : ks - STW_REFILL];
    acc[0][1] = T16<DT>::mfma32(a0, w, acc[0][1]);
    acc[1][1] = T16<DT>::mfma32(a1, w, acc[1][1]);
    if (ks + STW_REFILL < KS) bw[ks] = *(const u32x4_t*)(wp + 32 * STEM_KP + (ks + STW_REFILL) * 16);
  }

  // ---- epilogue: 16 pixels x 64 channels at a time through the wave's own staging -> 128 contiguous bytes per pixel.
  // acc[i][j][r] = pixel i * 32 + (r & 3) + 8 (r >> 2) + 4 lh of output row `wave`, channel j * 32 + lr
  char* const stg = smem + ST_PATCH * 2 + wave * STW_STG_WAVE;
  const unsigned sel = (lr & 1) ? 0x03020706u : 0x05040100u;  // v_perm_b32 selector of the channel-pair exchange
  const int cn = lane & 7, rr = lane >> 3;
  uint16_t* const yrow = y + (((long long)b * Ho + oy0 + wave) * Wo + ox0) * 64 + cn * 8;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // registers 8 h .. 8 h + 7 = pixels i * 32 + 16 h .. + 15
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();  // the wave's LDS accesses execute in order: the previous pass's reads are ahead
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          // own = (pixel r, pixel r + 1) of channel lr.  Even lanes keep pixel r and take the neighbour's: channels (lr, lr + 1);
          // odd lanes keep pixel r + 1: channels (lr - 1, lr)
          const uint32_t own = T16<DT>::pack2(acc[i][j][8 * h + 2 * t], acc[i][j][8 * h + 2 * t + 1]);
          const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
          const uint32_t o = __builtin_amdgcn_perm(nb, own, sel);
          const int rl = ((2 * t) & 3) + (lr & 1) + 8 * (t >> 1) + 4 * lh;
          *(uint32_t*)(stg + rl * STW_STG_PITCH + (j * 32 + (lr & ~1)) * 2) = o;
        }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        const int rl = rr + 8 * pp;
        const u32x4_t d = *(const u32x4_t*)(stg + rl * STW_STG_PITCH + cn * 16);
        const int c = i * 32 + 16 * h + rl;
        if (ox0 + c < Wo) *(u32x4_t*)(yrow + c * 64) = d;
      }
    }
}

// the new form measured faster at the op level at B = 32 and B = 16 (profiles/stem_upsample.md): the forward takes it
// wherever it can run.  Debug flag 128 keeps every launch on stem_conv_kernel.
static bool stem_wp_eligible(int mode, const void* x, int io, const void* Wt, const void* y, int plft) {
  if (mode != MODE_BF16 && mode != MODE_FP16) return false;
  const uintptr_t xa = (uintptr_t)x;
  return plft == 2 && xa % (io == IO_FP32 ? 16 : 8) == 0 && (uintptr_t)Wt % 16 == 0 && (uintptr_t)y % 16 == 0;
}

template <int DT>
static void launch_stem_wp(const void* x, int io, const void* Wt, void* y, int H, int W, int pt, int plft, dim3 grid,
                           hipStream_t stream) {
  if (io == IO_FP32)
    hipLaunchKernelGGL((stem_conv_kernel_wp<DT, IO_FP32>), grid, dim3(256), 0, stream, x, (const uint16_t*)Wt, (uint16_t*)y, H, W, pt, plft);
  else if (io == IO_BF16)
    hipLaunchKernelGGL((stem_conv_kernel_wp<DT, IO_BF16>), grid, dim3(256), 0, stream, x, (const uint16_t*)Wt, (uint16_t*)y, H, W, pt, plft);
  else
    hipLaunchKernelGGL((stem_conv_kernel_wp<DT, IO_FP16>), grid, dim3(256), 0, stream, x, (const uint16_t*)Wt, (uint16_t*)y, H, W, pt, plft);
}

hipError_t launch_stem_conv(int mode, const void* x, int io, const void* Wt, void* y, int B, int H, int W, Planes pl,
                            hipStream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  if (H % 8 != 0 || W % 8 != 0) return hipErrorInvalidValue;
  const int pt = max((Ho - 1) * 2 + 7 - H, 0) / 2, plft = max((Wo - 1) * 2 + 7 - W, 0) / 2;
  dim3 grid(((Wo + 63) / 64) * (Ho / 4), B);
  if (!(gemm_debug_flags() & 128) && stem_wp_eligible(mode, x, io, Wt, y, plft)) {
    if (mode == MODE_BF16) launch_stem_wp<DT_BF16>(x, io, Wt, y, H, W, pt, plft, grid, stream);
    else launch_stem_wp<DT_FP16>(x, io, Wt, y, H, W, pt, plft, grid, stream);
    return hipGetLastError();
  }
  const size_t smem = 256 * 68 * 4;  // C tile (69.6 KB) aliases the patch
  DPTX_DISPATCH_MODE(mode, {
    auto k = stem_conv_kernel<DT, PL>;
    ensure_dyn_smem((const void*)k, smem);
    hipLaunchKernelGGL(k, grid, dim3(256), smem, stream, x, io, (const uint16_t*)Wt, (uint16_t*)y, H, W, pt, plft, pl.act, pl.w);
  });
  return hipGetLastError();
}

}  // namespace dptx
