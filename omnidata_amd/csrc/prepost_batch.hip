// prepost_batch.hip -- pre/post-processing of demo.py for a whole batch of images of different sizes (include/dptx.h,
// "The same for a whole batch"): stream-ordered, caller's workspace only, no allocation, no host synchronisation, no cache.
//
//  pre : per 32 images two launches.
//        coeff_kernel   : Pillow's precompute_coeffs + normalize_coeffs_8bpc for the S cropped output columns and rows of every
//                         image, one thread per (image, axis, output index), in fp64 with the operations and the order of
//                         resample_coeffs() in prepost.hip.  Contraction is off for this file: a fused a*b+c would change
//                         `center`, `xmin` and the rounded fixed-point weights.
//        resize_kernel  : block = 32 output columns x TR output rows of one image (TR = 16, or 8 where the vertical scale makes
//                         16 rows' input window exceed the LDS tile).  The input rows the tile needs are fetched as aligned
//                         dwords into LDS a few rows at a time, their horizontal pass is formed ONCE (rounded uint8, as Pillow
//                         stores it between its passes) into an LDS tile [row][32] of packed channels, and the vertical pass
//                         reads that tile: lanes run along the output columns, so the tile reads, the weight reads and the
//                         fp32 stores are conflict-free / coalesced.
//        The descriptors travel by value in the kernel arguments (32 per launch), so there is no device table to fill.
//  post: colorize (plt.imsave: per-image min / max -> normalise -> LUT) in two launches; the batched normal / depth post kernels
//        are the single-image ones of prepost.hip with a batch index.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;  // Pillow: 22
constexpr int CHUNK = 32;                   // images per launch (descriptors by value: 32 * 56 B of kernel arguments)
constexpr int KMAX = 67;                    // taps per output at the scale limit: ceil(support < 33) * 2 + 1
constexpr int TC = 32;                      // output columns of a tile
constexpr int TR_MAX = 16;                  // output rows of a tile (16 or 8)
constexpr int ROWS_CAP = 304;               // input rows whose horizontal pass one tile holds
constexpr int STAGE_DW = 3072;              // dwords of raw input rows staged at a time

struct ImgArg {
  long long offset;
  int H, W, C, stride;
  int oh, ow, top, left;  // resized size and the centre crop's origin in it
  int ksh, ksv, tr, pad;
};
struct ImgArgs {
  ImgArg d[CHUNK];
};

// one output coordinate of Pillow's bilinear (triangle, support 1) filter over the whole axis: bounds2 = {first tap, taps},
// kk[0, ksize) = 22-bit fixed-point weights (zero behind the taps)
__host__ __device__ inline int coeff_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  return (int)ceil(support) * 2 + 1;
}

__device__ inline void coeff_one(int in_size, int out_size, int xx, int ksize, int* __restrict__ bounds2, int* __restrict__ kk) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > ksize) xmax = ksize;  // never taken (Pillow's own bound); keeps the stores inside the row whatever the input
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = (x + xmin - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    const double w = t < 1.0 ? 1.0 - t : 0.0;
    ww += w;
  }
  for (int x = 0; x < ksize; ++x) {
    int q = 0;
    if (x < xmax) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      double w = t < 1.0 ? 1.0 - t : 0.0;
      if (ww != 0.0) w /= ww;
      q = w < 0 ? (int)(-0.5 + w * (1 << PRECISION_BITS)) : (int)(0.5 + w * (1 << PRECISION_BITS));
    }
    kk[x] = q;
  }
  bounds2[0] = xmin;
  bounds2[1] = xmax;
}

__global__ __launch_bounds__(256) void coeff_axis_kernel(int in_size, int out_size, int ksize, int* __restrict__ bounds,
                                                         int* __restrict__ kk) {
  const int xx = blockIdx.x * 256 + threadIdx.x;
  if (xx >= out_size) return;
  coeff_one(in_size, out_size, xx, ksize, bounds + 2 * (size_t)xx, kk + (size_t)xx * ksize);
}

// workspace of one image slot (ints): [bh 2S | kh S*KMAX | bv 2S | kv S*KMAX]; rows of kh / kv are ksh / ksv ints apart
__host__ __device__ inline size_t slot_ints(int S) { return (size_t)2 * (2 + KMAX) * S; }

__global__ __launch_bounds__(256) void coeff_kernel(ImgArgs args, int n_img, int S, int* __restrict__ ws) {
  const int j = blockIdx.x * 256 + threadIdx.x;  // [0, 2S): horizontal axis first
  const int i = blockIdx.y;
  if (i >= n_img || j >= 2 * S) return;
  const ImgArg& a = args.d[i];
  int* base = ws + (size_t)i * slot_ints(S);
  if (j < S)
    coeff_one(a.W, a.ow, a.left + j, a.ksh, base + 2 * j, base + 2 * S + (size_t)j * a.ksh);
  else {
    const int r = j - S;
    base += (size_t)(2 + KMAX) * S;
    coeff_one(a.H, a.oh, a.top + r, a.ksv, base + 2 * r, base + 2 * S + (size_t)r * a.ksv);
  }
}

__device__ __forceinline__ int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void resize_kernel(const uint8_t* __restrict__ pixels, ImgArgs args, int n_img, int S,
                                                     const int* __restrict__ ws, int depth_norm, float* __restrict__ out) {
  __shared__ int s_wh[KMAX * TC];         // [tap][column]: lanes run along the columns
  __shared__ int s_wv[TR_MAX * KMAX];     // [row][tap]: one row per half wave, broadcast
  __shared__ int s_bh[TC * 2], s_bv[TR_MAX * 2];
  __shared__ uint32_t s_hp[ROWS_CAP * TC];  // horizontal pass: [input row][column], channels packed in the bytes
  __shared__ uint32_t s_in[STAGE_DW];       // raw input rows, from the dword that holds the tile's first byte

  const int i = blockIdx.y;
  if (i >= n_img) return;
  const ImgArg a = args.d[i];
  const int TR = a.tr;
  const int tiles_c = S / TC;
  const int tile = blockIdx.x;
  if (tile >= tiles_c * (S / TR)) return;
  const int c0 = (tile % tiles_c) * TC, r0 = (tile / tiles_c) * TR;
  const int tid = threadIdx.x;
  const int C = a.C, ksh = a.ksh, ksv = a.ksv;

  const int* bh = ws + (size_t)i * slot_ints(S);
  const int* kh = bh + 2 * S;
  const int* bv = bh + (size_t)(2 + KMAX) * S;
  const int* kv = bv + 2 * S;
  if (tid < 2 * TC) s_bh[tid] = bh[2 * c0 + tid];
  if (tid >= 64 && tid < 64 + 2 * TR) s_bv[tid - 64] = bv[2 * r0 + tid - 64];
  for (int e = tid; e < TC * ksh; e += 256) {  // kh rows of the 32 columns are contiguous: coalesced
    const int c = e / ksh, t = e - c * ksh;
    s_wh[t * TC + c] = kh[(size_t)c0 * ksh + e];
  }
  for (int e = tid; e < TR * ksv; e += 256) {
    const int r = e / ksv, t = e - r * ksv;
    s_wv[r * KMAX + t] = kv[(size_t)r0 * ksv + e];
  }
  __syncthreads();

  // bounds are non-decreasing along an axis: the tile's window is [first of the first, end of the last)
  const int row0 = s_bv[0];
  int nrows = s_bv[2 * (TR - 1)] + s_bv[2 * (TR - 1) + 1] - row0;
  if (nrows > ROWS_CAP) nrows = ROWS_CAP;  // never taken: the host sizes TR from the scale
  const int x0 = s_bh[0];
  const int segbytes = (s_bh[2 * (TC - 1)] + s_bh[2 * (TC - 1) + 1] - x0) * C;
  const int pitch = ((segbytes + 6) >> 2) | 1;  // dwords per staged row: up to 3 bytes of misalignment in front, odd
  int rch = STAGE_DW / pitch;                   // rows staged at a time (>= 1: the host bounds the segment)
  if (rch < 1) return;

  const uint8_t* img = pixels + a.offset;
  const size_t rowbytes = (size_t)a.W * C;
  for (int rb = 0; rb < nrows; rb += rch) {
    const int nr = min(rch, nrows - rb);
    // ---- stage nr input rows: aligned dwords where the dword lies inside the image row, guarded bytes at its two ends
    for (int e = tid; e < nr * pitch; e += 256) {
      const int rr = e / pitch, d = e - rr * pitch;
      const uint8_t* rowp = img + (size_t)(row0 + rb + rr) * a.stride;
      const uintptr_t first = (uintptr_t)(rowp + (size_t)x0 * C);
      const uintptr_t p = (first & ~(uintptr_t)3) + 4 * (uintptr_t)d;
      const uintptr_t lo = (uintptr_t)rowp, hi = lo + rowbytes;
      uint32_t v = 0;
      if (p >= lo && p + 4 <= hi) {
        v = *(const uint32_t*)p;
      } else {
        for (int b = 0; b < 4; ++b)
          if (p + b >= lo && p + b < hi) v |= (uint32_t)(*(const uint8_t*)(p + b)) << (8 * b);
      }
      s_in[rr * pitch + d] = v;
    }
    __syncthreads();
    // ---- horizontal pass of those rows for the tile's 32 columns
    for (int e = tid; e < nr * TC; e += 256) {
      const int rr = e >> 5, c = e & 31;
      const uint8_t* rowp = img + (size_t)(row0 + rb + rr) * a.stride;
      const int sh = (int)((uintptr_t)(rowp + (size_t)x0 * C) & 3);
      const int xmin = s_bh[2 * c], nx = s_bh[2 * c + 1];
      const uint8_t* src = (const uint8_t*)(s_in + rr * pitch) + sh + (xmin - x0) * C;
      uint32_t packed;
      if (C == 3) {
        int h0 = 1 << (PRECISION_BITS - 1), h1 = h0, h2 = h0;
        for (int t = 0; t < nx; ++t) {
          const int w = s_wh[t * TC + c];
          h0 += (int)src[3 * t] * w;
          h1 += (int)src[3 * t + 1] * w;
          h2 += (int)src[3 * t + 2] * w;
        }
        packed = (uint32_t)clip8(h0) | ((uint32_t)clip8(h1) << 8) | ((uint32_t)clip8(h2) << 16);
      } else {
        int h0 = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < nx; ++t) h0 += (int)src[t] * s_wh[t * TC + c];
        packed = (uint32_t)clip8(h0);
      }
      s_hp[(rb + rr) * TC + c] = packed;
    }
    __syncthreads();
  }

  // ---- vertical pass over the LDS tile, ToTensor / Normalize, 1 -> 3 channel repeat
  const size_t plane = (size_t)S * S;
  float* o = out + (size_t)i * 3 * plane;
  for (int e = tid; e < TR * TC; e += 256) {
    const int r = e >> 5, c = e & 31;
    const int ymin = s_bv[2 * r] - row0;
    int ny = s_bv[2 * r + 1];
    if (ymin + ny > nrows) ny = nrows - ymin;  // never taken (see nrows)
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < ny; ++t) {
      const uint32_t v = s_hp[(ymin + t) * TC + c];
      const int w = s_wv[r * KMAX + t];
      a0 += (int)(v & 255) * w;
      a1 += (int)((v >> 8) & 255) * w;
      a2 += (int)((v >> 16) & 255) * w;
    }
    const int v8[3] = {clip8(a0), C == 3 ? clip8(a1) : clip8(a0), C == 3 ? clip8(a2) : clip8(a0)};
    const size_t at = (size_t)(r0 + r) * S + c0 + c;
    for (int ch = 0; ch < 3; ++ch) {
      float f = (float)v8[ch] / 255.0f;       // ToTensor
      if (depth_norm) f = (f - 0.5f) / 0.5f;  // Normalize(mean=0.5, std=0.5)
      o[ch * plane + at] = f;
    }
  }
}

// resized size (torchvision Resize(int)): shorter side -> S, other = int(S*long/short); then the centre crop's origin
void resized_geometry(int H, int W, int S, int& oh, int& ow, int& top, int& left) {
  if ((W <= H && W == S) || (H <= W && H == S)) { oh = H; ow = W; }
  else if (W < H) { ow = S; oh = (int)((long long)S * H / W); }
  else { oh = S; ow = (int)((long long)S * W / H); }
  top = (int)std::nearbyint((oh - S) / 2.0);  // torchvision CenterCrop: round-half-to-even
  left = (int)std::nearbyint((ow - S) / 2.0);
}

bool fill_arg(const dptx_image_desc& d, int S, ImgArg& a) {
  if (d.offset < 0 || (d.C != 1 && d.C != 3) || d.H < 1 || d.W < 1 || d.H > 16384 || d.W > 16384) return false;
  if ((long long)d.row_stride_bytes < (long long)d.W * d.C) return false;
  if ((d.H < d.W ? d.H : d.W) > 32 * S) return false;
  a.offset = d.offset;
  a.H = d.H; a.W = d.W; a.C = d.C; a.stride = d.row_stride_bytes;
  resized_geometry(d.H, d.W, S, a.oh, a.ow, a.top, a.left);
  if (a.oh < S || a.ow < S || a.top < 0 || a.left < 0 || a.top + S > a.oh || a.left + S > a.ow) return false;
  a.ksh = coeff_ksize(d.W, a.ow);
  a.ksv = coeff_ksize(d.H, a.oh);
  if (a.ksh > KMAX || a.ksv > KMAX) return false;
  // a tile's input window: rows [c(first) - s + .5, c(last) + s + .5) with centres (TR - 1) * scale apart, at most 2 more
  const double sv = (double)d.H / a.oh, fv = sv < 1.0 ? 1.0 : sv;
  a.tr = (int)std::ceil((TR_MAX - 1) * sv + 2 * fv) + 2 <= ROWS_CAP ? TR_MAX : TR_MAX / 2;
  if ((int)std::ceil((a.tr - 1) * sv + 2 * fv) + 2 > ROWS_CAP) return false;
  const double sh = (double)d.W / a.ow, fh = sh < 1.0 ? 1.0 : sh;
  const long long segbytes = ((long long)std::ceil((TC - 1) * sh + 2 * fh) + 2) * d.C;
  if ((((segbytes + 6) >> 2) | 1) > STAGE_DW) return false;
  a.pad = 0;
  return true;
}

constexpr int MM_PARTS = 64;  // partial minima / maxima per image

__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ maps, long long N, float* __restrict__ part) {
  __shared__ float s_lo[256], s_hi[256];
  const float* m = maps + (size_t)blockIdx.y * N;
  float lo = INFINITY, hi = -INFINITY;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < N; e += (long long)MM_PARTS * 256) {
    const float v = m[e];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  s_lo[threadIdx.x] = lo;
  s_hi[threadIdx.x] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      s_lo[threadIdx.x] = fminf(s_lo[threadIdx.x], s_lo[threadIdx.x + s]);
      s_hi[threadIdx.x] = fmaxf(s_hi[threadIdx.x], s_hi[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[((size_t)blockIdx.y * MM_PARTS + blockIdx.x) * 2] = s_lo[0];
    part[((size_t)blockIdx.y * MM_PARTS + blockIdx.x) * 2 + 1] = s_hi[0];
  }
}

__global__ __launch_bounds__(256) void colorize_kernel(const float* __restrict__ maps, const uint32_t* __restrict__ lut, long long N,
                                                       const float* __restrict__ part, uint32_t* __restrict__ rgba) {
  __shared__ uint32_t s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  float lo = INFINITY, hi = -INFINITY;
  for (int p = 0; p < MM_PARTS; ++p) {  // every thread folds the same 64 pairs: min / max do not depend on the order
    lo = fminf(lo, part[((size_t)blockIdx.y * MM_PARTS + p) * 2]);
    hi = fmaxf(hi, part[((size_t)blockIdx.y * MM_PARTS + p) * 2 + 1]);
  }
  __syncthreads();
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const float v = maps[(size_t)blockIdx.y * N + e];
  const float n = hi > lo ? (v - lo) / (hi - lo) : 0.f;
  const float s = n * 256.0f;
  const int idx = s >= 255.f ? 255 : (s > 0.f ? (int)s : 0);  // NaN -> 0
  rgba[(size_t)blockIdx.y * N + e] = s_lut[idx];
}

}  // namespace

extern "C" {

int dptx_preprocess_batch_workspace_bytes(int32_t B, int32_t S, int64_t* bytes) {
  if (!bytes || B < 1 || B > 4096 || S < 32 || S > 1024 || S % 32) return DPTX_E_INVALID;
  *bytes = (int64_t)CHUNK * slot_ints(S) * sizeof(int);
  return DPTX_OK;
}

int dptx_preprocess_u8_batch(const void* pixels_dev, const dptx_image_desc* descs, int32_t B, int32_t S, int32_t depth_normalize,
                             void* x_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t need = 0;
  if (!pixels_dev || !descs || !x_dev || !workspace || dptx_preprocess_batch_workspace_bytes(B, S, &need) != DPTX_OK ||
      workspace_bytes < need || ((uintptr_t)workspace & 3) || ((uintptr_t)x_dev & 3))
    return DPTX_E_INVALID;
  ImgArg probe;
  for (int i = 0; i < B; ++i)
    if (!fill_arg(descs[i], S, probe)) return DPTX_E_INVALID;  // the whole batch is checked before the first launch
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int n = B - b0 < CHUNK ? B - b0 : CHUNK;
    ImgArgs args = {};
    for (int i = 0; i < n; ++i) fill_arg(descs[b0 + i], S, args.d[i]);
    // the chunks share the workspace: they are ordered on the stream
    hipLaunchKernelGGL(coeff_kernel, dim3((2 * S + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, args, n, S, (int*)workspace);
    hipLaunchKernelGGL(resize_kernel, dim3((S / TC) * (S / (TR_MAX / 2)), n), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)pixels_dev, args, n, S, (const int*)workspace, depth_normalize,
                       (float*)x_dev + (size_t)b0 * 3 * S * S);
  }
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

int dptx_resample_coeffs_device(int32_t in_size, int32_t out_size, void* bounds_dev, void* kk_dev, int32_t kk_capacity,
                                int32_t* ksize_host_out, void* stream) {
  if (in_size < 1 || out_size < 1 || in_size > (1 << 20) || out_size > (1 << 20) || !bounds_dev || !kk_dev || !ksize_host_out)
    return DPTX_E_INVALID;
  const int ks = coeff_ksize(in_size, out_size);
  *ksize_host_out = ks;
  if (ks > 4097 || (long long)kk_capacity < (long long)out_size * ks) return DPTX_E_INVALID;
  hipLaunchKernelGGL(coeff_axis_kernel, dim3((out_size + 255) / 256), dim3(256), 0, (hipStream_t)stream, in_size, out_size, ks,
                     (int*)bounds_dev, (int*)kk_dev);
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

int dptx_colorize_workspace_bytes(int32_t B, int64_t N, int64_t* bytes) {
  if (!bytes || B < 1 || B > 65535 || N < 1 || N > (1ll << 30)) return DPTX_E_INVALID;
  *bytes = (int64_t)B * MM_PARTS * 2 * sizeof(float);
  return DPTX_OK;
}

int dptx_colorize_u8_batch(const void* maps_dev, const void* lut_dev, int32_t B, int64_t N, void* rgba_dev, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  int64_t need = 0;
  if (!maps_dev || !lut_dev || !rgba_dev || !workspace || dptx_colorize_workspace_bytes(B, N, &need) != DPTX_OK ||
      workspace_bytes < need || ((uintptr_t)lut_dev & 3) || ((uintptr_t)rgba_dev & 3) || ((uintptr_t)workspace & 3))
    return DPTX_E_INVALID;
  hipLaunchKernelGGL(minmax_kernel, dim3(MM_PARTS, B), dim3(256), 0, (hipStream_t)stream, (const float*)maps_dev, (long long)N,
                     (float*)workspace);
  hipLaunchKernelGGL(colorize_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, (const float*)maps_dev,
                     (const uint32_t*)lut_dev, (long long)N, (const float*)workspace, (uint32_t*)rgba_dev);
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
