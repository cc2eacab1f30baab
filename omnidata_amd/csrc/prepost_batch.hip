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
//        The coefficient code and the tile live in resample_batch.h, shared with fullframe.hip (the whole image -> OH x OW).
//  post: colorize (plt.imsave: per-image min / max -> normalise -> LUT) in two launches; the batched normal / depth post kernels
//        are the single-image ones of prepost.hip with a batch index.
#include "resample_batch.h"

namespace {

__global__ __launch_bounds__(256) void coeff_axis_kernel(int in_size, int out_size, int ksize, int* __restrict__ bounds,
                                                         int* __restrict__ kk) {
  const int xx = blockIdx.x * 256 + threadIdx.x;
  if (xx >= out_size) return;
  coeff_one(in_size, out_size, xx, ksize, bounds + 2 * (size_t)xx, kk + (size_t)xx * ksize);
}

__global__ __launch_bounds__(256) void coeff_kernel(ImgArgs args, int n_img, int S, int* __restrict__ ws) {
  const int j = blockIdx.x * 256 + threadIdx.x;  // [0, 2S): horizontal axis first
  const int i = blockIdx.y;
  if (i >= n_img || j >= 2 * S) return;
  coeff_slot(args.d[i], i, j, S, S, ws);
}

__global__ __launch_bounds__(256) void resize_kernel(const uint8_t* __restrict__ pixels, ImgArgs args, int n_img, int S,
                                                     const int* __restrict__ ws, int depth_norm, float* __restrict__ out) {
  __shared__ ResizeTileLds s;
  const int i = blockIdx.y;
  if (i >= n_img) return;
  const ImgArg a = args.d[i];
  const int tile = blockIdx.x;
  if (tile >= (S / TC) * (S / a.tr)) return;
  resize_tile(s, pixels, a, i, tile, S, S, ws, depth_norm, out + (size_t)i * 3 * S * S);
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
  if (!desc_in_range(d)) return false;
  if ((d.H < d.W ? d.H : d.W) > 32 * S) return false;
  a.offset = d.offset;
  a.H = d.H; a.W = d.W; a.C = d.C; a.stride = d.row_stride_bytes;
  resized_geometry(d.H, d.W, S, a.oh, a.ow, a.top, a.left);
  if (a.oh < S || a.ow < S || a.top < 0 || a.left < 0 || a.top + S > a.oh || a.left + S > a.ow) return false;
  return fill_tile_geometry(d, a);
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
  *bytes = (int64_t)CHUNK * slot_ints(S, S) * sizeof(int);
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
