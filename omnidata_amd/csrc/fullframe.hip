// fullframe.hip -- whole-image inference around the forward (include/dptx.h, "Full-frame inference"): B images of different
// sizes -> one rectangular network input, and the network's maps -> B outputs of the images' own sizes in one packed buffer.
// Stream-ordered, caller's workspace only, no allocation, no host synchronisation, no cache; descriptors by value, 32 per launch.
//
//  pre : ToTensor(img.resize((OW, OH), BILINEAR)) per image (Pillow's antialiased two-pass 8-bit resampler, bit-identical): the
//        coefficient arithmetic and the tile of prepost_batch.hip (resample_batch.h) with an independent scale per axis and no
//        crop.  The grid is the sum of the images' tile counts (16- or 8-row tiles): a block finds its image from the first-tile
//        prefix that travels with the descriptors.
//  views: the same with a mirror per image, for test-time augmentation (dptx_preprocess_u8_views_batch): a descriptor may be a
//        window of an uploaded image (the parent's row stride), and the store of a mirrored view goes to column OW - 1 - x.
//  post: ATen's upsample_bilinear2d / upsample_bicubic2d (align_corners=False) from y [B][C][h][w] to every image's H x W.
//        Block = 128 output columns x 8 rows of ONE image, lanes along the columns; the 4 / 16 taps come from cache (one image's
//        source is <= 1.8 MB and is read by all of its tiles).  fp32 and RGBA outputs are one dword per lane, coalesced.  uint8
//        RGB rows are 3*W bytes and start at any byte: the tile's bytes are formed in LDS at the row's own misalignment and go
//        out as aligned dwords, with byte stores for the (at most 3 + 3) bytes at the two ends of a tile row -- no byte outside
//        [row start, row start + 3*W) is written, so neighbouring tiles, rows and images never touch each other's bytes.
//        DEPTH_RGBA: a first launch takes the minimum / maximum of exactly the DEPTH_F32 values (64 partials per image in the
//        workspace, each block walks its image's tiles in a fixed order), the second recomputes the values and looks them up.
// Contraction is off (resample_batch.h): the coordinates and blends are ATen's operations rounded one by one, and the two
// launches of DEPTH_RGBA compute the same bits.
#include "resample_batch.h"

namespace {

// ------------------------------------------------------------------------------------------------ pre
__global__ __launch_bounds__(256) void coeff_rect_kernel(ImgArgs args, int n_img, int OH, int OW, int* __restrict__ ws) {
  const int j = blockIdx.x * 256 + threadIdx.x;  // [0, OW + OH): horizontal axis first
  const int i = blockIdx.y;
  if (i >= n_img || j >= OW + OH) return;
  coeff_slot(args.d[i], i, j, OH, OW, ws);
}

__global__ __launch_bounds__(256) void resize_rect_kernel(const uint8_t* __restrict__ pixels, ImgArgs args, int n_img, int OH, int OW,
                                                          const int* __restrict__ ws, int depth_norm, float* __restrict__ out) {
  __shared__ ResizeTileLds s;
  const int blk = blockIdx.x;
  int i = 0;
  for (int k = 1; k < CHUNK; ++k)
    if (k < n_img && blk >= args.d[k].pad) i = k;  // .pad = first tile of image k (non-decreasing)
  const ImgArg a = args.d[i];
  resize_tile(s, pixels, a, i, blk - a.pad, OH, OW, ws, depth_norm, out + (size_t)i * 3 * OH * OW);
}

// the views of test-time augmentation: the same tile with the mirrored store
__global__ __launch_bounds__(256) void resize_views_kernel(const uint8_t* __restrict__ pixels, ImgArgs args, int n_img, int OH, int OW,
                                                           const int* __restrict__ ws, int depth_norm, float* __restrict__ out) {
  __shared__ ResizeTileLds s;
  const int blk = blockIdx.x;
  int i = 0;
  for (int k = 1; k < CHUNK; ++k)
    if (k < n_img && blk >= args.d[k].pad) i = k;
  const ImgArg a = args.d[i];
  resize_tile<true>(s, pixels, a, i, blk - a.pad, OH, OW, ws, depth_norm, out + (size_t)i * 3 * OH * OW);
}

bool fill_rect_arg(const dptx_image_desc& d, int OH, int OW, ImgArg& a) {
  if (!desc_in_range(d)) return false;
  if (d.H > 32 * OH || d.W > 32 * OW) return false;
  a.offset = d.offset;
  a.H = d.H; a.W = d.W; a.C = d.C; a.stride = d.row_stride_bytes;
  a.oh = OH; a.ow = OW; a.top = 0; a.left = 0;
  return fill_tile_geometry(d, a);
}

// ------------------------------------------------------------------------------------------------ post
constexpr int PW = 128, PH = 8;        // output tile: columns x rows
static_assert(256 % PW == 0 && PH % (256 / PW) == 0, "a thread keeps one column of the tile");
constexpr int ROW_DW = row_dw(PW);     // dwords of one uint8 RGB tile row in LDS (384 bytes + 3 of misalignment, padded)
constexpr int MM_PARTS = 64;           // partial minima / maxima per image
constexpr int M_NORMAL_U8 = DPTX_RESIZE_NORMAL_U8, M_NORMAL_F32 = DPTX_RESIZE_NORMAL_F32, M_DEPTH_F32 = DPTX_RESIZE_DEPTH_F32,
              M_DEPTH_RGBA = DPTX_RESIZE_DEPTH_RGBA;

struct OutArg {
  long long offset;
  int H, W, stride, tile0;  // tile0: the image's first tile of the launch
  float sy, sx;             // ATen's area_pixel_compute_scale: (float)in / (float)out, divided once on the host
};
struct OutArgs {
  OutArg d[CHUNK];
};

__host__ __device__ inline int tiles_of(int H, int W) { return ((W + PW - 1) / PW) * ((H + PH - 1) / PH); }

// source coordinates: src_coord / guard / lin_axis of resample_batch.h
__device__ __forceinline__ float bilinear(const float* __restrict__ p, int w, const Lin& y, const Lin& x) {
  const float* r0 = p + y.i0 * w;  // h * w <= 2^24
  const float* r1 = p + y.i1 * w;
  float t0 = x.l0 * r0[x.i0];
  t0 += x.l1 * r0[x.i1];
  float t1 = x.l0 * r1[x.i0];
  t1 += x.l1 * r1[x.i1];
  float t = y.l0 * t0;
  t += y.l1 * t1;
  return t;
}

// ATen get_cubic_upsample_coefficients (A = -0.75)
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
struct Cub {
  int i[4];
  float c[4];
};
__device__ __forceinline__ Cub cub_axis(int in, float scale, int dst) {
  Cub a;
  int idx;
  float t;
  guard(src_coord(scale, dst), in, idx, t);
  const float A = -0.75f;
  a.c[0] = cubic2(t + 1.f, A);
  a.c[1] = cubic1(t, A);
  const float u = 1.f - t;
  a.c[2] = cubic1(u, A);
  a.c[3] = cubic2(u + 1.f, A);
  for (int j = 0; j < 4; ++j) a.i[j] = min(max(idx - 1 + j, 0), in - 1);
  return a;
}
// demo.py:143-145 at the image's own size: bicubic, clamp(0, 1), 1 - x
__device__ __forceinline__ float depth_value(const float* __restrict__ p, int w, const Cub& y, const Cub& x) {
  float acc = 0.f;
  for (int j = 0; j < 4; ++j) {
    const float* r = p + y.i[j] * w;
    float t = x.c[0] * r[x.i[0]];
    for (int i = 1; i < 4; ++i) t += x.c[i] * r[x.i[i]];
    if (j == 0) acc = y.c[0] * t;
    else acc += y.c[j] * t;
  }
  acc = fminf(fmaxf(acc, 0.f), 1.f);
  return 1.f - acc;
}

// block -> (image slot, tile of that image)
__device__ __forceinline__ int find_image(const OutArgs& args, int n_img, int blk) {
  int i = 0;
  for (int k = 1; k < CHUNK; ++k)
    if (k < n_img && blk >= args.d[k].tile0) i = k;
  return i;
}

template <int MODE>
__global__ __launch_bounds__(256) void post_resize_kernel(const float* __restrict__ y, int h, int w, OutArgs args, int n_img, int renorm,
                                                          uint8_t* __restrict__ out, const uint32_t* __restrict__ lut,
                                                          const float* __restrict__ part) {
  __shared__ uint32_t s_row[MODE == M_NORMAL_U8 ? PH * ROW_DW : 1];
  __shared__ uint32_t s_lut[MODE == M_DEPTH_RGBA ? 256 : 1];
  const int tid = threadIdx.x;
  const int i = find_image(args, n_img, blockIdx.x);
  const OutArg a = args.d[i];
  const int tile = blockIdx.x - a.tile0;
  const int tiles_x = (a.W + PW - 1) / PW;
  const int c0 = (tile % tiles_x) * PW, r0 = (tile / tiles_x) * PH;
  const int H = a.H, W = a.W;
  const size_t hw = (size_t)h * w;
  uint8_t* o = out + a.offset;

  float lo = 0.f, hi = 0.f;
  if (MODE == M_DEPTH_RGBA) {
    s_lut[tid] = lut[tid];
    lo = INFINITY;
    hi = -INFINITY;
    for (int p = 0; p < MM_PARTS; ++p) {  // every thread folds the same 64 pairs: min / max do not depend on the order
      lo = fminf(lo, part[((size_t)i * MM_PARTS + p) * 2]);
      hi = fmaxf(hi, part[((size_t)i * MM_PARTS + p) * 2 + 1]);
    }
    __syncthreads();
  }

  // a thread keeps its column over the tile's rows: the column's taps and weights are formed once
  const int c = tid % PW, ox = c0 + c;
  const int oxc = min(ox, W - 1);
  Lin lx = {};
  Cub cx = {};
  if (MODE == M_NORMAL_U8 || MODE == M_NORMAL_F32) lx = lin_axis(w, W, a.sx, oxc);
  else cx = cub_axis(w, a.sx, oxc);
  for (int r = tid / PW; r < PH; r += 256 / PW) {
    const int oy = r0 + r;
    if (oy >= H || ox >= W) continue;
    if (MODE == M_NORMAL_U8 || MODE == M_NORMAL_F32) {
      const float* src = y + (size_t)i * 3 * hw;
      const Lin ly = lin_axis(h, H, a.sy, oy);
      float v[3];
      for (int ch = 0; ch < 3; ++ch) v[ch] = bilinear(src + ch * hw, w, ly, lx);
      if (renorm) {  // F.normalize of the decoded normal (oasis_eval_tta.py:339,441-445), re-encoded
        float n[3];
        for (int ch = 0; ch < 3; ++ch) n[ch] = 2.f * v[ch] - 1.f;
        float ss = n[0] * n[0];
        ss += n[1] * n[1];
        ss += n[2] * n[2];
        const float d = fmaxf(sqrtf(ss), 1e-12f);
        for (int ch = 0; ch < 3; ++ch) v[ch] = (n[ch] / d + 1.f) / 2.f;
      }
      for (int ch = 0; ch < 3; ++ch) v[ch] = fminf(fmaxf(v[ch], 0.f), 1.f);
      if (MODE == M_NORMAL_F32) {
        for (int ch = 0; ch < 3; ++ch)
          *(float*)(o + ((size_t)ch * H + oy) * a.stride + (size_t)ox * 4) = v[ch];
      } else {
        uint8_t* row = u8_row_slot<PW>(s_row, o, a.stride, oy, c0, r, c);
        for (int ch = 0; ch < 3; ++ch) row[ch] = (uint8_t)(v[ch] * 255.0f);  // ToPILImage: mul(255).byte() truncates
      }
    } else {
      const float v = depth_value(y + (size_t)i * hw, w, cub_axis(h, a.sy, oy), cx);
      if (MODE == M_DEPTH_F32) {
        *(float*)(o + (size_t)oy * a.stride + (size_t)ox * 4) = v;
      } else {
        const float n = hi > lo ? (v - lo) / (hi - lo) : 0.f;
        const float s = n * 256.0f;
        const int idx = s >= 255.f ? 255 : (s > 0.f ? (int)s : 0);  // NaN -> 0
        *(uint32_t*)(o + (size_t)oy * a.stride + (size_t)ox * 4) = s_lut[idx];
      }
    }
  }

  if (MODE == M_NORMAL_U8) {
    __syncthreads();
    flush_u8_rows<PW, PH>(s_row, o, a.stride, r0, c0, H, W);
  }
}

// grid (MM_PARTS, images): block p of an image walks its tiles p, p + 64, ... and leaves one (min, max) pair
__global__ __launch_bounds__(256) void depth_minmax_kernel(const float* __restrict__ y, int h, int w, OutArgs args,
                                                           float* __restrict__ part) {
  __shared__ float s_lo[256], s_hi[256];
  const int tid = threadIdx.x;
  const int i = blockIdx.y;
  const OutArg a = args.d[i];
  const int H = a.H, W = a.W;
  const int tiles_x = (W + PW - 1) / PW, ntiles = tiles_of(H, W);
  const float* src = y + (size_t)i * h * w;
  float lo = INFINITY, hi = -INFINITY;
  for (int tile = blockIdx.x; tile < ntiles; tile += MM_PARTS) {
    const int c0 = (tile % tiles_x) * PW, r0 = (tile / tiles_x) * PH;
    const int ox = c0 + tid % PW;
    const Cub cx = cub_axis(w, a.sx, min(ox, W - 1));
    for (int r = tid / PW; r < PH; r += 256 / PW) {
      const int oy = r0 + r;
      if (oy >= H || ox >= W) continue;
      const float v = depth_value(src, w, cub_axis(h, a.sy, oy), cx);
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  s_lo[tid] = lo;
  s_hi[tid] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      s_lo[tid] = fminf(s_lo[tid], s_lo[tid + s]);
      s_hi[tid] = fmaxf(s_hi[tid], s_hi[tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[((size_t)i * MM_PARTS + blockIdx.x) * 2] = s_lo[0];
    part[((size_t)i * MM_PARTS + blockIdx.x) * 2 + 1] = s_hi[0];
  }
}

int bytes_per_pixel(int base) { return base == M_NORMAL_U8 ? 3 : 4; }

bool fill_out_arg(const dptx_image_desc& d, int base, int h, int w, OutArg& a) {
  if (d.offset < 0 || d.H < 1 || d.W < 1 || d.H > 16384 || d.W > 16384) return false;
  if ((long long)d.row_stride_bytes < (long long)d.W * bytes_per_pixel(base)) return false;
  if (base != M_NORMAL_U8 && ((d.offset & 3) || (d.row_stride_bytes & 3))) return false;  // dword stores
  a.offset = d.offset;
  a.H = d.H; a.W = d.W; a.stride = d.row_stride_bytes;
  a.tile0 = 0;
  a.sy = (float)h / (float)d.H;
  a.sx = (float)w / (float)d.W;
  return true;
}

}  // namespace

extern "C" {

int dptx_preprocess_rect_batch_workspace_bytes(int32_t B, int32_t OH, int32_t OW, int64_t* bytes) {
  if (!bytes || B < 1 || B > 4096 || OH < 64 || OH > 1024 || OH % 32 || OW < 64 || OW > 1024 || OW % 32) return DPTX_E_INVALID;
  *bytes = (int64_t)CHUNK * slot_ints(OH, OW) * sizeof(int);
  return DPTX_OK;
}

}  // extern "C"

namespace {
// both rectangular entries; flips = nullptr and MIRROR = false: the plain one
template <bool MIRROR>
int rect_batch(const void* pixels_dev, const dptx_image_desc* descs, const uint8_t* flips, int32_t B, int32_t OH, int32_t OW,
               int32_t depth_normalize, void* x_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t need = 0;
  if (!pixels_dev || !descs || !x_dev || !workspace || dptx_preprocess_rect_batch_workspace_bytes(B, OH, OW, &need) != DPTX_OK ||
      workspace_bytes < need || ((uintptr_t)workspace & 3) || ((uintptr_t)x_dev & 3))
    return DPTX_E_INVALID;
  ImgArg probe;
  for (int i = 0; i < B; ++i)
    if (!fill_rect_arg(descs[i], OH, OW, probe)) return DPTX_E_INVALID;  // the whole batch is checked before the first launch
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int n = B - b0 < CHUNK ? B - b0 : CHUNK;
    ImgArgs args = {};
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
      fill_rect_arg(descs[b0 + i], OH, OW, args.d[i]);
      args.d[i].pad = tiles;
      args.d[i].flip = MIRROR && flips && flips[b0 + i] ? 1 : 0;
      tiles += (OW / TC) * (OH / args.d[i].tr);
    }
    // the chunks share the workspace: they are ordered on the stream
    hipLaunchKernelGGL(coeff_rect_kernel, dim3((OH + OW + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, args, n, OH, OW,
                       (int*)workspace);
    hipLaunchKernelGGL(MIRROR ? resize_views_kernel : resize_rect_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)pixels_dev, args, n, OH, OW, (const int*)workspace, depth_normalize,
                       (float*)x_dev + (size_t)b0 * 3 * OH * OW);
  }
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}
}  // namespace

extern "C" {

int dptx_preprocess_u8_rect_batch(const void* pixels_dev, const dptx_image_desc* descs, int32_t B, int32_t OH, int32_t OW,
                                  int32_t depth_normalize, void* x_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return rect_batch<false>(pixels_dev, descs, nullptr, B, OH, OW, depth_normalize, x_dev, workspace, workspace_bytes, stream);
}

int dptx_preprocess_u8_views_batch(const void* pixels_dev, const dptx_image_desc* descs, const uint8_t* flips, int32_t B, int32_t OH,
                                   int32_t OW, int32_t depth_normalize, void* x_dev, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  return rect_batch<true>(pixels_dev, descs, flips, B, OH, OW, depth_normalize, x_dev, workspace, workspace_bytes, stream);
}

int dptx_postprocess_resize_workspace_bytes(int32_t B, int32_t mode, int64_t* bytes) {
  const int base = mode & ~DPTX_RESIZE_RENORM;
  if (!bytes || B < 1 || B > 4096 || base < M_NORMAL_U8 || base > M_DEPTH_RGBA) return DPTX_E_INVALID;
  if ((mode & DPTX_RESIZE_RENORM) && base != M_NORMAL_U8 && base != M_NORMAL_F32) return DPTX_E_INVALID;
  *bytes = base == M_DEPTH_RGBA ? (int64_t)CHUNK * MM_PARTS * 2 * sizeof(float) : 0;
  return DPTX_OK;
}

int dptx_postprocess_resize_batch(const void* y_dev, int32_t B, int32_t C, int32_t h, int32_t w, const dptx_image_desc* descs,
                                  int32_t mode, void* out_dev, const void* lut_dev, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  int64_t need = 0;
  if (!y_dev || !descs || !out_dev || dptx_postprocess_resize_workspace_bytes(B, mode, &need) != DPTX_OK || h < 1 || w < 1 ||
      h > 4096 || w > 4096 || ((uintptr_t)y_dev & 3))
    return DPTX_E_INVALID;
  const int base = mode & ~DPTX_RESIZE_RENORM, renorm = (mode & DPTX_RESIZE_RENORM) ? 1 : 0;
  const bool normal = base == M_NORMAL_U8 || base == M_NORMAL_F32;
  if (C != (normal ? 3 : 1)) return DPTX_E_INVALID;
  if (base != M_NORMAL_U8 && ((uintptr_t)out_dev & 3)) return DPTX_E_INVALID;
  if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3) || !lut_dev || ((uintptr_t)lut_dev & 3)))
    return DPTX_E_INVALID;
  OutArg probe;
  for (int i = 0; i < B; ++i)
    if (!fill_out_arg(descs[i], base, h, w, probe)) return DPTX_E_INVALID;  // the whole batch is checked before the first launch
  const hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int n = B - b0 < CHUNK ? B - b0 : CHUNK;
    OutArgs args = {};
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
      fill_out_arg(descs[b0 + i], base, h, w, args.d[i]);
      args.d[i].tile0 = tiles;
      tiles += tiles_of(args.d[i].H, args.d[i].W);
    }
    const float* y = (const float*)y_dev + (size_t)b0 * C * h * w;
    uint8_t* out = (uint8_t*)out_dev;
    const uint32_t* lut = (const uint32_t*)lut_dev;
    float* part = (float*)workspace;
    switch (base) {
      case M_NORMAL_U8:
        hipLaunchKernelGGL(post_resize_kernel<M_NORMAL_U8>, dim3(tiles), dim3(256), 0, st, y, h, w, args, n, renorm, out, lut, part);
        break;
      case M_NORMAL_F32:
        hipLaunchKernelGGL(post_resize_kernel<M_NORMAL_F32>, dim3(tiles), dim3(256), 0, st, y, h, w, args, n, renorm, out, lut, part);
        break;
      case M_DEPTH_F32:
        hipLaunchKernelGGL(post_resize_kernel<M_DEPTH_F32>, dim3(tiles), dim3(256), 0, st, y, h, w, args, n, renorm, out, lut, part);
        break;
      default:
        // the chunks share the workspace: they are ordered on the stream
        hipLaunchKernelGGL(depth_minmax_kernel, dim3(MM_PARTS, n), dim3(256), 0, st, y, h, w, args, part);
        hipLaunchKernelGGL(post_resize_kernel<M_DEPTH_RGBA>, dim3(tiles), dim3(256), 0, st, y, h, w, args, n, renorm, out, lut, part);
        break;
    }
  }
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
