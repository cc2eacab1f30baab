// tta_common.h -- what the two merges of test-time augmentation share (tta.hip: surface normals; tta_depth.hip: depth): the output
// tile, the view descriptors that travel by value in the kernel arguments, the in-register selection of the M smallest values,
// the decode of a normal (tta.hip and the blend of tiles.hip) and the host-side checks of a call's views and outputs.  Contraction is off here as in resample_batch.h, whose taps both use.
#pragma once
#include "resample_batch.h"

namespace {

constexpr int TW = 64, TH = 4;  // output tile: columns x rows; 256 threads, one pixel each
constexpr int MAXV = DPTX_TTA_MAX_VIEWS;

struct ViewArg {
  long long first;  // index of the view's first float in views_dev
  int h, w;
  int y0, x0, ch, cw;
  int flip, pad;
  float sy, sx;  // ATen's area_pixel_compute_scale: (float)in / (float)out, divided once on the host
};
struct ViewArgs {
  ViewArg v[MAXV];  // 64 * 48 B of kernel arguments
};
struct MergeOut {
  long long offset;
  int H, W, stride, pad;
};

template <int M>
struct Lowest {  // the M smallest values so far, ascending
  float a[M > 0 ? M : 1];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < M; ++j) a[j] = INFINITY;
  }
  __device__ __forceinline__ void insert(float v) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const float lo = fminf(a[j], v);
      v = fmaxf(a[j], v);
      a[j] = lo;
    }
  }
  // a[i]: the list is ascending, so it is the largest of a[0..i].  (Written as a chain of `j == i ? a[j] : r` the compiler
  // turns the selects back into an indexed load, and the list into scratch.)
  __device__ __forceinline__ float at(int i) const {
    float r = a[0];
#pragma unroll
    for (int j = 1; j < M; ++j) r = fmaxf(r, j <= i ? a[j] : -INFINITY);
    return r;
  }
};

// a normal at `at` of a view's [3][plane] map: 2m - 1, then F.normalize over the channels (eps 1e-12) unless raw
__device__ __forceinline__ void decode(const float* __restrict__ p, int plane, int at, int raw, float n[3]) {
  for (int c = 0; c < 3; ++c) n[c] = 2.f * p[c * plane + at] - 1.f;
  if (!raw) {
    float ss = n[0] * n[0];
    ss += n[1] * n[1];
    ss += n[2] * n[2];
    const float d = fmaxf(sqrtf(ss), 1e-12f);
    for (int c = 0; c < 3; ++c) n[c] = n[c] / d;
  }
}

// bpp: bytes per pixel of the output, 3 (uint8 triples at any byte) or 4 (dword stores)
inline bool out_ok(const dptx_image_desc& d, int bpp) {
  if (d.offset < 0 || d.H < 1 || d.W < 1 || d.H > 16384 || d.W > 16384) return false;
  if ((long long)d.row_stride_bytes < (long long)d.W * bpp) return false;
  return bpp == 3 || !((d.offset & 3) || (d.row_stride_bytes & 3));
}

inline bool view_ok(const dptx_tta_view& v, const dptx_image_desc& d) {
  if (v.offset < 0 || (v.offset & 3) || v.h < 1 || v.w < 1 || v.h > 4096 || v.w > 4096) return false;
  if (v.y0 < 0 || v.x0 < 0 || v.ch < 1 || v.cw < 1) return false;
  return (long long)v.y0 + v.ch <= d.H && (long long)v.x0 + v.cw <= d.W;
}

// every image has 1..64 consecutive views, images ascending from 0 to B - 1, every view inside its image
inline bool views_ok(const dptx_tta_view* views, int n_views, const dptx_image_desc* outs, int B) {
  int expect = 0, count = 0;
  for (int k = 0; k < n_views; ++k) {
    const int img = views[k].image;
    if (img == expect + 1 && count > 0) {
      expect = img;
      count = 0;
    }
    if (img != expect || img >= B || ++count > MAXV || !view_ok(views[k], outs[img])) return false;
  }
  return expect == B - 1;
}

inline ViewArg view_arg(const dptx_tta_view& v) {
  ViewArg a = {};
  a.first = v.offset / 4;
  a.h = v.h; a.w = v.w;
  a.y0 = v.y0; a.x0 = v.x0; a.ch = v.ch; a.cw = v.cw;
  a.flip = v.flip ? 1 : 0;
  a.sy = (float)v.h / (float)v.ch;
  a.sx = (float)v.w / (float)v.cw;
  return a;
}

}  // namespace
