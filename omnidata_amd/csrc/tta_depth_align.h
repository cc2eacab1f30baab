// tta_depth_align.h -- the device code of the depth alignment, shared by the two units that fit maps of windows to a whole-image
// anchor (tta_depth.hip: the views of test-time augmentation; tiles.hip: the tiles of tiled inference): the value of a view at a
// pixel of its window, the anchor pass, the stats pass and the solve (include/dptx.h, "Test-time augmentation for depth", steps
// 1 to 3).  Both units launch these kernels with the same arguments for the same window, so a window's coefficients have the same
// bits whichever entry point computed them.  tta_depth.hip's head describes the passes.
#pragma once
#include "tta_common.h"
#include "select.h"

namespace {

constexpr int SW = 64, SH = 16;  // stats tile: columns x rows of a view's window; 256 threads, 4 rows each
constexpr int NSUM = 4;          // sum r, sum r^2, sum a, sum r a

// the value of view `a` at (ly, lx) of its window, ly in [0, ch), lx in [0, cw): clamp at the network's resolution, bilinear
__device__ __forceinline__ float view_value(const float* __restrict__ views, const ViewArg& a, int ly, int lx) {
  if (a.flip) lx = a.cw - 1 - lx;
  const Lin ay = lin_axis(a.h, a.ch, a.sy, ly);
  const Lin ax = lin_axis(a.w, a.cw, a.sx, lx);
  const float* p = views + a.first;
  const float d00 = fminf(fmaxf(p[ay.i0 * a.w + ax.i0], 0.f), 1.f);
  const float d01 = fminf(fmaxf(p[ay.i0 * a.w + ax.i1], 0.f), 1.f);
  const float d10 = fminf(fmaxf(p[ay.i1 * a.w + ax.i0], 0.f), 1.f);
  const float d11 = fminf(fmaxf(p[ay.i1 * a.w + ax.i1], 0.f), 1.f);
  float t0 = ax.l0 * d00;
  t0 += ax.l1 * d01;
  float t1 = ax.l0 * d10;
  t1 += ax.l1 * d11;
  float t = ay.l0 * t0;
  t += ay.l1 * t1;
  return t;
}

__global__ __launch_bounds__(256) void tta_depth_anchor_kernel(const float* __restrict__ views, ViewArg a, int H, int W,
                                                               float* __restrict__ plane) {
  const int tiles_x = (W + TW - 1) / TW;
  const int X = (blockIdx.x % tiles_x) * TW + threadIdx.x % TW, Y = (blockIdx.x / tiles_x) * TH + threadIdx.x / TW;
  if (X < W && Y < H) plane[(size_t)Y * W + X] = view_value(views, a, Y, X);  // the anchor's window is the image
}

struct StatsArgs {
  int first[MAXV + 1];  // view k's records are [first[k], first[k + 1]) of the image's list; block b of the grid writes record b
};

__global__ __launch_bounds__(256) void tta_depth_stats_kernel(const float* __restrict__ views, ViewArgs args, StatsArgs sa, int nv,
                                                              int anchor, int W, const float* __restrict__ plane,
                                                              double* __restrict__ partial) {
  __shared__ double red[4 * NSUM];
  int k = 0;
  while (k + 1 < nv && (int)blockIdx.x >= sa.first[k + 1]) ++k;  // uniform over the block
  if (k == anchor) return;                                       // its coefficients are (1, 0) by definition
  const ViewArg a = args.v[k];
  const int tile = blockIdx.x - sa.first[k];
  const int tiles_x = (a.cw + SW - 1) / SW;
  const int lx = (tile % tiles_x) * SW + threadIdx.x % SW;
  const int ly0 = (tile / tiles_x) * SH + threadIdx.x / SW;
  double s[NSUM] = {0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < SH / 4; ++j) {
    const int ly = ly0 + 4 * j;
    if (lx < a.cw && ly < a.ch) {
      const double r = (double)view_value(views, a, ly, lx);
      const double t = (double)plane[(size_t)(a.y0 + ly) * W + a.x0 + lx];
      s[0] += r;
      s[1] += r * r;
      s[2] += t;
      s[3] += r * t;
    }
  }
  dptx::block_sum<NSUM>(s, red, partial + (size_t)blockIdx.x * NSUM);
}

__global__ __launch_bounds__(64) void tta_depth_solve_kernel(ViewArgs args, StatsArgs sa, int anchor,
                                                             const double* __restrict__ partial, float* __restrict__ coeffs) {
  const int k = blockIdx.x, lane = threadIdx.x;
  double s[NSUM] = {0.0, 0.0, 0.0, 0.0};
  if (k != anchor)
    for (int j = sa.first[k] + lane; j < sa.first[k + 1]; j += 64)
#pragma unroll
      for (int q = 0; q < NSUM; ++q) s[q] += partial[(size_t)j * NSUM + q];
#pragma unroll
  for (int q = 0; q < NSUM; ++q) s[q] = dptx::wave_sum(s[q]);
  if (lane != 0) return;
  float scale = 1.f, shift = 0.f;
  if (k != anchor) {
    const double n = (double)args.v[k].ch * (double)args.v[k].cw;
    const double sr = s[0], srr = s[1], st = s[2], srt = s[3];
    const double det = n * srr - sr * sr;
    if (det > 1e-10 * n * srr) {
      scale = (float)((n * srt - sr * st) / det);
      shift = (float)((srr * st - sr * srt) / det);
    } else {  // flatter than 1e-5 of its own level (or not finite): only the level is fitted
      shift = (float)((st - sr) / n);
    }
  }
  coeffs[2 * k] = scale;
  coeffs[2 * k + 1] = shift;
}

// records of one window: 64 x 16 tiles
inline long long stats_tiles(int ch, int cw) { return (long long)((cw + SW - 1) / SW) * ((ch + SH - 1) / SH); }

}  // namespace
