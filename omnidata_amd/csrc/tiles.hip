// tiles.hip -- tiled high-resolution inference (include/dptx.h, "Tiled inference"): an image is cut into a grid of overlapping
// windows of one size, every window goes through the network at one network size, and the maps are blended back into a map of the
// image's own size with a weight that ramps down towards every window edge that is not on the image border.  Stream-ordered, the
// caller's workspace only, no allocation, no host synchronisation, no atomics; one blend launch per image with the image's grid
// (568 bytes: the two lists of starts) by value in the arguments, so up to 64 x 64 tiles cost no descriptor upload.
//
// Blend: block = 64 columns x 4 rows of one image, a thread owns one pixel (tta.hip's tile, and its uint8 row staging).  All
//   windows of an axis have one size and their starts ascend, so the tiles that reach the block's rows (columns) are a range
//   [iy0, iy1] ([ix0, ix1]) of the axis: the block finds both ranges with scalar loops over the starts (uniform: SALU and scalar
//   loads of the arguments), and a pixel then visits only those tiles -- 1 to 3 per axis with the planner's grids, whatever the
//   grid's size -- and skips the ones of the range that miss it.  Nothing is assumed about how many tiles cover a pixel.  The order
//   is iy ascending, then ix ascending; every step is an fp32 multiply, then an add (contraction is off, resample_batch.h).
// Tile value: tta.hip's (normals: decode, normalise at the network's resolution, bilinear) and tta_depth_align.h's view_value
//   (depth) for an unflipped view, the same operations in the same order: a 1 x 1 grid gives the bits of the TTA merges' mean.
// Alignment (depth): the anchor, stats and solve kernels of tta_depth_align.h, the device code dptx_tta_align_depth runs, driven
//   in chunks of at most 63 tiles plus the anchor -- the anchor sits behind the chunk's tiles with no records, and the solve is
//   launched over the tiles only.  The anchor is resized once per image; the chunks of all images share one region of records
//   (the launches of a stream run one after the other).
#include "tta_depth_align.h"

namespace {

constexpr int M_U8 = DPTX_RESIZE_NORMAL_U8, M_F32 = DPTX_RESIZE_NORMAL_F32;
constexpr int MAXT = DPTX_TILE_MAX_AXIS;  // tiles per axis
constexpr int CHUNK_TILES = MAXV - 1;     // tiles per alignment chunk: the 64th view is the anchor

struct GridArg {
  long long first;  // index of tile (0, 0)'s first float in views_dev
  int h, w, ch, cw;
  int ny, nx, ry, rx;
  float sy, sx;  // (float)h / (float)ch, (float)w / (float)cw
  int y0[MAXT], x0[MAXT];
};

// the weight along one axis at local coordinate t of a window of c pixels: a ramp of r pixels at an edge inside the image
__device__ __forceinline__ float axis_weight(int t, int c, int r, bool first, bool last) {
  const float left = (first || r == 0) ? 1.f : fminf(1.f, ((float)t + 0.5f) / (float)r);
  const float right = (last || r == 0) ? 1.f : fminf(1.f, ((float)(c - 1 - t) + 0.5f) / (float)r);
  return left * right;
}

// the tiles of an axis (n starts s[], ascending, windows of c pixels, no gap) that reach [lo, hi], lo <= hi inside the axis
__device__ __forceinline__ void covering(const int* s, int n, int c, int lo, int hi, int& i0, int& i1) {
  i0 = 0;
  while (i0 + 1 < n && s[i0] + c <= lo) ++i0;
  i1 = i0;
  while (i1 + 1 < n && s[i1 + 1] <= hi) ++i1;
}

template <int MODE>
__global__ __launch_bounds__(256) void tile_blend_normals_kernel(const float* __restrict__ views, GridArg g, MergeOut o, int raw,
                                                                 uint8_t* __restrict__ out) {
  __shared__ uint32_t s_row[MODE == M_U8 ? TH * row_dw(TW) : 1];
  const int tid = threadIdx.x;
  const int tiles_x = (o.W + TW - 1) / TW;
  const int c0 = (blockIdx.x % tiles_x) * TW, r0 = (blockIdx.x / tiles_x) * TH;
  const int c = tid % TW, r = tid / TW;
  const int X = c0 + c, Y = r0 + r;
  const bool inside = X < o.W && Y < o.H;
  uint8_t* dst = out + o.offset;

  int iy0, iy1, ix0, ix1;  // uniform over the block
  covering(g.y0, g.ny, g.ch, r0, min(r0 + TH, o.H) - 1, iy0, iy1);
  covering(g.x0, g.nx, g.cw, c0, min(c0 + TW, o.W) - 1, ix0, ix1);

  const int plane = g.h * g.w;  // <= 2^24
  float acc[3] = {0.f, 0.f, 0.f};
  for (int iy = iy0; iy <= iy1; ++iy) {
    const int ys = g.y0[iy], ly = Y - ys;
    if (!inside || ly < 0 || ly >= g.ch) continue;
    const float wy = axis_weight(ly, g.ch, g.ry, ys == 0, ys + g.ch == o.H);
    const Lin ay = lin_axis(g.h, g.ch, g.sy, ly);
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int xs = g.x0[ix], lx = X - xs;
      if (lx < 0 || lx >= g.cw) continue;
      const float wgt = wy * axis_weight(lx, g.cw, g.rx, xs == 0, xs + g.cw == o.W);
      const Lin ax = lin_axis(g.w, g.cw, g.sx, lx);
      const float* p = views + g.first + (long long)(iy * g.nx + ix) * 3 * plane;
      float n00[3], n01[3], n10[3], n11[3];
      decode(p, plane, ay.i0 * g.w + ax.i0, raw, n00);
      decode(p, plane, ay.i0 * g.w + ax.i1, raw, n01);
      decode(p, plane, ay.i1 * g.w + ax.i0, raw, n10);
      decode(p, plane, ay.i1 * g.w + ax.i1, raw, n11);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float t0 = ax.l0 * n00[ch];
        t0 += ax.l1 * n01[ch];
        float t1 = ax.l0 * n10[ch];
        t1 += ax.l1 * n11[ch];
        float t = ay.l0 * t0;
        t += ay.l1 * t1;
        t = wgt * t;
        acc[ch] += t;
      }
    }
  }

  float v[3];
  float ss = acc[0] * acc[0];
  ss += acc[1] * acc[1];
  ss += acc[2] * acc[2];
  const float d = fmaxf(sqrtf(ss), 1e-12f);
  for (int ch = 0; ch < 3; ++ch) v[ch] = fminf(fmaxf((acc[ch] / d + 1.f) / 2.f, 0.f), 1.f);

  if (MODE == M_F32) {
    if (inside)
      for (int ch = 0; ch < 3; ++ch) *(float*)(dst + ((size_t)ch * o.H + Y) * o.stride + (size_t)X * 4) = v[ch];
  } else {
    if (inside) {
      uint8_t* row = u8_row_slot<TW>(s_row, dst, o.stride, Y, c0, r, c);
      for (int ch = 0; ch < 3; ++ch) row[ch] = (uint8_t)(v[ch] * 255.0f);  // ToPILImage: mul(255).byte() truncates
    }
    __syncthreads();
    flush_u8_rows<TW, TH>(s_row, dst, o.stride, r0, c0, o.H, o.W);
  }
}

__global__ __launch_bounds__(256) void tile_blend_depth_kernel(const float* __restrict__ views, GridArg g, MergeOut o,
                                                               const float* __restrict__ coeffs, uint8_t* __restrict__ out) {
  const int tid = threadIdx.x;
  const int tiles_x = (o.W + TW - 1) / TW;
  const int c0 = (blockIdx.x % tiles_x) * TW, r0 = (blockIdx.x / tiles_x) * TH;
  const int X = c0 + tid % TW, Y = r0 + tid / TW;
  const bool inside = X < o.W && Y < o.H;

  int iy0, iy1, ix0, ix1;  // uniform over the block
  covering(g.y0, g.ny, g.ch, r0, min(r0 + TH, o.H) - 1, iy0, iy1);
  covering(g.x0, g.nx, g.cw, c0, min(c0 + TW, o.W) - 1, ix0, ix1);

  ViewArg a = {};  // a tile as view_value takes it: the window's origin is not used there
  a.h = g.h; a.w = g.w; a.ch = g.ch; a.cw = g.cw;
  a.sy = g.sy; a.sx = g.sx;
  const long long plane = (long long)g.h * g.w;
  float acc = 0.f, wsum = 0.f;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const int ys = g.y0[iy], ly = Y - ys;
    if (!inside || ly < 0 || ly >= g.ch) continue;
    const float wy = axis_weight(ly, g.ch, g.ry, ys == 0, ys + g.ch == o.H);
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int xs = g.x0[ix], lx = X - xs;
      if (lx < 0 || lx >= g.cw) continue;
      const float wgt = wy * axis_weight(lx, g.cw, g.rx, xs == 0, xs + g.cw == o.W);
      const int k = iy * g.nx + ix;
      a.first = g.first + k * plane;
      float t = view_value(views, a, ly, lx);
      if (coeffs) {
        t = coeffs[2 * k] * t;
        t += coeffs[2 * k + 1];
      }
      t = wgt * t;
      acc += t;
      wsum += wgt;
    }
  }
  const float v = acc / wsum;  // wsum >= 1 wherever the grid covers, and it covers the image
  if (inside) *(float*)(out + o.offset + (size_t)Y * o.stride + (size_t)X * 4) = 1.f - fminf(fmaxf(v, 0.f), 1.f);
}

// ------------------------------------------------------------------------------------------------ host
// starts ascending from 0, no gap between neighbouring windows, the last window ends at L
inline bool axis_ok(const int32_t* s, int n, int c, int L) {
  if (n < 1 || n > MAXT || c < 1 || c > L || s[0] != 0) return false;
  for (int i = 1; i < n; ++i)
    if (s[i] <= s[i - 1] || s[i] > s[i - 1] + c) return false;
  return (long long)s[n - 1] + c == L;
}

inline bool grid_ok(const dptx_tile_grid& t, const dptx_image_desc& d) {
  if (t.offset < 0 || (t.offset & 3) || t.h < 1 || t.w < 1 || t.h > 4096 || t.w > 4096) return false;
  if (t.ramp_y < 0 || t.ramp_x < 0) return false;
  return axis_ok(t.y0, t.ny, t.ch, d.H) && axis_ok(t.x0, t.nx, t.cw, d.W);
}

inline bool anchor_ok(const dptx_tile_grid& t) {
  return t.anchor_offset >= 0 && !(t.anchor_offset & 3) && t.ah >= 1 && t.aw >= 1 && t.ah <= 4096 && t.aw <= 4096;
}

// the whole call is checked before the first launch; bpp as out_ok takes it
bool call_ok(const dptx_tile_grid* grids, const dptx_image_desc* outs, int B, int bpp) {
  if (!grids || !outs || B < 1 || B > 4096) return false;
  for (int i = 0; i < B; ++i)
    if (!out_ok(outs[i], bpp) || !grid_ok(grids[i], outs[i])) return false;
  return true;
}

inline GridArg grid_arg(const dptx_tile_grid& t) {
  GridArg g = {};
  g.first = t.offset / 4;
  g.h = t.h; g.w = t.w; g.ch = t.ch; g.cw = t.cw;
  g.ny = t.ny; g.nx = t.nx; g.ry = t.ramp_y; g.rx = t.ramp_x;
  g.sy = (float)t.h / (float)t.ch;
  g.sx = (float)t.w / (float)t.cw;
  for (int i = 0; i < t.ny; ++i) g.y0[i] = t.y0[i];
  for (int i = 0; i < t.nx; ++i) g.x0[i] = t.x0[i];
  return g;
}

// workspace: [anchor plane of image 0 | ... | of image B - 1 | the records of one chunk], each part at a multiple of 256 bytes
long long layout(const dptx_tile_grid* grids, const dptx_image_desc* outs, int B, long long* plane_at, long long* records_at) {
  long long at = 0, records = 0;
  for (int i = 0; i < B; ++i) {
    if (plane_at) plane_at[i] = at;
    at += dptx::align256(4ll * outs[i].H * outs[i].W);
    const long long n = (long long)grids[i].ny * grids[i].nx;
    records = std::max(records, std::min<long long>(n, CHUNK_TILES) * stats_tiles(grids[i].ch, grids[i].cw));
  }
  if (records_at) *records_at = at;
  return at + dptx::align256(records * NSUM * (long long)sizeof(double));
}

}  // namespace

extern "C" int dptx_tile_blend_normals(const void* views_dev, const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B,
                                       int32_t mode, void* out_dev, void* stream) {
  if (!views_dev || ((uintptr_t)views_dev & 3) || !out_dev) return DPTX_E_INVALID;
  const int base = mode & ~DPTX_TTA_RAW_VIEWS;
  if (mode < 0 || (base != M_U8 && base != M_F32)) return DPTX_E_INVALID;
  if (base == M_F32 && ((uintptr_t)out_dev & 3)) return DPTX_E_INVALID;
  if (!call_ok(grids, outs, B, base == M_U8 ? 3 : 4)) return DPTX_E_INVALID;

  const int raw = (mode & DPTX_TTA_RAW_VIEWS) ? 1 : 0;
  const hipStream_t st = (hipStream_t)stream;
  const float* src = (const float*)views_dev;
  uint8_t* out = (uint8_t*)out_dev;
  for (int i = 0; i < B; ++i) {
    const GridArg g = grid_arg(grids[i]);
    const dptx_image_desc& d = outs[i];
    const MergeOut o = {d.offset, d.H, d.W, d.row_stride_bytes, 0};
    const int tiles = ((d.W + TW - 1) / TW) * ((d.H + TH - 1) / TH);  // <= 2^20
    if (base == M_U8) hipLaunchKernelGGL((tile_blend_normals_kernel<M_U8>), dim3(tiles), dim3(256), 0, st, src, g, o, raw, out);
    else hipLaunchKernelGGL((tile_blend_normals_kernel<M_F32>), dim3(tiles), dim3(256), 0, st, src, g, o, raw, out);
  }
  return dptx::launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

extern "C" int dptx_tile_depth_workspace_bytes(const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B, int64_t* bytes) {
  if (!bytes || !call_ok(grids, outs, B, 4)) return DPTX_E_INVALID;
  *bytes = layout(grids, outs, B, nullptr, nullptr);
  return DPTX_OK;
}

extern "C" int dptx_tile_align_depth(const void* views_dev, const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B,
                                     float* coeffs_dev, void* ws, int64_t ws_bytes, void* stream) {
  if (!views_dev || ((uintptr_t)views_dev & 3) || !call_ok(grids, outs, B, 4) || !coeffs_dev || ((uintptr_t)coeffs_dev & 3) || !ws ||
      ((uintptr_t)ws & 7))
    return DPTX_E_INVALID;
  for (int i = 0; i < B; ++i)
    if (!anchor_ok(grids[i])) return DPTX_E_INVALID;
  long long plane_at[4096], records_at = 0;
  if (ws_bytes < layout(grids, outs, B, plane_at, &records_at)) return DPTX_E_INVALID;

  const hipStream_t st = (hipStream_t)stream;
  const float* src = (const float*)views_dev;
  double* records = (double*)((char*)ws + records_at);
  size_t k0 = 0;  // the image's first tile in coeffs_dev
  for (int i = 0; i < B; ++i) {
    const dptx_tile_grid& t = grids[i];
    const dptx_image_desc& d = outs[i];
    const dptx_tta_view whole = {t.anchor_offset, t.ah, t.aw, i, 0, 0, d.H, d.W, 0};
    const ViewArg anchor = view_arg(whole);
    float* plane = (float*)((char*)ws + plane_at[i]);
    const int out_tiles = ((d.W + TW - 1) / TW) * ((d.H + TH - 1) / TH);
    hipLaunchKernelGGL(tta_depth_anchor_kernel, dim3(out_tiles), dim3(256), 0, st, src, anchor, d.H, d.W, plane);
    const int n_tiles = t.ny * t.nx;
    const long long rt = stats_tiles(t.ch, t.cw);  // <= 2^18
    const long long map_bytes = 4ll * t.h * t.w;
    for (int t0 = 0; t0 < n_tiles; t0 += CHUNK_TILES) {
      const int n = std::min(CHUNK_TILES, n_tiles - t0);
      ViewArgs args = {};
      StatsArgs sa = {};
      for (int j = 0; j < n; ++j) {
        const int k = t0 + j;
        const dptx_tta_view v = {t.offset + k * map_bytes, t.h, t.w, i, t.y0[k / t.nx], t.x0[k % t.nx], t.ch, t.cw, 0};
        args.v[j] = view_arg(v);
        sa.first[j] = (int)(j * rt);
      }
      args.v[n] = anchor;  // behind the chunk's tiles, without records: no block of the stats pass or the solve is its own
      sa.first[n] = sa.first[n + 1] = (int)(n * rt);
      hipLaunchKernelGGL(tta_depth_stats_kernel, dim3((unsigned)(n * rt)), dim3(256), 0, st, src, args, sa, n + 1, n, d.W, plane,
                         records);
      hipLaunchKernelGGL(tta_depth_solve_kernel, dim3(n), dim3(64), 0, st, args, sa, n, records, coeffs_dev + 2 * (k0 + t0));
    }
    k0 += (size_t)n_tiles;
  }
  return dptx::launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

extern "C" int dptx_tile_blend_depth(const void* views_dev, const dptx_tile_grid* grids, const float* coeffs_dev,
                                     const dptx_image_desc* outs, int32_t B, int32_t mode, void* out_dev, void* stream) {
  if (!views_dev || ((uintptr_t)views_dev & 3) || !out_dev || ((uintptr_t)out_dev & 3) || ((uintptr_t)coeffs_dev & 3))
    return DPTX_E_INVALID;
  if (mode != DPTX_RESIZE_DEPTH_F32 || !call_ok(grids, outs, B, 4)) return DPTX_E_INVALID;

  const hipStream_t st = (hipStream_t)stream;
  const float* src = (const float*)views_dev;
  uint8_t* out = (uint8_t*)out_dev;
  size_t k0 = 0;
  for (int i = 0; i < B; ++i) {
    const GridArg g = grid_arg(grids[i]);
    const dptx_image_desc& d = outs[i];
    const MergeOut o = {d.offset, d.H, d.W, d.row_stride_bytes, 0};
    const int tiles = ((d.W + TW - 1) / TW) * ((d.H + TH - 1) / TH);  // <= 2^20
    hipLaunchKernelGGL(tile_blend_depth_kernel, dim3(tiles), dim3(256), 0, st, src, g, o, coeffs_dev ? coeffs_dev + 2 * k0 : nullptr,
                       out);
    k0 += (size_t)grids[i].ny * grids[i].nx;
  }
  return dptx::launch_ok() ? DPTX_OK : DPTX_E_HIP;
}
