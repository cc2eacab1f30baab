// guided.hip -- guided full-frame upsampling (include/dptx.h, "Guided upsampling"): the network's maps y [B][C][h][w] -> B outputs of
// the images' own sizes, every output pixel a joint bilateral mean (Kopf et al. 2007) of the (2R)^2 map values around it.  The
// weights fall off with the distance in low-resolution pixels and with the colour difference between the full-resolution image
// at the output pixel (the packed uint8 pixels, G_hi) and the low-resolution image at the tap (the network input, G_lo).
// Stream-ordered, caller's workspace only, no allocation, no host synchronisation, no atomics; descriptors by value, 32 per launch.
//
//  Block = 64 output columns x 8 rows of ONE image, a wave per row; a thread keeps its column over two rows.  The block stages
//  the low-resolution footprint of its tile (the taps' bounding box, cut to the map) in LDS once: G_lo as one 16-byte cell,
//  S planar.  For any output at least as large as the map the footprint is at most (64 + 2R) x (8 + 2R) <= 980 cells and always
//  fits; a shrinking output whose footprint is larger reads its taps through the cache instead -- the same operations in the same
//  order, so the two paths give the same bits.  A thread holds the (2R)^2 exponents in registers between the two passes over
//  the taps: the minimum, then the weights and sums.
//  Mode steps, the uint8 rows that leave LDS as aligned dwords and the two launches of DEPTH_RGBA (64 partial minima / maxima per
//  image in the workspace, each block walks its image's tiles in a fixed order) are those of fullframe.hip.
// Contraction is off (resample_batch.h): every operation of the definition is rounded on its own, and the two launches of
// DEPTH_RGBA compute the same bits.
#include "resample_batch.h"

namespace {

constexpr int GW = 64, GH = 8;          // output tile: columns x rows; a thread keeps one column over GH * GW / 256 rows
static_assert(256 % GW == 0 && GH % (256 / GW) == 0, "a thread keeps one column of the tile");
constexpr int MAX_R = 3;
constexpr int CELLS = 1024;             // staged low-resolution cells of one tile
static_assert((GW + 2 * MAX_R) * (GH + 2 * MAX_R) <= CELLS, "the footprint of a tile that does not shrink always fits");
constexpr int MM_PARTS = 64;            // partial minima / maxima per image
constexpr int M_NORMAL_U8 = DPTX_RESIZE_NORMAL_U8, M_NORMAL_F32 = DPTX_RESIZE_NORMAL_F32, M_DEPTH_F32 = DPTX_RESIZE_DEPTH_F32,
              M_DEPTH_RGBA = DPTX_RESIZE_DEPTH_RGBA;

struct GArg {
  long long out_offset, guide_offset;
  int H, W, ostride, gstride, gC, tile0;  // tile0: the image's first tile of the launch
  float sy, sx;                           // (float)in / (float)out, divided once on the host
};
struct GArgs {
  GArg d[CHUNK];
};
struct Maps {  // one chunk's low-resolution inputs and the filter's constants
  const float* S;     // [n][C][h][w]
  const float* G;     // [n][3][h][w]
  int h, w;
  float ks, kr;
};

__host__ __device__ inline int tiles_of(int H, int W) { return ((W + GW - 1) / GW) * ((H + GH - 1) / GH); }

struct alignas(16) GuideCell {
  float g0, g1, g2, pad;  // one 16-byte read per tap
};
template <int C>
struct GuidedLds {
  GuideCell g[CELLS];  // G_lo of a cell
  float s[C][CELLS];  // S of a cell
};

// the taps of a tile lie in [y0, y1) x [x0, x1): their bounding box cut to the map (src_coord is monotonic in the destination)
struct Tile {
  int c0, r0, y0, y1, x0, x1;
  bool staged;
};

template <int R, int C>
__device__ __forceinline__ Tile stage_tile(GuidedLds<C>& lds, const Maps& m, const float* S, const float* G, const GArg& a, int tile) {
  Tile t;
  const int tiles_x = (a.W + GW - 1) / GW;
  t.c0 = (tile % tiles_x) * GW;
  t.r0 = (tile / tiles_x) * GH;
  const int rl = min(t.r0 + GH, a.H) - 1, cl = min(t.c0 + GW, a.W) - 1;
  t.y0 = max((int)floorf(src_coord(a.sy, t.r0)) - R + 1, 0);
  t.y1 = min((int)floorf(src_coord(a.sy, rl)) + R, m.h - 1) + 1;
  t.x0 = max((int)floorf(src_coord(a.sx, t.c0)) - R + 1, 0);
  t.x1 = min((int)floorf(src_coord(a.sx, cl)) + R, m.w - 1) + 1;
  const int fh = t.y1 - t.y0, fw = t.x1 - t.x0;
  t.staged = fh > 0 && fw > 0 && (long long)fh * fw <= CELLS;
  if (!t.staged) {  // the taps are tested against the map itself
    t.y0 = 0; t.y1 = m.h; t.x0 = 0; t.x1 = m.w;
    return t;
  }
  const size_t hw = (size_t)m.h * m.w;
  for (int e = threadIdx.x; e < fh * fw; e += 256) {
    const int cy = e / fw, cx = e - cy * fw;
    const size_t at = (size_t)(t.y0 + cy) * m.w + (t.x0 + cx);
    lds.g[e] = GuideCell{G[at], G[hw + at], G[2 * hw + at], 0.f};
    for (int c = 0; c < C; ++c) lds.s[c][e] = S[c * hw + at];
  }
  __syncthreads();
  return t;
}

// steps 1-5 of the definition for output pixel (oy, ox) -> v[C]
template <int R, int C, bool STAGED>
__device__ __forceinline__ void guided_pixel(const GuidedLds<C>& lds, const Maps& m, const float* S, const float* G, const Tile& t,
                                             const GArg& a, const uint8_t* guide, int oy, int ox, float (&v)[C]) {
  const uint8_t* gp = guide + (size_t)oy * a.gstride + (size_t)ox * a.gC;
  float gh[3];
  gh[0] = (float)gp[0] / 255.0f;
  gh[1] = a.gC == 3 ? (float)gp[1] / 255.0f : gh[0];
  gh[2] = a.gC == 3 ? (float)gp[2] / 255.0f : gh[0];
  const float sy = src_coord(a.sy, oy), sx = src_coord(a.sx, ox);
  const int by = (int)floorf(sy), bx = (int)floorf(sx);
  const int fw = t.x1 - t.x0;
  const size_t hw = (size_t)m.h * m.w;

  // A tap outside the map is skipped by an infinite squared distance: its exponent is +inf and its weight exp(-inf) = 0 adds
  // nothing to either sum (so does a tap whose exponent overflows).  Its loads go to the nearest cell inside, so every address
  // is in range without a branch; for the taps inside nothing changes.
  int row[2 * R], col[2 * R];
  float dy2[2 * R], dx2[2 * R];
#pragma unroll
  for (int k = 0; k < 2 * R; ++k) {
    const int qy = by - R + 1 + k, qx = bx - R + 1 + k;
    const float dy = (float)qy - sy, dx = (float)qx - sx;
    dy2[k] = qy >= t.y0 && qy < t.y1 ? dy * dy : INFINITY;
    dx2[k] = qx >= t.x0 && qx < t.x1 ? dx * dx : INFINITY;
    row[k] = STAGED ? (min(max(qy, t.y0), t.y1 - 1) - t.y0) * fw : min(max(qy, t.y0), t.y1 - 1) * m.w;  // h * w <= 2^24
    col[k] = STAGED ? min(max(qx, t.x0), t.x1 - 1) - t.x0 : min(max(qx, t.x0), t.x1 - 1);
  }

  float e[4 * R * R];
  float emin = INFINITY;
#pragma unroll
  for (int j = 0; j < 2 * R; ++j) {
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) {
      const int at = row[j] + col[i];
      float g0, g1, g2;
      if (STAGED) {
        const GuideCell g = lds.g[at];
        g0 = g.g0; g1 = g.g1; g2 = g.g2;
      } else {
        g0 = G[at]; g1 = G[hw + at]; g2 = G[2 * hw + at];
      }
      const float d2 = dy2[j] + dx2[i];
      const float c0 = gh[0] - g0, c1 = gh[1] - g1, c2 = gh[2] - g2;
      float rr = c0 * c0;
      rr += c1 * c1;
      rr += c2 * c2;
      float ee = m.ks * d2;
      ee += m.kr * rr;
      emin = fminf(emin, ee);
      e[j * 2 * R + i] = ee;
    }
  }

  float den = 0.f, acc[C];
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
  for (int j = 0; j < 2 * R; ++j) {
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) {
      const int at = row[j] + col[i];
      const float wgt = expf(-(e[j * 2 * R + i] - emin));
      den += wgt;
      for (int c = 0; c < C; ++c) acc[c] += wgt * (STAGED ? lds.s[c][at] : S[c * hw + at]);
    }
  }
  for (int c = 0; c < C; ++c) v[c] = acc[c] / den;
}

template <int R, int C>
__device__ __forceinline__ void tile_pixel(const GuidedLds<C>& lds, const Maps& m, const float* S, const float* G, const Tile& t,
                                           const GArg& a, const uint8_t* guide, int oy, int ox, float (&v)[C]) {
  if (t.staged) guided_pixel<R, C, true>(lds, m, S, G, t, a, guide, oy, ox, v);
  else guided_pixel<R, C, false>(lds, m, S, G, t, a, guide, oy, ox, v);
}

// block -> (image slot, tile of that image)
__device__ __forceinline__ int find_image(const GArgs& args, int n_img, int blk) {
  int i = 0;
  for (int k = 1; k < CHUNK; ++k)
    if (k < n_img && blk >= args.d[k].tile0) i = k;
  return i;
}

__device__ __forceinline__ float depth_finish(float v) { return 1.f - fminf(fmaxf(v, 0.f), 1.f); }

template <int R, int MODE>
__global__ __launch_bounds__(256) void guided_kernel(Maps m, const uint8_t* __restrict__ pixels, GArgs args, int n_img, int renorm,
                                                     uint8_t* __restrict__ out, const uint32_t* __restrict__ lut,
                                                     const float* __restrict__ part) {
  constexpr int C = (MODE == M_NORMAL_U8 || MODE == M_NORMAL_F32) ? 3 : 1;
  __shared__ GuidedLds<C> lds;
  __shared__ uint32_t s_row[MODE == M_NORMAL_U8 ? GH * row_dw(GW) : 1];
  __shared__ uint32_t s_lut[MODE == M_DEPTH_RGBA ? 256 : 1];
  const int tid = threadIdx.x;
  const int i = find_image(args, n_img, blockIdx.x);
  const GArg a = args.d[i];
  const int H = a.H, W = a.W;
  const size_t hw = (size_t)m.h * m.w;
  const float* S = m.S + (size_t)i * C * hw;
  const float* G = m.G + (size_t)i * 3 * hw;
  const uint8_t* guide = pixels + a.guide_offset;
  uint8_t* o = out + a.out_offset;

  float lo = 0.f, hi = 0.f;
  if (MODE == M_DEPTH_RGBA) {
    s_lut[tid] = lut[tid];
    lo = INFINITY;
    hi = -INFINITY;
    for (int p = 0; p < MM_PARTS; ++p) {  // every thread folds the same 64 pairs: min / max do not depend on the order
      lo = fminf(lo, part[((size_t)i * MM_PARTS + p) * 2]);
      hi = fmaxf(hi, part[((size_t)i * MM_PARTS + p) * 2 + 1]);
    }
  }
  const Tile t = stage_tile<R, C>(lds, m, S, G, a, blockIdx.x - a.tile0);
  if (MODE == M_DEPTH_RGBA && !t.staged) __syncthreads();  // s_lut

  const int c = tid % GW, ox = t.c0 + c;
  for (int r = tid / GW; r < GH; r += 256 / GW) {
    const int oy = t.r0 + r;
    if (oy >= H || ox >= W) continue;
    float v[C];
    tile_pixel<R, C>(lds, m, S, G, t, a, guide, oy, ox, v);
    if (MODE == M_NORMAL_U8 || MODE == M_NORMAL_F32) {
      if (renorm) {  // F.normalize of the decoded normal, re-encoded: the steps of dptx_postprocess_resize_batch
        float n[C];
        for (int ch = 0; ch < C; ++ch) n[ch] = 2.f * v[ch] - 1.f;
        float ss = n[0] * n[0];
        for (int ch = 1; ch < C; ++ch) ss += n[ch] * n[ch];
        const float d = fmaxf(sqrtf(ss), 1e-12f);
        for (int ch = 0; ch < C; ++ch) v[ch] = (n[ch] / d + 1.f) / 2.f;
      }
      for (int ch = 0; ch < C; ++ch) v[ch] = fminf(fmaxf(v[ch], 0.f), 1.f);
      if (MODE == M_NORMAL_F32) {
        for (int ch = 0; ch < C; ++ch) *(float*)(o + ((size_t)ch * H + oy) * a.ostride + (size_t)ox * 4) = v[ch];
      } else {
        uint8_t* row = u8_row_slot<GW>(s_row, o, a.ostride, oy, t.c0, r, c);
        for (int ch = 0; ch < C; ++ch) row[ch] = (uint8_t)(v[ch] * 255.0f);  // ToPILImage: mul(255).byte() truncates
      }
    } else {
      const float d = depth_finish(v[0]);
      if (MODE == M_DEPTH_F32) {
        *(float*)(o + (size_t)oy * a.ostride + (size_t)ox * 4) = d;
      } else {
        const float n = hi > lo ? (d - lo) / (hi - lo) : 0.f;
        const float s = n * 256.0f;
        const int idx = s >= 255.f ? 255 : (s > 0.f ? (int)s : 0);  // NaN -> 0
        *(uint32_t*)(o + (size_t)oy * a.ostride + (size_t)ox * 4) = s_lut[idx];
      }
    }
  }

  if (MODE == M_NORMAL_U8) {
    __syncthreads();
    flush_u8_rows<GW, GH>(s_row, o, a.ostride, t.r0, t.c0, H, W);
  }
}

// grid (MM_PARTS, images): block p of an image walks its tiles p, p + 64, ... and leaves one (min, max) pair of the DEPTH_F32 values
template <int R>
__global__ __launch_bounds__(256) void guided_minmax_kernel(Maps m, const uint8_t* __restrict__ pixels, GArgs args,
                                                            float* __restrict__ part) {
  __shared__ GuidedLds<1> lds;
  __shared__ float s_lo[256], s_hi[256];
  const int tid = threadIdx.x;
  const int i = blockIdx.y;
  const GArg a = args.d[i];
  const size_t hw = (size_t)m.h * m.w;
  const float* S = m.S + (size_t)i * hw;
  const float* G = m.G + (size_t)i * 3 * hw;
  const uint8_t* guide = pixels + a.guide_offset;
  const int ntiles = tiles_of(a.H, a.W);
  float lo = INFINITY, hi = -INFINITY;
  for (int tile = blockIdx.x; tile < ntiles; tile += MM_PARTS) {
    const Tile t = stage_tile<R, 1>(lds, m, S, G, a, tile);
    const int ox = t.c0 + tid % GW;
    for (int r = tid / GW; r < GH; r += 256 / GW) {
      const int oy = t.r0 + r;
      if (oy >= a.H || ox >= a.W) continue;
      float v[1];
      tile_pixel<R, 1>(lds, m, S, G, t, a, guide, oy, ox, v);
      const float d = depth_finish(v[0]);
      lo = fminf(lo, d);
      hi = fmaxf(hi, d);
    }
    __syncthreads();  // the next tile is staged over this one
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

bool fill_arg(const dptx_image_desc& g, const dptx_image_desc& d, int base, int h, int w, GArg& a) {
  if (!desc_in_range(g) || g.H != d.H || g.W != d.W) return false;
  const int bpp = base == M_NORMAL_U8 ? 3 : 4;
  if (d.offset < 0 || d.H < 1 || d.W < 1 || d.H > 16384 || d.W > 16384) return false;
  if ((long long)d.row_stride_bytes < (long long)d.W * bpp) return false;
  if (base != M_NORMAL_U8 && ((d.offset & 3) || (d.row_stride_bytes & 3))) return false;  // dword stores
  a.out_offset = d.offset;
  a.guide_offset = g.offset;
  a.H = d.H; a.W = d.W; a.ostride = d.row_stride_bytes;
  a.gstride = g.row_stride_bytes; a.gC = g.C;
  a.tile0 = 0;
  a.sy = (float)h / (float)d.H;
  a.sx = (float)w / (float)d.W;
  return true;
}

template <int R>
void launch_chunk(int base, const Maps& m, const uint8_t* pixels, const GArgs& args, int n, int tiles, int renorm, uint8_t* out,
                  const uint32_t* lut, float* part, hipStream_t st) {
  switch (base) {
    case M_NORMAL_U8:
      hipLaunchKernelGGL((guided_kernel<R, M_NORMAL_U8>), dim3(tiles), dim3(256), 0, st, m, pixels, args, n, renorm, out, lut, part);
      break;
    case M_NORMAL_F32:
      hipLaunchKernelGGL((guided_kernel<R, M_NORMAL_F32>), dim3(tiles), dim3(256), 0, st, m, pixels, args, n, renorm, out, lut, part);
      break;
    case M_DEPTH_F32:
      hipLaunchKernelGGL((guided_kernel<R, M_DEPTH_F32>), dim3(tiles), dim3(256), 0, st, m, pixels, args, n, renorm, out, lut, part);
      break;
    default:
      // the chunks share the workspace: they are ordered on the stream
      hipLaunchKernelGGL((guided_minmax_kernel<R>), dim3(MM_PARTS, n), dim3(256), 0, st, m, pixels, args, part);
      hipLaunchKernelGGL((guided_kernel<R, M_DEPTH_RGBA>), dim3(tiles), dim3(256), 0, st, m, pixels, args, n, renorm, out, lut, part);
      break;
  }
}

}  // namespace

extern "C" {

int dptx_postprocess_guided_workspace_bytes(int32_t B, int32_t mode, int64_t* bytes) {
  const int base = mode & ~DPTX_RESIZE_RENORM;
  if (!bytes || B < 1 || B > 4096 || base < M_NORMAL_U8 || base > M_DEPTH_RGBA) return DPTX_E_INVALID;
  if ((mode & DPTX_RESIZE_RENORM) && base != M_NORMAL_U8 && base != M_NORMAL_F32) return DPTX_E_INVALID;
  *bytes = base == M_DEPTH_RGBA ? (int64_t)CHUNK * MM_PARTS * 2 * sizeof(float) : 0;
  return DPTX_OK;
}

int dptx_postprocess_guided_batch(const void* y_dev, const void* guide_lo_dev, int32_t B, int32_t C, int32_t h, int32_t w,
                                  const void* pixels_dev, const dptx_image_desc* guides, const dptx_image_desc* outs,
                                  const dptx_guided_params* params, int32_t mode, void* out_dev, const void* lut_dev,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t need = 0;
  if (!y_dev || !guide_lo_dev || !pixels_dev || !guides || !outs || !params || !out_dev ||
      dptx_postprocess_guided_workspace_bytes(B, mode, &need) != DPTX_OK || h < 1 || w < 1 || h > 4096 || w > 4096 ||
      ((uintptr_t)y_dev & 3) || ((uintptr_t)guide_lo_dev & 3))
    return DPTX_E_INVALID;
  const int base = mode & ~DPTX_RESIZE_RENORM, renorm = (mode & DPTX_RESIZE_RENORM) ? 1 : 0;
  const bool normal = base == M_NORMAL_U8 || base == M_NORMAL_F32;
  if (C != (normal ? 3 : 1)) return DPTX_E_INVALID;
  if (base != M_NORMAL_U8 && ((uintptr_t)out_dev & 3)) return DPTX_E_INVALID;
  if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3) || !lut_dev || ((uintptr_t)lut_dev & 3)))
    return DPTX_E_INVALID;
  const int R = params->radius;
  if (R < 1 || R > MAX_R || !(params->sigma_space > 0.f) || !(params->sigma_range > 0.f)) return DPTX_E_INVALID;
  Maps m;
  m.h = h; m.w = w;
  m.ks = (float)(1.0 / (2.0 * (double)params->sigma_space * (double)params->sigma_space));
  m.kr = (float)(1.0 / (2.0 * (double)params->sigma_range * (double)params->sigma_range));
  if (!(m.ks > 0.f) || !(m.kr > 0.f) || !std::isfinite(m.ks) || !std::isfinite(m.kr)) return DPTX_E_INVALID;  // a sigma fp32 cannot hold
  GArg probe;
  for (int i = 0; i < B; ++i)
    if (!fill_arg(guides[i], outs[i], base, h, w, probe)) return DPTX_E_INVALID;  // the whole batch is checked before the first launch
  const hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += CHUNK) {
    const int n = B - b0 < CHUNK ? B - b0 : CHUNK;
    GArgs args = {};
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
      fill_arg(guides[b0 + i], outs[b0 + i], base, h, w, args.d[i]);
      args.d[i].tile0 = tiles;
      tiles += tiles_of(args.d[i].H, args.d[i].W);
    }
    m.S = (const float*)y_dev + (size_t)b0 * C * h * w;
    m.G = (const float*)guide_lo_dev + (size_t)b0 * 3 * h * w;
    const uint8_t* pixels = (const uint8_t*)pixels_dev;
    uint8_t* out = (uint8_t*)out_dev;
    const uint32_t* lut = (const uint32_t*)lut_dev;
    float* part = (float*)workspace;
    if (R == 1) launch_chunk<1>(base, m, pixels, args, n, tiles, renorm, out, lut, part, st);
    else if (R == 2) launch_chunk<2>(base, m, pixels, args, n, tiles, renorm, out, lut, part, st);
    else launch_chunk<3>(base, m, pixels, args, n, tiles, renorm, out, lut, part, st);
  }
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
