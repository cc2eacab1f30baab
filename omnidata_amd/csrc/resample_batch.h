// resample_batch.h -- device code shared by the ragged-batch resamplers (prepost_batch.hip: shorter side -> S, centre crop;
// fullframe.hip: the whole image -> OH x OW, and the mirrored views of test-time augmentation): Pillow's coefficient arithmetic
// and the tile that forms the horizontal pass of the input rows it needs once, in LDS, then runs the vertical pass with lanes
// along the output columns.  Behind them, what the writers of ragged outputs share (fullframe.hip, tta.hip): ATen's bilinear
// source coordinates and the tile rows of 3-byte pixels that leave LDS as aligned dwords.
// Contraction must be off where this is compiled: a fused a*b+c would change `center`, `xmin` and the rounded fixed-point weights.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;  // Pillow: 22
constexpr int CHUNK = 32;                   // images per launch (descriptors by value: 32 * 64 B of kernel arguments)
constexpr int KMAX = 67;                    // taps per output at the scale limit: ceil(support < 33) * 2 + 1
constexpr int TC = 32;                      // output columns of a tile
constexpr int TR_MAX = 16;                  // output rows of a tile (16 or 8)
constexpr int ROWS_CAP = 304;               // input rows whose horizontal pass one tile holds
constexpr int STAGE_DW = 3072;              // dwords of raw input rows staged at a time

struct ImgArg {
  long long offset;
  int H, W, C, stride;
  int oh, ow, top, left;  // resized size and the origin of the output window in it
  int ksh, ksv, tr, pad;  // pad: unused by the square entry; the rectangular one keeps the image's first tile of the launch here
  int flip, pad2;         // the views entry: the output is mirrored (column x is stored at OW - 1 - x); 0 elsewhere
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

// workspace of one image slot (ints) for an OH x OW output: [bh 2*OW | kh OW*KMAX | bv 2*OH | kv OH*KMAX]; rows of kh / kv are
// ksh / ksv ints apart
__host__ __device__ inline size_t slot_ints(int OH, int OW) { return (size_t)(2 + KMAX) * ((size_t)OH + OW); }

// thread j of image i: one output column (j < OW) or one output row (j - OW) of the window
__device__ inline void coeff_slot(const ImgArg& a, int i, int j, int OH, int OW, int* __restrict__ ws) {
  int* base = ws + (size_t)i * slot_ints(OH, OW);
  if (j < OW)
    coeff_one(a.W, a.ow, a.left + j, a.ksh, base + 2 * j, base + 2 * OW + (size_t)j * a.ksh);
  else {
    const int r = j - OW;
    base += (size_t)(2 + KMAX) * OW;
    coeff_one(a.H, a.oh, a.top + r, a.ksv, base + 2 * r, base + 2 * OH + (size_t)r * a.ksv);
  }
}

__device__ __forceinline__ int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// LDS of one resize tile (one 256-thread block)
struct ResizeTileLds {
  int wh[KMAX * TC];         // [tap][column]: lanes run along the columns
  int wv[TR_MAX * KMAX];     // [row][tap]: one row per half wave, broadcast
  int bh[TC * 2], bv[TR_MAX * 2];
  uint32_t hp[ROWS_CAP * TC];  // horizontal pass: [input row][column], channels packed in the bytes
  uint32_t in[STAGE_DW];       // raw input rows, from the dword that holds the tile's first byte
};

// Output tile `tile` (TC columns x a.tr rows, row-major over the OH x OW window) of image slot i -> o [3][OH][OW] fp32.
// MIRROR: the entry honours a.flip.
template <bool MIRROR = false>
__device__ __forceinline__ void resize_tile(ResizeTileLds& s, const uint8_t* __restrict__ pixels, const ImgArg& a, int i, int tile,
                                            int OH, int OW, const int* __restrict__ ws, int depth_norm, float* __restrict__ o) {
  const int TR = a.tr;
  const int tiles_c = OW / TC;
  const int c0 = (tile % tiles_c) * TC, r0 = (tile / tiles_c) * TR;
  const int tid = threadIdx.x;
  const int C = a.C, ksh = a.ksh, ksv = a.ksv;

  const int* bh = ws + (size_t)i * slot_ints(OH, OW);
  const int* kh = bh + 2 * OW;
  const int* bv = bh + (size_t)(2 + KMAX) * OW;
  const int* kv = bv + 2 * OH;
  if (tid < 2 * TC) s.bh[tid] = bh[2 * c0 + tid];
  if (tid >= 64 && tid < 64 + 2 * TR) s.bv[tid - 64] = bv[2 * r0 + tid - 64];
  for (int e = tid; e < TC * ksh; e += 256) {  // kh rows of the 32 columns are contiguous: coalesced
    const int c = e / ksh, t = e - c * ksh;
    s.wh[t * TC + c] = kh[(size_t)c0 * ksh + e];
  }
  for (int e = tid; e < TR * ksv; e += 256) {
    const int r = e / ksv, t = e - r * ksv;
    s.wv[r * KMAX + t] = kv[(size_t)r0 * ksv + e];
  }
  __syncthreads();

  // bounds are non-decreasing along an axis: the tile's window is [first of the first, end of the last)
  const int row0 = s.bv[0];
  int nrows = s.bv[2 * (TR - 1)] + s.bv[2 * (TR - 1) + 1] - row0;
  if (nrows > ROWS_CAP) nrows = ROWS_CAP;  // never taken: the host sizes TR from the scale
  const int x0 = s.bh[0];
  const int segbytes = (s.bh[2 * (TC - 1)] + s.bh[2 * (TC - 1) + 1] - x0) * C;
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
      s.in[rr * pitch + d] = v;
    }
    __syncthreads();
    // ---- horizontal pass of those rows for the tile's 32 columns
    for (int e = tid; e < nr * TC; e += 256) {
      const int rr = e >> 5, c = e & 31;
      const uint8_t* rowp = img + (size_t)(row0 + rb + rr) * a.stride;
      const int sh = (int)((uintptr_t)(rowp + (size_t)x0 * C) & 3);
      const int xmin = s.bh[2 * c], nx = s.bh[2 * c + 1];
      const uint8_t* src = (const uint8_t*)(s.in + rr * pitch) + sh + (xmin - x0) * C;
      uint32_t packed;
      if (C == 3) {
        int h0 = 1 << (PRECISION_BITS - 1), h1 = h0, h2 = h0;
        for (int t = 0; t < nx; ++t) {
          const int w = s.wh[t * TC + c];
          h0 += (int)src[3 * t] * w;
          h1 += (int)src[3 * t + 1] * w;
          h2 += (int)src[3 * t + 2] * w;
        }
        packed = (uint32_t)clip8(h0) | ((uint32_t)clip8(h1) << 8) | ((uint32_t)clip8(h2) << 16);
      } else {
        int h0 = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < nx; ++t) h0 += (int)src[t] * s.wh[t * TC + c];
        packed = (uint32_t)clip8(h0);
      }
      s.hp[(rb + rr) * TC + c] = packed;
    }
    __syncthreads();
  }

  // ---- vertical pass over the LDS tile, ToTensor / Normalize, 1 -> 3 channel repeat
  const size_t plane = (size_t)OH * OW;
  for (int e = tid; e < TR * TC; e += 256) {
    const int r = e >> 5, c = e & 31;
    const int ymin = s.bv[2 * r] - row0;
    int ny = s.bv[2 * r + 1];
    if (ymin + ny > nrows) ny = nrows - ymin;  // never taken (see nrows)
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < ny; ++t) {
      const uint32_t v = s.hp[(ymin + t) * TC + c];
      const int w = s.wv[r * KMAX + t];
      a0 += (int)(v & 255) * w;
      a1 += (int)((v >> 8) & 255) * w;
      a2 += (int)((v >> 16) & 255) * w;
    }
    const int v8[3] = {clip8(a0), C == 3 ? clip8(a1) : clip8(a0), C == 3 ? clip8(a2) : clip8(a0)};
    const int oc = MIRROR && a.flip ? OW - 1 - (c0 + c) : c0 + c;
    const size_t at = (size_t)(r0 + r) * OW + oc;
    for (int ch = 0; ch < 3; ++ch) {
      float f = (float)v8[ch] / 255.0f;       // ToTensor
      if (depth_norm) f = (f - 0.5f) / 0.5f;  // Normalize(mean=0.5, std=0.5)
      o[ch * plane + at] = f;
    }
  }
}

// what both entries check of a descriptor, and the tile geometry for an oh x ow resize of it (a.oh, a.ow set by the caller)
inline bool fill_tile_geometry(const dptx_image_desc& d, ImgArg& a) {
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
  a.flip = a.pad2 = 0;
  return true;
}

inline bool desc_in_range(const dptx_image_desc& d) {
  if (d.offset < 0 || (d.C != 1 && d.C != 3) || d.H < 1 || d.W < 1 || d.H > 16384 || d.W > 16384) return false;
  return (long long)d.row_stride_bytes >= (long long)d.W * d.C;
}

// ------------------------------------------------------------------------------------------------ ragged outputs
// ATen area_pixel_compute_scale / area_pixel_compute_source_index (align_corners=False) + guard_index_and_lambda
__device__ __forceinline__ float src_coord(float scale, int dst) { return scale * ((float)dst + 0.5f) - 0.5f; }
__device__ __forceinline__ void guard(float real, int in, int& idx, float& lam) {
  idx = min((int)floorf(real), in - 1);
  lam = fminf(fmaxf(real - (float)idx, 0.f), 1.f);
}
struct Lin {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lin lin_axis(int in, int out, float scale, int dst) {
  Lin a;
  if (in == out) {  // ATen copies
    a.i0 = a.i1 = dst; a.l0 = 1.f; a.l1 = 0.f;
    return a;
  }
  float real = src_coord(scale, dst);
  if (real < 0.f) real = 0.f;
  guard(real, in, a.i0, a.l1);
  a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
  a.l0 = 1.f - a.l1;
  return a;
}

// A tile of RH rows x RW columns of 3-byte pixels at (r0, c0) of an [H][W][3] uint8 output whose rows start at any byte:
// s_row holds row r at dword r * row_dw(RW), its bytes at the misalignment of the row's first byte in memory (u8_row_slot).
// The rows go out as aligned dwords, with byte stores for the (at most 3 + 3) bytes at the two ends of a tile row: no byte
// outside [row start, row start + 3 * W) is written.  All 256 threads of the block call it, after a __syncthreads().
__host__ __device__ constexpr int row_dw(int RW) { return 3 * RW / 4 + 4; }  // 3 * RW bytes + 3 of misalignment, padded
template <int RW>
__device__ __forceinline__ uint8_t* u8_row_slot(uint32_t* s_row, const uint8_t* o, int stride, int oy, int c0, int r, int c) {
  const int sh = (int)((uintptr_t)(o + (size_t)oy * stride + (size_t)c0 * 3) & 3);
  return (uint8_t*)(s_row + r * row_dw(RW)) + sh + 3 * c;
}
template <int RW, int RH>
__device__ __forceinline__ void flush_u8_rows(const uint32_t* s_row, uint8_t* o, int stride, int r0, int c0, int H, int W) {
  constexpr int ROW_DW = row_dw(RW);
  const int nbytes = 3 * min(RW, W - c0);
  for (int e = threadIdx.x; e < RH * ROW_DW; e += 256) {  // blocks of 256 threads
    const int r = e / ROW_DW, d = e - r * ROW_DW;
    if (r0 + r >= H) break;
    const uintptr_t p0 = (uintptr_t)(o + (size_t)(r0 + r) * stride + (size_t)c0 * 3), p1 = p0 + nbytes;
    const uintptr_t q = (p0 & ~(uintptr_t)3) + 4 * (uintptr_t)d;
    if (q >= p1) continue;
    const uint32_t v = s_row[r * ROW_DW + d];
    if (q >= p0 && q + 4 <= p1) {
      *(uint32_t*)q = v;
    } else {
      for (int b = 0; b < 4; ++b)
        if (q + b >= p0 && q + b < p1) *(uint8_t*)(q + b) = (uint8_t)(v >> (8 * b));
    }
  }
}

}  // namespace
