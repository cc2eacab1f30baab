// augment.hip -- the training augmentations (include/dptx.h, "Training augmentations"): the blur chain sharpness -> motion blur ->
// Gaussian blur on x [B][C][H][W] fp32 in ONE launch, and the crop / resize of all task tensors of a batch in ONE launch.
// Stream-ordered, no workspace, no allocation, no host synchronisation, no atomics; descriptors by value.
//
//  Chain.  Block = a TW x TH output tile of one (sample, channel) plane.  The block stages its tile plus the halo the active
//  stages need (1 + km/2 + kg/2 <= 7 pixels a side) in LDS, zero outside the image, and every stage but the last leaves its result
//  in an LDS buffer of its own, on the region the stages behind it still need: a pixel is read from memory once (apart from
//  halos) and written once.  All buffers share one coordinate system, (ly, lx) <-> image (r0 - HALO + ly, c0 - HALO + lx).
//  The Gaussian stage reflects at the IMAGE border: its taps index intermediate pixels inside the image, within kg/2 of the edge,
//  and those lie in the region a border tile holds (|reflected - tile| <= kg/2).
//  A thread computes strips of V vertically adjacent outputs: a window row is read from LDS once and feeds up to V accumulators
//  ((V + k - 1) k reads for V k^2 taps), lanes run along x, so the reads of a wave are consecutive dwords.  The stages are
//  specialised at compile time (which are active: 7 kernels) and the tap loops on the filter sizes (fully unrolled, weights in
//  registers); the size is uniform over a launch.
//  Gather.  Block = 64 x 16 outputs of one plane of one task; no LDS.
// Contraction is off (resample_batch.h): the fused operations are the fmaf calls the definition names, nothing else.
#include "resample_batch.h"

namespace {

constexpr int TW = 64, TH = 32;        // output tile
constexpr int V = 4;                   // outputs per strip
constexpr int HALO = 7;                // 1 + 3 + 3
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
static_assert(TH % V == 0 && TH >= V, "strips tile the output rows");

struct ChainArgs {
  const float* x;
  float* out;
  const float* sharp;   // [B]
  const float* motion;  // [B][km][km]
  const float* gy;      // [B][kgy]
  const float* gx;      // [B][kgx]
  int C, H, W, km, kgy, kgx, tiles_x, tiles_y;
};

struct TileCtx {
  int r0, c0, H, W;   // the tile's origin and the image size
  size_t plane;       // element offset of the (sample, channel) plane
};

// acc[o] = fma chain over the KY x KX window whose row i lies at LDS offset row[i] and whose column q at col[q], for the V outputs
// o whose windows start at rows o
template <int KY, int KX>
__device__ __forceinline__ void conv_strip(const float* src, const int (&row)[V + KY - 1], const int (&col)[KX],
                                           const float (&w)[KY * KX], float (&acc)[V]) {
#pragma unroll
  for (int o = 0; o < V; ++o) acc[o] = 0.f;
#pragma unroll
  for (int i = 0; i < V + KY - 1; ++i) {
#pragma unroll
    for (int q = 0; q < KX; ++q) {
      const float v = src[row[i] + col[q]];
#pragma unroll
      for (int o = 0; o < V; ++o) {
        const int r = i - o;
        if (r >= 0 && r < KY) acc[o] = fmaf(w[r * KX + q], v, acc[o]);
      }
    }
  }
}

// the strips of the region rows [ya, yb) x columns [xa, xb) (buffer coordinates): strip e -> its column and first row; the last
// strip of a column is moved up to end at yb (it repeats rows of the one before it: the same values)
struct Strips {
  int xa, ya, nx, nrows, count;
  __device__ __forceinline__ Strips(int ya_, int yb, int xa_, int xb) : xa(xa_), ya(ya_), nx(xb - xa_), nrows(yb - ya_) {
    count = nx * ((nrows + V - 1) / V);
  }
  __device__ __forceinline__ void at(int e, int& ly, int& lx) const {
    const int s = e / nx;
    lx = xa + e - s * nx;
    ly = ya + min(s * V, nrows - V);
  }
};

// where a stage leaves its V results: the next stage's LDS buffer (0 outside the image when the next stage pads with zeros), or,
// for the last stage, the output
template <bool LAST>
__device__ __forceinline__ void put(const TileCtx& t, float* dst, float* __restrict__ out, int ly, int lx, const float (&v)[V]) {
  const int x = t.c0 - HALO + lx;
#pragma unroll
  for (int o = 0; o < V; ++o) {
    const int y = t.r0 - HALO + ly + o;
    const bool inside = y >= 0 && y < t.H && x >= 0 && x < t.W;
    if (LAST) {
      if (inside) out[t.plane + (size_t)y * t.W + x] = v[o];
    } else {
      dst[(ly + o) * LW + lx] = inside ? v[o] : 0.f;
    }
  }
}

template <bool LAST>
__device__ __forceinline__ void sharp_stage(const TileCtx& t, const float* src, float* dst, float* __restrict__ out, float f, int hy,
                                            int hx) {
  const float a = (float)(1.0 / 13.0), b = (float)(5.0 / 13.0);
  const float w[9] = {a, a, a, a, b, a, a, a, a};
  const bool has_interior = t.H >= 3 && t.W >= 3;
  const Strips st(HALO - hy, HALO + TH + hy, HALO - hx, HALO + TW + hx);
  for (int e = threadIdx.x; e < st.count; e += 256) {
    int ly, lx;
    st.at(e, ly, lx);
    int row[V + 2], col[3];
#pragma unroll
    for (int i = 0; i < V + 2; ++i) row[i] = (ly - 1 + i) * LW;
#pragma unroll
    for (int q = 0; q < 3; ++q) col[q] = lx - 1 + q;
    float d[V], v[V];
    conv_strip<3, 3>(src, row, col, w, d);
    const int x = t.c0 - HALO + lx;
#pragma unroll
    for (int o = 0; o < V; ++o) {
      const int y = t.r0 - HALO + ly + o;
      const float xc = src[(ly + o) * LW + lx];
      const bool interior = has_interior && y >= 1 && y <= t.H - 2 && x >= 1 && x <= t.W - 2;
      const float dd = interior ? d[o] : xc;
      float s = xc - dd;
      s = s * f;
      s = dd + s;
      v[o] = f == 1.f ? xc : s;
    }
    put<LAST>(t, dst, out, ly, lx, v);
  }
}

// a value that is the same in every lane, moved to a scalar register: the 49 weights of a 7 x 7 table would otherwise take 49
// VGPRs of every thread
__device__ __forceinline__ float uniform(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
#else
  return v;
#endif
}

template <bool LAST, int K>
__device__ __forceinline__ void motion_stage_k(const TileCtx& t, const float* src, float* dst, float* __restrict__ out,
                                               const float* __restrict__ taps, int hy, int hx) {
  float w[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) w[i] = uniform(taps[i]);
  const Strips st(HALO - hy, HALO + TH + hy, HALO - hx, HALO + TW + hx);
  for (int e = threadIdx.x; e < st.count; e += 256) {
    int ly, lx;
    st.at(e, ly, lx);
    int row[V + K - 1], col[K];
#pragma unroll
    for (int i = 0; i < V + K - 1; ++i) row[i] = (ly - K / 2 + i) * LW;
#pragma unroll
    for (int q = 0; q < K; ++q) col[q] = lx - K / 2 + q;
    float v[V];
    conv_strip<K, K>(src, row, col, w, v);
    put<LAST>(t, dst, out, ly, lx, v);
  }
}

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// always the last stage: the taps are reflected at the image border and then held inside the rows / columns the tile has of the
// previous stage (a no-op for every output inside the image: see the head of the file)
template <int KY, int KX>
__device__ __forceinline__ void gauss_stage_k(const TileCtx& t, const float* src, float* __restrict__ out, const float* __restrict__ gy,
                                              const float* __restrict__ gx) {
  float w[KY * KX];
#pragma unroll
  for (int i = 0; i < KY; ++i)
#pragma unroll
    for (int j = 0; j < KX; ++j) w[i * KX + j] = uniform(gy[i] * gx[j]);
  const int ylo = max(t.r0 - KY / 2, 0), yhi = min(t.r0 + TH + KY / 2, t.H) - 1;
  const int xlo = max(t.c0 - KX / 2, 0), xhi = min(t.c0 + TW + KX / 2, t.W) - 1;
  const Strips st(HALO, HALO + TH, HALO, HALO + TW);
  for (int e = threadIdx.x; e < st.count; e += 256) {
    int ly, lx;
    st.at(e, ly, lx);
    const int y = t.r0 - HALO + ly, x = t.c0 - HALO + lx;
    int row[V + KY - 1], col[KX];
#pragma unroll
    for (int i = 0; i < V + KY - 1; ++i) row[i] = (min(max(reflect(y - KY / 2 + i, t.H), ylo), yhi) - t.r0 + HALO) * LW;
#pragma unroll
    for (int q = 0; q < KX; ++q) col[q] = min(max(reflect(x - KX / 2 + q, t.W), xlo), xhi) - t.c0 + HALO;
    float v[V];
    conv_strip<KY, KX>(src, row, col, w, v);
    put<true>(t, nullptr, out, ly, lx, v);
  }
}

template <int KY>
__device__ __forceinline__ void gauss_stage_y(const TileCtx& t, const float* src, float* __restrict__ out, const float* __restrict__ gy,
                                              const float* __restrict__ gx, int kgx) {
  switch (kgx) {
    case 1: gauss_stage_k<KY, 1>(t, src, out, gy, gx); break;
    case 3: gauss_stage_k<KY, 3>(t, src, out, gy, gx); break;
    case 5: gauss_stage_k<KY, 5>(t, src, out, gy, gx); break;
    default: gauss_stage_k<KY, 7>(t, src, out, gy, gx); break;
  }
}

// four waves per SIMD asked for: left alone, the scheduler hoists the 70 window loads of a 7 x 7 strip and ends a few VGPRs above 128
template <bool SHARP, bool MOTION, bool GAUSS>
#if defined(__HIP__)
#define FOUR_WAVES __attribute__((amdgpu_waves_per_eu(4)))
#else
#define FOUR_WAVES  // the host build of the tests
#endif
__global__ __launch_bounds__(256) FOUR_WAVES void augment_chain_kernel(ChainArgs a) {
  constexpr int NBUF = 1 + (SHARP && (MOTION || GAUSS) ? 1 : 0) + (MOTION && GAUSS ? 1 : 0);
  __shared__ float lds[NBUF][LH * LW];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % a.tiles_x;
  blk /= a.tiles_x;
  const int ty = blk % a.tiles_y;
  const int pl = blk / a.tiles_y;  // sample * C + channel
  const int b = pl / a.C;
  TileCtx t;
  t.r0 = ty * TH; t.c0 = tx * TW; t.H = a.H; t.W = a.W;
  t.plane = (size_t)pl * a.H * a.W;

  const int rs = SHARP ? 1 : 0, rm = MOTION ? a.km / 2 : 0;
  const int rgy = GAUSS ? a.kgy / 2 : 0, rgx = GAUSS ? a.kgx / 2 : 0;

  {  // the tile of x and the halo of all active stages, 0 outside the image
    const int hy = rs + rm + rgy, hx = rs + rm + rgx;
    const int nx = TW + 2 * hx, n = nx * (TH + 2 * hy);
    const float* __restrict__ xp = a.x + t.plane;
    for (int e = tid; e < n; e += 256) {
      const int r = e / nx;
      const int ly = HALO - hy + r, lx = HALO - hx + e - r * nx;
      const int y = t.r0 - HALO + ly, x = t.c0 - HALO + lx;
      lds[0][ly * LW + lx] = y >= 0 && y < t.H && x >= 0 && x < t.W ? xp[(size_t)y * t.W + x] : 0.f;
    }
  }
  __syncthreads();

  int cur = 0;
  if (SHARP) {
    constexpr bool LAST = !MOTION && !GAUSS;
    sharp_stage<LAST>(t, lds[cur], lds[LAST ? cur : cur + 1], a.out, a.sharp[b], rm + rgy, rm + rgx);
    if (!LAST) {
      ++cur;
      __syncthreads();
    }
  }
  if (MOTION) {
    constexpr bool LAST = !GAUSS;
    const float* taps = a.motion + (size_t)b * a.km * a.km;
    float* dst = lds[LAST ? cur : cur + 1];
    switch (a.km) {
      case 3: motion_stage_k<LAST, 3>(t, lds[cur], dst, a.out, taps, rgy, rgx); break;
      case 5: motion_stage_k<LAST, 5>(t, lds[cur], dst, a.out, taps, rgy, rgx); break;
      default: motion_stage_k<LAST, 7>(t, lds[cur], dst, a.out, taps, rgy, rgx); break;
    }
    if (!LAST) {
      ++cur;
      __syncthreads();
    }
  }
  if (GAUSS) {
    const float* gy = a.gy + (size_t)b * a.kgy;
    const float* gx = a.gx + (size_t)b * a.kgx;
    switch (a.kgy) {
      case 1: gauss_stage_y<1>(t, lds[cur], a.out, gy, gx, a.kgx); break;
      case 3: gauss_stage_y<3>(t, lds[cur], a.out, gy, gx, a.kgx); break;
      case 5: gauss_stage_y<5>(t, lds[cur], a.out, gy, gx, a.kgx); break;
      default: gauss_stage_y<7>(t, lds[cur], a.out, gy, gx, a.kgx); break;
    }
  }
}

// ------------------------------------------------------------------------------------------------ crop / resize of the tasks
constexpr int RW = 64, RH = 16;  // output tile of the gather: a thread keeps its column over RH * RW / 256 rows

struct GatherTask {
  const void* src;
  void* dst;
  int C, dtype, interp, block0;  // block0: the task's first block of the launch
};
struct GatherArgs {
  GatherTask t[DPTX_AUG_MAX_TASKS];
  int n_tasks, Hs, Ws, op, y0, x0, h, w, tiles_x, tiles_y;
  float sh, sw;  // (float)in / (float)out, divided once on the host
};

__device__ __forceinline__ float blend(const float* __restrict__ p, int w, const Lin& y, const Lin& x) {
  const float* r0 = p + (size_t)y.i0 * w;
  const float* r1 = p + (size_t)y.i1 * w;
  float t0 = x.l0 * r0[x.i0];
  t0 += x.l1 * r0[x.i1];
  float t1 = x.l0 * r1[x.i0];
  t1 += x.l1 * r1[x.i1];
  float v = y.l0 * t0;
  v += y.l1 * t1;
  return v;
}

__global__ __launch_bounds__(256) void augment_gather_kernel(GatherArgs a) {
  int k = 0;
  for (int i = 1; i < DPTX_AUG_MAX_TASKS; ++i)
    if (i < a.n_tasks && (int)blockIdx.x >= a.t[i].block0) k = i;
  const GatherTask g = a.t[k];
  int blk = blockIdx.x - g.block0;
  const int tx = blk % a.tiles_x;
  blk /= a.tiles_x;
  const int ty = blk % a.tiles_y;
  const int pl = blk / a.tiles_y;  // sample * C + channel
  const int c = threadIdx.x % RW, ox = tx * RW + c;
  if (ox >= a.w) return;
  const size_t sp = (size_t)pl * a.Hs * a.Ws, dp = (size_t)pl * a.h * a.w;
  const bool bilinear = a.op == DPTX_AUG_RESIZE && g.interp == DPTX_AUG_BILINEAR;
  Lin lx = {};
  int sx;
  if (a.op == DPTX_AUG_CROP) sx = a.x0 + ox;
  else sx = min((int)floorf((float)ox * a.sw), a.Ws - 1);
  if (bilinear) lx = lin_axis(a.Ws, a.w, a.sw, ox);
  for (int r = threadIdx.x / RW; r < RH; r += 256 / RW) {
    const int oy = ty * RH + r;
    if (oy >= a.h) break;
    const size_t at = dp + (size_t)oy * a.w + ox;
    if (bilinear) {
      ((float*)g.dst)[at] = blend((const float*)g.src + sp, a.Ws, lin_axis(a.Hs, a.h, a.sh, oy), lx);
      continue;
    }
    const int sy = a.op == DPTX_AUG_CROP ? a.y0 + oy : min((int)floorf((float)oy * a.sh), a.Hs - 1);
    const size_t from = sp + (size_t)sy * a.Ws + sx;
    if (g.dtype == DPTX_AUG_F32) ((uint32_t*)g.dst)[at] = ((const uint32_t*)g.src)[from];
    else ((uint8_t*)g.dst)[at] = ((const uint8_t*)g.src)[from];
  }
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

template <bool S, bool M, bool G>
void launch_chain(const ChainArgs& a, int blocks, hipStream_t st) {
  hipLaunchKernelGGL((augment_chain_kernel<S, M, G>), dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int dptx_augment_filter_chain(const void* x_dev, int32_t B, int32_t C, int32_t H, int32_t W, const float* sharp_factor_dev,
                              const float* motion_taps_dev, int32_t km, const float* gauss_y_dev, const float* gauss_x_dev,
                              int32_t kgy, int32_t kgx, void* out_dev, void* stream) {
  if (!x_dev || !out_dev || ((uintptr_t)x_dev & 3) || ((uintptr_t)out_dev & 3) || B < 1 || C < 1 || H < 1 || W < 1 || H > 16384 ||
      W > 16384)
    return DPTX_E_INVALID;
  const bool S = sharp_factor_dev != nullptr, M = motion_taps_dev != nullptr, G = gauss_y_dev != nullptr;
  if ((gauss_x_dev != nullptr) != G || !(S || M || G)) return DPTX_E_INVALID;
  if (M && km != 3 && km != 5 && km != 7) return DPTX_E_INVALID;
  if (G && ((kgy != 1 && kgy != 3 && kgy != 5 && kgy != 7) || (kgx != 1 && kgx != 3 && kgx != 5 && kgx != 7) || H <= kgy / 2 ||
            W <= kgx / 2))
    return DPTX_E_INVALID;
  if (((uintptr_t)sharp_factor_dev | (uintptr_t)motion_taps_dev | (uintptr_t)gauss_y_dev | (uintptr_t)gauss_x_dev) & 3)
    return DPTX_E_INVALID;
  const size_t bytes = (size_t)B * C * H * W * sizeof(float);
  if (overlap(x_dev, bytes, out_dev, bytes)) return DPTX_E_INVALID;
  ChainArgs a;
  a.x = (const float*)x_dev; a.out = (float*)out_dev;
  a.sharp = sharp_factor_dev; a.motion = motion_taps_dev; a.gy = gauss_y_dev; a.gx = gauss_x_dev;
  a.C = C; a.H = H; a.W = W; a.km = M ? km : 0; a.kgy = G ? kgy : 0; a.kgx = G ? kgx : 0;
  a.tiles_x = (W + TW - 1) / TW;
  a.tiles_y = (H + TH - 1) / TH;
  const long long blocks = (long long)B * C * a.tiles_x * a.tiles_y;
  if (blocks > 0x7FFFFFFFLL) return DPTX_E_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  const int n = (int)blocks;
  switch ((S ? 4 : 0) | (M ? 2 : 0) | (G ? 1 : 0)) {
    case 1: launch_chain<false, false, true>(a, n, st); break;
    case 2: launch_chain<false, true, false>(a, n, st); break;
    case 3: launch_chain<false, true, true>(a, n, st); break;
    case 4: launch_chain<true, false, false>(a, n, st); break;
    case 5: launch_chain<true, false, true>(a, n, st); break;
    case 6: launch_chain<true, true, false>(a, n, st); break;
    default: launch_chain<true, true, true>(a, n, st); break;
  }
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

int dptx_augment_resize_tasks(const dptx_augment_task* tasks, int32_t n_tasks, int32_t B, int32_t Hs, int32_t Ws, int32_t op,
                              int32_t y0, int32_t x0, int32_t h, int32_t w, void* stream) {
  if (!tasks || n_tasks < 1 || n_tasks > DPTX_AUG_MAX_TASKS || B < 1 || Hs < 1 || Ws < 1 || h < 1 || w < 1 || Hs > 16384 ||
      Ws > 16384 || h > 16384 || w > 16384 || (op != DPTX_AUG_CROP && op != DPTX_AUG_RESIZE))
    return DPTX_E_INVALID;
  if (op == DPTX_AUG_CROP && (y0 < 0 || x0 < 0 || (long long)y0 + h > Hs || (long long)x0 + w > Ws)) return DPTX_E_INVALID;
  GatherArgs a = {};
  a.n_tasks = n_tasks; a.Hs = Hs; a.Ws = Ws; a.op = op; a.y0 = y0; a.x0 = x0; a.h = h; a.w = w;
  a.tiles_x = (w + RW - 1) / RW;
  a.tiles_y = (h + RH - 1) / RH;
  a.sh = (float)Hs / (float)h;
  a.sw = (float)Ws / (float)w;
  long long blocks = 0;
  for (int i = 0; i < n_tasks; ++i) {
    const dptx_augment_task& t = tasks[i];
    if (!t.src || !t.dst || t.C < 1 || (t.dtype != DPTX_AUG_F32 && t.dtype != DPTX_AUG_U8)) return DPTX_E_INVALID;
    if (op == DPTX_AUG_RESIZE && t.interp != DPTX_AUG_NEAREST && !(t.interp == DPTX_AUG_BILINEAR && t.dtype == DPTX_AUG_F32))
      return DPTX_E_INVALID;
    const size_t el = t.dtype == DPTX_AUG_F32 ? 4 : 1;
    if (el == 4 && (((uintptr_t)t.src | (uintptr_t)t.dst) & 3)) return DPTX_E_INVALID;
    if (overlap(t.src, (size_t)B * t.C * Hs * Ws * el, t.dst, (size_t)B * t.C * h * w * el)) return DPTX_E_INVALID;
    a.t[i].src = t.src; a.t[i].dst = t.dst; a.t[i].C = t.C; a.t[i].dtype = t.dtype; a.t[i].interp = t.interp;
    a.t[i].block0 = (int)blocks;
    blocks += (long long)B * t.C * a.tiles_x * a.tiles_y;
    if (blocks > 0x7FFFFFFFLL) return DPTX_E_INVALID;
  }
  hipLaunchKernelGGL(augment_gather_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
