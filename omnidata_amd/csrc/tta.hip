// tta.hip -- the merge of test-time augmentation for surface normals (include/dptx.h, "Test-time augmentation"): the views of an
// image -- the network's maps for windows of it, possibly mirrored, each at its own size -- -> the image's map at its own size,
// per channel the median (np.median) or the mean of the views that cover a pixel, normalised again.  Stream-ordered, no
// workspace, no allocation, no host synchronisation; one launch per image with its (at most 64) views by value in the arguments.
//
// Block = 64 columns x 4 rows of one image, a thread owns one pixel and a wave one tile row, so whether a view covers the pixel
// is uniform over a wave except where a window's edge crosses it.  Per view the thread forms the y / x taps once, reads the
// 4 x 3 values through cache (a view is <= 1.8 MB typically and every tile of its window reads it), decodes and normalises the
// four corners, blends in ATen's order (resample_batch.h) and hands the three values to the selection.
//
// Selection: the median of n <= K values needs the elements (n - 1) / 2 and n / 2 of the sorted sequence, both among the
// K / 2 + 1 smallest.  Each channel keeps those in M = K / 2 + 1 registers, ascending, +inf where nothing is yet; a new value
// runs down the list through M (min, max) pairs with constant indices -- fully unrolled, no indexed register array, no scratch.
// The loop over the views is NOT unrolled: code size is one insertion, whatever K is.  The kernel is templated on the class
// K in {8, 16, 32, 64} (M = 5, 9, 17, 33: 15 .. 99 VGPRs of state); the host takes the smallest class that holds the image's
// views.  min / max move values and never round them, so the class does not change a bit of the result.  M = 0 is the mean.
// The alternative, per-thread columns in LDS, needs 3 x 64 KB per 256 threads for K = 64 (one channel at a time would form the
// taps three times) and ~K^2 / 4 LDS round trips per channel; see DESIGN.md.
// Contraction is off (resample_batch.h): two runs, and the same image in another batch, compute the same bits.
#include "tta_common.h"

namespace {

constexpr int M_U8 = DPTX_RESIZE_NORMAL_U8, M_F32 = DPTX_RESIZE_NORMAL_F32;

template <int M, int MODE>
__global__ __launch_bounds__(256) void tta_merge_kernel(const float* __restrict__ views, ViewArgs args, int nv, MergeOut o, int raw,
                                                        uint8_t* __restrict__ out) {
  __shared__ uint32_t s_row[MODE == M_U8 ? TH * row_dw(TW) : 1];
  const int tid = threadIdx.x;
  const int tiles_x = (o.W + TW - 1) / TW;
  const int c0 = (blockIdx.x % tiles_x) * TW, r0 = (blockIdx.x / tiles_x) * TH;
  const int c = tid % TW, r = tid / TW;
  const int X = c0 + c, Y = r0 + r;
  const bool inside = X < o.W && Y < o.H;
  uint8_t* dst = out + o.offset;

  Lowest<M> sel[3];
  float sum[3] = {0.f, 0.f, 0.f};
  int n = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) sel[ch].clear();

  for (int k = 0; k < nv; ++k) {
    const ViewArg a = args.v[k];
    const int ly = Y - a.y0;
    int lx = X - a.x0;
    if (!inside || ly < 0 || ly >= a.ch || lx < 0 || lx >= a.cw) continue;
    if (a.flip) lx = a.cw - 1 - lx;
    const Lin ay = lin_axis(a.h, a.ch, a.sy, ly);
    const Lin ax = lin_axis(a.w, a.cw, a.sx, lx);
    const float* p = views + a.first;
    const int plane = a.h * a.w;  // <= 2^24
    float n00[3], n01[3], n10[3], n11[3];
    decode(p, plane, ay.i0 * a.w + ax.i0, raw, n00);
    decode(p, plane, ay.i0 * a.w + ax.i1, raw, n01);
    decode(p, plane, ay.i1 * a.w + ax.i0, raw, n10);
    decode(p, plane, ay.i1 * a.w + ax.i1, raw, n11);
    ++n;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float t0 = ax.l0 * n00[ch];
      t0 += ax.l1 * n01[ch];
      float t1 = ax.l0 * n10[ch];
      t1 += ax.l1 * n11[ch];
      float t = ay.l0 * t0;
      t += ay.l1 * t1;
      if (ch == 0 && a.flip) t = -t;  // the mirrored network saw x pointing the other way
      if (M > 0) sel[ch].insert(t);
      else sum[ch] += t;
    }
  }

  float v[3] = {0.f, 0.f, 0.f};  // no view: the zero vector
  if (n > 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (M > 0) v[ch] = (sel[ch].at((n - 1) >> 1) + sel[ch].at(n >> 1)) * 0.5f;  // np.median
      else v[ch] = sum[ch] / (float)n;
    }
  }
  float ss = v[0] * v[0];
  ss += v[1] * v[1];
  ss += v[2] * v[2];
  const float d = fmaxf(sqrtf(ss), 1e-12f);
  for (int ch = 0; ch < 3; ++ch) v[ch] = fminf(fmaxf((v[ch] / d + 1.f) / 2.f, 0.f), 1.f);

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

template <int M>
void launch(int base, int tiles, hipStream_t st, const float* views, const ViewArgs& args, int nv, const MergeOut& o, int raw,
            uint8_t* out) {
  if (base == M_U8) hipLaunchKernelGGL((tta_merge_kernel<M, M_U8>), dim3(tiles), dim3(256), 0, st, views, args, nv, o, raw, out);
  else hipLaunchKernelGGL((tta_merge_kernel<M, M_F32>), dim3(tiles), dim3(256), 0, st, views, args, nv, o, raw, out);
}

}  // namespace

extern "C" int dptx_tta_merge_normals(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const dptx_image_desc* outs,
                                      int32_t B, int32_t mode, void* out_dev, void* stream) {
  if (!views_dev || !views || !outs || !out_dev || B < 1 || B > 4096 || n_views < B || (long long)n_views > (long long)MAXV * B ||
      ((uintptr_t)views_dev & 3))
    return DPTX_E_INVALID;
  const int base = mode & ~(DPTX_TTA_MEAN | DPTX_TTA_RAW_VIEWS);
  if (mode < 0 || (base != M_U8 && base != M_F32)) return DPTX_E_INVALID;
  if (base == M_F32 && ((uintptr_t)out_dev & 3)) return DPTX_E_INVALID;
  // the whole call is checked before the first launch: every image has 1..64 consecutive views, images ascending
  for (int i = 0; i < B; ++i)
    if (!out_ok(outs[i], base == M_U8 ? 3 : 4)) return DPTX_E_INVALID;
  if (!views_ok(views, n_views, outs, B)) return DPTX_E_INVALID;

  const int raw = (mode & DPTX_TTA_RAW_VIEWS) ? 1 : 0;
  const bool mean = (mode & DPTX_TTA_MEAN) != 0;
  int k = 0;
  for (int i = 0; i < B; ++i) {
    ViewArgs args = {};
    int nv = 0;
    for (; k < n_views && views[k].image == i; ++k, ++nv) args.v[nv] = view_arg(views[k]);
    const dptx_image_desc& d = outs[i];
    const MergeOut o = {d.offset, d.H, d.W, d.row_stride_bytes, 0};
    const int tiles = ((d.W + TW - 1) / TW) * ((d.H + TH - 1) / TH);  // <= 2^20
    const hipStream_t st = (hipStream_t)stream;
    const float* src = (const float*)views_dev;
    uint8_t* out = (uint8_t*)out_dev;
    if (mean) launch<0>(base, tiles, st, src, args, nv, o, raw, out);
    else if (nv <= 8) launch<5>(base, tiles, st, src, args, nv, o, raw, out);
    else if (nv <= 16) launch<9>(base, tiles, st, src, args, nv, o, raw, out);
    else if (nv <= 32) launch<17>(base, tiles, st, src, args, nv, o, raw, out);
    else launch<33>(base, tiles, st, src, args, nv, o, raw, out);
  }
  return hipGetLastError() == hipSuccess ? DPTX_OK : DPTX_E_HIP;
}
