// tta_depth.hip -- test-time augmentation for depth (include/dptx.h, "Test-time augmentation for depth"): the views of an image
// are maps that agree only up to an affine map each, so every view is first fitted to one anchor view that covers the whole
// image (the least-squares scale and shift the network was trained with, losses/midas_loss.py compute_scale_and_shift), and the
// merge takes the median (np.median) or the mean of scale * view + shift per pixel.  Stream-ordered, the caller's workspace
// only, no allocation, no host synchronisation, no float atomics; per image three launches for the alignment and one for the merge,
// with the image's (at most 64) views by value in the arguments.
//
// View value: clamp(m, 0, 1) at the network's resolution, then ATen's bilinear taps in the blend order of the normals merge
// (resample_batch.h lin_axis, tta.hip); view_value() (tta_depth_align.h) is the only place that forms it -- the anchor pass, the stats pass
// and the merge call it, so a pixel of a view has the same bits wherever it is used.
//
// Anchor pass: the anchor of the image -> [H][W] fp32 in the workspace, 64 x 4 tiles, one pixel per thread.  The stats pass
//   reads it coalesced instead of sampling the anchor again for each of up to 63 views.
// Stats pass: grid over (view, tile of its window), tiles of 64 columns x 16 rows, a thread owns one column and 4 rows (the
//   rows r, r + 4, r + 8, r + 12: a wave reads one row of the anchor plane at a time).  Per pixel: 4 taps through cache, one
//   coalesced anchor load, three fp32 -> fp64 conversions, two fp64 products and four fp64 additions.  The fp64 VALU runs at half
//   the fp32 rate on this part and the taps' address arithmetic is several times that work, so the pass is bound by the gathered
//   loads' latency, not by fp64: 4 pixels per thread amortise block_sum (24 fp64 shuffles, one LDS round) over 1024 pixels while
//   a 512 x 683 window still gives 352 blocks per view (13.7k per 40-view image) and the kernel stays under 40 VGPRs (8 waves per SIMD), so the
//   latency is hidden by occupancy, not by unrolling.  One record (sum r, sum r^2, sum a, sum r a) per block, at the tile's index
//   in the view's own list: the layout of a view's partials depends on its window alone, so two runs, and the same image in
//   another batch, add the same numbers in the same order.
// Solve: one wave per view; lane l adds the records l, l + 64, ... in index order, wave_sum joins the lanes (a fixed tree),
//   lane 0 solves the 2 x 2 system in fp64 and rounds once to fp32.  The anchor gets exactly (1, 0).
// Merge: tta_merge_kernel's structure (tta.hip) with one channel -- 64 x 4 tiles, Lowest<M> in the same four classes, the loop
//   over the views not unrolled -- and scale * r + shift (an fp32 multiply, then an add) in front of the selection.  The merge
//   reads the ANCHOR FROM ITS VIEW like every other view, not from the resized copy: the bits are the same (1 * r + 0), the
//   loop keeps one body, and the merge needs no workspace.
// Contraction is off (resample_batch.h), and select.h adds fp64 only.
#include "tta_depth_align.h"  // view_value, the anchor, stats and solve kernels: shared with tiles.hip

namespace {

template <int M>
__global__ __launch_bounds__(256) void tta_depth_merge_kernel(const float* __restrict__ views, ViewArgs args, int nv, MergeOut o,
                                                              const float* __restrict__ coeffs, uint8_t* __restrict__ out) {
  const int tid = threadIdx.x;
  const int tiles_x = (o.W + TW - 1) / TW;
  const int X = (blockIdx.x % tiles_x) * TW + tid % TW, Y = (blockIdx.x / tiles_x) * TH + tid / TW;
  const bool inside = X < o.W && Y < o.H;

  Lowest<M> sel;
  float sum = 0.f;
  int n = 0;
  sel.clear();

  for (int k = 0; k < nv; ++k) {
    const ViewArg a = args.v[k];
    const int ly = Y - a.y0, lx = X - a.x0;
    if (!inside || ly < 0 || ly >= a.ch || lx < 0 || lx >= a.cw) continue;
    float t = view_value(views, a, ly, lx);
    if (coeffs) {
      t = coeffs[2 * k] * t;
      t += coeffs[2 * k + 1];
    }
    ++n;
    if (M > 0) sel.insert(t);
    else sum += t;
  }

  float v = 0.f;  // no view (possible only without an anchor, coeffs == NULL)
  if (n > 0) {
    if (M > 0) v = (sel.at((n - 1) >> 1) + sel.at(n >> 1)) * 0.5f;  // np.median
    else v = sum / (float)n;
  }
  if (inside) *(float*)(out + o.offset + (size_t)Y * o.stride + (size_t)X * 4) = 1.f - fminf(fmaxf(v, 0.f), 1.f);
}

template <int M>
void launch_merge(int tiles, hipStream_t st, const float* views, const ViewArgs& args, int nv, const MergeOut& o, const float* coeffs,
                  uint8_t* out) {
  hipLaunchKernelGGL((tta_depth_merge_kernel<M>), dim3(tiles), dim3(256), 0, st, views, args, nv, o, coeffs, out);
}

// the whole call is checked before the first launch
bool shape_ok(const dptx_tta_view* views, int n_views, const dptx_image_desc* outs, int B) {
  if (!views || !outs || B < 1 || B > 4096 || n_views < B || (long long)n_views > (long long)MAXV * B) return false;
  for (int i = 0; i < B; ++i)
    if (!out_ok(outs[i], 4)) return false;
  return views_ok(views, n_views, outs, B);
}

inline long long stats_tiles(const dptx_tta_view& v) { return stats_tiles(v.ch, v.cw); }

// workspace: [anchor plane of image 0 | ... | of image B - 1 | the records of every view, in view order], each part at a
// multiple of 256 bytes.  -> total bytes; plane_at[i] (may be null) = byte offset of image i's plane, *records_at of the records
long long layout(const dptx_tta_view* views, int n_views, const dptx_image_desc* outs, int B, long long* plane_at,
                 long long* records_at) {
  long long at = 0;
  for (int i = 0; i < B; ++i) {
    if (plane_at) plane_at[i] = at;
    at += dptx::align256(4ll * outs[i].H * outs[i].W);
  }
  if (records_at) *records_at = at;
  long long records = 0;
  for (int k = 0; k < n_views; ++k) records += stats_tiles(views[k]);
  return at + dptx::align256(records * NSUM * (long long)sizeof(double));
}

}  // namespace

extern "C" int dptx_tta_depth_workspace_bytes(const dptx_tta_view* views, int32_t n_views, const dptx_image_desc* outs, int32_t B,
                                              int64_t* bytes) {
  if (!bytes || !shape_ok(views, n_views, outs, B)) return DPTX_E_INVALID;
  *bytes = layout(views, n_views, outs, B, nullptr, nullptr);
  return DPTX_OK;
}

extern "C" int dptx_tta_align_depth(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const int32_t* anchors,
                                    const dptx_image_desc* outs, int32_t B, float* coeffs_dev, void* ws, int64_t ws_bytes,
                                    void* stream) {
  if (!views_dev || ((uintptr_t)views_dev & 3) || !shape_ok(views, n_views, outs, B) || !anchors || !coeffs_dev ||
      ((uintptr_t)coeffs_dev & 3) || !ws || ((uintptr_t)ws & 7))
    return DPTX_E_INVALID;
  for (int i = 0; i < B; ++i) {  // the anchor is a view of its image and covers the whole of it
    const int a = anchors[i];
    if (a < 0 || a >= n_views || views[a].image != i) return DPTX_E_INVALID;
    const dptx_tta_view& v = views[a];
    if (v.y0 != 0 || v.x0 != 0 || v.ch != outs[i].H || v.cw != outs[i].W) return DPTX_E_INVALID;
  }
  long long plane_at[4096], records_at = 0;
  if (ws_bytes < layout(views, n_views, outs, B, plane_at, &records_at)) return DPTX_E_INVALID;

  const hipStream_t st = (hipStream_t)stream;
  const float* src = (const float*)views_dev;
  double* records = (double*)((char*)ws + records_at);
  int k = 0;
  for (int i = 0; i < B; ++i) {
    ViewArgs args = {};
    StatsArgs sa = {};
    const int k0 = k;
    int nv = 0;
    long long blocks = 0;
    for (; k < n_views && views[k].image == i; ++k, ++nv) {
      args.v[nv] = view_arg(views[k]);
      sa.first[nv] = (int)blocks;
      blocks += stats_tiles(views[k]);  // <= 64 * 2^18
    }
    sa.first[nv] = (int)blocks;
    const dptx_image_desc& d = outs[i];
    const int anchor = anchors[i] - k0;
    float* plane = (float*)((char*)ws + plane_at[i]);
    const int tiles = ((d.W + TW - 1) / TW) * ((d.H + TH - 1) / TH);
    hipLaunchKernelGGL(tta_depth_anchor_kernel, dim3(tiles), dim3(256), 0, st, src, args.v[anchor], d.H, d.W, plane);
    hipLaunchKernelGGL(tta_depth_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, args, sa, nv, anchor, d.W, plane,
                       records);
    hipLaunchKernelGGL(tta_depth_solve_kernel, dim3(nv), dim3(64), 0, st, args, sa, anchor, records, coeffs_dev + 2 * (size_t)k0);
    records += (size_t)blocks * NSUM;
  }
  return dptx::launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

extern "C" int dptx_tta_merge_depth(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const float* coeffs_dev,
                                    const dptx_image_desc* outs, int32_t B, int32_t mode, void* out_dev, const void* ws, void* stream) {
  (void)ws;  // the anchor is sampled from its view (see the head of this file): nothing of the workspace is read
  if (!views_dev || ((uintptr_t)views_dev & 3) || !shape_ok(views, n_views, outs, B) || !out_dev || ((uintptr_t)out_dev & 3) ||
      ((uintptr_t)coeffs_dev & 3))
    return DPTX_E_INVALID;
  if (mode != DPTX_RESIZE_DEPTH_F32 && mode != (DPTX_RESIZE_DEPTH_F32 | DPTX_TTA_MEAN)) return DPTX_E_INVALID;

  const bool mean = (mode & DPTX_TTA_MEAN) != 0;
  const hipStream_t st = (hipStream_t)stream;
  const float* src = (const float*)views_dev;
  uint8_t* out = (uint8_t*)out_dev;
  int k = 0;
  for (int i = 0; i < B; ++i) {
    ViewArgs args = {};
    const float* coeffs = coeffs_dev ? coeffs_dev + 2 * (size_t)k : nullptr;
    int nv = 0;
    for (; k < n_views && views[k].image == i; ++k, ++nv) args.v[nv] = view_arg(views[k]);
    const dptx_image_desc& d = outs[i];
    const MergeOut o = {d.offset, d.H, d.W, d.row_stride_bytes, 0};
    const int tiles = ((d.W + TW - 1) / TW) * ((d.H + TH - 1) / TH);  // <= 2^20
    if (mean) launch_merge<0>(tiles, st, src, args, nv, o, coeffs, out);
    else if (nv <= 8) launch_merge<5>(tiles, st, src, args, nv, o, coeffs, out);
    else if (nv <= 16) launch_merge<9>(tiles, st, src, args, nv, o, coeffs, out);
    else if (nv <= 32) launch_merge<17>(tiles, st, src, args, nv, o, coeffs, out);
    else launch_merge<33>(tiles, st, src, args, nv, o, coeffs, out);
  }
  return dptx::launch_ok() ? DPTX_OK : DPTX_E_HIP;
}
