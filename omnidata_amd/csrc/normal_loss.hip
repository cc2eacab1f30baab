// normal_loss.hip -- the surface-normal training objective of the reference (omnidata_tools/torch/train_normal.py:205-265 with
// losses/masked_losses.py) and its gradient with respect to the prediction, as stream-ordered stages on a caller-provided
// workspace (no allocation, no host synchronisation, no host read of the mask count).
//
//  a. loss pass: every thread takes units of four consecutive pixels of the flat [B][H][W] order (16-byte loads from the six
//     planes and one 4-byte load of the mask where H*W % 4 == 0 and the pointers allow it, scalar loads otherwise: the same
//     units, so the same sums on either path), evaluates the pixel's cosine term and its three |p - t| in fp32, and adds them
//     and the mask count in fp64; block_sum -> one partial triple per block.
//  b. finalize (one wave): the partials in index order -> N, cos = sum / N, l1 = sum / (3 N), total -> fp32 once each, and
//     the record (the counts) for the backward.
//  c. backward, the same units: re-reads the inputs and writes the closed-form gradient, evaluated in fp64 from the fp32
//     inputs with the clamp, sign and eps decisions of the fp32 forward, rounded once.
// dptx_masked_loss is the flat per-element form of (a)-(c) for masked_l1_loss / masked_mse_loss / masked_loss, and
// dptx_valid_mask is make_valid_mask (max_pool2d of 1 - m, nearest-neighbour resize back, == 0).
// Numerics: forward in fp32, every step rounded on its own as the reference's fp32 tensors are (no contraction in this unit);
// fp64 for every sum.  No atomics at all: every sum runs in a fixed order, so results are bitwise reproducible.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"
#include "select.h"

#pragma clang fp contract(off)

namespace {

using namespace dptx;

constexpr int TPB = 256;
constexpr int64_t PER_BLOCK = 1024;       // units (of four pixels / elements) per block of the loss pass, at least
constexpr int64_t MAX_BLOCKS = 1024;
constexpr int64_t MAX_FLAT_BLOCKS = 1 << 16;  // the elementwise kernels stride over the rest
constexpr int64_t MAX_ELEMS = 1ll << 40;
constexpr float EPS = 1e-12f;             // F.normalize's eps as an fp32 tensor sees it
static_assert(DPTX_NORMAL_RECORD_DOUBLES == 1, "record");  // the count alone: nl_finalize_kernel writes record[0]
constexpr int ALL_FLAGS = DPTX_NORMAL_L1 | DPTX_NORMAL_COS | DPTX_NORMAL_CLAMP_PRED;

struct Layout {
  int64_t HW, total, units, nblk, per_block, bytes;
};

// include/dptx.h dptx_normal_workspace_bytes / dptx_masked_workspace_bytes document these sizes
bool layout_flat(int64_t total, Layout& lo) {
  lo.total = total;
  lo.units = (total + 3) / 4;
  split(lo.units, PER_BLOCK, MAX_BLOCKS, lo.nblk, lo.per_block);
  lo.bytes = align256(lo.nblk * 3 * 8);  // fp64 [nblk][3]
  return true;
}

bool shape_ok(int32_t B, int32_t H, int32_t W) {
  return B >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE && (int64_t)H * W <= MAX_HW;
}

bool layout(int32_t B, int32_t H, int32_t W, Layout& lo) {
  if (!shape_ok(B, H, W)) return false;
  lo.HW = (int64_t)H * W;
  return layout_flat((int64_t)B * lo.HW, lo);
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

unsigned flat_blocks(int64_t items) { return (unsigned)std::min<int64_t>((items + TPB - 1) / TPB, MAX_FLAT_BLOCKS); }

// ---------------------------------------------------------------- the per-pixel arithmetic (fp32, as the reference's tensors)
// torch.clamp: NaN stays NaN
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
// torch's clamp passes its gradient where lo <= v <= hi, ends included
__device__ __forceinline__ bool inside(float v, float lo, float hi) { return v >= lo && v <= hi; }

// (2 p - 1).clamp(-1, 1) -> x, its norm as F.normalize takes it -> whether the norm (not eps) is the denominator
__device__ __forceinline__ bool scaled(const float p[3], float x[3], float& den) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = clampf(2.0f * p[c] - 1.0f, -1.0f, 1.0f);
  const float nrm = sqrtf((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  const bool big = !(nrm < EPS);  // clamp_min(eps): a NaN norm stays
  den = big ? nrm : EPS;
  return big;
}

// masked_cosine_angular_loss (:14-23) at one pixel: -(x / max(|x|, eps)) . (y / max(|y|, eps))
__device__ __forceinline__ float cos_term(const float p[3], const float t[3]) {
  float x[3], y[3], dx, dy;
  scaled(p, x, dx);
  scaled(t, y, dy);
  return -(((x[0] / dx) * (y[0] / dy) + (x[1] / dx) * (y[1] / dy)) + (x[2] / dx) * (y[2] / dy));
}

// one unit: four consecutive pixels q0 .. q0 + 3 of the flat [B][H][W] order; m[k] = in range and valid
struct Unit {
  float p[4][3], t[4][3];
  bool m[4];
  int64_t at[4];  // the offset of channel 0 of pixel k in the [B][3][H][W] tensors
};

template <bool VEC>
__device__ __forceinline__ void load_unit(const float* __restrict__ pred, const float* __restrict__ target,
                                          const uint8_t* __restrict__ mask, int64_t q0, int64_t total, int64_t HW, bool clamp_pred,
                                          Unit& u) {
  int64_t b = q0 / HW, r = q0 - b * HW;
  if constexpr (VEC) {  // H*W % 4 == 0: the four pixels lie in one image, every address is a multiple of 16 bytes
    const uint32_t mm = *(const uint32_t*)(mask + q0);
    const int64_t base = b * 3 * HW + r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u.m[k] = ((mm >> (8 * k)) & 255u) != 0;
      u.at[k] = base + k;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 a = *(const float4*)(pred + base + c * HW);
      const float4 g = *(const float4*)(target + base + c * HW);
      u.p[0][c] = a.x, u.p[1][c] = a.y, u.p[2][c] = a.z, u.p[3][c] = a.w;
      u.t[0][c] = g.x, u.t[1][c] = g.y, u.t[2][c] = g.z, u.t[3][c] = g.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = q0 + k < total;
      u.m[k] = in && mask[q0 + k] != 0;
      u.at[k] = b * 3 * HW + r;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        u.p[k][c] = u.m[k] ? pred[u.at[k] + c * HW] : 0.0f;
        u.t[k][c] = u.m[k] ? target[u.at[k] + c * HW] : 0.0f;
      }
      if (++r == HW) r = 0, ++b;
    }
  }
  if (clamp_pred)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) u.p[k][c] = clampf(u.p[k][c], 0.0f, 1.0f);
}

// ---------------------------------------------------------------- a. loss pass
template <bool VEC>
__global__ __launch_bounds__(TPB) void nl_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      const uint8_t* __restrict__ mask, int64_t total, int64_t HW, int64_t units,
                                                      int64_t per_block, int flags, double* __restrict__ part /*[nblk][3]*/) {
  __shared__ double red[4 * 3];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < units ? lo + per_block : units;
  const bool want_cos = flags & DPTX_NORMAL_COS, want_l1 = flags & DPTX_NORMAL_L1;
  double v[3] = {0.0, 0.0, 0.0};  // cos, l1, count
  for (int64_t i = lo + threadIdx.x; i < hi; i += TPB) {
    Unit u;
    load_unit<VEC>(pred, target, mask, 4 * i, total, HW, flags & DPTX_NORMAL_CLAMP_PRED, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!u.m[k]) continue;
      v[2] += 1.0;
      if (want_cos) v[0] += (double)cos_term(u.p[k], u.t[k]);
      if (want_l1)
        v[1] += ((double)fabsf(u.p[k][0] - u.t[k][0]) + (double)fabsf(u.p[k][1] - u.t[k][1])) + (double)fabsf(u.p[k][2] - u.t[k][2]);
    }
  }
  block_sum<3>(v, red, part + (int64_t)blockIdx.x * 3);
}

// ---------------------------------------------------------------- b. finalize
// the partials in index order -> sums[NS] in lane 0
template <int NS>
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int nblk, double (&s)[NS]) {
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 64)
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] += part[(int64_t)j * 3 + k];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = wave_sum(s[k]);
}

__global__ __launch_bounds__(64) void nl_finalize_kernel(const double* __restrict__ part, int nblk, int flags, float l1_weight,
                                                         float* __restrict__ losses, double* __restrict__ record /*nullable*/) {
  double s[3];
  sum_partials<3>(part, nblk, s);
  if (threadIdx.x != 0) return;
  const double N = s[2];
  const double cosv = (flags & DPTX_NORMAL_COS) ? s[0] / N : 0.0;  // N = 0: 0 / 0 = NaN, the mean of nothing
  const double l1 = (flags & DPTX_NORMAL_L1) ? s[1] / (3.0 * N) : 0.0;
  const double total = (flags & DPTX_NORMAL_COS) ? ((flags & DPTX_NORMAL_L1) ? cosv + (double)l1_weight * l1 : cosv) : l1;
  losses[0] = (float)total;
  losses[1] = (float)l1;
  losses[2] = (float)cosv;
  if (record) record[0] = N;
}

// ---------------------------------------------------------------- c. backward
__device__ __forceinline__ double sgn32(float v) { return (double)((v > 0.0f) - (v < 0.0f)); }

// x = clamp(2 p - 1) in fp64 on the branch the fp32 evaluation took; pass: the clamp lets the gradient through
__device__ __forceinline__ void scaled64(const float p[3], double x[3], bool pass[3], double& inv_den, bool& big) {
  float x32[3], den32;
  big = scaled(p, x32, den32);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pass[c] = inside(2.0f * p[c] - 1.0f, -1.0f, 1.0f);
    x[c] = pass[c] ? 2.0 * (double)p[c] - 1.0 : (double)x32[c];
  }
  inv_den = 1.0 / (big ? sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) : (double)EPS);
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void nl_backward_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, int64_t total, int64_t HW, int64_t units,
                                                          int flags, float l1_weight, const double* __restrict__ record,
                                                          const float* __restrict__ grad_losses, float* __restrict__ grad) {
  const bool want_cos = flags & DPTX_NORMAL_COS, want_l1 = flags & DPTX_NORMAL_L1, clamp_pred = flags & DPTX_NORMAL_CLAMP_PRED;
  const double N = record[0];
  const double g0 = (double)grad_losses[0];
  // d(g0 total + g1 l1 + g2 cos): total = cos + w l1 with both terms, else the one term; an absent term is the constant 0
  const double gc = want_cos ? (double)grad_losses[2] + g0 : 0.0;
  const double gl = want_l1 ? (double)grad_losses[1] + (want_cos ? g0 * (double)l1_weight : g0) : 0.0;
  const bool empty = !(N > 0.0);  // the reference's gradient of 0 / 0 over no pixel: nothing
  const double kc = empty ? 0.0 : gc / N, kl = empty ? 0.0 : gl / (3.0 * N);
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < units; i += (int64_t)gridDim.x * TPB) {
    Unit u;
    // the raw prediction: the clamp's own pass decision needs it
    load_unit<VEC>(pred, target, mask, 4 * i, total, HW, false, u);
    float out[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pc[3];
      bool pass1[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pass1[c] = !clamp_pred || inside(u.p[k][c], 0.0f, 1.0f);
        pc[c] = clamp_pred ? clampf(u.p[k][c], 0.0f, 1.0f) : u.p[k][c];
        out[c][k] = 0.0f;
      }
      if (!u.m[k] || empty) continue;
      double g[3] = {0.0, 0.0, 0.0};
      if (want_cos) {
        double x[3], y[3], ix, iy;
        bool px[3], py[3], bx, by;
        scaled64(pc, x, px, ix, bx);
        scaled64(u.t[k], y, py, iy, by);
        const double xh[3] = {x[0] * ix, x[1] * ix, x[2] * ix}, yh[3] = {y[0] * iy, y[1] * iy, y[2] * iy};
        // through max(|x|, eps): to |x| where it is the denominator, else the denominator is the constant eps
        const double dot = bx ? (xh[0] * yh[0] + xh[1] * yh[1]) + xh[2] * yh[2] : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = px[c] ? -2.0 * kc * ((yh[c] - dot * xh[c]) * ix) : 0.0;
      }
      if (want_l1)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] += kl * sgn32(pc[c] - u.t[k][c]);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c][k] = pass1[c] ? (float)g[c] : 0.0f;
    }
    if constexpr (VEC) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *(float4*)(grad + u.at[0] + c * HW) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * i + k < total)
#pragma unroll
          for (int c = 0; c < 3; ++c) grad[u.at[k] + c * HW] = out[c][k];
    }
  }
}

// ---------------------------------------------------------------- per-pixel terms
__global__ __launch_bounds__(TPB) void nl_pixels_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const uint8_t* __restrict__ mask, int64_t total, int64_t HW, int64_t units,
                                                        int flags, float* __restrict__ cos_out, float* __restrict__ l1_out) {
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < units; i += (int64_t)gridDim.x * TPB) {
    Unit u;
    load_unit<false>(pred, target, mask, 4 * i, total, HW, flags & DPTX_NORMAL_CLAMP_PRED, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (4 * i + k >= total) continue;
      float c = 0.0f, l = 0.0f;
      if (u.m[k]) {
        c = cos_term(u.p[k], u.t[k]);
        l = (float)(((double)fabsf(u.p[k][0] - u.t[k][0]) + (double)fabsf(u.p[k][1] - u.t[k][1])) +
                    (double)fabsf(u.p[k][2] - u.t[k][2]));
      }
      if (cos_out) cos_out[4 * i + k] = c;
      if (l1_out) l1_out[4 * i + k] = l;
    }
  }
}

// ---------------------------------------------------------------- the flat per-element form
struct Unit1 {
  float p[4], t[4];
  bool m[4];
};

template <bool VEC>
__device__ __forceinline__ void load_unit1(const float* __restrict__ pred, const float* __restrict__ target /*nullable*/,
                                           const uint8_t* __restrict__ mask, int64_t q0, int64_t n, Unit1& u) {
  if constexpr (VEC) {
    const uint32_t mm = *(const uint32_t*)(mask + q0);
    const float4 a = *(const float4*)(pred + q0);
    const float4 g = target ? *(const float4*)(target + q0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    u.p[0] = a.x, u.p[1] = a.y, u.p[2] = a.z, u.p[3] = a.w;
    u.t[0] = g.x, u.t[1] = g.y, u.t[2] = g.z, u.t[3] = g.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) u.m[k] = ((mm >> (8 * k)) & 255u) != 0;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u.m[k] = q0 + k < n && mask[q0 + k] != 0;
      u.p[k] = u.m[k] ? pred[q0 + k] : 0.0f;
      u.t[k] = u.m[k] && target ? target[q0 + k] : 0.0f;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void ml1_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ mask, int64_t n, int64_t units, int64_t per_block,
                                                       int what, double* __restrict__ part /*[nblk][3]*/) {
  __shared__ double red[4 * 2];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < units ? lo + per_block : units;
  double v[2] = {0.0, 0.0};  // sum, count
  for (int64_t i = lo + threadIdx.x; i < hi; i += TPB) {
    Unit1 u;
    load_unit1<VEC>(pred, target, mask, 4 * i, n, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!u.m[k]) continue;
      v[1] += 1.0;
      const float d = u.p[k] - u.t[k];
      v[0] += (double)(what == DPTX_MASKED_L1 ? fabsf(d) : (what == DPTX_MASKED_MSE ? d * d : u.p[k]));
    }
  }
  block_sum<2>(v, red, part + (int64_t)blockIdx.x * 3);
}

__global__ __launch_bounds__(64) void ml1_finalize_kernel(const double* __restrict__ part, int nblk, int empty_zero,
                                                          float* __restrict__ loss, double* __restrict__ record /*nullable*/) {
  double s[2];
  sum_partials<2>(part, nblk, s);
  if (threadIdx.x != 0) return;
  loss[0] = (empty_zero && s[1] == 0.0) ? 0.0f : (float)(s[0] / s[1]);
  if (record) record[0] = s[1];
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void ml1_backward_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           const uint8_t* __restrict__ mask, int64_t n, int64_t units, int what,
                                                           const double* __restrict__ record, const float* __restrict__ grad_loss,
                                                           float* __restrict__ grad) {
  const double N = record[0];
  const double kk = N > 0.0 ? (double)grad_loss[0] / N : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < units; i += (int64_t)gridDim.x * TPB) {
    Unit1 u;
    load_unit1<VEC>(pred, target, mask, 4 * i, n, u);
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double g = 0.0;
      if (u.m[k]) {
        if (what == DPTX_MASKED_L1) g = kk * sgn32(u.p[k] - u.t[k]);
        else if (what == DPTX_MASKED_MSE) g = kk * (2.0 * ((double)u.p[k] - (double)u.t[k]));
        else g = kk;
      }
      out[k] = (float)g;
    }
    if constexpr (VEC) {
      *(float4*)(grad + 4 * i) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * i + k < n) grad[4 * i + k] = out[k];
    }
  }
}

// ---------------------------------------------------------------- make_valid_mask
// F.interpolate(mode='nearest') back from the pooled grid: min(floor(dst * (float(in) / float(out))), in - 1)
__device__ __forceinline__ int nearest(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  return min((int)floorf((float)dst * scale), in - 1);
}

__global__ __launch_bounds__(TPB) void valid_mask_kernel(const float* __restrict__ m, int64_t total, int H, int W, int pool,
                                                         uint8_t* __restrict__ valid) {
  const int Hp = H / pool, Wp = W / pool;
  const int64_t HW = (int64_t)H * W;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < total; q += (int64_t)gridDim.x * TPB) {
    const int64_t b = q / HW;
    const int r = (int)(q - b * HW);
    const int i = r / W, j = r - i * W;
    const int wi = nearest(i, Hp, H) * pool, wj = nearest(j, Wp, W) * pool;
    const float* src = m + b * HW + (int64_t)wi * W + wj;
    // max_pool2d of 1 - m propagates NaN; the pixel is valid where the window's maximum is exactly 0
    float mx = -INFINITY;
    bool nan = false;
    for (int y = 0; y < pool; ++y)
      for (int x = 0; x < pool; ++x) {
        const float v = 1.0f - src[(int64_t)y * W + x];
        nan = nan || v != v;
        mx = v > mx ? v : mx;
      }
    valid[q] = (!nan && mx == 0.0f) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

int dptx_normal_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes) {
  Layout lo;
  if (!bytes || !layout(B, H, W, lo)) return DPTX_E_INVALID;
  *bytes = lo.bytes;
  return DPTX_OK;
}

int dptx_masked_workspace_bytes(int64_t n, int64_t* bytes) {
  Layout lo;
  if (!bytes || n < 1 || n > MAX_ELEMS || !layout_flat(n, lo)) return DPTX_E_INVALID;
  *bytes = lo.bytes;
  return DPTX_OK;
}

int dptx_normal_loss(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                     float l1_weight, float* losses, double* record, void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!pred || !target || !mask || !losses || !ws || !layout(B, H, W, lo) || ws_bytes < lo.bytes || (flags & ~ALL_FLAGS) ||
      !(flags & (DPTX_NORMAL_L1 | DPTX_NORMAL_COS)))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  const bool vec = lo.HW % 4 == 0 && aligned(pred, 16) && aligned(target, 16) && aligned(mask, 4);
  const dim3 grid((unsigned)lo.nblk);
  if (vec)
    hipLaunchKernelGGL(nl_loss_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, lo.total, lo.HW, lo.units, lo.per_block,
                       (int)flags, part);
  else
    hipLaunchKernelGGL(nl_loss_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, lo.total, lo.HW, lo.units, lo.per_block,
                       (int)flags, part);
  hipLaunchKernelGGL(nl_finalize_kernel, dim3(1), dim3(64), 0, st, part, (int)lo.nblk, (int)flags, l1_weight, losses, record);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_normal_loss_backward(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W,
                              int32_t flags, float l1_weight, const double* record, const float* grad_losses, float* grad_pred,
                              void* stream) {
  Layout lo;
  if (!pred || !target || !mask || !record || !grad_losses || !grad_pred || !layout(B, H, W, lo) || (flags & ~ALL_FLAGS) ||
      !(flags & (DPTX_NORMAL_L1 | DPTX_NORMAL_COS)))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = lo.HW % 4 == 0 && aligned(pred, 16) && aligned(target, 16) && aligned(mask, 4) && aligned(grad_pred, 16);
  const dim3 grid(flat_blocks(lo.units));
  if (vec)
    hipLaunchKernelGGL(nl_backward_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, lo.total, lo.HW, lo.units, (int)flags,
                       l1_weight, record, grad_losses, grad_pred);
  else
    hipLaunchKernelGGL(nl_backward_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, lo.total, lo.HW, lo.units, (int)flags,
                       l1_weight, record, grad_losses, grad_pred);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_normal_pixels(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                       float* cos, float* l1, void* stream) {
  Layout lo;
  if (!pred || !target || !mask || (!cos && !l1) || !layout(B, H, W, lo) || (flags & ~ALL_FLAGS)) return DPTX_E_INVALID;
  hipLaunchKernelGGL(nl_pixels_kernel, dim3(flat_blocks(lo.units)), dim3(TPB), 0, (hipStream_t)stream, pred, target, mask, lo.total,
                     lo.HW, lo.units, (int)flags, cos, l1);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_masked_loss(const float* pred, const float* target, const uint8_t* mask, int64_t n, int32_t kind, float* loss,
                     double* record, void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  const int what = kind & 3;
  if (!pred || !mask || !loss || !ws || n < 1 || n > MAX_ELEMS || (kind & ~7) || what == 3 ||
      (what == DPTX_MASKED_VALUE ? target != nullptr : target == nullptr) || !layout_flat(n, lo) || ws_bytes < lo.bytes)
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  const bool vec = n % 4 == 0 && aligned(pred, 16) && aligned(target, 16) && aligned(mask, 4);
  const dim3 grid((unsigned)lo.nblk);
  if (vec)
    hipLaunchKernelGGL(ml1_loss_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, n, lo.units, lo.per_block, what, part);
  else
    hipLaunchKernelGGL(ml1_loss_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, n, lo.units, lo.per_block, what, part);
  hipLaunchKernelGGL(ml1_finalize_kernel, dim3(1), dim3(64), 0, st, part, (int)lo.nblk, (kind & DPTX_MASKED_EMPTY_ZERO) ? 1 : 0, loss,
                     record);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_masked_loss_backward(const float* pred, const float* target, const uint8_t* mask, int64_t n, int32_t kind,
                              const double* record, const float* grad_loss, float* grad_pred, void* stream) {
  Layout lo;
  const int what = kind & 3;
  if (!pred || !mask || !record || !grad_loss || !grad_pred || n < 1 || n > MAX_ELEMS || (kind & ~7) || what == 3 ||
      (what == DPTX_MASKED_VALUE ? target != nullptr : target == nullptr) || !layout_flat(n, lo))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = n % 4 == 0 && aligned(pred, 16) && aligned(target, 16) && aligned(mask, 4) && aligned(grad_pred, 16);
  const dim3 grid(flat_blocks(lo.units));
  if (vec)
    hipLaunchKernelGGL(ml1_backward_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, n, lo.units, what, record, grad_loss,
                       grad_pred);
  else
    hipLaunchKernelGGL(ml1_backward_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, n, lo.units, what, record, grad_loss,
                       grad_pred);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_valid_mask(const float* mask_float, int32_t B, int32_t H, int32_t W, int32_t pool, uint8_t* valid, void* stream) {
  if (!mask_float || !valid || !shape_ok(B, H, W) || pool < 1 || H < pool || W < pool) return DPTX_E_INVALID;
  const int64_t total = (int64_t)B * H * W;
  hipLaunchKernelGGL(valid_mask_kernel, dim3(flat_blocks(total)), dim3(TPB), 0, (hipStream_t)stream, mask_float, total, (int)H, (int)W,
                     (int)pool, valid);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
