// eval_metrics.hip -- the evaluation metrics of the reference (paper_code/evaluation_metrics.py:13-106) for task='normal' and
// task='depth_zbuffer', forward only, as stream-ordered stages on a caller-provided workspace (no allocation, no host
// synchronisation, no host read of the mask count).  One call yields one row for the whole batch or one row per image.
//
//  a. terms pass, grid (blocks of an image, images): every thread takes units of four consecutive pixels of ONE image
//     (16-byte loads of the planes and one 4-byte load of the mask where H*W % 4 == 0 and the pointers allow it, scalar
//     loads over the same units otherwise: the same sums on either path), evaluates the pixel's terms in fp64 and adds
//     them; block_sum -> one partial row per block.  The normal form also writes each pixel's 64-bit order-preserving key
//     of its angle and builds pass 0 of the median's histogram in LDS, flushed once per block.
//  b. seven select passes over the keys (normal only), most significant digit first: 8 passes of 8 bits in all.
//  c. finalize, one block per row: the row's partials in index order -> the fields; the last histogram -> the median.
// Sums: fp64 in an order fixed by (H, W) alone -- the blocks of an image never depend on B or on the image's place in the
// batch, so a per-image row is the same bits in any batch.  No float atomics; the histograms are integer counts, so the
// median does not depend on the order of the atomics that built them.
// Median: the exact np.median of the valid pixels' fp64 angles.  Both middle ranks, floor((n - 1) / 2) and floor(n / 2),
// are selected at once (they coincide for odd n); while their prefixes agree one histogram serves both.  n is the total
// of pass 0's histogram, so no pass waits for a count from the host.  A pixel outside the mask, and a valid pixel whose
// angle is NaN, carries the key ~0 and enters no histogram; a row with such a NaN gets a NaN median (np.median's answer).
// Keys are WRITTEN ONCE (8 B / pixel of workspace) rather than recomputed in every pass: a recomputing pass would re-read
// 24 B / pixel and redo two square roots, a division and an fp64 acos per pixel seven more times, against an 8-byte read.
// Numerics: per-pixel arithmetic in fp64 on the fp32 inputs, no contraction in this unit: every product, sum, sqrt and
// division is the correctly rounded one, as on the CPU.  Masking follows the reference: every term is computed for every
// pixel and multiplied by the 0 / 1 mask, so a non-finite term outside the mask poisons its sum as it does there.
//
// dptx_eval_depth_aligned (a' below) is the depth form of a prediction that is first fitted to the target per image, by
// least squares or by median and mean deviation: midas_loss.hip's stats stages (midas_stats.h) leave every image's
// coefficients in the workspace, one terms pass aligns each pixel in fp32 as it loads it and adds the depth form's eight
// sums and seven more (AbsRel, SqRel, RMSE, RMSE-log, delta < 1.25^k), and one finalize launch writes the B per-image rows
// and the batch row.  The aligned tensor is never written unless the caller asks for it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"
#include "midas_stats.h"
#include "select.h"

#pragma clang fp contract(off)

namespace {

using namespace dptx;

constexpr int TPB = 256;
constexpr int64_t PER_BLOCK = 256;    // units (of four pixels) per block of the terms pass, at least
constexpr int64_t SEL_PER_BLOCK = 4096;  // keys per block of a select pass, at least
constexpr int64_t MAX_BLOCKS = 1024;  // per image, of either pass
constexpr int64_t MAX_FLAT_BLOCKS = 1 << 16;
constexpr int NS = 9;                 // sums per partial row (the depth form uses 8 of them)
constexpr int SPASS = 8;              // 8-bit digits of a 64-bit key
constexpr uint64_t NO_KEY = ~0ull;
static_assert(DPTX_EVAL_NORMAL_FIELDS == 9 && DPTX_EVAL_DEPTH_FIELDS == 8, "fields");

// one select (one row): its histograms and its state before each pass
struct SelState {
  uint64_t pre[2];   // the digits selected so far, for the two ranks
  uint32_t rank[2];  // the ranks left among the keys with that prefix
};
constexpr int64_t HIST_WORDS = (int64_t)SPASS * 2 * BINS;  // uint32 [SPASS][2][BINS]
constexpr int64_t HIST_BYTES = HIST_WORDS * 4;
constexpr int64_t STATE_BYTES = (int64_t)SPASS * sizeof(SelState);  // state[q] = before pass q, q = 1 .. 7

struct Layout {
  int64_t HW, total, units, nblk, per_block, sel_nblk, sel_per_block;
  int64_t off_part, off_hist, off_state, bytes;
};

// include/dptx.h dptx_eval_workspace_bytes documents these sizes
bool layout(int32_t B, int32_t H, int32_t W, Layout& lo) {
  if (B < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || (int64_t)H * W > MAX_HW) return false;
  lo.HW = (int64_t)H * W;
  lo.total = (int64_t)B * lo.HW;
  if (lo.total >= (1ll << 32)) return false;
  lo.units = (lo.HW + 3) / 4;
  split(lo.units, PER_BLOCK, MAX_BLOCKS, lo.nblk, lo.per_block);
  split(lo.HW, SEL_PER_BLOCK, MAX_BLOCKS, lo.sel_nblk, lo.sel_per_block);
  lo.off_part = align256(lo.total * 8);                               // keys uint64 [B][HW]
  lo.off_hist = lo.off_part + align256((int64_t)B * lo.nblk * NS * 8);  // partials fp64 [B][nblk][NS]
  lo.off_state = lo.off_hist + (int64_t)B * HIST_BYTES;               // histograms, one set per row (at most B rows)
  lo.bytes = lo.off_state + align256((int64_t)B * STATE_BYTES);
  return true;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---------------------------------------------------------------- the per-pixel arithmetic (fp64 on the fp32 inputs)
constexpr double DEG = 180.0 / 3.14159265358979323846;

// :36-43: acos of the cosine with (|p| |t|).clamp(min=1e-8), clamped to [-1, 1], in degrees; np_, nt: the two norms
__device__ __forceinline__ double angle(const double p[3], const double t[3], double& np_, double& nt) {
  const double dot = (p[0] * t[0] + p[1] * t[1]) + p[2] * t[2];
  np_ = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
  nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  double den = np_ * nt;
  den = den < 1e-8 ? 1e-8 : den;  // torch.clamp: NaN stays NaN
  double c = dot / den;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  return acos(c) * DEG;
}

// order-preserving key of a double; -0.0 and +0.0 are one key
__device__ __forceinline__ uint64_t d2key(double d) {
  const uint64_t u = (uint64_t)__double_as_longlong(d == 0.0 ? 0.0 : d);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double key2d(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

// one unit: four consecutive pixels r0 .. r0 + 3 of image b; in[k]: the pixel exists (r0 + k < HW)
template <int C>
struct Unit {
  float p[4][C], t[4][C];
  bool in[4], m[4];
};

template <int C, bool VEC>
__device__ __forceinline__ void load_unit(const float* __restrict__ pred, const float* __restrict__ target,
                                          const uint8_t* __restrict__ mask, int64_t b, int64_t r0, int64_t HW, Unit<C>& u) {
  const int64_t base = b * C * HW + r0;
  if constexpr (VEC) {  // H*W % 4 == 0: every address is a multiple of 16 bytes
    const uint32_t mm = *(const uint32_t*)(mask + b * HW + r0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u.in[k] = true;
      u.m[k] = ((mm >> (8 * k)) & 255u) != 0;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 a = *(const float4*)(pred + base + c * HW);
      const float4 g = *(const float4*)(target + base + c * HW);
      u.p[0][c] = a.x, u.p[1][c] = a.y, u.p[2][c] = a.z, u.p[3][c] = a.w;
      u.t[0][c] = g.x, u.t[1][c] = g.y, u.t[2][c] = g.z, u.t[3][c] = g.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u.in[k] = r0 + k < HW;
      u.m[k] = u.in[k] && mask[b * HW + r0 + k] != 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        u.p[k][c] = u.in[k] ? pred[base + k + c * HW] : 0.0f;
        u.t[k][c] = u.in[k] ? target[base + k + c * HW] : 0.0f;
      }
    }
  }
}

// ---------------------------------------------------------------- a. terms pass
// partial row of the normal form: sum of ang * m, of ang, of the soft-normalised |diff| * m, of its square, the count of
// the mask, the three counts of valid ang <= threshold, the count of valid NaN angles
template <bool VEC>
__global__ __launch_bounds__(TPB) void ev_normal_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const uint8_t* __restrict__ mask, int B, int64_t HW, int64_t units,
                                                        int64_t per_block, int per_image, uint64_t* __restrict__ keys,
                                                        double* __restrict__ part /*[B][nblk][NS]*/,
                                                        uint32_t* __restrict__ hist /*[rows][SPASS][2][BINS]*/) {
  __shared__ double red[4 * NS];
  __shared__ uint32_t lh[BINS];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < units ? lo + per_block : units;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    lh[threadIdx.x] = 0;
    __syncthreads();
    double v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += TPB) {
      Unit<3> u;
      load_unit<3, VEC>(pred, target, mask, b, 4 * i, HW, u);
      uint64_t key[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        key[k] = NO_KEY;
        if (!u.in[k]) continue;
        const double p[3] = {(double)u.p[k][0], (double)u.p[k][1], (double)u.p[k][2]};
        const double t[3] = {(double)u.t[k][0], (double)u.t[k][1], (double)u.t[k][2]};
        const double m = u.m[k] ? 1.0 : 0.0;
        double np_, nt;
        const double ang = angle(p, t, np_, nt);
        v[0] += ang * m;
        v[1] += ang;
        const double dp = np_ + 2e-2, dt = nt + 2e-2;  // :57-59
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double d = fabs(p[c] / dp - t[c] / dt) * m;
          v[2] += d;
          v[3] += d * d;
        }
        if (u.m[k]) {
          v[4] += 1.0;
          v[5] += ang <= 11.25 ? 1.0 : 0.0;  // a NaN compares false
          v[6] += ang <= 22.5 ? 1.0 : 0.0;
          v[7] += ang <= 30.0 ? 1.0 : 0.0;
          if (ang != ang) {
            v[8] += 1.0;
          } else {
            key[k] = d2key(ang);
            atomicAdd(&lh[(uint32_t)(key[k] >> 56)], 1u);
          }
        }
      }
      uint64_t* kp = keys + b * HW + 4 * i;
      if constexpr (VEC) {
        *(ulonglong2*)kp = make_ulonglong2(key[0], key[1]);
        *(ulonglong2*)(kp + 2) = make_ulonglong2(key[2], key[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (u.in[k]) kp[k] = key[k];
      }
    }
    block_sum<NS>(v, red, part + (b * gridDim.x + blockIdx.x) * NS);
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(hist + (per_image ? b : 0) * HIST_WORDS + threadIdx.x, c);
    __syncthreads();
  }
}

// the eight sums of the depth form for one pixel (p, t: the fp64 of the fp32 values, m: the 0 / 1 mask)
__device__ __forceinline__ void depth_terms(double p, double t, double m, double* v) {
  const double diff = fabs(p - t) * m;  // :61
  v[0] += m;
  v[1] += diff;
  v[2] += diff * diff;
  v[3] += log(1.0 + 64.0 * diff) * m;                              // :64
  const double dlog = fabs((log(1.0 + 64.0 * p) - log(1.0 + 64.0 * t)) * m);  // :68, :70
  v[4] += dlog;
  v[5] += dlog * dlog;
  v[6] += (diff / t) * m;                                          // :72: 0 / 0 outside the mask where target == 0
  const double ir = 1.0 / (1.0 + 64.0 * p) - 1.0 / (1.0 + 64.0 * t);  // :74
  v[7] += (ir * ir) * m;
}

// partial row of the depth form: the count, sums of |diff| m, its square, log(1 + 64 |diff| m) m, |dlog m|, its square,
// (|diff| m / t) m, (1 / (1 + 64 p) - 1 / (1 + 64 t))^2 m
template <bool VEC>
__global__ __launch_bounds__(TPB) void ev_depth_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ mask, int B, int64_t HW, int64_t units,
                                                       int64_t per_block, double* __restrict__ part /*[B][nblk][NS]*/) {
  __shared__ double red[4 * NS];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < units ? lo + per_block : units;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    double v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += TPB) {
      Unit<1> u;
      load_unit<1, VEC>(pred, target, mask, b, 4 * i, HW, u);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!u.in[k]) continue;
        depth_terms((double)u.p[k][0], (double)u.t[k][0], u.m[k] ? 1.0 : 0.0, v);
      }
    }
    block_sum<NS>(v, red, part + (b * gridDim.x + blockIdx.x) * NS);
  }
}

// ---------------------------------------------------------------- a'. the aligned depth form (dptx_eval_depth_aligned)
// The prediction is first mapped onto the target per image, with the coefficients that midas_loss.hip's stats stages left
// in the workspace (midas_stats.h: stats [B][DPTX_MIDAS_STATS] = t_p, t_g, s_p, s_g, n, scale, shift, argmedian), in fp32
// with every step rounded on its own:
//   LSTSQ   a = scale p, then a + shift                             (compute_scale_and_shift, midas_loss.py:10-30)
//   MEDIAN  pa = (p - t_p) / (s_p + 1e-6f), pa (s_g + 1e-6f), + t_g (masked_shift_and_scale, :33-56)
// then clamped to [0, 1] on request (a NaN stays a NaN).  Sums 0..7 are those of the depth form on that value, in the same
// partition and order; sums 8..14 are the benchmark fields over the VALID pixels only (selected, not multiplied), with
// a_e = max(a, min_depth), t_e = max(t, min_depth): |a_e - t_e| / t_e, (a_e - t_e)^2 / t_e, (a_e - t_e)^2,
// (ln a_e - ln t_e)^2 and the counts of max(a_e / t_e, t_e / a_e) < 1.25, 1.25^2, 1.25^3 (a NaN compares false).  A thread
// counts in integers; its counts (at most 4 per unit it takes, far below 2^32) enter the block's partial row as fp64, where
// sums of integers below 2^53 are exact: the row's count is the integer it would be in any order.
constexpr int NA = DPTX_EVAL_ALIGNED_FIELDS;  // sums per partial row of the aligned form
constexpr float ALIGN_EPS = 1e-6f;
static_assert(NA == 15 && DPTX_MIDAS_STATS == 8, "aligned fields");

struct Coef {
  float scale, shift;    // LSTSQ
  float tp, tg, dp, dg;  // MEDIAN: the medians and s + 1e-6f
};

__device__ __forceinline__ Coef load_coef(const float* __restrict__ st /*[DPTX_MIDAS_STATS]*/) {
  Coef c;
  c.tp = st[0], c.tg = st[1];
  c.dp = st[2] + ALIGN_EPS, c.dg = st[3] + ALIGN_EPS;
  c.scale = st[5], c.shift = st[6];
  return c;
}

template <bool MEDIAN>
__device__ __forceinline__ float align_value(float p, const Coef& c, bool clamp) {
  float a;
  if constexpr (MEDIAN) {
    const float pa = (p - c.tp) / c.dp;
    a = pa * c.dg;
    a = a + c.tg;
  } else {
    a = c.scale * p;
    a = a + c.shift;
  }
  if (clamp) a = a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a);  // torch.clamp: NaN stays NaN
  return a;
}

template <bool VEC, bool MEDIAN>
__global__ __launch_bounds__(TPB) void ev_aligned_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         const uint8_t* __restrict__ mask, int B, int64_t HW, int64_t units,
                                                         int64_t per_block, const float* __restrict__ stats, int clamp,
                                                         double min_depth, float* __restrict__ coeffs /*[B][2]*/,
                                                         float* __restrict__ aligned_out /*nullable*/,
                                                         double* __restrict__ part /*[B][nblk][NA]*/) {
  __shared__ double red[4 * NA];
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < units ? lo + per_block : units;
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const Coef c = load_coef(stats + b * DPTX_MIDAS_STATS);  // block-uniform
    if (blockIdx.x == 0 && threadIdx.x == 0) {               // the reported pair; MEDIAN: the equivalent scale and shift
      float cs = c.scale, ch = c.shift;
      if constexpr (MEDIAN) {
        cs = c.dg / c.dp;
        const float q = cs * c.tp;
        ch = c.tg - q;
      }
      coeffs[2 * b] = cs;
      coeffs[2 * b + 1] = ch;
    }
    double v[NA];
#pragma unroll
    for (int s = 0; s < NA; ++s) v[s] = 0.0;
    uint32_t within[3] = {0, 0, 0};
    for (int64_t i = lo + threadIdx.x; i < hi; i += TPB) {
      Unit<1> u;
      load_unit<1, VEC>(pred, target, mask, b, 4 * i, HW, u);
      float al[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        al[k] = 0.0f;
        if (!u.in[k]) continue;
        al[k] = align_value<MEDIAN>(u.p[k][0], c, clamp != 0);
        const double a = (double)al[k], t = (double)u.t[k][0];
        depth_terms(a, t, u.m[k] ? 1.0 : 0.0, v);
        if (u.m[k]) {
          const double ae = a < min_depth ? min_depth : a, te = t < min_depth ? min_depth : t;  // NaN stays NaN
          const double d = ae - te, dd = d * d;
          v[8] += fabs(d) / te;
          v[9] += dd / te;
          v[10] += dd;
          const double lg = log(ae) - log(te);
          v[11] += lg * lg;
          const double r1 = ae / te, r2 = te / ae;
          const double r = r1 > r2 ? r1 : r2;  // a_e, t_e > 0: one ratio is NaN only where the other is too
          within[0] += r < 1.25 ? 1u : 0u;
          within[1] += r < 1.5625 ? 1u : 0u;
          within[2] += r < 1.953125 ? 1u : 0u;
        }
      }
      if (aligned_out) {
        float* ap = aligned_out + b * HW + 4 * i;
        if constexpr (VEC) {
          *(float4*)ap = make_float4(al[0], al[1], al[2], al[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (u.in[k]) ap[k] = al[k];
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) v[12 + s] = (double)within[s];
    block_sum<NA>(v, red, part + (b * gridDim.x + blockIdx.x) * NA);
  }
}

// ---------------------------------------------------------------- b. the 64-bit select
// The state after the pass whose histograms are h0, h1 (for the two ranks; the same array while their prefixes agree):
// in = the state before that pass, out = prefix << 8 | digit and the rank left.  first: the pass was pass 0, whose total is
// n, and the ranks looked for are floor((n - 1) / 2) and floor(n / 2).  A histogram without the rank (no key at all) keeps
// prefix << 8 and rank 0.
__device__ __forceinline__ void resolve64(const uint32_t* __restrict__ h0, const uint32_t* __restrict__ h1, bool first,
                                          uint32_t (*sc)[BINS] /*LDS [2]*/, SelState* res /*LDS*/, uint64_t (&pre)[2],
                                          uint32_t (&rank)[2], uint32_t& n) {
  const int t = threadIdx.x;
  const uint32_t hv[2] = {h0[t], h1[t]};
  sc[0][t] = hv[0];
  sc[1][t] = hv[1];
  if (t < 2) {
    res->pre[t] = pre[t] << 8;
    res->rank[t] = 0;
  }
  block_scan256<2>(sc);
  n = sc[0][BINS - 1];
  if (first) {
    rank[0] = n ? (n - 1) / 2 : 0;
    rank[1] = n / 2;
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const uint32_t inc = sc[a][t], ex = inc - hv[a];
    if (ex <= rank[a] && rank[a] < inc) {  // at most one bin holds the rank
      res->pre[a] = (pre[a] << 8) | (uint64_t)t;
      res->rank[a] = rank[a] - ex;
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    pre[a] = res->pre[a];
    rank[a] = res->rank[a];
  }
  __syncthreads();
}

// the state before pass q (1 <= q <= SPASS) of one row, from the state before pass q - 1 and that pass's histograms
__device__ __forceinline__ void state_before(const uint32_t* __restrict__ hist, const SelState* __restrict__ state, int q,
                                             uint32_t (*sc)[BINS], SelState* res, uint64_t (&pre)[2], uint32_t (&rank)[2],
                                             uint32_t& n) {
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    pre[a] = q == 1 ? 0ull : state[q - 1].pre[a];
    rank[a] = q == 1 ? 0u : state[q - 1].rank[a];
  }
  const uint32_t* h = hist + (int64_t)(q - 1) * 2 * BINS;
  resolve64(h, pre[0] == pre[1] ? h : h + BINS, q == 1, sc, res, pre, rank, n);
}

// pass q, 1 <= q <= 7, grid (blocks of an image, images): digit q of the keys whose higher digits are a selected prefix
__global__ __launch_bounds__(TPB) void ev_select_kernel(const uint64_t* __restrict__ keys, int B, int64_t HW, int64_t per_block,
                                                        int per_image, int q, uint32_t* __restrict__ hist,
                                                        SelState* __restrict__ state) {
  __shared__ uint32_t sc[2][BINS];
  __shared__ uint32_t lh[2][BINS];
  __shared__ SelState res;
  const int64_t lo = (int64_t)blockIdx.x * per_block, hi = lo + per_block < HW ? lo + per_block : HW;
  const int shift = 64 - 8 * (q + 1);
  for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t row = per_image ? b : 0;
    uint32_t* h = hist + row * HIST_WORDS;
    SelState* st = state + row * SPASS;
    uint64_t pre[2];
    uint32_t rank[2], n;
    state_before(h, st, q, sc, &res, pre, rank, n);
    if (blockIdx.x == 0 && (per_image || b == 0) && threadIdx.x < 2) {
      st[q].pre[threadIdx.x] = pre[threadIdx.x];
      st[q].rank[threadIdx.x] = rank[threadIdx.x];
    }
    lh[0][threadIdx.x] = 0;
    lh[1][threadIdx.x] = 0;
    __syncthreads();
    const bool same = pre[0] == pre[1];
    for (int64_t r = lo + threadIdx.x; r < hi; r += TPB) {
      const uint64_t key = keys[b * HW + r];
      if (key == NO_KEY) continue;
      const uint64_t top = key >> (shift + 8);  // shift + 8 <= 56
      const uint32_t digit = (uint32_t)(key >> shift) & 255u;
      if (top == pre[0]) atomicAdd(&lh[0][digit], 1u);
      if (!same && top == pre[1]) atomicAdd(&lh[1][digit], 1u);
    }
    __syncthreads();
    uint32_t* hq = h + (int64_t)q * 2 * BINS;
    const uint32_t c0 = lh[0][threadIdx.x], c1 = lh[1][threadIdx.x];
    if (c0) atomicAdd(hq + threadIdx.x, c0);
    if (c1) atomicAdd(hq + BINS + threadIdx.x, c1);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- c. finalize
// the partials [first, first + count) of N sums each in index order -> sums[N], valid in every thread with t < N
template <int N = NS>
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int64_t first, int64_t count, double* red,
                                             double* sums /*LDS [N]*/) {
  double s[N];
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0;
  for (int64_t j = threadIdx.x; j < count; j += TPB)
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += part[(first + j) * N + k];
  block_sum<N>(s, red, sums);
}

__global__ __launch_bounds__(TPB) void ev_normal_finalize_kernel(const double* __restrict__ part, int64_t nblk, int B, int64_t HW,
                                                                 int per_image, int64_t rows, const uint32_t* __restrict__ hist,
                                                                 const SelState* __restrict__ state, double* __restrict__ out) {
  __shared__ double red[4 * NS];
  __shared__ double sums[NS];
  __shared__ uint32_t sc[2][BINS];
  __shared__ SelState res;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double numel = (double)(per_image ? HW : (int64_t)B * HW);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    sum_partials(part, per_image ? row * nblk : 0, per_image ? nblk : (int64_t)B * nblk, red, sums);
    uint64_t pre[2];
    uint32_t rank[2], n;
    state_before(hist + row * HIST_WORDS, state + row * SPASS, SPASS, sc, &res, pre, rank, n);
    if (threadIdx.x == 0) {
      const double N = sums[4], inv_valid = numel / N;
      double* o = out + row * DPTX_EVAL_NORMAL_FIELDS;
      o[0] = N;
      const bool some = N > 0.0;
      o[1] = some ? sums[0] / N : nan;                                              // :46
      o[2] = some && !(sums[8] > 0.0) ? (key2d(pre[0]) + key2d(pre[1])) * 0.5 : nan;  // :49-50; odd n: the two are one value
      o[3] = some ? sums[1] / numel : nan;                                          // :47
      o[4] = some ? sums[5] / N : nan;                                              // :52-54
      o[5] = some ? sums[6] / N : nan;
      o[6] = some ? sums[7] / N : nan;
      o[7] = some ? sums[2] / (3.0 * numel) * inv_valid * 100.0 : nan;              // :77, :85
      o[8] = some ? sums[3] / (3.0 * numel) * inv_valid * 100.0 : nan;              // :78-79, :84
    }
    __syncthreads();
  }
}

// the eight fields of the depth form from a row's sums
__device__ __forceinline__ void depth_fields(const double* sums, double numel, double* o) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double N = sums[0], inv_valid = numel / N;
  o[0] = N;
  const bool some = N > 0.0;
  o[1] = some ? sums[1] / numel * inv_valid * 100.0 : nan;          // :77, :85
  o[2] = some ? sums[2] / numel * inv_valid * 100.0 : nan;          // :78-79, :84
  o[3] = some ? sums[3] / numel * inv_valid : nan;                  // :66
  o[4] = some ? sums[4] / numel * inv_valid : nan;                  // :68
  o[5] = some ? sums[5] / N - (sums[4] * sums[4]) / (N * N) : nan;  // :71
  o[6] = some ? sums[6] / numel * inv_valid : nan;                  // :72
  o[7] = some ? sums[7] / numel * inv_valid : nan;                  // :74
}

__global__ __launch_bounds__(TPB) void ev_depth_finalize_kernel(const double* __restrict__ part, int64_t nblk, int B, int64_t HW,
                                                                int per_image, int64_t rows, double* __restrict__ out) {
  __shared__ double red[4 * NS];
  __shared__ double sums[NS];
  const double numel = (double)(per_image ? HW : (int64_t)B * HW);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    sum_partials(part, per_image ? row * nblk : 0, per_image ? nblk : (int64_t)B * nblk, red, sums);
    if (threadIdx.x == 0) {
      depth_fields(sums, numel, out + row * DPTX_EVAL_DEPTH_FIELDS);
    }
    __syncthreads();
  }
}

// rows 0 .. B - 1: the images (the partials of image `row`); row B: the whole batch (all partials), as the depth form's
// two kinds of call
__global__ __launch_bounds__(TPB) void ev_aligned_finalize_kernel(const double* __restrict__ part, int64_t nblk, int B, int64_t HW,
                                                                  double* __restrict__ out /*[B + 1][NA]*/) {
  __shared__ double red[4 * NA];
  __shared__ double sums[NA];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t row = blockIdx.x; row <= B; row += gridDim.x) {
    const bool image = row < B;
    sum_partials<NA>(part, image ? row * nblk : 0, image ? nblk : (int64_t)B * nblk, red, sums);
    if (threadIdx.x == 0) {
      double* o = out + row * NA;
      depth_fields(sums, (double)(image ? HW : (int64_t)B * HW), o);
      const double N = sums[0];
      const bool some = N > 0.0;
      o[8] = some ? sums[8] / N : nan;
      o[9] = some ? sums[9] / N : nan;
      o[10] = some ? sqrt(sums[10] / N) : nan;
      o[11] = some ? sqrt(sums[11] / N) : nan;
      o[12] = some ? sums[12] / N : nan;
      o[13] = some ? sums[13] / N : nan;
      o[14] = some ? sums[14] / N : nan;
    }
    __syncthreads();
  }
}

// include/dptx.h dptx_eval_aligned_workspace_bytes documents these sizes
struct AlignedLayout {
  Layout ev;  // the block partition of the depth form
  int64_t off_stats, off_midas, bytes;
};

bool aligned_layout(int32_t B, int32_t H, int32_t W, AlignedLayout& al) {
  int64_t midas = 0;
  if (!layout(B, H, W, al.ev) || !midas_stats_workspace(B, H, W, &midas)) return false;
  al.off_stats = align256((int64_t)B * al.ev.nblk * NA * 8);                   // partials fp64 [B][nblk][NA]
  al.off_midas = al.off_stats + align256((int64_t)B * DPTX_MIDAS_STATS * 4);  // stats fp32 [B][DPTX_MIDAS_STATS]
  al.bytes = al.off_midas + midas;                                            // the workspace of the stats stages
  return true;
}

// ---------------------------------------------------------------- per-pixel angles
__global__ __launch_bounds__(TPB) void ev_pixels_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t total,
                                                        int64_t HW, double* __restrict__ ang) {
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < total; q += (int64_t)gridDim.x * TPB) {
    const int64_t b = q / HW, at = b * 3 * HW + (q - b * HW);
    const double p[3] = {(double)pred[at], (double)pred[at + HW], (double)pred[at + 2 * HW]};
    const double t[3] = {(double)target[at], (double)target[at + HW], (double)target[at + 2 * HW]};
    double np_, nt;
    ang[q] = angle(p, t, np_, nt);
  }
}

bool vec_ok(const Layout& lo, const void* pred, const void* target, const void* mask, const void* ws) {
  return lo.HW % 4 == 0 && aligned(pred, 16) && aligned(target, 16) && aligned(mask, 4) && aligned(ws, 16);
}

}  // namespace

extern "C" {

int dptx_eval_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes) {
  Layout lo;
  if (!bytes || !layout(B, H, W, lo)) return DPTX_E_INVALID;
  *bytes = lo.bytes;
  return DPTX_OK;
}

int dptx_eval_normal(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                     double* out, void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!pred || !target || !mask || !out || !ws || !aligned(ws, 8) || !layout(B, H, W, lo) || ws_bytes < lo.bytes ||
      (flags & ~DPTX_EVAL_PER_IMAGE))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int per_image = (flags & DPTX_EVAL_PER_IMAGE) ? 1 : 0;
  const int64_t rows = per_image ? B : 1;
  uint64_t* keys = (uint64_t*)ws;
  double* part = (double*)((char*)ws + lo.off_part);
  uint32_t* hist = (uint32_t*)((char*)ws + lo.off_hist);
  SelState* state = (SelState*)((char*)ws + lo.off_state);
  // the histograms of the rows in use; keys, partials and states are written before they are read
  if (hipMemsetAsync(hist, 0, (size_t)(rows * HIST_BYTES), st) != hipSuccess) return DPTX_E_HIP;
  const dim3 grid((unsigned)lo.nblk, (unsigned)grid_y(B));
  if (vec_ok(lo, pred, target, mask, ws))
    hipLaunchKernelGGL(ev_normal_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, (int)B, lo.HW, lo.units, lo.per_block,
                       per_image, keys, part, hist);
  else
    hipLaunchKernelGGL(ev_normal_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, (int)B, lo.HW, lo.units, lo.per_block,
                       per_image, keys, part, hist);
  const dim3 sgrid((unsigned)lo.sel_nblk, (unsigned)grid_y(B));
  for (int q = 1; q < SPASS; ++q)
    hipLaunchKernelGGL(ev_select_kernel, sgrid, dim3(TPB), 0, st, keys, (int)B, lo.HW, lo.sel_per_block, per_image, q, hist, state);
  hipLaunchKernelGGL(ev_normal_finalize_kernel, dim3((unsigned)std::min<int64_t>(rows, MAX_GRID_Y)), dim3(TPB), 0, st, part, lo.nblk, (int)B, lo.HW,
                     per_image, rows, hist, state, out);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_eval_depth(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                    double* out, void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!pred || !target || !mask || !out || !ws || !aligned(ws, 8) || !layout(B, H, W, lo) || ws_bytes < lo.bytes ||
      (flags & ~DPTX_EVAL_PER_IMAGE))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int per_image = (flags & DPTX_EVAL_PER_IMAGE) ? 1 : 0;
  double* part = (double*)((char*)ws + lo.off_part);
  const dim3 grid((unsigned)lo.nblk, (unsigned)grid_y(B));
  if (vec_ok(lo, pred, target, mask, ws))
    hipLaunchKernelGGL(ev_depth_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, (int)B, lo.HW, lo.units, lo.per_block, part);
  else
    hipLaunchKernelGGL(ev_depth_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, (int)B, lo.HW, lo.units, lo.per_block, part);
  const int64_t rows = per_image ? B : 1;
  hipLaunchKernelGGL(ev_depth_finalize_kernel, dim3((unsigned)std::min<int64_t>(rows, MAX_GRID_Y)), dim3(TPB), 0, st, part, lo.nblk, (int)B, lo.HW,
                     per_image, rows, out);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_eval_aligned_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes) {
  AlignedLayout al;
  if (!bytes || !aligned_layout(B, H, W, al)) return DPTX_E_INVALID;
  *bytes = al.bytes;
  return DPTX_OK;
}

int dptx_eval_depth_aligned(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W,
                            int32_t align, int32_t flags, float min_depth, double* out, float* coeffs, float* aligned_out, void* ws,
                            int64_t ws_bytes, void* stream) {
  AlignedLayout al;
  if (!pred || !target || !mask || !out || !coeffs || !ws || !aligned(ws, 8) || !aligned_layout(B, H, W, al) ||
      ws_bytes < al.bytes || (align != DPTX_EVAL_ALIGN_LSTSQ && align != DPTX_EVAL_ALIGN_MEDIAN) ||
      (flags & ~DPTX_EVAL_ALIGNED_CLAMP) || !(min_depth > 0.0f) || !std::isfinite(min_depth))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const Layout& lo = al.ev;
  double* part = (double*)ws;
  float* stats = (float*)((char*)ws + al.off_stats);
  const bool median = align == DPTX_EVAL_ALIGN_MEDIAN;
  // the solve kernel of the stats stages writes the coefficients; the metric pass below reads them in stream order
  if (!midas_stats_launch(pred, target, mask, B, H, W, median ? DPTX_MIDAS_SSI : DPTX_MIDAS_ALIGN, stats, (char*)ws + al.off_midas, st))
    return DPTX_E_HIP;
  const dim3 grid((unsigned)lo.nblk, (unsigned)grid_y(B));
  const int clamp = (flags & DPTX_EVAL_ALIGNED_CLAMP) ? 1 : 0;
  const bool vec = vec_ok(lo, pred, target, mask, ws) && (!aligned_out || aligned(aligned_out, 16));
#define DPTX_EV_ALIGNED(V, M)                                                                                                   \
  hipLaunchKernelGGL((ev_aligned_kernel<V, M>), grid, dim3(TPB), 0, st, pred, target, mask, (int)B, lo.HW, lo.units, lo.per_block, \
                     (const float*)stats, clamp, (double)min_depth, coeffs, aligned_out, part)
  if (vec && median) DPTX_EV_ALIGNED(true, true);
  else if (vec) DPTX_EV_ALIGNED(true, false);
  else if (median) DPTX_EV_ALIGNED(false, true);
  else DPTX_EV_ALIGNED(false, false);
#undef DPTX_EV_ALIGNED
  hipLaunchKernelGGL(ev_aligned_finalize_kernel, dim3((unsigned)std::min<int64_t>((int64_t)B + 1, MAX_GRID_Y)), dim3(TPB), 0, st,
                     (const double*)part, lo.nblk, (int)B, lo.HW, out);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_eval_normal_pixels(const float* pred, const float* target, int32_t B, int32_t H, int32_t W, double* ang, void* stream) {
  Layout lo;
  if (!pred || !target || !ang || !layout(B, H, W, lo)) return DPTX_E_INVALID;
  const unsigned blocks = (unsigned)std::min<int64_t>((lo.total + TPB - 1) / TPB, MAX_FLAT_BLOCKS);
  hipLaunchKernelGGL(ev_pixels_kernel, dim3(blocks), dim3(TPB), 0, (hipStream_t)stream, pred, target, lo.total, lo.HW, ang);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
