// midas_loss.hip -- the MiDaS depth loss of the reference (omnidata_tools/torch/losses/midas_loss.py) and its gradient with
// respect to the prediction, as stream-ordered stages on a caller-provided workspace (no allocation, no host synchronisation,
// no host read of any count or median: graph-capturable).
//
//  a. count + select (:33-56): pass 0 counts the valid pixels n, the non-NaN valid values of prediction and target and the
//     mask of every gradient level (M_k), and histograms the first 8-bit digit of the order-preserving keys; passes 1..3
//     histogram the next digit of the keys under the prefix selected so far: the radix select of select.h, on both arrays
//     at once.  The rank is the lower median floor((k-1)/2) of the k non-NaN valid values (torch.nanmedian).  Integer
//     atomics only: deterministic.
//  b. stats pass: the median keys, the lowest linear index of a valid pixel with the prediction's median key (the pixel the
//     median's gradient flows to), per-block fp64 partial sums of |x - t| (prediction, target), sign(p - t_p) and the
//     alignment system of compute_scale_and_shift (:10-30).
//  c. solve (one wave per image): s = fp32(sum / (n + 1)), the 2x2 solve in fp64, scale / shift rounded to fp32, the weights
//     of the gradient levels under the reduction.
//  d. loss pass: sum |a - g| (:104-111) and every level's sum of m_x |d(y, x+2^k) - d(y, x)| (+ vertical) (:83-101) from
//     one pass over the pixels; with a gradient, also the per-image sums the backward's coefficients need.
//  e. per-image totals of the partials (one wave per image, fixed order); finalize (one block): (total, ssi, reg) and the
//     per-image coefficient record.
//  f. backward: one elementwise pass -> grad_pred.
// Numerics: fp32 where the reference keeps a per-pixel fp32 tensor (1/(x + 1e-6), t, s, a, g, scale, shift, r, d), every
// step rounded on its own (no contraction in this unit); fp64 for every sum and for the solve.  No float atomics: every
// reduction runs in a fixed order, so results are bitwise reproducible and per-image statistics do not depend on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"
#include "midas_stats.h"
#include "select.h"

#pragma clang fp contract(off)

namespace {

using namespace dptx;

constexpr int MAX_SCALES = 8;
constexpr int TPB = 256;
constexpr int64_t PX_PER_BLOCK = 4096;
constexpr int64_t MAX_BLOCKS = 1024;
constexpr int CNT = 16;               // uint32 counters per image: [0] n, [1] k_p, [2] k_t, [3] ~argmedian (0: none), [8+k] M_k
constexpr int NPART = 16;             // fp64 partial sums per (image, block)
constexpr int REC = DPTX_MIDAS_RECORD_DOUBLES;
constexpr float EPS = 1e-6f;
constexpr int ALL_TERMS = DPTX_MIDAS_SSI | DPTX_MIDAS_GRAD | DPTX_MIDAS_ALIGN | DPTX_MIDAS_INVERSE;

// record slots (per image, fp64); include/dptx.h documents the ones a caller reads
enum : int {
  R_TP = 0, R_TG, R_SP, R_SG, R_DP, R_DG, R_N, R_KP, R_SCALE, R_SHIFT, R_DETOK, R_MED, R_KD, R_KS, R_KMED, R_C00, R_C01, R_CB0,
  R_A00, R_A01, R_B0, R_B1, R_SU, R_W = 24
};
// stats-pass partials
enum : int { P_UP = 0, P_UG, P_SU, P_A00, P_A01, P_B0, P_B1, P_STATS };
// loss-pass partials
enum : int { P_SSI = 0, P_E, P_EU, P_S, P_T, P_L = 5 };

struct Layout {
  int64_t nblk, per_block;
  int64_t o_gcnt, o_cnt, o_hist, o_state, o_rec, o_tot, o_part, zero_bytes, total;
};

// include/dptx.h dptx_midas_workspace_bytes documents these sizes
bool layout(int32_t B, int32_t H, int32_t W, int32_t scales, Layout& lo) {
  if (B < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || (int64_t)H * W > MAX_HW || scales < 1 || scales > MAX_SCALES)
    return false;
  const int64_t HW = (int64_t)H * W;
  split(HW, PX_PER_BLOCK, MAX_BLOCKS, lo.nblk, lo.per_block);
  lo.o_gcnt = 0;                                        // uint64 [1 + MAX_SCALES]: sum n, sum_b M_k
  lo.o_cnt = 256;                                       // uint32 [B][CNT]
  lo.o_hist = lo.o_cnt + (int64_t)B * CNT * 4;          // uint32 [B][NPASS][2][BINS]
  lo.zero_bytes = align256(lo.o_hist + (int64_t)B * NPASS * 2 * BINS * 4);
  lo.o_state = lo.zero_bytes;                           // uint32 [B][NPASS + 1][2][2]
  lo.o_rec = lo.o_state + align256((int64_t)B * (NPASS + 1) * 16);  // fp64 [B][REC]
  lo.o_tot = lo.o_rec + align256((int64_t)B * REC * 8);              // fp64 [B][NPART]
  lo.o_part = lo.o_tot + align256((int64_t)B * NPART * 8);           // fp64 [B][nblk][NPART]
  lo.total = lo.o_part + align256((int64_t)B * lo.nblk * NPART * 8);
  return true;
}

struct Ws {
  unsigned long long* gcnt;
  uint32_t* cnt;
  uint32_t* hist;
  uint32_t* state;
  double* rec;
  double* tot;
  double* part;
};

Ws ws_view(void* ws, const Layout& lo) {
  char* base = (char*)ws;
  return Ws{(unsigned long long*)(base + lo.o_gcnt), (uint32_t*)(base + lo.o_cnt), (uint32_t*)(base + lo.o_hist),
            (uint32_t*)(base + lo.o_state), (double*)(base + lo.o_rec), (double*)(base + lo.o_tot), (double*)(base + lo.o_part)};
}

struct Shape {
  int B, H, W, scales, terms, nblk;
  uint32_t HW, per_block;
};

__device__ __forceinline__ int sgn(float v) { return (v > 0.0f) - (v < 0.0f); }

// x or 1 / (x + 1e-6) (:147-148: reciprocal, correctly rounded)
__device__ __forceinline__ float xform(float v, bool inv) { return inv ? 1.0f / (v + EPS) : v; }

// the select state of image b before pass q (select.h); the rank is the lower median (torch.nanmedian)
__device__ __forceinline__ void select_state(const Ws& w, int b, int q, uint32_t (*sc)[BINS], uint32_t* res, bool (&has)[2],
                                             uint32_t (&pre)[2], uint32_t (&rank)[2]) {
  const uint32_t* cnt = w.cnt + (int64_t)b * CNT;
  const uint32_t k[2] = {cnt[1], cnt[2]};
  uint32_t rank0[2];
  for (int a = 0; a < 2; ++a) {
    has[a] = k[a] > 0;
    rank0[a] = has[a] ? (k[a] - 1) / 2 : 0u;
  }
  dptx::select_state<2>(w.hist + (int64_t)b * NPASS * 2 * BINS, w.state + (int64_t)b * (NPASS + 1) * 4, q, sc, res, has, rank0, pre,
                        rank);
}

// ---------------------------------------------------------------- a. count + digit histograms
__global__ __launch_bounds__(TPB) void ml_pass_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                      const uint8_t* __restrict__ mask, Ws w, Shape s, int pass) {
  __shared__ uint32_t lh[2][BINS];
  __shared__ uint32_t sc[2][BINS];
  __shared__ uint32_t res[4];
  __shared__ uint32_t lc[4 + MAX_SCALES];
  const int t = threadIdx.x;
  const bool sel = s.terms & DPTX_MIDAS_SSI;
  for (int b = blockIdx.y; b < s.B; b += gridDim.y) {
    bool has[2] = {sel, sel};
    uint32_t pre[2] = {0, 0}, rank[2] = {0, 0};
    if (pass > 0) select_state(w, b, pass, sc, res, has, pre, rank);
    lh[0][t] = 0;
    lh[1][t] = 0;
    if (t < 4 + MAX_SCALES) lc[t] = 0;
    __syncthreads();
    const int64_t base = (int64_t)b * s.HW;
    const uint32_t lo = blockIdx.x * s.per_block;
    const uint32_t hi = min(s.HW, lo + s.per_block);
    const int hs = 32 - 8 * pass, ds = 24 - 8 * pass;
    uint32_t n = 0, kk[2] = {0, 0}, M[MAX_SCALES] = {};
    // depth is locally smooth: a thread's consecutive keys mostly share a bin, so equal bins are counted in a register and
    // added to LDS when the bin changes (same-address LDS atomics of a whole wave serialise)
    uint32_t run_bin[2] = {0, 0}, run_n[2] = {0, 0};
    for (uint32_t i = lo + t; i < hi; i += TPB) {
      const bool valid = mask[base + i] != 0;
      if (valid && (has[0] || has[1])) {
        const float v[2] = {pred[base + i], targ[base + i]};
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          if (!has[a] || v[a] != v[a]) continue;
          const uint32_t key = f2key(v[a]);
          if (pass == 0) ++kk[a];
          if (pass == 0 || (key >> hs) == pre[a]) {
            const uint32_t bin = (key >> ds) & 255u;
            if (bin != run_bin[a]) {
              if (run_n[a]) atomicAdd(&lh[a][run_bin[a]], run_n[a]);
              run_bin[a] = bin;
              run_n[a] = 0;
            }
            ++run_n[a];
          }
        }
      }
      if (pass == 0 && valid) {
        ++n;
        const uint32_t y = i / (uint32_t)s.W, x = i - y * (uint32_t)s.W;
        const uint32_t yx = y | x;
#pragma unroll
        for (int k = 0; k < MAX_SCALES; ++k) {
          if (k >= s.scales || (yx & ((1u << k) - 1u)) != 0) break;
          ++M[k];
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
      if (run_n[a]) atomicAdd(&lh[a][run_bin[a]], run_n[a]);
    if (pass == 0) {
      if (n) atomicAdd(&lc[0], n);
      if (kk[0]) atomicAdd(&lc[1], kk[0]);
      if (kk[1]) atomicAdd(&lc[2], kk[1]);
#pragma unroll
      for (int k = 0; k < MAX_SCALES; ++k)
        if (M[k]) atomicAdd(&lc[4 + k], M[k]);
    }
    __syncthreads();
    uint32_t* gh = w.hist + ((int64_t)b * NPASS + pass) * 2 * BINS;
    if (has[0] && lh[0][t]) atomicAdd(&gh[t], lh[0][t]);
    if (has[1] && lh[1][t]) atomicAdd(&gh[BINS + t], lh[1][t]);
    if (pass == 0) {
      uint32_t* cnt = w.cnt + (int64_t)b * CNT;
      if (t < 3 && lc[t]) atomicAdd(&cnt[t], lc[t]);
      if (t == 3 && lc[0]) atomicAdd(&w.gcnt[0], (unsigned long long)lc[0]);
      if (t >= 4 && t < 4 + s.scales && lc[t]) {
        atomicAdd(&cnt[8 + t - 4], lc[t]);
        atomicAdd(&w.gcnt[1 + t - 4], (unsigned long long)lc[t]);
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- b. medians, argmedian, per-block sums
__global__ __launch_bounds__(TPB) void ml_stats_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                       const uint8_t* __restrict__ mask, Ws w, Shape s) {
  __shared__ uint32_t sc[2][BINS];
  __shared__ uint32_t res[4];
  __shared__ double red[4 * P_STATS];
  __shared__ uint32_t lmin;
  const int t = threadIdx.x;
  const bool ssi = s.terms & DPTX_MIDAS_SSI, align = s.terms & DPTX_MIDAS_ALIGN, inv = s.terms & DPTX_MIDAS_INVERSE;
  for (int b = blockIdx.y; b < s.B; b += gridDim.y) {
    bool has[2] = {false, false};
    uint32_t pre[2] = {0, 0}, rank[2] = {0, 0};
    if (ssi) select_state(w, b, NPASS, sc, res, has, pre, rank);
    const float tp = has[0] ? key2f(pre[0]) : 0.0f, tg = has[1] ? key2f(pre[1]) : 0.0f;  // nanmedian; NaN -> 0 (:42, :50)
    if (t == 0) lmin = 0xffffffffu;
    __syncthreads();
    const int64_t base = (int64_t)b * s.HW;
    const uint32_t lo = blockIdx.x * s.per_block;
    const uint32_t hi = min(s.HW, lo + s.per_block);
    double v[P_STATS] = {};
    uint32_t imin = 0xffffffffu;
    for (uint32_t i = lo + t; i < hi; i += TPB) {
      const bool valid = mask[base + i] != 0;
      const float p = pred[base + i], g = targ[base + i];
      if (ssi && valid) {
        const float up = p - tp;
        v[P_UP] += (double)fabsf(up);
        v[P_UG] += (double)fabsf(g - tg);
        v[P_SU] += (double)sgn(up);
        if (has[0] && p == p && f2key(p) == pre[0] && i < imin) imin = i;
      }
      if (align) {  // compute_scale_and_shift on the multiplicative mask (0 * NaN stays NaN, as there)
        const double mf = valid ? 1.0 : 0.0;
        const double x = (double)xform(p, inv), y = (double)xform(g, inv);
        const double mx = mf * x;
        v[P_A00] += mx * x;
        v[P_A01] += mx;
        v[P_B0] += mx * y;
        v[P_B1] += mf * y;
      }
    }
    if (ssi) {
      for (int o = 32; o > 0; o >>= 1) imin = min(imin, (uint32_t)__shfl_xor(imin, o, 64));
      if ((t & 63) == 0 && imin != 0xffffffffu) atomicMin(&lmin, imin);
    }
    block_sum<P_STATS>(v, red, w.part + ((int64_t)b * s.nblk + blockIdx.x) * NPART);
    if (t == 0 && lmin != 0xffffffffu) atomicMax(&w.cnt[(int64_t)b * CNT + 3], ~lmin);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- c. per-image solve (one wave per image)
__global__ __launch_bounds__(64) void ml_solve_kernel(Ws w, Shape s, int image_based, float* __restrict__ stats) {
  const int t = threadIdx.x;
  const bool ssi = s.terms & DPTX_MIDAS_SSI, align = s.terms & DPTX_MIDAS_ALIGN;
  for (int b = blockIdx.x; b < s.B; b += gridDim.x) {
    double v[P_STATS] = {};
    if (ssi || align)
      for (int j = t; j < s.nblk; j += 64) {
        const double* p = w.part + ((int64_t)b * s.nblk + j) * NPART;
#pragma unroll
        for (int q = 0; q < P_STATS; ++q) v[q] += p[q];
      }
#pragma unroll
    for (int q = 0; q < P_STATS; ++q) v[q] = wave_sum(v[q]);
    if (t == 0) {
      const uint32_t* cnt = w.cnt + (int64_t)b * CNT;
      double* r = w.rec + (int64_t)b * REC;
      const double n = (double)cnt[0];
      const float sp = (float)(v[P_UP] / (n + 1.0)), sg = (float)(v[P_UG] / (n + 1.0));  // :39, :45, :53 (the +1)
      r[R_SP] = sp;
      r[R_SG] = sg;
      r[R_DP] = sp + EPS;
      r[R_DG] = sg + EPS;
      r[R_N] = n;
      r[R_KP] = (double)cnt[1];
      r[R_MED] = cnt[3] ? (double)(~cnt[3]) : -1.0;
      r[R_SU] = v[P_SU];
      r[R_W - 1] = 0.0;
      // the medians (stats pass, block 0 recorded the keys); NaN -> 0 (:42, :50)
      const uint32_t* key = w.state + (int64_t)b * (NPASS + 1) * 4 + NPASS * 4;
      r[R_TP] = (ssi && cnt[1]) ? (double)key2f(key[0]) : 0.0;
      r[R_TG] = (ssi && cnt[2]) ? (double)key2f(key[2]) : 0.0;
      // :20-30 in fp64: det != 0 -> x = A^-1 b with det + 1e-6, rounded to fp32
      const double a00 = v[P_A00], a01 = v[P_A01], a11 = n, b0 = v[P_B0], b1 = v[P_B1];
      const double det = a00 * a11 - a01 * a01;
      const bool ok = align && det != 0.0;
      const float sc = ok ? (float)((a11 * b0 - a01 * b1) / (det + 1e-6)) : 0.0f;
      const float sh = ok ? (float)((-a01 * b0 + a00 * b1) / (det + 1e-6)) : 0.0f;
      r[R_SCALE] = sc;
      r[R_SHIFT] = sh;
      r[R_DETOK] = ok ? 1.0 : 0.0;
      r[R_A00] = a00;
      r[R_A01] = a01;
      r[R_B0] = b0;
      r[R_B1] = b1;
      // weights of L_k,b in reg: image-based (:71-79) 1 / (B M_k,b), batch-based (:59-68) 1 / sum_b M_k,b
      for (int k = 0; k < MAX_SCALES; ++k) {
        double wk = 0.0;
        if (k < s.scales) {
          const double m = image_based ? (double)cnt[8 + k] : (double)w.gcnt[1 + k];
          if (m > 0.0) wk = image_based ? 1.0 / ((double)s.B * m) : 1.0 / m;
        }
        r[R_W + k] = wk;
      }
      if (stats) {
        float* o = stats + (int64_t)b * DPTX_MIDAS_STATS;
        o[0] = (float)r[R_TP];
        o[1] = (float)r[R_TG];
        o[2] = sp;
        o[3] = sg;
        o[4] = (float)n;
        o[5] = sc;
        o[6] = sh;
        o[7] = (float)r[R_MED];
      }
    }
  }
}

struct Img {
  float tp, tg, dp, dg, scale, shift;
  bool inv, align;
};

__device__ __forceinline__ Img load_img(const double* r, int terms) {
  Img I;
  I.tp = (float)r[R_TP];
  I.tg = (float)r[R_TG];
  I.dp = (float)r[R_DP];
  I.dg = (float)r[R_DG];
  I.scale = (float)r[R_SCALE];
  I.shift = (float)r[R_SHIFT];
  I.inv = terms & DPTX_MIDAS_INVERSE;
  I.align = terms & DPTX_MIDAS_ALIGN;
  return I;
}

// d = m (r - t') of the gradient term at pixel j (:87-88, :152): r = scale x' + shift (or x'), x' = x or 1 / (x + 1e-6)
__device__ __forceinline__ float dval(const float* __restrict__ pred, const float* __restrict__ targ, const uint8_t* __restrict__ mask,
                                      int64_t j, const Img& I, bool& valid) {
  valid = mask[j] != 0;
  float x = xform(pred[j], I.inv);
  const float y = xform(targ[j], I.inv);
  if (I.align) x = I.scale * x + I.shift;
  return (valid ? 1.0f : 0.0f) * (x - y);
}

// G = d reg / d r at pixel (y, x) (0 unless valid): for every level it lies on, the signs of its pairs' differences
// weighted by the level's weight; forward: adds this pixel's right / down pairs to L[k]
template <bool FWD, bool BWD>
__device__ __forceinline__ double grad_term(const float* __restrict__ pred, const float* __restrict__ targ,
                                            const uint8_t* __restrict__ mask, int64_t base, uint32_t y, uint32_t x, const Shape& s,
                                            const Img& I, const double* wk, double* L) {
  const int64_t i = base + (int64_t)y * s.W + x;
  bool mi;
  const float di = dval(pred, targ, mask, i, I, mi);
  double G = 0.0;
  const uint32_t yx = y | x;
#pragma unroll
  for (int k = 0; k < MAX_SCALES; ++k) {
    if (k >= s.scales || (yx & ((1u << k) - 1u)) != 0) break;
    const uint32_t st = 1u << k;
    int c = 0;
    bool mj;
    if (x + st < (uint32_t)s.W) {
      const float dd = dval(pred, targ, mask, i + st, I, mj) - di;
      const bool mx = mi && mj;
      if (FWD) L[k] += (double)((mx ? 1.0f : 0.0f) * fabsf(dd));
      if (BWD && mx) c -= sgn(dd);
    }
    if (y + st < (uint32_t)s.H) {
      const float dd = dval(pred, targ, mask, i + (int64_t)st * s.W, I, mj) - di;
      const bool my = mi && mj;
      if (FWD) L[k] += (double)((my ? 1.0f : 0.0f) * fabsf(dd));
      if (BWD && my) c -= sgn(dd);
    }
    if (BWD && mi) {
      if (x >= st) {
        const float dd = di - dval(pred, targ, mask, i - st, I, mj);
        if (mj) c += sgn(dd);
      }
      if (y >= st) {
        const float dd = di - dval(pred, targ, mask, i - (int64_t)st * s.W, I, mj);
        if (mj) c += sgn(dd);
      }
      G += wk[k] * (double)c;
    }
  }
  return G;
}

// ---------------------------------------------------------------- d. loss pass
template <bool BWD>
__global__ __launch_bounds__(TPB) void ml_loss_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                      const uint8_t* __restrict__ mask, Ws w, Shape s) {
  constexpr int NS = P_L + MAX_SCALES;
  __shared__ double red[4 * NS];
  const bool ssi = s.terms & DPTX_MIDAS_SSI, grad = s.terms & DPTX_MIDAS_GRAD;
  for (int b = blockIdx.y; b < s.B; b += gridDim.y) {
    const double* r = w.rec + (int64_t)b * REC;
    const Img I = load_img(r, s.terms);
    double wk[MAX_SCALES];
#pragma unroll
    for (int k = 0; k < MAX_SCALES; ++k) wk[k] = r[R_W + k];
    const int64_t base = (int64_t)b * s.HW;
    const uint32_t lo = blockIdx.x * s.per_block;
    const uint32_t hi = min(s.HW, lo + s.per_block);
    double v[NS] = {};
    for (uint32_t i = lo + threadIdx.x; i < hi; i += TPB) {
      if (ssi && mask[base + i]) {  // :104-111 with masked_l1_loss
        const float p = pred[base + i], g = targ[base + i];
        const float up = p - I.tp;
        const float diff = up / I.dp - (g - I.tg) / I.dg;
        v[P_SSI] += (double)fabsf(diff);
        if (BWD) {
          const int e = sgn(diff);
          v[P_E] += (double)e;
          v[P_EU] += (double)e * (double)up;
        }
      }
      if (grad) {
        const uint32_t y = i / (uint32_t)s.W, x = i - y * (uint32_t)s.W;
        const double G = grad_term<true, BWD>(pred, targ, mask, base, y, x, s, I, wk, v + P_L);
        if (BWD && I.align) {
          v[P_S] += G * (double)xform(pred[base + i], I.inv);
          v[P_T] += G;
        }
      }
    }
    block_sum<NS>(v, red, w.part + ((int64_t)b * s.nblk + blockIdx.x) * NPART);
  }
}

// ---------------------------------------------------------------- e. per-image totals (one wave per image), finalize (one block)
__global__ __launch_bounds__(64) void ml_reduce_kernel(Ws w, Shape s) {
  constexpr int NS = P_L + MAX_SCALES;
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < s.B; b += gridDim.x) {
    double v[NS] = {};
    for (int j = t; j < s.nblk; j += 64) {
      const double* p = w.part + ((int64_t)b * s.nblk + j) * NPART;
#pragma unroll
      for (int q = 0; q < NS; ++q) v[q] += p[q];
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) v[q] = wave_sum(v[q]);
    if (t == 0)
#pragma unroll
      for (int q = 0; q < NS; ++q) w.tot[(int64_t)b * NPART + q] = v[q];
  }
}

__global__ __launch_bounds__(TPB) void ml_finalize_kernel(Ws w, Shape s, int image_based, float alpha, int want_grad,
                                                          float* __restrict__ losses, double* __restrict__ record) {
  __shared__ double sN;
  const int t = threadIdx.x;
  const bool ssi = s.terms & DPTX_MIDAS_SSI, grad = s.terms & DPTX_MIDAS_GRAD;
  if (t == 0) {
    const double N = (double)w.gcnt[0];
    double ssum = 0.0;
    for (int b = 0; b < s.B; ++b) ssum += w.tot[(int64_t)b * NPART + P_SSI];
    const double ssi_v = ssum / N;  // :7: NaN when the whole batch is masked
    double reg = 0.0;
    for (int k = 0; k < s.scales; ++k) {
      double acc = 0.0;
      if (image_based) {  // :71-79: images with M = 0 keep their (zero) sum
        for (int b = 0; b < s.B; ++b) {
          const double L = w.tot[(int64_t)b * NPART + P_L + k];
          const double M = (double)w.cnt[(int64_t)b * CNT + 8 + k];
          acc += M != 0.0 ? L / M : L;
        }
        acc /= (double)s.B;
      } else {  // :59-68
        for (int b = 0; b < s.B; ++b) acc += w.tot[(int64_t)b * NPART + P_L + k];
        const double M = (double)w.gcnt[1 + k];
        acc = M != 0.0 ? acc / M : 0.0;
      }
      reg += acc;
    }
    double total;
    if (ssi && grad) total = ssi_v + (double)alpha * reg;
    else total = ssi ? ssi_v : reg;
    losses[0] = (float)total;
    losses[1] = ssi ? (float)ssi_v : 0.0f;
    losses[2] = grad ? (float)reg : 0.0f;
    sN = N;
  }
  __syncthreads();
  if (!record) return;
  const double N = sN;
  for (int b = t; b < s.B; b += TPB) {
    double* r = w.rec + (int64_t)b * REC;
    const double* o = w.tot + (int64_t)b * NPART;
    if (want_grad) {
      // SSI (:33-56): d ssi / d p_j = [j valid] (kd e_j - ks sign(u_j)) + [j = argmedian] kmed
      const double D = r[R_DP], n = r[R_N];
      const double kd = (ssi && N > 0.0) ? 1.0 / (N * D) : 0.0;
      const double ks = (ssi && N > 0.0) ? o[P_EU] / (N * D * D * (n + 1.0)) : 0.0;
      r[R_KD] = kd;
      r[R_KS] = ks;
      r[R_KMED] = -o[P_E] * kd + r[R_SU] * ks;
      // alignment chain: d reg / d (a00, a01, b0) from S = sum G x', T = sum G
      double c00 = 0.0, c01 = 0.0, cb0 = 0.0;
      if (grad && r[R_DETOK] != 0.0) {
        const double a00 = r[R_A00], a01 = r[R_A01], a11 = n, b0 = r[R_B0], b1 = r[R_B1];
        const double Q = (a00 * a11 - a01 * a01) + 1e-6;
        const double X0 = (a11 * b0 - a01 * b1) / Q, X1 = (-a01 * b0 + a00 * b1) / Q;
        const double S = o[P_S], T = o[P_T];
        c00 = S * (-X0 * a11 / Q) + T * (b1 / Q - X1 * a11 / Q);
        c01 = S * ((2.0 * a01 * X0 - b1) / Q) + T * ((2.0 * a01 * X1 - b0) / Q);
        cb0 = S * (a11 / Q) + T * (-a01 / Q);
      }
      r[R_C00] = c00;
      r[R_C01] = c01;
      r[R_CB0] = cb0;
    }
    double* dst = record + (int64_t)b * REC;
    for (int q = 0; q < REC; ++q) dst[q] = r[q];
  }
}

// ---------------------------------------------------------------- f. backward
__global__ __launch_bounds__(TPB) void ml_backward_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                          const uint8_t* __restrict__ mask, Shape s, float alpha,
                                                          const double* __restrict__ record, const float* __restrict__ gl,
                                                          float* __restrict__ grad_pred) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  const bool ssi = s.terms & DPTX_MIDAS_SSI, grad = s.terms & DPTX_MIDAS_GRAD;
  const double g_total = gl[0], g_ssi = gl[1], g_reg = gl[2];
  const double w_ssi = ssi ? g_total + g_ssi : 0.0;
  const double w_reg = grad ? (ssi ? (double)alpha : 1.0) * g_total + g_reg : 0.0;
  if (i >= s.HW) return;
  const uint32_t y = i / (uint32_t)s.W, x = i - y * (uint32_t)s.W;
  for (int b = blockIdx.y; b < s.B; b += gridDim.y) {
    const double* r = record + (int64_t)b * REC;
    const Img I = load_img(r, s.terms);
    const int64_t base = (int64_t)b * s.HW;
    const bool valid = mask[base + i] != 0;
    const float p = pred[base + i];
    double gp = 0.0;
    if (ssi) {
      if (valid) {
        const float g = targ[base + i];
        const float up = p - I.tp;
        const float diff = up / I.dp - (g - I.tg) / I.dg;
        gp += w_ssi * (r[R_KD] * (double)sgn(diff) - r[R_KS] * (double)sgn(up));
      }
      if ((double)i == r[R_MED]) gp += w_ssi * r[R_KMED];
    }
    if (grad && valid) {
      double wk[MAX_SCALES];
#pragma unroll
      for (int k = 0; k < MAX_SCALES; ++k) wk[k] = r[R_W + k];
      double dr = grad_term<false, true>(pred, targ, mask, base, y, x, s, I, wk, nullptr);
      const double xp = (double)xform(p, I.inv);
      if (I.align) {
        dr *= (double)I.scale;
        if (r[R_DETOK] != 0.0) dr += 2.0 * xp * r[R_C00] + r[R_C01] + (double)xform(targ[base + i], I.inv) * r[R_CB0];
      }
      if (I.inv) dr *= -(xp * xp);  // d (1 / (p + 1e-6)) / dp = -pi^2
      gp += w_reg * dr;
    }
    grad_pred[base + i] = (float)gp;
  }
}

// aligned tensors of masked_shift_and_scale (:46, :54) at every pixel
__global__ __launch_bounds__(TPB) void ml_align_kernel(const float* __restrict__ pred, const float* __restrict__ targ, Ws w, Shape s,
                                                       float* __restrict__ pa, float* __restrict__ ga) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= s.HW) return;
  for (int b = blockIdx.y; b < s.B; b += gridDim.y) {
    const Img I = load_img(w.rec + (int64_t)b * REC, s.terms);
    const int64_t j = (int64_t)b * s.HW + i;
    if (pa) pa[j] = (pred[j] - I.tp) / I.dp;
    if (ga) ga[j] = (targ[j] - I.tg) / I.dg;
  }
}

bool shape_of(int32_t B, int32_t H, int32_t W, int32_t terms, int32_t scales, Layout& lo, Shape& s) {
  if (!layout(B, H, W, scales, lo) || (terms & ~ALL_TERMS)) return false;
  s = Shape{B, H, W, scales, terms, (int)lo.nblk, (uint32_t)((int64_t)H * W), (uint32_t)lo.per_block};
  return true;
}

// stages a..c on the workspace
bool run_stats(const float* pred, const float* targ, const uint8_t* mask, const Shape& s, const Layout& lo, const Ws& w,
               int image_based, float* stats, hipStream_t st) {
  const int gy = grid_y(s.B);
  if (hipMemsetAsync((char*)w.gcnt, 0, (size_t)lo.zero_bytes, st) != hipSuccess) return false;
  const dim3 grid((unsigned)s.nblk, (unsigned)gy);
  hipLaunchKernelGGL(ml_pass_kernel, grid, dim3(TPB), 0, st, pred, targ, mask, w, s, 0);
  if (s.terms & DPTX_MIDAS_SSI)
    for (int p = 1; p < NPASS; ++p) hipLaunchKernelGGL(ml_pass_kernel, grid, dim3(TPB), 0, st, pred, targ, mask, w, s, p);
  if (s.terms & (DPTX_MIDAS_SSI | DPTX_MIDAS_ALIGN))
    hipLaunchKernelGGL(ml_stats_kernel, grid, dim3(TPB), 0, st, pred, targ, mask, w, s);
  hipLaunchKernelGGL(ml_solve_kernel, dim3((unsigned)gy), dim3(64), 0, st, w, s, image_based, stats);
  return true;
}

}  // namespace

// midas_stats.h: stages a..c for the other units, the call dptx_midas_stats makes
namespace dptx {

bool midas_stats_workspace(int32_t B, int32_t H, int32_t W, int64_t* bytes) {
  Layout lo;
  if (!layout(B, H, W, 1, lo)) return false;
  *bytes = lo.total;
  return true;
}

bool midas_stats_launch(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t terms,
                        float* stats, void* ws, hipStream_t stream) {
  Layout lo;
  Shape s;
  if (!shape_of(B, H, W, terms, 1, lo, s)) return false;
  return run_stats(pred, target, mask, s, lo, ws_view(ws, lo), 1, stats, stream);
}

}  // namespace dptx

extern "C" {

int dptx_midas_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t scales, int64_t* bytes) {
  Layout lo;
  if (!bytes || !layout(B, H, W, scales, lo)) return DPTX_E_INVALID;
  *bytes = lo.total;
  return DPTX_OK;
}

int dptx_midas_loss(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t terms,
                    int32_t scales, int32_t image_based, float alpha, float* losses, double* record, void* ws, int64_t ws_bytes,
                    void* stream) {
  Layout lo;
  Shape s;
  if (!pred || !target || !mask || !losses || !ws || !shape_of(B, H, W, terms, scales, lo, s) || ws_bytes < lo.total ||
      !(terms & (DPTX_MIDAS_SSI | DPTX_MIDAS_GRAD)) ||
      ((terms & (DPTX_MIDAS_ALIGN | DPTX_MIDAS_INVERSE)) && !(terms & DPTX_MIDAS_GRAD)) || !(alpha > 0.0f))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const Ws w = ws_view(ws, lo);
  if (!run_stats(pred, target, mask, s, lo, w, image_based, nullptr, st)) return DPTX_E_HIP;
  const int gy = grid_y(B);
  const dim3 grid((unsigned)s.nblk, (unsigned)gy);
  if (record) hipLaunchKernelGGL(ml_loss_kernel<true>, grid, dim3(TPB), 0, st, pred, target, mask, w, s);
  else hipLaunchKernelGGL(ml_loss_kernel<false>, grid, dim3(TPB), 0, st, pred, target, mask, w, s);
  hipLaunchKernelGGL(ml_reduce_kernel, dim3((unsigned)gy), dim3(64), 0, st, w, s);
  hipLaunchKernelGGL(ml_finalize_kernel, dim3(1), dim3(TPB), 0, st, w, s, image_based, alpha, record ? 1 : 0, losses, record);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_midas_loss_backward(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W,
                             int32_t terms, int32_t scales, int32_t image_based, float alpha, const double* record,
                             const float* grad_losses, float* grad_pred, void* stream) {
  Layout lo;
  Shape s;
  (void)image_based;  // folded into the record's level weights
  if (!pred || !target || !mask || !record || !grad_losses || !grad_pred || !shape_of(B, H, W, terms, scales, lo, s) ||
      !(terms & (DPTX_MIDAS_SSI | DPTX_MIDAS_GRAD)) ||
      ((terms & (DPTX_MIDAS_ALIGN | DPTX_MIDAS_INVERSE)) && !(terms & DPTX_MIDAS_GRAD)) || !(alpha > 0.0f))
    return DPTX_E_INVALID;
  const int gy = grid_y(B);
  hipLaunchKernelGGL(ml_backward_kernel, dim3((s.HW + TPB - 1) / TPB, (unsigned)gy), dim3(TPB), 0, (hipStream_t)stream, pred, target,
                     mask, s, alpha, record, grad_losses, grad_pred);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_midas_stats(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t terms,
                     float* stats, float* pred_aligned, float* target_aligned, void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  Shape s;
  if (!pred || !target || !mask || !stats || !ws || !shape_of(B, H, W, terms & ~DPTX_MIDAS_GRAD, 1, lo, s) || ws_bytes < lo.total ||
      !(terms & (DPTX_MIDAS_SSI | DPTX_MIDAS_ALIGN)) || ((terms & DPTX_MIDAS_INVERSE) && !(terms & DPTX_MIDAS_ALIGN)) ||
      ((pred_aligned || target_aligned) && !(terms & DPTX_MIDAS_SSI)))
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const Ws w = ws_view(ws, lo);
  if (!run_stats(pred, target, mask, s, lo, w, 1, stats, st)) return DPTX_E_HIP;
  if (pred_aligned || target_aligned) {
    const int gy = grid_y(B);
    hipLaunchKernelGGL(ml_align_kernel, dim3((s.HW + TPB - 1) / TPB, (unsigned)gy), dim3(TPB), 0, st, pred, target, w, s,
                       pred_aligned, target_aligned);
  }
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
