// refocus.hip -- the 3D refocus augmentation of the reference (omnidata_tools/torch/data/refocus_augmentation.py), the
// depth-aware defocus blur of the Omnidata paper, as four stream-ordered stages on a caller-provided workspace (no
// allocation, no host synchronisation, no host read of the radii: graph-capturable).
//
//  a. exact quantiles (:82-88): a multi-rank radix select over order-preserving uint32 keys (select.h) of the depth, four 8-bit
//     digit passes, per-block LDS histograms merged with global atomics (integer counts only: deterministic), then ATen's
//     quantile arithmetic (rank = fp32(q * (N-1)), floor / ceil, lerp) so that the values are those of CPU torch.quantile.
//  b. tap tables per (image, level) (:31-57, :77-79, :104-114): radius, M, the normalised Gaussian weights for
//     |k| <= max(H, W) and the cumulative tail sums C[j] = sum_{i >= j} w_i (fp64, rounded once).  With the tails a
//     replicate padding of any width costs nothing: every tap that lands outside the image lands on an edge pixel, so the
//     taps beyond an edge are one weight on that pixel.  Per pixel at most min(M, 2 max(H, W) + 1) taps.
//  c. horizontal pass of every blurred level into the workspace H-stack [B][n+1][C][H][W]; levels with r < 0.1 or M = 1
//     are the image itself (flag in the table, stage d reads the input).
//  d. vertical pass fused with the composite (:90-101, :123-140): per 64-pixel wave the levels its pixels use (depth is
//     locally smooth: usually 2-3) are convolved with wave-uniform control flow and blended in registers; the vertical
//     stack is never built.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"
#include "select.h"

namespace {

using namespace dptx;

constexpr int QSLOTS = 64;                       // distinct key prefixes per select chunk (= ranks per chunk)
constexpr int QBINS = 256;                       // 8-bit digits, 4 passes
constexpr int64_t QHIST_BYTES = (int64_t)QSLOTS * QBINS * 4;  // per image
constexpr int64_t QSLOT_BYTES = 512;             // per image: nslot + QSLOTS sorted prefixes
constexpr int64_t Q_PX_PER_BLOCK = 4096, Q_MAX_BLOCKS = 1024;  // pixels per block of a digit pass (at least), blocks (at most)

struct Layout {
  int64_t q_bytes, t_bytes, h_bytes, total;
  int L, TS;  // table: longest side, floats per (image, level)
};

// include/dptx.h dptx_refocus_workspace_bytes documents these sizes
bool layout(int32_t B, int32_t C, int32_t H, int32_t W, int32_t n, Layout& lo) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || n < 1 || H > MAX_SIDE || W > MAX_SIDE || (int64_t)H * W > MAX_HW) return false;
  const double n1 = (double)n + 1.0;
  const double est = (double)B * n1 * ((double)C * H * W * 4.0 + 16.0 * (MAX_SIDE + 4) + 66048.0 + 24.0);
  if (est > 9.0e18) return false;  // int64 overflow of the sizes below
  lo.L = H > W ? H : W;
  lo.TS = 2 * lo.L + 8;
  const int64_t R = 2 * ((int64_t)n + 1);
  lo.q_bytes = align256((int64_t)B * (QHIST_BYTES + QSLOT_BYTES + 12 * R));
  lo.t_bytes = align256((int64_t)B * ((int64_t)n + 1) * lo.TS * 4);
  lo.h_bytes = (int64_t)B * ((int64_t)n + 1) * C * H * W * 4;
  lo.total = lo.q_bytes + lo.t_bytes + lo.h_bytes;
  return true;
}

// fp32 steps rounded one by one, as the reference's CPU arithmetic rounds them.  Plain operators under `fp contract(off)`:
// the IR carries no `contract` flag then, so no FMA can absorb them (the __f*_rn intrinsics do not prevent that -- hipcc
// fused rank - floor(rank) with the product before it into one FMA, and the weight of the lerp moved by an ulp).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;  // correctly rounded (hipcc's default fp32 division)
}

// ATen quantile_compute (linear): ranks = q * last_index in fp32, q = fp32(i) / fp32(n)
__device__ __forceinline__ float quantile_rank(int i, int n, uint32_t N) {
  return mul_rn(div_rn((float)i, (float)n), (float)(N - 1));
}

struct QRow {  // one image's part of the quantile workspace
  uint32_t* hist;   // [QSLOTS][QBINS]
  uint32_t* slots;  // [0] = nslot, [1 ..] sorted prefixes
  uint32_t* state;  // [R][2]: key prefix so far, rank left inside the prefix group
  float* sel;       // [R] selected order statistics
};
__device__ __forceinline__ QRow qrow(void* ws, int B, int R, int b) {
  char* base = (char*)ws;
  QRow q;
  q.hist = (uint32_t*)(base + (int64_t)b * QHIST_BYTES);
  q.slots = (uint32_t*)(base + (int64_t)B * QHIST_BYTES + (int64_t)b * QSLOT_BYTES);
  q.state = (uint32_t*)(base + (int64_t)B * (QHIST_BYTES + QSLOT_BYTES) + (int64_t)b * R * 8);
  q.sel = (float*)(base + (int64_t)B * (QHIST_BYTES + QSLOT_BYTES + 8 * R) + (int64_t)b * R * 4);
  return q;
}

// stage 0: start a chunk of m <= QSLOTS ranks (rank g = chunk0 + t: below (even g) / above (odd g) of quantile g / 2);
// stage s = 1..4: consume the histogram of digit pass s - 1.  One workgroup of 64 per image.
__global__ __launch_bounds__(64) void q_step_kernel(void* ws, int B, uint32_t N, int n, int R, int chunk0, int m, int stage) {
  __shared__ uint32_t newp[QSLOTS];
  __shared__ uint32_t sp[QSLOTS];
  __shared__ int ns;
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    QRow q = qrow(ws, B, R, b);
    if (stage == 0) {
      for (int i = t; i < QSLOTS * QBINS; i += 64) q.hist[i] = 0;
      if (t < m) {
        const int g = chunk0 + t;
        const float rk = quantile_rank(g >> 1, n, N);
        const uint32_t r = (g & 1) ? (uint32_t)ceilf(rk) : (uint32_t)rk;
        q.state[2 * g] = 0;
        q.state[2 * g + 1] = r;
      }
      if (t == 0) {
        q.slots[0] = 1;
        q.slots[1] = 0;
      }
      __syncthreads();
      continue;
    }
    if (t == 0) ns = (int)q.slots[0];
    if (t < QSLOTS) sp[t] = q.slots[1 + t];
    __syncthreads();
    if (t < m) {
      const int g = chunk0 + t;
      const uint32_t pre = q.state[2 * g];
      uint32_t kk = q.state[2 * g + 1];
      int j = 0;
      while (j < ns - 1 && sp[j] != pre) ++j;
      const uint32_t* h = q.hist + j * QBINS;
      uint32_t cum = 0, digit = QBINS - 1;
      for (int d = 0; d < QBINS; ++d) {
        const uint32_t c = h[d];
        if (kk < cum + c) { digit = d; break; }
        cum += c;
      }
      const uint32_t key = (pre << 8) | digit;
      q.state[2 * g] = key;
      q.state[2 * g + 1] = kk - cum;
      newp[t] = key;
      if (stage == 4) q.sel[g] = key2f(key);
    }
    __syncthreads();
    for (int i = t; i < ns * QBINS; i += 64) q.hist[i] = 0;
    if (stage < 4 && t == 0) {  // sorted distinct prefixes of the next pass (m <= 64: insertion sort)
      int k = 0;
      for (int i = 0; i < m; ++i) {
        const uint32_t v = newp[i];
        int p = 0;
        while (p < k && sp[p] < v) ++p;
        if (p < k && sp[p] == v) continue;
        for (int r = k; r > p; --r) sp[r] = sp[r - 1];
        sp[p] = v;
        ++k;
      }
      q.slots[0] = (uint32_t)k;
      for (int i = 0; i < k; ++i) q.slots[1 + i] = sp[i];
    }
    __syncthreads();
  }
}

// digit pass p (0..3): per-block LDS histogram of the keys whose prefix (bits above the digit) is one of the image's slots
__global__ __launch_bounds__(256) void q_hist_kernel(const float* __restrict__ depth, void* ws, int B, uint32_t N, int R, int pass,
                                                     uint32_t per_block) {
  __shared__ uint32_t lh[QSLOTS * QBINS];
  __shared__ uint32_t sp[QSLOTS];
  __shared__ int ns;
  const int t = threadIdx.x;
  const int shift = 24 - 8 * pass;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    QRow q = qrow(ws, B, R, b);
    if (t == 0) ns = (int)q.slots[0];
    if (t < QSLOTS) sp[t] = q.slots[1 + t];
    __syncthreads();
    const int nsl = ns;
    for (int i = t; i < nsl * QBINS; i += 256) lh[i] = 0;
    __syncthreads();
    const float* d = depth + (int64_t)b * N;
    const uint32_t lo = blockIdx.x * per_block;
    const uint32_t hi = min(N, lo + per_block);
    for (uint32_t i = lo + t; i < hi; i += 256) {
      const uint32_t key = f2key(d[i]);
      int j = 0;
      if (pass > 0) {
        const uint32_t pre = key >> (shift + 8);
        int a = 0, e = nsl;
        while (a < e) {
          const int mid = (a + e) >> 1;
          if (sp[mid] < pre) a = mid + 1; else e = mid;
        }
        j = (a < nsl && sp[a] == pre) ? a : -1;
      }
      if (j >= 0) atomicAdd(&lh[j * QBINS + ((key >> shift) & 255u)], 1u);
    }
    __syncthreads();
    for (int i = t; i < nsl * QBINS; i += 256) {
      const uint32_t v = lh[i];
      if (v) atomicAdd(&q.hist[i], v);
    }
    __syncthreads();
  }
}

// ATen lerp as the CPU build runs it (vectorised fmadd): w < 0.5 ? a + w (e - a) : e + (w - 1)(e - a), one rounding;
// then compute_quantiles' eps on the first and last quantile (:85-86)
__global__ __launch_bounds__(256) void q_final_kernel(void* ws, int B, uint32_t N, int n, int R, float eps, float* __restrict__ qvals) {
  const int n1 = n + 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * n1) return;
  const int b = (int)(idx / n1), i = (int)(idx - (int64_t)b * n1);
  const QRow q = qrow(ws, B, R, b);
  const float rk = quantile_rank(i, n, N);
  const float w = sub_rn(rk, (float)(uint32_t)rk);
  const float a = q.sel[2 * i], e = q.sel[2 * i + 1];
  const bool small = fabsf(w) < 0.5f;
  float v = fmaf(small ? w : sub_rn(w, 1.0f), sub_rn(e, a), small ? a : e);
  if (i == 0) v = sub_rn(v, eps);
  if (i == n) v = add_rn(v, eps);
  qvals[idx] = v;
}

// ---------------------------------------------------------------- tap tables
// per (image, level), TS = 2L + 8 floats: [0] radius, [1] M (int bits), [2] identity flag (int bits), [3] h = (M-1)/2
// (int bits), [4 .. 4+L] w_i / filsum for i = 0..L (0 beyond h), [5+L .. 6+2L] C_j / filsum for j = 0..L+1
__device__ __forceinline__ float gauss_tap(int i, float sig2) {
  const float fi = (float)i;
  return expf(-div_rn(mul_rn(fi, fi), sig2));  // gaussian(): exp(-n**2 / (2 std std)), n exact in fp32
}

__global__ __launch_bounds__(256) void tables_kernel(int B, int n1, int L, int TS, const float* __restrict__ qvals,
                                                     const float* __restrict__ focus, const float* __restrict__ aperture,
                                                     float* __restrict__ tables) {
  __shared__ double red[2][256];
  __shared__ double chunk_suffix[257];
  const int t = threadIdx.x;
  const int l = blockIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    float* tb = tables + ((int64_t)b * n1 + l) * TS;
    // compute_circle_of_confusion_no_magnification (:77-79): aperture * |q - focus| / q
    const float qv = qvals[(int64_t)b * n1 + l];
    const float r = div_rn(mul_rn(aperture[b], fabsf(sub_rn(qv, focus[b]))), qv);
    int M = 1;
    if (r >= 0.1f) {  // separable_gaussian (:34): r < 1e-1 returns the image; NaN is treated the same (the wrapper raises)
      float m3 = mul_rn(r, 3.0f);      // get_blur_stack_single_image (:107): int(r * cutoff_multiplier)
      if (m3 > 16777216.0f) m3 = 16777216.0f;  // results are defined for M <= 2^24 (the wrapper raises beyond)
      M = (int)m3;
      if ((M & 1) == 0) M += 1;
    }
    const int h = (M - 1) / 2;
    const int identity = M == 1;
    if (t == 0) {
      tb[0] = r;
      tb[1] = __int_as_float(M);
      tb[2] = __int_as_float(identity);
      tb[3] = __int_as_float(h);
    }
    if (identity) {
      __syncthreads();
      continue;
    }
    const float sig2 = mul_rn(mul_rn(2.0f, r), r);
    // all taps i >= 1 (filsum) and the tail beyond L
    double s_all = 0.0, s_tail = 0.0;
    for (int i = t + 1; i <= h; i += 256) {
      const double w = (double)gauss_tap(i, sig2);
      s_all += w;
      if (i > L) s_tail += w;
    }
    red[0][t] = s_all;
    red[1][t] = s_tail;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) {
        red[0][t] += red[0][t + s];
        red[1][t] += red[1][t + s];
      }
      __syncthreads();
    }
    const double filsum = 1.0 + 2.0 * red[0][0];  // w_0 = exp(0) = 1
    const double tail = red[1][0];
    // C_j = tail + sum_{j <= i <= min(h, L)} w_i: per-thread chunks of [0, L], a suffix over the chunk sums, then each chunk
    const int cs = (L + 1 + 255) / 256;
    const int j0 = t * cs, j1 = min(L + 1, j0 + cs);
    double cl = 0.0;
    for (int j = j0; j < j1; ++j)
      if (j <= h) cl += (double)gauss_tap(j, sig2);
    chunk_suffix[t] = cl;
    __syncthreads();
    if (t == 0) {
      double run = tail;
      chunk_suffix[256] = tail;
      for (int k = 255; k >= 0; --k) {
        run += chunk_suffix[k];
        chunk_suffix[k] = run;  // C at the first index of chunk k
      }
    }
    __syncthreads();
    float* wn = tb + 4;
    float* cn = tb + 5 + L;
    double run = chunk_suffix[t + 1];
    for (int j = j1 - 1; j >= j0; --j) {
      const double w = j <= h ? (double)gauss_tap(j, sig2) : 0.0;
      run += w;
      wn[j] = (float)(w / filsum);
      cn[j] = (float)(run / filsum);
    }
    if (t == 0) cn[L + 1] = (float)(tail / filsum);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- horizontal pass
// one workgroup per (image, channel, row): the row and the level's weights staged in LDS; clamp-to-edge through the tails
__global__ __launch_bounds__(256) void hpass_kernel(const float* __restrict__ rgb, int B, int C, int H, int W, int n1, int L, int TS,
                                                    const float* __restrict__ tables, float* __restrict__ hstack) {
  extern __shared__ float lds[];
  float* row = lds;      // [W]
  float* wl = lds + W;   // [W]: w_0 .. w_{W-1}
  const int t = threadIdx.x;
  const int y = blockIdx.x;
  for (int bc = blockIdx.y; bc < B * C; bc += gridDim.y) {
    const int b = bc / C, c = bc - b * C;
    const float* src = rgb + (((int64_t)b * C + c) * H + y) * W;
    __syncthreads();
    for (int x = t; x < W; x += 256) row[x] = src[x];
    for (int l = 0; l < n1; ++l) {
      const float* tb = tables + ((int64_t)b * n1 + l) * TS;
      if (__float_as_int(tb[2])) continue;  // identity level: stage d reads the input
      const int h = __float_as_int(tb[3]);
      const float* cn = tb + 5 + L;
      __syncthreads();
      for (int k = t; k < W; k += 256) wl[k] = tb[4 + k];
      __syncthreads();
      const int hh = min(h, W - 2);
      const int e = max(W - 1, 1);
      const float left = row[0], right = row[W - 1];
      float* dst = hstack + ((((int64_t)b * n1 + l) * C + c) * H + y) * W;
      for (int x = t; x < W; x += 256) {
        float acc = cn[x] * left + cn[e - x] * right;
        const int ja = max(1, x - hh), jb = min(W - 2, x + hh);
        for (int j = ja; j <= jb; ++j) acc += wl[abs(j - x)] * row[j];
        dst[x] = acc;
      }
    }
  }
}

// ---------------------------------------------------------------- vertical pass + composite
// workgroup 64 x 4: each wave is 64 consecutive pixels of one row; the levels it uses are the wave-uniform range
// [min left, max right]
__device__ __forceinline__ float vconv(const float* __restrict__ P, const float* __restrict__ tb, int L, int H, int W, int y, int x) {
  const int h = __float_as_int(tb[3]);
  const float* wv = tb + 4;
  const float* cn = tb + 5 + L;
  const int hh = min(h, H - 2);
  const int e = max(H - 1, 1);
  float acc = cn[y] * P[x] + cn[e - y] * P[(int64_t)(H - 1) * W + x];
  const int ja = max(1, y - hh), jb = min(H - 2, y + hh);
  for (int j = ja; j <= jb; ++j) acc += wv[abs(j - y)] * P[(int64_t)j * W + x];
  return acc;
}

__global__ __launch_bounds__(256) void vpass_kernel(const float* __restrict__ rgb, const float* __restrict__ depth, int B, int C, int H,
                                                    int W, int n, int L, int TS, const float* __restrict__ qvals,
                                                    const float* __restrict__ tables, const float* __restrict__ hstack,
                                                    float* __restrict__ out, int64_t* __restrict__ segments) {
  const int n1 = n + 1;
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * 4 + threadIdx.y;
  const bool valid = x < W && y < H;
  const int xc = min(x, W - 1), yc = min(y, H - 1);
  const int64_t HW = (int64_t)H * W;
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const float* q = qvals + (int64_t)b * n1;
    const float d = depth[(int64_t)b * HW + (int64_t)yc * W + xc];
    // compute_quantile_membership (:90-101): right = searchsorted(q, d) (first q >= d), left = right - 1
    int a = 0, e = n1;
    while (a < e) {
      const int mid = (a + e) >> 1;
      if (q[mid] < d) a = mid + 1; else e = mid;
    }
    const int right = min(max(a, 1), n);  // in range for every input the wrapper accepts; clamped so that no read strays
    const int left = right - 1;
    const float ql = q[left], qr = q[right];
    const float dist = sub_rn(qr, ql);
    const float dl = div_rn(sub_rn(d, ql), dist), dr = div_rn(sub_rn(qr, d), dist);
    // composite_blur_stack (:123-140): weights 1 - dist^2, normalised by their sum
    const float sl = sub_rn(1.0f, mul_rn(dl, dl)), sr = sub_rn(1.0f, mul_rn(dr, dr));
    const float s = add_rn(sl, sr);
    const float wl = div_rn(sl, s), wr = div_rn(sr, s);
    if (segments && valid) segments[(int64_t)b * HW + (int64_t)y * W + x] = left;
    int lo = valid ? left : n1, hi = valid ? right : -1;
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    for (int c = 0; c < C; ++c) {
      const int64_t pix = (((int64_t)b * C + c) * H + yc) * W + xc;
      float vl = 0.f, vr = 0.f;
      for (int lv = lo; lv <= hi; ++lv) {  // wave-uniform
        const float* tb = tables + ((int64_t)b * n1 + lv) * TS;
        float v;
        if (__float_as_int(tb[2])) {
          v = rgb[pix];
        } else {
          const float* P = hstack + (((int64_t)b * n1 + lv) * C + c) * HW;
          v = vconv(P, tb, L, H, W, yc, xc);
        }
        if (lv == left) vl = v;
        if (lv == right) vr = v;
      }
      if (valid) out[(((int64_t)b * C + c) * H + y) * W + x] = add_rn(mul_rn(wl, vl), mul_rn(wr, vr));
    }
  }
}

}  // namespace

extern "C" {

int dptx_refocus_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t n_quantiles, int64_t* bytes) {
  Layout lo;
  if (!bytes || !layout(B, C, H, W, n_quantiles, lo)) return DPTX_E_INVALID;
  *bytes = lo.total;
  return DPTX_OK;
}

int dptx_refocus_quantiles(const float* depth, int32_t B, int32_t H, int32_t W, int32_t n_quantiles, float* qvals, void* ws,
                           int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!depth || !qvals || !ws || !layout(B, 1, H, W, n_quantiles, lo) || ws_bytes < lo.q_bytes) return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t N = (uint32_t)H * (uint32_t)W;
  const int n = n_quantiles, R = 2 * (n + 1);
  const int gy = grid_y(B);
  int64_t nblk, per_block;
  split(N, Q_PX_PER_BLOCK, Q_MAX_BLOCKS, nblk, per_block);
  for (int chunk0 = 0; chunk0 < R; chunk0 += QSLOTS) {
    const int m = std::min(QSLOTS, R - chunk0);
    hipLaunchKernelGGL(q_step_kernel, dim3(gy), dim3(64), 0, st, ws, B, N, n, R, chunk0, m, 0);
    for (int p = 0; p < 4; ++p) {
      hipLaunchKernelGGL(q_hist_kernel, dim3((unsigned)nblk, gy), dim3(256), 0, st, depth, ws, B, N, R, p, (uint32_t)per_block);
      hipLaunchKernelGGL(q_step_kernel, dim3(gy), dim3(64), 0, st, ws, B, N, n, R, chunk0, m, p + 1);
    }
  }
  const int64_t tot = (int64_t)B * (n + 1);
  hipLaunchKernelGGL(q_final_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, ws, B, N, n, R, 1e-4f, qvals);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_refocus(const float* rgb, const float* depth, int32_t B, int32_t C, int32_t H, int32_t W, int32_t n_quantiles,
                 const float* qvals, const float* focus, const float* aperture, float* out, int64_t* segments, void* ws,
                 int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!rgb || !depth || !qvals || !focus || !aperture || !out || !ws || !layout(B, C, H, W, n_quantiles, lo) ||
      ws_bytes < lo.total)
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int n = n_quantiles, n1 = n + 1;
  float* tables = (float*)((char*)ws + lo.q_bytes);
  float* hstack = (float*)((char*)ws + lo.q_bytes + lo.t_bytes);
  const int64_t bc = (int64_t)B * C;
  if (bc > 0x7fffffff) return DPTX_E_INVALID;
  const int gb = grid_y(B);
  const int gbc = bc < MAX_GRID_Y ? (int)bc : MAX_GRID_Y;
  hipLaunchKernelGGL(tables_kernel, dim3(n1, gb), dim3(256), 0, st, B, n1, lo.L, lo.TS, qvals, focus, aperture, tables);
  hipLaunchKernelGGL(hpass_kernel, dim3(H, gbc), dim3(256), (size_t)2 * W * sizeof(float), st, rgb, B, C, H, W, n1, lo.L, lo.TS,
                     tables, hstack);
  hipLaunchKernelGGL(vpass_kernel, dim3((W + 63) / 64, (H + 3) / 4, gb), dim3(64, 4), 0, st, rgb, depth, B, C, H, W, n, lo.L,
                     lo.TS, qvals, tables, hstack, out, segments);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
