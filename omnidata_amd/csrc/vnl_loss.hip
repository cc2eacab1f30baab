// vnl_loss.hip -- the virtual normal loss of the reference (omnidata_tools/torch/losses/virtual_normal_loss.py, VNL_Loss) and
// its gradient with respect to either argument, as stream-ordered stages on a caller-provided workspace (no allocation, no
// host synchronisation, no host read of K or of the cut value).
//
//  a. triple pass, one thread per (image, triple): gathers the six depths, back-projects (:44-50), the mask of the FIRST
//     argument (:95-128 with the constants of the call at :136-140), the z == 0 replacement on the SECOND (:144), both unit
//     normals and the per-triple loss (:169-189), all in registers; writes keep [B][n] and loss [B][n]; counts K and
//     histograms the first 8-bit digit of the loss bits (losses are >= 0: the fp32 bit pattern is an order-preserving key).
//  b. cut (select only): passes 1..3 histogram the next digit under the prefix selected so far: the radix select of
//     select.h, over the whole batch.  The rank is int(K * 0.25) = K >> 2.  A tie pass counts, per block of the flat
//     (image, triple) order, the kept triples whose loss equals the cut value.
//  c. reduce: every block ranks its tied triples (exclusive sum of the tie counts of the blocks before it + a scan inside the
//     block), so that among kept triples at the cut value the EARLIEST in (image, triple) order are dropped first (the
//     stable sort's order); fp64 sum of the kept, not-dropped losses per block in a fixed order; finalize (one wave): the
//     total / (K - (K >> 2)) -> fp32 loss, and the record (K, rank, cut, per-triple "active" flags) for the backward.
//  p. prepare: the inverse index pixel -> the (triple, position) entries that use it, ascending: a stable LSD radix sort
//     (8-bit digits) of the 3n pixel indices with per-block digit counts, one scan block and a stable one-wave scatter.
//  d. backward, one thread per (image, pixel): walks the pixel's entries in that fixed order, recomputes each active
//     triple and adds the closed-form gradient of its depth at that position (fp64), times grad_out / (K - (K >> 2)).
// Numerics: forward in fp32, every step rounded on its own as the reference's fp32 tensors are (no contraction in this
// unit); fp64 for every sum and for the backward's chain rule (its exact-zero-norm decisions are the forward's fp32 ones).
// Integer atomics only: every floating-point sum runs in a fixed order, so results are bitwise reproducible and an
// image's per-triple outputs do not depend on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dptx.h"
#include "select.h"

#pragma clang fp contract(off)

namespace {

using namespace dptx;

constexpr int64_t MAX_TRIPLES = (1ll << 31) - 1;  // B * n
constexpr int MAX_N = 1 << 29;
constexpr int TPB = 256;
constexpr int64_t PER_BLOCK = 1024;     // triples per block of the flat passes (at least)
constexpr int64_t MAX_BLOCKS = 1024;
constexpr int64_t SORT_CHUNK = 1024;    // entries per sort block (at least)
constexpr int64_t SORT_MAX_BLOCKS = 512;
constexpr int HDR = DPTX_VNL_RECORD_HEADER;
constexpr float DELTA_COS = 0.867f, DELTA_DIFF = 0.005f;  // :136-140
constexpr float ENERGY_EPS = 1e-8f, ZERO_FILL = 0.0001f, NORM_FILL = 0.01f;

struct Layout {
  int64_t N, N3, nblk, per_block, snb, schunk;
  int spass;
  int64_t o_skey, o_sent, o_bh, sort_end, o_cnt, o_hist, zero_bytes, o_state, o_tie, o_part, o_loss, o_keep, total;
};

// include/dptx.h dptx_vnl_workspace_bytes documents these sizes
bool layout(int32_t B, int32_t H, int32_t W, int32_t n, Layout& lo) {
  if (B < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || (int64_t)H * W > MAX_HW || n < 1 || n > MAX_N ||
      (int64_t)B * n > MAX_TRIPLES)
    return false;
  const int64_t HW = (int64_t)H * W;
  lo.N = (int64_t)B * n;
  lo.N3 = 3 * (int64_t)n;
  split(lo.N, PER_BLOCK, MAX_BLOCKS, lo.nblk, lo.per_block);
  split(lo.N3, SORT_CHUNK, SORT_MAX_BLOCKS, lo.snb, lo.schunk);
  int bits = 0;  // keys are 0 .. HW (HW: an entry of a triple with an index out of range, sorted last)
  while ((HW >> bits) != 0) ++bits;
  lo.spass = (bits + 7) / 8;
  lo.o_skey = 0;                                            // uint32 [3n]
  lo.o_sent = lo.o_skey + align256(lo.N3 * 4);              // uint32 [3n]
  lo.o_bh = lo.o_sent + align256(lo.N3 * 4);                // uint32 [BINS][snb]
  lo.sort_end = lo.o_bh + align256(BINS * lo.snb * 4);
  lo.o_cnt = lo.sort_end;                                   // uint32 [64]: [0] K
  lo.o_hist = lo.o_cnt + 256;                               // uint32 [NPASS][BINS]
  lo.zero_bytes = 256 + NPASS * BINS * 4;
  lo.o_state = lo.o_hist + NPASS * BINS * 4;                // uint32 [NPASS + 1][2]
  lo.o_tie = lo.o_state + align256((NPASS + 1) * 8);        // uint32 [nblk]
  lo.o_part = lo.o_tie + align256(lo.nblk * 4);             // fp64 [nblk]
  lo.o_loss = lo.o_part + align256(lo.nblk * 8);            // fp32 [B][n]
  lo.o_keep = lo.o_loss + align256(lo.N * 4);               // uint8 [B][n]
  lo.total = lo.o_keep + align256(lo.N);
  return true;
}

struct Ws {
  uint32_t* skey;
  uint32_t* sent;
  uint32_t* bh;
  uint32_t* cnt;
  uint32_t* hist;
  uint32_t* state;
  uint32_t* tie;
  double* part;
  float* loss;
  uint8_t* keep;
};

Ws ws_view(void* ws, const Layout& lo) {
  char* b = (char*)ws;
  return Ws{(uint32_t*)(b + lo.o_skey), (uint32_t*)(b + lo.o_sent), (uint32_t*)(b + lo.o_bh), (uint32_t*)(b + lo.o_cnt),
            (uint32_t*)(b + lo.o_hist), (uint32_t*)(b + lo.o_state), (uint32_t*)(b + lo.o_tie), (double*)(b + lo.o_part),
            (float*)(b + lo.o_loss), (uint8_t*)(b + lo.o_keep)};
}

struct Geo {
  int B, H, W, n;
  uint32_t HW;
  float fx, fy, delta_z;
};

struct Idx {
  const int32_t* p[3];
};

// the record's header (include/dptx.h documents it)
struct Header {
  uint32_t K, rank, cut, tdrop;
  double sum, count;
  float loss;
};
static_assert(sizeof(Header) <= HDR, "record header");

// ---------------------------------------------------------------- the per-triple arithmetic (fp32, as the reference's tensors)
struct Pts {
  float c[3][3];  // [coordinate x, y, z][point]
};

// transfer_xyz (:44-50) at the three pixels of a triple
__device__ __forceinline__ Pts backproject(const float d[3], const float u[3], const float v[3], float fx, float fy) {
  Pts P;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float a = fabsf(d[j]);
    P.c[0][j] = (u[j] * a) / fx;
    P.c[1][j] = (v[j] * a) / fy;
    P.c[2][j] = d[j];
  }
  return P;
}

// filter_mask (:95-128) with delta_cos = 0.867 and delta_diff = 0.005
__device__ __forceinline__ bool keep_mask(const Pts& P, float delta_z) {
  float df[3][3];  // [coordinate][difference: P2 - P1, P3 - P1, P3 - P2]
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    df[c][0] = P.c[c][1] - P.c[c][0];
    df[c][1] = P.c[c][2] - P.c[c][0];
    df[c][2] = P.c[c][2] - P.c[c][1];
  }
  float q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = sqrtf((df[0][i] * df[0][i] + df[1][i] * df[1][i]) + df[2][i] * df[2][i]);
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {  // the matrix is symmetric
      const float en = (df[0][i] * df[0][j] + df[1][i] * df[1][j]) + df[2][i] * df[2][j];
      const float E = en / (q[i] * q[j] + ENERGY_EPS);
      const int hit = (E > DELTA_COS) || (E < -DELTA_COS);
      cnt += i == j ? hit : 2 * hit;
    }
  const bool collinear = cnt > 3;
  const bool pad = P.c[2][0] > delta_z && P.c[2][1] > delta_z && P.c[2][2] > delta_z;
  bool near[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    near[c] = fabsf(df[c][0]) < DELTA_DIFF || fabsf(df[c][1]) < DELTA_DIFF || fabsf(df[c][2]) < DELTA_DIFF;
  return pad && !((near[0] && near[1] && near[2]) || collinear);
}

// :144: where point j has z == 0, coordinate row j of all three points becomes 0.0001; ow[c]: row c was overwritten
__device__ __forceinline__ void zero_fill(Pts& P, bool ow[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) ow[j] = P.c[2][j] == 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (ow[c]) P.c[c][0] = P.c[c][1] = P.c[c][2] = ZERO_FILL;
}

// :169-187: cross(P2 - P1, P3 - P1) / its norm (0.01 where the norm is exactly 0); returns whether it was
__device__ __forceinline__ bool unit_normal(const Pts& P, float nh[3]) {
  float a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = P.c[c][1] - P.c[c][0];
    b[c] = P.c[c][2] - P.c[c][0];
  }
  const float N[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  float s = sqrtf((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
  const bool zero = s == 0.0f;
  if (zero) s = s + NORM_FILL;
#pragma unroll
  for (int c = 0; c < 3; ++c) nh[c] = N[c] / s;
  return zero;
}

// the pixel indices of triple i -> in range?; u - u0, v - v0 (exact in fp32)
__device__ __forceinline__ bool triple_pixels(const Idx& ix, const Geo& g, int i, uint32_t px[3], float u[3], float v[3]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int32_t p = ix.p[j][i];
    ok = ok && p >= 0 && (uint32_t)p < g.HW;
    px[j] = (uint32_t)p;
  }
  if (!ok) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint32_t y = px[j] / (uint32_t)g.W, x = px[j] - y * (uint32_t)g.W;
    u[j] = (float)((int)x - g.W / 2);
    v[j] = (float)((int)y - g.H / 2);
  }
  return true;
}

// ---------------------------------------------------------------- a. triple pass
__global__ __launch_bounds__(TPB) void vnl_triple_kernel(const float* __restrict__ first, const float* __restrict__ second, Geo g,
                                                         Idx ix, uint8_t* __restrict__ keep_out, float* __restrict__ loss_out,
                                                         float* __restrict__ normals /*nullable*/, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ hist /*both nullable*/) {
  __shared__ uint32_t lh[BINS];
  __shared__ uint32_t lk;
  const int t = threadIdx.x;
  const int i = blockIdx.x * TPB + t;
  lh[t] = 0;
  if (t == 0) lk = 0;
  __syncthreads();
  uint32_t px[3] = {0, 0, 0};
  float u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
  const bool in = i < g.n;
  const bool ok = in && triple_pixels(ix, g, i, px, u, v);
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    bool keep = false;
    float loss = 0.0f, ng[3] = {0, 0, 0}, nd[3] = {0, 0, 0};
    if (ok) {
      const int64_t base = (int64_t)b * g.HW;
      const float d1[3] = {first[base + px[0]], first[base + px[1]], first[base + px[2]]};
      const float d2[3] = {second[base + px[0]], second[base + px[1]], second[base + px[2]]};
      const Pts P = backproject(d1, u, v, g.fx, g.fy);
      Pts Q = backproject(d2, u, v, g.fx, g.fy);
      keep = keep_mask(P, g.delta_z);
      bool ow[3];
      zero_fill(Q, ow);
      unit_normal(P, ng);
      unit_normal(Q, nd);
      loss = (fabsf(ng[0] - nd[0]) + fabsf(ng[1] - nd[1])) + fabsf(ng[2] - nd[2]);
    }
    if (in) {
      const int64_t o = (int64_t)b * g.n + i;
      keep_out[o] = keep ? 1 : 0;
      loss_out[o] = keep ? loss : 0.0f;
      if (normals) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          normals[o * 6 + c] = ng[c];
          normals[o * 6 + 3 + c] = nd[c];
        }
      }
    }
    if (hist && keep) {
      atomicAdd(&lk, 1u);
      atomicAdd(&lh[(__float_as_uint(loss) & 0x7fffffffu) >> 24], 1u);
    }
  }
  if (!hist) return;
  __syncthreads();
  if (lh[t]) atomicAdd(&hist[t], lh[t]);
  if (t == 0 && lk) atomicAdd(&cnt[0], lk);
}

// ---------------------------------------------------------------- b. radix select of rank K >> 2 among the kept losses
// the select state before pass q (select.h).  After the last pass: pre = the bits of the cut value, rank = how many of the
// kept triples AT the cut value are dropped.
__device__ __forceinline__ void select_state(const Ws& w, int q, uint32_t (*sc)[BINS], uint32_t* res, uint32_t& pre, uint32_t& rank) {
  const uint32_t K = w.cnt[0];
  const bool has[1] = {K > 0};
  const uint32_t rank0[1] = {K >> 2};  // int(K * 0.25)
  uint32_t p[1], r[1];
  dptx::select_state<1>(w.hist, w.state, q, sc, res, has, rank0, p, r);
  pre = p[0];
  rank = r[0];
}

__global__ __launch_bounds__(TPB) void vnl_pass_kernel(Ws w, uint32_t N, uint32_t per_block, int pass) {
  __shared__ uint32_t lh[BINS];
  __shared__ uint32_t sc[1][BINS];
  __shared__ uint32_t res[2];
  const int t = threadIdx.x;
  uint32_t pre, rank;
  select_state(w, pass, sc, res, pre, rank);
  lh[t] = 0;
  __syncthreads();
  const uint32_t lo = blockIdx.x * per_block, hi = min(N, lo + per_block);
  const int hs = 32 - 8 * pass, ds = 24 - 8 * pass;
  for (uint32_t i = lo + t; i < hi; i += TPB) {
    if (!w.keep[i]) continue;
    const uint32_t key = __float_as_uint(w.loss[i]) & 0x7fffffffu;
    if ((key >> hs) == pre) atomicAdd(&lh[(key >> ds) & 255u], 1u);
  }
  __syncthreads();
  if (lh[t]) atomicAdd(&w.hist[pass * BINS + t], lh[t]);
}

// the cut of this call: with select, the state after the last pass; without, nothing is dropped
__device__ void final_state(const Ws& w, int select, uint32_t (*sc)[BINS], uint32_t* res, uint32_t& cut, uint32_t& tdrop) {
  cut = 0;
  tdrop = 0;
  if (select) select_state(w, NPASS, sc, res, cut, tdrop);
}

// kept triples of this block's range whose loss equals the cut value
__global__ __launch_bounds__(TPB) void vnl_tie_kernel(Ws w, uint32_t N, uint32_t per_block, int select) {
  __shared__ uint32_t sc[1][BINS];
  __shared__ uint32_t res[2];
  __shared__ uint32_t lt;
  const int t = threadIdx.x;
  uint32_t cut, tdrop;
  final_state(w, select, sc, res, cut, tdrop);
  if (t == 0) lt = 0;
  __syncthreads();
  const uint32_t lo = blockIdx.x * per_block, hi = min(N, lo + per_block);
  uint32_t c = 0;
  for (uint32_t i = lo + t; i < hi; i += TPB)
    c += (w.keep[i] && (__float_as_uint(w.loss[i]) & 0x7fffffffu) == cut) ? 1u : 0u;
  if (c) atomicAdd(&lt, c);
  __syncthreads();
  if (t == 0) w.tie[blockIdx.x] = lt;
}

// ---------------------------------------------------------------- c. reduce
__global__ __launch_bounds__(TPB) void vnl_reduce_kernel(Ws w, uint32_t N, uint32_t per_block, int select,
                                                         uint8_t* __restrict__ active /*nullable*/) {
  __shared__ uint32_t sc[1][BINS];
  __shared__ uint32_t res[2];
  __shared__ uint32_t lbase;
  __shared__ uint32_t wsum[4];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t cut, tdrop;
  final_state(w, select, sc, res, cut, tdrop);
  if (t == 0) lbase = 0;
  __syncthreads();
  uint32_t c = 0;  // ties in the blocks before this one
  for (uint32_t j = t; j < blockIdx.x; j += TPB) c += w.tie[j];
  if (c) atomicAdd(&lbase, c);
  __syncthreads();
  uint32_t run = lbase;
  const uint32_t lo = blockIdx.x * per_block, hi = min(N, lo + per_block);
  double v[1] = {0.0};
  for (uint32_t tile = lo; tile < hi; tile += TPB) {  // uniform trip count: the block scans every tile together
    const uint32_t i = tile + t;
    const bool in = i < hi;
    const bool kept = in && w.keep[i] != 0;
    const float loss = in ? w.loss[i] : 0.0f;
    const uint32_t key = __float_as_uint(loss) & 0x7fffffffu;
    const bool tie = kept && key == cut;
    const unsigned long long bal = __ballot(tie);
    const uint32_t wrank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      before += k < wave ? wsum[k] : 0u;
      all += wsum[k];
    }
    const bool act = kept && (key > cut || (tie && run + before + wrank >= tdrop));
    run += all;
    __syncthreads();
    if (act) v[0] += (double)loss;
    if (active && in) active[i] = act ? 1 : 0;
  }
  block_sum<1>(v, red, w.part + blockIdx.x);
}

__global__ __launch_bounds__(64) void vnl_finalize_kernel(Ws w, int nblk, int select, float* __restrict__ loss_out,
                                                          uint8_t* __restrict__ record /*nullable*/) {
  const int t = threadIdx.x;
  double v = 0.0;
  for (int j = t; j < nblk; j += 64) v += w.part[j];
  v = wave_sum(v);
  if (t != 0) return;
  const uint32_t K = w.cnt[0];
  const uint32_t rank = select ? (K >> 2) : 0u;
  const double count = (double)(K - rank);
  const float loss = (float)(v / count);  // K = 0: 0 / 0 = NaN, the mean of nothing (:193)
  loss_out[0] = loss;
  if (record) {
    Header h;
    h.K = K;
    h.rank = rank;
    h.cut = select ? w.state[NPASS * 2] : 0u;
    h.tdrop = select ? w.state[NPASS * 2 + 1] : 0u;
    h.sum = v;
    h.count = count;
    h.loss = loss;
    *(Header*)record = h;
  }
}

// ---------------------------------------------------------------- p. inverse index: stable LSD radix sort of the 3n pixel indices
// entry e = 3 i + position; key = its pixel, or HW for every entry of a triple with an index out of range
__global__ __launch_bounds__(TPB) void vnl_sort_init_kernel(Idx ix, int n, uint32_t HW, uint32_t* __restrict__ key,
                                                            uint32_t* __restrict__ ent) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int32_t p[3] = {ix.p[0][i], ix.p[1][i], ix.p[2][i]};
  const bool ok = p[0] >= 0 && (uint32_t)p[0] < HW && p[1] >= 0 && (uint32_t)p[1] < HW && p[2] >= 0 && (uint32_t)p[2] < HW;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    key[3 * (int64_t)i + j] = ok ? (uint32_t)p[j] : HW;
    ent[3 * (int64_t)i + j] = 3u * (uint32_t)i + (uint32_t)j;
  }
}

// digit counts of this block's chunk -> bh[digit][block]
__global__ __launch_bounds__(64) void vnl_sort_count_kernel(const uint32_t* __restrict__ key, uint32_t N3, uint32_t chunk, int shift,
                                                            uint32_t* __restrict__ bh) {
  __shared__ uint32_t lh[BINS];
  const int t = threadIdx.x;
  for (int d = t; d < BINS; d += 64) lh[d] = 0;
  __syncthreads();
  const uint32_t lo = blockIdx.x * chunk, hi = min(N3, lo + chunk);
  for (uint32_t j = lo + t; j < hi; j += 64) atomicAdd(&lh[(key[j] >> shift) & 255u], 1u);
  __syncthreads();
  for (int d = t; d < BINS; d += 64) bh[(uint32_t)d * gridDim.x + blockIdx.x] = lh[d];
}

// exclusive scan of bh in (digit, block) order, in place (one block; thread d owns digit d)
__global__ __launch_bounds__(BINS) void vnl_sort_scan_kernel(uint32_t* __restrict__ bh, int snb) {
  __shared__ uint32_t sc[1][BINS];
  const int t = threadIdx.x;
  uint32_t* row = bh + (int64_t)t * snb;
  uint32_t tot = 0;
  for (int j = 0; j < snb; ++j) tot += row[j];
  sc[0][t] = tot;
  block_scan256<1>(sc);
  uint32_t run = sc[0][t] - tot;
  for (int j = 0; j < snb; ++j) {
    const uint32_t c = row[j];
    row[j] = run;
    run += c;
  }
}

// stable scatter: one wave per chunk, 64 entries at a time in order; lanes with the same digit rank themselves by ballots
__global__ __launch_bounds__(64) void vnl_sort_scatter_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ ent,
                                                              uint32_t N3, uint32_t chunk, int shift,
                                                              const uint32_t* __restrict__ bh, uint32_t* __restrict__ key_out,
                                                              uint32_t* __restrict__ ent_out) {
  __shared__ uint32_t off[BINS];
  const int t = threadIdx.x;
  for (int d = t; d < BINS; d += 64) off[d] = bh[(uint32_t)d * gridDim.x + blockIdx.x];
  __syncthreads();
  const uint32_t lo = blockIdx.x * chunk, hi = min(N3, lo + chunk);
  for (uint32_t tile = lo; tile < hi; tile += 64) {
    const uint32_t j = tile + t;
    const bool in = j < hi;
    const uint32_t k = in ? key[j] : 0u, e = in ? ent[j] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    unsigned long long peers = __ballot(in);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const unsigned long long bal = __ballot(in && one);
      peers &= one ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << t) - 1ull));
    const uint32_t slot = in ? off[d] + rank : 0u;
    __syncthreads();
    if (in && (peers >> t) == 1ull) off[d] = slot + 1;  // the last lane of the digit's peers
    __syncthreads();
    if (in && slot < N3) {
      key_out[slot] = k;
      ent_out[slot] = e;
    }
  }
}

// first[pixel] = 1 + the slot of its first entry (0: no triple uses the pixel)
__global__ __launch_bounds__(TPB) void vnl_first_kernel(const uint32_t* __restrict__ skey, uint32_t N3, uint32_t HW,
                                                        uint32_t* __restrict__ first) {
  const uint32_t j = blockIdx.x * TPB + threadIdx.x;
  if (j >= N3) return;
  const uint32_t k = skey[j];
  if (k < HW && (j == 0 || skey[j - 1] != k)) first[k] = j + 1;
}

// ---------------------------------------------------------------- d. backward
struct Pts64 {
  double c[3][3];
};

__device__ __forceinline__ Pts64 backproject64(const float d[3], const float u[3], const float v[3], double fx, double fy) {
  Pts64 P;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double a = fabs((double)d[j]);
    P.c[0][j] = ((double)u[j] * a) / fx;
    P.c[1][j] = ((double)v[j] * a) / fy;
    P.c[2][j] = (double)d[j];
  }
  return P;
}

struct Normal64 {
  double a[3], b[3], nh[3], s;
};

__device__ __forceinline__ Normal64 unit_normal64(const Pts64& P, bool zero) {
  Normal64 r;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    r.a[c] = P.c[c][1] - P.c[c][0];
    r.b[c] = P.c[c][2] - P.c[c][0];
  }
  const double N[3] = {r.a[1] * r.b[2] - r.a[2] * r.b[1], r.a[2] * r.b[0] - r.a[0] * r.b[2], r.a[0] * r.b[1] - r.a[1] * r.b[0]};
  const double s = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
  r.s = zero ? s + (double)NORM_FILL : s;
#pragma unroll
  for (int c = 0; c < 3; ++c) r.nh[c] = N[c] / r.s;
  return r;
}

__device__ __forceinline__ double sgn64(double v) { return (double)((v > 0.0) - (v < 0.0)); }

// d loss / d depth at position `pos` of one argument: wv = d loss / d (its unit normal) -> through n / |n| (no gradient
// through the norm where it was replaced), the cross product, and dP/dd; ow: coordinate rows overwritten by :144
__device__ __forceinline__ double depth_grad(const Normal64& m, bool zero, const double wv[3], int pos, float d, float u, float v,
                                             double fx, double fy, const bool ow[3]) {
  double G[3];
  const double dot = zero ? 0.0 : (m.nh[0] * wv[0] + m.nh[1] * wv[1]) + m.nh[2] * wv[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) G[c] = (wv[c] - m.nh[c] * dot) / m.s;
  // N = a x b: dL/da = b x G, dL/db = G x a; P1 takes -(da + db), P2 da, P3 db
  const double da[3] = {m.b[1] * G[2] - m.b[2] * G[1], m.b[2] * G[0] - m.b[0] * G[2], m.b[0] * G[1] - m.b[1] * G[0]};
  const double db[3] = {G[1] * m.a[2] - G[2] * m.a[1], G[2] * m.a[0] - G[0] * m.a[2], G[0] * m.a[1] - G[1] * m.a[0]};
  double gp[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gp[c] = pos == 0 ? -(da[c] + db[c]) : (pos == 1 ? da[c] : db[c]);
    if (ow[c]) gp[c] = 0.0;
  }
  const double sd = sgn64((double)d);
  return (gp[0] * ((double)u * sd / fx) + gp[1] * ((double)v * sd / fy)) + gp[2];
}

__global__ __launch_bounds__(TPB) void vnl_backward_kernel(const float* __restrict__ first, const float* __restrict__ second, Geo g,
                                                           Idx ix, const uint8_t* __restrict__ record,
                                                           const uint32_t* __restrict__ inverse, const float* __restrict__ grad_out,
                                                           float* __restrict__ grad_first, float* __restrict__ grad_second) {
  const uint32_t pix = blockIdx.x * TPB + threadIdx.x;
  if (pix >= g.HW) return;
  const uint32_t N3 = 3u * (uint32_t)g.n;
  const uint32_t* skey = inverse + g.HW;
  const uint32_t* sent = skey + N3;
  const uint8_t* active = record + HDR;
  const Header* h = (const Header*)record;
  const double scale = h->count > 0.0 ? (double)grad_out[0] / h->count : 0.0;
  const double fx = (double)g.fx, fy = (double)g.fy;
  const uint32_t f = inverse[pix];
  const bool none[3] = {false, false, false};
  for (int b = blockIdx.y; b < g.B; b += gridDim.y) {
    const int64_t base = (int64_t)b * g.HW;
    double acc1 = 0.0, acc2 = 0.0;
    if (f != 0)
      for (uint32_t j = f - 1; j < N3 && skey[j] == pix; ++j) {
        const uint32_t e = sent[j];
        const int i = (int)(e / 3u), pos = (int)(e - 3u * (uint32_t)i);
        if (i >= g.n || !active[(int64_t)b * g.n + i]) continue;
        uint32_t px[3];
        float u[3], v[3];
        if (!triple_pixels(ix, g, i, px, u, v)) continue;  // never: such a triple is not kept
        const float d1[3] = {first[base + px[0]], first[base + px[1]], first[base + px[2]]};
        const float d2[3] = {second[base + px[0]], second[base + px[1]], second[base + px[2]]};
        // the forward's fp32 decisions: rows overwritten in the second argument, norms that were exactly 0
        const Pts P32 = backproject(d1, u, v, g.fx, g.fy);
        Pts Q32 = backproject(d2, u, v, g.fx, g.fy);
        bool ow[3];
        zero_fill(Q32, ow);
        float tmp[3];
        const bool z1 = unit_normal(P32, tmp), z2 = unit_normal(Q32, tmp);
        const Pts64 P = backproject64(d1, u, v, fx, fy);
        Pts64 Q = backproject64(d2, u, v, fx, fy);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (ow[c]) Q.c[c][0] = Q.c[c][1] = Q.c[c][2] = (double)ZERO_FILL;
        const Normal64 ng = unit_normal64(P, z1), nd = unit_normal64(Q, z2);
        double wg[3], wd[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          wg[c] = sgn64(ng.nh[c] - nd.nh[c]);
          wd[c] = -wg[c];
        }
        const float dg = pos == 0 ? d1[0] : (pos == 1 ? d1[1] : d1[2]);
        const float dd = pos == 0 ? d2[0] : (pos == 1 ? d2[1] : d2[2]);
        const float uu = pos == 0 ? u[0] : (pos == 1 ? u[1] : u[2]);
        const float vv = pos == 0 ? v[0] : (pos == 1 ? v[1] : v[2]);
        if (grad_first) acc1 += depth_grad(ng, z1, wg, pos, dg, uu, vv, fx, fy, none);
        if (grad_second) acc2 += depth_grad(nd, z2, wd, pos, dd, uu, vv, fx, fy, ow);
      }
    if (grad_first) grad_first[base + pix] = (float)(acc1 * scale);
    if (grad_second) grad_second[base + pix] = (float)(acc2 * scale);
  }
}

Geo geo(int32_t B, int32_t H, int32_t W, int32_t n, float fx, float fy, float delta_z) {
  return Geo{B, H, W, n, (uint32_t)((int64_t)H * W), fx, fy, delta_z};
}

}  // namespace

extern "C" {

int dptx_vnl_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n, int64_t* bytes) {
  Layout lo;
  if (!bytes || !layout(B, H, W, n, lo)) return DPTX_E_INVALID;
  *bytes = lo.total;
  return DPTX_OK;
}

int dptx_vnl_prepare(const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, int32_t H, int32_t W, uint32_t* inverse,
                     void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!p1 || !p2 || !p3 || !inverse || !ws || !layout(1, H, W, n, lo) || ws_bytes < lo.sort_end) return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const Ws w = ws_view(ws, lo);
  const uint32_t HW = (uint32_t)((int64_t)H * W), N3 = (uint32_t)lo.N3;
  uint32_t* first = inverse;
  uint32_t* key[2] = {w.skey, inverse + HW};
  uint32_t* ent[2] = {w.sent, inverse + HW + N3};
  int cur = (lo.spass & 1) ? 0 : 1;  // the last pass lands in `inverse`
  if (hipMemsetAsync(first, 0, (size_t)HW * 4, st) != hipSuccess) return DPTX_E_HIP;
  hipLaunchKernelGGL(vnl_sort_init_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, Idx{{p1, p2, p3}}, n, HW, key[cur],
                     ent[cur]);
  for (int p = 0; p < lo.spass; ++p, cur ^= 1) {
    const int shift = 8 * p;
    hipLaunchKernelGGL(vnl_sort_count_kernel, dim3((unsigned)lo.snb), dim3(64), 0, st, key[cur], N3, (uint32_t)lo.schunk, shift, w.bh);
    hipLaunchKernelGGL(vnl_sort_scan_kernel, dim3(1), dim3(BINS), 0, st, w.bh, (int)lo.snb);
    hipLaunchKernelGGL(vnl_sort_scatter_kernel, dim3((unsigned)lo.snb), dim3(64), 0, st, key[cur], ent[cur], N3, (uint32_t)lo.schunk,
                       shift, w.bh, key[cur ^ 1], ent[cur ^ 1]);
  }
  hipLaunchKernelGGL(vnl_first_kernel, dim3((N3 + TPB - 1) / TPB), dim3(TPB), 0, st, key[1], N3, HW, first);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_vnl_loss(const float* first, const float* second, int32_t B, int32_t H, int32_t W, float fx, float fy, float delta_z,
                  const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, int32_t select, float* loss_out,
                  uint8_t* record, void* ws, int64_t ws_bytes, void* stream) {
  Layout lo;
  if (!first || !second || !p1 || !p2 || !p3 || !loss_out || !ws || !layout(B, H, W, n, lo) || ws_bytes < lo.total)
    return DPTX_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const Ws w = ws_view(ws, lo);
  const Geo g = geo(B, H, W, n, fx, fy, delta_z);
  const uint32_t N = (uint32_t)lo.N, per = (uint32_t)lo.per_block;
  const int sel = select ? 1 : 0;
  if (hipMemsetAsync(w.cnt, 0, (size_t)lo.zero_bytes, st) != hipSuccess) return DPTX_E_HIP;
  hipLaunchKernelGGL(vnl_triple_kernel, dim3((unsigned)((n + TPB - 1) / TPB), (unsigned)grid_y(B)), dim3(TPB), 0, st, first,
                     second, g, Idx{{p1, p2, p3}}, w.keep, w.loss, (float*)nullptr, w.cnt, w.hist);
  const dim3 grid((unsigned)lo.nblk);
  if (sel)
    for (int p = 1; p < NPASS; ++p) hipLaunchKernelGGL(vnl_pass_kernel, grid, dim3(TPB), 0, st, w, N, per, p);
  hipLaunchKernelGGL(vnl_tie_kernel, grid, dim3(TPB), 0, st, w, N, per, sel);
  hipLaunchKernelGGL(vnl_reduce_kernel, grid, dim3(TPB), 0, st, w, N, per, sel, record ? record + HDR : (uint8_t*)nullptr);
  hipLaunchKernelGGL(vnl_finalize_kernel, dim3(1), dim3(64), 0, st, w, (int)lo.nblk, sel, loss_out, record);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_vnl_loss_backward(const float* first, const float* second, int32_t B, int32_t H, int32_t W, float fx, float fy,
                           const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, const uint8_t* record,
                           const uint32_t* inverse, const float* grad_out, float* grad_first, float* grad_second, void* stream) {
  Layout lo;
  if (!first || !second || !p1 || !p2 || !p3 || !record || !inverse || !grad_out || (!grad_first && !grad_second) ||
      !layout(B, H, W, n, lo))
    return DPTX_E_INVALID;
  const Geo g = geo(B, H, W, n, fx, fy, 0.0f);
  hipLaunchKernelGGL(vnl_backward_kernel, dim3((g.HW + TPB - 1) / TPB, (unsigned)grid_y(B)), dim3(TPB), 0,
                     (hipStream_t)stream, first, second, g, Idx{{p1, p2, p3}}, record, inverse, grad_out, grad_first, grad_second);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

int dptx_vnl_triples(const float* first, const float* second, int32_t B, int32_t H, int32_t W, float fx, float fy, float delta_z,
                     const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, uint8_t* keep, float* loss, float* normals,
                     void* stream) {
  Layout lo;
  if (!first || !second || !p1 || !p2 || !p3 || !keep || !loss || !layout(B, H, W, n, lo)) return DPTX_E_INVALID;
  hipLaunchKernelGGL(vnl_triple_kernel, dim3((unsigned)((n + TPB - 1) / TPB), (unsigned)grid_y(B)), dim3(TPB), 0,
                     (hipStream_t)stream, first, second, geo(B, H, W, n, fx, fy, delta_z), Idx{{p1, p2, p3}}, keep, loss, normals,
                     (uint32_t*)nullptr, (uint32_t*)nullptr);
  return launch_ok() ? DPTX_OK : DPTX_E_HIP;
}

}  // extern "C"
