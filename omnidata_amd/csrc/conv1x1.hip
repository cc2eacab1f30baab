// conv1x1.hip -- streaming kernel for the small-K 1x1 convolutions (ResNetV2 stages, refinenet out_conv).
//
//   C[M,N] = act( A[M,K] * W[N,K]^T + bias ),  K = Cin in {64, 128, 256}, stride 1 or 2, one 16-bit plane,
//   optional GroupNorm records of the raw accumulators (GemmParams::gn_part).
//
// These launches have one to four k-tiles of MFMA work per output tile: in gemm_glds_kernel a tile is a DMA prologue with
// nothing under it and an fp32 trip of the accumulators through LDS.  Here a block stays alive over many tiles:
//
// * The block's W panel (BN x K, at most 64 KB) is fetched once by LDS-DMA and stays in LDS for the block's life: the one
//   __syncthreads() of the kernel publishes it.  Blocks never talk to each other: no flags, counters or grid barriers.
// * After that every WAVE is a pipeline of its own over 32-row blocks of A (the unit of a GroupNorm record): its 32 x K
//   A rows arrive by LDS-DMA in a wave-private buffer (the loader idiom of gemm_glds_kernel: 128-byte k-tile rows, the
//   XOR swizzle applied to the source chunk, rows >= M fetched from an out-of-range offset, which reads as zeros), the
//   K / 16 fragments go to registers, and the DMA of the wave's NEXT row block is issued into the same buffer at once --
//   it lands under this block's MFMAs and epilogue.  Stores count in vmcnt on gfx9: the prefetch is waited for after the
//   MFMAs of the first 64 columns, before the first store of the row block.
// * Arithmetic is that of gemm_glds_kernel's staged form: v_mfma_f32_32x32x16 over ascending k-steps from a zero
//   accumulator, lane = output column, registers = rows -- so the GroupNorm records come from gn_records() (gemm_impl.h)
//   unchanged, and bias / ReLU / rounding see the same fp32 values.
// * Accumulators -> memory: bias, ReLU and the rounding to 16 bits happen in registers (T16::pack2, the conversion of
//   store8f); lanes 2c and 2c+1 swap one half of each packed pair (one DPP move and one v_perm_b32 per two values), so
//   that LDS receives packed 16-bit column pairs: half the bytes and half the ds_write_b32 of the fp32 staging.  The
//   staging is wave-private (16 rows x 64 columns at a time), read back as 16-byte row pieces: no block barrier.
//
// Forms (template parameter FORM; kernels.h C1_*).  A stride-1 convolution followed by a GroupNorm runs the kernel twice
// instead of storing the raw map and reading it back (K is small: the second product costs fewer bytes than the round trip):
// * C1_STATS: the MFMAs and gn_records() of the plain form -- the same records, bit for bit -- and nothing else: no bias, no
//   staging, no store; p.C is never touched.
// * C1_GN: the plain form up to the 16-byte row piece a lane reads back from the staging -- the rounded value the plain form
//   stores and gn_apply_kernel (norm.hip) loads -- then gn_apply_kernel's arithmetic on it, same order, same roundings:
//   x a[c] + d[c] (one fma), + the shortcut piece of p.R1 (itself r ra[c] + rd[c] behind a downsample branch), ReLU,
//   rounding, one 16-byte store.  The affines are the tables of launch_gn_finalize (p.gn_tab[img][4][N]): a 32-row block lies
//   in one image (rows per image % 32 == 0), so the table row is wave-uniform.  In the forward a wave's next row block lies
//   in another image (the stride is the whole grid), so nothing is kept across row blocks: the affines of a lane's 8 columns
//   and its shortcut pieces are fetched per 64-column pass, before the stores of the pass in front of it, so that waiting for
//   them never waits for a store.
//
// LDS: K = 64: 32 + 16 + 9 KB (BN = 256), K = 128: 32 + 32 + 9 KB (BN = 128) -- two blocks per CU; K = 256: 64 + 64 + 9 KB.
// (C1_GN at K = 64: BN = 128, 16 + 16 + 9 KB -- launch_c1_dt.)
#include "gemm_impl.h"

namespace dptx {

constexpr int C1_STG_PITCH = 144;                  // bytes per staged row: 64 columns x 2 + 16 (rows 1 and 4 apart: other banks)
constexpr int C1_STG_WAVE = 16 * C1_STG_PITCH;     // 16 rows per pass
constexpr int C1_WAVES = 4;

template <int KT, int BN>
constexpr size_t conv1x1_smem_bytes() {
  return (size_t)KT * BN * 128 + (size_t)C1_WAVES * KT * 32 * 128 + (size_t)C1_WAVES * C1_STG_WAVE;
}

// 8 packed 16-bit values <-> floats (common.h unpack8 / pack8 on the kernel's vector type)
template <int DT>
__device__ __forceinline__ void c1_unpack8(const u32x4_t v, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = T16<DT>::tof((uint16_t)(v[i] & 0xffffu));
    f[2 * i + 1] = T16<DT>::tof((uint16_t)(v[i] >> 16));
  }
}

template <int DT, int KT, int BN, int FORM>
__global__ __launch_bounds__(64 * C1_WAVES, KT <= 2 ? 2 : 1) void conv1x1_stream_kernel(const GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NSUB = BN / 64;            // 64-column passes over the panel
  constexpr int KS = KT * 4;               // k-steps of 16
  constexpr int W_BYTES = KT * BN * 128;   // [k-tile][BN rows][128 B]
  constexpr int A_WAVE = KT * 32 * 128;    // [k-tile][32 rows][128 B]
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;

  // block -> (W panel, slot of row blocks).  XCD x = blockIdx % 8 (observed placement; only speed depends on it): the
  // blocks that read the same A rows for different panels are neighbours on one XCD and share them out of its L2.
  const int npan = p.N / BN;
  const int x = (int)blockIdx.x & 7, l = (int)blockIdx.x >> 3;
  const int n0 = (l % npan) * BN;
  const int slots = ((int)gridDim.x / npan) * C1_WAVES;             // the grid is a multiple of 8 * npan blocks
  const int rb_total = (p.M + 31) >> 5;
  int rb = ((l / npan) * 8 + x) * C1_WAVES + wave;                  // this wave's first 32-row block

  const int w_bytes = (int)((long long)p.N * p.ldw * 2);
  const __amdgpu_buffer_rsrc_t rsrcA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.A), 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrcW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.W), 0, w_bytes, 0x00020000);

  char* const sw = smem;
  char* const sa = smem + W_BYTES + wave * A_WAVE;
  char* const stg = smem + W_BYTES + C1_WAVES * A_WAVE + wave * C1_STG_WAVE;

  // loader: lane (r0 = lane >> 3, kc = lane & 7) owns LDS chunk kc of rows r0 + 8 i of a k-tile and fetches the SOURCE
  // chunk kc ^ ((row >> 1) & 7)
  const int kc = lane & 7, r0 = lane >> 3;
  auto issue_a = [&](int rblk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = r0 + 8 * i;
      const int m = rblk * 32 + row;
      const bool ok = m < p.M;
      const int mm = ok ? m : 0;
      int rem, ox;  // M < 2^23 (launch_conv1x1_stream): reciprocal division
      const int img = row_div(mm, p.a_rpi, p.a_rpi_rcp, false, rem);
      const int oy = row_div(rem, p.Wout, p.wout_rcp, false, ox);
      const int iy = oy * p.stride - p.pad_t, ix = ox * p.stride - p.pad_l;
      const bool valid = ok && ((unsigned)iy < (unsigned)p.Hin) && ((unsigned)ix < (unsigned)p.Win);
      const long long e = (long long)img * p.a_img_stride + p.a_off + ((long long)iy * p.Win + ix) * p.a_pix_stride +
                          (kc ^ ((row >> 1) & 7)) * 8;
      const unsigned base = (unsigned)(e * 2);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const unsigned vo = valid ? base + kt * 128 : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcA, (__attribute__((address_space(3))) void*)(sa + kt * 4096 + i * 1024), 16, vo,
                                                 0, 0, 0);
      }
    }
  };

  // ---- prologue: the first row block and the W panel
  if (rb < rb_total) issue_a(rb);
  for (int idx = wave; idx < KT * (BN / 8); idx += C1_WAVES) {
    const int kt = idx / (BN / 8), rg = idx - kt * (BN / 8);
    const int row = rg * 8 + r0;
    const unsigned vo = (unsigned)(((long long)(n0 + row) * p.ldw + kt * 64 + (kc ^ ((row >> 1) & 7)) * 8) * 2);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcW, (__attribute__((address_space(3))) void*)(sw + kt * (BN * 128) + rg * 1024), 16, vo,
                                             0, 0, 0);
  }
  float bias_c[NSUB][2];
#pragma unroll
  for (int s = 0; s < NSUB; ++s)
#pragma unroll
    for (int j = 0; j < 2; ++j) bias_c[s][j] = FORM == C1_PLAIN && p.bias != nullptr ? p.bias[n0 + s * 64 + j * 32 + lr] : 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // the only block barrier: the W panel is in LDS

  const int swz = (lr >> 1) & 7;                                // every fragment row is 32 q + lr
  const unsigned sel = (lr & 1) ? 0x03020706u : 0x05040100u;    // v_perm_b32 selector of the column-pair exchange
  const int cn = lane & 7, rr = lane >> 3;

  // C1_GN: what the epilogue of 64-column pass s reads besides the staging -- the affines of this lane's 8 columns (table
  // row of the block's image) and its four shortcut pieces.  Fetched one pass ahead, in front of the stores of the pass before
  const bool has_r = FORM == C1_GN && p.R1 != nullptr;
  const bool r_gn = has_r && p.gn_tab_rgn != 0;

  for (; rb < rb_total; rb += slots) {
    const int m0 = rb * 32;
    float ga[NSUB][8], gd[NSUB][8], gra[NSUB][8], grd[NSUB][8];
    u32x4_t rq[NSUB][4];
    auto load_epi = [&](int s) {
      const int img = m0 / p.gn_hw;  // wave-uniform: rows per image % 32 == 0
      const float* tab = p.gn_tab + (long long)img * 4 * p.N + n0 + s * 64 + cn * 8;
      if (has_r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m0 + 16 * (i >> 1) + rr + 8 * (i & 1);  // < M: M % 32 == 0 in this form
          rq[s][i] = *(const u32x4_t*)((const uint16_t*)p.R1 + (long long)(p.c_row_off + m) * p.ldc + (n0 + s * 64 + cn * 8));
        }
      }
      *(float4*)&ga[s][0] = *(const float4*)(tab);
      *(float4*)&ga[s][4] = *(const float4*)(tab + 4);
      *(float4*)&gd[s][0] = *(const float4*)(tab + p.N);
      *(float4*)&gd[s][4] = *(const float4*)(tab + p.N + 4);
      if (r_gn) {
        *(float4*)&gra[s][0] = *(const float4*)(tab + 2 * p.N);
        *(float4*)&gra[s][4] = *(const float4*)(tab + 2 * p.N + 4);
        *(float4*)&grd[s][0] = *(const float4*)(tab + 3 * p.N);
        *(float4*)&grd[s][4] = *(const float4*)(tab + 3 * p.N + 4);
      }
    };
    if (FORM == C1_GN) load_epi(0);
    // ---- A fragments of this row block (landed: waited for below, or in the prologue) -> registers
    u32x4_t af[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      af[ks] = *(const u32x4_t*)(sa + (ks >> 2) * 4096 + lr * 128 + (((2 * (ks & 3) + lh) ^ swz) << 4));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads have returned: the buffer may be overwritten
    const bool prefetch = rb + slots < rb_total;
    if (prefetch) issue_a(rb + slots);

#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
      f32x16_t acc[1][2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][j][r] = 0.f;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        u32x4_t bf[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            bf[q][j] = *(const u32x4_t*)(sw + kt * (BN * 128) + (s * 64 + j * 32 + lr) * 128 + (((2 * q + lh) ^ swz) << 4));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[0][j] = T16<DT>::mfma32(af[kt * 4 + q], bf[q][j], acc[0][j]);
      }
      // the prefetched DMA before the first store of the row block (a vmcnt wait after stores would wait for them to
      // reach memory)
      if (s == 0) {
        __builtin_amdgcn_sched_barrier(0);  // behind the MFMAs, not among them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (FORM == C1_STATS || (FORM == C1_PLAIN && p.gn_part != nullptr)) gn_records<1, 2>(p, m0, n0 + s * 64, 0, 0, lr, lh, acc);
      if (FORM == C1_STATS) continue;
      if (FORM == C1_GN && s + 1 < NSUB) load_epi(s + 1);  // ahead of this pass's stores

#pragma unroll
      for (int h = 0; h < 2; ++h) {  // registers 8 h .. 8 h + 7 = tile rows 16 h .. 16 h + 15
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();  // the wave's LDS accesses execute in order: the previous pass's reads are ahead
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            float v0 = acc[0][j][8 * h + 2 * t] + bias_c[s][j], v1 = acc[0][j][8 * h + 2 * t + 1] + bias_c[s][j];
            if (FORM != C1_GN && p.act == 1) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }  // C1_GN: the ReLU follows the GroupNorm
            // own = (row r, row r + 1) of column lr.  Even lanes keep row r and take the neighbour's: (lr, lr + 1) of row r;
            // odd lanes keep row r + 1: (lr - 1, lr) of row r + 1
            const uint32_t own = T16<DT>::pack2(v0, v1);
            const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
            const uint32_t o = __builtin_amdgcn_perm(nb, own, sel);
            const int rl = ((2 * t) & 3) + (lr & 1) + 8 * (t >> 1) + 4 * lh;
            *(uint32_t*)(stg + rl * C1_STG_PITCH + (j * 32 + (lr & ~1)) * 2) = o;
          }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          const int rl = rr + 8 * pp;
          u32x4_t d = *(const u32x4_t*)(stg + rl * C1_STG_PITCH + cn * 16);
          const int m = m0 + 16 * h + rl;
          if (FORM == C1_GN) {  // gn_apply_kernel on the value it would have loaded: one fma each, a rounded add, ReLU
            float f[8];
            c1_unpack8<DT>(d, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = __builtin_fmaf(f[e], ga[s][e], gd[s][e]);
            if (has_r) {
              float r[8];
              c1_unpack8<DT>(rq[s][2 * h + pp], r);
              if (r_gn) {
#pragma unroll
                for (int e = 0; e < 8; ++e) r[e] = __builtin_fmaf(r[e], gra[s][e], grd[s][e]);
              }
#pragma unroll
              for (int e = 0; e < 8; ++e) f[e] = __fadd_rn(f[e], r[e]);
            }
            if (p.act == 1) {
#pragma unroll
              for (int e = 0; e < 8; ++e) f[e] = fmaxf(f[e], 0.f);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = T16<DT>::pack2(f[2 * e], f[2 * e + 1]);
          }
          if (FORM == C1_GN || m < p.M) *(u32x4_t*)((uint16_t*)p.C + (long long)(p.c_row_off + m) * p.ldc + (n0 + s * 64 + cn * 8)) = d;
        }
      }
    }
  }
#endif
}

bool conv1x1_stream_eligible(int mode, const GemmParams& p) {
  if (mode != MODE_BF16 && mode != MODE_FP16) return false;
  if (p.ksz != 1 || p.pad_t != 0 || p.pad_l != 0 || (p.stride != 1 && p.stride != 2)) return false;
  if (p.K != p.Cin || (p.K != 64 && p.K != 128 && p.K != 256) || p.N % 64 != 0) return false;
  if (p.a_fp32 || p.c_fp32 || p.epi2 || p.a_relu || p.R1 != nullptr || p.R2 != nullptr || p.bias_per_img) return false;
  if (p.c_rpi != 0x7fffffff || p.C8 != nullptr || p.C16 != nullptr || p.out_scale != 0.f) return false;
  if (p.row_stats != nullptr || p.ln_stats != nullptr || (p.act != 0 && p.act != 1)) return false;
  if (p.ldc % 8 != 0 || p.a_pix_stride % 8 != 0 || p.a_off % 8 != 0 || p.a_img_stride % 8 != 0) return false;
  // what the loader can address (the limits of the direct-to-LDS path of launch_cfg).  Either kernel gives the same bits, so
  // a batch that crosses them changes the speed of the launch and nothing else
  if (p.a_bytes <= 0 || p.a_bytes >= (1ll << 31) || (long long)p.N * p.ldw * 2 >= (1ll << 31) || p.M >= (1 << 23)) return false;
  return true;
}

// The (K, N, stride) classes that take this kernel in the forward: those whose op-level time at B = 32, records on, was below
// the tiled kernels' by more than the spread of five alternating repetitions (profiles/conv1x1_stream.md).  Left on the tiled
// kernels: K = 256 with N = 1024 (stage 2 conv3: a tie) and the stride-2 downsample of stage 1 (1 us, the size of the
// spread); K = 256, N = 256 (refinenet out_conv) wins at 96 x 96 and 48 x 48 and loses at 24 x 24 and 12 x 12, where a
// block fetches its 64 KB W panel for four or five row blocks -- the rule takes the rows of ONE image, so it depends on the
// layer's geometry and never on the batch.
bool conv1x1_stream_adopted(const GemmParams& p) {
  if (p.stride != 1) return false;
  if (p.K == 64) return p.N == 256 || p.N == 64;
  if (p.K == 128) return p.N == 512;
  if (p.K == 256) return p.N == 64 || p.N == 128 || (p.N == 256 && p.a_rpi >= 48 * 48);
  return false;
}

// the folded GroupNorm (C1_STATS + C1_GN); p: the plain convolution in front of the GroupNorm
bool conv1x1_gn_eligible(int mode, const GemmParams& p) {
  if (!conv1x1_stream_eligible(mode, p) || p.stride != 1 || p.bias != nullptr || p.act != 0) return false;
  const int cpg = p.N / 32;
  if (p.a_rpi % 32 != 0 || p.M % p.a_rpi != 0 || p.N > 1024 || (cpg & (cpg - 1)) != 0) return false;  // whole records; gn_records
  return p.c_row_off == 0 && p.ldc == p.N;  // the shortcut and the tables are addressed like a dense [M][N] map
}

// The (K, N) classes in which statistics pass + finalize + GroupNorm-epilogue pass measured faster than conv + apply pass by
// more than the spread of five alternating repetitions at B = 32 and B = 16 (profiles/conv1x1_gn_epilogue.md): conv3 of
// stages 0 and 1.  Left on conv + apply pass: K = 256, N = 1024 (stage 2: 1.5 us slower at B = 32, a tie at B = 16 -- eight
// W panels of 64 KB per 18 row blocks of an image, fetched twice).
bool conv1x1_gn_adopted(const GemmParams& p) {
  if (p.K == 64) return p.N == 256;
  if (p.K == 128) return p.N == 512;
  return false;
}

template <int DT, int KT, int BN, int FORM>
static hipError_t launch_c1(const GemmParams& p, hipStream_t stream) {
  constexpr size_t smem = conv1x1_smem_bytes<KT, BN>();
  static_assert(smem <= 160 * 1024 && (KT > 2 || 2 * smem <= 160 * 1024), "two blocks per CU at K <= 128");
  const int npan = p.N / BN;
  const int rb_total = (p.M + 31) / 32;
  const int want = (rb_total + C1_WAVES - 1) / C1_WAVES;       // blocks per panel that have a row block for every wave
  int cap = (KT <= 2 ? 512 : 256) / npan;                      // persistent: the block slots of the chip
  if (cap < 8) cap = 8;
  int groups = want < cap ? want : cap;
  groups = (groups + 7) / 8 * 8;
  auto k = conv1x1_stream_kernel<DT, KT, BN, FORM>;
  set_smem_attr(k, smem);
  hipLaunchKernelGGL(k, dim3(groups * npan), dim3(64 * C1_WAVES), smem, stream, p);
  return hipGetLastError();
}

template <int DT, int FORM>
static hipError_t launch_c1_dt(const GemmParams& p, hipStream_t stream) {
  if (p.K == 64) {
    // (the GroupNorm epilogue holds two passes' affines and shortcut pieces next to the accumulators: four passes of them do
    // not fit the 256 registers of two blocks per CU, so that form takes the 128-column panel)
    if constexpr (FORM != C1_GN)
      if (p.N % 256 == 0) return launch_c1<DT, 1, 256, FORM>(p, stream);
    if (p.N % 128 == 0) return launch_c1<DT, 1, 128, FORM>(p, stream);
    return launch_c1<DT, 1, 64, FORM>(p, stream);
  }
  if (p.K == 128) return p.N % 128 == 0 ? launch_c1<DT, 2, 128, FORM>(p, stream) : launch_c1<DT, 2, 64, FORM>(p, stream);
  return p.N % 128 == 0 ? launch_c1<DT, 4, 128, FORM>(p, stream) : launch_c1<DT, 4, 64, FORM>(p, stream);
}

template <int FORM>
static hipError_t launch_c1_form(int mode, const GemmParams& p, hipStream_t stream) {
  return mode == MODE_BF16 ? launch_c1_dt<DT_BF16, FORM>(p, stream) : launch_c1_dt<DT_FP16, FORM>(p, stream);
}

hipError_t launch_conv1x1_stream(int mode, const GemmParams& p0, hipStream_t stream, int form) {
  if (form == C1_PLAIN) {
    if (!conv1x1_stream_eligible(mode, p0) || p0.gn_tab != nullptr) return hipErrorInvalidValue;
    return launch_c1_form<C1_PLAIN>(mode, p0, stream);
  }
  // the two GroupNorm forms are launched directly: what launch_gemm fills in, and the checks on the plain convolution
  GemmParams p = p0;
  p.trace = nullptr;
  p.a_rpi_rcp = 1.0f / (float)(p.a_rpi > 0 ? p.a_rpi : 1);
  p.wout_rcp = 1.0f / (float)(p.Wout > 0 ? p.Wout : 1);
  GemmParams q = p;
  q.R1 = nullptr; q.act = 0; q.gn_tab = nullptr; q.gn_tab_rgn = 0; q.r1_fp32 = 0;
  if (p.M <= 0 || p.ldw < p.K || p.ldw % 8 != 0 || !conv1x1_gn_eligible(mode, q) || p.r1_fp32) return hipErrorInvalidValue;
  p.gn_hw = p.a_rpi; p.gn_blocks = p.a_rpi / 32; p.gn_cpg = p.N / 32;
  if (form == C1_STATS) {
    if (p.gn_part == nullptr || p.R1 != nullptr || p.act != 0 || p.gn_tab != nullptr) return hipErrorInvalidValue;
    return launch_c1_form<C1_STATS>(mode, p, stream);
  }
  if (form != C1_GN || p.gn_tab == nullptr || p.gn_part != nullptr || p.C == nullptr || p.C == p.R1) return hipErrorInvalidValue;
  return launch_c1_form<C1_GN>(mode, p, stream);
}

// one pass of conv1x1 + GroupNorm folded into three launches: how the statistics pass and the epilogue pass derive their
// parameters from the plain convolution's, and what the finalize pass reads from them (images = M / a_rpi, rows per image =
// a_rpi, one record per 32 rows)
hipError_t launch_conv1x1_gn_pass(int mode, const GemmParams& conv, const ConvGnFold& f, int pass, hipStream_t stream) {
  GemmParams q = conv;
  if (pass == C1_PASS_STATS) {
    q.gn_part = f.records;
    return launch_conv1x1_stream(mode, q, stream, C1_STATS);
  }
  const bool r_gn = f.r_gamma != nullptr;
  if (pass == C1_PASS_FINALIZE) {
    if (conv.a_rpi <= 0) return hipErrorInvalidValue;
    return launch_gn_finalize(f.records, f.gamma, f.beta, r_gn ? f.r_records : nullptr, f.r_gamma, r_gn ? f.r_beta : nullptr,
                              f.tables, conv.M / conv.a_rpi, conv.a_rpi, conv.N, conv.a_rpi / 32, f.eps, stream);
  }
  if (pass != C1_PASS_EPILOGUE) return hipErrorInvalidValue;
  q.R1 = f.R; q.act = f.relu ? 1 : 0; q.gn_tab = f.tables; q.gn_tab_rgn = r_gn;
  return launch_conv1x1_stream(mode, q, stream, C1_GN);
}

}  // namespace dptx
