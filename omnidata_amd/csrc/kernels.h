// kernels.h -- host-visible launchers of the dptx HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace dptx {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: sets it once per (kernel, current
// device) -- one process may hold engines on several GPUs (misc.hip)
void ensure_dyn_smem(const void* kernel, size_t bytes);

// One implicit-GEMM problem: C[M,N] = epilogue( gatherA[M,K] * W[N,K]^T ).
// A is addressed as an NHWC image batch so that a dense row-major matrix, a strided 1x1
// convolution and a kxk convolution are the same code path:
//   m -> (img, oy, ox) with a_rpi = Hout*Wout rows per image;  k -> (ky, kx, c), c < Cin
//   elem = A + img*a_img_stride + a_off + ((oy*stride+ky-pad_t)*Win + (ox*stride+kx-pad_l))*a_pix_stride + c
// out-of-image taps read as zero.  K = ksz*ksz*Cin, Cin % 64 == 0, K % 64 == 0, N % BN == 0.
struct GemmParams {
  const void* A;
  const void* W;  // [N][K] 16-bit, K contiguous, K ordered (ky,kx,c)
  void* C;
  const float* bias;  // [N] or (bias_per_img) [imgs][N]; may be null
  const void* R1;     // residual, same addressing as C; may be null
  const void* R2;     // second residual; may be null
  int M, N, K;
  int ldw;  // elements between rows of W (>= K; ProjectReadout uses half of a [768][1536] matrix)
  int a_rpi, Wout, Hin, Win, Cin, a_pix_stride;
  long long a_img_stride, a_off;
  long long a_bytes;  // size of the A buffer in bytes (bounds of the buffer descriptor; glds path needs < 2^31)
  int ksz, stride, pad_t, pad_l;
  // C row of m: img = m / c_rpi, p = m % c_rpi -> row = img*c_img_rows + c_row_off + p
  int c_rpi, c_img_rows, c_row_off, ldc;
  int r2_bcast;      // R2 row = c_row_off + p (broadcast over images: pos_embed)
  int bias_per_img;  // bias row = img (of the C mapping)
  int act;           // 0 none, 1 relu, 2 gelu(erf)
  int a_relu;        // relu applied to A while staging (RCU pre-activation)
  int a_fp32;        // A elements are fp32 (converted while staging)
  int c_fp32, r1_fp32, r2_fp32;
  Planes planes;  // hi->lo plane distances (bf16x3 mode only)
  // per-layer precision policy (dtype "mixed"): epi2 = 1 runs the two-plane epilogue on a single-pass (one MFMA per product)
  // fp16 kernel -- residuals are read with their lo planes and C is written as a hi/lo pair; *_hi_only (two-plane epilogues,
  // also of the 3-MFMA kernels) switch off the lo plane of C / R1 / R2 individually
  int epi2, c_hi_only, r1_hi_only, r2_hi_only;
  // a_hi_only (fp16 hi/lo-plane kernels): TWO MFMAs per product -- a_hi w_hi + a_hi w_lo; the lo plane of A is not read
  // (per-layer precision 2 of dptx_set_layer_precision: the weights keep their full precision, the activations are rounded
  // to fp16 once)
  int a_hi_only;
  int xcd_m, xcd_n;  // XCD grid of the tile partition (filled in by launch_gemm)
  float cu_share;  // part of the chip this launch can count on, for the 256x256 rule (filled in by launch_gemm from
                   // gemm_set_cu_share; 0 = 1)
  float pad0;      // unused: kept so that the argument layout of the kernels does not move
  int k_tap_fast;    // visit the k-tiles taps-fastest inside a 64-channel block (3x3 convs with Cin >= 512: +12..17 %)
  // GroupNorm(32) statistics of the output from the epilogue (null: none): partial[img][gn_blocks][32] float2 records
  // of (sum, sum of squares) per 32-row block; gn_hw = rows per image (% 32 == 0), gn_cpg = N / 32 channels per group
  float* gn_part;
  int gn_hw, gn_blocks, gn_cpg;
  // fp8 (MODE_FP8: A and W are e4m3 bytes, K and ldw count bytes): C *= out_scale * out_scale_v[n] before the bias
  // (out_scale 0 = none; out_scale_v: optional per-output-channel vector -- the inverse of the power-of-two scale the
  // weights of channel n were quantised with; out_scale then carries the inverse of the activation scale).  C8: optional
  // e4m3 copy of the final output times q_scale (0 = 1.0; same addressing as C, 1 byte per element), ReLU'd first when
  // q_relu -- also available to the 16-bit modes (the producers of an fp8 GEMM's input run in bf16)
  void* C8;
  int q_relu;
  float out_scale, q_scale;
  const float* out_scale_v;
  // LayerNorm folded into the GEMMs around it (timm Block: x += proj(attn(norm1(x))); x += fc2(gelu(fc1(norm2(x))))):
  //  * PRODUCER side (patch-embed, proj, fc2 -- the launches that write the fp32 token stream): C16 = 16-bit copy of the
  //    final output rows (the next GEMM's A operand), row_stats = per (C row, 128-column block) float2 (sum, sum of
  //    squares) of the fp32 output, [rows][stats_nblk = 8] (row stride; N / 128 of them are written); needs
  //    N % 128 == 0, N <= 1024 and a tile at least 128 columns wide.
  //  * CONSUMER side (qkv, fc1): A is that 16-bit copy of the UN-normalised stream, W = gamma (.) W and bias = W beta + b
  //    were folded at pack time, ln_colsum[n] = sum_k W'[n][k] (of the ROUNDED operand values, so that the mean
  //    component cancels exactly), and the epilogue applies  y = (acc - mu * colsum) * rstd + bias  with (mu, rstd) of
  //    GEMM row m combined from the records ln_stats[m][0..ln_nblk) (ln_nblk = 6 or 8, row stride 8).
  void* C16;
  float* row_stats;
  int stats_nblk;
  const float* ln_stats;
  const float* ln_colsum;
  int ln_nblk;
  float ln_eps, ln_inv_dim;
  long long* trace;  // debug: s_memtime stamps of block 0 (dptx_debug_set_trace); null in production
  int debug_flags;   // debug (dptx_debug_set_gemm_flags): 1 = staged epilogue everywhere, 2 = one block per tile, 4 = lockstep two-plane 128x128 kernel,
                     // 8 = never take the streaming 1x1 kernel, 16 = take it wherever it can run (not only in the adopted classes),
                     // 32 / 64 = never / wherever eligible: the GroupNorm-epilogue schedule of the streaming kernel (read by the callers)
                     // (128 / 256 are read by launch_stem_conv / launch_upsample2x through gemm_debug_flags())
  float a_rpi_rcp, wout_rcp;  // 1 / a_rpi, 1 / Wout (filled in by launch_gemm: row -> (image, y, x) without integer division)
  // conv1x1.hip, GroupNorm-epilogue form (launch_conv1x1_stream form C1_GN): the per-(image, channel) affines of
  // launch_gn_finalize, gn_tab[img][4][N] = (a, d, ra, rd); the epilogue stores act( x a + d + (R1 ? (gn_tab_rgn ? r ra + rd : r) : 0) )
  // with x the rounded 16-bit convolution output and r the 16-bit R1 (same addressing as C), act = ReLU when p.act == 1
  const float* gn_tab;
  int gn_tab_rgn;
};

// ---- the launch forms of the schedule (launch_forms.hip): how each form is parameterised is written there and nowhere else.
// The forward (engine.hip) and the op-level entry points (ops.hip) call these and assign only pointers and their own choices
// (A, W, C, bias, R1, R2, act, a_relu, a_fp32, c_fp32, r*_fp32, planes) themselves.
// The four gemm_params_* reset p and fill a geometry; the gemm_add_* / gemm_use_* / gemm_set_* add one form to it.
// Fills the "plain dense row-major" defaults for A [M,K] (lda = K) and C [M,N].  a_elem_bytes: 2, or 1 for e4m3 operands.
void gemm_params_dense(GemmParams& p, int M, int N, int K, int a_elem_bytes = 2);
// Fills the geometry of an NHWC convolution [B,Hin,Win,Cin] -> [B,Hout,Wout,Cout] (weights [Cout][ksz][ksz][Cin], C dense
// [M,N]): M, N, K, ldw, the a_* and c_* fields, ldc and the tap order k_tap_fast.  a_elem_bytes: 2, or 1 for e4m3 operands.
void gemm_params_conv(GemmParams& p, int B, int Hin, int Win, int Cin, int Cout, int ksz, int stride, int pad_t, int pad_l,
                      int Hout, int Wout, int a_elem_bytes);
// The version-1 UNet's 3x3 convolution (pad 1, stride 1) at one level: gemm_params_conv of [B,H,W,Cin] -> [B,H,W,Cout] whose A
// operand is a channel slice of a wider NHWC buffer -- channels x_off .. x_off + Cin of pixels x_pix_stride elements apart
// (x_pix_stride = Cin, x_off = 0: dense); x_bytes = the size of the WHOLE buffer, the bound of the buffer descriptor.
void gemm_params_unet_conv(GemmParams& p, int B, int H, int W, int Cin, int Cout, int x_pix_stride, int x_off, long long x_bytes);
// Patch embedding: dense A [B*NP, K] -> rows 1 .. NP of every image's S = NP + 1 token rows of the fp32 stream C [B*S, D] (row 0
// is the cls row), plus R2 = the fp32 position embedding [S, D], broadcast over the images.  The caller assigns R2 (and C).
void gemm_params_patch_embed(GemmParams& p, int B, int NP, int S, int D, int K);
// ProjectReadout's token GEMM: A = the NP patch rows of every image of the 16-bit stream [B*S, D] (the cls row is skipped),
// W = the token half of the [D][2D] projection, bias = one row per image (the cls half, launch_readout_cls); C [B*NP, D].
void gemm_params_readout(GemmParams& p, int B, int NP, int S, int D);
// GroupNorm(32) records of the output from the epilogue (GemmParams::gn_part); HW rows per image, HW % 32 == 0
void gemm_add_gn_records(GemmParams& p, float* part, int HW);
// LayerNorm fold, consumer side (qkv, fc1): (mu, rstd) of row m from the records stats[m][0 .. nblk), row stride 8
void gemm_add_ln_consumer(GemmParams& p, const float* stats, const float* colsum, int nblk, float eps);
// LayerNorm fold, producer side: row_stats[row][8] of the stream this launch writes -- p.C, assigned by the caller, who also
// assigns R1 = C where the launch adds to the stream in place (proj, fc2).  C16 != null: C is the fp32 stream and C16 receives
// its 16-bit copy; C16 == null: C is the 16-bit stream itself.
void gemm_add_ln_producer(GemmParams& p, void* C16, float* row_stats);
// e4m3 operands (MODE_FP8; the geometry was filled with a_elem_bytes = 1): the accumulators are multiplied by out_scale (the
// inverse of the activation tensor's scale) and by out_scale_v[n] (the inverses of the weight's channel scales; may be null)
void gemm_use_fp8_operands(GemmParams& p, const void* A8, const void* W8, float out_scale, const float* out_scale_v);
// e4m3 copy of the output times scale, ReLU'd first when relu
void gemm_add_fp8_copy(GemmParams& p, void* C8, int relu, float scale);
// per-layer plane policy of the "mixed" dtype: x3 = the layer multiplies on hi/lo planes (2 or 3 MFMAs per product),
// a_reads_lo = it reads the lo plane of A (3 MFMAs), r1_lo / r2_lo = the residuals have a lo plane, out_lo = a consumer needs
// the lo plane of C.  Returns the kernel mode to launch with (MODE_FP16X3 / MODE_FP16).
int gemm_set_plane_policy(GemmParams& p, bool x3, bool a_reads_lo, bool r1_lo, bool r2_lo, bool out_lo);
// dtype 0 bf16 / 1 fp16.  Picks the tile configuration from (M, N).  Returns hipError_t.
hipError_t launch_gemm(int dtype, const GemmParams& p, hipStream_t stream);
// debug: every following GEMM launch stamps s_memtime per k-tile phase for the 8 waves of block 0 into dev_buf
// ([wave][64 k-tiles][4] int64; null switches it off)
void gemm_set_trace(long long* dev_buf);
// debug / tests: 1 = no register-direct epilogue, 2 = no persistent launch, 4 = no two-plane ping-pong kernel, 8 = never take
// the streaming 1x1 kernel, 16 = take it for every launch it can serve, also outside the classes it was adopted for, 32 = never
// fold a GroupNorm into a second pass of the streaming kernel (conv1x1_gn_*: the schedule conv -> gn_apply), 64 = fold it
// wherever that form can run, adopted or not (same results either way), 128 = the stem convolution and the x2 up-sampling on
// their first kernels (stem_conv_kernel, upsample2x_kernel) everywhere, 256 = the strip form of the up-sampling wherever it can
// run, not only in the classes it was adopted for (same results either way)
void gemm_set_debug_flags(int flags);
int gemm_debug_flags();
// conv1x1.hip: the streaming kernel for dense / strided 1x1 convolutions with K = Cin in {64, 128, 256}, N % 64 == 0, one 16-bit
// plane, optional per-column bias, ReLU and GroupNorm records (bf16 / fp16 modes): conv1x1_stream_eligible().  launch_gemm
// sends there what is eligible AND belongs to a (K, N, stride) class in which the kernel measured faster
// (conv1x1_stream_adopted(); debug flag 16 drops that second condition, flag 8 switches the kernel off); the bits are those
// of the tiled kernels.
bool conv1x1_stream_eligible(int mode, const GemmParams& p);
bool conv1x1_stream_adopted(const GemmParams& p);
// Two more forms of the same kernel fold the GroupNorm behind a stride-1 convolution into a SECOND pass over it (K is small:
// multiplying twice moves fewer bytes than storing the raw map and reading it back): C1_STATS runs the MFMAs and writes the
// records p.gn_part and nothing else (p.C is not touched); launch_gn_finalize turns the records into affines; C1_GN multiplies
// again and applies GroupNorm + shortcut (p.R1) + ReLU (p.act) to the rounded 16-bit value in the epilogue (p.gn_tab) -- the
// bits of conv -> launch_gn_apply.  conv1x1_gn_eligible() takes the parameters of the plain convolution (no R1, act 0) and
// needs rows per image % 32 == 0; conv1x1_gn_adopted() lists the (K, N) classes in which the folded schedule measured faster
// (debug flag 64 drops that condition, 32 switches the form off).  Direct launches: they do not pass through launch_gemm.
enum { C1_PLAIN = 0, C1_STATS = 1, C1_GN = 2 };
bool conv1x1_gn_eligible(int mode, const GemmParams& p);
bool conv1x1_gn_adopted(const GemmParams& p);
hipError_t launch_conv1x1_stream(int mode, const GemmParams& p, hipStream_t stream, int form = C1_PLAIN);
// The folded schedule as one definition: its operands, and one pass of it launched from the parameters of the plain
// convolution (A, W, C, planes assigned; conv1x1_gn_eligible).  Whether to take the folded schedule stays the caller's decision.
struct ConvGnFold {
  float* records;                          // (sum, sum of squares) records of the convolution output: a_rpi / 32 per image
  const float *gamma, *beta;               // [N]
  const void* R;                           // optional shortcut, addressed like C
  const float *r_records, *r_gamma, *r_beta;  // optional GroupNorm of the shortcut (all three or none)
  float* tables;                           // [imgs][4][N], written by the finalize pass, read by the epilogue pass
  int relu;
  float eps;
};
enum { C1_PASS_STATS = 1, C1_PASS_FINALIZE = 2, C1_PASS_EPILOGUE = 4 };
hipError_t launch_conv1x1_gn_pass(int mode, const GemmParams& conv, const ConvGnFold& f, int pass, hipStream_t stream);
// tile selection: the following launches share the chip with (1 / share - 1) concurrent streams of the same forward
void gemm_set_cu_share(float share);

hipError_t launch_attention(int mode, const void* qkv, void* out, int B, int S, int heads, Planes pl, hipStream_t stream);

hipError_t launch_layernorm(int mode, const float* x, const float* gamma, const float* beta, void* y,
                            int M, int C, float eps, Planes pl, hipStream_t stream);

// GroupNorm(32) on NHWC 16-bit: stats pass writes partial[B][chunks][32][2] fp32,
// apply pass: Y = act( gn(X) + (R ? (r_gamma ? gn2(R) : R) : 0) ).  In-place (Y==X) allowed.
struct GnParams {
  const void* X; void* Y;
  const float* gamma; const float* beta;  // [C]
  float* partial;                         // [B][chunks][32][2]
  const void* R;                          // optional residual (same shape)
  const float* r_gamma; const float* r_beta; const float* r_partial;  // optional GN on residual
  int B, HW, C, relu;
  float eps;
  int nrec;  // partial records per image in `partial` / `r_partial`: 0 = gn_chunks(HW, C) (written by launch_gn_stats),
             // HW / 32 when a GEMM epilogue wrote them (GemmParams::gn_part)
};
// launch_forms.hip: Y = act( gn(X) ) with the records in `partial`; from_gemm_records: a GEMM epilogue wrote them
// (gemm_add_gn_records) and not launch_gn_stats.  gn_add_residual: + R, normalised with its own triple when r_gamma != null
// (its records come from the same kind of producer as `partial`).
GnParams gn_params(const void* X, void* Y, const float* gamma, const float* beta, float* partial, int B, int HW, int C, int relu,
                   float eps, bool from_gemm_records);
void gn_add_residual(GnParams& g, const void* R, const float* r_gamma = nullptr, const float* r_beta = nullptr,
                     const float* r_partial = nullptr);
// the affines launch_gn_apply computes in its prologue, as tables for the GroupNorm epilogue of the streaming 1x1 kernel
// (GemmParams::gn_tab): tab[b][0..1][C] = (a, d) of (partial, gamma, beta), tab[b][2..3][C] those of the r_ triple (skipped
// when r_partial is null); nrec records per image.  One launch, one block per (image, triple).
hipError_t launch_gn_finalize(const float* partial, const float* gamma, const float* beta, const float* r_partial,
                              const float* r_gamma, const float* r_beta, float* tab, int B, int HW, int C, int nrec, float eps,
                              hipStream_t stream);
int gn_chunks(int HW, int C);  // blocks per image of the GroupNorm stats/apply grids = partial records per image
hipError_t launch_gn_stats(int mode, const void* X, float* partial, int B, int HW, int C, Planes pl, hipStream_t stream);
hipError_t launch_gn_apply(int mode, const GnParams& p, Planes pl, hipStream_t stream);
// stem: Y[B,Ho,Wo,C] = maxpool3x3s2_SAME( relu(gn(X[B,H,W,C])) ); H and W even (hipErrorInvalidValue otherwise)
hipError_t launch_gn_relu_maxpool(int mode, const void* X, void* Y, const float* gamma, const float* beta,
                                  const float* partial, int B, int H, int W, int C, float eps, Planes pl, hipStream_t stream);

// fused stem conv 7x7 s2 TF-SAME: x NCHW fp32 [B,3,H,W] -> y NHWC 16-bit [B,H/2,W/2,64]; Wt [64][176], k = (c*7+ky)*8 + kx
// io: element type of x (common.h IO_*: fp32 / bf16 / fp16).  bf16 / fp16 modes run stem_conv_kernel_wp (wave-private 16-bit
// staging, four blocks per CU; the same bits) unless debug flag 128 is set or x / Wt / y are not 16-byte aligned
hipError_t launch_stem_conv(int mode, const void* x, int io, const void* Wt, void* y, int B, int H, int W, Planes pl,
                            hipStream_t stream);

// bilinear x2 align_corners=True on NHWC 16-bit
// Y8 (optional): e4m3 copy of the output times q_scale, 1 byte per element, for an fp8 convolution downstream
hipError_t launch_upsample2x(int mode, const void* X, void* Y, int B, int H, int W, int C, Planes pl, hipStream_t stream,
                             void* Y8 = nullptr, float q_scale = 1.0f, bool out_hi_only = false);
// the strip form alone (bf16 / fp16, no e4m3 copy): R = 4 or 8 output rows per thread.  launch_upsample2x takes it in the (H, C)
// classes where it measured faster (debug flag 256: wherever it can run, 128: nowhere); the bits are upsample2x_kernel's
hipError_t launch_upsample2x_strip(int mode, const void* X, void* Y, int B, int H, int W, int C, int R, hipStream_t stream);
// fp8 calibration: atomicMax(*amax_bits, bits of max |x| (relu: max(x, 0)) over n 16-bit elements); *amax_bits starts at 0
hipError_t launch_amax(int mode, const void* X, size_t n, int relu, unsigned* amax_bits, hipStream_t stream);

// range check: *flag |= 1 if the 16-bit tensor X (n elements, n % 8 == 0; hi plane only) holds an Inf or a NaN
hipError_t launch_nonfinite_scan(int mode, const void* X, size_t n, unsigned* flag, hipStream_t stream);

// debug: *out += 64-bit sum of the 32-bit words of [p, p + bytes)
hipError_t launch_checksum(const void* p, size_t bytes, unsigned long long* out, hipStream_t stream);
hipError_t launch_spin(long long ticks_100mhz, hipStream_t stream);   // one sleeping wave (dptx_probe_stream_overlap)

// y NCHW fp32 [B,Cout,HW] = act( W[Cout][32] * x[B*HW,32] + b ),  Cout <= 4
hipError_t launch_head_out(int mode, const void* X, const float* w, const float* b, void* y, int io, int B, int HW,
                           int Cout, int relu, Planes pl, hipStream_t stream);

// X[b*577] = cls + pos[0]  (fp32 token stream)
// fused tail of the head: x2 bilinear -> conv3x3 128->32 -> ReLU -> conv1x1 32->C -> ReLU (head.hip)
// (hi / lo-plane modes: head_tail_x3_kernel, three MFMAs per product; `pl` = the plane distances of H0 and W2)
hipError_t launch_head_tail(int mode, const void* H0, const void* W2, const float* b2, const float* w4, const float* b4,
                            void* y, int io, int B, int Hs, int Ws, int C, int relu_out, hipStream_t stream, Planes pl = Planes{0, 0});
hipError_t launch_pos_resize(const float* src, float* dst, int g_old, int gh, int gw, int C, hipStream_t stream);
// X16 / stats (optional, LayerNorm fold): 16-bit copy of the rows and their (sum, sum of squares) per 128-column block; X may
// be null (16-bit token stream: no fp32 copy)
hipError_t launch_cls_rows(int mode, const float* cls, const float* pos, float* X, int B, int S, int C, void* X16, float* stats,
                           hipStream_t stream, void* X8 = nullptr, float q_scale = 1.0f);

// out[b][n] = bias[n] + sum_k x[b*x_stride + k] * W[n*ldw + w_off + k]   (x fp32, W 16-bit, out fp32)
// x16 != 0: x points at 16-bit values (the 16-bit token stream of the single-pass dtypes)
hipError_t launch_readout_cls(int mode, const float* x, long long x_stride, const void* W, int ldw, int w_off,
                              const float* bias, float* out, int B, int N, int K, Planes pl, hipStream_t stream, int x16 = 0);
// fp32 -> 16-bit (hi/lo planes in bf16x3 mode), n % 8 == 0
hipError_t launch_cast_f32(int mode, const float* src, void* dst, size_t n, Planes pl, hipStream_t stream);

// DPT-Large: x NCHW [B,3,H,W] (io type) -> 16x16 patches P[B*(H/16)*(W/16)][768], k = (c, ky, kx)
hipError_t launch_patchify16(int mode, const void* x, int io, void* P, int B, int H, int W, Planes pl, hipStream_t stream);
// G[(b,y,x)][(dy*k+dx)*C + c] -> Y[b][y*k+dy][x*k+dx][c]  (the re-layout half of a ConvTranspose2d with kernel == stride)
hipError_t launch_depth_to_space(int mode, const void* G, void* Y, int B, int h, int w, int k, int C, Planes pl, hipStream_t stream);

// generic 16-bit / fp32 -> fp32 copy for taps
hipError_t launch_to_f32(int mode, const void* src, float* dst, size_t n, Planes pl, hipStream_t stream);

}  // namespace dptx
