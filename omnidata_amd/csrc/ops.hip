// ops.hip -- the op-level entry points of include/dptx.h (dptx_op_*) and the process-wide debug switches of the GEMM
// launcher: single launches on caller-owned device buffers, for the op-level tests.  None of them touches a handle; the
// launch forms are the ones the forward's schedule uses (kernels.h / launch_forms.hip: gemm_params_*, gemm_add_*, gn_params).
#include <hip/hip_runtime.h>

#include "../../include/dptx.h"
#include "kernels.h"

using namespace dptx;

extern "C" {

static int rc(hipError_t r) { return r == hipSuccess ? DPTX_OK : DPTX_E_HIP; }

static Planes g_op_planes{0, 0};
int dptx_op_set_planes(int64_t act_plane_elems, int64_t w_plane_elems) {
  g_op_planes.act = act_plane_elems;
  g_op_planes.w = w_plane_elems;
  return DPTX_OK;
}

int dptx_op_gemm(int32_t dtype, const void* A, const void* W, const float* bias, const void* R, void* C, int32_t M, int32_t N,
                 int32_t K, int32_t act, int32_t a_fp32, int32_t c_fp32, int32_t r_fp32, void* stream) {
  GemmParams p;
  gemm_params_dense(p, M, N, K);
  p.A = A; p.W = W; p.C = C; p.bias = bias; p.R1 = R; p.act = act; p.a_fp32 = a_fp32; p.c_fp32 = c_fp32; p.r1_fp32 = r_fp32;
  p.planes = g_op_planes;
  return rc(launch_gemm(dtype, p, (hipStream_t)stream));
}

// dense GEMM with the LayerNorm fold's CONSUMER epilogue (tests/test_gpu_coresidency.py): C = act((A W^T - mu colsum) rstd + bias),
// (mu, rstd) of row m from the (sum, sum of squares) records ln_stats[m][0 .. ln_nblk) (row stride 8 records)
int dptx_op_gemm_ln(int32_t dtype, const void* A, const void* W, const float* bias, void* C, int32_t M, int32_t N, int32_t K,
                    int32_t act, const float* ln_stats, const float* ln_colsum, int32_t ln_nblk, float ln_eps, void* stream) {
  GemmParams p;
  gemm_params_dense(p, M, N, K);
  p.A = A; p.W = W; p.C = C; p.bias = bias; p.act = act; p.planes = g_op_planes;
  gemm_add_ln_consumer(p, ln_stats, ln_colsum, ln_nblk, ln_eps);
  return rc(launch_gemm(dtype, p, (hipStream_t)stream));
}

// dense GEMM with the LayerNorm fold's PRODUCER epilogue on the 16-bit token stream (what the proj / fc2 launches run):
// C <- C + A W^T + bias in place, and (sum, sum of squares) of every new row per 128-column block into row_stats[m][0 .. N / 128)
int dptx_op_gemm_stream(int32_t dtype, const void* A, const void* W, const float* bias, void* C, float* row_stats, int32_t M,
                        int32_t N, int32_t K, void* stream) {
  GemmParams p;
  gemm_params_dense(p, M, N, K);
  p.A = A; p.W = W; p.C = C; p.R1 = C; p.bias = bias; p.planes = g_op_planes;
  gemm_add_ln_producer(p, nullptr, row_stats);
  return rc(launch_gemm(dtype, p, (hipStream_t)stream));
}

// the same on the fp32 token stream of the parity mode: X (fp32) <- X + A W^T + bias in place, its 16-bit image into C16
int dptx_op_gemm_stream32(int32_t dtype, const void* A, const void* W, const float* bias, float* X, void* C16, float* row_stats,
                          int32_t M, int32_t N, int32_t K, void* stream) {
  GemmParams p;
  gemm_params_dense(p, M, N, K);
  p.A = A; p.W = W; p.C = X; p.c_fp32 = 1; p.R1 = X; p.r1_fp32 = 1; p.bias = bias; p.planes = g_op_planes;
  gemm_add_ln_producer(p, C16, row_stats);
  return rc(launch_gemm(dtype, p, (hipStream_t)stream));
}

int dptx_op_head_tail(int32_t dtype, const void* H0, const void* W2, const float* b2, const float* w4, const float* b4, float* y,
                      int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t relu_out, void* stream) {
  return rc(launch_head_tail(dtype, H0, W2, b2, w4, b4, y, DPTX_IO_FP32, B, Hs, Ws, C, relu_out, (hipStream_t)stream, g_op_planes));
}

int dptx_op_head_tail_io(int32_t dtype, const void* H0, const void* W2, const float* b2, const float* w4, const float* b4, void* y,
                         int32_t io, int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t relu_out, void* stream) {
  if (io != DPTX_IO_FP32 && io != DPTX_IO_BF16 && io != DPTX_IO_FP16) return DPTX_E_INVALID;
  return rc(launch_head_tail(dtype, H0, W2, b2, w4, b4, y, io, B, Hs, Ws, C, relu_out, (hipStream_t)stream, g_op_planes));
}

// the 1x1 projection of the unfused tail (misc.hip head_out_kernel): what bf16x3, and every size the fused form refuses, run
int dptx_op_head_out(int32_t dtype, const void* X, const float* w, const float* b, void* y, int32_t io, int32_t B, int32_t HW,
                     int32_t Cout, int32_t relu, void* stream) {
  if (io != DPTX_IO_FP32 && io != DPTX_IO_BF16 && io != DPTX_IO_FP16) return DPTX_E_INVALID;
  if (Cout < 1 || Cout > 4 || B < 1 || HW < 1) return DPTX_E_INVALID;
  if (dtype != DPTX_DTYPE_BF16 && dtype != DPTX_DTYPE_FP16 && dtype != DPTX_DTYPE_BF16X3 && dtype != DPTX_DTYPE_FP16X3)
    return DPTX_E_INVALID;
  return rc(launch_head_out(dtype, X, w, b, y, io, B, HW, Cout, relu, g_op_planes, (hipStream_t)stream));
}

int dptx_op_conv(int32_t dtype, const void* X, const void* Wt, const float* bias, const void* R, void* Y, int32_t B, int32_t H,
                 int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho,
                 int32_t Wo, int32_t a_relu, int32_t act, void* stream) {
  GemmParams p;
  gemm_params_conv(p, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, 2);
  p.A = X; p.W = Wt; p.C = Y; p.bias = bias; p.R1 = R; p.act = act; p.a_relu = a_relu; p.planes = g_op_planes;
  return rc(launch_gemm(dtype, p, (hipStream_t)stream));
}

int dptx_op_conv_planes(int32_t dtype, const void* X, const void* Wt, const float* bias, const void* R, void* Y, int32_t B, int32_t H,
                        int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho,
                        int32_t Wo, int32_t a_relu, int32_t act, int32_t epi2, int32_t c_hi_only, int32_t r1_hi_only, void* stream) {
  GemmParams p;
  gemm_params_conv(p, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, 2);
  p.A = X; p.W = Wt; p.C = Y; p.bias = bias; p.R1 = R; p.act = act; p.a_relu = a_relu; p.planes = g_op_planes;
  // the raw bits, set directly and not through gemm_set_plane_policy: this entry point's arguments are the fields themselves
  // and admit combinations that function never produces (epi2 with every lo plane switched off, r2_hi_only left 0), so
  // mapping them through it would need a second code path
  p.epi2 = epi2 & 1; p.a_hi_only = (epi2 >> 1) & 1; p.c_hi_only = c_hi_only; p.r1_hi_only = r1_hi_only;
  return rc(launch_gemm(dtype, p, (hipStream_t)stream));
}

int dptx_op_stem_conv(int32_t dtype, const float* x, const void* Wt, void* y, int32_t B, int32_t H, int32_t W, void* stream) {
  return rc(launch_stem_conv(dtype, x, DPTX_IO_FP32, Wt, y, B, H, W, g_op_planes, (hipStream_t)stream));
}

int dptx_op_stem_conv_io(int32_t dtype, const void* x, int32_t io, const void* Wt, void* y, int32_t B, int32_t H, int32_t W, void* stream) {
  if (io != DPTX_IO_FP32 && io != DPTX_IO_BF16 && io != DPTX_IO_FP16) return rc(hipErrorInvalidValue);
  return rc(launch_stem_conv(dtype, x, io, Wt, y, B, H, W, g_op_planes, (hipStream_t)stream));
}

int dptx_op_attention(int32_t dtype, const void* qkv, void* out, int32_t B, int32_t S, int32_t heads, void* stream) {
  return rc(launch_attention(dtype, qkv, out, B, S, heads, g_op_planes, (hipStream_t)stream));
}

int dptx_op_layernorm(int32_t dtype, const float* x, const float* gamma, const float* beta, void* y, int32_t M, int32_t C,
                      float eps, void* stream) {
  return rc(launch_layernorm(dtype, x, gamma, beta, y, M, C, eps, g_op_planes, (hipStream_t)stream));
}

int dptx_op_groupnorm(int32_t dtype, const void* X, const float* gamma, const float* beta, const void* R, void* Y, int32_t B,
                      int32_t HW, int32_t C, int32_t relu, float eps, void* scratch_f32, void* stream) {
  if (scratch_f32 == nullptr) return DPTX_E_INVALID;
  hipError_t r = launch_gn_stats(dtype, X, (float*)scratch_f32, B, HW, C, g_op_planes, (hipStream_t)stream);
  if (r != hipSuccess) return DPTX_E_HIP;
  GnParams g = gn_params(X, Y, gamma, beta, (float*)scratch_f32, B, HW, C, relu, eps, false);
  gn_add_residual(g, R);
  return rc(launch_gn_apply(dtype, g, g_op_planes, (hipStream_t)stream));
}

// the stem's GroupNorm + ReLU + MaxPool2dSame(3, 2): the stats pass, then the fused apply / pool.  Odd H / W are refused by
// launch_gn_relu_maxpool itself -- the guard the forward relies on -- and deliberately not here, so that the op-level test
// reaches it (the stats pass before it is harmless at any size).
int dptx_op_gn_relu_maxpool(int32_t dtype, const void* X, const float* gamma, const float* beta, void* Y, int32_t B, int32_t H,
                            int32_t W, int32_t C, float eps, void* scratch_f32, void* stream) {
  if (scratch_f32 == nullptr) return DPTX_E_INVALID;
  hipError_t r = launch_gn_stats(dtype, X, (float*)scratch_f32, B, H * W, C, g_op_planes, (hipStream_t)stream);
  if (r != hipSuccess) return DPTX_E_HIP;
  return rc(launch_gn_relu_maxpool(dtype, X, Y, gamma, beta, (const float*)scratch_f32, B, H, W, C, eps, g_op_planes, (hipStream_t)stream));
}

int dptx_op_cls_rows(int32_t dtype, const float* cls, const float* pos, float* X, int32_t B, int32_t S, int32_t C, void* X16,
                     float* row_stats, void* X8, float q_scale, void* stream) {
  if (row_stats != nullptr && C > 8 * 128) return DPTX_E_INVALID;  // records have a row stride of 8: C <= 1024
  return rc(launch_cls_rows(dtype, cls, pos, X, B, S, C, X16, row_stats, (hipStream_t)stream, X8, q_scale));
}

int dptx_debug_set_trace(void* dev_buf) {
  gemm_set_trace((long long*)dev_buf);
  return DPTX_OK;
}

int dptx_debug_set_gemm_flags(int32_t flags) {
  gemm_set_debug_flags(flags);
  return DPTX_OK;
}

int dptx_op_conv_fp8(const void* X8, const void* Wt8, const float* bias, const void* R, void* Y, void* Y8, int32_t B, int32_t H,
                     int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho,
                     int32_t Wo, int32_t act, int32_t q_relu, float out_scale, void* stream) {
  GemmParams p;
  gemm_params_conv(p, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, 1);
  p.C = Y; p.bias = bias; p.R1 = R; p.act = act;
  gemm_use_fp8_operands(p, X8, Wt8, out_scale, nullptr);
  gemm_add_fp8_copy(p, Y8, q_relu, 0.f);
  return rc(launch_gemm(MODE_FP8, p, (hipStream_t)stream));
}

int dptx_op_conv_groupnorm(int32_t dtype, const void* X, const void* Wt, void* Yraw, const float* gamma, const float* beta,
                           const void* R, void* Y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize,
                           int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo, int32_t relu, float eps,
                           void* scratch_f32, void* stream) {
  if (scratch_f32 == nullptr || (Ho * Wo) % 32 != 0) return DPTX_E_INVALID;
  GemmParams p;
  gemm_params_conv(p, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, 2);
  p.A = X; p.W = Wt; p.C = Yraw; p.planes = g_op_planes;
  gemm_add_gn_records(p, (float*)scratch_f32, Ho * Wo);
  if (launch_gemm(dtype, p, (hipStream_t)stream) != hipSuccess) return DPTX_E_HIP;
  GnParams g = gn_params(Yraw, Y, gamma, beta, (float*)scratch_f32, B, Ho * Wo, Cout, relu, eps, true);
  gn_add_residual(g, R);
  return rc(launch_gn_apply(dtype, g, g_op_planes, (hipStream_t)stream));
}

// conv1x1 (stride 1) + GroupNorm as the forward's folded schedule runs it (kernels.h C1_STATS / C1_GN): statistics pass,
// launch_gn_finalize, GroupNorm-epilogue pass.  passes: 1 = statistics pass (records; Y is the launch's C and is not touched),
// 2 = finalize (records, and r_records when R has a GroupNorm of its own -> tables), 4 = epilogue pass (-> Y); 7 = the whole op
int dptx_op_conv_groupnorm_fused(int32_t dtype, const void* X, const void* Wt, const float* gamma, const float* beta, const void* R,
                                 const float* r_gamma, const float* r_beta, const float* r_records, void* Y, int32_t B, int32_t H,
                                 int32_t W, int32_t Cin, int32_t Cout, int32_t relu, float eps, void* records_f32, void* tables_f32,
                                 int32_t passes, void* stream) {
  if (records_f32 == nullptr || tables_f32 == nullptr || (passes & ~7) != 0 || passes == 0 || H <= 0 || W <= 0) return DPTX_E_INVALID;
  if ((r_gamma != nullptr) != (r_beta != nullptr) || (r_gamma != nullptr) != (r_records != nullptr)) return DPTX_E_INVALID;
  if (r_gamma != nullptr && R == nullptr) return DPTX_E_INVALID;
  GemmParams p;
  gemm_params_conv(p, B, H, W, Cin, Cout, 1, 1, 0, 0, H, W, 2);
  p.A = X; p.W = Wt; p.C = Y; p.planes = g_op_planes;
  if (!conv1x1_gn_eligible(dtype, p)) return DPTX_E_INVALID;
  const ConvGnFold f{(float*)records_f32, gamma, beta, R, r_records, r_gamma, r_beta, (float*)tables_f32, relu, eps};
  for (int pass : {C1_PASS_STATS, C1_PASS_FINALIZE, C1_PASS_EPILOGUE})
    if ((passes & pass) && launch_conv1x1_gn_pass(dtype, p, f, pass, (hipStream_t)stream) != hipSuccess) return DPTX_E_HIP;
  return DPTX_OK;
}

// the apply pass alone, from caller-supplied records: what the forward's gn_apply launches behind a convolution that wrote
// GroupNorm records (gn_params with from_gemm_records, gn_add_residual, launch_gn_apply)
int dptx_op_groupnorm_records(int32_t dtype, const void* X, const float* gamma, const float* beta, const float* records,
                              const void* R, const float* r_gamma, const float* r_beta, const float* r_records, void* Y, int32_t B,
                              int32_t HW, int32_t C, int32_t relu, float eps, void* stream) {
  if (dtype != DPTX_DTYPE_BF16 && dtype != DPTX_DTYPE_FP16 && dtype != DPTX_DTYPE_BF16X3 && dtype != DPTX_DTYPE_FP16X3)
    return DPTX_E_INVALID;
  if (X == nullptr || Y == nullptr || gamma == nullptr || beta == nullptr || records == nullptr) return DPTX_E_INVALID;
  if (B < 1 || HW < 32 || HW % 32 != 0 || C < 64 || C % 64 != 0 || C > 1024) return DPTX_E_INVALID;
  if ((r_gamma != nullptr) != (r_beta != nullptr) || (r_gamma != nullptr) != (r_records != nullptr)) return DPTX_E_INVALID;
  if (r_gamma != nullptr && R == nullptr) return DPTX_E_INVALID;
  GnParams g = gn_params(X, Y, gamma, beta, const_cast<float*>(records), B, HW, C, relu, eps, true);
  gn_add_residual(g, R, r_gamma, r_beta, r_records);
  return rc(launch_gn_apply(dtype, g, g_op_planes, (hipStream_t)stream));
}

int dptx_op_upsample2x(int32_t dtype, const void* X, void* Y, int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
  return rc(launch_upsample2x(dtype, X, Y, B, H, W, C, g_op_planes, (hipStream_t)stream));
}

int dptx_op_upsample2x_strip(int32_t dtype, const void* X, void* Y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t rows,
                             void* stream) {
  return rc(launch_upsample2x_strip(dtype, X, Y, B, H, W, C, rows, (hipStream_t)stream));
}

// ---- the glue kernels of misc.hip, one launch each (tests/test_gpu_glue.py).  Every argument the launcher or the kernel would
// mishandle -- a size its 32-bit index arithmetic overflows on, a count that leaves an empty grid, a stride that breaks the
// alignment of its vector loads -- is refused here, before any launch.
static bool op_dtype16(int32_t dtype) {
  return dtype == DPTX_DTYPE_BF16 || dtype == DPTX_DTYPE_FP16 || dtype == DPTX_DTYPE_BF16X3 || dtype == DPTX_DTYPE_FP16X3;
}
static bool op_io(int32_t io) { return io == DPTX_IO_FP32 || io == DPTX_IO_BF16 || io == DPTX_IO_FP16; }

int dptx_op_patchify16(int32_t dtype, const void* x, int32_t io, void* P, int32_t B, int32_t H, int32_t W, void* stream) {
  if (!op_dtype16(dtype) || !op_io(io) || x == nullptr || P == nullptr) return DPTX_E_INVALID;
  if (B < 1 || H < 16 || W < 16 || H % 16 != 0 || W % 16 != 0) return DPTX_E_INVALID;
  return rc(launch_patchify16(dtype, x, io, P, B, H, W, g_op_planes, (hipStream_t)stream));
}

int dptx_op_depth_to_space(int32_t dtype, const void* G, void* Y, int32_t B, int32_t h, int32_t w, int32_t k, int32_t C,
                           void* stream) {
  if (!op_dtype16(dtype) || G == nullptr || Y == nullptr || G == Y) return DPTX_E_INVALID;
  if (B < 1 || h < 1 || w < 1 || k < 1 || k > 16 || C < 8 || C % 8 != 0) return DPTX_E_INVALID;
  if ((long long)h * k >= (1ll << 31) || (long long)w * k >= (1ll << 31)) return DPTX_E_INVALID;  // y*k + dy, x*k + dx are ints
  return rc(launch_depth_to_space(dtype, G, Y, B, h, w, k, C, g_op_planes, (hipStream_t)stream));
}

int dptx_op_pos_resize(const float* src, float* dst, int32_t g_old, int32_t gh, int32_t gw, int32_t C, void* stream) {
  if (src == nullptr || dst == nullptr || g_old < 1 || gh < 1 || gw < 1 || C < 1) return DPTX_E_INVALID;
  // the kernel's element index, and its source offset (y * g_old + x) * C, are ints
  if (((long long)gh * gw + 1) * C + 255 >= (1ll << 31) || (long long)g_old * g_old * C >= (1ll << 31)) return DPTX_E_INVALID;
  return rc(launch_pos_resize(src, dst, g_old, gh, gw, C, (hipStream_t)stream));
}

int dptx_op_readout_cls(int32_t dtype, const void* x, int64_t x_stride, const void* W, int32_t ldw, int32_t w_off,
                        const float* bias, float* out, int32_t B, int32_t N, int32_t K, int32_t x16, void* stream) {
  if (!op_dtype16(dtype) || x == nullptr || W == nullptr || out == nullptr) return DPTX_E_INVALID;
  if (B < 1 || N < 1 || K < 4 || K % 4 != 0 || w_off < 0 || w_off % 4 != 0 || ldw % 4 != 0 || ldw < w_off + K) return DPTX_E_INVALID;
  if (x_stride < K || x_stride % 4 != 0 || (long long)B * N + 3 >= (1ll << 31)) return DPTX_E_INVALID;
  if (x16 != 0 && mode_is_x3(dtype)) return DPTX_E_INVALID;  // the two-plane modes keep the fp32 stream: no lo plane of x is read
  return rc(launch_readout_cls(dtype, (const float*)x, x_stride, W, ldw, w_off, bias, out, B, N, K, g_op_planes,
                               (hipStream_t)stream, x16 != 0));
}

int dptx_op_cast_f32(int32_t dtype, const float* src, void* dst, int64_t n, void* stream) {
  if (!op_dtype16(dtype) || src == nullptr || dst == nullptr || n < 8 || n % 8 != 0) return DPTX_E_INVALID;
  return rc(launch_cast_f32(dtype, src, dst, (size_t)n, g_op_planes, (hipStream_t)stream));
}

int dptx_op_to_f32(int32_t dtype, const void* src, float* dst, int64_t n, void* stream) {
  if (!op_dtype16(dtype) || src == nullptr || dst == nullptr || n < 8 || n % 8 != 0) return DPTX_E_INVALID;  // cast_f32's rule
  return rc(launch_to_f32(dtype, src, dst, (size_t)n, g_op_planes, (hipStream_t)stream));
}

int dptx_op_amax(int32_t dtype, const void* X, int64_t n, int32_t relu, uint32_t* amax_bits, void* stream) {
  if (!op_dtype16(dtype) || X == nullptr || amax_bits == nullptr || n < 8 || n % 8 != 0) return DPTX_E_INVALID;
  return rc(launch_amax(dtype, X, (size_t)n, relu != 0, amax_bits, (hipStream_t)stream));
}

int dptx_op_nonfinite_scan(int32_t dtype, const void* X, int64_t n, uint32_t* flag, void* stream) {
  if (!op_dtype16(dtype) || X == nullptr || flag == nullptr || n < 8 || n % 8 != 0) return DPTX_E_INVALID;
  return rc(launch_nonfinite_scan(dtype, X, (size_t)n, flag, (hipStream_t)stream));
}

}  // extern "C"
