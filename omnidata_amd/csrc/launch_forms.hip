// launch_forms.hip -- how each launch form of the schedule is parameterised (kernels.h): the geometries of GemmParams and what
// a launch does beyond the plain product, one definition each.  Host code only; the forwards (engine.hip, unet_engine.hip) and
// the op-level entry points (ops.hip, unet.hip) both launch what these functions fill in.
#include "kernels.h"

namespace dptx {

void gemm_params_dense(GemmParams& p, int M, int N, int K, int a_elem_bytes) {
  p = GemmParams{};
  p.M = M; p.N = N; p.K = K; p.ldw = K;
  p.a_rpi = M > 0 ? M : 1; p.Wout = p.a_rpi; p.Hin = 1; p.Win = p.a_rpi; p.Cin = K; p.a_pix_stride = K;
  p.a_img_stride = 0; p.a_off = 0; p.ksz = 1; p.stride = 1; p.pad_t = 0; p.pad_l = 0;
  p.c_rpi = 0x7fffffff; p.c_img_rows = 0; p.c_row_off = 0; p.ldc = N;
  p.a_bytes = (long long)M * K * a_elem_bytes;
}

void gemm_params_conv(GemmParams& p, int B, int Hin, int Win, int Cin, int Cout, int ksz, int stride, int pad_t, int pad_l,
                      int Hout, int Wout, int a_elem_bytes) {
  p = GemmParams{};
  p.M = B * Hout * Wout; p.N = Cout; p.K = ksz * ksz * Cin; p.ldw = p.K;
  p.a_rpi = Hout * Wout; p.Wout = Wout; p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.a_pix_stride = Cin;
  p.a_img_stride = (long long)Hin * Win * Cin; p.a_off = 0; p.ksz = ksz; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
  p.c_rpi = 0x7fffffff; p.c_img_rows = 0; p.c_row_off = 0; p.ldc = Cout;
  p.a_bytes = (long long)B * Hin * Win * Cin * a_elem_bytes;
  p.k_tap_fast = (ksz == 3 && Cin >= 512) ? 1 : 0;  // measured per layer: profiles/r01_experiments.md
}

void gemm_params_unet_conv(GemmParams& p, int B, int H, int W, int Cin, int Cout, int x_pix_stride, int x_off, long long x_bytes) {
  gemm_params_conv(p, B, H, W, Cin, Cout, 3, 1, 1, 1, H, W, 2);
  p.a_pix_stride = x_pix_stride; p.a_off = x_off; p.a_img_stride = (long long)H * W * x_pix_stride; p.a_bytes = x_bytes;
}

void gemm_params_patch_embed(GemmParams& p, int B, int NP, int S, int D, int K) {
  gemm_params_dense(p, B * NP, D, K);
  p.c_rpi = NP; p.c_img_rows = S; p.c_row_off = 1; p.ldc = D; p.c_fp32 = 1;
  p.r2_bcast = 1; p.r2_fp32 = 1;
}

// (written out field by field, not through gemm_params_dense: A is addressed per image here, and tile selection and the row
// mapping read a_rpi / c_rpi = NP)
void gemm_params_readout(GemmParams& p, int B, int NP, int S, int D) {
  p = GemmParams{};
  p.a_bytes = (long long)B * S * D * 2;
  p.ldw = 2 * D;
  p.M = B * NP; p.N = D; p.K = D;
  p.a_rpi = NP; p.Wout = NP; p.Hin = 1; p.Win = NP; p.Cin = D; p.a_pix_stride = D;
  p.a_img_stride = (long long)S * D; p.a_off = D;  // skip the cls row
  p.ksz = 1; p.stride = 1;
  p.c_rpi = NP; p.c_img_rows = NP; p.c_row_off = 0; p.ldc = D;
  p.bias_per_img = 1;
}

void gemm_add_gn_records(GemmParams& p, float* part, int HW) {
  p.gn_part = part; p.gn_hw = HW; p.gn_blocks = HW / 32; p.gn_cpg = p.N / 32;
}

GnParams gn_params(const void* X, void* Y, const float* gamma, const float* beta, float* partial, int B, int HW, int C, int relu,
                   float eps, bool from_gemm_records) {
  GnParams g{};
  g.X = X; g.Y = Y; g.gamma = gamma; g.beta = beta; g.partial = partial;
  g.B = B; g.HW = HW; g.C = C; g.relu = relu; g.eps = eps;
  g.nrec = from_gemm_records ? HW / 32 : 0;
  return g;
}

void gn_add_residual(GnParams& g, const void* R, const float* r_gamma, const float* r_beta, const float* r_partial) {
  g.R = R; g.r_gamma = r_gamma; g.r_beta = r_beta; g.r_partial = r_partial;
}

void gemm_add_ln_consumer(GemmParams& p, const float* stats, const float* colsum, int nblk, float eps) {
  p.ln_stats = stats; p.ln_colsum = colsum; p.ln_nblk = nblk; p.ln_eps = eps; p.ln_inv_dim = 1.0f / (float)p.K;
}

void gemm_add_ln_producer(GemmParams& p, void* C16, float* row_stats) {
  p.C16 = C16; p.row_stats = row_stats; p.stats_nblk = 8;
}

void gemm_use_fp8_operands(GemmParams& p, const void* A8, const void* W8, float out_scale, const float* out_scale_v) {
  p.A = A8; p.W = W8; p.a_relu = 0;  // the producer of the e4m3 copy applied the ReLU
  p.out_scale = out_scale; p.out_scale_v = out_scale_v;
}

void gemm_add_fp8_copy(GemmParams& p, void* C8, int relu, float scale) {
  p.C8 = C8; p.q_relu = relu; p.q_scale = scale;
}

int gemm_set_plane_policy(GemmParams& p, bool x3, bool a_reads_lo, bool r1_lo, bool r2_lo, bool out_lo) {
  p.a_hi_only = x3 && !a_reads_lo;
  p.r1_hi_only = !r1_lo; p.r2_hi_only = !r2_lo; p.c_hi_only = !out_lo;
  p.epi2 = (!x3 && (out_lo || r1_lo || r2_lo)) ? 1 : 0;
  return x3 ? MODE_FP16X3 : MODE_FP16;
}

}  // namespace dptx
