// unet.h -- launchers of the version-1 UNet kernels (unet.hip): NHWC 16-bit activations (bf16 / fp16), fp32 arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace dptx {

// ---- small-channel 3x3 convolution (pad 1, stride 1, bias) with GroupNorm(8) records from the epilogue
// A block owns an 8 x 32 tile of output pixels of one image: one record per (image, tile, group).
constexpr int UNET_TILE_H = 8, UNET_TILE_W = 32;
inline int unet_conv_tiles(int H, int W) { return ((H + UNET_TILE_H - 1) / UNET_TILE_H) * ((W + UNET_TILE_W - 1) / UNET_TILE_W); }

struct UnetConvParams {
  const void* X;          // [B][H][W][x_pix_stride] 16-bit; the layer reads channels x_off .. x_off + Cin of every pixel
  const void* Wt;         // [Cout][taps * Cin] 16-bit, k = (ky*3 + kx) * Cin + c
  const float* bias;      // [Cout]
  void* Y;                // [B][H][W][Cout] 16-bit, dense: bias added, not normalised
  float* gn_part;         // [B][unet_conv_tiles][8] float2 (sum, sum of squares) of the stored (rounded) values; may be null
  int B, H, W, Cin, Cout, taps;  // taps 9, or 1 (a 1x1 product: the first layer behind unet_im2col3)
  int x_pix_stride, x_off;       // elements; both multiples of 8
};
bool unet_conv_small_supported(int Cin, int Cout, int taps);
hipError_t launch_unet_conv_small(int mode, const UnetConvParams& p, hipStream_t stream);

// first layer: x NCHW [B,3,H,W] (io type) -> P [B][H][W][32] 16-bit, P[.][(ky*3+kx)*3 + c] = x[c][y+ky-1][x+kx-1] (zero outside
// the image), elements 27..31 zero: down1.conv1 is then a 1-tap product with one padded k-block of 32
hipError_t launch_unet_im2col3(int mode, const void* x, int io, void* P, int B, int H, int W, hipStream_t stream);

// ---- GroupNorm(8): records -> (mean, rstd) -> apply
// statistics pass over a dense 16-bit tensor [B][HW][C] (C % 16 == 0, 16..1024): unet_gn_chunks(HW, C) records per image
int unet_gn_chunks(int HW, int C);
hipError_t launch_unet_gn_stats(int mode, const void* X, float* partial, int B, int HW, int C, hipStream_t stream);
// stats[b][g] = (mean, rstd) from nrec records per image, combined in double in a fixed order; variance clamped at 0;
// *flag |= 1 when a sum is not finite
hipError_t launch_unet_gn_finalize(const float* partial, int nrec, float* stats, int B, int HW, int C, float eps, unsigned* flag,
                                   hipStream_t stream);
struct UnetGnApply {
  const void* X;                 // raw [B][H][W][C] dense
  const float* stats;            // [B][8][2]
  const float* gamma; const float* beta;
  void* Y; int y_pix_stride, y_off;   // relu(gn(X)) at full size into a channel slice; Y may be null
  void* P; int p_pix_stride, p_off;   // 2x2 / 2 max-pooled copy (H and W even); may be null
  int B, H, W, C;
};
hipError_t launch_unet_gn_apply(int mode, const UnetGnApply& p, hipStream_t stream);
// last_bn + ReLU + last_conv2 (1x1, 16 -> OC <= 4): y NCHW fp32 [B][OC][H][W]; w [OC][16], b [OC] fp32
hipError_t launch_unet_gn_head(int mode, const void* X, const float* stats, const float* gamma, const float* beta, const float* w,
                               const float* b, float* y, int B, int HW, int OC, hipStream_t stream);

// bilinear x2, align_corners=False: X [B][H][W][C] dense -> Y [B][2H][2W] channel slice (pixel stride, offset)
hipError_t launch_unet_upsample2x(int mode, const void* X, void* Y, int B, int H, int W, int C, int y_pix_stride, int y_off,
                                  hipStream_t stream);

}  // namespace dptx
