// midas_stats.h -- the per-image alignment statistics of midas_loss.hip (stages a..c there: count + select, stats pass,
// solve) for the other units of the library.  midas_loss.hip defines both functions and dptx_midas_stats runs the very same
// stages, so a caller gets the medians, s, scale and shift of that entry point bit for bit; eval_metrics.hip
// (dptx_eval_depth_aligned) is the caller.  Host code only: nothing here is compiled for the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dptx {

// the workspace of midas_stats_launch = dptx_midas_workspace_bytes(B, H, W, 1); false for a shape outside the limits
bool midas_stats_workspace(int32_t B, int32_t H, int32_t W, int64_t* bytes);

// stats [B][DPTX_MIDAS_STATS] fp32 on the device (t_p, t_g, s_p, s_g, n, scale, shift, argmedian), for terms =
// DPTX_MIDAS_SSI and / or DPTX_MIDAS_ALIGN, written in stream order.  The caller has validated the pointers and the shape
// and owns `ws` (256-byte aligned within its allocation, midas_stats_workspace bytes).  false: a HIP call failed.
bool midas_stats_launch(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t terms,
                        float* stats, void* ws, hipStream_t stream);

}  // namespace dptx
