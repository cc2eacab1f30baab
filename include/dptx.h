/* dptx.h -- C ABI of libdptx.so: the MI355X (gfx950) DPT-Hybrid-384 inference engine.
 *
 * This is the drop-in boundary for ONE path of EPFL-VILAB/omnidata: the forward pass of
 *   DPTDepthModel(backbone='vitb_rn50_384', num_channels={3|1})
 * (omnidata_tools/torch/modules/midas/dpt_depth.py:87-107, DPT.forward :67-85) that the
 * reference reaches from demo.py:140 (`model(img_tensor)`) and from the torch.hub entry
 * points `surface_normal_dpt_hybrid_384` / `depth_dpt_hybrid_384` (README.md:23-29).
 * The reference has no FFI of its own (it is pure Python on ATen); every entry point
 * below names the reference interface it replaces.  Plain pointers and sizes only; no
 * torch types, no C++ exceptions across the boundary.  All functions return 0 on success
 * or a negative DPTX_E_* code; dptx_last_error() gives the message.
 *
 * Ownership: the caller owns x / y device buffers (e.g. torch tensors' data_ptr());
 * the engine owns its packed weights and activation arena and never frees caller memory.
 * Threading: one handle per (device, stream); a handle is not re-entrant (the reference
 * is not either: vit.py:158 keeps hook outputs in a module-global dict); independent
 * handles may be used from independent threads.
 */
#ifndef DPTX_H_
#define DPTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dptx_engine* dptx_handle;

enum {
  DPTX_OK = 0,
  DPTX_E_INVALID = -1,   /* bad argument / wrong call order            */
  DPTX_E_KEY = -2,       /* unknown / missing / mis-shaped tensor key  */
  DPTX_E_HIP = -3,       /* a HIP runtime call failed                  */
  DPTX_E_NODEVICE = -4,  /* compute entry point called on a host-only handle */
  DPTX_E_ALLOC = -5
};

/* arithmetic type of the MFMA operands and of the stored activations.
 * BF16X3 is the high-precision mode: every 16-bit tensor is a pair of bf16 planes (hi, lo = x - hi,
 * 16 significand bits) and every product is 3 MFMAs (lo*hi + hi*lo + hi*hi) with fp32 accumulate:
 * ~3x the MFMA work and 2x the activation bytes, meets 1e-3 abs against the fp32 reference. */
enum { DPTX_DTYPE_BF16 = 0, DPTX_DTYPE_FP16 = 1, DPTX_DTYPE_BF16X3 = 2,
       /* FP16X3: the same hi/lo scheme with fp16 planes (hi = fp16(x) is also a valid single-pass fp16 operand).
        * MIXED : fp16 planes; the layer groups named in dptx_config.x3_groups run with 3 MFMAs per product, the others
        *         single-pass fp16 on the hi plane -- a per-layer precision policy (profiles/r02_precision_frontier.md). */
       DPTX_DTYPE_FP16X3 = 3, DPTX_DTYPE_MIXED = 4,
       /* FP8 (BASELINE.json configs[4] "fp8 MFMA weights"): a bf16 engine whose decoder convolutions -- the RCU 3x3 convs,
        *         out_conv and the first head conv: 31 % of a single-task forward's MACs, 43 % of the dual-task one's --
        *         run on OCP e4m3 operands (weights quantised at load time after a per-layer power-of-two scale, activations
        *         quantised by their producers' epilogues) on v_mfma_scale_f32_32x32x64_f8f6f4 at unit block scale, fp32
        *         accumulate.  Half the operand bytes per flop and twice the MFMA rate of bf16; per-conv error ~3 % rms
        *         (4-bit significand) -- a throughput mode with its own stated tolerance, NOT a parity mode
        *         (tests/test_gpu_fp8.py, profiles/r02_precision_frontier.md). */
       DPTX_DTYPE_FP8 = 5 };
/* layer groups of the forward for dptx_config.x3_groups (dtype = DPTX_DTYPE_MIXED).  A 3-MFMA group may only read
 * tensors produced by 3-MFMA groups (its lo planes must exist): HEAD needs FUSION needs RN needs RESNET and REASSEMBLE;
 * EMBED needs RESNET; the 12 ViT blocks exchange only the fp32 token stream and are free.  dptx_create rejects others. */
enum { DPTX_GROUP_RESNET = 1,      /* stem + ResNetV2 stages (convs and GroupNorms)            */
       DPTX_GROUP_EMBED = 2,       /* patch_embed.proj                                         */
       DPTX_GROUP_VIT = 4,         /* the 12 transformer blocks (LN, qkv, attention, proj, MLP) */
       DPTX_GROUP_REASSEMBLE = 8,  /* ProjectReadout + act_postprocess3/4 convs                */
       DPTX_GROUP_RN = 16,         /* scratch.layerN_rn                                        */
       DPTX_GROUP_FUSION = 32,     /* scratch.refinenet4..1                                    */
       DPTX_GROUP_HEAD = 64,       /* scratch.output_conv                                      */
       DPTX_GROUP_ALL = 127 };
/* backbones behind the same ABI (dpt_depth.py:27-35 `backbone=`) */
enum { DPTX_BACKBONE_VITB_RN50_384 = 0, DPTX_BACKBONE_VITL16_384 = 1 };
/* element type of the caller-side image AND result buffers of one forward call (`x_dtype`): fp32 is the drop-in default
 * (the reference feeds and returns fp32 tensors); with BF16 / FP16 the stem reads and the head writes 16-bit NCHW
 * tensors directly (SURVEY.md 8d config 2 feeds bf16) -- half the bytes at the boundary, no conversion pass. */
enum { DPTX_IO_FP32 = 0, DPTX_IO_BF16 = 1, DPTX_IO_FP16 = 2 };

typedef struct dptx_config {
  int32_t num_channels;  /* 3 = surface normals, 1 = depth (dpt_depth.py:88 num_channels)      */
  int32_t max_batch;     /* arena is sized for this many max_height x max_width images per call (1..48) */
  int32_t dtype;         /* DPTX_DTYPE_*                                                        */
  int32_t device_id;     /* HIP device ordinal; -1 = host-only handle (weight packing only)     */
  int32_t non_negative;  /* final ReLU of the head (dpt_depth.py:88,98 non_negative=True)       */
  int32_t ws_form;       /* 0: (w-mean)/(std+eps) timm 0.4.x;  1: (w-mean)/sqrt(var+eps)        */
  float   ws_eps;        /* StdConv2dSame eps (timm vit_base_r50_s16: 1e-8)                     */
  int32_t max_height;    /* largest input the arena is planned for; 0 = 384. Multiples of 32,   */
  int32_t max_width;     /*   >= 64, and max_batch*max_height*max_width*256 < 2^31 (see dptx_forward_hw) */
  int32_t dual_task;     /* 1: two decoders on one shared encoder (see dptx_forward_dual); needs num_channels = 3 */
  int32_t streams;       /* n = 2..4: a forward of >= 2 images runs as n sub-batches on n internal streams, forked   */
                         /*   from / joined to the caller's stream (same bits); 1: caller's stream only; 0 (default):  */
                         /*   MEASURED choice between 1 and 2 -- one stream until dptx_tune_schedule has timed both    */
  int32_t x3_groups;     /* dtype MIXED: OR of DPTX_GROUP_* that run with 3 MFMAs per product; 0 = the default policy  */
                         /*   (everything except the ViT blocks).  Ignored by the other dtypes.                      */
  int32_t backbone;      /* DPTX_BACKBONE_*: 0 = vitb_rn50_384 (DPT-Hybrid, the default), 1 = vitl16_384 (DPT-Large:  */
                         /*   dpt_depth.py:41-45 hooks [5,11,17,23], blocks.py:12-18, vit.py:176-309; demo.py:81)       */
  int32_t flags;         /* OR of DPTX_FLAG_*: switches for A/B runs of the fused schedules (0 = everything on)  */
  int32_t reserved;      /* must be zero                                                        */
} dptx_config;
/* dptx_config.flags.  NO_LN_FOLD: keep the 24 LayerNorm launches of the ViT blocks instead of folding the LayerNorm into
 * the qkv / fc1 GEMMs (gamma into W, W beta into the bias, (x W' - mu colsum(W')) rstd in the epilogue; row statistics and
 * the 16-bit operand copy of the fp32 token stream come out of the preceding proj / fc2 / patch-embed epilogue).  The fold
 * applies to single-pass ViT blocks only (bf16, fp16, fp8, and mixed policies without DPTX_GROUP_VIT).
 * GROUP_POLICY (dtype MIXED): do not install the default per-LAYER table of the decoder (see dptx_set_layer_precision);
 * every layer then follows its group's bit in x3_groups (round 2's policy: 2.14x the MFMA work of single-pass instead of
 * 1.66x, 1.5-2x smaller deviation from the fp32 forward). */
/* FP32_STREAM: keep the fp32 copy of the ViT token stream in the single-pass dtypes (BF16 / FP16 / FP8).  By default these
 * dtypes, with the LayerNorm fold, carry the residual stream of the 12 blocks only as the 16-bit tensor that the qkv / fc1
 * GEMMs multiply (what the reference itself does under model.half() / .bfloat16()): the proj / fc2 epilogues move 4 instead
 * of 10 bytes per element; the deviation from the fp32 forward grows by 1-5 % of itself (profiles/r03_experiments.md).
 * MIXED and the 3-MFMA dtypes always keep the fp32 stream. */
/* NO_RANGE_CHECK: skip the per-forward range scan of the fp16-plane dtypes (see dptx_range_status). */
/* FP8_ALL (dtype FP8): run all 19 eligible decoder convolutions (14 RCU 3x3, 4 out_conv, output_conv.0) on e4m3 operands --
 * round 3's mode: 7.5 - 9 degrees of mean angular error on the synthetic weight families, a lossy throughput mode.  Without the
 * flag only the six resConfUnit1 convolutions of refinenet1..3 do (oracle/fp8_layers.py: the set that keeps the mode within
 * 2 x the bf16 engine's error on both families). */
/* FP8_VIT (dtype FP8, round 6): qkv / fc1 / fc2 of every transformer block on e4m3 operands too (45 of the 127.6 GMAC; weights per
 * output channel, ONE calibrated power-of-two scale per activation tensor -- the token stream after proj / fc2 and the GELU
 * output get e4m3 copies from the producing epilogues; proj stays bf16).  Needs the LayerNorm fold and the 16-bit token stream
 * (the defaults).  oracle/fp8_vit.py: +2.1-2.7 / +1.2-1.9 degrees of mean angular error on the two synthetic weight families when
 * taken alone; on the GPU, together with the default decoder preset: 4.62 / 1.98 degrees against the bf16 engine's 4.18 / 1.07 --
 * inside the default preset's own bar (<= 2 x bf16 on both families, tests/test_gpu_fp8.py).  Not a parity mode. */
enum { DPTX_FLAG_NO_LN_FOLD = 1, DPTX_FLAG_GROUP_POLICY = 2, DPTX_FLAG_FP32_STREAM = 4, DPTX_FLAG_NO_RANGE_CHECK = 8, DPTX_FLAG_FP8_ALL = 16,
       DPTX_FLAG_FP8_VIT = 32 };

/* Fills *cfg with the reference defaults: C=3, max_batch=32, dtype MIXED (the mode that matches the reference's fp32
 * forward within 1e-3; DPTX_DTYPE_BF16 is the ~1.6x faster throughput mode that does not), device 0, non_negative=1,
 * ws_form=0, ws_eps=1e-8. */
void dptx_default_config(dptx_config* cfg);

/* Replaces the constructor DPTDepthModel(...) (dpt_depth.py:87-104). */
int dptx_create(dptx_handle* out, const dptx_config* cfg);
void dptx_destroy(dptx_handle h);

/* Replaces `model.load_state_dict(state_dict)` (demo.py:72; BaseModel.load base_model.py:4-16),
 * one tensor at a time.  `ref_key` is the reference state_dict key after the Lightning
 * `model.` prefix has been stripped (demo.py:65-70), e.g.
 * "pretrained.model.blocks.0.attn.qkv.weight"; `host_fp32` is a contiguous fp32 host array of
 * the given shape (OIHW for convs, [out,in] for linears).  Keys the forward never reads
 * (pretrained.model.norm.*, pretrained.model.head.*, scratch.refinenet4.resConfUnit1.*) are
 * accepted and ignored.  Unknown keys or wrong shapes -> DPTX_E_KEY. */
int dptx_load_tensor(dptx_handle h, const char* ref_key, const float* host_fp32,
                     const int64_t* shape, int32_t ndim);

/* Strict check + packing: every tensor the forward reads must have been loaded (else DPTX_E_KEY,
 * the message lists the missing keys -- mirrors load_state_dict(strict=True)).  Folds the
 * StdConv2dSame weight standardisation (input independent) into the conv weights, re-lays
 * OIHW -> [O][kh][kw][I], converts GEMM operands to cfg.dtype and builds one contiguous blob.
 * On a device handle the blob is uploaded and the activation arena is allocated. */
int dptx_finalize_weights(dptx_handle h);

/* Size of the packed blob (valid after finalize, or for any handle: depends only on cfg). */
size_t dptx_packed_bytes(dptx_handle h);
/* Copies the packed blob to host memory (works on host-only handles: used by CPU tests). */
int dptx_export_packed_host(dptx_handle h, void* dst_host, size_t bytes);
/* Copies the packed blob to / from a caller DEVICE buffer on `stream`.  This is the multi-GPU
 * start-up path: rank 0 finalizes, exports into a torch uint8 tensor, torch.distributed
 * (RCCL) broadcasts it over xGMI, the other ranks import it instead of packing themselves. */
int dptx_export_packed_device(dptx_handle h, void* dst_dev, size_t bytes, void* stream);
int dptx_import_packed_device(dptx_handle h, const void* src_dev, size_t bytes, void* stream);
/* Round 5: `dst` uses `src`'s packed weights IN PLACE (no copy): both handles must live on the same device and have been created
 * with configurations that pack the same blob (same layout header, same size); `src` must have its weights on the device.  The
 * allocation is reference-counted: the handles may be destroyed in any order (the last one frees it), and a handle that loads or
 * imports weights while others read its blob writes a fresh allocation instead -- sharing is a snapshot, never an alias of a
 * blob that changes under a reader.  A handle is not
 * re-entrant, so several forwards in flight on one GPU need several handles (each with its own activation arena, on its own
 * stream): this lets them read ONE copy of the 244 MB of weights out of L2 / Infinity Cache instead of one copy each
 * (omnidata_amd/pipeline.py ForwardPipeline: two batch-32 forwards in flight, +8 % images/s over the two-halves-of-one-forward
 * schedule -- the ResNetV2 stages of one forward then run under the MFMA-bound ViT / decoder launches of the other).
 * The packed blob is read-only during forwards. */
int dptx_share_packed(dptx_handle dst, dptx_handle src);

/* Bytes of device memory held by the handle (packed weights + activation arena). */
size_t dptx_workspace_bytes(dptx_handle h);

/* Replaces `DPTDepthModel.forward(x)` (dpt_depth.py:106-107 -> DPT.forward :67-85).
 *   x_dev : [batch,3,384,384] contiguous NCHW of x_dtype (DPTX_IO_FP32 / _BF16 / _FP16); normal model expects
 *           values in [0,1], depth model in [-1,1] (omnidata_tools/torch/README.md:46,49).
 *   y_dev : [batch,C,384,384] contiguous NCHW of the same x_dtype (for C=1 this is bit-identical to the
 *           reference's squeezed [batch,384,384]); >= 0 when non_negative, NOT clamped to 1
 *           (callers clamp: demo.py:140).
 * Asynchronous on `stream` (a hipStream_t; NULL = default stream). 1 <= batch <= max_batch. */
int dptx_forward(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev,
                 int32_t batch, void* stream);

/* Same forward at another input size: what the reference does when DPTDepthModel is fed a tensor
 * that is not 384x384 -- forward_flex (vit.py:119-155) resamples pos_embed to the (height/16, width/16)
 * patch grid with _resize_pos_embed (vit.py:102-116, bilinear, align_corners=False) and everything else
 * is convolutional.  height, width: multiples of 32 (the reference's own constraint: the 1/32-scale map is
 * up-sampled x2 and added to the 1/16-scale map), >= 64, height*width <= max_height*max_width of the config.
 *   x_dev [batch,3,height,width] NCHW fp32  ->  y_dev [batch,C,height,width] NCHW fp32.
 * dptx_forward(...) == dptx_forward_hw(..., 384, 384, ...). */
int dptx_forward_hw(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev,
                    int32_t batch, int32_t height, int32_t width, void* stream);

/* Dual-task forward (BASELINE.json configs[4]): ONE encoder pass (`pretrained.*`: ResNetV2 stem and
 * stages, ViT blocks, read-outs, DPT.forward dpt_depth.py:71) feeds TWO decoders -- `scratch.*` (surface normals, 3
 * channels) and `depth.scratch.*` (depth, 1 channel; same layer names as dpt_depth.py:73-83 behind the "depth." prefix).
 * 185.29 GMAC per image instead of 2 x 127.62.  This is a composition the reference does not ship (its two checkpoints
 * are separately fine-tuned full models); parity is defined against the reference forward run twice with `pretrained.*`
 * tied.  Needs a handle created with dual_task = 1, num_channels = 3; both heads see the same input tensor.
 *   y_normal_dev [batch,3,height,width], y_depth_dev [batch,1,height,width], NCHW fp32.
 * dptx_tap after a dual forward: encoder taps as usual, the depth decoder's under "depth.<name>"; the normal decoder's
 * are not available (its buffers were re-used). */
int dptx_forward_dual(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_normal_dev, void* y_depth_dev,
                      int32_t batch, int32_t height, int32_t width, void* stream);

/* dtype MIXED: per-layer precision inside the decoder (scratch.layerN_rn, refinenet*, output_conv.0 / .2).  `mfmas` = 1: the
 * convolution multiplies the hi planes only (one MFMA per product); 3: hi/lo planes, three MFMAs; 2: hi/lo planes of the weights,
 * hi plane of the activations (a_hi w_hi + a_hi w_lo: the input is rounded to fp16 once, the weights are exact to 22 bits --
 * half of the layer's rounding variance for two thirds of the 3-MFMA cost).  Layers that were never set follow their group's
 * bit in dptx_config.x3_groups.  Tensors between layers carry a lo plane exactly where a 3-MFMA consumer reads it, so every
 * assignment is valid.  With x3_groups = 0 dptx_create installs the default table (oracle/precision_layers.py);
 * DPTX_FLAG_GROUP_POLICY suppresses it.  (Measured option outside the default: "scratch.output_conv.0.weight" = 2 is +3.9 %
 * throughput for a worst-case deviation of 7.6e-4 instead of 6.3e-4 over a 32-image batch.)  May be called at any time before a forward; does not
 * touch the packed weights.  The reference has no counterpart (it computes in fp32 throughout). */
int dptx_set_layer_precision(dptx_handle h, const char* conv_weight_key, int32_t mfmas);

/* fp8 dtype: activation scales.  Every tensor that has an e4m3 copy (the inputs of the decoder's fp8 convolutions) is
 * quantised as e4m3(x * s) with a per-tensor power-of-two scale s; e4m3 covers 2^-9 .. 448, so with s = 1 (a fresh handle)
 * activations beyond 448 saturate and activations below 2^-9 vanish.  dptx_calibrate_fp8 runs ONE forward of the given
 * batch with the decoder convolutions on their bf16 operands, measures max |x| of every such tensor and sets s so that
 * the maximum lands in (112, 224] (one binade of headroom); the results y (and y2 for a dual-task handle, else NULL) are
 * the bf16-decoder results of that batch.  Call it once after loading weights, on a representative batch, before the
 * first dptx_forward.  The reference has no counterpart (it has no fp8 path); weights are quantised per output channel
 * at dptx_finalize_weights. */
int dptx_calibrate_fp8(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev, void* y2_dev,
                       int32_t batch, int32_t height, int32_t width, void* stream);
/* Number of e4m3 tensors of the last forward (<= 128); copies their scales / calibration max |x| (either may be NULL).
 * dptx_fp8_set_calibration installs scales measured elsewhere (rank 0 calibrates, the others receive: positive powers of
 * two, slot order = launch order of the forward). */
int dptx_fp8_get_calibration(dptx_handle h, float* scales, float* amax, int32_t capacity);
int dptx_fp8_set_calibration(dptx_handle h, const float* scales, int32_t n);

/* Range check of the fp16-plane dtypes (FP16, FP16X3, MIXED): fp16 planes cannot hold |x| > 65504 and nothing in the forward
 * clamps.  Every forward of such a handle scans the first head convolution's output -- the tensor that every decoder path
 * and, through them, the ViT blocks reach by residual additions -- for Inf / NaN (one 9.4 MB/image read, ~0.3 % of the
 * forward) and ORs the finding into a STICKY device flag.  dptx_range_status waits for `stream`, stores the flag in
 * *nonfinite (0 / 1), and clears it when reset != 0.  The check reads the activations, not the result: ReLUs behind the
 * scanned tensor turn a NaN into 0, so an overflow can leave a finite, wrong output.  Always 0 for the bf16-plane dtypes
 * (fp32's exponent range) and with DPTX_FLAG_NO_RANGE_CHECK.  omnidata_amd.model reads it after the first forward of a
 * set of weights and periodically afterwards, and falls back to bf16 planes (BF16X3 / BF16) when it is set. */
int dptx_range_status(dptx_handle h, int32_t* nonfinite, int32_t reset, void* stream);

/* Debug hook for stage-level parity (SURVEY.md A.1 tap names: "stem","s0","s1","s2","tok0",
 * "blk0".."blk11","l3","l4","l1_rn".."l4_rn","p4","p3","p2","p1","h0","h1").  Copies the
 * stage activation of the LAST forward, converted to fp32 in the engine's internal layout
 * (NHWC for feature maps, [batch*S,768] for tokens; S = (H/16)*(W/16)+1 = 577 at 384x384), to dst_host.  *shape4
 * receives {batch, H, W, C} (or {batch,S,768,1}).  Returns DPTX_E_KEY for unknown names.  Taps make the forward run
 * as one pass over the whole batch on the caller's stream and keep the three-launch head tail (so "h1" exists). */
int dptx_tap(dptx_handle h, const char* name, float* dst_host, size_t capacity_floats,
             int64_t shape4[4]);
/* The fp32 token stream is updated in place by the 12 blocks; "tok0"/"blkN" taps therefore need
 * copies.  on=1 allocates 13 snapshots and makes dptx_forward record them (debug only). */
int dptx_enable_taps(dptx_handle h, int on);

/* Number of kernel launches issued by one dptx_forward and algorithmic vs executed MACs
 * per image (algorithmic 127.624e9 for C=3; executed differs because out_conv
 * is commuted in front of the x2 upsample). */
int dptx_forward_info(dptx_handle h, int64_t* launches, double* algorithmic_macs,
                      double* executed_macs);

/* Intra-forward schedule of a handle created with streams = 0 (round 6).  Whether two half-batches on two internal streams
 * beat one whole-batch run depends on what the runtime does with the two streams on THIS box in THIS process (hardware-queue
 * sharing, priorities: measured from +6 % to -25 %, profiles/r05_experiments.md, r06_experiments.md) -- so it is measured,
 * not assumed: dptx_tune_schedule runs the forward of this very batch `reps` times per schedule (after one untimed run each),
 * timed with HIP events on `stream`, keeps the two-stream schedule only if it is at least 3 % faster, and blocks until done.
 * The result of either schedule is the same bits.  dptx_schedule_info reports the decision: *split = 1 two half-batches,
 * 0 one stream; *tuned = 0 while nothing has been measured (one stream); ms_* = the measured times (0 before).
 * Handles with streams >= 1 (or DPTX_STREAMS set) keep the schedule they were told: tune returns DPTX_OK without measuring.
 * y_depth_dev: dual-task handles only (else NULL). */
int dptx_tune_schedule(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev, void* y_depth_dev, int32_t batch,
                       int32_t height, int32_t width, int32_t reps, void* stream);
int dptx_schedule_info(dptx_handle h, int32_t* split, int32_t* tuned, float* ms_single, float* ms_split);

/* Do two streams of `device_id` actually run concurrently?  Work on two streams that the runtime has mapped onto ONE hardware
 * queue executes in order (profiles/r05_experiments.md: 1974 instead of 2600 images/s), and nothing in the API says so.  The
 * probe launches a sleeping one-wave kernel of `spin_us` microseconds (0 = 2000) on stream_a alone, then on both streams at
 * once, host-timed: *ratio = t_both / t_alone -- ~1.0 concurrent, ~2.0 serialised.  Blocks (two stream synchronisations per
 * measurement); both streams must be idle-able.  omnidata_amd/pipeline.py checks its slot streams with it. */
int dptx_probe_stream_overlap(int32_t device_id, void* stream_a, void* stream_b, int32_t spin_us, float* ratio);

/* Per-launch timing of the NEXT forwards with one HIP event after every launch on the forward's
 * stream (kernels of one forward are serialized, so consecutive events bracket one kernel plus
 * its launch gap).  dptx_profile_get sums the last forward by category:
 * 0 = implicit-GEMM MFMA kernel, 1 = attention, 2 = LayerNorm/GroupNorm, 3 = other glue. */
int dptx_set_profiling(dptx_handle h, int on);
int dptx_profile_get(dptx_handle h, int32_t category, double* ms, int64_t* launches,
                     double* macs_per_image);
/* Writes "idx,category,name,ms" for every launch of the last profiled forward. */
int dptx_profile_dump(dptx_handle h, const char* path);

const char* dptx_last_error(dptx_handle h);
const char* dptx_version(void);

/* ---- GPU-side pre/post-processing of demo.py (no handle needed; all pointers are DEVICE pointers) ----
 * dptx_preprocess_u8 replaces demo.py:74-76 / 92-95 / 130-138 for RGB (C=3) or greyscale (C=1) uint8 HWC images:
 * Resize(384, BILINEAR, shorter side) with Pillow's antialiased 8-bit two-pass resampler (bit-identical),
 * CenterCrop(384), ToTensor (/255), optional Normalize(0.5,0.5) (depth), 1->3 channel repeat.
 * x_dev: [3,384,384] fp32.  Both image sides must be >= 1 and the resized image >= 384x384 (always true). */
int dptx_preprocess_u8(const void* img_dev, int32_t H, int32_t W, int32_t C, int32_t row_stride_bytes,
                       int32_t depth_normalize, void* x_dev, void* stream);
/* demo.py:140,150: clamp(0,1) -> *255 -> uint8 (truncation), [3,384,384] fp32 -> [384,384,3] uint8. */
int dptx_postprocess_normal_u8(const void* y_dev, void* rgb_u8_dev, void* stream);
/* demo.py:143-145: bicubic 384->512 (align_corners=False), clamp(0,1), 1-x; [384,384] -> [512,512] fp32. */
int dptx_postprocess_depth(const void* y_dev, void* out512_dev, void* stream);
/* Host-side helper (exposed for tests): Pillow's fixed-point bilinear resampling coefficients for one axis.
 * bounds: [out_size][2] (first tap, tap count); kk: [out_size][*ksize] 22-bit fixed-point weights. */
int dptx_resample_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* kk, int32_t kk_capacity,
                         int32_t* ksize);

/* ---- The same for a whole batch of images of different sizes (no handle; DEVICE pointers unless stated otherwise) ----
 * Every call is stream-ordered on `stream`, uses only the caller's workspace (no allocation, no host synchronisation, no
 * process-lifetime cache: graph-capturable) and returns DPTX_E_INVALID for bad arguments before anything is launched.
 *
 * dptx_preprocess_u8_batch: B uint8 HWC images inside one packed pixel buffer -> x [B][3][S][S] fp32, per image what
 * dptx_preprocess_u8 computes for S = 384 (bit-identical to Pillow's resampler).  `descs` is a HOST array of B descriptors,
 * read before the call returns; image i starts at pixels_dev + descs[i].offset.  Image i's result depends on image i only.
 * Range: 1 <= B <= 4096, S a multiple of 32 in [32, 1024], C in {1, 3}, 1 <= H, W <= 16384, row_stride_bytes >= W*C,
 * min(H, W) <= 32*S.  The resample weights are computed on the device (fp64, Pillow's operations in Pillow's order) into the
 * workspace, 32 images at a time; each block then forms the horizontal pass of the input rows its output tile needs once,
 * in LDS.  Workspace: 17664 * S bytes, whatever B is (dptx_preprocess_batch_workspace_bytes; host-only). */
typedef struct dptx_image_desc {
  int64_t offset;            /* bytes from pixels_dev to the image's first pixel */
  int32_t H, W, C;           /* rows, columns, channels (1 or 3)                 */
  int32_t row_stride_bytes;  /* >= W*C                                           */
} dptx_image_desc;
int dptx_preprocess_batch_workspace_bytes(int32_t B, int32_t S, int64_t* bytes);
int dptx_preprocess_u8_batch(const void* pixels_dev, const dptx_image_desc* descs, int32_t B, int32_t S,
                             int32_t depth_normalize, void* x_dev, void* workspace, int64_t workspace_bytes, void* stream);
/* One axis of the tables dptx_preprocess_u8_batch builds, as the device computes them: the layout of dptx_resample_coeffs
 * in DEVICE memory (bounds_dev [out_size][2], kk_dev [out_size][*ksize_host_out]); *ksize_host_out is written on the host
 * before the call returns.  1 <= in_size, out_size <= 2^20, ksize <= 4097, kk_capacity >= out_size * ksize. */
int dptx_resample_coeffs_device(int32_t in_size, int32_t out_size, void* bounds_dev, void* kk_dev, int32_t kk_capacity,
                                int32_t* ksize_host_out, void* stream);
/* y [B][3][S][S] fp32 -> [B][S][S][3] uint8 (clamp, *255, truncate), one launch.  1 <= B <= 65535, 1 <= S <= 4096. */
int dptx_postprocess_normal_u8_batch(const void* y_dev, int32_t B, int32_t S, void* rgb_u8_dev, void* stream);
/* y [B][S][S] fp32 -> [B][512][512] fp32: dptx_postprocess_depth per image (bit-identical), one launch.
 * 1 <= B <= 65535, 1 <= S <= 4096. */
int dptx_postprocess_depth_batch(const void* y_dev, int32_t B, int32_t S, void* out512_dev, void* stream);
/* plt.imsave's normalisation and colormap look-up: maps [B][N] fp32, lut [256][4] uint8 (the caller's colormap) ->
 * rgba [B][N][4] uint8.  Per image lo / hi = exact min / max, n = (v - lo) / (hi - lo) in fp32 (0 when hi == lo),
 * index = min((int)(n * 256), 255); a non-finite value reads some entry of the LUT, never outside it.  Two launches; the
 * partial minima / maxima go through the workspace (512 * B bytes).  1 <= B <= 65535, 1 <= N <= 2^30. */
int dptx_colorize_workspace_bytes(int32_t B, int64_t N, int64_t* bytes);
int dptx_colorize_u8_batch(const void* maps_dev, const void* lut_dev, int32_t B, int64_t N, void* rgba_dev, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ---- Full-frame inference: the whole image in, a map of the image's own size out (no handle; DEVICE pointers unless stated) ----
 * The reference's whole-image protocol (paper_code/oasis_eval_tta.py:324-339: a fixed network size regardless of the aspect,
 * the prediction back to (orig_height, orig_width) with F.interpolate(mode='bilinear'), normalised again) and the aspect-
 * preserving network size DPT is normally run with (modules/midas/transforms.py:94-160, Resize.get_size with
 * keep_aspect_ratio=True, ensure_multiple_of=32).  Same conventions as the block above: stream-ordered, the caller's workspace
 * only, no allocation, no host synchronisation, no cache (graph-capturable), DPTX_E_INVALID before anything is launched; `descs`
 * is a HOST array read before the call returns; image i's result depends on image i only; no float atomics, bitwise
 * reproducible.
 *
 * dptx_preprocess_u8_rect_batch: B uint8 HWC images (C in {1, 3}) of one packed buffer -> x [B][3][OH][OW] fp32; per image
 * exactly ToTensor(img.resize((OW, OH), PIL.Image.BILINEAR)) -- the whole image, no crop, an independent scale per axis, either
 * axis up or down (Pillow's antialiased two-pass 8-bit resampler, bit-identical) -- then the optional Normalize(0.5, 0.5) and
 * the 1 -> 3 channel repeat.  Range: 1 <= B <= 4096; OH, OW multiples of 32 in [64, 1024]; 1 <= H, W <= 16384; H <= 32*OH;
 * W <= 32*OW; row_stride_bytes >= W*C.  Workspace: 8832 * (OH + OW) bytes, whatever B is (host-only). */
int dptx_preprocess_rect_batch_workspace_bytes(int32_t B, int32_t OH, int32_t OW, int64_t* bytes);
int dptx_preprocess_u8_rect_batch(const void* pixels_dev, const dptx_image_desc* descs, int32_t B, int32_t OH, int32_t OW,
                                  int32_t depth_normalize, void* x_dev, void* workspace, int64_t workspace_bytes, void* stream);
/* dptx_preprocess_u8_views_batch: dptx_preprocess_u8_rect_batch with a mirror per image -- the views of test-time augmentation.
 * A descriptor may be a WINDOW of an uploaded image: offset points at the window's first pixel, H / W are the window's and
 * row_stride_bytes is the parent's, so an image is uploaded once however many views it has; no byte outside a window's own
 * pixels is read.  flips: HOST array of B bytes (read before the call returns), NULL = no view is mirrored.  Per view exactly
 * ToTensor(ImageOps.mirror(img.crop(box).resize((OW, OH), BILINEAR))), bit-identical to Pillow: the mirror follows the resize
 * (the value of output column x is stored at column OW - 1 - x).  Ranges, workspace (dptx_preprocess_rect_batch_workspace_bytes)
 * and conventions are those of dptx_preprocess_u8_rect_batch; with flips = NULL so are the bits. */
int dptx_preprocess_u8_views_batch(const void* pixels_dev, const dptx_image_desc* descs, const uint8_t* flips, int32_t B, int32_t OH,
                                   int32_t OW, int32_t depth_normalize, void* x_dev, void* workspace, int64_t workspace_bytes,
                                   void* stream);
/* dptx_postprocess_resize_batch: y [B][C][h][w] fp32 -> B outputs of DIFFERENT sizes in one packed buffer.  descs[i] gives
 * output i: offset (bytes from out_dev), H, W and row_stride_bytes (rows may be padded; the field C is ignored); no byte outside
 * [row start, row start + W * bytes per pixel) of a row is written.  Source coordinates are ATen's (align_corners=False):
 * scale = in / out in fp32, src = scale * (dst + 0.5) - 0.5, clamped at 0 for bilinear only; an axis with in == out is copied.
 *   DPTX_RESIZE_NORMAL_U8   C = 3: bilinear (not antialiased: F.interpolate), clamp(0, 1) * 255 truncated -> [H][W][3] uint8
 *                           (demo.py:140,150 at the image's own size); 3 bytes per pixel, any byte alignment;
 *   DPTX_RESIZE_NORMAL_F32  C = 3: the same value unquantised, planar [3][H][W] fp32, planes H * row_stride_bytes apart;
 *   | DPTX_RESIZE_RENORM    (both NORMAL modes) after the interpolation and before the clamp: n = 2v - 1,
 *                           n^ = n / max(||n||_2, 1e-12) (F.normalize, oasis_eval_tta.py:339,441-445), re-encoded (n^ + 1) / 2;
 *   DPTX_RESIZE_DEPTH_F32   C = 1: bicubic (A = -0.75), clamp(0, 1), 1 - x (demo.py:143-145 at any size) -> [H][W] fp32;
 *   DPTX_RESIZE_DEPTH_RGBA  C = 1: the same, then plt.imsave's normalisation and look-up as dptx_colorize_u8_batch defines
 *                           them (lut_dev: [256][4] uint8) -> [H][W][4] uint8; per image min / max over exactly the
 *                           DPTX_RESIZE_DEPTH_F32 values, 64 partials per image through the workspace in a fixed order.
 * The 4-byte-per-pixel modes need offset, row_stride_bytes and out_dev to be multiples of 4.  lut_dev and the workspace
 * (16384 bytes, whatever B is; host-only) are used by DPTX_RESIZE_DEPTH_RGBA only and may be NULL / 0 otherwise.
 * Range: 1 <= B <= 4096; 1 <= h, w <= 4096; 1 <= H, W <= 16384; row_stride_bytes >= W * bytes per pixel. */
#define DPTX_RESIZE_NORMAL_U8 1
#define DPTX_RESIZE_NORMAL_F32 2
#define DPTX_RESIZE_DEPTH_F32 3
#define DPTX_RESIZE_DEPTH_RGBA 4
#define DPTX_RESIZE_RENORM 16
int dptx_postprocess_resize_workspace_bytes(int32_t B, int32_t mode, int64_t* bytes);
int dptx_postprocess_resize_batch(const void* y_dev, int32_t B, int32_t C, int32_t h, int32_t w, const dptx_image_desc* descs,
                                  int32_t mode, void* out_dev, const void* lut_dev, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/* ---- Guided upsampling: dptx_postprocess_resize_batch with edges where the image has them (DEVICE pointers unless stated) ----
 * Joint bilateral upsampling (Kopf et al. 2007): every output pixel is a weighted mean of the low-resolution map values around
 * it; the weights fall off with the distance and with the colour difference between the full-resolution image at the pixel and
 * the low-resolution image at the tap.  Conventions as above: stream-ordered, the caller's workspace only, no allocation, no host
 * synchronisation (graph-capturable), DPTX_E_INVALID before anything is launched; `guides`, `outs` and `params` are HOST data
 * read before the call returns; no atomics, bitwise reproducible; an image's result does not depend on the batch.
 *
 * Inputs, per image i of a batch that shares the network shape h x w:
 *   S     y_dev[i]: [C][h][w] fp32, already clamped to [0, 1] by the caller; C = 3 for the NORMAL modes, 1 for the DEPTH modes;
 *   G_lo  guide_lo_dev[i]: [3][h][w] fp32 in [0, 1], the image as the network saw it;
 *   G_hi  the image's own uint8 pixels at pixels_dev + guides[i].offset (C in {1, 3}, any row stride), g = u8 / 255 in fp32; a
 *         grey image uses its one channel three times.  guides[i].H, W equal outs[i].H, W;
 *   radius R in {1, 2, 3}, sigma_space > 0 in low-resolution pixels, sigma_range > 0 in [0, 1] colour units.  The host computes
 *   ks = 1 / (2 sigma_space^2) and kr = 1 / (2 sigma_range^2) in double and rounds each once to fp32 (both must come out positive and finite).
 * Output pixel (Y, X) of an H x W output; all arithmetic fp32, every operation rounded on its own (no contraction):
 *   1. sy = (h / H) * (Y + 0.5) - 0.5 and sx likewise: ATen's align_corners=False coordinate with scale = in / out in fp32, not
 *      clamped; by = floor(sy), bx = floor(sx).
 *   2. Taps qy in {by - R + 1, ..., by + R}, qx in {bx - R + 1, ..., bx + R}; a tap outside [0, h) x [0, w) is skipped, not
 *      replicated.  At least one tap is always inside.
 *   3. e_q = ks * ((qy - sy)^2 + (qx - sx)^2) + kr * sum_c (G_hi[c](Y, X) - G_lo[c](qy, qx))^2, c = 0, 1, 2 in order.
 *   4. e_min = the minimum over the valid taps; w_q = exp(-(e_q - e_min)): the largest weight is exactly 1 and the denominator
 *      lies in [1, 4 R^2].
 *   5. v_c = (sum_q w_q * S_c(q)) / sum_q w_q, both sums from 0 over the valid taps in (qy, qx) order.
 *   6. The mode's steps, exactly those of dptx_postprocess_resize_batch behind its interpolation: the NORMAL modes optionally
 *      DPTX_RESIZE_RENORM, then the clamp and the quantisation; DPTX_RESIZE_DEPTH_F32 clamp(0, 1), 1 - x; DPTX_RESIZE_DEPTH_RGBA
 *      min / max over exactly the DEPTH_F32 values (64 partials per image through the workspace in a fixed order), then the LUT.
 *   7. Inputs are assumed finite; non-finite ones neither fault nor hang and affect only the image they belong to.  The
 *      definition is total for any h, w, H, W in range: an output smaller than the map is allowed.
 * outs, out_dev, lut_dev, the workspace (16384 bytes for DPTX_RESIZE_DEPTH_RGBA, 0 otherwise; host-only) and the ranges are
 * those of dptx_postprocess_resize_batch; guides as for dptx_preprocess_u8_rect_batch (C in {1, 3}, row_stride_bytes >= W*C).
 * A guide whose H, W differ from its output's, C not in {1, 3}, a radius outside {1, 2, 3} or a sigma that is not positive
 * is DPTX_E_INVALID. */
typedef struct dptx_guided_params {
  int32_t radius;     /* 1, 2 or 3: (2 * radius)^2 taps */
  float sigma_space;  /* > 0, low-resolution pixels      */
  float sigma_range;  /* > 0, colour units of [0, 1]     */
} dptx_guided_params;
int dptx_postprocess_guided_workspace_bytes(int32_t B, int32_t mode, int64_t* bytes);
int dptx_postprocess_guided_batch(const void* y_dev, const void* guide_lo_dev, int32_t B, int32_t C, int32_t h, int32_t w,
                                  const void* pixels_dev, const dptx_image_desc* guides, const dptx_image_desc* outs,
                                  const dptx_guided_params* params, int32_t mode, void* out_dev, const void* lut_dev,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Training augmentations: the blur chain on the image and the crop / resize of a batch's task tensors (no handle; DEVICE
 * pointers unless stated) ----
 * The two steps of omnidata_tools/torch/data/augmentation.py:14-118 (augment_rgb, resize_augmentation) as kernels; the random
 * decisions stay with the caller (omnidata_amd/augmentation.py).  Conventions as above: stream-ordered, no workspace, no
 * allocation, no host synchronisation (graph-capturable), DPTX_E_INVALID before anything is launched; no atomics, bitwise
 * reproducible; an image's result does not depend on the batch.  All arithmetic fp32; "fma chain" below means acc = 0, then
 * acc = fma(weight, value, acc) for the taps in row-major order, one rounding per tap.
 *
 * dptx_augment_filter_chain: x [B][C][H][W] fp32 -> out, the same shape; every filter works per channel with the parameters of
 * its sample b.  The active stages (a non-NULL parameter pointer) run in the order sharpness, motion blur, Gaussian blur, each
 * on the previous stage's result and each with its own rule at the image border.  One launch.
 *   Sharpness, f = sharp_factor[b] (Pillow's ImageEnhance.Sharpness: SMOOTH filter, untouched border, blend):
 *     1. d(y, x) = fma chain of x over the 3 x 3 window around (y, x) with the weights fl(1/13), centre fl(5/13), for
 *        1 <= y <= H - 2 and 1 <= x <= W - 2; d = x on the one-pixel border and everywhere when H < 3 or W < 3;
 *     2. s = d + (x - d) * f: a subtraction, a product, a sum, each rounded;  f == 1: s = x, bit for bit.
 *   Motion blur, t = motion_taps[b] ([km][km], km in {3, 5, 7}; the caller builds and normalises the table):
 *     m(y, x) = fma chain over t[r][q] and s(y + r - km/2, x + q - km/2), a correlation; s is 0 outside the image.
 *   Gaussian blur, gy = gauss_y[b] ([kgy]), gx = gauss_x[b] ([kgx]), kgy, kgx in {1, 3, 5, 7}, H > kgy/2 and W > kgx/2:
 *     g(y, x) = fma chain over the weights gy[i] * gx[j] (one fp32 product) and m(R(y + i - kgy/2, H), R(x + j - kgx/2, W)) with
 *     the reflection R(i, n) = -i for i < 0, 2 (n - 1) - i for i >= n (F.pad's 'reflect': the edge is not repeated).
 *   A table that is the identity (one weight 1, the others 0) returns its stage's input for finite values.
 * out must not overlap x.  Range: 1 <= B, C; 1 <= H, W <= 16384; at least one stage; gauss_y and gauss_x both or neither.
 *
 * dptx_augment_resize_tasks: the same window or the same resize for every task tensor of a batch, in one launch.  `tasks` is a
 * HOST array of 1..8 descriptors read before the call returns: src [B][C][Hs][Ws] -> dst [B][C][h][w], contiguous, of 4-byte
 * (DPTX_AUG_F32) or 1-byte (DPTX_AUG_U8) elements; dst must not overlap src.
 *   DPTX_AUG_CROP    dst(y, x) = src(y0 + y, x0 + x), bit for bit; the window lies inside the source;
 *   DPTX_AUG_RESIZE  F.interpolate(src, (h, w)) with align_corners=False (y0, x0 ignored):
 *     DPTX_AUG_NEAREST   src(min((int)floorf(y * sh), Hs - 1), min((int)floorf(x * sw), Ws - 1)) with sh = (float)Hs / h,
 *                        sw = (float)Ws / w -- CPU ATen's index rule, bit for bit;
 *     DPTX_AUG_BILINEAR  (DPTX_AUG_F32 only) the coordinates and the blend of dptx_postprocess_resize_batch's bilinear modes:
 *                        s = max(sh * (y + 0.5) - 0.5, 0), i0 = min(floor(s), Hs - 1), i1 = i0 + (i0 < Hs - 1), l1 = s - i0,
 *                        l0 = 1 - l1 (an axis whose sizes agree copies); ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d),
 *                        every operation rounded on its own.
 * Range: 1 <= B, C; 1 <= Hs, Ws, h, w <= 16384. */
#define DPTX_AUG_F32 0
#define DPTX_AUG_U8 1
#define DPTX_AUG_BILINEAR 0
#define DPTX_AUG_NEAREST 1
#define DPTX_AUG_CROP 0
#define DPTX_AUG_RESIZE 1
#define DPTX_AUG_MAX_TASKS 8
typedef struct dptx_augment_task {
  const void* src; /* [B][C][Hs][Ws] */
  void* dst;       /* [B][C][h][w]   */
  int32_t C;
  int32_t dtype;   /* DPTX_AUG_F32 / DPTX_AUG_U8 */
  int32_t interp;  /* DPTX_AUG_BILINEAR / DPTX_AUG_NEAREST; read for DPTX_AUG_RESIZE only */
  int32_t reserved;
} dptx_augment_task;
int dptx_augment_filter_chain(const void* x_dev, int32_t B, int32_t C, int32_t H, int32_t W, const float* sharp_factor_dev,
                              const float* motion_taps_dev, int32_t km, const float* gauss_y_dev, const float* gauss_x_dev,
                              int32_t kgy, int32_t kgx, void* out_dev, void* stream);
int dptx_augment_resize_tasks(const dptx_augment_task* tasks, int32_t n_tasks, int32_t B, int32_t Hs, int32_t Ws, int32_t op,
                              int32_t y0, int32_t x0, int32_t h, int32_t w, void* stream);

/* ---- Test-time augmentation for surface normals: the merge of an image's views (no handle; DEVICE pointers unless stated) ----
 * The protocol of paper_code/oasis_eval_tta.py:440-448,487-534 (SurfaceNormalsTTAWrapper, MedianMerger): every view -- a window
 * of the image, possibly mirrored, at its own network size -- is mapped back into its window, and the views that cover a pixel
 * are merged per channel.  Same conventions as the blocks above: stream-ordered, no workspace, no allocation, no host
 * synchronisation (graph-capturable), DPTX_E_INVALID before anything is launched; `views` and `outs` are HOST arrays read before
 * the call returns; no atomics, a fixed order, bitwise reproducible; an image's result does not depend on the batch.
 *
 * View v is the network's map m [3][h][w] fp32 (values in [0, 1], contiguous) at views_dev + offset.  outs[i] describes output i
 * as in dptx_postprocess_resize_batch (offset from out_dev, H, W, row_stride_bytes; C ignored; no byte outside a row's own
 * pixels is written).  Output pixel (Y, X) of image i:
 *   1. the views of image i, in order, whose window [y0, y0 + ch) x [x0, x0 + cw) contains the pixel;
 *   2. n = 2m - 1 at the view's own resolution, then n / max(||n||_2, 1e-12) there unless DPTX_TTA_RAW_VIEWS
 *      (oasis_eval_tta.py:441-445; the OASIS z-sign change of line 442 is not reproduced);
 *   3. the value of F.interpolate(n, (ch, cw), mode='bilinear', align_corners=False) at (Y - y0, X - x0) -- with `flip` at
 *      (Y - y0, cw - 1 - (X - x0)) and the x component (channel 0) negated; coordinates as dptx_postprocess_resize_batch;
 *   4. per channel np.median over those values: the middle one or (a + b) * 0.5 of the two middle ones (NOT torch's lower
 *      median); with DPTX_TTA_MEAN the fp32 sum in view order divided by the count;
 *   5. F.normalize (eps 1e-12), (n + 1) / 2, then clamp and quantisation of DPTX_RESIZE_NORMAL_U8 / DPTX_RESIZE_NORMAL_F32;
 *   6. a pixel no view covers: the zero vector, encoded 0.5, 0.5, 0.5.
 * Inputs are assumed finite; non-finite ones neither fault nor hang (the affected pixels are unspecified).
 * mode = DPTX_RESIZE_NORMAL_U8 or DPTX_RESIZE_NORMAL_F32, | DPTX_TTA_MEAN, | DPTX_TTA_RAW_VIEWS; nothing else.
 * Range: 1 <= B <= 4096; every image has 1..64 views, consecutive in `views`, images ascending from 0 to B - 1 (so
 * B <= n_views <= 64 * B); 1 <= h, w <= 4096; offset >= 0 and a multiple of 4, as views_dev; the window inside the image;
 * outs as for dptx_postprocess_resize_batch.  One launch per image. */
typedef struct dptx_tta_view {
  int64_t offset;         /* bytes from views_dev to this view's [3][h][w] fp32 planes, contiguous, multiple of 4 */
  int32_t h, w;           /* the network's map for this view, 1..4096 */
  int32_t image;          /* output image it belongs to; views of one image are consecutive, images ascending */
  int32_t y0, x0, ch, cw; /* its window in the output image, inside [0,H) x [0,W) */
  int32_t flip;           /* the network saw the mirrored window */
} dptx_tta_view;
#define DPTX_TTA_MEAN 32
#define DPTX_TTA_RAW_VIEWS 64
#define DPTX_TTA_MAX_VIEWS 64
int dptx_tta_merge_normals(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const dptx_image_desc* outs,
                           int32_t B, int32_t mode, void* out_dev, void* stream);

/* ---- Test-time augmentation for depth: align the views to an anchor, then merge them (no handle; DEVICE pointers unless stated) ----
 * The network's depth is defined up to a scale and a shift per forward (it is trained with the least-squares alignment of
 * losses/midas_loss.py:10-30, compute_scale_and_shift), so the views of an image cannot be merged as they are: every view is
 * first fitted to one ANCHOR view that covers the whole image.  The reference has no depth TTA script; this block pins the
 * protocol.  Conventions as above: stream-ordered, the caller's workspace only, no allocation, no host synchronisation (graph-
 * capturable), DPTX_E_INVALID before anything is launched; `views`, `anchors` and `outs` are HOST arrays read before the call
 * returns; no float atomics, fixed orders, bitwise reproducible; an image's result does not depend on the batch.
 *
 * dptx_tta_view is reused; offset points at a [1][h][w] fp32 plane m.  For image i of size H x W:
 *   1. View value: d = clamp(m, 0, 1) at the network's resolution (demo.py:140); its value at image pixel (Y, X) of the window
 *      is that of F.interpolate(d, (ch, cw), mode='bilinear', align_corners=False) at (Y - y0, X - x0), with `flip` at
 *      (Y - y0, cw - 1 - (X - x0)); no sign changes.  Coordinates and blend order are those of dptx_tta_merge_normals.
 *   2. Anchor: anchors[i] is the index (into `views`) of a view of image i with y0 = x0 = 0, ch = H, cw = W.  Its coefficients
 *      are exactly (1, 0).
 *   3. Alignment of a view k that is not the anchor, over all n = ch * cw pixels of its window, r = the view's value and a = the
 *      anchor's value at the same image pixel (both fp32 as step 1 computes them): fp64 sums in a fixed order Sr, Srr, Sa, Sra;
 *      det = n Srr - Sr^2; scale = (n Sra - Sr Sa) / det, shift = (Srr Sa - Sr Sra) / det, solved in fp64 and rounded once to
 *      fp32.  A degenerate view, !(det > 1e-10 n Srr) (flatter than 1e-5 of its own level), gets scale = 1 and
 *      shift = (Sa - Sr) / n.  The scale is not clamped.
 *   4. Merge: the candidates scale_k * r_k + shift_k (an fp32 multiply, then an add) of the views that cover the pixel, in view
 *      order; np.median -- the middle one or (a + b) * 0.5 of the two middle ones -- or with DPTX_TTA_MEAN the fp32 sum in view
 *      order divided by the count; then clamp(0, 1) and 1 - x, the convention of DPTX_RESIZE_DEPTH_F32 -> [H][W] fp32 at
 *      outs[i] (offset, row_stride_bytes and out_dev multiples of 4).  coeffs_dev = NULL merges the views unaligned; a pixel
 *      no view covers (possible only then) is 0 before the inversion.
 *   5. Inputs are assumed finite; non-finite ones neither fault nor hang and affect only the image they belong to.
 * dptx_tta_align_depth writes coeffs_dev [n_views][2] fp32 (scale, shift).  Its workspace (dptx_tta_depth_workspace_bytes,
 * host-only; 8-byte aligned) holds every anchor resized to [H][W] fp32 and one record of the four sums per 64 x 16 tile of every
 * view's window; a view's records depend on its window alone.  dptx_tta_merge_depth samples the anchor from its view like any
 * other, so it reads nothing of `ws` (pass what the alignment wrote, or NULL).  mode = DPTX_RESIZE_DEPTH_F32, | DPTX_TTA_MEAN;
 * nothing else.  Ranges are those of dptx_tta_merge_normals; in addition an anchor index that is not a view of its image, or an
 * anchor that does not cover the whole image, is DPTX_E_INVALID. */
int dptx_tta_depth_workspace_bytes(const dptx_tta_view* views, int32_t n_views, const dptx_image_desc* outs, int32_t B,
                                   int64_t* bytes);
int dptx_tta_align_depth(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const int32_t* anchors,
                         const dptx_image_desc* outs, int32_t B, float* coeffs_dev, void* ws, int64_t ws_bytes, void* stream);
int dptx_tta_merge_depth(const void* views_dev, const dptx_tta_view* views, int32_t n_views, const float* coeffs_dev,
                         const dptx_image_desc* outs, int32_t B, int32_t mode, void* out_dev, const void* ws, void* stream);

/* ---- Tiled inference: overlapping tiles of one size, blended with feathered weights (no handle; DEVICE pointers unless stated) ----
 * An image of any size up to 16384 a side is cut into ny x nx windows of ch x cw pixels, every window goes through the network at
 * one network size h x w, and the maps are blended into a map of the image's own size.  The reference has no tiled script; this
 * block pins the protocol (omnidata_amd/tiled.py states the planner).  Conventions as above: stream-ordered, the caller's workspace
 * only, no allocation, no host synchronisation (graph-capturable), DPTX_E_INVALID before anything is launched; `grids` and `outs`
 * are HOST arrays (one entry per image) read before the call returns; no atomics, fixed orders, bitwise reproducible; an image's
 * result does not depend on the batch.  One blend launch per image, the grid by value in the kernel's arguments.
 *
 *   1. Grid: the starts y0[0 .. ny), x0[0 .. nx) ascend strictly, the first is 0, the last window ends at H / W, and neighbouring
 *      windows leave no gap (s[i + 1] <= s[i] + c).  Tile (iy, ix) is the window [y0[iy], y0[iy] + ch) x [x0[ix], x0[ix] + cw);
 *      its map m [C][h][w] fp32 (C = 3 normals, 1 depth) lies at views_dev + offset + (iy * nx + ix) * C * h * w * 4.
 *   2. Tile value: that of an unflipped view of the TTA merges.  Normals: n = 2m - 1, normalised at the network's resolution
 *      unless DPTX_TTA_RAW_VIEWS; depth: d = clamp(m, 0, 1).  Then the value of F.interpolate(., (ch, cw), mode='bilinear',
 *      align_corners=False) at the pixel's place in the window; coordinates and blend order as dptx_tta_merge_normals.
 *   3. Weight at local coordinate t in [0, c) of an axis with ramp r, start s and length L, in fp32:
 *        left  = (s == 0 || r == 0)     ? 1 : fminf(1, (t + 0.5f) / r)
 *        right = (s + c == L || r == 0) ? 1 : fminf(1, ((c - 1 - t) + 0.5f) / r)
 *      w_axis = left * right, w = w_y * w_x: an edge on the image border is not ramped, w > 0 everywhere in a window, and the sum of
 *      the weights at a pixel is >= 1.
 *   4. Blend over the tiles that cover the pixel, iy ascending, then ix ascending, every step an fp32 multiply, then an add:
 *      normals  acc_c += w * v_c; then F.normalize (eps 1e-12), (n + 1) / 2, clamp and quantisation of DPTX_RESIZE_NORMAL_U8 /
 *               DPTX_RESIZE_NORMAL_F32 (mode = one of them, | DPTX_TTA_RAW_VIEWS; nothing else);
 *      depth    acc += w * (scale_k * r_k + shift_k) (k = iy * nx + ix), wsum += w; then acc / wsum, clamp(0, 1) and 1 - x as
 *               DPTX_RESIZE_DEPTH_F32 (the only mode).  coeffs_dev = NULL blends the tiles unaligned, for comparison.
 *   5. Alignment (depth): the anchor -- the whole image's map [1][ah][aw] at views_dev + anchor_offset -- is used for the
 *      alignment only, it is not blended.  Every tile is fitted to it by step 3 of dptx_tta_align_depth, unchanged (the same
 *      device code: fp64 sums per 64 x 16 tile of the window, the degenerate rule, one rounding to fp32): a tile's coefficients
 *      equal, bit for bit, what dptx_tta_align_depth gives for the same window and anchor.
 *   6. Inputs are assumed finite; non-finite ones neither fault nor hang and affect only the image they belong to.
 * coeffs_dev: [tiles of image 0 | of image 1 | ...][2] fp32 (scale, shift), an image's tiles in grid order.  The workspace of
 * dptx_tile_align_depth (dptx_tile_depth_workspace_bytes, host-only; 8-byte aligned): every anchor resized to [H][W] fp32 and the
 * records of one chunk of at most 63 tiles.  Range: 1 <= B <= 4096; 1 <= ny, nx <= 64; 1 <= h, w, ah, aw <= 4096; offsets >= 0
 * and multiples of 4, as views_dev; ramps >= 0; outs as for dptx_tta_merge_normals / dptx_tta_merge_depth.  A grid that breaks
 * rule 1, and for dptx_tile_align_depth an image without an anchor, is DPTX_E_INVALID. */
#define DPTX_TILE_MAX_AXIS 64
typedef struct dptx_tile_grid {
  int64_t offset;          /* bytes to tile (0,0)'s [C][h][w] fp32 map; tile (iy,ix) at + (iy*nx+ix)*C*h*w*4 */
  int64_t anchor_offset;   /* depth: bytes to the anchor's [1][ah][aw] map; -1 = none */
  int32_t h, w, ch, cw;    /* every tile's network map and window size */
  int32_t ny, nx;          /* 1..64 each */
  int32_t ramp_y, ramp_x;  /* >= 0 */
  int32_t ah, aw;
  int32_t y0[64], x0[64];  /* ascending, first 0, last + c == H / W, no gap */
} dptx_tile_grid;          /* one per image */
int dptx_tile_blend_normals(const void* views_dev, const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B, int32_t mode,
                            void* out_dev, void* stream);
int dptx_tile_depth_workspace_bytes(const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B, int64_t* bytes);
int dptx_tile_align_depth(const void* views_dev, const dptx_tile_grid* grids, const dptx_image_desc* outs, int32_t B,
                          float* coeffs_dev, void* ws, int64_t ws_bytes, void* stream);
int dptx_tile_blend_depth(const void* views_dev, const dptx_tile_grid* grids, const float* coeffs_dev, const dptx_image_desc* outs,
                          int32_t B, int32_t mode, void* out_dev, void* stream);

/* ---- 3D refocus augmentation (omnidata_tools/torch/data/refocus_augmentation.py; no handle; DEVICE pointers) ----
 * All three are stream-ordered on `stream` and use only the caller's workspace: no allocation, no host synchronisation, no
 * host read of the radii (graph-capturable).  Shapes: B >= 1, C >= 1, 1 <= H, W <= 8192, H*W <= 2^24, n_quantiles >= 1;
 * rgb [B][C][H][W] and depth [B][1][H][W] fp32 contiguous.  Anything else -> DPTX_E_INVALID.
 * Host-only (no GPU needed): the workspace of dptx_refocus (dptx_refocus_quantiles needs its first part only, Q), with
 * R = 2(n+1), L = max(H, W) and A(x) = x rounded up to a multiple of 256:
 *   Q = A(B * (66048 + 12 R)),  T = A(8 * B * (n+1) * (L + 4)),  *bytes = Q + T + 4 * B * (n+1) * C * H * W. */
int dptx_refocus_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t n_quantiles, int64_t* bytes);
/* Replaces refocus_augmentation.py:82-88 with eps = 1e-4 and quantiles q_i = fp32(i) / fp32(n), i = 0..n (:187):
 * qvals [B][n+1] (already transposed as :189 does) = torch.quantile(depth.reshape(B, -1), q, dim=1) (linear) with
 * q_0 -= eps and q_n += eps.  Exact order statistics (radix select), ATen's rank / lerp arithmetic: the values of CPU
 * torch.quantile; -0.0 and +0.0 count as one value (+0.0). */
int dptx_refocus_quantiles(const float* depth, int32_t B, int32_t H, int32_t W, int32_t n_quantiles,
                           float* qvals /*[B][n+1], eps applied*/, void* ws, int64_t ws_bytes, void* stream);
/* Replaces refocus_image (:143-157) for the given quantiles, focus distances [B] and apertures [B]: radii (:77-79), the
 * separable Gaussian blur stack with cutoff 3r and replicate padding (:31-57, :104-120), segments (:90-101) and the
 * composite (:123-140).  out [B][C][H][W]; segments (nullable) [B][1][H][W] int64 = the left quantile index.  Results are
 * defined for radii that are finite with M = int(3r) (+1 if even) <= 2^24 and depths in (q_0, q_n], where the reference
 * itself runs (omnidata_amd/refocus.py raises ValueError otherwise); any other input stays in bounds. */
int dptx_refocus(const float* rgb, const float* depth, int32_t B, int32_t C, int32_t H, int32_t W, int32_t n_quantiles,
                 const float* qvals, const float* focus /*[B]*/, const float* aperture /*[B]*/,
                 float* out, int64_t* segments /*nullable*/, void* ws, int64_t ws_bytes, void* stream);

/* ---- MiDaS depth loss (omnidata_tools/torch/losses/midas_loss.py; no handle; DEVICE pointers) ----
 * Stream-ordered on `stream`, on the caller's workspace only: no allocation, no host synchronisation, no host read of any
 * count or median (graph-capturable).  No float atomics: results are bitwise reproducible and every per-image statistic
 * is the same alone and inside any batch.  pred, target [B][H][W] fp32 and mask [B][H][W] uint8 (0 / 1) contiguous;
 * shapes B >= 1, 1 <= H, W <= 8192, H*W <= 2^24, 1 <= scales <= 8.  Anything else -> DPTX_E_INVALID.
 * terms, an OR of:
 *   DPTX_MIDAS_SSI      the scale-and-shift-invariant MAE of SSIMAE (:104-111, :33-56): lower nanmedian t, s = sum |x - t| /
 *                       (n + 1), (x - t) / (s + 1e-6), masked L1 over the batch;
 *   DPTX_MIDAS_GRAD     the gradient-matching term of GradientMatchingTerm (:83-101, :114-134) over `scales` levels;
 *   DPTX_MIDAS_ALIGN    the gradient term sees scale * x + shift, least squares on the mask (compute_scale_and_shift, :10-30);
 *   DPTX_MIDAS_INVERSE  the gradient term and the alignment see 1 / (x + 1e-6) of prediction and target (:147-148).
 * MidasLoss = all four (DPTX_MIDAS_ALL).  Numerics: fp32 per-pixel values rounded step by step as the reference's fp32
 * tensors, fp64 sums and 2x2 solve; det == 0 exactly (e.g. a constant prediction on the mask) gives scale = shift = 0.
 * Host-only (no GPU needed): the workspace of all three calls, with A(x) = x rounded up to a multiple of 256 and
 * nblk = min(ceil(H*W / 4096), 1024):
 *   *bytes = A(256 + 8256 B) + A(80 B) + A(256 B) + A(128 B) + A(128 B nblk). */
#define DPTX_MIDAS_SSI 1
#define DPTX_MIDAS_GRAD 2
#define DPTX_MIDAS_ALIGN 4
#define DPTX_MIDAS_INVERSE 8
#define DPTX_MIDAS_ALL 15
#define DPTX_MIDAS_RECORD_DOUBLES 32 /* per image */
#define DPTX_MIDAS_STATS 8           /* floats per image of dptx_midas_stats */
int dptx_midas_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t scales, int64_t* bytes);
/* losses [3] fp32 = (total, ssi, reg): total = ssi + alpha * reg with both terms, else the one term (0 for the absent one).
 * reduction: image_based != 0 -> mean over images of L_k,b / M_k,b (MidasLoss's default), 0 -> sum L / sum M (batch-based).
 * record (nullable): [B][DPTX_MIDAS_RECORD_DOUBLES] per-image coefficients of the gradient, owned by the caller until the
 * matching dptx_midas_loss_backward; computed only when given.  alpha > 0 (the reference raises otherwise). */
int dptx_midas_loss(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t terms,
                    int32_t scales, int32_t image_based, float alpha, float* losses, double* record /*nullable*/, void* ws,
                    int64_t ws_bytes, void* stream);
/* grad_pred [B][H][W] = d(g0 total + g1 ssi + g2 reg) / d pred for grad_losses = (g0, g1, g2) [3] fp32 on the device, from the
 * record of the forward on the same inputs and arguments.  d|x| / dx = sign(x) with sign(0) = 0; the median passes its
 * gradient to the lowest linear index of a valid pixel holding the median value (-0.0 = +0.0); nothing flows through scale /
 * shift where det == 0.  No workspace. */
int dptx_midas_loss_backward(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W,
                             int32_t terms, int32_t scales, int32_t image_based, float alpha, const double* record,
                             const float* grad_losses, float* grad_pred, void* stream);
/* Per-image statistics, stats [B][DPTX_MIDAS_STATS] fp32: t_p, t_g, s_p, s_g, n, scale, shift, argmedian of pred (-1: none).
 * terms: DPTX_MIDAS_SSI (medians and s; 0 otherwise) and / or DPTX_MIDAS_ALIGN (+ DPTX_MIDAS_INVERSE) (scale and shift; 0
 * otherwise).  pred_aligned / target_aligned (nullable, SSI): (x - t) / (s + 1e-6) at every pixel (masked_shift_and_scale). */
int dptx_midas_stats(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t terms,
                     float* stats, float* pred_aligned /*nullable*/, float* target_aligned /*nullable*/, void* ws,
                     int64_t ws_bytes, void* stream);

/* ---- virtual normal loss (omnidata_tools/torch/losses/virtual_normal_loss.py, VNL_Loss; no handle; DEVICE pointers) ----
 * The third term of the reference's depth objective (train_depth.py:268-279).  Stream-ordered on `stream`, on the caller's
 * buffers only: no allocation, no host synchronisation, no host read of K or of the cut value.  Integer atomics only and
 * every floating-point sum in fp64 in a fixed order: results are bitwise reproducible, and the per-triple outputs of an
 * image are the same alone and inside any batch.
 * first, second [B][H][W] fp32 contiguous: the two arguments of VNL_Loss.forward in its order (the reference names them
 * gt_depth, pred_depth, and train_depth.py passes the prediction FIRST).  p1, p2, p3 [n] int32: linear pixel indices
 * y * W + x of the three points of every triple, shared by all images.  A triple with an index outside [0, H*W) reads
 * nothing and is dropped (not kept, no gradient): a non-zero return would need a synchronisation.
 * Per triple, in fp32 with every step rounded on its own as the reference's fp32 tensors:
 *   points   (x, y, z) = ((u - W/2) |d| / fx, (v - H/2) |d| / fy, d) (:44-50, integer W/2, H/2);
 *   kept     by the FIRST argument only (:95-128 with the constants of the call, :136-140): all three z > delta_z, and not
 *            (for each of x, y, z some pairwise difference is below 0.005 in magnitude), and not more than 3 of the 9 entries
 *            of <d_i, d_j> / (|d_i| |d_j| + 1e-8) over d = (P2-P1, P3-P1, P3-P2) beyond +-0.867;
 *   :144     on the SECOND argument: where point j (0, 1, 2) has z == 0, COORDINATE row j (x, y, z) of all three points
 *            becomes 0.0001 (the reference's index lands on that axis), and no gradient flows into those entries;
 *   normals  cross(P2-P1, P3-P1) / norm, a norm of exactly 0 replaced by 0.01; loss = sum_c |n_first,c - n_second,c|.
 * K = the number of kept triples of the batch.  select != 0: the int(K * 0.25) smallest losses are dropped and the rest
 * averaged; among kept triples whose loss EQUALS the cut value, the earliest in (image, triple) order are dropped first
 * (the order of a stable sort; the reference's torch.sort leaves it unspecified).  select == 0: the mean of all K.
 * K == 0 gives NaN and an all-zero gradient.  The masks, the 0.01 / 0.0001 replacements and the cut are piecewise constant:
 * no gradient through them; d|x| / dx = sign(x) with sign(0) = 0.
 * Shapes: B >= 1, 1 <= H, W <= 8192, H*W <= 2^24, 1 <= n <= 2^29, B*n < 2^31.  Anything else -> DPTX_E_INVALID.
 * Host-only (no GPU needed): the workspace of dptx_vnl_prepare (any B >= 1) and dptx_vnl_loss, with A(x) = x rounded up
 * to a multiple of 256, nblk = min(ceil(B n / 1024), 1024) and snb = min(ceil(3 n / 1024), 512):
 *   *bytes = 2 A(12 n) + A(1024 snb) + 4352 + A(40) + A(4 nblk) + A(8 nblk) + A(4 B n) + A(B n). */
#define DPTX_VNL_RECORD_HEADER 64 /* bytes */
int dptx_vnl_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n, int64_t* bytes);
/* The inverse index of one draw of triples, for the backward: inverse, uint32 [H*W + 6 n], owned by the caller and kept
 * with the indices: [H*W] 1 + the slot of the pixel's first entry (0: no triple uses it), then [3 n] pixels and [3 n]
 * entries 3 i + position, sorted by pixel and, within a pixel, ascending (a stable radix sort of the 3 n indices). */
int dptx_vnl_prepare(const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, int32_t H, int32_t W, uint32_t* inverse,
                     void* ws, int64_t ws_bytes, void* stream);
/* loss_out [1] fp32.  record (nullable; needed by the backward): [DPTX_VNL_RECORD_HEADER + B n] bytes owned by the caller
 * until the matching dptx_vnl_loss_backward: uint32 K, uint32 number dropped, uint32 bits of the cut value, uint32 number
 * dropped among the triples at the cut value, fp64 sum of the averaged losses, fp64 their number, fp32 loss; from byte
 * DPTX_VNL_RECORD_HEADER on, uint8 [B][n]: 1 where the triple is kept and not dropped. */
int dptx_vnl_loss(const float* first, const float* second, int32_t B, int32_t H, int32_t W, float fx, float fy, float delta_z,
                  const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, int32_t select, float* loss_out,
                  uint8_t* record /*nullable*/, void* ws, int64_t ws_bytes, void* stream);
/* grad_first / grad_second [B][H][W] fp32 (either may be null, not both) = grad_out[0] * d loss / d argument, from the record
 * of the forward on the same inputs and the inverse index of the same triples.  One thread per (image, pixel) adds the
 * closed-form gradients of the pixel's entries in the inverse index's order, in fp64 (the exact-zero-norm and z == 0
 * decisions are the forward's fp32 ones); pixels that no kept triple uses get 0.  No workspace. */
int dptx_vnl_loss_backward(const float* first, const float* second, int32_t B, int32_t H, int32_t W, float fx, float fy,
                           const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, const uint8_t* record,
                           const uint32_t* inverse, const float* grad_out, float* grad_first /*nullable*/,
                           float* grad_second /*nullable*/, void* stream);
/* Per-triple outputs for tests and debugging: keep uint8 [B][n], loss fp32 [B][n] (0 where not kept), normals (nullable)
 * fp32 [B][n][2][3]: the unit normals of the first and of the second argument.  No workspace. */
int dptx_vnl_triples(const float* first, const float* second, int32_t B, int32_t H, int32_t W, float fx, float fy, float delta_z,
                     const int32_t* p1, const int32_t* p2, const int32_t* p3, int32_t n, uint8_t* keep, float* loss,
                     float* normals /*nullable*/, void* stream);

/* ---- surface-normal loss (omnidata_tools/torch/train_normal.py:205-265, losses/masked_losses.py; no handle; DEVICE pointers) ----
 * The normal objective of the reference: normal_loss = cos_loss + 10 * l1_loss on the prediction clamped to [0, 1], with
 * its gradient with respect to the prediction; the flat masked losses; make_valid_mask.  Stream-ordered on `stream`, on
 * the caller's workspace only: no allocation, no host synchronisation, no host read of any count (graph-capturable).  No
 * atomics: every sum is fp64 in a fixed order that depends on the shape alone (not on the alignment of the pointers), so
 * results are bitwise reproducible.  pred, target [B][3][H][W] fp32 and mask [B][H][W] uint8 (0 / non-zero) contiguous;
 * shapes B >= 1, 1 <= H, W <= 8192, H*W <= 2^24; all indexing in 64 bits.  Anything else -> DPTX_E_INVALID.
 * Per valid pixel, in fp32 with every step rounded on its own as the reference's fp32 tensors (p = clamp(pred, 0, 1) first
 * with DPTX_NORMAL_CLAMP_PRED):
 *   x = clamp(2 p - 1, -1, 1), y the same of the target; xh = x / max(|x|, 1e-12) (F.normalize); cos term -(xh . yh);
 *   l1 terms |p_c - t_c|, c = 0, 1, 2.
 * N = the number of valid pixels; cos = sum of the cos terms / N, l1 = sum of the l1 terms / (3 N), sums in fp64, each
 * rounded to fp32 once; total = cos + l1_weight * l1 from the fp64 values, rounded once.  flags selects the terms
 * (DPTX_NORMAL_L1, DPTX_NORMAL_COS, at least one): an absent term is 0 and total is the present one.  N == 0 gives NaN for
 * every present term and for total, and an all-zero gradient.
 * Host-only (no GPU needed): the workspace, with A(x) = x rounded up to a multiple of 256, units = ceil(B H W / 4) and
 * nblk = min(ceil(units / 1024), 1024):
 *   *bytes = A(24 nblk). */
#define DPTX_NORMAL_L1 1
#define DPTX_NORMAL_COS 2
#define DPTX_NORMAL_CLAMP_PRED 4 /* pred -> clamp(pred, 0, 1) first (train_normal.py:251) */
#define DPTX_NORMAL_RECORD_DOUBLES 1
int dptx_normal_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes);
/* losses [3] fp32 = (total, l1, cos).  record (nullable; needed by the backward): [DPTX_NORMAL_RECORD_DOUBLES] fp64 owned
 * by the caller until the matching dptx_normal_loss_backward: N, the count alone. */
int dptx_normal_loss(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                     float l1_weight, float* losses, double* record /*nullable*/, void* ws, int64_t ws_bytes, void* stream);
/* grad_pred [B][3][H][W] = d(g0 total + g1 l1 + g2 cos) / d pred for grad_losses = (g0, g1, g2) [3] fp32 on the device, from
 * the record of the forward on the same inputs and arguments; the inputs are read again.  Evaluated in fp64 from the fp32
 * inputs and rounded once; the clamp, sign and eps decisions are the forward's fp32 ones.  d|x| / dx = sign(x) with
 * sign(0) = 0; a clamp passes its gradient where lo <= v <= hi, ends included (torch's rule), and nothing outside; through
 * max(|x|, eps) the gradient goes to |x| where |x| >= eps, (yh - (xh . yh) xh) / |x|, and the denominator is the constant
 * eps otherwise: a pixel whose scaled prediction is the zero vector has gradient -2 yh / (eps N) per component, the
 * reference's value.  Pixels outside the mask get 0.  No workspace. */
int dptx_normal_loss_backward(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W,
                              int32_t flags, float l1_weight, const double* record, const float* grad_losses, float* grad_pred,
                              void* stream);
/* Per-pixel terms for tests and debugging: cos [B][H][W] fp32 the cos term, l1 [B][H][W] fp32 the fp64 sum of the three l1
 * terms rounded once; 0 outside the mask.  Either may be null, not both.  flags: DPTX_NORMAL_CLAMP_PRED or 0.  No workspace. */
int dptx_normal_pixels(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                       float* cos /*nullable*/, float* l1 /*nullable*/, void* stream);
/* The flat per-element form: masked_l1_loss, masked_mse_loss and masked_loss of losses/masked_losses.py on n elements,
 * 1 <= n <= 2^40, with a mask per element: the fp64 sum of |p - t| (DPTX_MASKED_L1), of (p - t)^2 (DPTX_MASKED_MSE; the
 * difference and the square each rounded to fp32) or of p (DPTX_MASKED_VALUE: `pred` holds the element-wise loss, target is
 * NULL) over the mask, divided by its count N.  N == 0 gives NaN, or 0 with DPTX_MASKED_EMPTY_ZERO (masked_loss :28-29),
 * decided on the device.  record (nullable; needed by the backward): [1] fp64, N.  The gradient is sign(p - t) / N,
 * 2 (p - t) / N or 1 / N on the mask, times grad_loss[0], and 0 elsewhere and where N == 0.
 * Host-only: the workspace, with units = ceil(n / 4) and nblk = min(ceil(units / 1024), 1024): *bytes = A(24 nblk). */
#define DPTX_MASKED_L1 0
#define DPTX_MASKED_MSE 1
#define DPTX_MASKED_VALUE 2
#define DPTX_MASKED_EMPTY_ZERO 4 /* OR-ed into kind */
int dptx_masked_workspace_bytes(int64_t n, int64_t* bytes);
int dptx_masked_loss(const float* pred, const float* target /*NULL for VALUE*/, const uint8_t* mask, int64_t n, int32_t kind,
                     float* loss, double* record /*nullable*/, void* ws, int64_t ws_bytes, void* stream);
int dptx_masked_loss_backward(const float* pred, const float* target, const uint8_t* mask, int64_t n, int32_t kind,
                              const double* record, const float* grad_loss, float* grad_pred, void* stream);
/* make_valid_mask (train_normal.py:205-232): valid [B][H][W] uint8 = 1 where the maximum of 1 - mask_float over the pixel's
 * pool x pool window is exactly 0 (a NaN in the window: 0).  With Hp = H / pool, Wp = W / pool (integer division), the window
 * of pixel (i, j) is row min(floor(i * (float(Hp) / float(H))), Hp - 1) and the like column of the pooled grid (max_pool2d,
 * then F.interpolate(mode='nearest') back to H x W): rows and columns beyond pool * Hp are never pooled and take their nearest
 * pooled window.  Requires H, W >= pool >= 1.  No workspace. */
int dptx_valid_mask(const float* mask_float, int32_t B, int32_t H, int32_t W, int32_t pool, uint8_t* valid, void* stream);

/* ---- evaluation metrics (paper_code/evaluation_metrics.py:13-106, get_metrics for task='normal' and 'depth_zbuffer'; no
 * handle; DEVICE pointers) ----
 * Forward only.  Stream-ordered on `stream`, on the caller's workspace only: no allocation, no host synchronisation, no
 * host read of the mask count.  pred, target [B][C][H][W] fp32 (C = 3 normal, 1 depth) and mask [B][H][W] uint8
 * (0 / non-zero) contiguous; B >= 1, 1 <= H, W <= 8192, H*W <= 2^24 and B*H*W < 2^32.  A null pointer, an unknown flag, a
 * workspace that is too small or another shape -> DPTX_E_INVALID, before anything is launched.
 * Rows: one for the whole batch (the reference's call), or with DPTX_EVAL_PER_IMAGE one per image, each what the
 * reference returns for that image alone (paper_code/test_normal.py:377-389 calls it per image).  A per-image row does not
 * depend on B or on the image's place in the batch, and equals the batch row of a B = 1 call bit for bit.
 * Every per-pixel term is evaluated in fp64 on the fp32 inputs (:18-19 .double()), each operation rounded on its own, for
 * EVERY pixel, and multiplied by the 0 / 1 mask as the reference does: a non-finite term outside the mask poisons its sum
 * exactly as there (a masked-out pixel with target == 0 makes rel_error NaN).  Sums are fp64 in an order fixed by (H, W)
 * alone; there are no float atomics, so results are bitwise reproducible.  With n = the number of valid pixels of the row
 * and numel = all its pixels:
 *   normal (:33-59)  cos = (p . t) / max(|p| |t|, 1e-8) clamped to [-1, 1], ang = acos(cos) * (180 / pi);
 *     out row [DPTX_EVAL_NORMAL_FIELDS] = n, ang_error_mean = sum(ang m) / n, ang_error_median, ang_error_without_masking =
 *     sum(ang) / numel, the fractions of the valid pixels with ang <= 11.25, 22.5, 30 (a NaN compares false), eval_L1 and
 *     eval_mse = 100 (numel / n) mean over pixels and channels of d and of d^2, d = |p / (|p| + 2e-2) - t / (|t| + 2e-2)| m.
 *     ang_error_median is the exact np.median (:50) of the valid pixels' angles -- the value of rank floor((n - 1) / 2) for
 *     odd n, (a + b) * 0.5 of ranks n / 2 - 1 and n / 2 for even n --, found by a radix select on 64-bit order-preserving
 *     keys (8 passes of 8 bits, integer histograms); NaN if any valid pixel's angle is NaN, as np.median answers.
 *   depth (:61-79)  d = |p - t| m, dlog = |(log(1 + 64 p) - log(1 + 64 t)) m|;
 *     out row [DPTX_EVAL_DEPTH_FIELDS] = n, eval_L1 and eval_mse = 100 (numel / n) mean of d and of d^2, log10_diff =
 *     (numel / n) mean(log(1 + 64 d) m), log10 = (numel / n) mean(dlog), si_log = sum(dlog^2) / n - sum(dlog)^2 / n^2,
 *     rel_error = (numel / n) mean((d / t) m), irmse = (numel / n) mean((1 / (1 + 64 p) - 1 / (1 + 64 t))^2 m).
 * A row with an empty mask gets n = 0 and NaN in every other field, decided on the device (:30-31 returns None).
 * Host-only (no GPU needed): the workspace, with A(x) = x rounded up to a multiple of 256, units = ceil(H W / 4) and
 * nblk = min(ceil(units / 256), 1024):
 *   *bytes = A(8 B H W) + A(72 B nblk) + 16384 B + A(192 B)
 * (the keys, the partial sums, and per possible row the histograms and the select states).  The call clears what it needs in stream order, so
 * one workspace serves any sequence of calls of its shape ON ONE STREAM AT A TIME: two calls in flight on two streams need
 * two workspaces.  The size is one per shape for both tasks: dptx_eval_depth asks for it too but never touches the key
 * region, the histograms or the states (at B = 32, 384 x 384 about 38 MB of the 40 MB); a caller that evaluates depth only
 * pays that for the single size function. */
#define DPTX_EVAL_PER_IMAGE 1     /* rows = B (one per image); otherwise rows = 1 (the whole batch) */
#define DPTX_EVAL_NORMAL_FIELDS 9 /* count, ang_error_mean, ang_error_median, ang_error_without_masking, within_11.25,
                                     within_22.5, within_30, eval_L1, eval_mse */
#define DPTX_EVAL_DEPTH_FIELDS 8  /* count, eval_L1, eval_mse, log10_diff, log10, si_log, rel_error, irmse */
int dptx_eval_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes);
int dptx_eval_normal(const float* pred, const float* target /*[B,3,H,W]*/, const uint8_t* mask /*[B,H,W]*/, int32_t B, int32_t H,
                     int32_t W, int32_t flags, double* out /*[rows][9]*/, void* ws, int64_t ws_bytes, void* stream);
int dptx_eval_depth(const float* pred, const float* target /*[B,1,H,W]*/, const uint8_t* mask /*[B,H,W]*/, int32_t B, int32_t H,
                    int32_t W, int32_t flags, double* out /*[rows][8]*/, void* ws, int64_t ws_bytes, void* stream);
/* Per-pixel angles for tests and debugging (:43): ang [B][H][W] fp64, degrees, the mask not applied.  No workspace. */
int dptx_eval_normal_pixels(const float* pred, const float* target, int32_t B, int32_t H, int32_t W, double* ang, void* stream);

/* ---- scale-and-shift-aligned depth evaluation (no handle; DEVICE pointers) ----
 * The depth network's output is defined up to a scale and a shift per image, so a depth checkpoint is judged on the
 * prediction FITTED to the ground truth per image.  One call: the fit of every image, then every metric of the fitted
 * prediction.  Same contract as the two sections it composes (MiDaS statistics, evaluation metrics): stream-ordered on
 * `stream`, on the caller's workspace only, no allocation, no host synchronisation, no float atomics, bitwise reproducible,
 * a per-image row the same alone and inside any batch.  Shapes as dptx_eval_depth.  A null pointer (`aligned` excepted),
 * an unknown `align` or `flags` bit, a min_depth that is not positive and finite, a workspace that is too small or another
 * shape -> DPTX_E_INVALID, before anything is launched.
 * Coefficients, per image, from the stages of dptx_midas_stats (the same bits):
 *   DPTX_EVAL_ALIGN_LSTSQ   scale, shift of compute_scale_and_shift(pred, target, mask) (midas_loss.py:10-30; DPTX_MIDAS_ALIGN),
 *                           (0, 0) where det == 0;  aligned = scale p, then + shift;
 *   DPTX_EVAL_ALIGN_MEDIAN  t_p, t_g, s_p, s_g of masked_shift_and_scale (:33-56; DPTX_MIDAS_SSI);  aligned =
 *                           (p - t_p) / (s_p + 1e-6f), then (s_g + 1e-6f) times that, then + t_g.
 * fp32, every step rounded on its own; with DPTX_EVAL_ALIGNED_CLAMP then clamped to [0, 1] (paper_code/test_depth.py:207; a NaN
 * stays a NaN).  coeffs [B][2] fp32 = scale, shift; for MEDIAN the equivalent pair ((s_g + 1e-6f) / (s_p + 1e-6f), t_g - that
 * t_p), for reporting only.  aligned (nullable) [B][1][H][W] receives the aligned value of every pixel, masked or not.
 * out [B + 1][DPTX_EVAL_ALIGNED_FIELDS] fp64: rows 0 .. B - 1 the images, row B the whole batch (the reference's get_metrics
 * on the stacked aligned batch), all from one pass.
 *   Fields 0-7: the row of dptx_eval_depth for the aligned tensor, bit for bit (rows 0 .. B - 1: with DPTX_EVAL_PER_IMAGE; row
 *   B: without): the same per-pixel fp64 arithmetic, block partition and summation order.
 *   Fields 8-14, over the valid pixels only (selected by the mask, not multiplied by it), in fp64 with a_e = max(aligned,
 *   min_depth), t_e = max(target, min_depth): abs_rel = mean |a_e - t_e| / t_e, sq_rel = mean (a_e - t_e)^2 / t_e, rmse =
 *   sqrt(mean (a_e - t_e)^2), rmse_log = sqrt(mean (ln a_e - ln t_e)^2), delta1..3 = the fraction with max(a_e / t_e,
 *   t_e / a_e) < 1.25, 1.5625, 1.953125 (a NaN compares false).
 *   The delta counts are integers (counted per thread, exact in the fp64 rows of partial sums).
 * A row with an empty mask gets n = 0 and NaN elsewhere, decided on the device.  Every other row is finite for finite inputs
 * with one exception inherited from dptx_eval_depth: rel_error (field 6) divides by the target, so a VALID pixel with target
 * == 0 makes it +inf (NaN if the aligned value is 0 there too) in its image's row and in row B; fields 8-14 floor the target
 * and stay finite.  Inputs are assumed finite; non-finite ones touch only their own image's rows and row B.
 * Host-only (no GPU needed): the workspace, with A(x) = x rounded up to a multiple of 256, nblk = min(ceil(ceil(H W / 4) /
 * 256), 1024) (the blocks of dptx_eval_depth) and M = what dptx_midas_workspace_bytes(B, H, W, 1, .) gives:
 *   *bytes = A(120 B nblk) + A(32 B) + M
 * (the partial sums, the per-image statistics, the workspace of the statistics' stages).  One stream at a time per
 * workspace, as above. */
#define DPTX_EVAL_ALIGN_LSTSQ 1
#define DPTX_EVAL_ALIGN_MEDIAN 2
#define DPTX_EVAL_ALIGNED_CLAMP 1   /* flags: clamp the aligned value to [0, 1] */
#define DPTX_EVAL_ALIGNED_FIELDS 15 /* the 8 of DPTX_EVAL_DEPTH_FIELDS, abs_rel, sq_rel, rmse, rmse_log, delta1, delta2, delta3 */
int dptx_eval_aligned_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes);
int dptx_eval_depth_aligned(const float* pred, const float* target /*[B,1,H,W]*/, const uint8_t* mask /*[B,H,W]*/, int32_t B,
                            int32_t H, int32_t W, int32_t align, int32_t flags, float min_depth, double* out /*[B + 1][15]*/,
                            float* coeffs /*[B][2]*/, float* aligned /*nullable*/, void* ws, int64_t ws_bytes, void* stream);

/* ---- op-level entry points (unit tests + micro-benchmarks of the individual kernels) ----
 * dtype: DPTX_DTYPE_*.  All pointers are device pointers; row-major / NHWC. */

/* For dtype = DPTX_DTYPE_BF16X3 the op entry points read/write hi/lo plane pairs: the lo plane of
 * every activation (weight) tensor lies act_plane_elems (w_plane_elems) 16-bit elements after its
 * hi plane.  Process-global, test use only. */
int dptx_op_set_planes(int64_t act_plane_elems, int64_t w_plane_elems);

/* C[M,N] = act(A[M,K] * W[N,K]^T + bias) (+R); A,W,C,R 16-bit `dtype`; bias fp32 or NULL;
 * act: 0 none, 1 relu, 2 gelu(erf); c_fp32/r_fp32 select fp32 C / R. */
int dptx_op_gemm(int32_t dtype, const void* A, const void* W, const float* bias, const void* R,
                 void* C, int32_t M, int32_t N, int32_t K, int32_t act, int32_t a_fp32,
                 int32_t c_fp32, int32_t r_fp32, void* stream);
/* NHWC conv as implicit GEMM: X[B,H,W,Cin], Wt[Cout][k][k][Cin], Y[B,Ho,Wo,Cout]. */
int dptx_op_conv(int32_t dtype, const void* X, const void* Wt, const float* bias, const void* R,
                 void* Y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                 int32_t ksize, int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho,
                 int32_t Wo, int32_t a_relu, int32_t act, void* stream);
/* the same convolution with the plane switches of the MIXED dtype's per-layer policy (kernels.h GemmParams::epi2 /
 * c_hi_only / r1_hi_only / a_hi_only): epi2 = 1 with dtype FP16 multiplies the hi planes only but reads R and writes Y as hi/lo
 * pairs; epi2 = 2 with dtype FP16X3 is the 2-MFMA form (both planes of Wt, the hi plane of X only) */
int dptx_op_conv_planes(int32_t dtype, const void* X, const void* Wt, const float* bias, const void* R, void* Y, int32_t B,
                        int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad_t,
                        int32_t pad_l, int32_t Ho, int32_t Wo, int32_t a_relu, int32_t act, int32_t epi2, int32_t c_hi_only,
                        int32_t r1_hi_only, void* stream);
/* Fused stem: x NCHW fp32 [B,3,H,W] -> y NHWC 16-bit [B,H/2,W/2,64] = conv 7x7 stride 2 with TF-SAME padding;
 * Wt [64][176] 16-bit with k = (c*7 + ky)*8 + kx (kx = 7 and k >= 168 are zero).  H % 8 == 0, W % 128 == 0. */
int dptx_op_stem_conv(int32_t dtype, const float* x, const void* Wt, void* y, int32_t B, int32_t H, int32_t W,
                      void* stream);
/* The same with a caller image of element type io (DPTX_IO_FP32 / _BF16 / _FP16). */
int dptx_op_stem_conv_io(int32_t dtype, const void* x, int32_t io, const void* Wt, void* y, int32_t B, int32_t H, int32_t W,
                         void* stream);
/* qkv[B*S,3*H*64] packed (which, head, dim) -> out[B*S,H*64]; softmax(q k^T / 8) v. */
int dptx_op_attention(int32_t dtype, const void* qkv, void* out, int32_t B, int32_t S,
                      int32_t heads, void* stream);
/* y16[M,C] = LayerNorm(x32[M,C]; gamma, beta, eps), C = 768 or 1024 */
int dptx_op_layernorm(int32_t dtype, const float* x, const float* gamma, const float* beta,
                      void* y, int32_t M, int32_t C, float eps, void* stream);
/* GroupNorm(32) (+ optional residual R, + optional ReLU) on NHWC 16-bit, out of place.  scratch_f32 receives the
 * per-block partial sums: B * ceil(HW / pix) * 64 floats with pix = clamp(16384 / C, 16, 256). */
int dptx_op_groupnorm(int32_t dtype, const void* X, const float* gamma, const float* beta,
                      const void* R, void* Y, int32_t B, int32_t HW, int32_t C, int32_t relu,
                      float eps, void* scratch_f32, void* stream);
/* The stem's GroupNorm(32) + ReLU + MaxPool2dSame(3, 2) on NHWC 16-bit: Y[B,H/2,W/2,C] = maxpool(relu(gn(X[B,H,W,C]))) with
 * SAME padding (0, 1) of -inf.  H and W even (odd sizes -> DPTX_E_INVALID); scratch_f32 as for dptx_op_groupnorm. */
int dptx_op_gn_relu_maxpool(int32_t dtype, const void* X, const float* gamma, const float* beta, void* Y, int32_t B,
                            int32_t H, int32_t W, int32_t C, float eps, void* scratch_f32, void* stream);
/* The cls rows of the token stream (vit.py:141-147): row b*S of X (fp32, may be NULL) = cls + pos[0..C); X16 (optional): its
 * 16-bit copy; row_stats (optional): its (sum, sum of squares) per 128-column block as float2 records row_stats[b*S][0 .. C/128)
 * (row stride 8 records, so C <= 1024 with row_stats); X8 (optional): its e4m3 copy of (value * q_scale).  C % 128 == 0.  Other
 * rows are not touched. */
int dptx_op_cls_rows(int32_t dtype, const float* cls, const float* pos, float* X, int32_t B, int32_t S, int32_t C, void* X16,
                     float* row_stats, void* X8, float q_scale, void* stream);
/* Debug: s_memtime stamps of the GEMM k-loop (block 0, lane 0 of each wave; [wave][64 k-tiles][4 phases] int64) into a
 * device buffer of 8*64*4 int64 for every following GEMM launch; NULL switches it off (tools/gpu/gemm_trace.py). */
int dptx_debug_set_trace(void* dev_buf);
/* Debug / tests (tests/test_gpu_poison.py): the activation arena of a handle.  A forward must not read an arena byte it
 * has not written itself -- dptx_debug_arena_fill sets every byte of the arena (all planes) to byte_value (0xFF: NaN in
 * every element type used) after a device synchronisation; the next forward's result must not change.
 * dptx_debug_arena_read copies a byte range to the host; dptx_debug_arena_layout writes "key value" / "buf name off bytes
 * off2" lines (off: whole-batch plan, off2: inside a sub-batch region of the multi-stream plan) and returns the size needed. */
int dptx_debug_arena_fill(dptx_handle h, int32_t byte_value);
int dptx_debug_arena_read(dptx_handle h, void* dst_host, size_t offset, size_t bytes);
int dptx_debug_arena_layout(dptx_handle h, char* dst, size_t capacity);
/* One 64-bit word sum per arena buffer, sub-batch region and plane of the layout the LAST forward used, computed on `stream`
 * behind that forward: out_dev[(plane * regions + region) * nbuf + buf] (uint64, device memory), buffers in the order of
 * dptx_debug_arena_layout.  Returns the number of sums; with out_dev = NULL the capacity needed.  Two forwards of one input
 * must give the same vector; the first entry that differs names the tensor. */
int dptx_debug_arena_checksums(dptx_handle h, void* out_dev, int32_t capacity, void* stream);
/* Debug / tests: switches (per calling host thread) of the 256x256 GEMM kernel's launch form -- 1: staged epilogue instead of the
 * register-direct one, 2: one block per tile instead of the persistent tile loop, 4: the lockstep loop instead of the ping-pong
 * schedule in the two-plane 128x128 kernel -- and of the streaming kernel for the small-K 1x1 convolutions -- 8: never take it,
 * 16: take it for every launch it can serve, not only in the shape classes it was adopted for -- and of the forward's
 * folding of norm3 into a second pass of that kernel -- 32: never (conv3, then the GroupNorm apply pass), 64: wherever the
 * folded form can run, not only in the shape classes it was adopted for -- and of the stem convolution and the x2 up-sampling --
 * 128: both on their first kernels everywhere, 256: the strip form of the up-sampling wherever it can run, not only in the
 * (H, C) classes it was adopted for.  Results do not depend on them. */
int dptx_debug_set_gemm_flags(int32_t flags);
/* NHWC conv on OCP e4m3 operands (the fp8 dtype's convolution): X8[B,H,W,Cin] and Wt8[Cout][k][k][Cin] are e4m3 bytes
 * (Cin % 128 == 0), fp32 accumulate on the block-scaled fp8 MFMA at unit scale; Y = act(out_scale * conv + bias) (+R) in
 * bf16; Y8 (optional) receives the e4m3 copy of Y (ReLU'd first when q_relu). */
int dptx_op_conv_fp8(const void* X8, const void* Wt8, const float* bias, const void* R, void* Y, void* Y8, int32_t B,
                     int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t pad_t,
                     int32_t pad_l, int32_t Ho, int32_t Wo, int32_t act, int32_t q_relu, float out_scale, void* stream);
/* Bias-free convolution followed by GroupNorm(32) (+ residual R, + ReLU) the way the ResNetV2 stages run it: the
 * statistics come out of the conv's GEMM epilogue (fp32 accumulators, one record per 32-row block and group, fixed
 * order), the apply pass normalises the stored 16-bit map.  Yraw receives the conv output, Y the normalised result
 * (Y == Yraw allowed).  Ho*Wo % 32 == 0, Cout % 64 == 0; scratch_f32: B * (Ho*Wo/32) * 64 floats. */
int dptx_op_conv_groupnorm(int32_t dtype, const void* X, const void* Wt, void* Yraw, const float* gamma, const float* beta,
                           const void* R, void* Y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                           int32_t ksize, int32_t stride, int32_t pad_t, int32_t pad_l, int32_t Ho, int32_t Wo,
                           int32_t relu, float eps, void* scratch_f32, void* stream);
/* The same result for a 1x1 stride-1 convolution with Cin in {64, 128, 256} (bf16 / fp16), computed the way the forward
 * folds norm3 into its conv3: the streaming kernel runs twice -- a statistics pass that writes the records and nothing else,
 * a finalize launch that turns them into per-(image, channel) affines, and a second pass that multiplies again and applies
 * GroupNorm + R + ReLU in its epilogue -- so that the raw map is never stored.  Y = act( gn(conv(X)) + R' ), R' = R, or
 * gn_r(R) with (r_gamma, r_beta) and the records r_records of R (as dptx_op_conv_groupnorm leaves them in its scratch) --
 * the first block of a stage, whose shortcut is the downsample branch.  Bit-identical to dptx_op_conv_groupnorm.
 * records_f32: B * (H*W/32) * 64 floats; tables_f32: B * 4 * Cout floats.  H*W % 32 == 0, Cout % 64 == 0, Y != R.
 * passes: 1 = statistics pass (Y is not touched), 2 = finalize, 4 = epilogue pass; 7 = all three. */
int dptx_op_conv_groupnorm_fused(int32_t dtype, const void* X, const void* Wt, const float* gamma, const float* beta,
                                 const void* R, const float* r_gamma, const float* r_beta, const float* r_records, void* Y,
                                 int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t relu, float eps,
                                 void* records_f32, void* tables_f32, int32_t passes, void* stream);
/* The apply pass of dptx_op_conv_groupnorm alone, from caller-supplied records -- the launch the forward's gn_apply makes
 * behind a convolution that wrote GroupNorm records: Y = act( gn(X) + R' ) of the stored 16-bit map X [B][HW][C] with the
 * statistics of records[B][HW/32][32][2] ((sum, sum of squares) per 32-row block and group, as the convolution's epilogue
 * leaves them), R' = nothing (R null), R, or gn_r(R) with (r_gamma, r_beta) and the records r_records of R.  Y == X allowed.
 * HW % 32 == 0, C % 64 == 0, C <= 1024; r_gamma, r_beta and r_records come together and need R. */
int dptx_op_groupnorm_records(int32_t dtype, const void* X, const float* gamma, const float* beta, const float* records,
                              const void* R, const float* r_gamma, const float* r_beta, const float* r_records, void* Y,
                              int32_t B, int32_t HW, int32_t C, int32_t relu, float eps, void* stream);
/* bilinear x2, align_corners=True, NHWC 16-bit. */
int dptx_op_upsample2x(int32_t dtype, const void* X, void* Y, int32_t B, int32_t H, int32_t W,
                       int32_t C, void* stream);
/* The strip form of that kernel alone (dtype 0 / 1): a thread emits `rows` (4 or 8) output rows from rows / 2 + 2 source rows. */
int dptx_op_upsample2x_strip(int32_t dtype, const void* X, void* Y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t rows,
                             void* stream);
/* Dense GEMM with the consumer epilogue of the LayerNorm fold (what the qkv / fc1 launches run): C[M,N] (16-bit) =
 * act((A[M,K] W[N,K]^T - mu colsum) rstd + bias), with (mu, rstd) of row m combined from the (sum, sum of squares) records
 * ln_stats[m][0 .. ln_nblk) (float2, row stride 8 records; ln_nblk = K / 128 = 6 or 8) and ln_colsum[n] = sum_k W[n][k]. */
int dptx_op_gemm_ln(int32_t dtype, const void* A, const void* W, const float* bias, void* C, int32_t M, int32_t N, int32_t K,
                    int32_t act, const float* ln_stats, const float* ln_colsum, int32_t ln_nblk, float ln_eps, void* stream);
/* Dense GEMM with the PRODUCER epilogue of the LayerNorm fold on the 16-bit token stream (what the proj / fc2 launches run,
 * vit.py:150-151 x = x + attn(...) / x + mlp(...)): C[M,N] (16-bit) <- C + A[M,K] W[N,K]^T + bias in place, and the (sum, sum of
 * squares) of every new row per 128-column block as float2 records row_stats[m][0 .. N / 128) (row stride 8 records; N a
 * multiple of 128, <= 1024). */
int dptx_op_gemm_stream(int32_t dtype, const void* A, const void* W, const float* bias, void* C, float* row_stats, int32_t M,
                        int32_t N, int32_t K, void* stream);
/* The same on the fp32 token stream (the parity mode's ViT blocks): X[M,N] (fp32) <- X + A W^T + bias in place, the 16-bit image
 * of the new rows into C16 (what the next qkv / fc1 GEMM multiplies), records as above. */
int dptx_op_gemm_stream32(int32_t dtype, const void* A, const void* W, const float* bias, float* X, void* C16, float* row_stats,
                          int32_t M, int32_t N, int32_t K, void* stream);
/* Fused tail of the head (dpt_depth.py:93-98): Interpolate(x2, bilinear, align_corners=True) -> Conv2d(128,32,3,pad 1)
 * -> ReLU -> Conv2d(32,C,1) -> ReLU(if relu_out).  H0 NHWC 16-bit [B,Hs,Ws,128]; W2 16-bit [32][3][3][128]
 * (O,kh,kw,I); b2 fp32[32]; w4 fp32 [C][32]; b4 fp32[C]; y NCHW fp32 [B,C,2Hs,2Ws].  BF16 / FP16 only; C <= 3. */
int dptx_op_head_tail(int32_t dtype, const void* H0, const void* W2, const float* b2, const float* w4,
                      const float* b4, float* y, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                      int32_t relu_out, void* stream);
/* The same with a result of element type io (DPTX_IO_FP32 / _BF16 / _FP16; anything else -> DPTX_E_INVALID): the fp32 value
 * rounded to nearest, as the forward stores a 16-bit result image. */
int dptx_op_head_tail_io(int32_t dtype, const void* H0, const void* W2, const float* b2, const float* w4,
                         const float* b4, void* y, int32_t io, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                         int32_t relu_out, void* stream);
/* The 1x1 projection of the three-launch tail (dpt_depth.py:96-98): X [B*HW][32] 16-bit (a hi/lo pair for BF16X3 / FP16X3,
 * planes of dptx_op_set_planes) -> y NCHW [B][Cout][HW] of element type io = w X + b, ReLU if relu.  w fp32 [Cout][32],
 * b fp32 [Cout].  Cout outside 1..4, B < 1, HW < 1, an unknown io or another dtype -> DPTX_E_INVALID. */
int dptx_op_head_out(int32_t dtype, const void* X, const float* w, const float* b, void* y, int32_t io, int32_t B,
                     int32_t HW, int32_t Cout, int32_t relu, void* stream);

/* The glue kernels of the forward, one launch each (tests/test_gpu_glue.py).  dtype is BF16 / FP16 / BF16X3 / FP16X3; a 16-bit
 * tensor is a hi/lo pair in the two-plane dtypes (planes of dptx_op_set_planes).  A null pointer, another dtype and every
 * argument named below as refused -> DPTX_E_INVALID, before anything is launched or written. */
/* The 16x16 patches of DPT-Large's patch embedding: x NCHW [B,3,H,W] of element type io -> P [B*(H/16)*(W/16)][768] 16-bit
 * with k = (c*16 + ky)*16 + kx, each element rounded to nearest (split for a pair).  Refused: an unknown io, B < 1, H or W
 * below 16 or no multiple of 16. */
int dptx_op_patchify16(int32_t dtype, const void* x, int32_t io, void* P, int32_t B, int32_t H, int32_t W, void* stream);
/* The re-layout behind a ConvTranspose2d with kernel == stride as a GEMM: G [B*h*w][(dy*k + dx)*C + c] ->
 * Y [B][h*k][w*k][C] (NHWC) with Y[b][y*k + dy][x*k + dx][c] = G[(b, y, x)][(dy*k + dx)*C + c]; both planes of a pair are
 * copied bit for bit.  Refused: B, h, w < 1, k outside 1..16, C < 8 or no multiple of 8, G == Y. */
int dptx_op_depth_to_space(int32_t dtype, const void* G, void* Y, int32_t B, int32_t h, int32_t w, int32_t k, int32_t C,
                           void* stream);
/* _resize_pos_embed (vit.py:102-116): src fp32 [1 + g_old*g_old][C] -> dst fp32 [1 + gh*gw][C]; row 0 (cls) is copied, the
 * grid rows are F.interpolate(mode="bilinear", align_corners=False) in ATen's fp32 index arithmetic.  Refused: g_old, gh, gw
 * or C < 1, (gh*gw + 1)*C or g_old*g_old*C at or above 2^31. */
int dptx_op_pos_resize(const float* src, float* dst, int32_t g_old, int32_t gh, int32_t gw, int32_t C, void* stream);
/* The cls half of ProjectReadout: out[b*N + n] (fp32) = sum_k x[b*x_stride + k] W[n*ldw + w_off + k] + bias[n] (bias may be
 * NULL).  x is fp32, or 16-bit of the dtype's type when x16 != 0 (BF16 / FP16 only); W is 16-bit, hi + lo in the two-plane
 * dtypes (weight plane of dptx_op_set_planes).  Refused: B, N < 1, K < 4, K / w_off / ldw / x_stride no multiple of 4,
 * w_off < 0, ldw < w_off + K, x_stride < K, x16 with a two-plane dtype. */
int dptx_op_readout_cls(int32_t dtype, const void* x, int64_t x_stride, const void* W, int32_t ldw, int32_t w_off,
                        const float* bias, float* out, int32_t B, int32_t N, int32_t K, int32_t x16, void* stream);
/* dst[i] (16-bit) = src[i] (fp32) rounded to nearest, hi = rn(x), lo = rn(x - hi) for a pair.  Refused: n < 8, n % 8 != 0. */
int dptx_op_cast_f32(int32_t dtype, const float* src, void* dst, int64_t n, void* stream);
/* dst[i] (fp32) = src[i] (16-bit), fl32(hi + lo) for a pair: the export of a debug tap.  Refused: n < 8, n % 8 != 0
 * (the rule of dptx_op_cast_f32, whose inverse it is). */
int dptx_op_to_f32(int32_t dtype, const void* src, float* dst, int64_t n, void* stream);
/* *amax_bits = max(*amax_bits, bits of max_i |X[i]|) (relu != 0: of max_i max(X[i], 0)) over the n 16-bit values of ONE plane
 * (the two-plane dtypes name the plane type only): the fp8 calibration's reduction; a non-negative float orders like its
 * bits.  Refused: n < 8, n % 8 != 0. */
int dptx_op_amax(int32_t dtype, const void* X, int64_t n, int32_t relu, uint32_t* amax_bits, void* stream);
/* *flag |= 1 if any of the n 16-bit values of ONE plane is an Inf or a NaN: the forward's range check.  Refused: n < 8,
 * n % 8 != 0. */
int dptx_op_nonfinite_scan(int32_t dtype, const void* X, int64_t n, uint32_t* flag, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The reference's version-1 UNet (omnidata_tools/torch/modules/unet.py:8-105; checkpoint omnidata_unet_normal_v1.pth),
 * inference forward: downsample = 6, in_channels = 3, out_channels 1..4, GroupNorm(8) + ReLU behind every 3x3
 * convolution, 2x2 max-pool down, bilinear x2 (align_corners=False) up, torch.cat((up, skip)) into each up block.
 * A handle type of its own with the conventions of dptx_handle.  UNetRelu, UNetV2 and other depths are not covered.
 *
 * Precision: NHWC 16-bit activations (fp16, the default, or bf16), 16-bit convolution weights, fp32 accumulation,
 * fp32 norm vectors and biases.  Every convolution stores its raw output (bias added) in 16 bit; the GroupNorm
 * statistics are those of the stored values; the last GroupNorm + ReLU + 1x1 convolution stay in fp32.  Results are
 * bitwise reproducible and an image's result does not depend on the rest of its batch. */
typedef struct dptx_unet_engine* dptx_unet_handle;
typedef struct dptx_unet_config {
  int32_t out_channels; /* 1..4 (normals 3, depth 1)                                                         */
  int32_t max_batch;    /* 1..32: the arena is planned once for max_batch x max_height x max_width           */
  int32_t dtype;        /* DPTX_DTYPE_FP16 (default) or DPTX_DTYPE_BF16; every other dtype: DPTX_E_INVALID   */
  int32_t device_id;    /* HIP device ordinal; -1 = host-only handle (weight packing only)                   */
  int32_t max_height;   /* multiples of 64 in 64..512                                                        */
  int32_t max_width;
  int32_t reserved[2];  /* must be zero                                                                      */
} dptx_unet_config;
/* out_channels 3, max_batch 32, fp16, device 0, 384 x 384 */
void dptx_unet_default_config(dptx_unet_config* cfg);
int dptx_unet_create(dptx_unet_handle* out, const dptx_unet_config* cfg);
void dptx_unet_destroy(dptx_unet_handle h);
const char* dptx_unet_last_error(dptx_unet_handle h);
/* One tensor of the reference's state dict (174 keys: "down1.conv1.weight", "down_blocks.3.bn2.bias", "mid_conv1.weight",
 * "bn1.weight", "up_blocks.5.conv1.weight", "last_conv2.bias", ...; OIHW convolution weights), fp32 on the host.  Unknown keys
 * or wrong shapes -> DPTX_E_KEY. */
int dptx_unet_load_tensor(dptx_unet_handle h, const char* ref_key, const float* host_fp32, const int64_t* shape, int32_t ndim);
/* Strict: every key must have been loaded (DPTX_E_KEY, the message lists the missing ones).  Packs one blob -- the entries in
 * state-dict order, each 256-byte aligned: 3x3 weights as 16-bit [O][ky][kx][I] (an up block's conv1 keeps torch.cat's order
 * of I: the up-sampled channels, then the skip), down1.conv1 as 16-bit [16][32] with k = (ky*3 + kx)*3 + c and k = 27..31 zero,
 * last_conv2.weight, biases and norm vectors verbatim in fp32 -- and, on a device handle, uploads it and allocates the arena. */
int dptx_unet_finalize_weights(dptx_unet_handle h);
size_t dptx_unet_packed_bytes(dptx_unet_handle h);
/* byte offset and size of one state-dict tensor inside the packed blob */
int dptx_unet_packed_entry(dptx_unet_handle h, const char* ref_key, int64_t* offset, int64_t* bytes);
/* the packed blob (works on host-only handles) */
int dptx_unet_export_packed_host(dptx_unet_handle h, void* dst_host, size_t bytes);
/* packed weights + activation arena of a device handle */
size_t dptx_unet_device_bytes(dptx_unet_handle h);
/* x [B,3,H,W] NCHW of x_dtype (DPTX_IO_*), values in [0, 1] -> y [B,out_channels,H,W] NCHW fp32.  H and W: multiples of 64 in
 * 64..max_height / max_width, 1 <= B <= max_batch, otherwise DPTX_E_INVALID.  Asynchronous on `stream`; no allocation and no
 * synchronisation inside. */
int dptx_unet_forward(dptx_unet_handle h, const void* x_dev, void* y_dev, int32_t batch, int32_t height, int32_t width,
                      int32_t x_dtype, void* stream);
/* Raw convolution outputs are stored before normalisation, so fp16 can overflow on weights nobody has seen.  The GroupNorm
 * statistics read every stored element: a non-finite sum sets a STICKY device flag.  Waits for `stream`, stores the flag in
 * *nonfinite and clears it when reset != 0 (the convention of dptx_range_status). */
int dptx_unet_range_status(dptx_unet_handle h, int32_t* nonfinite, int32_t reset, void* stream);
/* debug: every byte of the arena := byte_value (after a device synchronisation) */
int dptx_unet_debug_arena_fill(dptx_unet_handle h, int32_t byte_value);
/* debug / timing: a forward that enqueues only the launches of the classes in `classes` (1: small-channel convolutions and
 * the im2col, 2: launch_gemm convolutions, 4: GroupNorm / up-sample / head passes; 7 = dptx_unet_forward).  Anything but 7
 * leaves garbage in y: for timing the classes only (tools/unet_bench.py). */
int dptx_unet_debug_forward_classes(dptx_unet_handle h, const void* x_dev, void* y_dev, int32_t batch, int32_t height,
                                    int32_t width, int32_t x_dtype, int32_t classes, void* stream);

/* Op-level entry points of the UNet kernels (unet.hip), BF16 / FP16, NHWC 16-bit.
 * 3x3 convolution, pad 1, stride 1, bias, for (Cin, Cout) in {(3,16), (16,16), (16,32), (32,32), (32,64), (48,16), (96,32)}:
 * X [B][H][W][x_pix_stride], the layer reads channels x_off .. x_off + Cin (both multiples of 8); Wt [Cout][3][3][Cin];
 * Y [B][H][W][Cout] raw output; gn_part (may be NULL): B * dptx_op_unet_conv_records(H, W) * 8 float2 (sum, sum of squares)
 * records of the stored values per (image, 8 x 32 tile, group of GroupNorm(8)).  Cin = 3: X is the fp32 NCHW image [B,3,H,W],
 * Wt the padded [Cout][32] block (k = (ky*3 + kx)*3 + c) and `scratch` holds B*H*W*32 16-bit elements. */
int dptx_op_unet_conv3x3(int32_t dtype, const void* X, int32_t x_pix_stride, int32_t x_off, const void* Wt, const float* bias,
                         void* Y, float* gn_part, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* scratch,
                         void* stream);
int32_t dptx_op_unet_conv_records(int32_t H, int32_t W);
/* dptx_op_unet_conv3x3 for Cin = 3 on a caller image x [B,3,H,W] NCHW of element type io (DPTX_IO_FP32 / _BF16 / _FP16; anything
 * else: DPTX_E_INVALID): Wt the padded [Cout][32] block, Y, gn_part and scratch (B*H*W*32 16-bit elements) as above. */
int dptx_op_unet_conv3x3_io(int32_t dtype, const void* x, int32_t io, const void* Wt, const float* bias, void* Y, float* gn_part,
                            int32_t B, int32_t H, int32_t W, int32_t Cout, void* scratch, void* stream);
/* A 3x3 convolution (pad 1, stride 1, bias) of the layers with Cin and Cout >= 64, launched exactly as the forward launches
 * it (the implicit GEMM; BF16 / FP16 only, a plane dtype is DPTX_E_INVALID, and so is whatever the GEMM launcher refuses:
 * Cin % 64 != 0, Cout % 32 != 0).  X [B][H][W][x_pix_stride] 16-bit, the layer reads channels x_off .. x_off + Cin of every
 * pixel (x_pix_stride and x_off multiples of 8; dense: x_pix_stride = Cin, x_off = 0); x_bytes = the size of the WHOLE X
 * buffer in bytes (>= B*H*W*x_pix_stride*2), beyond which nothing is read; Wt [Cout][3][3][Cin] 16-bit; bias [Cout] fp32
 * (may be NULL); Y [B][H][W][Cout] 16-bit, dense: exactly B*H*W*Cout elements are written. */
int dptx_op_unet_conv_gemm(int32_t dtype, const void* X, int32_t x_pix_stride, int32_t x_off, int64_t x_bytes, const void* Wt,
                           const float* bias, void* Y, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stream);
/* last_bn + ReLU + last_conv2 in one pass: X [B][HW][16] 16-bit raw values, stats [B][8][2] fp32 (mean, rstd) per (image,
 * group of 2 channels) supplied by the caller, gamma / beta [16], w [OC][16] and bias [OC] fp32; y [B][OC][HW] fp32 (NCHW):
 * exactly B*OC*HW elements are written.  OC 1..4, BF16 / FP16; otherwise DPTX_E_INVALID. */
int dptx_op_unet_gn_head(int32_t dtype, const void* X, const float* stats, const float* gamma, const float* beta, const float* w,
                         const float* bias, float* y, int32_t B, int32_t HW, int32_t OC, void* stream);
/* GroupNorm(8) + ReLU of a dense X [B][H][W][C] (C % 16 == 0, 16..1024): statistics pass, (mean, rstd) in double, apply.
 * Y (may be NULL): full size, into channels y_off .. y_off + C of pixels y_pix_stride apart; P (may be NULL; H, W even): the
 * 2x2 / 2 max-pooled result, likewise.  scratch_f32: B * (dptx_op_unet_gn_records(H*W, C) * 16 + 16) floats. */
int dptx_op_unet_groupnorm(int32_t dtype, const void* X, const float* gamma, const float* beta, void* Y, int32_t y_pix_stride,
                           int32_t y_off, void* P, int32_t p_pix_stride, int32_t p_off, int32_t B, int32_t H, int32_t W,
                           int32_t C, float eps, void* scratch_f32, void* stream);
int32_t dptx_op_unet_gn_records(int32_t HW, int32_t C);
/* bilinear x2, align_corners=False (torch's rule: weights 0.25 / 0.75, edge clamp): X [B][H][W][C] dense -> channels
 * y_off .. y_off + C of Y [B][2H][2W][y_pix_stride] */
int dptx_op_unet_upsample2x(int32_t dtype, const void* X, void* Y, int32_t B, int32_t H, int32_t W, int32_t C,
                            int32_t y_pix_stride, int32_t y_off, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DPTX_H_ */
