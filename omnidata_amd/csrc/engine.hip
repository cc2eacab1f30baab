// engine.hip -- libdptx.so host side: the handle-based C ABI of include/dptx.h, the weight spec and its folding / packing,
// the activation arena plan and the fixed kernel schedule of one forward (DPT-Hybrid-384 or DPT-Large-384).  The op-level
// entry points (dptx_op_*), which touch no handle, live in ops.hip.
//
// Reference being replaced (paths under omnidata_tools/torch/modules/midas/):
//   dpt_depth.py:67-85  DPT.forward          -> Run::forward
//   vit.py:119-155      forward_flex         -> stem / stages / tokens / 12 (24) blocks
//   vit.py:61-99        forward_vit          -> Run::readout: readout + reassemble (act_postprocess1..4)
//   blocks.py:263-341   RCU / FeatureFusion  -> Run::rcu and the fusion loop of Run::decode
//   dpt_depth.py:91-99  head                 -> head convs + head tail / head_out (end of Run::decode)
// timm 0.4.12 vit_base_resnet50_384 (vit.py:483) is restated per SURVEY.md A.2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dptx.h"
#include "host_util.h"
#include "kernels.h"

using namespace dptx;

namespace {

constexpr int IMG = 384;
constexpr int S_TOK = 577;
constexpr int FEAT = 256;
const int STAGE_DEPTH[3] = {3, 4, 9};
const int STAGE_OUT[3] = {256, 512, 1024};
const int STAGE_STRIDE[3] = {1, 2, 2};

// ---------------------------------------------------------------- host 16-bit conversions (f32 -> 16-bit: host_util.h)
inline float fp16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu, u;
  if (e == 0) {
    if (m == 0) u = sign;
    else {  // subnormal half: normalise
      int sh = 0;
      while (!(m & 0x400u)) { m <<= 1; ++sh; }
      u = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
  else u = sign | ((e + 112u) << 23) | (m << 13);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// OCP e4m3 (fp8 "fn": bias 7, 3 mantissa bits, max 448, no infinities), round to nearest even, saturating
inline uint8_t f32_to_e4m3(float f) {
  if (f != f) return 0x7f;
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  double a = std::fabs((double)f);
  if (a >= 448.0) return sign | 0x7e;
  if (a < std::ldexp(1.0, -10)) return sign;  // below half of the smallest subnormal (2^-9)
  int e;
  (void)std::frexp(a, &e);  // a = m * 2^e, m in [0.5, 1)
  e -= 1;                   // a = (1.xxx) * 2^e
  if (e < -6) {             // subnormal: multiples of 2^-9
    const int q = (int)std::nearbyint(std::ldexp(a, 9));
    return sign | (uint8_t)q;  // q == 8 is the smallest normal (exp field 1, mantissa 0): the same bit pattern
  }
  int m = (int)std::nearbyint((std::ldexp(a, -e) - 1.0) * 8.0);
  if (m == 8) { m = 0; ++e; }
  if (e > 8) return sign | 0x7e;
  return sign | (uint8_t)(((e + 7) << 3) | m);
}

inline float e4m3_to_f32(uint8_t v) {
  const int e = (v >> 3) & 0xf, m = v & 7;
  const double a = e == 0 ? std::ldexp((double)m, -9) : std::ldexp(1.0 + m / 8.0, e - 7);
  return (float)((v & 0x80) ? -a : a);
}

// Power-of-two scale that puts a weight channel's max |w| into (224, 448] (e4m3 tops out at 448; 1 for an
// all-zero channel); *inv receives its inverse, which the GEMM epilogue multiplies the channel's accumulators with
inline float e4m3_channel_scale(float amax, float* inv) {
  const float sc = std::ldexp(1.0f, amax > 0.f ? (int)std::floor(std::log2(448.0 / (double)amax)) : 0);
  *inv = 1.0f / sc;
  return sc;
}

// --------------------------------------------------------------------------- weight spec
// R_DECONV: ConvTranspose2d [Cin, Cout, k, k] with kernel == stride, packed as the GEMM operand [(dy*k+dx)*Cout + co][ci];
// R_DECONV_BIAS: its bias, tiled k*k times so that the GEMM epilogue can add it per column
// R_DERIVED: fp32 vector that is not part of the state_dict but computed at pack time (LayerNorm fold: column sums of the
// folded qkv / fc1 weights)
enum Role { R_STDCONV, R_CONV, R_LINEAR, R_VEC, R_HEAD4, R_UNUSED, R_DECONV, R_DECONV_BIAS, R_DERIVED };
struct Spec {
  std::string key;
  std::vector<int64_t> shape;
  Role role;
};

void add(std::vector<Spec>& v, const std::string& k, std::vector<int64_t> s, Role r) { v.push_back({k, std::move(s), r}); }

// One timm Block under prefix p: its 12 state-dict entries, then the entries derived at pack time -- the LayerNorm fold's
// column sums and, for the fp8 dtype (DPTX_FLAG_FP8_VIT, round 6), the per-output-channel inverse scales of the e4m3 copies of
// qkv / fc1 / fc2 and the column sums of the DEQUANTISED folded e4m3 weights (the fold's mean term must cancel against what
// the MFMA actually multiplies)
void add_vit_block(std::vector<Spec>& v, const std::string& p, int D_VIT, int D_MLP) {
  add(v, p + "norm1.weight", {D_VIT}, R_VEC);
  add(v, p + "norm1.bias", {D_VIT}, R_VEC);
  add(v, p + "attn.qkv.weight", {3 * D_VIT, D_VIT}, R_LINEAR);
  add(v, p + "attn.qkv.bias", {3 * D_VIT}, R_VEC);
  add(v, p + "attn.proj.weight", {D_VIT, D_VIT}, R_LINEAR);
  add(v, p + "attn.proj.bias", {D_VIT}, R_VEC);
  add(v, p + "norm2.weight", {D_VIT}, R_VEC);
  add(v, p + "norm2.bias", {D_VIT}, R_VEC);
  add(v, p + "mlp.fc1.weight", {D_MLP, D_VIT}, R_LINEAR);
  add(v, p + "mlp.fc1.bias", {D_MLP}, R_VEC);
  add(v, p + "mlp.fc2.weight", {D_VIT, D_MLP}, R_LINEAR);
  add(v, p + "mlp.fc2.bias", {D_VIT}, R_VEC);
  add(v, p + "attn.qkv.lnsum", {3 * D_VIT}, R_DERIVED);
  add(v, p + "mlp.fc1.lnsum", {D_MLP}, R_DERIVED);
  add(v, p + "attn.qkv.f8scale", {3 * D_VIT}, R_DERIVED);
  add(v, p + "mlp.fc1.f8scale", {D_MLP}, R_DERIVED);
  add(v, p + "mlp.fc2.f8scale", {D_VIT}, R_DERIVED);
  add(v, p + "attn.qkv.lnsum8", {3 * D_VIT}, R_DERIVED);
  add(v, p + "mlp.fc1.lnsum8", {D_MLP}, R_DERIVED);
}

// pretrained.act_postprocess<n>: ProjectReadout, the 1x1 conv to f channels and the resampling layer "4" -- a ConvTranspose2d
// with kernel == stride == deconv_k, or (conv3) the 3x3 stride-2 convolution, or neither
void add_readout(std::vector<Spec>& v, int n, int D_VIT, int f, int deconv_k, bool conv3) {
  const std::string p = "pretrained.act_postprocess" + std::to_string(n) + ".";
  add(v, p + "0.project.0.weight", {D_VIT, 2 * D_VIT}, R_LINEAR);
  add(v, p + "0.project.0.bias", {D_VIT}, R_VEC);
  add(v, p + "3.weight", {f, D_VIT, 1, 1}, R_CONV);
  add(v, p + "3.bias", {f}, R_VEC);
  if (deconv_k) { add(v, p + "4.weight", {f, f, deconv_k, deconv_k}, R_DECONV); add(v, p + "4.bias", {f}, R_DECONV_BIAS); }
  if (conv3) { add(v, p + "4.weight", {f, f, 3, 3}, R_CONV); add(v, p + "4.bias", {f}, R_VEC); }
}

// Mirrors omnidata_amd/weights.py:state_dict_spec (reference key names).
// `dual`: a second decoder (depth, 1 channel) under "depth.scratch.*" next to the normal one (3 channels) under
// "scratch.*"; both read the one shared encoder "pretrained.*" (SURVEY.md 8d config 5).
// backbone 0: vitb_rn50_384 (DPT-Hybrid); 1: vitl16_384 (DPT-Large; omnidata_amd/weights.py
// vitl16_state_dict_spec)
std::vector<Spec> build_spec(int C, bool dual, int backbone) {
  std::vector<Spec> v;
  const std::string vp = "pretrained.model.";
  const int D_VIT = backbone == 1 ? 1024 : 768, D_MLP = 4 * D_VIT, depth = backbone == 1 ? 24 : 12;
  add(v, vp + "cls_token", {1, 1, D_VIT}, R_VEC);
  add(v, vp + "pos_embed", {1, S_TOK, D_VIT}, R_VEC);
  if (backbone == 1) {
    add(v, vp + "patch_embed.proj.weight", {D_VIT, 3, 16, 16}, R_LINEAR);  // flattened (c, ky, kx) = the patch matrix's k order
    add(v, vp + "patch_embed.proj.bias", {D_VIT}, R_VEC);
  } else {
    const std::string bp = vp + "patch_embed.backbone.";
    add(v, bp + "stem.conv.weight", {64, 3, 7, 7}, R_STDCONV);
    add(v, bp + "stem.norm.weight", {64}, R_VEC);
    add(v, bp + "stem.norm.bias", {64}, R_VEC);
    int cin = 64;
    for (int s = 0; s < 3; ++s) {
      const int cout = STAGE_OUT[s], mid = cout / 4;
      for (int b = 0; b < STAGE_DEPTH[s]; ++b) {
        const std::string p = bp + "stages." + std::to_string(s) + ".blocks." + std::to_string(b) + ".";
        if (b == 0) {
          add(v, p + "downsample.conv.weight", {cout, cin, 1, 1}, R_STDCONV);
          add(v, p + "downsample.norm.weight", {cout}, R_VEC);
          add(v, p + "downsample.norm.bias", {cout}, R_VEC);
        }
        add(v, p + "conv1.weight", {mid, cin, 1, 1}, R_STDCONV);
        add(v, p + "norm1.weight", {mid}, R_VEC);
        add(v, p + "norm1.bias", {mid}, R_VEC);
        add(v, p + "conv2.weight", {mid, mid, 3, 3}, R_STDCONV);
        add(v, p + "norm2.weight", {mid}, R_VEC);
        add(v, p + "norm2.bias", {mid}, R_VEC);
        add(v, p + "conv3.weight", {cout, mid, 1, 1}, R_STDCONV);
        add(v, p + "norm3.weight", {cout}, R_VEC);
        add(v, p + "norm3.bias", {cout}, R_VEC);
        cin = cout;
      }
    }
    add(v, vp + "patch_embed.proj.weight", {D_VIT, 1024, 1, 1}, R_CONV);
    add(v, vp + "patch_embed.proj.bias", {D_VIT}, R_VEC);
  }
  for (int l = 0; l < depth; ++l) add_vit_block(v, vp + "blocks." + std::to_string(l) + ".", D_VIT, D_MLP);
  add(v, vp + "norm.weight", {D_VIT}, R_UNUSED);
  add(v, vp + "norm.bias", {D_VIT}, R_UNUSED);
  add(v, vp + "head.weight", {1000, D_VIT}, R_UNUSED);
  add(v, vp + "head.bias", {1000}, R_UNUSED);
  if (backbone == 1) {
    add_readout(v, 1, D_VIT, 256, 4, false);
    add_readout(v, 2, D_VIT, 512, 2, false);
    add_readout(v, 3, D_VIT, 1024, 0, false);
    add_readout(v, 4, D_VIT, 1024, 0, true);
  } else {
    add_readout(v, 3, D_VIT, D_VIT, 0, false);
    add_readout(v, 4, D_VIT, D_VIT, 0, true);
  }
  // "<conv>.f8scale": per-output-channel inverse of the power-of-two scale the e4m3 copy of the weight was quantised with
  // (fp8 dtype; derived at pack time, zero otherwise)
  auto decoder = [&](const std::string& pre, int ch) {
    const int rn_in[4] = {256, 512, D_VIT, D_VIT};
    for (int i = 1; i <= 4; ++i) add(v, pre + "scratch.layer" + std::to_string(i) + "_rn.weight", {FEAT, rn_in[i - 1], 3, 3}, R_CONV);
    for (int i = 1; i <= 4; ++i) {
      const std::string p = pre + "scratch.refinenet" + std::to_string(i) + ".";
      add(v, p + "out_conv.weight", {FEAT, FEAT, 1, 1}, R_CONV);
      add(v, p + "out_conv.bias", {FEAT}, R_VEC);
      add(v, p + "out_conv.f8scale", {FEAT}, R_DERIVED);
      for (int u = 1; u <= 2; ++u)
        for (int c = 1; c <= 2; ++c) {
          const bool unused = (i == 4 && u == 1);  // blocks.py:329-333: resConfUnit1 needs two inputs
          const std::string q = p + "resConfUnit" + std::to_string(u) + ".conv" + std::to_string(c) + ".";
          add(v, q + "weight", {FEAT, FEAT, 3, 3}, unused ? R_UNUSED : R_CONV);
          add(v, q + "bias", {FEAT}, unused ? R_UNUSED : R_VEC);
          if (!unused) add(v, q + "f8scale", {FEAT}, R_DERIVED);
        }
    }
    add(v, pre + "scratch.output_conv.0.weight", {FEAT / 2, FEAT, 3, 3}, R_CONV);
    add(v, pre + "scratch.output_conv.0.bias", {FEAT / 2}, R_VEC);
    add(v, pre + "scratch.output_conv.0.f8scale", {FEAT / 2}, R_DERIVED);
    add(v, pre + "scratch.output_conv.2.weight", {32, FEAT / 2, 3, 3}, R_CONV);
    add(v, pre + "scratch.output_conv.2.bias", {32}, R_VEC);
    add(v, pre + "scratch.output_conv.4.weight", {ch, 32, 1, 1}, R_HEAD4);
    add(v, pre + "scratch.output_conv.4.bias", {ch}, R_VEC);
  };
  decoder("", dual ? 3 : C);
  if (dual) decoder("depth.", 1);
  return v;
}

inline size_t numel(const std::vector<int64_t>& s) {
  size_t n = 1;
  for (auto d : s) n *= (size_t)d;
  return n;
}

constexpr int STEM_K = 176;  // stem K axis ordered (c, ky, kx) with kx padded 7 -> 8 (168) and rounded up to 11 MFMA k-steps

size_t packed_entry_bytes(const Spec& s) {
  switch (s.role) {
    case R_STDCONV:
      if (s.shape[3] == 7) return (size_t)s.shape[0] * STEM_K * 2;
      return numel(s.shape) * 2;
    case R_CONV:
    case R_DECONV:
    case R_LINEAR: return numel(s.shape) * 2;
    case R_VEC:
    case R_DERIVED:
    case R_HEAD4: return numel(s.shape) * 4;
    case R_DECONV_BIAS: return numel(s.shape) * 4 * 16;  // room for the 4x4 case (the 2x2 one uses a quarter)
    default: return 0;
  }
}

// The packed blob starts with a 256-byte header that names the layout it was packed for: ranks (dptx_import_packed_device) and
// the on-disk cache refuse a blob whose packing differs from what this handle would produce itself -- e.g. a rank whose
// environment switched the LayerNorm fold off would otherwise multiply folded qkv / fc1 weights as if they were plain.
constexpr size_t BLOB_HEADER = 256;
struct BlobHeader {
  char magic[8];          // "DPTXBLOB"
  uint32_t version;       // layout version of this header / of the packing code
  int32_t dtype, backbone, dual_task, num_channels, ln_fold, ws_form;
  float ws_eps;
  uint64_t packed_single, packed_bytes;
};
static_assert(sizeof(BlobHeader) <= BLOB_HEADER, "header fits its slot");
constexpr uint32_t BLOB_VERSION = 5;   // 5: fp8 entries of the ViT linears (round 6)

struct Buf {  // arena slice: `off` in the whole-batch plan, `off2` in the half-batch plan (two sub-batches on two streams)
  size_t off = 0, bytes = 0, off2 = 0;
};

inline bool ends_with(const std::string& k, const char* suf) {
  const size_t n = strlen(suf);
  return k.size() >= n && k.compare(k.size() - n, n, suf) == 0;
}

struct TapInfo {
  const void* ptr;
  int64_t shape[4];
  bool fp32;
  int mode;  // kernel mode of the group that produced it (single-pass groups of a MIXED engine write the hi plane only)
};

}  // namespace

struct dptx_engine {
  dptx_config cfg;
  int backbone = 0;                              // 0 vitb_rn50_384, 1 vitl16_384
  int dv = 768, dm = 3072, nh = 12, depth = 12;  // ViT width, MLP width, heads, blocks
  std::vector<Spec> spec;
  std::unordered_map<std::string, size_t> spec_index;
  std::unordered_map<std::string, size_t> packed_off;  // byte offset inside the blob
  size_t packed_bytes = 0;    // total blob bytes (hi blob [+ lo blob in bf16x3 mode])
  size_t packed_single = 0;   // bytes of one plane of the blob
  size_t arena_single = 0;    // bytes of one plane of the arena
  Planes pl{0, 0};
  std::map<std::string, std::vector<float>> staged;  // fp32 tensors loaded so far
  std::vector<uint8_t> host_blob;
  bool finalized = false;  // host blob valid
  bool device_ready = false;
  char* d_blob = nullptr;
  // The packed blob's allocation is reference-counted: dptx_share_packed hands a second handle the same memory, and whichever
  // handle is destroyed LAST frees it -- destroying the handle that loaded the weights while others still read them is legal.
  std::shared_ptr<void> blob_hold;
  bool blob_shared = false;   // this handle did not load the blob it reads (dptx_share_packed): it never writes it
  char* d_arena = nullptr;
  size_t arena_bytes = 0;
  std::string err;
  std::map<std::string, TapInfo> taps;
  bool taps_on = false;
  // kernel mode (common.h MODE_*) of a layer group: the engine dtype, or -- MIXED -- fp16x3 / fp16 per dptx_config.x3_groups
  int mode_of(int group) const {
    if (cfg.dtype == DPTX_DTYPE_FP8) return MODE_BF16;  // fp8 GEMMs are launched explicitly (Run::conv), the rest is bf16
    if (cfg.dtype != DPTX_DTYPE_MIXED) return cfg.dtype;
    return (cfg.x3_groups & group) ? MODE_FP16X3 : MODE_FP16;
  }
  bool fp8() const { return cfg.dtype == DPTX_DTYPE_FP8; }
  // Per-LAYER precision inside the decoder groups (RN / FUSION / HEAD) of the MIXED dtype: conv key (reference name without
  // a "depth." prefix) -> 1 (one MFMA per product on the hi planes), 3 (hi/lo planes, three MFMAs) or 2 (hi/lo planes of the
  // weights, hi plane of the activations: a_hi w_hi + a_hi w_lo); keys that are not listed follow their group's bit in x3_groups.  The default table (dptx_create) is the cheapest assignment found by
  // oracle/precision_layers.py that keeps the emulated deviation from the fp32 forward where the all-3-MFMA decoder has it.
  std::unordered_map<std::string, int> layer_prec;
  bool mixed() const { return cfg.dtype == DPTX_DTYPE_MIXED; }
  int layer_mfmas(const std::string& wkey, int group) const {
    const std::string k = wkey.compare(0, 6, "depth.") == 0 ? wkey.substr(6) : wkey;
    auto it = layer_prec.find(k);
    if (it != layer_prec.end()) return it->second;
    return (cfg.x3_groups & group) ? 3 : 1;
  }
  // hi/lo-plane kernel (2 or 3 MFMAs per product: the weights' lo plane is used) / the layer reads the lo plane of its INPUT
  bool layer_x3(const std::string& wkey, int group) const { return layer_mfmas(wkey, group) >= 2; }
  bool layer_reads_lo(const std::string& wkey, int group) const { return layer_mfmas(wkey, group) == 3; }
  // LayerNorm of the ViT blocks folded into the qkv / fc1 GEMMs (include/dptx.h DPTX_FLAG_NO_LN_FOLD): the packed qkv / fc1
  // weights and biases are then the folded ones, so this is fixed at dptx_create
  bool ln_fold = false;
  // 16-bit token stream (include/dptx.h DPTX_FLAG_FP32_STREAM): with the fold in place the single-pass dtypes need the
  // residual stream of the ViT blocks only as the 16-bit tensor the qkv / fc1 GEMMs multiply -- Hn IS the stream, the
  // proj / fc2 epilogues read and write 2 + 2 bytes per element instead of 4 + 4 + 2, and no fp32 copy exists
  bool stream16 = false;
  // fp8: the second plane of the arena / blob holds the e4m3 copies (byte offset off / 2 inside it) instead of lo planes
  bool two_planes() const {
    return cfg.dtype == DPTX_DTYPE_BF16X3 || cfg.dtype == DPTX_DTYPE_FP16X3 || cfg.dtype == DPTX_DTYPE_MIXED || fp8();
  }
  bool bf16_storage() const { return cfg.dtype == DPTX_DTYPE_BF16 || cfg.dtype == DPTX_DTYPE_BF16X3 || fp8(); }
  // convolutions that CAN run on e4m3 operands in the fp8 dtype (their weights get an e4m3 copy at pack time): the decoder's
  // RCU convs, out_conv and the first head conv ...
  static bool fp8_weight(const std::string& key) {
    return key.find("scratch.") != std::string::npos && key.size() > 7 && ends_with(key, ".weight") &&
           (key.find("resConfUnit") != std::string::npos || key.find("out_conv") != std::string::npos ||
            key.find("output_conv.0.") != std::string::npos);
  }
  // ... and the ones that actually do (include/dptx.h DPTX_FLAG_FP8_ALL): by default only the six convolutions of the
  // resConfUnit1 blocks of refinenet1..3 -- 14.3 GMAC per decoder whose e4m3 rounding moves the output least
  // (oracle/fp8_layers.py: the set costs <= 1.5 deg of mean angular error on either synthetic weight family, so that the
  // mode stays within 2 x the bf16 engine's error); with the flag all 19 (round 3's mode: 7.5 - 9 deg, a lossy throughput mode)
  bool fp8_all = false;
  // DPTX_FLAG_FP8_VIT (round 6): qkv / fc1 / fc2 of every transformer block on e4m3 operands as well -- 45 of the forward's
  // 127.6 GMAC (proj stays bf16: its operand is the attention kernel's output, which has no e4m3 copy).  oracle/fp8_vit.py: with
  // per-output-channel weight scales and ONE calibrated scale per activation tensor these layers cost 2.1-2.7 deg of mean
  // angular error on the default weight family and 1.2-1.9 deg on the trained-like one, about what the six default decoder
  // convolutions cost -- not the "destroyed output" that rounds 3-5 assumed.
  bool fp8_vit = false;
  static bool fp8_vit_weight(const std::string& key) {
    return key.find("pretrained.model.blocks.") != std::string::npos &&
           (ends_with(key, "attn.qkv.weight") || ends_with(key, "mlp.fc1.weight") || ends_with(key, "mlp.fc2.weight"));
  }
  bool fp8_use(const std::string& key) const {
    if (!fp8()) return false;
    if (fp8_vit_weight(key)) return fp8_vit && ln_fold && stream16;
    if (!fp8_weight(key)) return false;
    return fp8_all || key.find("resConfUnit1.") != std::string::npos;
  }
  const void* w8(const std::string& key) const { return d_blob + packed_single + packed_off.at(key) / 2; }
  // per-output-channel inverse weight scales of an fp8 conv ("....weight" -> "....f8scale" entry of the blob)
  const float* wscale(const std::string& key) const { return f(key.substr(0, key.size() - 6) + "f8scale"); }
  // fp8 activation scales: every tensor that has an e4m3 copy gets a power-of-two scale s (the copy holds e4m3(x * s), the
  // consuming conv multiplies its accumulators by 1 / s), indexed by the order in which a forward produces the copies.
  // 1.0 until dptx_calibrate_fp8 has measured the tensors' max |x| on a calibration batch (slot -> max |x| in act_amax).
  static constexpr int MAX_Q8 = 128;
  std::vector<float> act_scale = std::vector<float>(MAX_Q8, 1.0f);
  std::vector<float> act_amax = std::vector<float>(MAX_Q8, 0.0f);
  int n_q8 = 0;                  // slots used by the last forward
  bool calibrating = false, calibrated = false;
  unsigned* d_amax = nullptr;    // [MAX_Q8] float bits (calibration forwards only)
  // range check of the fp16-plane dtypes (include/dptx.h dptx_range_status): sticky device flag, set by a scan of H0
  unsigned* d_range = nullptr;
  bool range_check() const {
    return (cfg.dtype == DPTX_DTYPE_FP16 || cfg.dtype == DPTX_DTYPE_FP16X3 || cfg.dtype == DPTX_DTYPE_MIXED) &&
           !(cfg.flags & DPTX_FLAG_NO_RANGE_CHECK);
  }
  void* q8(const void* p) const { return d_arena + arena_single + ((const char*)p - d_arena) / 2; }  // e4m3 copy of an arena tensor
  // fused head tail (head.hip): no stage taps wanted; a 3-MFMA second head conv has its fused form for fp16 planes only
  // (head_tail_x3_kernel: "mixed", fp16x3)
  bool head_fused(bool conv2_x3) const {
    if (taps_on) return false;
    return !conv2_x3 || cfg.dtype == DPTX_DTYPE_MIXED || cfg.dtype == DPTX_DTYPE_FP16X3;
  }
  size_t tok_tap_stride = 0;      // floats per token-stream snapshot
  float* d_tok_taps = nullptr;  // [13][max_batch*(max tokens)*768] fp32 copies of the token stream (taps_on)
  int64_t launches = 0;
  double exec_macs = 0.0;
  int last_batch = 0;
  int last_regions = 1;  // sub-batch regions the last forward used (1: the whole-batch plan)
  // optional per-launch timing (one event after every launch; kernels are serialized on the stream)
  bool profiling = false;
  std::vector<hipEvent_t> events;
  std::vector<int> event_cat;
  std::vector<std::string> event_name;
  double cat_ms[4] = {0, 0, 0, 0};
  int64_t cat_launches[4] = {0, 0, 0, 0};
  double cat_macs[4] = {0, 0, 0, 0};

  // two sub-batches on two internal streams (MFMA-bound and HBM-bound launches of the two halves overlap, tails fill)
  static constexpr int MAX_STREAMS = 4;
  int n_streams = 2;              // cfg.streams (0 = auto: 2 streams exist, used only when measured faster); 1 = caller's stream
  // cfg.streams == 0 and no DPTX_STREAMS: the two-half schedule is used only after dptx_tune_schedule measured it >= 3 % faster
  bool auto_streams = false, split_tuned = false, split_on = false;
  float tune_ms_single = 0.f, tune_ms_split = 0.f;
  int force_schedule = -1;        // dptx_tune_schedule: 0 / 1 while it times a candidate
  int half_batch = 0;             // images per sub-batch region (ceil(max_batch / n_streams))
  size_t half_region = 0;         // bytes of one sub-batch region (n_streams of them fit in one arena plane)
  hipStream_t sub_stream[MAX_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[MAX_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
  // arena slices
  int max_h = 384, max_w = 384;   // largest supported input (cfg.max_height/max_width; 0 = 384)
  Buf pos_alt;
  Buf sraw, stem, S[3], T1, T2, PA, PB, DS, part[4], gntab, X, Hn, QKV, AO, F1, R3, R4, L3, T4, L4, clsb, lrn[4], tA, tB,
      tC, P[4], H0, H0U, H1, lnst;
  // every buffer of the plan with its name, in plan order (recorded by plan_arena_for: what it takes is what
  // dptx_debug_arena_layout lists and dptx_debug_arena_checksums sums)
  std::vector<std::pair<std::string, const Buf*>> arena_bufs;

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  const void* w(const std::string& key) const { return d_blob + packed_off.at(key); }
  const float* f(const std::string& key) const { return (const float*)(d_blob + packed_off.at(key)); }
  BlobHeader blob_header() const {
    BlobHeader hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, "DPTXBLOB", 8);
    hd.version = BLOB_VERSION;
    hd.dtype = cfg.dtype; hd.backbone = backbone; hd.dual_task = cfg.dual_task; hd.num_channels = cfg.num_channels;
    hd.ln_fold = ln_fold ? 1 : 0; hd.ws_form = cfg.ws_form; hd.ws_eps = cfg.ws_eps;
    hd.packed_single = packed_single; hd.packed_bytes = packed_bytes;
    return hd;
  }
};

namespace {

#define HIPCHK(e, call)                                                                   \
  do {                                                                                    \
    hipError_t _r = (call);                                                               \
    if (_r != hipSuccess) return (e)->fail(DPTX_E_HIP, std::string(#call) + ": " + hipGetErrorString(_r)); \
  } while (0)

// Bump-allocates every activation buffer for Bn images; half = false fills Buf::off (one run over the whole batch),
// half = true fills Buf::off2 (layout of ONE of the two half-batch regions).  The whole-batch pass also records every buffer
// it takes, by name, in dptx_engine::arena_bufs.  Returns the bytes used.
size_t plan_arena_for(dptx_engine* e, size_t B, bool half) {
  // every buffer scales with the pixel count of the largest supported input (H, W multiples of 32); P = H*W
  const size_t P = (size_t)e->max_h * e->max_w;
  const size_t p2 = P / 4, p4 = P / 16, p8 = P / 64, p16 = P / 256, p32 = P / 1024, S = p16 + 1;
  const size_t DV = (size_t)e->dv;
  size_t off = 0;
  if (!half) e->arena_bufs.clear();
  auto take = [&](const std::string& name, Buf& b, size_t elems, size_t esz) {
    const size_t bytes = align_up(elems * esz, 256);
    if (half) b.off2 = off; else { b.off = off; b.bytes = bytes; e->arena_bufs.push_back({name, &b}); }
    off += bytes;
  };
  auto idx = [](const char* name, int i) { return name + std::to_string(i); };
  take("sraw", e->sraw, B * p2 * 64, 2);
  take("stem", e->stem, B * p4 * 64, 2);
  take("S0", e->S[0], B * p4 * 256, 2);
  take("S1", e->S[1], B * p8 * 512, 2);
  take("S2", e->S[2], B * p16 * 1024, 2);
  take("T1", e->T1, B * p4 * 128, 2);  // largest conv1 output: stage1 block0 (128 ch @ 1/4 resolution)
  take("T2", e->T2, B * p4 * 64, 2);   // largest conv2 output: stage0 (64 ch @ 1/4 resolution)
  take("PA", e->PA, B * p4 * 256, 2);
  take("PB", e->PB, B * p4 * 256, 2);
  take("DS", e->DS, B * p4 * 256, 2);
  // GroupNorm partial records (32 groups x float2): p2/256 chunks for the stem, p4/32 MFMA row blocks for a stage conv
  for (int i = 0; i < 4; ++i) take(idx("part", i), e->part[i], B * (std::max(p2 / 256, p4 / 32) + 64) * 64, 4);
  take("gntab", e->gntab, B * 4 * 1024, 4);  // norm3 folded into conv3: the affines (a, d, ra, rd) per image and channel (<= 1024)
  take("X", e->X, B * S * DV, 4);
  take("lnst", e->lnst, B * S * 8 * 2, 4);  // LayerNorm fold: (sum, sum of squares) per token row and 128-column block (<= 8 blocks)
  take("Hn", e->Hn, B * S * DV, 2);
  take("QKV", e->QKV, B * S * 3 * DV, 2);
  take("AO", e->AO, B * S * DV, 2);
  take("F1", e->F1, B * S * (size_t)e->dm, 2);
  take("R3", e->R3, B * p16 * DV, 2);
  take("R4", e->R4, B * p16 * DV, 2);
  take("L3", e->L3, B * p16 * DV, 2);
  take("T4", e->T4, B * p16 * DV, 2);
  take("L4", e->L4, B * p32 * DV, 2);
  take("clsb", e->clsb, B * DV, 4);
  take("pos_alt", e->pos_alt, S * DV, 4);  // bilinearly resized pos_embed for inputs other than 384x384
  const size_t rn_px[4] = {p4, p8, p16, p32};
  for (int i = 0; i < 4; ++i) take(idx("lrn", i), e->lrn[i], B * rn_px[i] * FEAT, 2);
  take("tA", e->tA, B * p4 * FEAT, 2);
  take("tB", e->tB, B * p4 * FEAT, 2);
  take("tC", e->tC, B * p4 * FEAT, 2);
  const size_t p_px[4] = {p2, p4, p8, p16};  // P[0]=path_1 (1/2 res) ... P[3]=path_4 (1/16 res)
  for (int i = 0; i < 4; ++i) take(idx("P", i), e->P[i], B * p_px[i] * FEAT, 2);
  take("H0", e->H0, B * p2 * 128, 2);
  take("H0U", e->H0U, B * P * 128, 2);
  take("H1", e->H1, B * P * 32, 2);
  return off;
}

void plan_arena(dptx_engine* e) {
  const size_t full = plan_arena_for(e, (size_t)e->cfg.max_batch, false);
  const int ns = e->n_streams > 1 ? e->n_streams : 2;
  e->half_batch = (e->cfg.max_batch + ns - 1) / ns;
  e->half_region = align_up(plan_arena_for(e, (size_t)e->half_batch, true), 256);
  const size_t off = std::max(full, (size_t)ns * e->half_region);
  e->arena_single = off;
  const int npl = e->two_planes() ? 2 : 1;
  e->arena_bytes = off * npl;
  e->pl.act = npl == 2 ? (long long)(off / 2) : 0;
}

// ------------------------------------------------------------------------------- packing
int pack_host(dptx_engine* e) {
  std::string missing;
  for (const auto& s : e->spec)
    if (s.role != R_UNUSED && s.role != R_DERIVED && !e->staged.count(s.key)) missing += (missing.empty() ? "" : ", ") + s.key;
  if (!missing.empty()) return e->fail(DPTX_E_KEY, "missing tensors (strict load): " + missing);
  e->host_blob.assign(e->packed_bytes, 0);
  {
    const BlobHeader hd = e->blob_header();
    memcpy(e->host_blob.data(), &hd, sizeof hd);
  }
  const bool bf = e->bf16_storage();
  const bool x3 = e->two_planes() && !e->fp8();
  const size_t lo_elems = e->packed_single / 2;  // uint16 distance hi -> lo plane
  auto bf16_to_f32 = [](uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
  // writes element i of a 16-bit tensor (and its lo plane in bf16x3 mode)
  auto put = [&](uint16_t* d16, size_t i, float x) {
    if (!bf) {
      const uint16_t hi = f32_to_fp16(x);
      d16[i] = hi;
      if (x3) d16[i + lo_elems] = f32_to_fp16(x - fp16_to_f32(hi));
      return;
    }
    const uint16_t hi = f32_to_bf16(x);
    d16[i] = hi;
    if (x3) d16[i + lo_elems] = f32_to_bf16(x - bf16_to_f32(hi));
  };
  // value the MFMA sees for a packed single-plane operand element
  auto r16 = [&](float x) { return bf ? bf16_to_f32(f32_to_bf16(x)) : fp16_to_f32(f32_to_fp16(x)); };
  for (const auto& s : e->spec) {
    if (s.role == R_UNUSED || s.role == R_DERIVED) continue;
    const std::vector<float>& src = e->staged.at(s.key);
    uint8_t* dst = e->host_blob.data() + e->packed_off.at(s.key);
    // LayerNorm fold (kernels.h GemmParams::ln_stats): qkv / fc1 of every block become W' = W diag(gamma), b' = b + W beta
    // and the column sums of the ROUNDED W' go to the derived "...lnsum" entry
    const bool fold_w = e->ln_fold && s.role == R_LINEAR && (ends_with(s.key, "attn.qkv.weight") || ends_with(s.key, "mlp.fc1.weight"));
    const bool fold_b = e->ln_fold && s.role == R_VEC && (ends_with(s.key, "attn.qkv.bias") || ends_with(s.key, "mlp.fc1.bias"));
    if (fold_w || fold_b) {
      const bool qkv = s.key.find("attn.qkv") != std::string::npos;
      const std::string blk = s.key.substr(0, s.key.find(qkv ? "attn.qkv" : "mlp.fc1"));
      const std::string wkey = blk + (qkv ? "attn.qkv.weight" : "mlp.fc1.weight");
      const std::vector<float>& W = e->staged.at(wkey);
      const std::vector<float>& gamma = e->staged.at(blk + (qkv ? "norm1.weight" : "norm2.weight"));
      const std::vector<float>& beta = e->staged.at(blk + (qkv ? "norm1.bias" : "norm2.bias"));
      const size_t K = gamma.size(), N = W.size() / K;
      if (fold_b) {
        float* d32 = (float*)dst;
        for (size_t n = 0; n < N; ++n) {
          double acc = src[n];
          for (size_t k = 0; k < K; ++k) acc += (double)W[n * K + k] * (double)beta[k];
          d32[n] = (float)acc;
        }
      } else {
        uint16_t* d16 = (uint16_t*)dst;
        float* cs = (float*)(e->host_blob.data() + e->packed_off.at(blk + (qkv ? "attn.qkv.lnsum" : "mlp.fc1.lnsum")));
        for (size_t n = 0; n < N; ++n) {
          double acc = 0.0;
          for (size_t k = 0; k < K; ++k) {
            const float wf = W[n * K + k] * gamma[k];
            put(d16, n * K + k, wf);
            acc += (double)r16(wf);
          }
          cs[n] = (float)acc;
        }
      }
      continue;
    }
    if (s.role == R_VEC || s.role == R_HEAD4) {
      memcpy(dst, src.data(), src.size() * 4);
      continue;
    }
    if (s.role == R_DECONV_BIAS) {  // bias[co] for every one of the (up to 16) taps: column (tap*Cout + co) of the GEMM
      for (int t = 0; t < 16; ++t) memcpy(dst + (size_t)t * src.size() * 4, src.data(), src.size() * 4);
      continue;
    }
    uint16_t* d16 = (uint16_t*)dst;
    if (s.role == R_LINEAR) {
      for (size_t i = 0; i < src.size(); ++i) put(d16, i, src[i]);
      continue;
    }
    if (s.role == R_DECONV) {  // [Cin][Cout][k][k] -> GEMM operand W[(dy*k + dx)*Cout + co][ci]
      const int CI = (int)s.shape[0], CO = (int)s.shape[1], K = (int)s.shape[2];
      for (int ci = 0; ci < CI; ++ci)
        for (int co = 0; co < CO; ++co)
          for (int dy = 0; dy < K; ++dy)
            for (int dx = 0; dx < K; ++dx)
              put(d16, ((size_t)(dy * K + dx) * CO + co) * CI + ci, src[(((size_t)ci * CO + co) * K + dy) * K + dx]);
      continue;
    }
    // convolution OIHW -> [O][kh][kw][I]; StdConv2dSame weights are standardised first
    const int O = (int)s.shape[0], I = (int)s.shape[1], KH = (int)s.shape[2], KW = (int)s.shape[3];
    const size_t per_o = (size_t)I * KH * KW;
    const bool stem = (KH == 7);
    const size_t out_k = stem ? STEM_K : per_o;
    for (int o = 0; o < O; ++o) {
      const float* wo = src.data() + (size_t)o * per_o;
      double mean = 0.0, scale = 1.0;
      if (s.role == R_STDCONV) {
        double sum = 0.0;
        for (size_t i = 0; i < per_o; ++i) sum += wo[i];
        mean = sum / (double)per_o;
        double var = 0.0;
        for (size_t i = 0; i < per_o; ++i) { const double t = wo[i] - mean; var += t * t; }
        var /= (double)per_o;  // biased, as torch.std_mean(unbiased=False)
        scale = e->cfg.ws_form == 0 ? 1.0 / (std::sqrt(var) + (double)e->cfg.ws_eps)
                                    : 1.0 / std::sqrt(var + (double)e->cfg.ws_eps);
      }
      for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx)
          for (int i = 0; i < I; ++i) {
            const double wv = ((double)wo[((size_t)i * KH + ky) * KW + kx] - mean) * scale;
            // stem (stem.hip): k = (c*7 + ky)*8 + kx; every other conv: k = (ky*KW + kx)*I + c
            const size_t kidx = stem ? ((size_t)i * 7 + ky) * 8 + kx : ((size_t)ky * KW + kx) * I + i;
            put(d16, (size_t)o * out_k + kidx, (float)wv);
          }
    }
  }
  if (e->fp8()) {
    // e4m3 copies of the fp8 layers' weights (same [O][kh][kw][I] order as the bf16 copy, one byte per element, second
    // plane of the blob), quantised per OUTPUT CHANNEL after e4m3_channel_scale; the inverses go to the layer's "f8scale"
    // vector.
    for (size_t si = 0; si < e->spec.size(); ++si) {
      const Spec& sp = e->spec[si];
      if (sp.role != R_CONV || !dptx_engine::fp8_weight(sp.key)) continue;
      const size_t off = e->packed_off.at(sp.key);
      const std::vector<float>& src = e->staged.at(sp.key);
      const int O = (int)sp.shape[0], I = (int)sp.shape[1], KH = (int)sp.shape[2], KW = (int)sp.shape[3];
      const size_t per_o = (size_t)I * KH * KW;
      uint8_t* d8 = e->host_blob.data() + e->packed_single + off / 2;
      float* inv = (float*)(e->host_blob.data() + e->packed_off.at(sp.key.substr(0, sp.key.size() - 6) + "f8scale"));
      for (int o = 0; o < O; ++o) {
        float mx = 0.f;
        for (size_t i = 0; i < per_o; ++i) mx = std::max(mx, std::fabs(src[(size_t)o * per_o + i]));
        const float sc = e4m3_channel_scale(mx, &inv[o]);
        for (int ky = 0; ky < KH; ++ky)
          for (int kx = 0; kx < KW; ++kx)
            for (int i = 0; i < I; ++i)
              d8[(size_t)o * per_o + ((size_t)ky * KW + kx) * I + i] = f32_to_e4m3(src[(((size_t)o * I + i) * KH + ky) * KW + kx] * sc);
      }
    }
  }
  if (e->fp8()) {
    // e4m3 copies of qkv / fc1 / fc2 (DPTX_FLAG_FP8_VIT decides whether they are USED; they are always packed, so that the
    // blob's layout does not depend on the flag): the weight the bf16 GEMM multiplies -- folded with the LayerNorm's gamma for
    // qkv / fc1 -- per OUTPUT CHANNEL after a power-of-two scale into (224, 448]; "lnsum8" = column sums of the dequantised copy
    for (size_t si = 0; si < e->spec.size(); ++si) {
      const Spec& sp = e->spec[si];
      if (sp.role != R_LINEAR || !dptx_engine::fp8_vit_weight(sp.key)) continue;
      const std::vector<float>& W = e->staged.at(sp.key);
      const size_t N = (size_t)sp.shape[0], K = (size_t)sp.shape[1];
      const bool fc2 = ends_with(sp.key, "mlp.fc2.weight"), qkv = ends_with(sp.key, "attn.qkv.weight");
      const std::string stem_key = sp.key.substr(0, sp.key.size() - 6);   // "....attn.qkv." / "....mlp.fc1." / "....mlp.fc2."
      const std::string blk = sp.key.substr(0, sp.key.find(qkv ? "attn.qkv" : (fc2 ? "mlp.fc2" : "mlp.fc1")));
      const std::vector<float>* gamma = (!fc2 && e->ln_fold) ? &e->staged.at(blk + (qkv ? "norm1.weight" : "norm2.weight")) : nullptr;
      uint8_t* d8 = e->host_blob.data() + e->packed_single + e->packed_off.at(sp.key) / 2;
      float* inv = (float*)(e->host_blob.data() + e->packed_off.at(stem_key + "f8scale"));
      float* cs8 = fc2 ? nullptr : (float*)(e->host_blob.data() + e->packed_off.at(stem_key + "lnsum8"));
      for (size_t n = 0; n < N; ++n) {
        float mx = 0.f;
        for (size_t k = 0; k < K; ++k) mx = std::max(mx, std::fabs(W[n * K + k] * (gamma ? (*gamma)[k] : 1.0f)));
        const float sc = e4m3_channel_scale(mx, &inv[n]);
        double acc = 0.0;
        for (size_t k = 0; k < K; ++k) {
          const uint8_t q = f32_to_e4m3(W[n * K + k] * (gamma ? (*gamma)[k] : 1.0f) * sc);
          d8[n * K + k] = q;
          acc += (double)e4m3_to_f32(q);
        }
        if (cs8) cs8[n] = (float)(acc / (double)sc);
      }
    }
  }
  e->finalized = true;
  return DPTX_OK;
}

// ------------------------------------------------------------------------------ schedule
// What one GEMM of the schedule does besides the plain product (Run::conv, Run::rcu and Run::dense).
// Every call names what it sets: GemmOpt().bias(b).act(1)
enum { LN_NONE = 0, LN_CONSUMER = 1, LN_PRODUCER = 2 };
struct GemmOpt {
  const float* bias_ = nullptr;
  int act_ = 0, a_relu_ = 0;                  // GemmParams::act / a_relu
  const void *R1_ = nullptr, *R2_ = nullptr;  // residuals
  // fp8 dtype: the epilogue also writes the e4m3 copy of the output, for a consumer that multiplies on e4m3 operands (one
  // calibrated power-of-two scale per tensor); 2 (conv): ReLU'd, for consumers that pre-activate
  int q_ = 0;
  // conv: != nullptr: the epilogue also writes the GroupNorm(32) statistics of the output (per 32-row block records,
  // kernels.h GemmParams::gn_part); the caller checked gn_fusable(Hout * Wout)
  float* gn_part_ = nullptr;
  // conv, MIXED dtype, decoder groups only (-1 elsewhere): 1 = some consumer multiplies this tensor with 3 MFMAs and needs
  // its lo plane, 0 = nobody reads it.  The layer's own arithmetic follows dptx_engine::layer_x3.
  int out_lo_ = -1;
  int c_fp32_ = 0, r1_fp32_ = 0;  // dense: C / R1 is the fp32 token stream
  // dense: the layer's part in the folded LayerNorm -- consumer (qkv, fc1: normalises in the epilogue, with the column sums
  // `colsum` of its folded weight; only a consumer reads them) or producer (proj, fc2: 16-bit copy + row statistics of the
  // stream it writes)
  int ln_ = LN_NONE;
  const float* colsum_ = nullptr;
  GemmOpt& bias(const float* v) { bias_ = v; return *this; }
  GemmOpt& act(int v) { act_ = v; return *this; }
  GemmOpt& a_relu(int v) { a_relu_ = v; return *this; }
  GemmOpt& R1(const void* v) { R1_ = v; return *this; }
  GemmOpt& R2(const void* v) { R2_ = v; return *this; }
  GemmOpt& q(int v) { q_ = v; return *this; }
  GemmOpt& gn_part(float* v) { gn_part_ = v; return *this; }
  GemmOpt& out_lo(int v) { out_lo_ = v; return *this; }
  GemmOpt& c_fp32(int v) { c_fp32_ = v; return *this; }
  GemmOpt& r1_fp32(int v) { r1_fp32_ = v; return *this; }
  GemmOpt& ln(int v) { ln_ = v; return *this; }
  GemmOpt& colsum(const float* v) { colsum_ = v; return *this; }
};

struct Run {
  dptx_engine* e;
  int B;
  hipStream_t st;
  int dt;
  int Hi = 384, Wi = 384;  // input size (multiples of 32)
  int io = 0;              // element type of the caller's x / y buffers (DPTX_IO_*)
  size_t abase = 0;        // byte offset of this run's arena region
  bool half = false;       // half-batch plan (Buf::off2) instead of the whole-batch plan
  hipError_t err = hipSuccess;
  const char* where = "";
  int64_t launches = 0;    // accounting of this run (copied to the engine by the caller)
  double exec_macs = 0.0, cat_macs[4] = {0, 0, 0, 0};
  // fp8: slot (dptx_engine::act_scale index) of the latest e4m3 copy of an arena buffer; slots count up in launch order
  std::unordered_map<const void*, int> q8_slot;
  int q8_count = 0;
  int q8_produce(const void* out) {
    const int slot = q8_count < dptx_engine::MAX_Q8 ? q8_count : dptx_engine::MAX_Q8 - 1;
    ++q8_count;
    q8_slot[out] = slot;
    return slot;
  }
  float q8_scale_of(const void* in) const {
    auto it = q8_slot.find(in);
    return it == q8_slot.end() ? 1.0f : e->act_scale[it->second];
  }
  // calibration forwards (dptx_calibrate_fp8) measure max |x| of every tensor that gets an e4m3 copy
  void q8_measure(const void* out, size_t n, int relu, int slot) {
    if (e->calibrating && e->d_amax) chk(launch_amax(MODE_BF16, out, n, relu, e->d_amax + slot, st), "fp8.amax");
  }
  // the epilogue of p also writes the e4m3 copy of its output `out`, which takes the next slot (returned)
  int fp8_copy(GemmParams& p, const void* out, int relu) {
    const int slot = q8_produce(out);
    gemm_add_fp8_copy(p, e->q8(out), relu, e->act_scale[slot]);
    return slot;
  }
  // p multiplies the e4m3 copies of `in` and of the weight; the accumulators are rescaled by the inverses of their scales
  void fp8_operands(GemmParams& p, const void* in, const std::string& wkey) {
    gemm_use_fp8_operands(p, e->q8(in), e->w8(wkey), 1.0f / q8_scale_of(in), e->wscale(wkey));
  }

  char* A(const Buf& b) const { return e->d_arena + abase + (half ? b.off2 : b.off); }

  void chk(hipError_t r, const char* w, int cat = 3) {
    if (err == hipSuccess && r != hipSuccess) { err = r; where = w; }
    launches++;
    if (e->profiling) {
      const size_t i = e->event_cat.size() + 1;  // events[0] marks the start of the forward
      if (i >= e->events.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return;
        e->events.push_back(ev);
      }
      (void)hipEventRecord(e->events[i], st);
      e->event_cat.push_back(cat);
      e->event_name.emplace_back(w);
    }
  }
  // one GEMM of the schedule: its MACs per image (executed and algorithmic), then the launch
  void gemm(int mode, const GemmParams& p, const char* name) {
    exec_macs += (double)p.M / B * p.N * p.K;
    cat_macs[0] += (double)p.M / B * p.N * p.K;
    chk(launch_gemm(mode, p, st), name, 0);
  }
  // MIXED dtype, decoder groups: which arena tensors currently have a valid lo plane (set by their producers)
  std::unordered_map<const void*, bool> lo_valid_;
  bool has_lo(const void* p) const {
    auto it = lo_valid_.find(p);
    return it != lo_valid_.end() && it->second;
  }
  void mark_lo(const void* p, bool v) { lo_valid_[p] = v; }
  int cur_group = 0;
  void tap(const char* name, const void* p, int64_t h, int64_t w, int64_t c, bool fp32 = false) {
    int m = dt;
    if (e->mixed() && lo_valid_.count(p)) m = has_lo(p) ? MODE_FP16X3 : MODE_FP16;  // decoder tensors: by their own planes
    e->taps[name] = TapInfo{p, {B, h, w, c}, fp32, m};
  }
  void group(int g) { dt = e->mode_of(g); cur_group = g; }  // the launches that follow belong to layer group g

  // NHWC convolution as implicit GEMM
  void conv(const void* in, int Hin, int Win, int Cin, const std::string& wkey, int ksz, int stride, int pad_t, int pad_l,
            int Hout, int Wout, int Cout, void* out, const GemmOpt& o = GemmOpt()) {
    // fp8 dtype: a conv whose weight has an e4m3 copy runs on the fp8 MFMA, reading the e4m3 copy of `in` (ReLU'd by its
    // producer)
    // (a calibration forward runs these convs on their bf16 operands: a saturated e4m3 copy upstream must not distort the
    // max |x| measured downstream)
    const bool f8 = e->fp8_use(wkey) && !e->calibrating;
    GemmParams p;
    gemm_params_conv(p, B, Hin, Win, Cin, Cout, ksz, stride, pad_t, pad_l, Hout, Wout, f8 ? 1 : 2);
    p.A = in; p.W = e->w(wkey); p.C = out; p.bias = o.bias_; p.R1 = o.R1_; p.R2 = o.R2_;
    const int slot = e->fp8() && o.q_ ? fp8_copy(p, out, o.q_ == 2) : -1;
    p.act = o.act_; p.a_relu = o.a_relu_; p.planes = e->pl;
    if (o.gn_part_) gemm_add_gn_records(p, o.gn_part_, Hout * Wout);
    if (f8) fp8_operands(p, in, wkey);
    int mode = f8 ? MODE_FP8 : dt;
    if (o.out_lo_ >= 0 && e->mixed()) {  // per-layer policy
      const bool x3 = e->layer_x3(wkey, cur_group), a_lo = e->layer_reads_lo(wkey, cur_group);
      if (a_lo && !has_lo(in)) {  // cannot happen with the schedule below: every producer honours its consumers' needs
        if (err == hipSuccess) { err = hipErrorInvalidValue; where = "precision policy: a 3-MFMA layer reads a tensor without lo plane"; }
        return;
      }
      const bool r1lo = o.R1_ != nullptr && has_lo(o.R1_), r2lo = o.R2_ != nullptr && has_lo(o.R2_);
      mode = gemm_set_plane_policy(p, x3, a_lo, r1lo, r2lo, o.out_lo_ != 0);
      mark_lo(out, o.out_lo_ != 0);
    }
    gemm(mode, p, wkey.c_str());
    if (slot >= 0) q8_measure(out, (size_t)p.M * p.N, o.q_ == 2, slot);
  }

  // GroupNorm statistics come out of the producing conv's epilogue when an image's rows are whole 32-row MFMA blocks
  // (always at 384x384)
  static bool gn_fusable(int HW) { return HW % 32 == 0; }
  void gn_stats(const void* X, float* part, int HW, int C) { chk(launch_gn_stats(dt, X, part, B, HW, C, e->pl, st), "gn_stats", 2); }
  void gn_apply(void* X, const std::string& nkey, float* part, int HW, int C, int relu, const void* R = nullptr,
                const std::string& rkey = "", const float* rpart = nullptr) {
    GnParams g = gn_params(X, X, e->f(nkey + ".weight"), e->f(nkey + ".bias"), part, B, HW, C, relu, 1e-5f, gn_fusable(HW));
    if (rkey.empty()) gn_add_residual(g, R);
    else gn_add_residual(g, R, e->f(rkey + ".weight"), e->f(rkey + ".bias"), rpart);
    chk(launch_gn_apply(dt, g, e->pl, st), nkey.c_str(), 2);
  }

  // conv3 + norm3 of a bottleneck without the raw map (conv1x1.hip C1_STATS / C1_GN): the streaming kernel runs a statistics
  // pass that stores nothing but the records, gn_finalize turns them (and, in a stage's first block, those of the downsample
  // branch) into affine tables, and a second pass of the kernel applies GroupNorm + shortcut + ReLU in its epilogue -- the
  // bits of conv() followed by gn_apply().  Returns false, having launched nothing, where the form cannot run or was not
  // adopted for the (K, N) class (debug flags 32 / 64): the caller then takes that schedule.
  bool conv_gn_folded(const void* in, int H, int W, int Cin, const std::string& wkey, int Cout, void* out, const std::string& nkey,
                      float* part, int relu, const void* R, const std::string& rkey = "", const float* rpart = nullptr) {
    const int flags = gemm_debug_flags();
    if ((flags & (8 | 32)) || !gn_fusable(H * W) || out == R || (e->fp8_use(wkey) && !e->calibrating)) return false;
    GemmParams p;
    gemm_params_conv(p, B, H, W, Cin, Cout, 1, 1, 0, 0, H, W, 2);
    p.A = in; p.W = e->w(wkey); p.C = out; p.planes = e->pl;
    if (!conv1x1_gn_eligible(dt, p) || !((flags & 64) || conv1x1_gn_adopted(p))) return false;
    const bool r_gn = !rkey.empty();
    const ConvGnFold f{part, e->f(nkey + ".weight"), e->f(nkey + ".bias"), R, r_gn ? rpart : nullptr,
                       r_gn ? e->f(rkey + ".weight") : nullptr, r_gn ? e->f(rkey + ".bias") : nullptr, (float*)A(e->gntab), relu,
                       1e-5f};
    const double macs = (double)p.M / B * p.N * p.K;
    exec_macs += macs; cat_macs[0] += macs;
    chk(launch_conv1x1_gn_pass(dt, p, f, C1_PASS_STATS, st), (wkey + ".stats").c_str(), 0);
    chk(launch_conv1x1_gn_pass(dt, p, f, C1_PASS_FINALIZE, st), (nkey + ".finalize").c_str(), 2);
    exec_macs += macs; cat_macs[0] += macs;
    chk(launch_conv1x1_gn_pass(dt, p, f, C1_PASS_EPILOGUE, st), wkey.c_str(), 0);
    return true;
  }

  // RCU (blocks.py:263-286): out = conv2(relu(conv1(relu(x)))) + x (+ o.R2)
  // Of `o` the unit reads R2 (the extra summand), q (fp8 dtype: e4m3 copy of the unit's output -- 2 when its consumer
  // pre-activates (another RCU), 1 otherwise) and out_lo (MIXED per-layer policy: does a consumer of the unit's output need
  // its lo plane)
  void rcu(const std::string& p, const void* x, int H, int W, void* tmp, void* out, const GemmOpt& o) {
    const int mid_lo = e->mixed() ? (int)e->layer_reads_lo(p + "conv2.weight", cur_group) : -1;
    conv(x, H, W, FEAT, p + "conv1.weight", 3, 1, 1, 1, H, W, FEAT, tmp,
         GemmOpt().bias(e->f(p + "conv1.bias")).act(1).a_relu(1).q(e->fp8_use(p + "conv2.weight") ? 1 : 0).out_lo(mid_lo));
    conv(tmp, H, W, FEAT, p + "conv2.weight", 3, 1, 1, 1, H, W, FEAT, out,
         GemmOpt().bias(e->f(p + "conv2.bias")).R1(x).R2(o.R2_).q(o.q_).out_lo(e->mixed() ? o.out_lo_ : -1));
  }

  // ---- one forward: the geometry and the pointers every stage uses (begin() fills them), then the stages in schedule order
  const std::string vp = "pretrained.model.";
  const void* x = nullptr;   // the caller's input
  int D_VIT = 0, D_MLP = 0, N_HEADS = 0;
  bool large = false;        // DPT-Large (vitl16_384): no ResNet, patchify + 24 blocks, four readouts
  float *part0 = nullptr, *part1 = nullptr, *part2 = nullptr, *part3 = nullptr;  // GroupNorm records
  int h2 = 0, w2 = 0, h4 = 0, w4 = 0, gh = 0, gw = 0, h32 = 0, w32 = 0;
  int NP = 0;                // patch tokens per image (576 at 384x384)
  int S = 0;                 // + cls
  int M = 0;                 // token rows of the batch
  size_t tok_elems = 0;
  const float* pos = nullptr;  // position embedding of this input's patch grid
  float* X = nullptr;          // fp32 token stream
  // LayerNorm fold (kernels.h GemmParams::ln_stats): every launch that writes the fp32 token stream also writes its 16-bit
  // copy into Hn and the per-row (sum, sum of squares) records into lnst; qkv / fc1 read Hn and normalise in the epilogue
  float* lnst = nullptr;
  int ln_nblk = 0;    // records per token row (6 or 8; the row stride is always 8)
  bool s16 = false;   // Hn is the (16-bit) token stream; X is not written
  int hn_slot = -1;   // fp8 ViT: calibration slot of the token stream's latest e4m3 copy
  bool mx = false;    // MIXED dtype

  void begin(const void* x_in);
  void resnet();
  void embed();
  void tok_tap(int idx, const char* name);
  void dense(const void* in, const std::string& wkey, int N, int K, void* C, const GemmOpt& o);
  void vit_block(int l);
  void readout(int n);
  void mark_encoder_planes();
  void decode(const std::string& pre, int ch, void* yout);
  int finish();
  int forward(const void* x_in, void* y, void* y2);

  // MIXED dtype, decoder groups (false / -1 / dt elsewhere)
  bool X3(const std::string& key, int grp) const { return mx && e->layer_x3(key, grp); }            // computes with lo planes
  bool RLO(const std::string& key, int grp) const { return mx && e->layer_reads_lo(key, grp); }   // reads its input's lo plane
  int lo_of(bool need) const { return mx ? (int)need : -1; }
  int planes_mode(const void* t) const { return mx ? (has_lo(t) ? MODE_FP16X3 : MODE_FP16) : dt; }  // elementwise kernels
};

// The schedule of one forward, stage by stage (DPT.forward, dpt_depth.py:67-85)
int Run::forward(const void* x_in, void* y, void* y2) {
  begin(x_in);
  if (!large) resnet();
  embed();
  // ---- 12 (24) transformer blocks (timm Block; LN eps 1e-6) -------------------------------
  for (int l = 0; l < e->depth; ++l) {
    vit_block(l);
    if (large) {
      if (l % 6 == 5) readout(l / 6 + 1);  // dpt_depth.py:41-45 hooks [5, 11, 17, 23]
    } else {
      if (l == 8) readout(3);  // hooks [0, 1, 8, 11]: the first two are the ResNet stages
      if (l == 11) readout(4);
    }
  }
  // timm's final model.norm is dead compute in the reference (vit.py:153, result discarded :64)
  mark_encoder_planes();
  decode("", e->cfg.num_channels, y);
  if (e->cfg.dual_task) {
    // the second decoder re-uses the first one's arena buffers: the first one's stage taps are gone (debug a decoder
    // with a single-task handle -- its results are bit-identical)
    for (const char* n : {"l1_rn", "l2_rn", "l3_rn", "l4_rn", "p1", "p2", "p3", "p4", "h0", "h1"}) e->taps.erase(n);
    decode("depth.", 1, y2);
  }
  return finish();
}

void Run::begin(const void* x_in) {
  x = x_in;
  e->taps.clear();
  e->event_cat.clear();
  e->event_name.clear();
  if (e->profiling) {
    if (e->events.empty()) {
      hipEvent_t ev;
      if (hipEventCreate(&ev) == hipSuccess) e->events.push_back(ev);
    }
    if (!e->events.empty()) (void)hipEventRecord(e->events[0], st);
  }
  D_VIT = e->dv; D_MLP = e->dm; N_HEADS = e->nh;
  large = e->backbone == DPTX_BACKBONE_VITL16_384;
  part0 = (float*)A(e->part[0]);
  part1 = (float*)A(e->part[1]);
  part2 = (float*)A(e->part[2]);
  part3 = (float*)A(e->part[3]);
  h2 = Hi / 2; w2 = Wi / 2; h4 = Hi / 4; w4 = Wi / 4; gh = Hi / 16; gw = Wi / 16; h32 = Hi / 32; w32 = Wi / 32;
  NP = gh * gw;
  S = NP + 1;
  M = B * S;
  tok_elems = (size_t)M * D_VIT;
  X = (float*)A(e->X);
  lnst = (float*)A(e->lnst);
  ln_nblk = D_VIT / 128;
  s16 = e->stream16;
  mx = e->mixed();
  const bool native = (gh == 24 && gw == 24);
  pos = e->f("pretrained.model.pos_embed");
  if (!native) {  // vit.py:119-125: forward_flex resizes pos_embed to the input's patch grid on every call
    chk(launch_pos_resize(pos, (float*)A(e->pos_alt), 24, gh, gw, D_VIT, st), "pos_resize");
    pos = (const float*)A(e->pos_alt);
  }
}

int Run::finish() {
  e->n_q8 = q8_count < dptx_engine::MAX_Q8 ? q8_count : dptx_engine::MAX_Q8;
  if (err != hipSuccess) return e->fail(DPTX_E_HIP, std::string("launch failed at ") + where + ": " + hipGetErrorString(err));
  return DPTX_OK;
}

// ---- the ResNetV2 of the hybrid model: stem, then stages (3,4,9)
void Run::resnet() {
  const std::string bp = vp + "patch_embed.backbone.";
  // ---- stem: fused conv7x7 s2 SAME (stem.hip, no im2col) -> GN+ReLU -> MaxPool2dSame(3,2) ---------
  group(DPTX_GROUP_RESNET);
  chk(launch_stem_conv(dt, x, io, e->w(bp + "stem.conv.weight"), A(e->sraw), B, Hi, Wi, e->pl, st), "stem.conv", 0);
  exec_macs += (double)h2 * w2 * 64 * STEM_K;
  cat_macs[0] += (double)h2 * w2 * 64 * STEM_K;
  gn_stats(A(e->sraw), part0, h2 * w2, 64);
  chk(launch_gn_relu_maxpool(dt, A(e->sraw), A(e->stem), e->f(bp + "stem.norm.weight"), e->f(bp + "stem.norm.bias"),
                             part0, B, h2, w2, 64, 1e-5f, e->pl, st),
      "stem.pool", 2);
  tap("stem", A(e->stem), h4, w4, 64);

  // ---- ResNetV2 stages (3,4,9) non-preact bottlenecks -----------------------------------
  const void* cur = A(e->stem);
  int H = h4, Wd = w4, cin = 64;
  for (int s = 0; s < 3; ++s) {
    const int cout = STAGE_OUT[s], mid = cout / 4;
    for (int b = 0; b < STAGE_DEPTH[s]; ++b) {
      const std::string p = bp + "stages." + std::to_string(s) + ".blocks." + std::to_string(b) + ".";
      const int stride = (b == 0) ? STAGE_STRIDE[s] : 1;
      const int Ho = H / stride, Wo = Wd / stride;
      void* out = (b == STAGE_DEPTH[s] - 1) ? (void*)A(e->S[s]) : (void*)((b & 1) ? A(e->PB) : A(e->PA));
      const bool f_in = gn_fusable(H * Wd), f_out = gn_fusable(Ho * Wo);  // statistics from the conv epilogues
      if (b == 0) {
        conv(cur, H, Wd, cin, p + "downsample.conv.weight", 1, stride, 0, 0, Ho, Wo, cout, A(e->DS), GemmOpt().gn_part(f_out ? part3 : nullptr));
        if (!f_out) gn_stats(A(e->DS), part3, Ho * Wo, cout);
      }
      conv(cur, H, Wd, cin, p + "conv1.weight", 1, 1, 0, 0, H, Wd, mid, A(e->T1), GemmOpt().gn_part(f_in ? part0 : nullptr));
      if (!f_in) gn_stats(A(e->T1), part0, H * Wd, mid);
      gn_apply(A(e->T1), p + "norm1", part0, H * Wd, mid, 1);
      // 3x3, stride on conv2 (V1.5); TF-SAME: s1 -> pad (1,1); s2 on even H -> pad (0,1)
      const int pad = (stride == 1) ? 1 : 0;
      conv(A(e->T1), H, Wd, mid, p + "conv2.weight", 3, stride, pad, pad, Ho, Wo, mid, A(e->T2), GemmOpt().gn_part(f_out ? part1 : nullptr));
      if (!f_out) gn_stats(A(e->T2), part1, Ho * Wo, mid);
      gn_apply(A(e->T2), p + "norm2", part1, Ho * Wo, mid, 1);
      // conv3 + norm3 (+ shortcut + ReLU): folded into two passes of the streaming kernel where that was adopted
      const bool folded = b == 0 ? conv_gn_folded(A(e->T2), Ho, Wo, mid, p + "conv3.weight", cout, out, p + "norm3", part2, 1, A(e->DS),
                                                  p + "downsample.norm", part3)
                                 : conv_gn_folded(A(e->T2), Ho, Wo, mid, p + "conv3.weight", cout, out, p + "norm3", part2, 1, cur);
      if (!folded) {
        conv(A(e->T2), Ho, Wo, mid, p + "conv3.weight", 1, 1, 0, 0, Ho, Wo, cout, out, GemmOpt().gn_part(f_out ? part2 : nullptr));
        if (!f_out) gn_stats(out, part2, Ho * Wo, cout);
        if (b == 0)
          gn_apply(out, p + "norm3", part2, Ho * Wo, cout, 1, A(e->DS), p + "downsample.norm", part3);
        else
          gn_apply(out, p + "norm3", part2, Ho * Wo, cout, 1, cur);
      }
      cur = out;
      H = Ho;
      Wd = Wo;
      cin = cout;
    }
    const char* names[3] = {"s0", "s1", "s2"};
    tap(names[s], cur, H, Wd, cout);
  }
}

// ---- tokens: 1x1 proj + bias + pos_embed -> fp32 stream X[b*S + 1 + p] (S = 577 at 384x384); cls rows ----
void Run::embed() {
  group(DPTX_GROUP_EMBED);
  {
    // hybrid: the 1x1 projection of the ResNet's 1/16-resolution map (K = 1024); DPT-Large: timm PatchEmbed, a 16x16
    // stride-16 convolution = a dense GEMM over the patch matrix (K = 3*16*16 = 768, misc.hip patchify16)
    const int Kp = large ? 768 : 1024;
    // (the patch matrix lives in F1, which is free here: Hn receives the 16-bit copy of the token stream below)
    if (large) chk(launch_patchify16(dt, x, io, A(e->F1), B, Hi, Wi, e->pl, st), "patchify");
    GemmParams p;
    gemm_params_patch_embed(p, B, NP, S, D_VIT, Kp);
    p.A = large ? A(e->F1) : A(e->S[2]); p.W = e->w(vp + "patch_embed.proj.weight"); p.C = X;
    p.bias = e->f(vp + "patch_embed.proj.bias");
    p.R2 = pos; p.planes = e->pl;
    if (s16) { p.C = A(e->Hn); p.c_fp32 = 0; }  // the 16-bit tensor is the stream itself
    if (e->ln_fold) gemm_add_ln_producer(p, s16 ? nullptr : A(e->Hn), lnst);
    // fp8 ViT (DPTX_FLAG_FP8_VIT): block 0's qkv multiplies the e4m3 copy of the stream
    hn_slot = e->fp8_use(vp + "blocks.0.attn.qkv.weight") ? fp8_copy(p, A(e->Hn), 0) : -1;
    gemm(dt, p, "patch_embed.proj");
  }
  chk(launch_cls_rows(e->mode_of(DPTX_GROUP_VIT), e->f(vp + "cls_token"), pos, s16 ? nullptr : X, B, S, D_VIT,
                      e->ln_fold ? A(e->Hn) : nullptr, e->ln_fold ? lnst : nullptr, st,
                      hn_slot >= 0 ? e->q8(A(e->Hn)) : nullptr, hn_slot >= 0 ? e->act_scale[hn_slot] : 1.0f),
      "cls_rows");
  if (hn_slot >= 0) q8_measure(A(e->Hn), (size_t)B * S * D_VIT, 0, hn_slot);
  tok_tap(0, "tok0");
}

void Run::tok_tap(int idx, const char* name) {
  if (!e->taps_on) return;
  float* dst = e->d_tok_taps + (size_t)idx * e->tok_tap_stride;
  if (s16) {  // debug copy: not a launch of the schedule (not counted, not timed)
    const hipError_t r = launch_to_f32(e->mode_of(DPTX_GROUP_VIT), A(e->Hn), dst, tok_elems, e->pl, st);
    if (err == hipSuccess && r != hipSuccess) { err = r; where = "tok_tap"; }
  } else if (err == hipSuccess) {
    err = hipMemcpyAsync(dst, X, tok_elems * 4, hipMemcpyDeviceToDevice, st);
  }
  e->taps[name] = TapInfo{dst, {B, S, D_VIT, 1}, true, dt};
}

// One linear layer of a transformer block over the M token rows
void Run::dense(const void* in, const std::string& wkey, int N, int K, void* C, const GemmOpt& o) {
  const bool f8 = e->fp8_use(wkey) && !e->calibrating;  // e4m3 operands: the e4m3 copies of A and of the (folded) weight
  GemmParams p;
  gemm_params_dense(p, M, N, K, f8 ? 1 : 2);
  p.A = in; p.W = e->w(wkey); p.C = C; p.c_fp32 = o.c_fp32_; p.bias = o.bias_; p.act = o.act_;
  p.R1 = o.R1_; p.r1_fp32 = o.r1_fp32_; p.planes = e->pl;
  if (o.ln_ == LN_CONSUMER)
    gemm_add_ln_consumer(p, lnst, f8 ? e->f(wkey.substr(0, wkey.size() - 6) + "lnsum8") : o.colsum_, ln_nblk, 1e-6f);
  if (o.ln_ == LN_PRODUCER) {
    if (s16) {  // in place on the 16-bit stream: every thread reads exactly the elements it then writes
      p.C = A(e->Hn); p.c_fp32 = 0; p.R1 = A(e->Hn); p.r1_fp32 = 0;
    }
    gemm_add_ln_producer(p, s16 ? nullptr : A(e->Hn), lnst);
  }
  if (f8) fp8_operands(p, in, wkey);
  const int slot = o.q_ ? fp8_copy(p, p.C, 0) : -1;
  gemm(f8 ? MODE_FP8 : dt, p, wkey.c_str());
  if (slot >= 0) q8_measure(p.C, (size_t)M * N, 0, slot);
}

// ProjectReadout + reassemble for hook n (hybrid: 3 -> block 8, 4 -> block 11; DPT-Large: 1..4 -> blocks 5, 11, 17, 23,
// n = 1, 2 followed by a ConvTranspose2d with kernel == stride: a GEMM whose N enumerates (dy, dx, co) + a re-layout)
void Run::readout(int n) {
  group(DPTX_GROUP_REASSEMBLE);
  const std::string pp = "pretrained.act_postprocess" + std::to_string(n) + ".";
  float* clsb = (float*)A(e->clsb);
  chk(launch_readout_cls(dt, s16 ? (const float*)A(e->Hn) : X, (long long)S * D_VIT, e->w(pp + "0.project.0.weight"), 2 * D_VIT,
                         D_VIT, e->f(pp + "0.project.0.bias"), clsb, B, D_VIT, D_VIT, e->pl, st, s16 ? 1 : 0),
      "readout_cls");
  // the token GEMM reads a 16-bit image of the fp32 stream: with the LayerNorm fold the last fc2 epilogue has already
  // written it (single-plane: the fold implies single-pass ViT blocks; a 3-MFMA reassemble group then still needs the
  // lo plane, so it casts); otherwise Hn is free between blocks
  if (!(e->ln_fold && !mode_is_x3(dt))) chk(launch_cast_f32(dt, X, A(e->Hn), (size_t)B * S * D_VIT, e->pl, st), "readout_cast");
  exec_macs += (double)D_VIT * D_VIT;  // per image
  void* R = (n & 1) ? A(e->R3) : A(e->R4);
  GemmParams p;
  gemm_params_readout(p, B, NP, S, D_VIT);
  p.A = A(e->Hn); p.planes = e->pl;
  p.W = e->w(pp + "0.project.0.weight"); p.C = R;
  p.bias = clsb; p.act = 2;
  gemm(dt, p, "readout");
  const int f = n == 1 ? 256 : (n == 2 ? 512 : D_VIT);  // n <= 2: DPT-Large only
  conv(R, gh, gw, D_VIT, pp + "3.weight", 1, 1, 0, 0, gh, gw, f, n == 3 ? A(e->L3) : A(e->T4), GemmOpt().bias(e->f(pp + "3.bias")));
  if (n <= 2) {
    const int k = n == 1 ? 4 : 2;
    GemmParams d;
    gemm_params_dense(d, B * NP, k * k * f, f);
    d.A = A(e->T4); d.W = e->w(pp + "4.weight"); d.C = A(e->F1); d.bias = e->f(pp + "4.bias"); d.planes = e->pl;
    gemm(dt, d, "reassemble.deconv");
    chk(launch_depth_to_space(dt, A(e->F1), A(e->S[n - 1]), B, gh, gw, k, f, e->pl, st), "reassemble.d2s");
    tap(n == 1 ? "l1" : "l2", A(e->S[n - 1]), gh * k, gw * k, f);
  } else if (n == 3) {
    tap("l3", A(e->L3), gh, gw, D_VIT);
  } else {
    conv(A(e->T4), gh, gw, D_VIT, pp + "4.weight", 3, 2, 1, 1, h32, w32, D_VIT, A(e->L4), GemmOpt().bias(e->f(pp + "4.bias")));
    tap("l4", A(e->L4), h32, w32, D_VIT);
  }
}

// one transformer block (timm Block; LN eps 1e-6)
void Run::vit_block(int l) {
  group(DPTX_GROUP_VIT);
  const std::string p = vp + "blocks." + std::to_string(l) + ".";
  const bool lf = e->ln_fold;
  const int ln_in = lf ? LN_CONSUMER : LN_NONE, ln_out = lf ? LN_PRODUCER : LN_NONE;  // qkv, fc1 / proj, fc2
  if (!lf) chk(launch_layernorm(dt, X, e->f(p + "norm1.weight"), e->f(p + "norm1.bias"), A(e->Hn), M, D_VIT, 1e-6f, e->pl, st), "ln1", 2);
  // fp8 ViT: the tensors that an e4m3 GEMM reads get their e4m3 copy from the epilogue that produces them -- the stream
  // after proj (fc1's operand), the GELU output (fc2's), the stream after fc2 (the next block's qkv)
  const std::string pn = vp + "blocks." + std::to_string(l + 1) + ".";
  const bool q_fc1 = e->fp8_use(p + "mlp.fc1.weight"), q_fc2 = e->fp8_use(p + "mlp.fc2.weight");
  const bool q_next = l + 1 < e->depth && e->fp8_use(pn + "attn.qkv.weight");
  dense(A(e->Hn), p + "attn.qkv.weight", 3 * D_VIT, D_VIT, A(e->QKV),
        GemmOpt().bias(e->f(p + "attn.qkv.bias")).ln(ln_in).colsum(e->f(p + "attn.qkv.lnsum")));
  chk(launch_attention(dt, A(e->QKV), A(e->AO), B, S, N_HEADS, e->pl, st), "attention", 1);
  exec_macs += 2.0 * N_HEADS * (double)S * S * 64;
  cat_macs[1] += 2.0 * N_HEADS * (double)S * S * 64;
  dense(A(e->AO), p + "attn.proj.weight", D_VIT, D_VIT, X,
        GemmOpt().c_fp32(1).bias(e->f(p + "attn.proj.bias")).R1(X).r1_fp32(1).ln(ln_out).q(q_fc1));
  if (!lf) chk(launch_layernorm(dt, X, e->f(p + "norm2.weight"), e->f(p + "norm2.bias"), A(e->Hn), M, D_VIT, 1e-6f, e->pl, st), "ln2", 2);
  dense(A(e->Hn), p + "mlp.fc1.weight", D_MLP, D_VIT, A(e->F1),
        GemmOpt().bias(e->f(p + "mlp.fc1.bias")).act(2).ln(ln_in).colsum(e->f(p + "mlp.fc1.lnsum")).q(q_fc2));
  dense(A(e->F1), p + "mlp.fc2.weight", D_VIT, D_MLP, X,
        GemmOpt().c_fp32(1).bias(e->f(p + "mlp.fc2.bias")).R1(X).r1_fp32(1).ln(ln_out).q(q_next));
  char nm[16];
  snprintf(nm, sizeof nm, "blk%d", l);
  tok_tap(l + 1, nm);
}

// MIXED dtype: the decoder groups follow the per-LAYER precision table (dptx_engine::layer_prec); a producer writes the lo
// plane of its output exactly when a consumer multiplies it with 3 MFMAs (or, for the path tensors, when it was computed
// with 3 MFMAs itself), whatever its own arithmetic is.  The encoder's outputs carry lo planes when their groups are 3-MFMA.
void Run::mark_encoder_planes() {
  if (mx) {
    const bool enc_lo = mode_is_x3(e->mode_of(large ? DPTX_GROUP_REASSEMBLE : DPTX_GROUP_RESNET));
    const bool re_lo = mode_is_x3(e->mode_of(DPTX_GROUP_REASSEMBLE));
    mark_lo(A(e->S[0]), enc_lo); mark_lo(A(e->S[1]), enc_lo); mark_lo(A(e->L3), re_lo); mark_lo(A(e->L4), re_lo);
  }
}

// one decoder = scratch.* of one task ("" -> scratch.*, "depth." -> depth.scratch.*); the dual-task engine runs two
// on the same encoder outputs (S[0], S[1], L3, L4 are not modified by a decoder)
void Run::decode(const std::string& pre, int ch, void* yout) {
  // ---- scratch.layerN_rn (3x3, no bias) ---------------------------------------------------
  const void* rn_in[4] = {A(e->S[0]), A(e->S[1]), A(e->L3), A(e->L4)};
  const int rn_h[4] = {h4, Hi / 8, gh, h32};
  const int rn_w[4] = {w4, Wi / 8, gw, w32};
  const int rn_c[4] = {256, 512, D_VIT, D_VIT};
  const char* rn_names[4] = {"l1_rn", "l2_rn", "l3_rn", "l4_rn"};
  group(DPTX_GROUP_RN);
  for (int i = 0; i < 4; ++i) {
    // consumer of lrn[i] as a GEMM operand: refinenet4.resConfUnit2.conv1 (i = 3), refinenet{i+1}.resConfUnit1.conv1 (else)
    const std::string cons = pre + "scratch.refinenet" + std::to_string(i + 1) + (i == 3 ? ".resConfUnit2.conv1.weight" : ".resConfUnit1.conv1.weight");
    conv(rn_in[i], rn_h[i], rn_w[i], rn_c[i], pre + "scratch.layer" + std::to_string(i + 1) + "_rn.weight", 3, 1, 1, 1, rn_h[i],
         rn_w[i], FEAT, A(e->lrn[i]),
         GemmOpt().q(/*every consumer pre-activates*/ e->fp8_use(cons) ? 2 : 0).out_lo(lo_of(RLO(cons, DPTX_GROUP_FUSION))));
    tap((pre + rn_names[i]).c_str(), A(e->lrn[i]), rn_h[i], rn_w[i], FEAT);
  }

  // ---- RefineNet fusion 4 -> 1 (blocks.py:320-341).  out_conv (1x1) is applied BEFORE the x2
  // bilinear upsample: both are linear and the interpolation weights sum to 1, so
  // out_conv(up(x)) == up(out_conv(x)) exactly in real arithmetic, at a quarter of the MACs.
  group(DPTX_GROUP_FUSION);
  const void* path = nullptr;
  const char* p_names[4] = {"p1", "p2", "p3", "p4"};
  const std::string oc = pre + "scratch.output_conv.";
  for (int i = 4; i >= 1; --i) {
    const std::string p = pre + "scratch.refinenet" + std::to_string(i) + ".";
    const int h = rn_h[i - 1], w = rn_w[i - 1];
    const void* sum;
    if (i == 4) {
      sum = A(e->lrn[3]);
    } else {
      rcu(p + "resConfUnit1.", A(e->lrn[i - 1]), h, w, A(e->tA), A(e->tB),  // tB = path + RCU1(lrn)
          GemmOpt().R2(path).q(e->fp8_use(p + "resConfUnit2.conv1.weight") ? 2 : 0)
              .out_lo(lo_of(RLO(p + "resConfUnit2.conv1.weight", DPTX_GROUP_FUSION))));
      sum = A(e->tB);
    }
    rcu(p + "resConfUnit2.", sum, h, w, A(e->tA), A(e->tC),
        GemmOpt().q(e->fp8_use(p + "out_conv.weight") ? 1 : 0).out_lo(lo_of(RLO(p + "out_conv.weight", DPTX_GROUP_FUSION))));
    // the path tensor keeps a lo plane when out_conv computed one (it is added to the next stage's sum in fp32) and when
    // the first head conv multiplies it with 3 MFMAs.  A 2-MFMA head conv reads the hi plane only: path_1 is then interpolated
    // from both planes of the low-resolution tensor and rounded ONCE, into the hi plane
    conv(A(e->tC), h, w, FEAT, p + "out_conv.weight", 1, 1, 0, 0, h, w, FEAT, A(e->tA),
         GemmOpt().bias(e->f(p + "out_conv.bias"))
             .out_lo(lo_of(X3(p + "out_conv.weight", DPTX_GROUP_FUSION) || (i == 1 && X3(oc + "0.weight", DPTX_GROUP_HEAD)))));
    // path_1 feeds the first head conv: in the fp8 dtype the up-sampling also writes its e4m3 copy
    {
      const bool up8 = i == 1 && e->fp8_use(oc + "0.weight");
      const int slot = up8 ? q8_produce(A(e->P[0])) : -1;
      const bool hi_only = mx && i == 1 && has_lo(A(e->tA)) && !RLO(oc + "0.weight", DPTX_GROUP_HEAD);
      chk(launch_upsample2x(planes_mode(A(e->tA)), A(e->tA), A(e->P[i - 1]), B, h, w, FEAT, e->pl, st,
                            up8 ? e->q8(A(e->P[0])) : nullptr, up8 ? e->act_scale[slot] : 1.0f, hi_only),
          "fusion.up");
      if (up8) q8_measure(A(e->P[0]), (size_t)B * 4 * h * w * FEAT, 0, slot);
      if (mx) mark_lo(A(e->P[i - 1]), has_lo(A(e->tA)) && !hi_only);
    }
    path = A(e->P[i - 1]);
    tap((pre + p_names[i - 1]).c_str(), path, 2 * h, 2 * w, FEAT);
  }

  // ---- head (dpt_depth.py:91-99) ----------------------------------------------------------
  group(DPTX_GROUP_HEAD);
  const bool conv2_x3 = mx ? X3(oc + "2.weight", DPTX_GROUP_HEAD) : mode_is_x3(dt);
  conv(path, h2, w2, FEAT, oc + "0.weight", 3, 1, 1, 1, h2, w2, 128, A(e->H0), GemmOpt().bias(e->f(oc + "0.bias")).out_lo(lo_of(conv2_x3)));
  tap((pre + "h0").c_str(), A(e->H0), h2, w2, 128);
  // fp16-plane dtypes: did anything upstream leave the fp16 range?  (one pass over the hi plane of H0: every decoder path and,
  // through them, the ViT blocks reach it by residual adds; the ResNetV2 stages cannot overflow -- standardised weights and
  // a GroupNorm behind every convolution bound them whatever the checkpoint)
  if (e->range_check() && e->d_range)
    chk(launch_nonfinite_scan(mx ? MODE_FP16 : dt, A(e->H0), (size_t)B * h2 * w2 * 128, e->d_range, st), "range.scan");
  // (a 2-MFMA second head conv -- dptx_set_layer_precision(..., 2) -- has no fused form: head_tail_x3_kernel always spends three
  //  MFMAs and reads H0's lo plane, so the fused and the tapped forward would differ; it takes the three-launch tail.  ADVICE r4)
  const bool conv2_two = mx && e->layer_mfmas(oc + "2.weight", DPTX_GROUP_HEAD) == 2;
  if (e->head_fused(conv2_x3) && !conv2_two) {
    // x2 upsample + conv 128->32 + ReLU + conv 1x1 + ReLU in one launch (head.hip): the 37.7 MB/image up-sampled map
    // and the 32-channel map never reach memory.  Not with a 3-MFMA conv2, and not while stage taps are recorded ("h1").
    chk(launch_head_tail(conv2_x3 ? MODE_FP16X3 : (mx ? MODE_FP16 : dt), A(e->H0), e->w(oc + "2.weight"), e->f(oc + "2.bias"),
                         e->f(oc + "4.weight"), e->f(oc + "4.bias"), yout, io, B, h2, w2, ch, e->cfg.non_negative, st, e->pl),
        "head.tail", 0);
    exec_macs += (double)Hi * Wi * 32 * 1152;
    cat_macs[0] += (double)Hi * Wi * 32 * (1152 + ch);
  } else {
    chk(launch_upsample2x(planes_mode(A(e->H0)), A(e->H0), A(e->H0U), B, h2, w2, 128, e->pl, st), "head.up");
    if (mx) mark_lo(A(e->H0U), has_lo(A(e->H0)));
    conv(A(e->H0U), Hi, Wi, 128, oc + "2.weight", 3, 1, 1, 1, Hi, Wi, 32, A(e->H1),
         GemmOpt().bias(e->f(oc + "2.bias")).act(1).out_lo(lo_of(conv2_x3)));
    tap((pre + "h1").c_str(), A(e->H1), Hi, Wi, 32);
    chk(launch_head_out(planes_mode(A(e->H1)), A(e->H1), e->f(oc + "4.weight"), e->f(oc + "4.bias"), yout, io, B, Hi * Wi, ch,
                        e->cfg.non_negative, e->pl, st),
        "head.out");
  }
  exec_macs += (double)Hi * Wi * 32 * ch;
}

}  // namespace

// =================================================================================== C ABI
extern "C" {

#ifndef DPTX_SRC_HASH
#define DPTX_SRC_HASH "unknown"
#endif
#define DPTX_BUILD_KIND ""
// "src=<hash>": sha256 of the sources this binary was built from (omnidata_amd/build.py source_hash); the Python loader
// compares it with the sources next to the .so and refuses a stale binary
const char* dptx_version(void) { return "dptx 0.3.0 (gfx950) src=" DPTX_SRC_HASH; }

void dptx_default_config(dptx_config* cfg) {
  memset(cfg, 0, sizeof *cfg);
  cfg->num_channels = 3;
  cfg->max_batch = 32;
  cfg->dtype = DPTX_DTYPE_MIXED;  // the mode that matches the reference's fp32 forward within 1e-3; BF16 is the throughput mode
  cfg->device_id = 0;
  cfg->non_negative = 1;
  cfg->ws_form = 0;
  cfg->ws_eps = 1e-8f;
}

int dptx_create(dptx_handle* out, const dptx_config* cfg) {
  if (!out || !cfg) return DPTX_E_INVALID;
  *out = nullptr;
  // max_batch <= 48: the largest activation (up-sampled head input, 37.7 MB/image) must stay below the 2 GB that a
  // 32-bit buffer offset of the direct-to-LDS loads can address; callers chunk larger batches (model.py does).
  const int max_h = cfg->max_height ? cfg->max_height : IMG, max_w = cfg->max_width ? cfg->max_width : IMG;
  if (max_h < 64 || max_w < 64 || max_h % 32 != 0 || max_w % 32 != 0 || max_h > 4096 || max_w > 4096) return DPTX_E_INVALID;
  if ((long long)cfg->max_batch * max_h * max_w * 256 >= (1ll << 31)) return DPTX_E_INVALID;  // = max_batch <= 56 at 384x384
  if (cfg->streams < 0 || cfg->streams > 4) return DPTX_E_INVALID;
  if (cfg->backbone != DPTX_BACKBONE_VITB_RN50_384 && cfg->backbone != DPTX_BACKBONE_VITL16_384) return DPTX_E_INVALID;
  // (the attention kernel's 32-bit LDS-DMA offsets over its qkv rows [B * S][3 * width] need B * S * 3 * width * 2 < 2^31: with
  //  S = h * w / 256 + 1 and width <= 1024 that is implied by the activation bound above for both backbones, so there is no
  //  separate check here; attention.hip launch_attention keeps the backstop.  ADVICE r5)
  if (cfg->backbone == DPTX_BACKBONE_VITL16_384 && cfg->dual_task) return DPTX_E_INVALID;  // the dual-task model is the hybrid
  if ((cfg->dual_task != 0 && (cfg->dual_task != 1 || cfg->num_channels != 3)) ||
      (cfg->num_channels != 1 && cfg->num_channels != 3) || cfg->max_batch < 1 || cfg->max_batch > 48 ||
      cfg->dtype < DPTX_DTYPE_BF16 || cfg->dtype > DPTX_DTYPE_FP8 || (cfg->ws_form != 0 && cfg->ws_form != 1) ||
      (cfg->flags & ~(DPTX_FLAG_NO_LN_FOLD | DPTX_FLAG_GROUP_POLICY | DPTX_FLAG_FP32_STREAM | DPTX_FLAG_NO_RANGE_CHECK | DPTX_FLAG_FP8_ALL |
                      DPTX_FLAG_FP8_VIT)) ||
      cfg->reserved != 0)
    return DPTX_E_INVALID;
  int x3_groups = 0;
  if (cfg->dtype == DPTX_DTYPE_MIXED) {
    x3_groups = cfg->x3_groups ? cfg->x3_groups : (DPTX_GROUP_ALL & ~DPTX_GROUP_VIT);
    if (x3_groups & ~DPTX_GROUP_ALL) return DPTX_E_INVALID;
    if (cfg->backbone == DPTX_BACKBONE_VITL16_384) x3_groups |= DPTX_GROUP_RESNET;  // no such layers: nothing depends on them
    // a 3-MFMA group reads the lo planes of its inputs: every producer of those must be a 3-MFMA group as well
    auto needs = [&](int g, int producers) { return !(x3_groups & g) || (x3_groups & producers) == producers; };
    if (!needs(DPTX_GROUP_EMBED, DPTX_GROUP_RESNET) || !needs(DPTX_GROUP_RN, DPTX_GROUP_RESNET | DPTX_GROUP_REASSEMBLE) ||
        !needs(DPTX_GROUP_FUSION, DPTX_GROUP_RN) || !needs(DPTX_GROUP_HEAD, DPTX_GROUP_FUSION))
      return DPTX_E_INVALID;
  }
  dptx_engine* e = new (std::nothrow) dptx_engine();
  if (!e) return DPTX_E_ALLOC;
  e->cfg = *cfg;
  e->cfg.x3_groups = x3_groups;
  e->backbone = cfg->backbone;
  if (e->backbone == DPTX_BACKBONE_VITL16_384) { e->dv = 1024; e->dm = 4096; e->nh = 16; e->depth = 24; }
  e->max_h = max_h;
  e->fp8_all = (cfg->flags & DPTX_FLAG_FP8_ALL) != 0;
  e->fp8_vit = (cfg->flags & DPTX_FLAG_FP8_VIT) != 0;
  if (cfg->dtype == DPTX_DTYPE_MIXED && cfg->x3_groups == 0 && !(cfg->flags & DPTX_FLAG_GROUP_POLICY)) {
    // default per-layer table of the decoder (oracle/precision_layers.py: per-layer sensitivities on both synthetic weight
    // families; "policy A" of profiles/r03_precision_layers.md): these nine 3x3 convolutions -- 30.6 of the decoder's 57.7
    // GMAC -- run one MFMA per product, because their operand rounding moves the output 10x less per MAC than the 1x1
    // out_convs, the deep (low-resolution) fusion stages and the head do
    for (const char* k : {"scratch.layer1_rn.weight",
                          "scratch.refinenet1.resConfUnit1.conv1.weight", "scratch.refinenet1.resConfUnit1.conv2.weight",
                          "scratch.refinenet1.resConfUnit2.conv1.weight", "scratch.refinenet1.resConfUnit2.conv2.weight",
                          "scratch.refinenet2.resConfUnit1.conv1.weight", "scratch.refinenet2.resConfUnit1.conv2.weight",
                          "scratch.refinenet3.resConfUnit1.conv1.weight", "scratch.refinenet3.resConfUnit1.conv2.weight"})
      e->layer_prec[k] = 1;
    // round 4, NOT in the default table: the first head convolution (10.9 of the head's 16.3 GMAC, 2.2 of the 19.5 ms) on TWO MFMAs
    // (dptx_set_layer_precision(h, "scratch.output_conv.0.weight", 2): the weights keep their lo plane, the input is rounded
    // once) is +3.9 % (1636 -> 1700 img/s) for rms 1.07e-4 -> 1.19e-4; the worst of the 14.2 M outputs of a B = 32 batch moves
    // from 6.3e-4 to 7.6e-4 -- inside north_star's 1e-3, but with 1.3x instead of 1.6x margin (profiles/r04_experiments.md).
  }
  {
    // fused schedules (include/dptx.h DPTX_FLAG_*)
    e->ln_fold = !(cfg->flags & DPTX_FLAG_NO_LN_FOLD) && !mode_is_x3(e->mode_of(DPTX_GROUP_VIT));
    e->stream16 = e->ln_fold && !(cfg->flags & DPTX_FLAG_FP32_STREAM) &&
                  (cfg->dtype == DPTX_DTYPE_BF16 || cfg->dtype == DPTX_DTYPE_FP16 || cfg->dtype == DPTX_DTYPE_FP8);
  }
  {
    const char* t = getenv("DPTX_STREAMS");  // experiments: overrides cfg.streams
    const int ns = t ? atoi(t) : cfg->streams;
    e->n_streams = ns == 0 ? 2 : (ns < 1 ? 1 : (ns > dptx_engine::MAX_STREAMS ? dptx_engine::MAX_STREAMS : ns));
    e->auto_streams = ns == 0;
  }
  e->max_w = max_w;
  e->tok_tap_stride = (size_t)cfg->max_batch * ((size_t)max_h * max_w / 256 + 1) * (size_t)e->dv;
  e->spec = build_spec(cfg->num_channels, cfg->dual_task != 0, e->backbone);
  size_t off = BLOB_HEADER;  // the blob's layout tag (BlobHeader)
  for (size_t i = 0; i < e->spec.size(); ++i) {
    e->spec_index[e->spec[i].key] = i;
    const size_t b = packed_entry_bytes(e->spec[i]);
    if (b) {
      e->packed_off[e->spec[i].key] = off;
      off += align_up(b, 256);
    }
  }
  e->packed_single = off;
  e->packed_bytes = off * (e->two_planes() ? 2 : 1);
  e->pl.w = e->two_planes() ? (long long)(off / 2) : 0;
  plan_arena(e);
  if (cfg->device_id >= 0) {
    int n = 0;
    hipError_t r = hipGetDeviceCount(&n);
    if (r != hipSuccess || cfg->device_id >= n) {
      delete e;
      return DPTX_E_NODEVICE;
    }
  }
  *out = e;
  return DPTX_OK;
}

void dptx_destroy(dptx_handle h) {
  if (!h) return;
  if (h->cfg.device_id >= 0) {
    DeviceGuard guard(h->cfg.device_id);
    h->blob_hold.reset();   // frees the packed blob if this was its last user (hipFree in the deleter)
    if (h->d_arena) (void)hipFree(h->d_arena);
    if (h->d_tok_taps) (void)hipFree(h->d_tok_taps);
    if (h->d_amax) (void)hipFree(h->d_amax);
    if (h->d_range) (void)hipFree(h->d_range);
    for (auto ev : h->events) (void)hipEventDestroy(ev);
    for (int r = 0; r < dptx_engine::MAX_STREAMS; ++r) {
      if (h->sub_stream[r]) (void)hipStreamDestroy(h->sub_stream[r]);
      if (h->ev_join[r]) (void)hipEventDestroy(h->ev_join[r]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  }
  delete h;
}

const char* dptx_last_error(dptx_handle h) { return h ? h->err.c_str() : "null handle"; }

int dptx_load_tensor(dptx_handle h, const char* ref_key, const float* host_fp32, const int64_t* shape, int32_t ndim) {
  if (!h || !ref_key || !host_fp32 || !shape || ndim < 1) return DPTX_E_INVALID;
  auto it = h->spec_index.find(ref_key);
  if (it == h->spec_index.end()) return h->fail(DPTX_E_KEY, std::string("unexpected key: ") + ref_key);
  const Spec& s = h->spec[it->second];
  bool ok = (size_t)ndim == s.shape.size();
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == s.shape[i];
  if (!ok) return h->fail(DPTX_E_KEY, std::string("shape mismatch for ") + ref_key);
  if (s.role == R_UNUSED) return DPTX_OK;
  h->staged[s.key].assign(host_fp32, host_fp32 + numel(s.shape));
  h->finalized = false;
  h->device_ready = false;
  return DPTX_OK;
}

static int ensure_sub_streams(dptx_handle h);
// own_blob: the caller is about to WRITE the blob (finalize / import): a handle that shares another's gets one of its own first
static int ensure_device_memory(dptx_handle h, bool own_blob = true) {
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  // a handle about to WRITE a blob that others read too (it shares somebody's, or somebody shares its own) takes a fresh one
  if (own_blob && h->d_blob && (h->blob_shared || h->blob_hold.use_count() > 1)) {
    h->blob_hold.reset();
    h->d_blob = nullptr;
    h->blob_shared = false;
    h->device_ready = false;
  }
  if (!h->d_blob && own_blob) {
    void* p = nullptr;
    HIPCHK(h, hipMalloc(&p, h->packed_bytes));
    const int dev = h->cfg.device_id;
    h->blob_hold = std::shared_ptr<void>(p, [dev](void* q) {
      DeviceGuard g(dev);
      (void)hipFree(q);
    });
    h->d_blob = (char*)p;
  }
  if (!h->d_arena) HIPCHK(h, hipMalloc((void**)&h->d_arena, h->arena_bytes));
  if (!h->d_range) {
    HIPCHK(h, hipMalloc((void**)&h->d_range, 256));
    HIPCHK(h, hipMemset(h->d_range, 0, 256));
  }
  return ensure_sub_streams(h);
}

int dptx_finalize_weights(dptx_handle h) {
  if (!h) return DPTX_E_INVALID;
  int r = pack_host(h);
  if (r != DPTX_OK) return r;
  if (h->cfg.device_id < 0) return DPTX_OK;
  r = ensure_device_memory(h);
  if (r != DPTX_OK) return r;
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipMemcpy(h->d_blob, h->host_blob.data(), h->packed_bytes, hipMemcpyHostToDevice));
  h->device_ready = true;
  h->staged.clear();  // fp32 staging copies are no longer needed
  return DPTX_OK;
}

size_t dptx_packed_bytes(dptx_handle h) { return h ? h->packed_bytes : 0; }

int dptx_export_packed_host(dptx_handle h, void* dst_host, size_t bytes) {
  if (!h || !dst_host) return DPTX_E_INVALID;
  if (!h->finalized) return h->fail(DPTX_E_INVALID, "export before dptx_finalize_weights");
  if (bytes < h->packed_bytes) return h->fail(DPTX_E_INVALID, "export buffer too small");
  memcpy(dst_host, h->host_blob.data(), h->packed_bytes);
  return DPTX_OK;
}

int dptx_export_packed_device(dptx_handle h, void* dst_dev, size_t bytes, void* stream) {
  if (!h || !dst_dev) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  if (!h->device_ready) return h->fail(DPTX_E_INVALID, "export before weights are on the device");
  if (bytes < h->packed_bytes) return h->fail(DPTX_E_INVALID, "export buffer too small");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipMemcpyAsync(dst_dev, h->d_blob, h->packed_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DPTX_OK;
}

int dptx_import_packed_device(dptx_handle h, const void* src_dev, size_t bytes, void* stream) {
  if (!h || !src_dev) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  if (bytes != h->packed_bytes) return h->fail(DPTX_E_INVALID, "packed blob size mismatch (different config/build?)");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  {
    // the blob's layout tag must be the one this handle packs itself (dtype, backbone, LayerNorm fold, weight-std form ...).
    // Checked BEFORE the handle's state is touched: a rejected import leaves a working handle -- its own blob,
    // or the one it shares -- exactly as it was
    BlobHeader got;
    HIPCHK(h, hipMemcpyAsync(&got, src_dev, sizeof got, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    const BlobHeader want = h->blob_header();
    if (memcmp(&got, &want, sizeof got) != 0) {
      char msg[320];
      snprintf(msg, sizeof msg,
               "packed blob was packed for another layout: magic %.8s version %u dtype %d backbone %d dual %d channels %d ln_fold %d "
               "ws_form %d (this handle: version %u dtype %d backbone %d dual %d channels %d ln_fold %d ws_form %d)",
               got.magic, got.version, got.dtype, got.backbone, got.dual_task, got.num_channels, got.ln_fold, got.ws_form,
               want.version, want.dtype, want.backbone, want.dual_task, want.num_channels, want.ln_fold, want.ws_form);
      return h->fail(DPTX_E_INVALID, msg);
    }
  }
  const int r = ensure_device_memory(h);   // un-shares / allocates: only now that the source is known to be importable
  if (r != DPTX_OK) return r;
  HIPCHK(h, hipMemcpyAsync(h->d_blob, src_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  h->device_ready = true;
  return DPTX_OK;
}

int dptx_share_packed(dptx_handle dst, dptx_handle src) {
  if (!dst || !src || dst == src) return DPTX_E_INVALID;
  if (dst->cfg.device_id < 0 || src->cfg.device_id < 0) return dst->fail(DPTX_E_NODEVICE, "host-only handle");
  if (dst->cfg.device_id != src->cfg.device_id) return dst->fail(DPTX_E_INVALID, "dptx_share_packed: the handles live on different devices");
  if (!src->device_ready || !src->d_blob) return dst->fail(DPTX_E_INVALID, "dptx_share_packed: the source handle has no weights on the device");
  const BlobHeader a = dst->blob_header(), b = src->blob_header();
  if (dst->packed_bytes != src->packed_bytes || memcmp(&a, &b, sizeof a) != 0)
    return dst->fail(DPTX_E_INVALID, "dptx_share_packed: the handles pack different blobs (dtype / backbone / channels / dual task / fold)");
  DeviceGuard guard(dst->cfg.device_id);
  HIPCHK(dst, guard.err);
  dst->blob_hold = src->blob_hold;   // (a blob of dst's own is released here if nobody else holds it)
  dst->d_blob = src->d_blob;
  dst->blob_shared = true;
  const int r = ensure_device_memory(dst, false);   // arena + range flag
  if (r != DPTX_OK) return r;
  dst->device_ready = true;
  return DPTX_OK;
}

size_t dptx_workspace_bytes(dptx_handle h) { return h ? h->packed_bytes + h->arena_bytes : 0; }

int dptx_enable_taps(dptx_handle h, int on) {
  if (!h) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  if (on && !h->d_tok_taps) {
    DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
    HIPCHK(h, hipMalloc((void**)&h->d_tok_taps, (size_t)(h->depth + 1) * h->tok_tap_stride * 4));
  }
  h->taps_on = on != 0;
  return DPTX_OK;
}

// Runs one forward: either one Run over the whole batch on the caller's stream, or -- two streams, no taps, no per-launch
// timing, batch >= 2 -- two Runs over the two halves of the batch on the handle's two internal streams, forked from and
// joined to the caller's stream with events.  Images are independent and every kernel is batch-invariant bit for bit, so
// both schedules return the same bits; the second one lets the MFMA-bound launches of one half overlap the HBM-bound
// launches and the tails of the other.
// The internal streams of the sub-batch schedule.  Created when the handle gets its device memory (round 5), not at the first
// forward: HIP maps streams onto hardware queues as they are created, and a handle whose streams came into being AFTER a
// process had created many others (torch's stream pool) was measured with its two half-batch runs no longer overlapping --
// 1990 instead of 2600 images/s (profiles/r05_experiments.md).
static int ensure_sub_streams(dptx_handle h) {
  if (h->ev_fork || h->n_streams < 2) return DPTX_OK;
  // One stream PRIORITY per sub-batch stream, cycling through the device's range: the runtime keeps a separate pool of
  // hardware queues per priority, so streams of different priorities can never be mapped onto the same queue -- which is what
  // happens to same-priority streams once a process holds more streams than queues (GPU_MAX_HW_QUEUES, 4), and then the two
  // half-batch runs execute one after the other (1974 instead of 2600 images/s, lease r5l4).  The priorities only order the
  // dispatch of ready work between the halves; both halves are needed before the forward is complete.
  int pri_least = 0, pri_greatest = 0;
  HIPCHK(h, hipDeviceGetStreamPriorityRange(&pri_least, &pri_greatest));   // numerically: least >= greatest
  const int levels = pri_least - pri_greatest + 1;
  for (int r = 0; r < h->n_streams && r < dptx_engine::MAX_STREAMS; ++r) {
    const int pri = levels > 1 ? pri_least - (r % levels) : pri_least;
    HIPCHK(h, hipStreamCreateWithPriority(&h->sub_stream[r], hipStreamNonBlocking, pri));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_join[r], hipEventDisableTiming));
  }
  HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  return DPTX_OK;
}

static int run_forward(dptx_handle h, const void* x, int io, void* y, void* y2, int batch, int height, int width,
                       hipStream_t stream) {
  const int C = h->cfg.num_channels;
  const size_t esz = io == DPTX_IO_FP32 ? 4 : 2;  // bytes per element of the caller's buffers
  const bool want_split = h->force_schedule >= 0 ? h->force_schedule == 1 : (!h->auto_streams || (h->split_tuned && h->split_on));
  const bool split = want_split && h->n_streams >= 2 && batch >= 2 && !h->taps_on && !h->profiling && !h->calibrating;
  // tile selection of the GEMMs (kernels.h gemm_set_cu_share): a sub-batch run shares the chip with the other streams' runs.
  // Measured (profiles/r03_experiments.md, two streams): the 256x256 rule judged against 1 / streams of the chip (the
  // half-batch qkv, proj and fc2 GEMMs then take the ping-pong kernel) -- with the lockstep-epilogue kernel of the first half
  // of round 3 0.7 was the optimum (+1.2 %) and 0.5 lost; with the persistent, register-direct form 0.5 wins on boxes that
  // are not power-bound (+1.3 ... 2.9 % together with the 1.5 x per-tile advantage in launch_dt) and is neutral on those
  // that are.  Scaled narrow-tile thresholds lose.
  // whatever path leaves this function (HIPCHK returns included), the thread's tile-selection state is back at "whole chip"
  struct ShareReset { ~ShareReset() { gemm_set_cu_share(1.0f); } } share_reset;
  if (!split) {
    // (a whole-batch run that shares the GPU with another handle's forward -- omnidata_amd/pipeline.py -- is tiled for the
    // whole chip too: scaling it was measured neutral, profiles/r05_experiments.md)
    gemm_set_cu_share(1.0f);
    Run run{h, batch, stream, h->cfg.dtype, height, width, io};
    const int rc = run.forward(x, y, y2);
    h->launches = run.launches;
    h->exec_macs = run.exec_macs;
    for (int c = 0; c < 4; ++c) h->cat_macs[c] = run.cat_macs[c];
    h->last_batch = batch;
    h->last_regions = 1;
    return rc;
  }
  const int nr = batch < h->n_streams ? batch : h->n_streams;  // sub-batches: the first (batch % nr) get one image more
  gemm_set_cu_share(1.0f / (float)nr);
  {
    const int rs = ensure_sub_streams(h);
    if (rs != DPTX_OK) return rs;
  }
  HIPCHK(h, hipEventRecord(h->ev_fork, stream));
  const size_t px = (size_t)height * width;
  int rc = DPTX_OK;
  int64_t launches = 0;
  size_t first = 0;
  for (int r = 0; r < nr; ++r) {
    const int nb = batch / nr + (r < batch % nr ? 1 : 0);
    HIPCHK(h, hipStreamWaitEvent(h->sub_stream[r], h->ev_fork, 0));
    Run run{h, nb, h->sub_stream[r], h->cfg.dtype, height, width, io};
    run.abase = (size_t)r * h->half_region;
    run.half = true;
    const int rr = run.forward((const char*)x + first * 3 * px * esz, (char*)y + first * C * px * esz,
                               y2 ? (char*)y2 + first * px * esz : nullptr);
    if (rc == DPTX_OK) rc = rr;
    launches += run.launches;
    if (r == 0) {
      h->exec_macs = run.exec_macs;
      for (int c = 0; c < 4; ++c) h->cat_macs[c] = run.cat_macs[c];
    }
    HIPCHK(h, hipEventRecord(h->ev_join[r], h->sub_stream[r]));
    HIPCHK(h, hipStreamWaitEvent(stream, h->ev_join[r], 0));
    first += (size_t)nb;
  }
  gemm_set_cu_share(1.0f);
  h->taps.clear();  // stage taps describe whole-batch runs only (dptx_enable_taps makes the forward single-pass)
  h->launches = launches;
  h->last_batch = batch;
  h->last_regions = nr;
  return rc;
}

int dptx_forward(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev, int32_t batch, void* stream) {
  return dptx_forward_hw(h, x_dev, x_dtype, y_dev, batch, IMG, IMG, stream);
}

// The argument checks of the two forward entry points; `fn` names the caller in the messages, `dual` says which kind of
// handle it serves
static int check_forward_args(dptx_handle h, const char* fn, bool dual, int32_t x_dtype, int32_t batch, int32_t height, int32_t width) {
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, std::string(fn) + " on a host-only handle");
  if (dual != (h->cfg.dual_task != 0))
    return h->fail(DPTX_E_INVALID, dual ? "dptx_forward_dual needs a handle created with dual_task = 1" : "dual-task handle: call dptx_forward_dual");
  if (!h->device_ready) return h->fail(DPTX_E_INVALID, std::string(fn) + " before weights were finalized/imported");
  if (batch < 1 || batch > h->cfg.max_batch) return h->fail(DPTX_E_INVALID, "batch out of range [1, max_batch]");
  if (x_dtype != DPTX_IO_FP32 && x_dtype != DPTX_IO_BF16 && x_dtype != DPTX_IO_FP16)
    return h->fail(DPTX_E_INVALID, "unsupported x_dtype (DPTX_IO_FP32 / DPTX_IO_BF16 / DPTX_IO_FP16)");
  if (height < 64 || width < 64 || height % 32 != 0 || width % 32 != 0)
    return h->fail(DPTX_E_INVALID, "input height/width must be multiples of 32, >= 64");
  if ((long long)height * width > (long long)h->max_h * h->max_w)
    return h->fail(DPTX_E_INVALID, "input larger than the engine was planned for (dptx_config.max_height/max_width)");
  return DPTX_OK;
}

int dptx_forward_hw(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev, int32_t batch, int32_t height,
                    int32_t width, void* stream) {
  if (!h || !x_dev || !y_dev) return DPTX_E_INVALID;
  const int rc = check_forward_args(h, "dptx_forward", false, x_dtype, batch, height, width);
  if (rc != DPTX_OK) return rc;
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  return run_forward(h, x_dev, x_dtype, y_dev, nullptr, batch, height, width, (hipStream_t)stream);
}

int dptx_forward_dual(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_normal_dev, void* y_depth_dev, int32_t batch,
                      int32_t height, int32_t width, void* stream) {
  if (!h || !x_dev || !y_normal_dev || !y_depth_dev) return DPTX_E_INVALID;
  const int rc = check_forward_args(h, "dptx_forward_dual", true, x_dtype, batch, height, width);
  if (rc != DPTX_OK) return rc;
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  return run_forward(h, x_dev, x_dtype, y_normal_dev, y_depth_dev, batch, height, width, (hipStream_t)stream);
}

int dptx_tune_schedule(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev, void* y_depth_dev, int32_t batch,
                       int32_t height, int32_t width, int32_t reps, void* stream) {
  if (!h || !x_dev || !y_dev) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "dptx_tune_schedule on a host-only handle");
  if (!h->device_ready) return h->fail(DPTX_E_INVALID, "dptx_tune_schedule before weights were finalized/imported");
  if ((h->cfg.dual_task != 0) != (y_depth_dev != nullptr)) return h->fail(DPTX_E_INVALID, "dptx_tune_schedule: y_depth_dev is for dual-task handles");
  if (!h->auto_streams || h->n_streams < 2 || batch < 2) return DPTX_OK;   // nothing to choose
  if (reps < 1) reps = 2;
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(h, hipEventCreate(&e0));
  HIPCHK(h, hipEventCreate(&e1));
  struct Cleanup { dptx_handle h; hipEvent_t a, b; ~Cleanup() { h->force_schedule = -1; (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } cleanup{h, e0, e1};
  float ms[2] = {0.f, 0.f};
  auto fwd = [&]() {
    return h->cfg.dual_task ? dptx_forward_dual(h, x_dev, x_dtype, y_dev, y_depth_dev, batch, height, width, stream)
                            : dptx_forward_hw(h, x_dev, x_dtype, y_dev, batch, height, width, stream);
  };
  for (int cand = 0; cand < 2; ++cand) {
    h->force_schedule = cand;
    int rc = fwd();   // untimed: first-use costs (kernel attributes, stream wake-up)
    if (rc != DPTX_OK) return rc;
    HIPCHK(h, hipEventRecord(e0, (hipStream_t)stream));
    for (int r = 0; r < reps; ++r) {
      rc = fwd();
      if (rc != DPTX_OK) return rc;
    }
    HIPCHK(h, hipEventRecord(e1, (hipStream_t)stream));
    HIPCHK(h, hipEventSynchronize(e1));
    HIPCHK(h, hipEventElapsedTime(&ms[cand], e0, e1));
    ms[cand] /= (float)reps;
  }
  h->tune_ms_single = ms[0];
  h->tune_ms_split = ms[1];
  h->split_on = ms[1] < 0.97f * ms[0];   // the two-stream schedule has to EARN its place: ties go to the simpler one
  h->split_tuned = true;
  return DPTX_OK;
}

int dptx_schedule_info(dptx_handle h, int32_t* split, int32_t* tuned, float* ms_single, float* ms_split) {
  if (!h) return DPTX_E_INVALID;
  if (split) *split = h->auto_streams ? (int32_t)(h->split_tuned && h->split_on) : (int32_t)(h->n_streams >= 2);
  if (tuned) *tuned = (int32_t)(h->auto_streams && h->split_tuned);
  if (ms_single) *ms_single = h->tune_ms_single;
  if (ms_split) *ms_split = h->tune_ms_split;
  return DPTX_OK;
}

int dptx_probe_stream_overlap(int32_t device_id, void* stream_a, void* stream_b, int32_t spin_us, float* ratio) {
  if (!ratio || device_id < 0) return DPTX_E_INVALID;
  DeviceGuard guard(device_id);
  if (guard.err != hipSuccess) return DPTX_E_HIP;
  hipStream_t a = (hipStream_t)stream_a, b = (hipStream_t)stream_b;
  const long long ticks = (long long)(spin_us > 0 ? spin_us : 2000) * 100;   // s_memrealtime: 100 MHz
  auto run = [&](bool both, double& sec) -> bool {
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return false;
    const auto t0 = std::chrono::steady_clock::now();
    if (launch_spin(ticks, a) != hipSuccess) return false;
    if (both && launch_spin(ticks, b) != hipSuccess) return false;
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return false;
    sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return true;
  };
  double warm = 0, alone = 0, pair = 0;
  if (!run(true, warm) || !run(false, alone) || !run(true, pair) || alone <= 0) return DPTX_E_HIP;
  *ratio = (float)(pair / alone);
  return DPTX_OK;
}

int dptx_set_layer_precision(dptx_handle h, const char* conv_weight_key, int32_t mfmas) {
  if (!h || !conv_weight_key || mfmas < 1 || mfmas > 3) return DPTX_E_INVALID;
  if (!h->mixed()) return h->fail(DPTX_E_INVALID, "per-layer precision applies to dtype = DPTX_DTYPE_MIXED");
  std::string k = conv_weight_key;
  if (k.compare(0, 6, "depth.") == 0) k = k.substr(6);
  const bool decoder = k.compare(0, 8, "scratch.") == 0 && k.size() > 7 && k.compare(k.size() - 7, 7, ".weight") == 0 &&
                       k.find("output_conv.4") == std::string::npos && h->spec_index.count(k) && h->spec[h->spec_index[k]].role == R_CONV;
  if (!decoder) return h->fail(DPTX_E_KEY, std::string("not a decoder convolution (scratch.*): ") + conv_weight_key);
  h->layer_prec[k] = mfmas;
  return DPTX_OK;
}

int dptx_calibrate_fp8(dptx_handle h, const void* x_dev, int32_t x_dtype, void* y_dev, void* y2_dev, int32_t batch, int32_t height,
                       int32_t width, void* stream) {
  if (!h || !x_dev || !y_dev) return DPTX_E_INVALID;
  if (!h->fp8()) return h->fail(DPTX_E_INVALID, "dptx_calibrate_fp8 needs a handle created with dtype = DPTX_DTYPE_FP8");
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "dptx_calibrate_fp8 on a host-only handle");
  if (!h->device_ready) return h->fail(DPTX_E_INVALID, "dptx_calibrate_fp8 before weights were finalized/imported");
  if (batch < 1 || batch > h->cfg.max_batch) return h->fail(DPTX_E_INVALID, "batch out of range [1, max_batch]");
  if (x_dtype != DPTX_IO_FP32 && x_dtype != DPTX_IO_BF16 && x_dtype != DPTX_IO_FP16) return h->fail(DPTX_E_INVALID, "unsupported x_dtype");
  if (height < 64 || width < 64 || height % 32 != 0 || width % 32 != 0 || (long long)height * width > (long long)h->max_h * h->max_w)
    return h->fail(DPTX_E_INVALID, "input height/width must be multiples of 32, >= 64, within the planned size");
  if ((h->cfg.dual_task != 0) != (y2_dev != nullptr)) return h->fail(DPTX_E_INVALID, "y2_dev: the depth output of a dual-task handle");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  hipStream_t st = (hipStream_t)stream;
  if (!h->d_amax) HIPCHK(h, hipMalloc((void**)&h->d_amax, dptx_engine::MAX_Q8 * sizeof(unsigned)));
  HIPCHK(h, hipMemsetAsync(h->d_amax, 0, dptx_engine::MAX_Q8 * sizeof(unsigned), st));
  h->calibrating = true;
  const int rc = run_forward(h, x_dev, x_dtype, y_dev, y2_dev, batch, height, width, st);
  h->calibrating = false;
  if (rc != DPTX_OK) return rc;
  unsigned bits[dptx_engine::MAX_Q8];
  HIPCHK(h, hipMemcpyAsync(bits, h->d_amax, sizeof bits, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  for (int i = 0; i < dptx_engine::MAX_Q8; ++i) {
    float a;
    memcpy(&a, &bits[i], 4);
    h->act_amax[i] = a;
    // power of two that puts the calibration maximum into (112, 224]: one binade of headroom below e4m3's 448
    int k = (a > 0.f && std::isfinite(a)) ? (int)std::floor(std::log2(224.0 / (double)a)) : 0;
    k = k < -24 ? -24 : (k > 24 ? 24 : k);
    h->act_scale[i] = std::ldexp(1.0f, k);
  }
  h->calibrated = true;
  return DPTX_OK;
}

int dptx_fp8_get_calibration(dptx_handle h, float* scales, float* amax, int32_t capacity) {
  if (!h) return DPTX_E_INVALID;
  if (!h->fp8()) return h->fail(DPTX_E_INVALID, "not an fp8 handle");
  const int n = h->n_q8;
  if (capacity < n) return h->fail(DPTX_E_INVALID, "capacity < number of e4m3 tensors of the last forward");
  for (int i = 0; i < n; ++i) {
    if (scales) scales[i] = h->act_scale[i];
    if (amax) amax[i] = h->act_amax[i];
  }
  return n;
}

int dptx_fp8_set_calibration(dptx_handle h, const float* scales, int32_t n) {
  if (!h || !scales || n < 0 || n > dptx_engine::MAX_Q8) return DPTX_E_INVALID;
  if (!h->fp8()) return h->fail(DPTX_E_INVALID, "not an fp8 handle");
  for (int i = 0; i < n; ++i) {
    int e2 = 0;
    const float m = std::frexp(scales[i], &e2);
    if (!(scales[i] > 0.f) || m != 0.5f) return h->fail(DPTX_E_INVALID, "activation scales must be positive powers of two");
    h->act_scale[i] = scales[i];
  }
  h->calibrated = true;
  return DPTX_OK;
}

int dptx_range_status(dptx_handle h, int32_t* nonfinite, int32_t reset, void* stream) {
  if (!h || !nonfinite) return DPTX_E_INVALID;
  *nonfinite = 0;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  if (!h->range_check() || !h->d_range) return DPTX_OK;  // bf16-plane dtypes have fp32's range: nothing to report
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  unsigned v = 0;
  HIPCHK(h, hipMemcpyAsync(&v, h->d_range, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
  if (reset) HIPCHK(h, hipMemsetAsync(h->d_range, 0, sizeof v, (hipStream_t)stream));
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  *nonfinite = v != 0;
  return DPTX_OK;
}

int dptx_tap(dptx_handle h, const char* name, float* dst_host, size_t capacity_floats, int64_t shape4[4]) {
  if (!h || !name || !dst_host || !shape4) return DPTX_E_INVALID;
  auto it = h->taps.find(name);
  if (it == h->taps.end()) return h->fail(DPTX_E_KEY, std::string("unknown or unavailable tap: ") + name);
  const TapInfo& t = it->second;
  size_t n = 1;
  for (int i = 0; i < 4; ++i) { shape4[i] = t.shape[i]; n *= (size_t)t.shape[i]; }
  if (capacity_floats < n) return h->fail(DPTX_E_INVALID, "tap buffer too small");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipDeviceSynchronize());
  if (t.fp32) {
    HIPCHK(h, hipMemcpy(dst_host, t.ptr, n * 4, hipMemcpyDeviceToHost));
  } else {
    float* tmp = nullptr;
    HIPCHK(h, hipMalloc((void**)&tmp, n * 4));
    hipError_t r = launch_to_f32(t.mode, t.ptr, tmp, n, h->pl, nullptr);
    if (r == hipSuccess) r = hipMemcpy(dst_host, tmp, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    if (r != hipSuccess) return h->fail(DPTX_E_HIP, hipGetErrorString(r));
  }
  return DPTX_OK;
}

int dptx_forward_info(dptx_handle h, int64_t* launches, double* algorithmic_macs, double* executed_macs) {
  if (!h) return DPTX_E_INVALID;
  if (launches) *launches = h->launches;
  if (algorithmic_macs)  // SURVEY.md 8d (dual: 69.96 shared + 2 x 57.67 per image pair)
    *algorithmic_macs = h->backbone == DPTX_BACKBONE_VITL16_384
                            ? (h->cfg.num_channels == 3 ? 258.216e9 : 258.206e9)  // DPT-Large: 200.12 encoder + 58.08 decoder
                            : (h->cfg.dual_task ? 185.29e9 : (h->cfg.num_channels == 3 ? 127.624e9 : 127.615e9));
  if (executed_macs) *executed_macs = h->exec_macs;
  return DPTX_OK;
}

int dptx_set_profiling(dptx_handle h, int on) {
  if (!h) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  h->profiling = on != 0;
  return DPTX_OK;
}

int dptx_profile_get(dptx_handle h, int32_t category, double* ms, int64_t* launches, double* macs_per_image) {
  if (!h || category < 0 || category > 3) return DPTX_E_INVALID;
  if (h->event_cat.empty()) return h->fail(DPTX_E_INVALID, "no profiled forward recorded");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipEventSynchronize(h->events[h->event_cat.size()]));
  double t = 0.0;
  int64_t n = 0;
  for (size_t i = 0; i < h->event_cat.size(); ++i) {
    if (h->event_cat[i] != category) continue;
    float dt = 0.f;
    HIPCHK(h, hipEventElapsedTime(&dt, h->events[i], h->events[i + 1]));
    t += dt;
    ++n;
  }
  if (ms) *ms = t;
  if (launches) *launches = n;
  if (macs_per_image) *macs_per_image = h->cat_macs[category];
  return DPTX_OK;
}

int dptx_profile_dump(dptx_handle h, const char* path) {
  if (!h || !path) return DPTX_E_INVALID;
  if (h->event_cat.empty()) return h->fail(DPTX_E_INVALID, "no profiled forward recorded");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipEventSynchronize(h->events[h->event_cat.size()]));
  FILE* fp = fopen(path, "w");
  if (!fp) return h->fail(DPTX_E_INVALID, std::string("cannot open ") + path);
  fprintf(fp, "idx,category,name,ms\n");
  for (size_t i = 0; i < h->event_cat.size(); ++i) {
    float dt = 0.f;
    (void)hipEventElapsedTime(&dt, h->events[i], h->events[i + 1]);
    fprintf(fp, "%zu,%d,%s,%.5f\n", i, h->event_cat[i], h->event_name[i].c_str(), dt);
  }
  fclose(fp);
  return DPTX_OK;
}

// ---- arena debugging (tests/test_gpu_poison.py): a forward must not read an arena byte it did not write itself
int dptx_debug_arena_fill(dptx_handle h, int32_t byte_value) {
  if (!h) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  if (!h->d_arena) return h->fail(DPTX_E_INVALID, "no arena yet (weights not finalized / imported)");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemset(h->d_arena, byte_value & 0xff, h->arena_bytes));
  HIPCHK(h, hipDeviceSynchronize());
  return DPTX_OK;
}

int dptx_debug_arena_read(dptx_handle h, void* dst_host, size_t offset, size_t bytes) {
  if (!h || !dst_host) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return h->fail(DPTX_E_NODEVICE, "host-only handle");
  if (!h->d_arena || offset > h->arena_bytes || bytes > h->arena_bytes - offset) return h->fail(DPTX_E_INVALID, "arena range");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(dst_host, h->d_arena + offset, bytes, hipMemcpyDeviceToHost));
  return DPTX_OK;
}

int dptx_debug_arena_layout(dptx_handle h, char* dst, size_t capacity) {
  if (!h) return DPTX_E_INVALID;
  std::string s;
  char line[256];
  snprintf(line, sizeof line, "arena_bytes %zu\narena_single %zu\nhalf_region %zu\nhalf_batch %d\nmax_batch %d\nn_streams %d\nplanes %d\n",
           h->arena_bytes, h->arena_single, h->half_region, h->half_batch, h->cfg.max_batch, h->n_streams, h->two_planes() ? 2 : 1);
  s += line;
  for (const auto& nb : h->arena_bufs) {
    snprintf(line, sizeof line, "buf %s %zu %zu %zu\n", nb.first.c_str(), nb.second->off, nb.second->bytes, nb.second->off2);
    s += line;
  }
  if (dst && capacity > 0) {
    const size_t n = s.size() < capacity - 1 ? s.size() : capacity - 1;
    memcpy(dst, s.data(), n);
    dst[n] = 0;
  }
  return (int)s.size() + 1;
}

// One 64-bit word sum (order-independent) per arena buffer, sub-batch region and plane of the layout the LAST forward used, on
// `stream` (i.e. behind that forward): out_dev[(plane * regions + region) * nbuf + buf], buffers in dptx_debug_arena_layout
// order.  Returns the number of sums (or the capacity needed when out_dev is null).  Comparing the vectors of two forwards of
// the same input names the first tensor that differs (round 4's hunt, profiles/history.md section 10).
int dptx_debug_arena_checksums(dptx_handle h, void* out_dev, int32_t capacity, void* stream) {
  if (!h) return DPTX_E_INVALID;
  const auto& bufs = h->arena_bufs;
  const int nbuf = (int)bufs.size();
  const int regions = h->last_regions > 1 ? h->last_regions : 1;
  const int planes = h->two_planes() ? 2 : 1;
  const int total = planes * regions * nbuf;
  if (!out_dev) return total;
  if (capacity < total) return h->fail(DPTX_E_INVALID, "checksum buffer too small");
  if (h->cfg.device_id < 0 || !h->d_arena) return h->fail(DPTX_E_INVALID, "no arena");
  DeviceGuard guard(h->cfg.device_id);
  HIPCHK(h, guard.err);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(h, hipMemsetAsync(out_dev, 0, (size_t)total * 8, st));
  // extent of a buffer in the plan in use: up to the next buffer's offset
  std::vector<std::pair<size_t, int>> order;
  for (int i = 0; i < nbuf; ++i) order.push_back({regions > 1 ? bufs[i].second->off2 : bufs[i].second->off, i});
  std::sort(order.begin(), order.end());
  const size_t plan_end = regions > 1 ? h->half_region : h->arena_single;
  for (int pl = 0; pl < planes; ++pl)
    for (int r = 0; r < regions; ++r)
      for (int k = 0; k < nbuf; ++k) {
        const size_t off = order[k].first, end = k + 1 < nbuf ? order[k + 1].first : plan_end;
        if (end <= off) continue;
        const char* base = h->d_arena + (size_t)pl * h->arena_single + (regions > 1 ? (size_t)r * h->half_region : 0) + off;
        HIPCHK(h, launch_checksum(base, end - off, (unsigned long long*)out_dev + ((size_t)pl * regions + r) * nbuf + order[k].second, st));
      }
  return total;
}

}  // extern "C"
