// unet_engine.hip -- the version-1 UNet behind a handle of its own (include/dptx.h dptx_unet_*): strict loading of the
// reference's 174 state-dict tensors, packing into one blob, the activation arena and the forward's schedule.
//
// Schedule (c_i = 16 * 2^i channels at level i = 1 / 2^i of the input size):
//   im2col -> down1 (3 convs at level 0, 16 ch) -> down_blocks.i (3 convs at level i, c_{i+1} ch, 2x2 max-pool to level i+1)
//   -> 3 mid convs (1024 ch, level 6) -> up_blocks.i for i = 5..0 (bilinear x2 to level i, concat, 3 convs, c_i ch)
//   -> last_conv1 -> last_bn + ReLU + last_conv2 (fp32 NCHW result).
// Every convolution stores its raw 16-bit output (bias added); GroupNorm(8) + ReLU is a pass of its own.  torch.cat((up, skip))
// costs nothing: level i has ONE buffer CAT_i of 3 c_i channels per pixel; the up-sample writes channels [0, 2 c_i) and the skip's
// producer (the pooled GroupNorm apply of down_blocks.(i-1), down1's last apply for level 0) writes [2 c_i, 3 c_i).  The next down
// block reads that same slice as its input, so no tensor is stored twice.
// Layers with Cin or Cout below 64 run on unet.hip's small-channel kernel (GroupNorm records from its epilogue); the others go
// through launch_gemm, followed by a statistics pass.  Either way the statistics are those of the stored (rounded) values, so
// an fp16 overflow reaches the sums and sets the range flag.  tests/unet_restatement.py restates exactly this.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/dptx.h"
#include "host_util.h"
#include "kernels.h"
#include "unet.h"

using namespace dptx;

namespace {

constexpr int LEVELS = 6;
inline int chan(int i) { return 16 << i; }

struct ConvLayer {
  std::string name;        // "down1.conv1", "mid_conv1", ...
  int cin, cout, ksz;
  size_t w_off, b_off;     // bytes into the blob
};
struct NormLayer {
  std::string name;        // "down1.bn1", "bn1", "last_bn"
  int c;
  size_t g_off, b_off;
};
struct Entry {             // one state-dict tensor
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
};

}  // namespace

struct dptx_unet_engine {
  dptx_unet_config cfg;
  int mode;  // MODE_BF16 / MODE_FP16
  std::vector<ConvLayer> convs;
  std::vector<NormLayer> norms;
  std::map<std::string, int> conv_index, norm_index;
  std::vector<std::string> keys;  // the 174 keys in state-dict order
  std::map<std::string, Entry> entries;
  std::map<std::string, std::pair<size_t, size_t>> packed_off;  // key -> (offset, bytes)
  size_t packed_bytes = 0;
  std::vector<uint8_t> blob;
  bool finalized = false;
  // device
  uint8_t* d_blob = nullptr;
  uint8_t* d_arena = nullptr;
  unsigned* d_flag = nullptr;
  size_t arena_bytes = 0;
  // arena offsets (bytes)
  size_t o_p = 0, o_raw = 0, o_a = 0, o_b = 0, o_xa = 0, o_xb = 0, o_rec = 0, o_stats = 0, o_cat[LEVELS] = {};
  std::string err;
};

namespace {

void add_conv(dptx_unet_engine* e, const std::string& name, int cin, int cout, int ksz) {
  ConvLayer c{name, cin, cout, ksz, 0, 0};
  e->conv_index[name] = (int)e->convs.size();
  e->convs.push_back(c);
  e->keys.push_back(name + ".weight");
  e->entries[name + ".weight"].shape = {cout, cin, ksz, ksz};
  e->keys.push_back(name + ".bias");
  e->entries[name + ".bias"].shape = {cout};
}
void add_norm(dptx_unet_engine* e, const std::string& name, int c) {
  e->norm_index[name] = (int)e->norms.size();
  e->norms.push_back(NormLayer{name, c, 0, 0});
  e->keys.push_back(name + ".weight");
  e->entries[name + ".weight"].shape = {c};
  e->keys.push_back(name + ".bias");
  e->entries[name + ".bias"].shape = {c};
}
void add_block(dptx_unet_engine* e, const std::string& pre, int cin, int cout) {
  for (int j = 1; j <= 3; ++j) {
    add_conv(e, pre + ".conv" + std::to_string(j), j == 1 ? cin : cout, cout, 3);
    add_norm(e, pre + ".bn" + std::to_string(j), cout);
  }
}

void build_layers(dptx_unet_engine* e) {
  add_block(e, "down1", 3, 16);
  for (int i = 0; i < LEVELS; ++i) add_block(e, "down_blocks." + std::to_string(i), chan(i), chan(i + 1));
  for (int j = 1; j <= 3; ++j) {
    add_conv(e, "mid_conv" + std::to_string(j), 1024, 1024, 3);
    add_norm(e, "bn" + std::to_string(j), 1024);
  }
  for (int i = 0; i < LEVELS; ++i) add_block(e, "up_blocks." + std::to_string(i), 3 * chan(i), chan(i));
  add_conv(e, "last_conv1", 16, 16, 3);
  add_norm(e, "last_bn", 16);
  add_conv(e, "last_conv2", 16, e->cfg.out_channels, 1);
  // blob layout: the entries in key order, 256-byte aligned.  Convolution weights: 16-bit [O][ky][kx][I]; down1.conv1: 16-bit
  // [16][32], k = (ky*3 + kx)*3 + c, k = 27..31 zero; last_conv2.weight: fp32 [O][16]; biases and norm vectors: fp32
  size_t off = 0;
  for (const std::string& k : e->keys) {
    const Entry& en = e->entries[k];
    size_t n = 1;
    for (int64_t d : en.shape) n *= (size_t)d;
    size_t bytes = n * 4;
    if (en.shape.size() == 4) {
      if (k == "down1.conv1.weight") bytes = 16 * 32 * 2;
      else if (k == "last_conv2.weight") bytes = n * 4;
      else bytes = n * 2;
    }
    e->packed_off[k] = {off, bytes};
    off += align_up(bytes, 256);
  }
  e->packed_bytes = off;
  for (ConvLayer& c : e->convs) {
    c.w_off = e->packed_off[c.name + ".weight"].first;
    c.b_off = e->packed_off[c.name + ".bias"].first;
  }
  for (NormLayer& n : e->norms) {
    n.g_off = e->packed_off[n.name + ".weight"].first;
    n.b_off = e->packed_off[n.name + ".bias"].first;
  }
}

void plan_arena(dptx_unet_engine* e) {
  const size_t B = (size_t)e->cfg.max_batch, HW = (size_t)e->cfg.max_height * e->cfg.max_width;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  const size_t big = B * HW * 32 * 2;  // the largest raw / activation tensor: 32 channels at level 0 (= c_{i+1} at level i)
  e->o_p = take(big);                  // im2col of the input
  e->o_raw = take(big);
  e->o_a = take(big);
  e->o_b = take(big);
  e->o_xa = take(B * HW * 16 * 2);     // block outputs: c_i channels at level i, 1024 at level 6
  e->o_xb = take(B * HW * 16 * 2);
  for (int i = 0; i < LEVELS; ++i) e->o_cat[i] = take(B * (HW >> (2 * i)) * 3 * chan(i) * 2);
  size_t nrec = (size_t)unet_conv_tiles(e->cfg.max_height, e->cfg.max_width);
  for (int i = 0; i <= LEVELS; ++i) {
    const size_t r = (size_t)unet_gn_chunks((int)(HW >> (2 * i)), 1024);  // the largest chunk count of any C at that level
    if (r > nrec) nrec = r;
  }
  e->o_rec = take(B * nrec * 8 * 8);
  e->o_stats = take(B * 8 * 8);
  e->arena_bytes = off;
}

int fail(dptx_unet_engine* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}

#define UCHK(h, call)                                                                         \
  do {                                                                                        \
    const hipError_t r_ = (call);                                                             \
    if (r_ != hipSuccess) return fail(h, DPTX_E_HIP, std::string(#call) + ": " + hipGetErrorString(r_)); \
  } while (0)

// launch classes of dptx_unet_debug_forward_classes
constexpr int CLS_SMALL = 1, CLS_GEMM = 2, CLS_PASS = 4;

struct Fwd {
  dptx_unet_engine* h;
  hipStream_t st;
  int B, H, W, classes;
  hipError_t rc = hipSuccess;
  const char* where = "";

  uint16_t* buf(size_t off) const { return (uint16_t*)(h->d_arena + off); }
  float* rec() const { return (float*)(h->d_arena + h->o_rec); }
  float* stats() const { return (float*)(h->d_arena + h->o_stats); }
  const float* f32(size_t off) const { return (const float*)(h->d_blob + off); }
  void note(hipError_t r, const char* w) {
    if (rc == hipSuccess && r != hipSuccess) { rc = r; where = w; }
  }

  // raw convolution output into RAW and the (mean, rstd) table of its GroupNorm
  void conv(const std::string& name, const void* X, int pix_stride, int off, size_t x_bytes, int Hl, int Wl, bool first = false) {
    const ConvLayer& c = h->convs[h->conv_index.at(name)];
    int nrec;
    const bool small = first || unet_conv_small_supported(c.cin, c.cout, 9);
    if (small) {
      UnetConvParams p{};
      p.X = X; p.Wt = h->d_blob + c.w_off; p.bias = f32(c.b_off); p.Y = buf(h->o_raw); p.gn_part = rec();
      p.B = B; p.H = Hl; p.W = Wl; p.Cin = first ? 32 : c.cin; p.Cout = c.cout; p.taps = first ? 1 : 9;
      p.x_pix_stride = pix_stride; p.x_off = off;
      if (classes & CLS_SMALL) note(launch_unet_conv_small(h->mode, p, st), "small conv");
      nrec = unet_conv_tiles(Hl, Wl);
    } else {
      GemmParams p;
      gemm_params_unet_conv(p, B, Hl, Wl, c.cin, c.cout, pix_stride, off, (long long)x_bytes);
      p.A = X; p.W = h->d_blob + c.w_off; p.C = buf(h->o_raw); p.bias = f32(c.b_off);
      if (classes & CLS_GEMM) note(launch_gemm(h->mode, p, st), "gemm conv");
      if (classes & CLS_PASS) note(launch_unet_gn_stats(h->mode, buf(h->o_raw), rec(), B, Hl * Wl, c.cout, st), "gn stats");
      nrec = unet_gn_chunks(Hl * Wl, c.cout);
    }
    if (classes & CLS_PASS)
      note(launch_unet_gn_finalize(rec(), nrec, stats(), B, Hl * Wl, c.cout, 1e-5f, h->d_flag, st), "gn finalize");
  }
  void apply(const std::string& norm, int Hl, int Wl, void* Y, int ys, int yo, void* P, int ps, int po) {
    const NormLayer& n = h->norms[h->norm_index.at(norm)];
    UnetGnApply a{};
    a.X = buf(h->o_raw); a.stats = stats(); a.gamma = f32(n.g_off); a.beta = f32(n.b_off);
    a.Y = Y; a.y_pix_stride = ys; a.y_off = yo; a.P = P; a.p_pix_stride = ps; a.p_off = po;
    a.B = B; a.H = Hl; a.W = Wl; a.C = n.c;
    if (classes & CLS_PASS) note(launch_unet_gn_apply(h->mode, a, st), "gn apply");
  }
  // conv1..3 of a block at (Hl, Wl): the last apply goes to (Y / P) as given
  void block(const std::string& pre, const void* X, int xs, int xo, size_t x_bytes, int Hl, int Wl, int cout, void* Y, int ys, int yo,
             void* P, int ps, int po, bool first = false) {
    const size_t act_bytes = (size_t)B * Hl * Wl * cout * 2;
    conv(pre + ".conv1", X, xs, xo, x_bytes, Hl, Wl, first);
    apply(pre + ".bn1", Hl, Wl, buf(h->o_a), cout, 0, nullptr, 0, 0);
    conv(pre + ".conv2", buf(h->o_a), cout, 0, act_bytes, Hl, Wl);
    apply(pre + ".bn2", Hl, Wl, buf(h->o_b), cout, 0, nullptr, 0, 0);
    conv(pre + ".conv3", buf(h->o_b), cout, 0, act_bytes, Hl, Wl);
    apply(pre + ".bn3", Hl, Wl, Y, ys, yo, P, ps, po);
  }

  void run(const void* x, int io, float* y) {
    if (classes & CLS_SMALL) note(launch_unet_im2col3(h->mode, x, io, buf(h->o_p), B, H, W, st), "im2col");
    auto cat_bytes = [&](int i) { return (size_t)B * (H >> i) * (W >> i) * 3 * chan(i) * 2; };
    // down1: its output is level 0's skip
    block("down1", buf(h->o_p), 32, 0, (size_t)B * H * W * 32 * 2, H, W, 16, buf(h->o_cat[0]), 48, 32, nullptr, 0, 0, true);
    // down blocks: read level i's skip slice, pool into level i+1's skip slice (the last one into a dense tensor)
    for (int i = 0; i < LEVELS; ++i) {
      const int Hl = H >> i, Wl = W >> i, co = chan(i + 1);
      void* P = i + 1 < LEVELS ? (void*)buf(h->o_cat[i + 1]) : (void*)buf(h->o_xa);
      const int ps = i + 1 < LEVELS ? 3 * co : co, po = i + 1 < LEVELS ? 2 * co : 0;
      block("down_blocks." + std::to_string(i), buf(h->o_cat[i]), 3 * chan(i), 2 * chan(i), cat_bytes(i), Hl, Wl, co, nullptr, 0, 0, P, ps, po);
    }
    // middle, at level 6
    {
      const int Hl = H >> LEVELS, Wl = W >> LEVELS;
      const size_t bytes = (size_t)B * Hl * Wl * 1024 * 2;
      conv("mid_conv1", buf(h->o_xa), 1024, 0, bytes, Hl, Wl);
      apply("bn1", Hl, Wl, buf(h->o_a), 1024, 0, nullptr, 0, 0);
      conv("mid_conv2", buf(h->o_a), 1024, 0, bytes, Hl, Wl);
      apply("bn2", Hl, Wl, buf(h->o_b), 1024, 0, nullptr, 0, 0);
      conv("mid_conv3", buf(h->o_b), 1024, 0, bytes, Hl, Wl);
      apply("bn3", Hl, Wl, buf(h->o_xa), 1024, 0, nullptr, 0, 0);
    }
    // up blocks: x (2 c_i channels at level i+1) -> CAT_i[0, 2 c_i), three convs, c_i channels at level i
    size_t xin = h->o_xa, xout = h->o_xb;
    for (int i = LEVELS - 1; i >= 0; --i) {
      const int Hl = H >> i, Wl = W >> i, c = chan(i);
      if (classes & CLS_PASS)
        note(launch_unet_upsample2x(h->mode, buf(xin), buf(h->o_cat[i]), B, Hl / 2, Wl / 2, 2 * c, 3 * c, 0, st), "upsample");
      block("up_blocks." + std::to_string(i), buf(h->o_cat[i]), 3 * c, 0, cat_bytes(i), Hl, Wl, c, buf(xout), c, 0, nullptr, 0, 0);
      std::swap(xin, xout);
    }
    conv("last_conv1", buf(xin), 16, 0, (size_t)B * H * W * 16 * 2, H, W);
    const NormLayer& n = h->norms[h->norm_index.at("last_bn")];
    const ConvLayer& c2 = h->convs[h->conv_index.at("last_conv2")];
    if (classes & CLS_PASS)
      note(launch_unet_gn_head(h->mode, buf(h->o_raw), stats(), f32(n.g_off), f32(n.b_off), f32(c2.w_off), f32(c2.b_off), y, B, H * W,
                               h->cfg.out_channels, st), "head");
  }
};

int check_forward_args(dptx_unet_engine* h, const void* x, void* y, int B, int H, int W, int x_dtype) {
  if (!h) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return fail(h, DPTX_E_NODEVICE, "host-only handle");
  if (!h->finalized || !h->d_blob) return fail(h, DPTX_E_INVALID, "weights not finalized");
  if (!x || !y) return fail(h, DPTX_E_INVALID, "null buffer");
  if (x_dtype < DPTX_IO_FP32 || x_dtype > DPTX_IO_FP16) return fail(h, DPTX_E_INVALID, "bad x_dtype");
  if (B < 1 || B > h->cfg.max_batch) return fail(h, DPTX_E_INVALID, "batch outside 1..max_batch");
  if (H % 64 != 0 || W % 64 != 0 || H < 64 || W < 64 || H > h->cfg.max_height || W > h->cfg.max_width)
    return fail(h, DPTX_E_INVALID, "height and width must be multiples of 64 in 64..max_height / max_width");
  return DPTX_OK;
}

int forward_impl(dptx_unet_engine* h, const void* x, void* y, int B, int H, int W, int x_dtype, void* stream, int classes) {
  const int rc = check_forward_args(h, x, y, B, H, W, x_dtype);
  if (rc != DPTX_OK) return rc;
  DeviceGuard guard(h->cfg.device_id);
  Fwd f{h, (hipStream_t)stream, B, H, W, classes};
  f.run(x, x_dtype, (float*)y);
  if (f.rc != hipSuccess) return fail(h, DPTX_E_HIP, std::string(f.where) + ": " + hipGetErrorString(f.rc));
  return DPTX_OK;
}

}  // namespace

extern "C" {

void dptx_unet_default_config(dptx_unet_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->out_channels = 3;
  cfg->max_batch = 32;
  cfg->dtype = DPTX_DTYPE_FP16;
  cfg->device_id = 0;
  cfg->max_height = 384;
  cfg->max_width = 384;
}

int dptx_unet_create(dptx_unet_handle* out, const dptx_unet_config* cfg) {
  if (!out || !cfg) return DPTX_E_INVALID;
  *out = nullptr;
  if (cfg->out_channels < 1 || cfg->out_channels > 4 || cfg->max_batch < 1 || cfg->max_batch > 32 ||
      (cfg->dtype != DPTX_DTYPE_FP16 && cfg->dtype != DPTX_DTYPE_BF16) || cfg->max_height % 64 != 0 || cfg->max_width % 64 != 0 ||
      cfg->max_height < 64 || cfg->max_width < 64 || cfg->max_height > 512 || cfg->max_width > 512 || cfg->reserved[0] != 0 ||
      cfg->reserved[1] != 0)
    return DPTX_E_INVALID;
  dptx_unet_engine* e = new (std::nothrow) dptx_unet_engine();
  if (!e) return DPTX_E_ALLOC;
  e->cfg = *cfg;
  e->mode = cfg->dtype == DPTX_DTYPE_FP16 ? MODE_FP16 : MODE_BF16;
  build_layers(e);
  plan_arena(e);
  if (cfg->device_id >= 0) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || cfg->device_id >= n) {
      delete e;
      return DPTX_E_NODEVICE;
    }
  }
  *out = e;
  return DPTX_OK;
}

void dptx_unet_destroy(dptx_unet_handle h) {
  if (!h) return;
  if (h->cfg.device_id >= 0) {
    DeviceGuard guard(h->cfg.device_id);
    if (h->d_blob) (void)hipFree(h->d_blob);
    if (h->d_arena) (void)hipFree(h->d_arena);
    if (h->d_flag) (void)hipFree(h->d_flag);
  }
  delete h;
}

const char* dptx_unet_last_error(dptx_unet_handle h) { return h ? h->err.c_str() : "null handle"; }

int dptx_unet_load_tensor(dptx_unet_handle h, const char* ref_key, const float* host_fp32, const int64_t* shape, int32_t ndim) {
  if (!h || !ref_key || !host_fp32 || !shape || ndim < 1) return DPTX_E_INVALID;
  auto it = h->entries.find(ref_key);
  if (it == h->entries.end()) return fail(h, DPTX_E_KEY, std::string("unexpected key ") + ref_key);
  Entry& en = it->second;
  bool same = (size_t)ndim == en.shape.size();
  for (int i = 0; same && i < ndim; ++i) same = shape[i] == en.shape[i];
  if (!same) {
    std::string got, want;
    for (int i = 0; i < ndim; ++i) got += (i ? "," : "") + std::to_string(shape[i]);
    for (size_t i = 0; i < en.shape.size(); ++i) want += (i ? "," : "") + std::to_string(en.shape[i]);
    return fail(h, DPTX_E_KEY, std::string("shape mismatch for ") + ref_key + ": got [" + got + "], expected [" + want + "]");
  }
  size_t n = 1;
  for (int64_t d : en.shape) n *= (size_t)d;
  en.data.assign(host_fp32, host_fp32 + n);
  en.loaded = true;
  h->finalized = false;
  return DPTX_OK;
}

int dptx_unet_finalize_weights(dptx_unet_handle h) {
  if (!h) return DPTX_E_INVALID;
  std::string missing;
  int nmiss = 0;
  for (const std::string& k : h->keys)
    if (!h->entries[k].loaded) {
      if (nmiss < 16) missing += (nmiss ? ", " : "") + k;
      ++nmiss;
    }
  if (nmiss) return fail(h, DPTX_E_KEY, "missing tensors (" + std::to_string(nmiss) + "): " + missing + (nmiss > 16 ? ", ..." : ""));
  h->blob.assign(h->packed_bytes, 0);
  const bool bf = h->mode == MODE_BF16;
  auto cvt = [&](float f) { return bf ? f32_to_bf16(f) : f32_to_fp16(f); };
  for (const std::string& k : h->keys) {
    const Entry& en = h->entries[k];
    uint8_t* dst = h->blob.data() + h->packed_off[k].first;
    if (en.shape.size() == 4 && k != "last_conv2.weight") {
      const int O = (int)en.shape[0], I = (int)en.shape[1];
      uint16_t* d16 = (uint16_t*)dst;
      if (k == "down1.conv1.weight") {  // [16][32], k = (ky*3 + kx)*3 + c
        for (int o = 0; o < O; ++o)
          for (int c = 0; c < 3; ++c)
            for (int t = 0; t < 9; ++t) d16[o * 32 + t * 3 + c] = cvt(en.data[((size_t)o * 3 + c) * 9 + t]);
      } else {  // OIHW -> [O][ky][kx][I]; an up block's conv1 keeps torch.cat's order (up-sampled channels, then the skip)
        for (int o = 0; o < O; ++o)
          for (int c = 0; c < I; ++c)
            for (int t = 0; t < 9; ++t) d16[((size_t)o * 9 + t) * I + c] = cvt(en.data[((size_t)o * I + c) * 9 + t]);
      }
    } else {
      memcpy(dst, en.data.data(), en.data.size() * 4);
    }
  }
  if (h->cfg.device_id >= 0) {
    DeviceGuard guard(h->cfg.device_id);
    if (!h->d_blob) UCHK(h, hipMalloc((void**)&h->d_blob, h->packed_bytes));
    if (!h->d_arena) UCHK(h, hipMalloc((void**)&h->d_arena, h->arena_bytes));
    if (!h->d_flag) {
      UCHK(h, hipMalloc((void**)&h->d_flag, sizeof(unsigned)));
      UCHK(h, hipMemset(h->d_flag, 0, sizeof(unsigned)));
    }
    UCHK(h, hipDeviceSynchronize());  // no forward may be reading the old weights
    UCHK(h, hipMemcpy(h->d_blob, h->blob.data(), h->packed_bytes, hipMemcpyHostToDevice));
  }
  h->finalized = true;
  return DPTX_OK;
}

size_t dptx_unet_packed_bytes(dptx_unet_handle h) { return h ? h->packed_bytes : 0; }

int dptx_unet_packed_entry(dptx_unet_handle h, const char* ref_key, int64_t* offset, int64_t* bytes) {
  if (!h || !ref_key) return DPTX_E_INVALID;
  auto it = h->packed_off.find(ref_key);
  if (it == h->packed_off.end()) return fail(h, DPTX_E_KEY, std::string("unexpected key ") + ref_key);
  if (offset) *offset = (int64_t)it->second.first;
  if (bytes) *bytes = (int64_t)it->second.second;
  return DPTX_OK;
}

int dptx_unet_export_packed_host(dptx_unet_handle h, void* dst_host, size_t bytes) {
  if (!h || !dst_host) return DPTX_E_INVALID;
  if (!h->finalized) return fail(h, DPTX_E_INVALID, "weights not finalized");
  if (bytes < h->packed_bytes) return fail(h, DPTX_E_INVALID, "buffer too small");
  memcpy(dst_host, h->blob.data(), h->packed_bytes);
  return DPTX_OK;
}

size_t dptx_unet_device_bytes(dptx_unet_handle h) {
  if (!h || h->cfg.device_id < 0) return 0;
  return h->packed_bytes + h->arena_bytes;
}

int dptx_unet_forward(dptx_unet_handle h, const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t x_dtype, void* stream) {
  return forward_impl(h, x, y, B, H, W, x_dtype, stream, CLS_SMALL | CLS_GEMM | CLS_PASS);
}

int dptx_unet_debug_forward_classes(dptx_unet_handle h, const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t x_dtype,
                                    int32_t classes, void* stream) {
  return forward_impl(h, x, y, B, H, W, x_dtype, stream, classes & 7);
}

int dptx_unet_range_status(dptx_unet_handle h, int32_t* nonfinite, int32_t reset, void* stream) {
  if (!h || !nonfinite) return DPTX_E_INVALID;
  *nonfinite = 0;
  if (h->cfg.device_id < 0) return fail(h, DPTX_E_NODEVICE, "host-only handle");
  if (!h->d_flag) return DPTX_OK;  // no forward yet
  DeviceGuard guard(h->cfg.device_id);
  unsigned v = 0;
  UCHK(h, hipMemcpyAsync(&v, h->d_flag, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
  UCHK(h, hipStreamSynchronize((hipStream_t)stream));
  if (reset) UCHK(h, hipMemsetAsync(h->d_flag, 0, sizeof v, (hipStream_t)stream));
  *nonfinite = v ? 1 : 0;
  return DPTX_OK;
}

int dptx_unet_debug_arena_fill(dptx_unet_handle h, int32_t byte_value) {
  if (!h) return DPTX_E_INVALID;
  if (h->cfg.device_id < 0) return fail(h, DPTX_E_NODEVICE, "host-only handle");
  if (!h->d_arena) return fail(h, DPTX_E_INVALID, "weights not finalized");
  DeviceGuard guard(h->cfg.device_id);
  UCHK(h, hipDeviceSynchronize());
  UCHK(h, hipMemset(h->d_arena, byte_value, h->arena_bytes));
  UCHK(h, hipDeviceSynchronize());
  return DPTX_OK;
}

}  // extern "C"
