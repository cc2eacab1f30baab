// Runs dptx_tta_align_depth and dptx_tta_merge_depth of csrc/tta_depth.hip, compiled for the host, on a case read from files:
// maps (fp32), views (dptx_tta_view[]), outs (dptx_image_desc[]), anchors (int32[]); writes the packed output and the
// coefficients.  Every buffer is a heap block of exactly its size, so AddressSanitizer reports any access outside it.
//   main <maps> <views> <outs> <anchors> <mode> <align 0|1> <output bytes> <output file> <coeffs file>
//
// The stand-in for <hip/hip_runtime.h> is the one of tests/tta_cpu_build (through -I): blocks and threads run one after the
// other.  The stats and solve kernels reduce over a block (select.h: wave_sum, block_sum), which the launch below makes exact
// for sequential threads:
//   - the threads of a block run from the LAST to the first.  __shfl_down(v, o) of lane l reads lane l + o, which has already
//     finished and has logged the value it passed at every call; a reduction tree's calls are the same in every lane, so call i
//     of lane l pairs with call i of lane l + o, as on the device.
//   - every block runs TWICE.  block_sum hands the four waves' sums through LDS (a static array here) behind a barrier; in the
//     second run every slot holds what the first run stored -- the same values, the kernels are deterministic -- so the threads
//     that combine them read what they would read behind the barrier.  Stores of the first run are overwritten by the second.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

constexpr int SHFL_CALLS = 64;
static double g_shfl[64][SHFL_CALLS];
static int g_shfl_call;
static inline double __shfl_down(double v, int o, int) {
  const int lane = threadIdx.x & 63, i = g_shfl_call++;
  if (i >= SHFL_CALLS) abort();
  g_shfl[lane][i] = v;
  return lane + o < 64 ? g_shfl[lane + o][i] : v;
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shmem, st, ...) do { dim3 g_ = grid, b_ = block; blockDim = b_; \
  for (unsigned bx = 0; bx < g_.x; ++bx) for (int pass = 0; pass < 2; ++pass) for (unsigned tx = b_.x; tx-- > 0;) { \
    blockIdx = dim3(bx); threadIdx = dim3(tx); g_shfl_call = 0; k(__VA_ARGS__); } } while (0)

#include "../../omnidata_amd/csrc/tta_depth.hip"

static std::vector<char> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> b(n);
  if (n && fread(b.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return b;
}

static void dump(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) exit(2);
  fwrite(p, 1, n, f);
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  const std::vector<char> maps = slurp(argv[1]), views = slurp(argv[2]), outs = slurp(argv[3]), anchors = slurp(argv[4]);
  const int mode = atoi(argv[5]), align = atoi(argv[6]);
  const long nbytes = atol(argv[7]);
  const int n_views = (int)(views.size() / sizeof(dptx_tta_view)), B = (int)(outs.size() / sizeof(dptx_image_desc));
  // exact heap blocks with the alignment of their element types
  float* m = (float*)malloc(maps.size());
  memcpy(m, maps.data(), maps.size());
  dptx_tta_view* v = (dptx_tta_view*)malloc(views.size());
  memcpy(v, views.data(), views.size());
  dptx_image_desc* o = (dptx_image_desc*)malloc(outs.size());
  memcpy(o, outs.data(), outs.size());
  int32_t* an = (int32_t*)malloc(anchors.size());
  memcpy(an, anchors.data(), anchors.size());
  uint32_t* out = (uint32_t*)malloc(nbytes);
  memset(out, 0xA5, nbytes);
  float* coeffs = (float*)malloc((size_t)n_views * 8);
  memset(coeffs, 0xFF, (size_t)n_views * 8);

  int rc = 0;
  void* ws = nullptr;
  if (align) {
    int64_t ws_bytes = 0;
    if (anchors.size() != (size_t)B * 4) return 2;
    rc = dptx_tta_depth_workspace_bytes(v, n_views, o, B, &ws_bytes);
    if (rc == 0) {
      ws = malloc(ws_bytes);
      memset(ws, 0xFF, ws_bytes);  // NaN records: a record the solve reads but the stats pass did not write shows in the result
      rc = dptx_tta_align_depth(m, v, n_views, an, o, B, coeffs, ws, ws_bytes, nullptr);
    }
  }
  if (rc == 0) rc = dptx_tta_merge_depth(m, v, n_views, align ? coeffs : nullptr, o, B, mode, out, ws, nullptr);
  dump(argv[8], out, nbytes);
  dump(argv[9], coeffs, (size_t)n_views * 8);
  free(ws); free(coeffs); free(out); free(an); free(o); free(v); free(m);
  return rc == 0 ? 0 : 1;
}
