// Runs the entry points of csrc/tiles.hip, compiled for the host, on a case read from files: maps (fp32), grids
// (dptx_tile_grid[]), outs (dptx_image_desc[]); writes the packed output and the coefficients.  Every buffer is a heap block of
// exactly its size, so AddressSanitizer reports any access outside it.
//   main <maps> <grids> <outs> <task: normal|depth> <mode> <align 0|1> <output bytes> <output file> <coeffs file>
//
// The stand-in for <hip/hip_runtime.h> is the one of tests/tta_cpu_build (through -I); the launch below is the one of
// tests/tta_depth_cpu_build/main.cpp: the threads of a block run from the last to the first and every block runs twice, which
// makes the shuffles of the stats and solve kernels, block_sum's LDS round and -- new here -- the uint8 rows that leave LDS
// behind a barrier exact for sequential threads (in the second run the staging rows hold what the first run stored).
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

#include "../../omnidata_amd/csrc/tiles.hip"

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
  const std::vector<char> maps = slurp(argv[1]), grids = slurp(argv[2]), outs = slurp(argv[3]);
  const bool depth = strcmp(argv[4], "depth") == 0;
  const int mode = atoi(argv[5]), align = atoi(argv[6]);
  const long nbytes = atol(argv[7]);
  const int B = (int)(outs.size() / sizeof(dptx_image_desc));
  if (grids.size() != (size_t)B * sizeof(dptx_tile_grid)) return 2;
  // exact heap blocks with the alignment of their element types
  float* m = (float*)malloc(maps.size());
  memcpy(m, maps.data(), maps.size());
  dptx_tile_grid* g = (dptx_tile_grid*)malloc(grids.size());
  memcpy(g, grids.data(), grids.size());
  dptx_image_desc* o = (dptx_image_desc*)malloc(outs.size());
  memcpy(o, outs.data(), outs.size());
  uint32_t* out = (uint32_t*)malloc(nbytes);
  memset(out, 0xA5, nbytes);
  size_t n_tiles = 0;
  for (int i = 0; i < B; ++i) n_tiles += (size_t)g[i].ny * g[i].nx;
  float* coeffs = (float*)malloc(n_tiles * 8);
  memset(coeffs, 0xFF, n_tiles * 8);

  int rc = 0;
  void* ws = nullptr;
  if (!depth) {
    rc = dptx_tile_blend_normals(m, g, o, B, mode, out, nullptr);
  } else {
    if (align) {
      int64_t ws_bytes = 0;
      rc = dptx_tile_depth_workspace_bytes(g, o, B, &ws_bytes);
      if (rc == 0) {
        ws = malloc(ws_bytes);
        memset(ws, 0xFF, ws_bytes);  // NaN records: a record the solve reads but the stats pass did not write shows in the result
        rc = dptx_tile_align_depth(m, g, o, B, coeffs, ws, ws_bytes, nullptr);
      }
    }
    if (rc == 0) rc = dptx_tile_blend_depth(m, g, align ? coeffs : nullptr, o, B, mode, out, nullptr);
  }
  dump(argv[8], out, nbytes);
  dump(argv[9], coeffs, n_tiles * 8);
  free(ws); free(coeffs); free(out); free(o); free(g); free(m);
  return rc == 0 ? 0 : 1;
}
