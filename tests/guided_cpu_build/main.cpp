// Runs the entry point of csrc/guided.hip, compiled for the host, on a case read from files: y (fp32 [B][C][h][w]), guide_lo (fp32
// [B][3][h][w]), pixels (uint8, packed), guides and outs (dptx_image_desc[B] each); writes the packed output.  Every buffer is a
// heap block of exactly its size, so AddressSanitizer reports any access outside it.
//   main <y> <guide_lo> <pixels> <guides> <outs> <C> <h> <w> <mode> <radius> <sigma_space> <sigma_range> <output bytes> <output file>
//
// The stand-in for <hip/hip_runtime.h> is the one of tests/tta_cpu_build (through -I).  The launch below also walks the grid's y
// axis (the min / max kernel has one row of blocks per image) and runs every block three times: the threads run one after the
// other, so in the first run a thread meets a tile only partly staged; in the second run LDS holds what the first one staged for
// the same tile and the values are exact; in the third the uint8 rows, which leave LDS behind a barrier, hold the second run's
// values when they are flushed.  That does not hold for DEPTH_RGBA, whose min / max kernel reduces through LDS: there only the
// addresses are meaningful.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shmem, st, ...) do { dim3 g_ = grid, b_ = block; blockDim = b_; \
  for (unsigned by = 0; by < g_.y; ++by) for (unsigned bx = 0; bx < g_.x; ++bx) for (int pass = 0; pass < 3; ++pass) \
    for (unsigned tx = 0; tx < b_.x; ++tx) { blockIdx = dim3(bx, by); threadIdx = dim3(tx); k(__VA_ARGS__); } } while (0)

#include "../../omnidata_amd/csrc/guided.hip"

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

// an exact heap block with the file's bytes
static void* block(const std::vector<char>& b) {
  void* p = malloc(b.size());
  memcpy(p, b.data(), b.size());
  return p;
}

int main(int argc, char** argv) {
  if (argc != 15) return 2;
  const std::vector<char> y = slurp(argv[1]), lo = slurp(argv[2]), px = slurp(argv[3]), gd = slurp(argv[4]), od = slurp(argv[5]);
  const int C = atoi(argv[6]), h = atoi(argv[7]), w = atoi(argv[8]), mode = atoi(argv[9]);
  dptx_guided_params params = {atoi(argv[10]), (float)atof(argv[11]), (float)atof(argv[12])};
  const long nbytes = atol(argv[13]);
  const int B = (int)(od.size() / sizeof(dptx_image_desc));
  if (gd.size() != od.size() || y.size() != (size_t)B * C * h * w * 4 || lo.size() != (size_t)B * 3 * h * w * 4) return 2;
  void *yp = block(y), *lop = block(lo), *pxp = block(px), *gp = block(gd), *op = block(od);
  uint32_t* out = (uint32_t*)malloc(nbytes);
  memset(out, 0xA5, nbytes);
  uint32_t lut[256];
  for (int i = 0; i < 256; ++i) lut[i] = 0x01010101u * (uint32_t)i;
  uint32_t* lutp = (uint32_t*)malloc(sizeof(lut));
  memcpy(lutp, lut, sizeof(lut));

  int64_t ws_bytes = 0;
  int rc = dptx_postprocess_guided_workspace_bytes(B, mode, &ws_bytes);
  void* ws = nullptr;
  if (rc == 0) {
    if (ws_bytes) {
      ws = malloc(ws_bytes);
      memset(ws, 0, ws_bytes);
    }
    rc = dptx_postprocess_guided_batch(yp, lop, B, C, h, w, pxp, (const dptx_image_desc*)gp, (const dptx_image_desc*)op, &params, mode,
                                       out, lutp, ws, ws_bytes, nullptr);
  }
  FILE* f = fopen(argv[14], "wb");
  if (!f) return 2;
  fwrite(out, 1, nbytes, f);
  fclose(f);
  free(ws); free(lutp); free(out); free(op); free(gp); free(pxp); free(lop); free(yp);
  return rc == 0 ? 0 : 1;
}
