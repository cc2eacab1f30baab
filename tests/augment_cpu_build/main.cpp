// Runs the entry points of csrc/augment.hip, compiled for the host, on a case read from files.  Every buffer is a heap block of
// exactly its size, so AddressSanitizer reports any access outside it.
//   main chain  <x> B C H W <sharp|-> <motion|-> km <gy|-> <gx|-> kgy kgx <out>
//   main resize B Hs Ws op y0 x0 h w n { <src> C dtype interp <out> } x n
// Prints the entry point's return code; exits 0 when it ran (a sanitizer report ends the program with its text).
//
// The stand-in for <hip/hip_runtime.h> is the one of tests/tta_cpu_build (through -I): the threads of a block run one after the
// other, so a stage that reads what all threads of the stage before it left in LDS sees it only in a later run of the block.
// Every block therefore runs four times -- the staged input is complete after the first run, the sharpness result after the
// second, the motion result after the third, the output after the fourth; every stage has an LDS buffer of its own, so a run
// never overwrites what a later thread of the same run still reads.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shmem, st, ...) do { dim3 g_ = grid, b_ = block; blockDim = b_; \
  for (unsigned bx = 0; bx < g_.x; ++bx) for (int pass = 0; pass < 4; ++pass) for (unsigned tx = 0; tx < b_.x; ++tx) { \
    blockIdx = dim3(bx); threadIdx = dim3(tx); k(__VA_ARGS__); } } while (0)

#include "../../omnidata_amd/csrc/augment.hip"

static void* slurp(const char* path, size_t* n_out = nullptr) {
  if (strcmp(path, "-") == 0) return nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc(n);  // an exact heap block
  if (n && fread(p, 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  if (n_out) *n_out = n;
  return p;
}

static void dump(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) exit(2);
  fwrite(p, 1, n, f);
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (strcmp(argv[1], "chain") == 0) {
    if (argc != 15) return 2;
    size_t nx = 0;
    float* x = (float*)slurp(argv[2], &nx);
    const int B = atoi(argv[3]), C = atoi(argv[4]), H = atoi(argv[5]), W = atoi(argv[6]);
    if (nx != (size_t)B * C * H * W * 4) return 2;
    float* sharp = (float*)slurp(argv[7]);
    float* motion = (float*)slurp(argv[8]);
    const int km = atoi(argv[9]);
    float* gy = (float*)slurp(argv[10]);
    float* gx = (float*)slurp(argv[11]);
    const int kgy = atoi(argv[12]), kgx = atoi(argv[13]);
    float* out = (float*)malloc(nx);
    memset(out, 0xFF, nx);  // NaN: an output the kernel does not write shows
    const int rc = dptx_augment_filter_chain(x, B, C, H, W, sharp, motion, km, gy, gx, kgy, kgx, out, nullptr);
    dump(argv[14], out, nx);
    printf("%d\n", rc);
    free(out); free(gx); free(gy); free(motion); free(sharp); free(x);
    return 0;
  }
  if (strcmp(argv[1], "resize") == 0) {
    if (argc < 11) return 2;
    const int B = atoi(argv[2]), Hs = atoi(argv[3]), Ws = atoi(argv[4]), op = atoi(argv[5]), y0 = atoi(argv[6]), x0 = atoi(argv[7]),
              h = atoi(argv[8]), w = atoi(argv[9]), n = atoi(argv[10]);
    if (n < 1 || n > 8 || argc != 11 + 5 * n) return 2;
    dptx_augment_task tasks[8] = {};
    size_t out_bytes[8];
    for (int i = 0; i < n; ++i) {
      char** a = argv + 11 + 5 * i;
      size_t ns = 0;
      tasks[i].src = slurp(a[0], &ns);
      tasks[i].C = atoi(a[1]);
      tasks[i].dtype = atoi(a[2]);
      tasks[i].interp = atoi(a[3]);
      const size_t el = tasks[i].dtype == DPTX_AUG_F32 ? 4 : 1;
      if (ns != (size_t)B * tasks[i].C * Hs * Ws * el) return 2;
      out_bytes[i] = (size_t)B * tasks[i].C * h * w * el;
      tasks[i].dst = malloc(out_bytes[i]);
      memset(tasks[i].dst, 0xFF, out_bytes[i]);
    }
    const int rc = dptx_augment_resize_tasks(tasks, n, B, Hs, Ws, op, y0, x0, h, w, nullptr);
    for (int i = 0; i < n; ++i) {
      dump(argv[11 + 5 * i + 4], tasks[i].dst, out_bytes[i]);
      free(tasks[i].dst);
      free((void*)tasks[i].src);
    }
    printf("%d\n", rc);
    return 0;
  }
  return 2;
}
