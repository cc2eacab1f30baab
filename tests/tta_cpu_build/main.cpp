// Runs dptx_tta_merge_normals of csrc/tta.hip, compiled for the host (hip/hip_runtime.h next to this file), on a case read from
// files: maps (fp32), views (dptx_tta_view[]), outs (dptx_image_desc[]); writes the packed output.  Every buffer is a heap block
// of exactly its size, so AddressSanitizer reports any access outside it.
//   main <maps> <views> <outs> <mode> <output bytes> <output file>
#include "../../omnidata_amd/csrc/tta.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<char> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> b(n);
  if (fread(b.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const std::vector<char> maps = slurp(argv[1]), views = slurp(argv[2]), outs = slurp(argv[3]);
  const int mode = atoi(argv[4]);
  const long nbytes = atol(argv[5]);
  std::vector<float> m(maps.size() / 4);
  memcpy(m.data(), maps.data(), m.size() * 4);
  std::vector<uint32_t> out((nbytes + 3) / 4, 0xA5A5A5A5u);
  const int rc = dptx_tta_merge_normals(m.data(), (const dptx_tta_view*)views.data(), (int)(views.size() / sizeof(dptx_tta_view)),
                                        (const dptx_image_desc*)outs.data(), (int)(outs.size() / sizeof(dptx_image_desc)), mode,
                                        out.data(), nullptr);
  FILE* f = fopen(argv[6], "wb");
  fwrite(out.data(), 1, nbytes, f);
  fclose(f);
  return rc == 0 ? 0 : 1;
}
