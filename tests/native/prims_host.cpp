// Host (CPU) build of csrc/hsv_test_prims.hpp: the same dispatch text the
// device kernels of csrc/hsv_test_prims.hip run, so tests/test_prims_host.py
// pins the plain C++ branches of the field, scalar and lattice headers (built
// with -DHSV_CHECK_BOUNDS) and tests/test_prims_gpu.py has the host's lattice
// answers to compare the device's with.  Test infrastructure only.
//
//   prims_host --field  [file]    records of 24 words in, 24 words out
//   prims_host --scalar [file]    records of 32 words in, 16 words out
// Records are raw little-endian 32-bit words, read from the file or stdin and
// written to stdout (csrc/hsv_test_prims.hpp has the layout).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hsv_test_prims.hpp"

using namespace hsv;

int main(int argc, char **argv) {
  if (argc < 2 || argc > 3 || (std::strcmp(argv[1], "--field") != 0 && std::strcmp(argv[1], "--scalar") != 0)) {
    std::fprintf(stderr, "usage: prims_host --field|--scalar [file]\n");
    return 2;
  }
  const bool field = std::strcmp(argv[1], "--field") == 0;
  const size_t win = field ? kPrimFieldIn : kPrimScalarIn, wout = field ? kPrimFieldOut : kPrimScalarOut;
  FILE *f = argc == 3 ? std::fopen(argv[2], "rb") : stdin;
  if (!f) {
    std::perror(argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  uint32_t buf[4096];
  size_t got;
  while ((got = std::fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
  if (f != stdin) std::fclose(f);
  if (in.size() % win != 0) {
    std::fprintf(stderr, "prims_host: input is not a whole number of %zu-word records\n", win);
    return 2;
  }
  const size_t n = in.size() / win;
  std::vector<uint32_t> out(n * wout, 0u);
  for (size_t i = 0; i < n; ++i) {
    if (field)
      prim_field_op(&in[i * win], (uint32_t)i, &out[i * wout]);
    else
      prim_scalar_op(&in[i * win], &out[i * wout]);
  }
  if (n && std::fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 1;
  return 0;
}
