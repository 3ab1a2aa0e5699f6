// Host (CPU) build of the point pass's 2-bit column format with digits in
// {-1 .. 2} (csrc/hsv_verify_hc.hpp: recode_cols, joint_column<kColOffset>,
// col_class), for tests/test_cols_host.py.  Test infrastructure: the product
// library never runs this code on the CPU.
//
//   --recode     lines "scalar_hex" (big-endian, 40 digits, < 2^138) -> the 70 digits,
//                top first, as straus_joint reads them
//   --indexmap   the 32 rows "ci cj flip line neg" of joint_column<kColOffset>
//   --class      lines "c0_hex c1_hex" -> col_class(c0, c1)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "hsv_lattice.hpp"
#include "hsv_verify_core.hpp"
#include "hsv_verify_hc.hpp"

using namespace hsv;

static bool parse_scalar(const std::string &s, uint32_t x[5]) {
  if (s.size() != 40) return false;
  for (int i = 0; i < 5; ++i) {
    unsigned v;
    if (sscanf(s.substr(8 * (4 - i), 8).c_str(), "%8x", &v) != 1) return false;
    x[i] = v;
  }
  return true;
}

int main(int argc, char **argv) {
  using G = HalfCombWindows<2>;
  if (argc > 1 && strcmp(argv[1], "--recode") == 0) {
    std::string hs;
    while (std::cin >> hs) {
      uint32_t x[5], d[5];
      if (!parse_scalar(hs, x)) { printf("ERR\n"); continue; }
      recode_cols<G::NW>(x, d);
      for (int c = 0; c < G::NW; ++c) {
        printf("%d%c", (int)(d[4] >> 30) - kColOffset, c + 1 < G::NW ? ' ' : '\n');
        limbs_shl<5>(d, 2);
      }
    }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--indexmap") == 0) {
    for (uint32_t flip = 0; flip < 2; ++flip)
      for (uint32_t ci = 0; ci < 4; ++ci)
        for (uint32_t cj = 0; cj < 4; ++cj) {
          uint32_t neg = 7;
          const uint32_t line = joint_column<kColOffset>(ci, cj, flip, neg);
          printf("%u %u %u %u %u\n", ci, cj, flip, line, neg);
        }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--class") == 0) {
    std::string a, b;
    while (std::cin >> a >> b) {
      uint32_t c0[5], c1[5];
      if (!parse_scalar(a, c0) || !parse_scalar(b, c1)) { printf("ERR\n"); continue; }
      printf("%u\n", col_class(c0, c1));
    }
    return 0;
  }
  fprintf(stderr, "usage: cols_host --recode | --indexmap | --class\n");
  return 2;
}
