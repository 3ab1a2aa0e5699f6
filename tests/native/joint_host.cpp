// Host (CPU) build of the joint point pass (csrc/hsv_verify_hc.hpp: the 2-bit
// record format, joint_column, jt_build, straus_joint and the JOINT form of
// verify_one_prepped), for tests/test_joint_table.py.  Test infrastructure:
// the product library never runs this code on the CPU.
//
//   (no argument)   lines "pk_hex sig_hex msg_hex" -> the flag byte per line, through
//                   prep_scalars (2-bit columns) and the joint verify_one_prepped, or
//                   the full-length path for a fallback item ("fallback" on stderr);
//                   HSV_LAT_BITS sets the lattice bound
//   --inject MODE   the same with the table stores corrupted as the kernel's fault
//                   injection does: "fault" or the flag byte
//   --recode        lines "scalar_hex" (big-endian, < 2^138) -> the 70 digits, top first
//   --indexmap      the 32 rows "ci cj flip line neg" of joint_column
//   --table         lines "P_hex Q_hex" (compressed points) -> per line of the table
//                   "l i j ok x_hex y_hex": ok = the stored line equals iP + jQ by
//                   repeated ge_add_cached as affine points and its 2dT fits them
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "hsv_comb.hpp"
#include "hsv_lattice.hpp"
#include "hsv_verify_core.hpp"
#include "hsv_verify_hc.hpp"

using namespace hsv;

// the lane's slot: kJointLines lines; the full-length path's table 0 in lines 1 .. 8
struct HostJointTab {
  uint32_t e[kJointLines + 1][32];
  uint32_t inject = kInjectNone;
  HostJointTab() {
    memset(e, 0xa5, sizeof(e));  // a line read before it is written shows up
    cached_pack(ge_cached_identity(), e[0]);
  }
  void store(uint32_t l, const uint32_t w[32], bool flip) {
    if (l < 1 || l > (uint32_t)kJointLines) { fprintf(stderr, "line %u out of the slot\n", l); exit(3); }
    memcpy(e[l], w, 128);
    if (inject == kInjectZeroTables) memset(e[l], 0, 128);
    if (inject == kInjectFlipTables && flip) e[l][0] ^= 1u;
  }
  void load(uint32_t l, uint32_t w[32]) const {
    if (l > (uint32_t)kJointLines) { fprintf(stderr, "line %u out of the slot\n", l); exit(3); }
    memcpy(w, e[l], 128);
  }
  void put(int t, int m, const uint32_t w[32]) {
    if (t != 0 || m > 8) { fprintf(stderr, "table %d entry %d out of the slot\n", t, m); exit(3); }
    if (m) store((uint32_t)m, w, true);
  }
  void get(int t, uint32_t m, uint32_t w[32]) const {
    if (t != 0 || m > 8) { fprintf(stderr, "table %d entry %u out of the slot\n", t, m); exit(3); }
    load(m, w);
  }
  void put_line(uint32_t l, const uint32_t w[32]) { store(l, w, l >= kJointFirstLineOfR); }
  void get_line(uint32_t l, uint32_t w[32]) const { load(l, w); }
};

// wide comb table of B (16-bit digits, 48 MiB), built once on first use
static const uint32_t *comb16_b() {
  static std::vector<uint32_t> tab;
  if (tab.empty()) {
    tab.resize(kComb16TableWords);
    std::vector<uint32_t> tmp(kComb16Chunk * 8);
    const uint32_t bw[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                            0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    fe x, y;
    ge_decompress(bw, x, y);
    for (int j = 0; j < kComb16Pos; ++j)
      for (uint32_t c = 0; c < (uint32_t)kComb16ChunksPerPos; ++c) comb16_build_chunk(x, y, j, c, tab.data(), tmp.data());
  }
  return tab.data();
}

static bool parse_hex(const std::string &s, uint8_t *out, size_t n) {
  if (s.size() != 2 * n) return false;
  for (size_t i = 0; i < n; ++i) {
    unsigned v;
    if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

static void to_words(const uint8_t *b, uint32_t *w, int n) {
  for (int i = 0; i < n; ++i)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
}

static void print_fe(const fe &a) {
  uint32_t w[8];
  fe_pack(a, w);
  for (int i = 7; i >= 0; --i) printf("%08x", w[i]);
}

static const int g_lat_bits = getenv("HSV_LAT_BITS") ? atoi(getenv("HSV_LAT_BITS")) : kLatCombBits;

static ge_ext affine_ext(const fe &x, const fe &y) {
  ge_ext p;
  p.X = x;
  p.Y = y;
  p.Z = fe_small(1);
  p.T = fe_mul(x, y);
  return p;
}

int main(int argc, char **argv) {
  using G = HalfCombWindows<2>;
  if (argc > 1 && strcmp(argv[1], "--recode") == 0) {
    std::string hs;
    while (std::cin >> hs) {
      uint8_t be[20], le[20];
      if (!parse_hex(hs, be, 20)) { printf("ERR\n"); continue; }
      for (int i = 0; i < 20; ++i) le[i] = be[19 - i];
      uint32_t x[5], d[5];
      to_words(le, x, 5);
      recode_top5<2, G::NW>(x, d);
      for (int c = 0; c < G::NW; ++c) {  // as straus_joint reads them: the top chunk, then shift
        printf("%d%c", (int)(d[4] >> 30) - 2, c + 1 < G::NW ? ' ' : '\n');
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
          const uint32_t line = joint_column(ci, cj, flip, neg);
          printf("%u %u %u %u %u\n", ci, cj, flip, line, neg);
        }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--table") == 0) {
    std::string ps, qs;
    while (std::cin >> ps >> qs) {
      uint8_t pb[32], qb[32];
      uint32_t pw[8], qw[8];
      if (!parse_hex(ps, pb, 32) || !parse_hex(qs, qb, 32)) { printf("ERR\n"); continue; }
      to_words(pb, pw, 8);
      to_words(qb, qw, 8);
      fe xp, yp, xq, yq;
      if (!ge_decompress(pw, xp, yp) || !ge_decompress(qw, xq, yq)) { printf("ERR\n"); continue; }
      HostJointTab vt;
      jt_build(vt, xp, yp, xq, yq);
      const ge_cached cp = ge_to_cached(affine_ext(xp, yp)), cq = ge_to_cached(affine_ext(xq, yq));
      for (int i = 0; i <= 2; ++i)
        for (int j = -2; j <= 2; ++j) {
          uint32_t neg;
          const uint32_t l = joint_line(i, j, neg);
          if (neg || l == 0) continue;  // the folded half and the identity have no line
          ge_ext r = ge_identity();
          for (int k = 0; k < i; ++k) r = ge_add_cached<true>(r, cp);
          for (int k = 0; k < (j < 0 ? -j : j); ++k) r = ge_add_cached<true>(r, ge_cached_cneg(cq, j < 0));
          uint32_t w[32];
          vt.get_line(l, w);
          const ge_cached c = cached_unpack(w);
          // (Y+X) - (Y-X) = 2X, their sum 2Y, and 2Z: the same point projectively
          const fe X = fe_carry(fe_sub(c.YpX, fe_carry(c.YmX))), Y = fe_carry(fe_add(c.YpX, c.YmX)), Z = c.Z2;
          const uint32_t same = fe_eq(fe_mul(X, r.Z), fe_mul(r.X, Z)) & fe_eq(fe_mul(Y, r.Z), fe_mul(r.Y, Z)) &
                                (fe_is_zero(Z) ^ 1u);
          // 2dT 2Z = 4d XY = d (2X)(2Y)
          const uint32_t t_ok = fe_eq(fe_mul(c.T2d, Z), fe_mul(fe_mul(X, Y), fe_d()));
          const fe zi = fe_invert(Z);
          printf("%u %d %d %u ", l, i, j, same & t_ok);
          print_fe(fe_mul(X, zi));
          printf(" ");
          print_fe(fe_mul(Y, zi));
          printf("\n");
        }
    }
    return 0;
  }
  const uint32_t inject = (argc > 2 && strcmp(argv[1], "--inject") == 0) ? (uint32_t)atoi(argv[2]) : kInjectNone;
  std::string ps, ss, ms;
  while (std::cin >> ps >> ss >> ms) {
    uint8_t pk[32], sig[64], msg[32];
    if (!parse_hex(ps, pk, 32) || !parse_hex(ss, sig, 64) || !parse_hex(ms, msg, 32)) {
      printf("ERR\n");
      continue;
    }
    uint32_t pw[8], sw[16], mw[8], rec[kPrepWords];
    to_words(pk, pw, 8);
    to_words(sig, sw, 16);
    to_words(msg, mw, 8);
    HostJointTab vt;
    vt.inject = inject;
    uint32_t f;
    if (prep_scalars<4, PutPlain, 2>(pw, sw, mw, rec, 1, g_lat_bits)) {
      f = verify_one_full_comb<4, false, 16>(pw, sw, mw, comb16_b(), vt);
      fprintf(stderr, "fallback\n");
    } else {
      f = verify_one_prepped<4, 16, true>(pw, sw, rec, 1, rec[18], comb16_b(), vt);
    }
    if (f & kFault) printf("fault\n");
    else printf("%02x\n", f & 0xffu);
  }
  return 0;
}
