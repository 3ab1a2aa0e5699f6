// Host (CPU) build of the kernel's per-lane verification core, for unit tests
// in this GPU-less container.  This is test infrastructure: the product
// library never runs this code on the CPU.
//
// Reads lines "pk_hex sig_hex msg_hex" (32/64/32 bytes) on stdin and prints
// the flag byte per line in hex.  With "--selftest-field" it instead prints
// field/scalar/SHA results for random-ish inputs so Python can compare.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <string>
#include <iostream>

#include "hsv_comb.hpp"
#include "hsv_lattice.hpp"
#include "hsv_verify_core.hpp"
#include "hsv_verify_hc.hpp"
#include "hsv_txhash.hpp"
#include <vector>

using namespace hsv;

static const uint32_t kBTable[256 * 24] = {
#include "hsv_btable.inc"
};
static const uint32_t kBTable133[256 * 24] = {
#include "hsv_btable133.inc"
};
static const uint32_t kBTable134[256 * 24] = {
#include "hsv_btable134.inc"
};

struct HostBTab {
  const uint32_t *tab = kBTable;
  ge_niels load(uint32_t idx) const {
    const uint32_t *e = tab + 24 * idx;
    ge_niels n;
    n.ypx = fe_from_words_masked(e);
    n.ymx = fe_from_words_masked(e + 8);
    n.xy2d = fe_from_words_masked(e + 16);
    return n;
  }
};

// per-lane variable-base tables (the kernel keeps them in a global-memory slot)
// inject: the kernel's fault injection (GlobalVarTab::put, hsv_pointpass.hpp)
struct HostVarTab {
  uint32_t e[2][17][32];
  uint32_t inject = kInjectNone;
  void put(int t, int m, const uint32_t w[32]) {
    memcpy(e[t][m], w, 128);
    if (m == 0) return;
    if (inject == kInjectZeroTables) memset(e[t][m], 0, 128);
    if (inject == kInjectFlipTables && t == 0) e[t][m][0] ^= 1u;
  }
  void get(int t, uint32_t m, uint32_t w[32]) const { memcpy(w, e[t][m], 128); }
};

// comb table of B (hsv_comb.hpp), built once on first use
static const uint32_t *comb_b() {
  static std::vector<uint32_t> tab;
  if (tab.empty()) {
    tab.resize(kCombTableWords);
    std::vector<uint32_t> tmp(kCombEnt * 8);
    const uint32_t bw[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                            0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    fe x, y;
    ge_decompress(bw, x, y);
    for (int j = 0; j < kCombPos; ++j)
      comb_build_position(comb_position_base(x, y, 0, j), tab.data() + (uint64_t)j * kCombEnt * kCombEntryWords,
                          tmp.data());
  }
  return tab.data();
}

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
      for (uint32_t c = 0; c < (uint32_t)kComb16ChunksPerPos; ++c)
        comb16_build_chunk(x, y, j, c, tab.data(), tmp.data());
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

// Lattice bound of the comb paths (variants 16-21): HSV_LAT_BITS, default
// kLatCombBits; the fallback fixtures are built for 133.
static const int g_lat_bits = getenv("HSV_LAT_BITS") ? atoi(getenv("HSV_LAT_BITS")) : kLatCombBits;

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "--field") == 0) {
    // lines: op a_hex b_hex (big-endian hex of 256-bit values)
    std::string op, as, bs;
    while (std::cin >> op >> as >> bs) {
      uint8_t ab[32], bb[32];
      // big-endian hex -> little-endian bytes
      uint8_t tmp[32];
      parse_hex(as, tmp, 32);
      for (int i = 0; i < 32; ++i) ab[i] = tmp[31 - i];
      parse_hex(bs, tmp, 32);
      for (int i = 0; i < 32; ++i) bb[i] = tmp[31 - i];
      uint32_t aw[8], bw[8];
      to_words(ab, aw, 8);
      to_words(bb, bw, 8);
      const fe a = fe_from_words_masked(aw), b = fe_from_words_masked(bw);
      fe r;
      if (op == "mul") r = fe_mul(a, b);
      else if (op == "sq") r = fe_sq(a);
      else if (op == "add") r = fe_add(a, b);
      else if (op == "sub") r = fe_sub(a, b);
      else if (op == "inv") r = fe_invert(a);
      else if (op == "pow") r = fe_pow22523(a);
      else r = fe_canon(a);
      print_fe(r);
      printf("\n");
    }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--hashk") == 0) {
    // lines: R A M hex -> k (big-endian hex)
    std::string rs, as, ms;
    while (std::cin >> rs >> as >> ms) {
      uint8_t r[32], a[32], m[32];
      parse_hex(rs, r, 32);
      parse_hex(as, a, 32);
      parse_hex(ms, m, 32);
      uint32_t rw[8], aw[8], mw[8], h[16];
      to_words(r, rw, 8);
      to_words(a, aw, 8);
      to_words(m, mw, 8);
      sha512_96(rw, aw, mw, h);
      uint32_t hc[16];  // the one-body form of the latency kernels must agree
      sha512_96<true>(rw, aw, mw, hc);
      if (memcmp(h, hc, sizeof(h)) != 0) { fprintf(stderr, "sha512_compress_compact differs\n"); exit(4); }
      sc k = sc_reduce512(h);
      for (int i = 7; i >= 0; --i) printf("%08x", k.v[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--txrec") == 0) {
    // lines: shift tx_hex -> 128-byte record pk||sig||SHA-512(message)[..32] (hex)
    // The transaction is placed at byte `shift` of a 16-aligned buffer whose
    // other bytes are 0xa5, so realignment errors and stray reads show up.
    std::string shs, txs;
    while (std::cin >> shs >> txs) {
      const size_t sh = (size_t)atoi(shs.c_str()), len = txs.size() / 2;
      std::vector<uint32_t> buf((sh + len + 64) / 4 + 8, 0xa5a5a5a5u);
      uint8_t *bytes = reinterpret_cast<uint8_t *>(buf.data());
      parse_hex(txs, bytes + sh, len);
      const uint64_t q_last = (sh + len - 1) >> 4;
      auto ld = [&](uint64_t k, uint32_t w[4]) {
        if (k > q_last) { fprintf(stderr, "load past the transaction\n"); exit(3); }
        memcpy(w, bytes + 16 * k, 16);
      };
      uint32_t rec[32];
      tx_record(ld, sh, len, rec);
      for (int i = 0; i < 32; ++i)
        for (int b = 0; b < 4; ++b) printf("%02x", (rec[i] >> (8 * b)) & 0xffu);
      printf("\n");
    }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--degenerate") == 0) {
    // the (0 : 0 : 0 : 0) accumulator (zeroed table memory) against the final
    // checks: "neutral eq_affine" must print "0 0"; the neutral point "1 ..."
    ge_ext z;
    z.X = fe_small(0);
    z.Y = fe_small(0);
    z.Z = fe_small(0);
    z.T = fe_small(0);
    const ge_ext o = ge_identity();
    const fe x = fe_small(0), y = fe_small(1);
    printf("%u %u %u %u\n", ge_is_neutral(z), ge_eq_affine(z, x, y), ge_is_neutral(o), ge_eq_affine(o, x, y));
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--sanity") == 0) {
    // ge_is_sane (the device self-check) on: the identity, (0 : 0 : 0 : 0),
    // B, B with X + 1, [2^10]B, and (X : Y : 0 : T) of B
    const uint32_t bw[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                            0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    fe x, y;
    ge_decompress(bw, x, y);
    ge_ext b;
    b.X = x;
    b.Y = y;
    b.Z = fe_small(1);
    b.T = fe_mul(x, y);
    ge_ext z;
    z.X = z.Y = z.Z = z.T = fe_small(0);
    ge_ext bx = b;
    bx.X = fe_carry(fe_add(b.X, fe_small(1)));
    ge_ext b10 = b;
    for (int i = 0; i < 10; ++i) b10 = ge_dbl<true>(b10);
    ge_ext bz = b;
    bz.Z = fe_small(0);
    printf("%u %u %u %u %u %u\n", ge_is_sane(ge_identity()), ge_is_sane(z), ge_is_sane(b), ge_is_sane(bx),
           ge_is_sane(b10), ge_is_sane(bz));
    return 0;
  }
  if (argc > 2 && strcmp(argv[1], "--inject") == 0) {
    // the two-pass form (variant 21) with the table stores corrupted as the
    // kernel's fault injection does; per record: "fault" or the flag byte
    const uint32_t mode = (uint32_t)atoi(argv[2]);
    std::string ps, ss, ms;
    while (std::cin >> ps >> ss >> ms) {
      uint8_t pk[32], sig[64], msg[32];
      parse_hex(ps, pk, 32);
      parse_hex(ss, sig, 64);
      parse_hex(ms, msg, 32);
      uint32_t pw[8], sw[16], mw[8], rec[kPrepWords];
      to_words(pk, pw, 8);
      to_words(sig, sw, 16);
      to_words(msg, mw, 8);
      HostVarTab vt;
      vt.inject = mode;
      const uint32_t f = prep_scalars<4>(pw, sw, mw, rec, 1, g_lat_bits)
                             ? verify_one_full_comb<4, true, 16>(pw, sw, mw, comb16_b(), vt)
                             : verify_one_prepped<4, 16>(pw, sw, rec, 1, rec[18], comb16_b(), vt);
      if (f & kFault) printf("fault\n");
      else printf("%02x\n", f & 0xffu);
    }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--lattice") == 0) {
    // lines: k (big-endian hex, < l) -> "ok c0_neg c0 c1" (hex, big-endian);
    // optional argv[2]: the bound in bits (default kLatMaxBits)
    std::string ks;
    while (std::cin >> ks) {
      uint8_t kb[32], tmp[32];
      parse_hex(ks, tmp, 32);
      for (int i = 0; i < 32; ++i) kb[i] = tmp[31 - i];
      sc k;
      to_words(kb, k.v, 8);
      const LatOut o = lattice_reduce(k, argc > 2 ? atoi(argv[2]) : kLatMaxBits);
      printf("%u %u ", o.ok, o.c0_neg);
      for (int i = 4; i >= 0; --i) printf("%08x", o.c0[i]);
      printf(" ");
      for (int i = 4; i >= 0; --i) printf("%08x", o.c1[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc > 1 && strcmp(argv[1], "--comb") == 0) {
    // line 1: nkeys; then nkeys pk hex lines; then "idx sig_hex msg_hex" lines;
    // optional argv[2]: fault injection mode (niels_injected on the first key entry)
    const uint32_t inject = argc > 2 ? (uint32_t)atoi(argv[2]) : kInjectNone;
    size_t nkeys = 0;
    std::cin >> nkeys;
    std::vector<uint32_t> pkw(8 * nkeys), kflags(nkeys);
    std::vector<uint32_t> tables(nkeys * kCombTableWords), btab(kCombTableWords), tmp(kCombEnt * 8);
    auto build = [&](const uint32_t enc[8], uint32_t neg, uint32_t *tab) -> uint32_t {
      fe x, y;
      const uint32_t ok = ge_decompress(enc, x, y);
      for (int j = 0; j < kCombPos; ++j)
        comb_build_position(comb_position_base(x, y, neg, j), tab + (uint64_t)j * kCombEnt * kCombEntryWords,
                            tmp.data());
      return (ok ? kKeyAOk : 0u) | (ok && y_is_small_order(y) ? kKeySmallA : 0u);
    };
    const uint32_t bw[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                            0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    build(bw, 0, btab.data());
    for (size_t k = 0; k < nkeys; ++k) {
      std::string hs;
      std::cin >> hs;
      uint8_t b[32];
      parse_hex(hs, b, 32);
      to_words(b, &pkw[8 * k], 8);
      kflags[k] = build(&pkw[8 * k], 1, tables.data() + k * kCombTableWords);
    }
    size_t idx;
    std::string ss, ms;
    while (std::cin >> idx >> ss >> ms) {
      uint8_t sig[64], msg[32];
      parse_hex(ss, sig, 64);
      parse_hex(ms, msg, 32);
      uint32_t sw[16], mw[8];
      to_words(sig, sw, 16);
      to_words(msg, mw, 8);
      const uint32_t f = verify_one_comb(&pkw[8 * idx], kflags[idx], sw, mw, tables.data() + idx * kCombTableWords,
                                         btab.data(), inject);
      if (f & kFault) printf("fault\n");
      else printf("%02x\n", f & 0xffu);
    }
    return 0;
  }
  HostBTab bt;
  int variant = (argc > 2 && strcmp(argv[1], "--variant") == 0) ? atoi(argv[2]) : 1;
  std::string ps, ss, ms;
  while (std::cin >> ps >> ss >> ms) {
    uint8_t pk[32], sig[64], msg[32];
    if (!parse_hex(ps, pk, 32) || !parse_hex(ss, sig, 64) || !parse_hex(ms, msg, 32)) {
      printf("ERR\n");
      continue;
    }
    uint32_t pw[8], sw[16], mw[8];
    to_words(pk, pw, 8);
    to_words(sig, sw, 16);
    to_words(msg, mw, 8);
    uint32_t f;
    switch (variant) {
      case 0: f = verify_one<2, 8>(pw, sw, mw, bt); break;
      case 2: f = verify_one<4, 8>(pw, sw, mw, bt); break;
      case 4: f = verify_one<3, 6>(pw, sw, mw, bt); break;
      case 10:
      case 11: {
        bool fb = false;
        HostBTab b2;
        b2.tab = variant == 10 ? kBTable133 : kBTable134;
        f = variant == 10 ? verify_one_half<3, 9>(pw, sw, mw, bt, b2, fb) : verify_one_half<2, 8>(pw, sw, mw, bt, b2, fb);
        if (fb) f = verify_one<3, 9>(pw, sw, mw, bt) | 0x100u;  // mark fallback for the test
        break;
      }
      case 12:
      case 13: {
        bool fb = false;
        HostBTab b2;
        HostVarTab vt;
        b2.tab = variant == 12 ? kBTable133 : kBTable134;
        f = variant == 12 ? verify_one_half_mt<3, 9>(pw, sw, mw, bt, b2, vt, fb)
                          : verify_one_half_mt<2, 8>(pw, sw, mw, bt, b2, vt, fb);
        if (fb) f = verify_one_mt<3, 9>(pw, sw, mw, bt, vt) | 0x100u;
        break;
      }
      case 14: {
        HostVarTab vt;
        f = verify_one_mt<3, 9>(pw, sw, mw, bt, vt);
        break;
      }
      case 15: {
        HostVarTab vt;
        f = verify_one_mt<4, 8>(pw, sw, mw, bt, vt);
        break;
      }
      case 16:
      case 17:
      case 19: {
        bool fb = false;
        HostVarTab vt;
        f = variant == 16 ? verify_one_half_comb<3>(pw, sw, mw, comb_b(), vt, fb, g_lat_bits)
          : variant == 17 ? verify_one_half_comb<4>(pw, sw, mw, comb_b(), vt, fb, g_lat_bits)
                          : verify_one_half_comb<5>(pw, sw, mw, comb_b(), vt, fb, g_lat_bits);
        if (fb) f = verify_one_full_comb<3>(pw, sw, mw, comb_b(), vt) | 0x100u;
        break;
      }
      case 20: {
        bool fb = false;
        HostVarTab vt;
        f = verify_one_half_comb<4, true, 16>(pw, sw, mw, comb16_b(), vt, fb, g_lat_bits);
        if (fb) f = verify_one_full_comb<4, true, 16>(pw, sw, mw, comb16_b(), vt) | 0x100u;
        break;
      }
      case 18: {
        HostVarTab vt;
        f = verify_one_full_comb<3>(pw, sw, mw, comb_b(), vt);
        break;
      }
      case 21: {  // two-pass form (GPU variants 19/20): scalar prepass record, then the point pass
        HostVarTab vt;
        uint32_t rec[kPrepWords];
        if (prep_scalars<4>(pw, sw, mw, rec, 1, g_lat_bits))
          f = verify_one_full_comb<4, true, 16>(pw, sw, mw, comb16_b(), vt) | 0x100u;
        else
          f = verify_one_prepped<4, 16>(pw, sw, rec, 1, rec[18], comb16_b(), vt);
        break;
      }
      default: f = verify_one<3, 9>(pw, sw, mw, bt); break;
    }
    // a device self-check failure on the host has no excuse: it prints a
    // token the tests cannot parse as flags
    if (f & kFault) printf("fault\n");
    else printf("%02x\n", f & 0xffu);
    if (f & 0x100u) fprintf(stderr, "fallback\n");
  }
  return 0;
}
