// Host (CPU) check of the compact comb core (verify_one_comb4_k,
// verify_one_comb4 and the builder comb4_build_group, csrc/hsv_comb.hpp): the
// 4-bit digit tables of hsv_committee_create_ex(..., 4, ...).  Test
// infrastructure, built under AddressSanitizer + UBSan by
// tests/test_comb4_host.py; the product never runs this code on the CPU.
//
// stdin:  nkeys, then nkeys lines "pk_hex";
//         then lines "key_index sig_hex msg_hex flags_hex" (msg_hex "-" = empty).
// Both tables of every key are built here, and both combs of B: the 8-bit one
// verify_one_comb_k reads and the wide 16-bit one the compact core reads.  For
// every item k is hashed over the whole message (msg_hash,
// csrc/hsv_msghash.hpp); verify_one_comb4_k's and verify_one_comb_k's bytes
// must equal flags_hex (the Python oracle's), and for a 32-byte message also
// verify_one_comb4's.
// Then crafted challenges against key 0, fed straight to verify_one_comb4_k:
// k = 0, 1, 7, 8, 9, l - 1, and three k whose recoded nibbles at positions
// 0..62 are all 0x0 (digit -8), all 0xF (digit +7), or alternate between the
// two, each kept below l by its top nibble.  For each, R = [s]B - [k]A comes
// from plain double-and-add (hsv_point.hpp), independent of both combs: the
// flags must carry EQ_OK, and must not with one bit of s flipped.
// The compact table's entries are also compared with the full table's: T4[2i][m]
// and T4[2i+1][m] are T[i][m] and T[i][16m], byte for byte.
// Prints "comb4 host ok <items> <of them 32-byte> <crafted k> <crafted checks>
// <entries compared>" and exits 0, or says what failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "hsv_comb.hpp"
#include "hsv_msghash.hpp"

using namespace hsv;

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

static ge_ext affine_point(const fe &x, const fe &y) {
  ge_ext p;
  p.X = x;
  p.Y = y;
  p.Z = fe_small(1);
  p.T = fe_mul(x, y);
  return p;
}

// [k]P by double-and-add over the 256 bits of k
static ge_ext scalar_mult(const ge_ext &p, const uint32_t k[8]) {
  const ge_cached pc = ge_to_cached(p);
  ge_ext r = ge_identity();
  for (int b = 255; b >= 0; --b) {
    r = ge_dbl<true>(r);
    if ((k[b >> 5] >> (b & 31)) & 1u) r = ge_add_cached<true>(r, pc);
  }
  return r;
}

// x -= y over 8 words; returns the borrow
static uint32_t sub8(uint32_t x[8], const uint32_t y[8]) {
  uint64_t borrow = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t t = (uint64_t)x[i] - y[i] - borrow;
    x[i] = (uint32_t)t;
    borrow = (t >> 32) & 1u;
  }
  return (uint32_t)borrow;
}

// k whose recoded nibble at position j < 63 is lo (j even) or hi (j odd), with
// top nibble `top`: k = that value - C4
static bool pattern_k(uint32_t lo, uint32_t hi, uint32_t top, uint32_t k[8]) {
  uint32_t c4[8];
  for (int i = 0; i < 8; ++i) {
    k[i] = 0;
    c4[i] = 0x88888888u;
  }
  for (int j = 0; j < kComb4Pos; ++j) {
    const uint32_t nib = j == kComb4Pos - 1 ? top : ((j & 1) ? hi : lo);
    k[j >> 3] |= nib << (4 * (j & 7));
  }
  if (sub8(k, c4)) return false;
  if (!sc_is_canonical(k)) return false;
  // the recoding must give the pattern back
  uint32_t kr[9];
  recode_add<9, 4, kComb4Pos>(k, 8, kr);
  if (kr[8] != 0) return false;
  for (int j = 0; j < kComb4Pos; ++j) {
    const uint32_t nib = (kr[j >> 3] >> (4 * (j & 7))) & 0xfu;
    if (nib != (j == kComb4Pos - 1 ? top : ((j & 1) ? hi : lo))) return false;
  }
  return true;
}

int main() {
  size_t nkeys = 0;
  if (!(std::cin >> nkeys) || nkeys == 0 || nkeys > 16) return 2;
  std::vector<uint32_t> pkw(8 * nkeys), kflags(nkeys);
  std::vector<uint32_t> tables(nkeys * kCombTableWords), tables4(nkeys * kComb4TableWords);
  std::vector<uint32_t> btab(kCombTableWords), tmp(kCombEnt * 8);
  static_assert(kComb4GroupEnt * 8 <= kCombEnt * 8, "one scratch serves both builders");
  static_assert(kComb4TableWords == 12288, "48 KiB per key");
  auto build = [&](const uint32_t enc[8], uint32_t neg, uint32_t *tab) -> uint32_t {
    fe x, y;
    const uint32_t ok = ge_decompress(enc, x, y);
    for (int j = 0; j < kCombPos; ++j)
      comb_build_position(comb_position_base(x, y, neg, j), tab + (uint64_t)j * kCombEnt * kCombEntryWords,
                          tmp.data());
    return (ok ? kKeyAOk : 0u) | (ok && y_is_small_order(y) ? kKeySmallA : 0u);
  };
  auto build4 = [&](const uint32_t enc[8], uint32_t neg, uint32_t *tab) {
    fe x, y;
    (void)ge_decompress(enc, x, y);
    for (int g = 0; g < kComb4Groups; ++g) comb4_build_group(x, y, neg, g, tab, tmp.data());
  };
  const uint32_t bw[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                          0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
  build(bw, 0, btab.data());
  // The wide comb of B, built chunk by chunk (128 entries, the build kernel's
  // unit) as the scalars ask for them: all 4096 chunks would take most of the
  // run.  An entry of a chunk that was not built reads as zeros, which is no
  // curve point: the self-check bit of the flags would say so.
  std::vector<uint32_t> btab16(kComb16TableWords), tmp16(kComb16Chunk * 8);
  std::vector<bool> have16(kComb16Pos * kComb16ChunksPerPos, false);
  fe b16x, b16y;
  if (!ge_decompress(bw, b16x, b16y)) return 2;
  size_t chunks16 = 0;
  auto need16 = [&](const uint32_t s[8]) {
    uint32_t sr[9];
    recode_add<9, 16, kComb16Pos>(s, 8, sr);
    for (int j = 0; j < kComb16Pos; ++j) {
      const int32_t d = (int32_t)((sr[j >> 1] >> (16 * (j & 1))) & 0xffffu) - (1 << 15);
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d), c = mag ? (mag - 1) / kComb16Chunk : 0;
      if (have16[j * kComb16ChunksPerPos + c]) continue;
      comb16_build_chunk(b16x, b16y, j, c, btab16.data(), tmp16.data());
      have16[j * kComb16ChunksPerPos + c] = true;
      ++chunks16;
    }
  };
  for (size_t k = 0; k < nkeys; ++k) {
    std::string hs;
    uint8_t b[32];
    if (!(std::cin >> hs) || !parse_hex(hs, b, 32)) return 2;
    to_words(b, &pkw[8 * k], 8);
    kflags[k] = build(&pkw[8 * k], 1, tables.data() + k * kCombTableWords);
    build4(&pkw[8 * k], 1, tables4.data() + k * kComb4TableWords);
  }
  // the compact table's entries are entries of the full one: T4[2i][m] = T[i][m]
  // and T4[2i+1][m] = T[i][16m], byte for byte (both canonical affine Niels)
  size_t shared = 0;
  for (size_t k = 0; k < nkeys; ++k) {
    if (!(kflags[k] & kKeyAOk)) continue;
    for (int i = 0; i < kCombPos; ++i)
      for (int m = 1; m <= kComb4Ent; ++m) {
        const uint32_t *full = tables.data() + k * kCombTableWords + (uint64_t)i * kCombEnt * kCombEntryWords;
        const uint32_t *c4 = tables4.data() + k * kComb4TableWords + (uint64_t)(2 * i) * kComb4Ent * kCombEntryWords;
        if (memcmp(c4 + (m - 1) * kCombEntryWords, full + (m - 1) * kCombEntryWords, 96) != 0 ||
            memcmp(c4 + (kComb4Ent + m - 1) * kCombEntryWords, full + (16 * m - 1) * kCombEntryWords, 96) != 0) {
          printf("key %zu: compact entries of byte position %d, multiple %d differ from the full table's\n", k, i, m);
          return 1;
        }
        shared += 2;
      }
  }
  size_t idx, items = 0, short32 = 0;
  std::string ss, ms, fs;
  while (std::cin >> idx >> ss >> ms >> fs) {
    if (idx >= nkeys) return 2;
    const size_t len = ms == "-" ? 0 : ms.size() / 2;
    uint8_t sig[64];
    // the message ends flush with its buffer: a read past its last chunk is a heap overflow
    std::vector<uint8_t> msg((len + 15) & ~size_t(15));
    if (!parse_hex(ss, sig, 64) || (len && !parse_hex(ms, msg.data(), len))) return 2;
    const unsigned want = (unsigned)strtoul(fs.c_str(), nullptr, 16);
    uint32_t sw[16], head[16], hw[16];
    to_words(sig, sw, 16);
    memcpy(head, sw, 32);                 // R
    memcpy(head + 8, &pkw[8 * idx], 32);  // A
    const uint64_t q_last = len ? (len - 1) >> 4 : 0;
    auto ld = [&](uint64_t q, uint32_t w[4]) {
      if (len == 0 || q > q_last) { fprintf(stderr, "load outside the message's chunks\n"); exit(3); }
      memcpy(w, msg.data() + 16 * q, 16);
    };
    msg_hash(ld, head, 0, len, hw);
    const sc k = sc_reduce512(hw);
    const uint32_t *ta = tables.data() + idx * kCombTableWords;
    const uint32_t *ta4 = tables4.data() + idx * kComb4TableWords;
    need16(sw + 8);
    const uint32_t f4 = verify_one_comb4_k(kflags[idx], sw, k, ta4, btab16.data());
    const uint32_t f8 = verify_one_comb_k(kflags[idx], sw, k, ta, btab.data());
    if ((f4 & kFault) || (f4 & 0xffu) != want || (f8 & kFault) || (f8 & 0xffu) != want) {
      printf("item %zu (len %zu): verify_one_comb4_k %03x, verify_one_comb_k %03x, oracle %02x\n", items, len, f4, f8,
             want);
      return 1;
    }
    if (len == 32) {
      uint32_t mw[8];
      to_words(msg.data(), mw, 8);
      const uint32_t g = verify_one_comb4(&pkw[8 * idx], kflags[idx], sw, mw, ta4, btab16.data());
      if ((g & kFault) || (g & 0xffu) != want) {
        printf("item %zu: verify_one_comb4 %03x, oracle %02x\n", items, g, want);
        return 1;
      }
      ++short32;
    }
    ++items;
  }

  // crafted challenges against key 0 (an honest key)
  if (!(kflags[0] & kKeyAOk) || (kflags[0] & kKeySmallA)) return 2;
  std::vector<sc> ks;
  for (uint32_t small : {0u, 1u, 7u, 8u, 9u}) {
    sc k{};
    k.v[0] = small;
    ks.push_back(k);
  }
  {
    sc k{};
    sc_l(k.v);
    k.v[0] -= 1u;  // l is odd: no borrow
    ks.push_back(k);
  }
  const uint32_t pat[3][3] = {{0x0u, 0x0u, 9u}, {0xfu, 0xfu, 8u}, {0x0u, 0xfu, 9u}};  // lo, hi, top nibble
  for (const auto &p : pat) {
    sc k{};
    if (!pattern_k(p[0], p[1], p[2], k.v)) {
      printf("pattern %x/%x top %x: not a canonical k with those nibbles\n", p[0], p[1], p[2]);
      return 1;
    }
    ks.push_back(k);
  }
  fe ax, ay, bx, by;
  if (!ge_decompress(&pkw[0], ax, ay) || !ge_decompress(bw, bx, by)) return 2;
  const ge_ext neg_a = affine_point(fe_carry(fe_neg(ax)), ay), bpt = affine_point(bx, by);
  size_t crafted = 0, checks = 0;
  for (const sc &k : ks) {
    uint32_t sw[16];
    for (int i = 0; i < 8; ++i) sw[8 + i] = 0x01234567u * (uint32_t)(i + 1) + (uint32_t)crafted;
    sw[15] &= 0x03ffffffu;  // s < 2^250 < l, and stays so with bit 40 flipped
    const ge_ext r = ge_add_cached<true>(scalar_mult(bpt, sw + 8), ge_to_cached(scalar_mult(neg_a, k.v)));
    ge_compress(r, sw);
    need16(sw + 8);
    const uint32_t good = verify_one_comb4_k(kflags[0], sw, k, tables4.data(), btab16.data());
    if ((good & kFault) || !(good & kEqOk) || !(good & kStrictOk)) {
      printf("crafted k %zu: R = [s]B - [k]A gives %03x, want EQ_OK\n", crafted, good);
      return 1;
    }
    sw[9] ^= 1u << 8;  // bit 40 of s
    need16(sw + 8);
    const uint32_t bad = verify_one_comb4_k(kflags[0], sw, k, tables4.data(), btab16.data());
    if ((bad & kFault) || (bad & kEqOk) || !(bad & kSOk)) {
      printf("crafted k %zu: a flipped s bit gives %03x, want no EQ_OK\n", crafted, bad);
      return 1;
    }
    checks += 2;
    ++crafted;
  }
  if (chunks16 < 16) return 2;  // every position of B was read
  printf("comb4 host ok %zu %zu %zu %zu %zu\n", items, short32, crafted, checks, shared);
  return 0;
}
