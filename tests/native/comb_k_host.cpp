// Host (CPU) check of the k-taking comb core (verify_one_comb_k,
// csrc/hsv_comb.hpp): the core the comb pass of hsv_committee_verify_msgs*
// runs with k = SHA-512(R || A || M) mod l read from the route kernel's record.
// Test infrastructure, built under AddressSanitizer + UBSan by
// tests/test_comb_k_host.py; the product never runs this code on the CPU.
//
// stdin:  nkeys, then nkeys lines "pk_hex";
//         then lines "key_index sig_hex msg_hex flags_hex" (msg_hex "-" = empty).
// For every item: k is hashed here over the whole message (msg_hash,
// csrc/hsv_msghash.hpp), verify_one_comb_k's byte must equal flags_hex (the
// Python oracle's), and for a 32-byte message also verify_one_comb's byte.
// Prints "comb k host ok <items> <of them 32-byte>" and exits 0, or says
// which item failed and exits 1.
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

int main() {
  size_t nkeys = 0;
  if (!(std::cin >> nkeys) || nkeys == 0 || nkeys > 16) return 2;
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
    uint8_t b[32];
    if (!(std::cin >> hs) || !parse_hex(hs, b, 32)) return 2;
    to_words(b, &pkw[8 * k], 8);
    kflags[k] = build(&pkw[8 * k], 1, tables.data() + k * kCombTableWords);
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
    memcpy(head, sw, 32);               // R
    memcpy(head + 8, &pkw[8 * idx], 32);  // A
    const uint64_t q_last = len ? (len - 1) >> 4 : 0;
    auto ld = [&](uint64_t q, uint32_t w[4]) {
      if (len == 0 || q > q_last) { fprintf(stderr, "load outside the message's chunks\n"); exit(3); }
      memcpy(w, msg.data() + 16 * q, 16);
    };
    msg_hash(ld, head, 0, len, hw);
    const sc k = sc_reduce512(hw);
    const uint32_t *ta = tables.data() + idx * kCombTableWords;
    const uint32_t f = verify_one_comb_k(kflags[idx], sw, k, ta, btab.data());
    if ((f & kFault) || (f & 0xffu) != want) {
      printf("item %zu (len %zu): verify_one_comb_k %03x, oracle %02x\n", items, len, f, want);
      return 1;
    }
    if (len == 32) {
      uint32_t mw[8];
      to_words(msg.data(), mw, 8);
      const uint32_t g = verify_one_comb(&pkw[8 * idx], kflags[idx], sw, mw, ta, btab.data());
      if (g != f) {
        printf("item %zu: verify_one_comb %03x, verify_one_comb_k %03x\n", items, g, f);
        return 1;
      }
      ++short32;
    }
    ++items;
  }
  printf("comb k host ok %zu %zu\n", items, short32);
  return 0;
}
