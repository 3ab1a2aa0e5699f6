// Host (CPU) check of what hsv_committee_verify_msgs_indexed* computes per
// item: k = SHA-512(R || member key || M) mod l by the head_*<64> block
// arithmetic (head_msg_hash<64>, csrc/hsv_msghash.hpp -- the arithmetic
// msg_hash_wave<64> runs on the device with the head gathered through the key
// index), fed to the k-taking comb cores of both table widths
// (verify_one_comb_k, verify_one_comb4_k, csrc/hsv_comb.hpp).
// Test infrastructure, built under AddressSanitizer + UBSan by
// tests/test_committee_msgs_indexed_host.py; the product never runs this code
// on the CPU.
//
// stdin:  nkeys, then nkeys lines "pk_hex";
//         then lines "key_index sig_hex msg_hex flags_hex" (msg_hex "-" = empty).
// For every item the message is hashed at byte shifts 0, 1, 7 and 15 of its
// buffer (which ends flush with the message's last 16-byte chunk: a read past
// it is a heap overflow); the four digests must be equal and equal to
// msg_hash's, and both cores' bytes must equal flags_hex (the Python oracle's).
// Prints "cmsg indexed host ok <items>" and exits 0, or says which item failed
// and exits 1.
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
  std::vector<uint32_t> tables(nkeys * kCombTableWords), tables4(nkeys * kComb4TableWords);
  std::vector<uint32_t> btab(kCombTableWords), tmp(kCombEnt * 8);
  static_assert(kComb4GroupEnt * 8 <= kCombEnt * 8, "one scratch serves both builders");
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
  // the wide comb of B, chunk by chunk as the scalars ask for them (tests/native/comb4_host.cpp)
  std::vector<uint32_t> btab16(kComb16TableWords), tmp16(kComb16Chunk * 8);
  std::vector<bool> have16(kComb16Pos * kComb16ChunksPerPos, false);
  fe b16x, b16y;
  if (!ge_decompress(bw, b16x, b16y)) return 2;
  auto need16 = [&](const uint32_t s[8]) {
    uint32_t sr[9];
    recode_add<9, 16, kComb16Pos>(s, 8, sr);
    for (int j = 0; j < kComb16Pos; ++j) {
      const int32_t d = (int32_t)((sr[j >> 1] >> (16 * (j & 1))) & 0xffffu) - (1 << 15);
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d), c = mag ? (mag - 1) / kComb16Chunk : 0;
      if (have16[j * kComb16ChunksPerPos + c]) continue;
      comb16_build_chunk(b16x, b16y, j, c, btab16.data(), tmp16.data());
      have16[j * kComb16ChunksPerPos + c] = true;
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
  size_t idx, items = 0;
  std::string ss, ms, fs;
  while (std::cin >> idx >> ss >> ms >> fs) {
    if (idx >= nkeys) return 2;
    const size_t len = ms == "-" ? 0 : ms.size() / 2;
    uint8_t sig[64];
    std::vector<uint8_t> plain(len ? len : 1);
    if (!parse_hex(ss, sig, 64) || (len && !parse_hex(ms, plain.data(), len))) return 2;
    const unsigned want = (unsigned)strtoul(fs.c_str(), nullptr, 16);
    uint32_t sw[16], head[16], hw[16], hw0[16];
    to_words(sig, sw, 16);
    memcpy(head, sw, 32);                 // R
    memcpy(head + 8, &pkw[8 * idx], 32);  // the member's key, through its index
    for (const size_t shift : {(size_t)0, (size_t)1, (size_t)7, (size_t)15}) {
      std::vector<uint8_t> msg((shift + len + 15) & ~size_t(15));
      if (len) memcpy(msg.data() + shift, plain.data(), len);
      const uint64_t q_last = len ? (shift + len - 1) >> 4 : 0;
      auto ld = [&](uint64_t q, uint32_t w[4]) {
        if (len == 0 || q > q_last) { fprintf(stderr, "load outside the message's chunks\n"); exit(3); }
        memcpy(w, msg.data() + 16 * q, 16);
      };
      head_msg_hash<64>(ld, head, shift, len, hw);
      if (shift == 0) {
        memcpy(hw0, hw, sizeof hw0);
        uint32_t ref[16];
        msg_hash(ld, head, 0, len, ref);
        if (memcmp(ref, hw, sizeof ref) != 0) {
          printf("item %zu (len %zu): head_msg_hash<64> differs from msg_hash\n", items, len);
          return 1;
        }
      } else if (memcmp(hw0, hw, sizeof hw0) != 0) {
        printf("item %zu (len %zu): the digest at shift %zu differs\n", items, len, shift);
        return 1;
      }
    }
    const sc k = sc_reduce512(hw);
    need16(sw + 8);
    const uint32_t f8 = verify_one_comb_k(kflags[idx], sw, k, tables.data() + idx * kCombTableWords, btab.data());
    const uint32_t f4 = verify_one_comb4_k(kflags[idx], sw, k, tables4.data() + idx * kComb4TableWords, btab16.data());
    if ((f4 & kFault) || (f4 & 0xffu) != want || (f8 & kFault) || (f8 & 0xffu) != want) {
      printf("item %zu (key %zu, len %zu): verify_one_comb_k %03x, verify_one_comb4_k %03x, oracle %02x\n", items, idx,
             len, f8, f4, want);
      return 1;
    }
    ++items;
  }
  printf("cmsg indexed host ok %zu\n", items);
  return 0;
}
