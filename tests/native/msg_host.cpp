// Host (CPU) build of the any-length message hash of the verifier
// (csrc/hsv_msghash.hpp, the header hsv_msg_prep_kernel is built from) and of
// the split scalar prepass (csrc/hsv_verify_hc.hpp, prep_from_hash).  Test
// infrastructure: the product library never runs this code on the CPU.
//
//   --hash   lines "shift head_hex msg_hex" (head = R || A, 64 bytes; msg "-"
//            when empty) -> SHA-512(head || msg) as 128 hex digits.  The
//            message sits at byte `shift` of a 16-byte-aligned buffer whose
//            other bytes are 0xa5; the chunk loader aborts when it is asked for
//            a chunk outside [first byte's chunk, last byte's chunk], or at all
//            for an empty message.
//   --prep BITS   lines "pk_hex sig_hex msg_hex" (32 / 64 / 32 bytes) ->
//            "fb_unsplit fb_split fb_krec fb_void meta_void rec_unsplit
//            rec_split rec_krec k": the fallback answers and the kPrepWords
//            record words (hex) of prep_scalars, of prep_from_hash on the same
//            hash, and of its KREC form (and that form's answer and meta word
//            for an item marked void), and k mod l (8 words), at the lattice
//            bound BITS.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <iostream>
#include <string>
#include <vector>

#include "hsv_msghash.hpp"
#include "hsv_verify_hc.hpp"

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

static void print_words(const uint32_t *w, int n) {
  for (int i = 0; i < n; ++i) printf("%08x", w[i]);
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "--hash") == 0) {
    std::string shs, hs, ms;
    while (std::cin >> shs >> hs >> ms) {
      const size_t sh = (size_t)atoi(shs.c_str()), len = ms == "-" ? 0 : ms.size() / 2;
      uint8_t head[64];
      if (!parse_hex(hs, head, 64)) return 2;
      uint32_t hw[16];
      to_words(head, hw, 16);
      // the message ends flush with the buffer: a read past its last chunk is a heap overflow
      const size_t cap = len ? ((sh + len + 15) & ~size_t(15)) : 16;
      uint8_t *bytes = static_cast<uint8_t *>(aligned_alloc(16, cap));
      memset(bytes, 0xa5, cap);
      if (len && !parse_hex(ms, bytes + sh, len)) return 2;
      const uint64_t q_first = sh >> 4, q_last = len ? (sh + len - 1) >> 4 : 0;
      auto ld = [&](uint64_t k, uint32_t w[4]) {
        if (len == 0) { fprintf(stderr, "load for an empty message\n"); exit(3); }
        if (k < q_first || k > q_last) { fprintf(stderr, "load outside the message's chunks\n"); exit(3); }
        memcpy(w, bytes + 16 * k, 16);
      };
      uint32_t out[16];
      // an empty message may point one past an allocation: give it an address no load may touch
      msg_hash(ld, hw, len ? sh : (uint64_t)cap + sh, len, out);
      for (int i = 0; i < 16; ++i)
        for (int b = 0; b < 4; ++b) printf("%02x", (out[i] >> (8 * b)) & 0xffu);
      printf("\n");
      free(bytes);
    }
    return 0;
  }
  if (argc > 2 && strcmp(argv[1], "--prep") == 0) {
    const int bits = atoi(argv[2]);
    std::string ps, ss, ms;
    while (std::cin >> ps >> ss >> ms) {
      uint8_t pk[32], sig[64], msg[32];
      if (!parse_hex(ps, pk, 32) || !parse_hex(ss, sig, 64) || !parse_hex(ms, msg, 32)) return 2;
      uint32_t pw[8], sw[16], mw[8], h[16];
      to_words(pk, pw, 8);
      to_words(sig, sw, 16);
      to_words(msg, mw, 8);
      uint32_t r0[kPrepWords], r1[kPrepWords], r2[kPrepWords];
      const bool f0 = prep_scalars<4>(pw, sw, mw, r0, 1, bits);
      sha512_96(sw, pw, mw, h);
      const bool f1 = prep_from_hash<4>(h, sw + 8, r1, 1, bits);
      const bool f2 = prep_from_hash<4, PutPlain, true>(h, sw + 8, r2, 1, bits);
      uint32_t r3[kPrepWords];
      const bool f3 = prep_from_hash<4, PutPlain, true>(h, sw + 8, r3, 1, bits, true);  // a void item
      const sc k = sc_reduce512(h);
      printf("%d %d %d %d %08x ", (int)f0, (int)f1, (int)f2, (int)f3, r3[kPrepWords - 1]);
      print_words(r0, kPrepWords);
      printf(" ");
      print_words(r1, kPrepWords);
      printf(" ");
      print_words(r2, kPrepWords);
      printf(" ");
      print_words(k.v, 8);
      printf("\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: msg_host --hash | --prep BITS\n");
  return 2;
}
