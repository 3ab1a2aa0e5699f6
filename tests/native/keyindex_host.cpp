// Host check of the host key index (csrc/hsv_keyindex.hpp): KeyIndex, which
// the QC paths probe with attacker-chosen key bytes, and KeyHash against the
// device table's mix (hsv::keytab_hash).  Every answer is compared with a
// brute-force scan of the key list.  Built with -fsanitize=address,undefined
// by tests/test_keyindex_host.py and run directly.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hsv_keyindex.hpp"

namespace {

using hsvh::Key32;
using hsvh::KeyHash;
using hsvh::KeyIndex;
using hsvh::key_of;

int g_failed = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
      ++g_failed;                                        \
    }                                                    \
  } while (0)

std::vector<uint8_t> random_keys(size_t n, uint32_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<uint8_t> k(32 * n);
  for (auto &b : k) b = (uint8_t)rng();
  return k;
}

// the first index among pks[0 .. 32 n) holding `key`, or -1
int64_t scan(const std::vector<uint8_t> &pks, size_t n, const uint8_t *key) {
  for (size_t j = 0; j < n; ++j)
    if (std::memcmp(&pks[32 * j], key, 32) == 0) return (int64_t)j;
  return -1;
}

KeyIndex index_of(const std::vector<uint8_t> &pks, size_t n) {
  KeyIndex ix;
  for (size_t i = 0; i < n; ++i) ix.emplace(key_of(&pks[32 * i]), (uint32_t)i);
  return ix;
}

// every member at its first index; its one-bit neighbours in bytes 0 and 7
// (the 8-byte tag changes) and 8 and 31 (the tag stays: the full compare
// decides) and strangers answer as the scan does
void check_index(const std::vector<uint8_t> &pks, size_t n, const char *what) {
  const KeyIndex ix = index_of(pks, n);
  size_t distinct = 0;
  for (size_t i = 0; i < n; ++i) distinct += scan(pks, n, &pks[32 * i]) == (int64_t)i;
  CHECK(ix.size() == distinct, "%s: %zu keys, size %zu, %zu distinct", what, n, ix.size(), distinct);
  for (size_t i = 0; i < n; ++i) {
    const int64_t got = ix.find(&pks[32 * i]), want = scan(pks, n, &pks[32 * i]);
    CHECK(got == want, "%s: key %zu found at %lld, first index %lld", what, i, (long long)got, (long long)want);
    for (int byte : {0, 7, 8, 31}) {
      uint8_t k[32];
      std::memcpy(k, &pks[32 * i], 32);
      k[byte] ^= (uint8_t)(1u << (i % 8));
      const int64_t g = ix.find(k), w = scan(pks, n, k);  // (-1, but for a 2^-240 chance)
      CHECK(g == w, "%s: key %zu with byte %d changed: %lld, scan %lld", what, i, byte, (long long)g, (long long)w);
    }
  }
  const std::vector<uint8_t> others = random_keys(16, 0xabcdu);
  for (size_t i = 0; i < 16; ++i)
    CHECK(ix.find(&others[32 * i]) == scan(pks, n, &others[32 * i]), "%s: a stranger was found", what);
}

}  // namespace

int main() {
  {
    const KeyIndex empty;
    const std::vector<uint8_t> k = random_keys(1, 5);
    CHECK(empty.find(k.data()) == -1 && empty.size() == 0, "an empty index answers");
  }
  // 64 slots hold 32 keys: 33 grows once, 1000 five times, 4097 eight times
  for (size_t n : {0u, 1u, 31u, 32u, 33u, 1000u, 4097u}) {
    std::vector<uint8_t> pks = random_keys(n, (uint32_t)n + 1);
    check_index(pks, n, "distinct keys");
    // duplicates: every third key repeats an earlier one
    for (size_t i = 3; i < n; i += 3) std::memcpy(&pks[32 * i], &pks[32 * (i / 2)], 32);
    check_index(pks, n, "duplicated keys");
  }
  // A copy, then different keys into the original and into the copy (a cache
  // view starts from its base's index): each answers for its own keys only.
  for (size_t n : {0u, 31u, 32u, 1000u}) {
    const std::vector<uint8_t> base = random_keys(n, 11), more_a = random_keys(40, 12), more_b = random_keys(40, 13);
    KeyIndex a = index_of(base, n);
    KeyIndex b = a;
    std::vector<uint8_t> all_a = base, all_b = base;
    all_a.insert(all_a.end(), more_a.begin(), more_a.end());
    all_b.insert(all_b.end(), more_b.begin(), more_b.end());
    for (size_t i = 0; i < 40; ++i) {
      a.emplace(key_of(&more_a[32 * i]), (uint32_t)(n + i));
      b.emplace(key_of(&more_b[32 * i]), (uint32_t)(n + i));
    }
    CHECK(a.size() == n + 40 && b.size() == n + 40, "copy of %zu keys: sizes %zu and %zu", n, a.size(), b.size());
    for (const std::vector<uint8_t> *q : {&all_a, &all_b})
      for (size_t i = 0; i < n + 40; ++i) {
        const uint8_t *k = &(*q)[32 * i];
        CHECK(a.find(k) == scan(all_a, n + 40, k), "copy of %zu keys: the original is wrong on key %zu", n, i);
        CHECK(b.find(k) == scan(all_b, n + 40, k), "copy of %zu keys: the copy is wrong on key %zu", n, i);
      }
  }
  // one mix: KeyHash is the device table's keytab_hash under KeyHash's seed
  {
    const std::vector<uint8_t> keys = random_keys(1000, 21);
    for (size_t i = 0; i < 1000; ++i) {
      uint32_t w[8];
      for (int j = 0; j < 8; ++j) {  // the key's eight little-endian words
        const uint8_t *p = &keys[32 * i + 4 * j];
        w[j] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
      }
      const Key32 k = key_of(&keys[32 * i]);
      CHECK((uint64_t)KeyHash()(k) == hsv::keytab_hash(KeyHash::seed(), w), "KeyHash differs from keytab_hash on key %zu", i);
    }
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("keyindex host ok\n");
  return 0;
}
