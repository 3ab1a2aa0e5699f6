// Host check of the device key table (csrc/hsv_keytab.hpp): the builder and
// keytab_find, the function the route kernel of
// hsv_committee_verify_transactions* runs per transaction.  Built with
// -fsanitize=address,undefined by tests/test_keytab_host.py and run directly.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hsv_keytab.hpp"

namespace {

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

uint32_t find(const std::vector<uint32_t> &tab, uint64_t seed, const std::vector<uint8_t> &pks, const uint8_t *key) {
  uint32_t w[8];
  std::memcpy(w, key, 32);
  return hsv::keytab_find(tab.data(), (uint32_t)tab.size() - 1u, seed, pks.data(), w);
}

std::vector<uint8_t> random_keys(size_t n, uint32_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<uint8_t> k(32 * n);
  for (auto &b : k) b = (uint8_t)rng();
  return k;
}

// the first index holding the same 32 bytes as key i
size_t first_index(const std::vector<uint8_t> &pks, size_t i) {
  for (size_t j = 0; j < i; ++j)
    if (std::memcmp(&pks[32 * j], &pks[32 * i], 32) == 0) return j;
  return i;
}

// every member at its first index, its one-bit neighbours miss
void check_table(const std::vector<uint8_t> &pks, size_t n, uint64_t seed, const char *what) {
  const std::vector<uint32_t> tab = hsv::keytab_build(pks.data(), n, seed);
  const size_t cap = tab.size();
  CHECK(cap >= 2 && (cap & (cap - 1)) == 0 && cap >= 2 * n, "%s: capacity %zu for %zu keys", what, cap, n);
  size_t used = 0;
  for (uint32_t e : tab) {
    CHECK(e <= n, "%s: slot %u out of range", what, e);
    used += e != 0;
  }
  CHECK(used <= n, "%s: %zu slots used by %zu keys", what, used, n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t got = find(tab, seed, pks, &pks[32 * i]);
    CHECK(got == first_index(pks, i), "%s: key %zu found at %u, first index %zu", what, i, got, first_index(pks, i));
    for (int byte : {0, 7, 8, 31}) {
      uint8_t k[32];
      std::memcpy(k, &pks[32 * i], 32);
      k[byte] ^= (uint8_t)(1u << (i % 8));
      bool member = false;  // (a random neighbour is a member with probability 2^-240)
      for (size_t j = 0; j < n; ++j) member |= std::memcmp(&pks[32 * j], k, 32) == 0;
      if (!member)
        CHECK(find(tab, seed, pks, k) == hsv::kKeytabMiss, "%s: key %zu with byte %d changed was found", what, i, byte);
    }
  }
  const std::vector<uint8_t> others = random_keys(16, 0xabcdu);
  for (size_t i = 0; i < 16; ++i)
    CHECK(find(tab, seed, pks, &others[32 * i]) == hsv::kKeytabMiss, "%s: a stranger was found", what);
}

}  // namespace

int main() {
  const uint64_t seed_a = 0x9e3779b97f4a7c15ull, seed_b = 0x0123456789abcdefull;
  for (size_t n : {0u, 1u, 31u, 32u, 33u, 1000u}) {
    std::vector<uint8_t> pks = random_keys(n, (uint32_t)n + 1);
    check_table(pks, n, seed_a, "distinct keys");
    // duplicates: every third key repeats an earlier one
    for (size_t i = 3; i < n; i += 3) std::memcpy(&pks[32 * i], &pks[32 * (i / 2)], 32);
    check_table(pks, n, seed_a, "duplicated keys");
    // two seeds: two layouts, identical answers
    const std::vector<uint32_t> ta = hsv::keytab_build(pks.data(), n, seed_a), tb = hsv::keytab_build(pks.data(), n, seed_b);
    if (n >= 31) CHECK(ta != tb, "n = %zu: the seed does not move the layout", n);
    for (size_t i = 0; i < n; ++i)
      CHECK(find(ta, seed_a, pks, &pks[32 * i]) == find(tb, seed_b, pks, &pks[32 * i]), "n = %zu: seeds disagree on key %zu",
            n, i);
  }
  // a cluster: twenty keys, found by search, that all hash to the last slot of
  // a 64-slot table, so the run of occupied slots wraps past the table's end
  {
    std::mt19937_64 rng(7);
    std::vector<uint8_t> pks;
    while (pks.size() < 20 * 32) {
      uint8_t k[32];
      uint32_t w[8];
      for (auto &b : k) b = (uint8_t)rng();
      std::memcpy(w, k, 32);
      if ((hsv::keytab_hash(seed_a, w) & 63u) == 63u) pks.insert(pks.end(), k, k + 32);
    }
    const std::vector<uint32_t> tab = hsv::keytab_build(pks.data(), 20, seed_a);
    CHECK(tab.size() == 64, "20 keys: %zu slots", tab.size());
    CHECK(tab[63] == 1u, "the first key is not in its home slot");
    for (int s = 0; s < 19; ++s) CHECK(tab[s] == (uint32_t)s + 2u, "slot %d holds %u: the cluster did not wrap", s, tab[s]);
    check_table(pks, 20, seed_a, "wrapped cluster");
    // a stranger with the same home slot walks the whole cluster and misses
    for (int found = 0; found < 4;) {
      uint8_t k[32];
      uint32_t w[8];
      for (auto &b : k) b = (uint8_t)rng();
      std::memcpy(w, k, 32);
      if ((hsv::keytab_hash(seed_a, w) & 63u) != 63u) continue;
      CHECK(find(tab, seed_a, pks, k) == hsv::kKeytabMiss, "a stranger in the cluster was found");
      ++found;
    }
  }
  // a table without an empty slot (never built by keytab_build) still ends
  {
    const std::vector<uint8_t> pks = random_keys(4, 99);
    const std::vector<uint32_t> full = {1u, 2u, 3u, 4u};
    const std::vector<uint8_t> other = random_keys(1, 100);
    CHECK(find(full, seed_a, pks, other.data()) == hsv::kKeytabMiss, "a full table: a stranger was found");
    CHECK(find(full, seed_a, pks, &pks[64]) == 2u, "a full table: member 2 not found");
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("keytab host ok\n");
  return 0;
}
