// Host check of the census table's insert step (csrc/hsv_census.hpp): the
// function the lanes of hsv_census_count_kernel run per distinct key, here with
// threads in the place of lanes.  Built with -fsanitize=address,undefined by
// tests/test_census_host.py and run directly.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <thread>
#include <vector>

#include "hsv_census.hpp"

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

using Key = std::vector<uint8_t>;
using Census = std::map<Key, uint64_t>;

// the input: n keys of 32 bytes, as the key form of the kernel reads them
struct Items {
  const uint8_t *pks;
  void load(uint32_t j, uint32_t w[8]) const { std::memcpy(w, pks + 32 * (size_t)j, 32); }
};

std::vector<uint8_t> random_keys(size_t n, uint32_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<uint8_t> k(32 * n);
  for (auto &b : k) b = (uint8_t)rng();
  return k;
}

struct Table {
  std::vector<uint32_t> tab, counts;
  uint64_t overflow = 0, claimed = 0;
  explicit Table(uint32_t slots) : tab(slots, 0u), counts(slots, 0u) {}
};

// items [lo, hi) of pks, each once (count 1), into t; returns {overflowed items, claimed slots}
void insert_range(Table &t, const std::vector<uint8_t> &pks, size_t lo, size_t hi, uint64_t seed, uint64_t *overflow,
                  uint64_t *claimed) {
  const Items in{pks.data()};
  uint64_t o = 0, c = 0;
  for (size_t i = lo; i < hi; ++i) {
    uint32_t w[8];
    std::memcpy(w, &pks[32 * i], 32);
    const uint32_t r = hsv::census_insert(t.tab.data(), t.counts.data(), (uint32_t)t.tab.size() - 1u, seed, in,
                                          (uint32_t)i, w, 1u, true);
    o += r == hsv::kCensusOverflow;
    c += r == hsv::kCensusClaimed;
  }
  *overflow = o;
  *claimed = c;
}

Census expected(const std::vector<uint8_t> &pks, size_t n) {
  Census c;
  for (size_t i = 0; i < n; ++i) ++c[Key(&pks[32 * i], &pks[32 * i] + 32)];
  return c;
}

// what the table holds: claimer's key -> count; checks every slot's claimer is in range
Census recorded(const Table &t, const std::vector<uint8_t> &pks, size_t n, const char *what) {
  Census c;
  for (size_t s = 0; s < t.tab.size(); ++s) {
    const uint32_t e = t.tab[s];
    if (e == 0u) {
      CHECK(t.counts[s] == 0u, "%s: empty slot %zu has count %u", what, s, t.counts[s]);
      continue;
    }
    CHECK(e <= n, "%s: slot %zu claimed by item %u of %zu", what, s, e - 1u, n);
    if (e > n) continue;
    const Key k(&pks[32 * (size_t)(e - 1u)], &pks[32 * (size_t)(e - 1u)] + 32);
    CHECK(c.find(k) == c.end(), "%s: a key holds two slots", what);
    c[k] = t.counts[s];
  }
  return c;
}

// a table with room: everything recorded, exactly
void check_exact(const std::vector<uint8_t> &pks, size_t n, uint32_t slots, uint64_t seed, const char *what) {
  Table t(slots);
  uint64_t o = 0, c = 0;
  insert_range(t, pks, 0, n, seed, &o, &c);
  const Census want = expected(pks, n), got = recorded(t, pks, n, what);
  CHECK(o == 0, "%s: %llu items overflowed", what, (unsigned long long)o);
  CHECK(c == want.size(), "%s: %llu slots claimed for %zu distinct keys", what, (unsigned long long)c, want.size());
  CHECK(got == want, "%s: the census differs (n = %zu, slots = %u)", what, n, slots);
}

}  // namespace

int main() {
  const uint64_t seed_a = 0x9e3779b97f4a7c15ull, seed_b = 0x0123456789abcdefull;
  CHECK(hsv::census_slots_ok(16) && hsv::census_slots_ok(1u << 22) && !hsv::census_slots_ok(0) &&
            !hsv::census_slots_ok(15) && !hsv::census_slots_ok(24) && !hsv::census_slots_ok(1u << 23),
        "census_slots_ok");
  // 0, 1, 15, 16, 17 and 1000 distinct keys, each once, then with duplicates
  for (size_t n : {0u, 1u, 15u, 16u, 17u, 1000u}) {
    std::vector<uint8_t> pks = random_keys(n, (uint32_t)n + 1);
    uint32_t slots = 16;
    while (slots < 4 * n) slots <<= 1;
    check_exact(pks, n, slots, seed_a, "distinct keys");
    check_exact(pks, n, slots, seed_b, "distinct keys, second seed");
    // duplicates: every third key repeats an earlier one; and the whole batch twice over
    for (size_t i = 3; i < n; i += 3) std::memcpy(&pks[32 * i], &pks[32 * (i / 2)], 32);
    check_exact(pks, n, slots, seed_a, "duplicated keys");
    std::vector<uint8_t> twice = pks;
    twice.insert(twice.end(), pks.begin(), pks.end());
    check_exact(twice, 2 * n, slots, seed_a, "the batch twice");
    // one-bit neighbours in bytes 0, 7, 8 and 31 are keys of their own
    if (n && n <= 17) {
      std::vector<uint8_t> nb = pks;
      for (size_t i = 0; i < n; ++i)
        for (int byte : {0, 7, 8, 31}) {
          uint8_t k[32];
          std::memcpy(k, &pks[32 * i], 32);
          k[byte] ^= (uint8_t)(1u << (i % 8));
          nb.insert(nb.end(), k, k + 32);
        }
      check_exact(nb, nb.size() / 32, 512, seed_a, "one-bit neighbours");
    }
  }
  // a group's population count goes in with one insert
  {
    const std::vector<uint8_t> pks = random_keys(2, 5);
    Table t(16);
    const Items in{pks.data()};
    uint32_t w[8];
    std::memcpy(w, &pks[32], 32);
    CHECK(hsv::census_insert(t.tab.data(), t.counts.data(), 15u, seed_a, in, 1u, w, 40u, true) == hsv::kCensusClaimed,
          "first insert does not claim");
    CHECK(hsv::census_insert(t.tab.data(), t.counts.data(), 15u, seed_a, in, 1u, w, 24u, true) == hsv::kCensusMatched,
          "second insert does not match");
    // a caller with nothing to insert changes nothing
    CHECK(hsv::census_insert(t.tab.data(), t.counts.data(), 15u, seed_a, in, 1u, w, 7u, false) == hsv::kCensusIdle,
          "an idle caller is not idle");
    const Census got = recorded(t, pks, 2, "group counts");
    CHECK(got.size() == 1 && got.begin()->second == 64u, "group counts: not 64");
  }
  // a cluster that wraps past the end of a 16-slot table: 8 keys, found by
  // search, whose home slot is 13, under two seeds
  for (uint64_t seed : {seed_a, seed_b}) {
    std::mt19937_64 rng(7);
    std::vector<uint8_t> pks;
    while (pks.size() < 8 * 32) {
      uint8_t k[32];
      uint32_t w[8];
      for (auto &b : k) b = (uint8_t)rng();
      std::memcpy(w, k, 32);
      if ((hsv::keytab_hash(seed, w) & 15u) == 13u) pks.insert(pks.end(), k, k + 32);
    }
    std::vector<uint8_t> thrice;
    for (int r = 0; r < 3; ++r) thrice.insert(thrice.end(), pks.begin(), pks.end());
    Table t(16);
    uint64_t o = 0, c = 0;
    insert_range(t, thrice, 0, 24, seed, &o, &c);
    CHECK(o == 0 && c == 8, "wrapped cluster: overflow %llu, claimed %llu", (unsigned long long)o,
          (unsigned long long)c);
    for (int k = 0; k < 8; ++k) {
      const size_t s = (13 + k) & 15;
      CHECK(t.tab[s] == (uint32_t)k + 1u && t.counts[s] == 3u, "wrapped cluster: slot %zu holds item %u, count %u", s,
            t.tab[s] - 1u, t.counts[s]);
    }
    CHECK(recorded(t, thrice, 24, "wrapped cluster") == expected(thrice, 24), "wrapped cluster: census differs");
  }
  // a full table: 16 slots, 1000 distinct keys, each twice.  Every recorded
  // count is exact, the overflow is the rest, and every walk ends within the
  // bound (the call returns; a walk past min(slots, 256) slots would have to
  // wrap around a table that never empties)
  {
    const std::vector<uint8_t> once = random_keys(1000, 77);
    std::vector<uint8_t> pks = once;
    pks.insert(pks.end(), once.begin(), once.end());
    Table t(16);
    uint64_t o = 0, c = 0;
    insert_range(t, pks, 0, 2000, seed_a, &o, &c);
    const Census got = recorded(t, pks, 2000, "full table");
    CHECK(c == 16 && got.size() == 16, "full table: %llu slots claimed", (unsigned long long)c);
    uint64_t counted = 0;
    for (const auto &kv : got) {
      CHECK(kv.second == 2u, "full table: a recorded key has count %llu", (unsigned long long)kv.second);
      counted += kv.second;
    }
    CHECK(counted + o == 2000, "full table: counted %llu + overflow %llu != 2000", (unsigned long long)counted,
          (unsigned long long)o);
  }
  // the bound itself: 512 slots, the first 300 filled by hand with one foreign
  // key; a key whose home is slot 0 walks 256 of them and gives up although
  // slot 300 is empty, one whose home is slot 100 reaches it
  {
    std::mt19937_64 rng(11);
    std::vector<uint8_t> pks = random_keys(1, 3);  // item 0: the squatter
    uint32_t home[2] = {0u, 100u};
    for (uint32_t h : home)
      for (;;) {
        uint8_t k[32];
        uint32_t w[8];
        for (auto &b : k) b = (uint8_t)rng();
        std::memcpy(w, k, 32);
        if ((hsv::keytab_hash(seed_a, w) & 511u) == h) {
          pks.insert(pks.end(), k, k + 32);
          break;
        }
      }
    Table t(512);
    for (int s = 0; s < 300; ++s) t.tab[s] = 1u;
    const Items in{pks.data()};
    uint32_t w[8];
    std::memcpy(w, &pks[32], 32);
    CHECK(hsv::census_insert(t.tab.data(), t.counts.data(), 511u, seed_a, in, 1u, w, 1u, true) == hsv::kCensusOverflow,
          "a walk of more than 256 slots was not given up");
    std::memcpy(w, &pks[64], 32);
    CHECK(hsv::census_insert(t.tab.data(), t.counts.data(), 511u, seed_a, in, 2u, w, 1u, true) == hsv::kCensusClaimed &&
              t.tab[300] == 3u && t.counts[300] == 1u,
          "a walk of 201 slots did not reach the empty one");
  }
  // the same items from 8 threads at once: the same multiset out
  for (uint32_t slots : {4096u, 16u}) {
    const size_t distinct = slots == 16u ? 12 : 700, n = 8 * 1500;
    const std::vector<uint8_t> base = random_keys(distinct, 123);
    std::vector<uint8_t> pks(32 * n);
    std::mt19937 rng(9);
    for (size_t i = 0; i < n; ++i) std::memcpy(&pks[32 * i], &base[32 * (rng() % distinct)], 32);
    Table t(slots);
    uint64_t o[8], c[8];
    std::vector<std::thread> th;
    for (int k = 0; k < 8; ++k)
      th.emplace_back([&, k] { insert_range(t, pks, n * k / 8, n * (k + 1) / 8, seed_a, &o[k], &c[k]); });
    for (auto &x : th) x.join();
    uint64_t os = 0, cs = 0;
    for (int k = 0; k < 8; ++k) os += o[k], cs += c[k];
    const Census want = expected(pks, n);
    CHECK(os == 0 && cs == want.size(), "8 threads, %u slots: overflow %llu, claimed %llu of %zu", slots,
          (unsigned long long)os, (unsigned long long)cs, want.size());
    CHECK(recorded(t, pks, n, "8 threads") == want, "8 threads, %u slots: the census differs", slots);
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("census host ok\n");
  return 0;
}
