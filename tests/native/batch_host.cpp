// Host (CPU) check of csrc/hsv_batch.hpp -- the chunk walk, chunk geometry and
// length validation the staged host calls share -- against a brute-force walk
// written here.  Test infrastructure; plain g++, no HIP.
//
//   --walk      ragged batches with random lengths (0 included, one item far
//               above the others), fixed-stride batches (len <= stride) and
//               stride 0, each at item caps 1, 3, n and byte caps 1, one item's
//               size, several items' sizes: the chunks partition [0, n) in
//               order; no chunk exceeds a cap unless it is a single item; every
//               chunk is maximal; relative offsets run from 0 to the span.
//   --validate  first_bad_item on decreasing offsets and too-short items.
// Prints "ok <checks>"; the first failed check is printed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>

#include "hsv_batch.hpp"

using hsvh::BatchSpan;

static long g_checks = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    ++g_checks;                                  \
    if (!(cond)) {                               \
      fprintf(stderr, "FAILED %s: ", #cond);     \
      fprintf(stderr, __VA_ARGS__);              \
      fprintf(stderr, "\n");                     \
      exit(1);                                   \
    }                                            \
  } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd(uint64_t below) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (g_rng >> 33) % below;
}

// bytes item i counts for against the byte cap, and where it sits: the
// brute-force description of a batch, built without the header
struct Items {
  std::vector<uint64_t> start, cost, len;
};

static void walk(const BatchSpan &s, const Items &it, size_t max_items, size_t max_bytes) {
  const size_t n = it.start.size();
  // brute force: grow every chunk one item at a time by summed cost
  std::vector<size_t> want;
  for (size_t a = 0; a < n;) {
    size_t b = a + 1;
    uint64_t sum = it.cost[a];
    while (b < n && b - a < max_items && sum + it.cost[b] <= max_bytes) sum += it.cost[b++];
    want.push_back(b);
    a = b;
  }
  size_t a = 0, ci = 0;
  std::vector<uint64_t> rel;
  while (a < n) {
    const size_t b = s.chunk_end(a, n, max_items, max_bytes);
    CHECK(b > a && b <= n, "chunk [%zu, %zu) of %zu", a, b, n);
    CHECK(ci < want.size() && b == want[ci], "chunk from %zu ends at %zu, brute force says %zu (caps %zu items, %zu bytes)",
          a, b, ci < want.size() ? want[ci] : 0, max_items, max_bytes);
    uint64_t cost = 0;
    for (size_t i = a; i < b; ++i) cost += it.cost[i];
    CHECK(b - a <= max_items, "chunk [%zu, %zu) above the item cap %zu", a, b, max_items);
    CHECK(cost <= max_bytes || b - a == 1, "chunk [%zu, %zu) of %llu bytes above the cap %zu", a, b,
          (unsigned long long)cost, max_bytes);
    if (cost > max_bytes) CHECK(b == a + 1, "an item above the byte cap is not alone");
    CHECK(b == n || b - a == max_items || cost + it.cost[b] > max_bytes, "chunk [%zu, %zu) is not maximal", a, b);
    // geometry
    CHECK(s.first_byte(a) == it.start[a], "first byte of %zu", a);
    const uint64_t span = it.start[b - 1] + it.len[b - 1] - it.start[a];
    CHECK(s.span_bytes(a, b) == span, "span of [%zu, %zu): %zu, expected %llu", a, b, s.span_bytes(a, b),
          (unsigned long long)span);
    if (s.offsets) {
      rel.assign(b - a + 2, 0xdeadbeefull);
      s.rel_offsets(a, b, rel.data());
      CHECK(rel[0] == 0 && rel[b - a] == span, "relative offsets of [%zu, %zu) do not run from 0 to the span", a, b);
      CHECK(rel[b - a + 1] == 0xdeadbeefull, "relative offsets written past b - a + 1");
      for (size_t k = 0; k < b - a; ++k)
        CHECK(rel[k] == it.start[a + k] - it.start[a] && rel[k + 1] - rel[k] == it.len[a + k], "relative offset %zu", k);
    }
    a = b;
    ++ci;
  }
  CHECK(a == n && ci == want.size(), "the chunks do not partition [0, %zu)", n);
}

static void walk_caps(const BatchSpan &s, const Items &it) {
  const size_t n = it.start.size();
  uint64_t biggest = 0, typical = it.cost[n / 2];
  for (uint64_t c : it.cost) biggest = c > biggest ? c : biggest;
  const size_t item_caps[] = {1, 3, n};
  const size_t byte_caps[] = {1, (size_t)typical, (size_t)typical + 1, (size_t)(3 * typical + 1), (size_t)biggest,
                              (size_t)(4 * biggest)};
  for (size_t mi : item_caps)
    for (size_t mb : byte_caps) walk(s, it, mi, mb ? mb : 1);
}

static int run_walk() {
  // ragged: random lengths with zeros, one item far above every cap but the last
  for (int round = 0; round < 40; ++round) {
    const size_t n = 1 + rnd(70);
    std::vector<uint64_t> offs(n + 1);
    offs[0] = rnd(1000);
    const size_t big = rnd(n);
    Items it;
    for (size_t i = 0; i < n; ++i) {
      uint64_t len = rnd(4) == 0 ? 0 : rnd(200);
      if (i == big && round % 2) len = 5000 + rnd(5000);
      offs[i + 1] = offs[i] + len;
      it.start.push_back(offs[i]);
      it.cost.push_back(len);
      it.len.push_back(len);
    }
    const BatchSpan s{offs.data(), 0, 0};
    walk_caps(s, it);
  }
  // fixed stride (len == stride: transactions; len < stride: padded messages) and stride 0
  const size_t shapes[][2] = {{97, 97}, {512, 512}, {64, 33}, {16, 0}, {0, 40}, {0, 0}};
  for (auto &sh : shapes)
    for (size_t n : {1, 2, 7, 257}) {
      Items it;
      for (size_t i = 0; i < n; ++i) {
        it.start.push_back(i * sh[0]);
        it.cost.push_back(sh[0]);
        it.len.push_back(sh[1]);
      }
      const BatchSpan s{nullptr, sh[0], sh[1]};
      walk_caps(s, it);
      // stride 0 is bounded by the item cap alone, at any byte cap
      if (sh[0] == 0) CHECK(s.chunk_end(0, n, 3, 1) == (n < 3 ? n : 3), "stride 0 under a byte cap of 1");
    }
  // a walk inside a sub-range [lo, hi), as a sharded call makes it
  {
    std::vector<uint64_t> offs(41);
    for (size_t i = 0; i <= 40; ++i) offs[i] = 100 * i;
    const BatchSpan s{offs.data(), 0, 0};
    CHECK(s.chunk_end(10, 30, 64, 350) == 13, "sub-range chunk");
    CHECK(s.chunk_end(28, 30, 64, 350) == 30, "sub-range chunk stops at hi");
    CHECK(s.first_byte(10) == 1000 && s.span_bytes(10, 13) == 300, "sub-range geometry");
  }
  return 0;
}

static int run_validate() {
  using hsvh::first_bad_item;
  const uint64_t good[] = {5, 101, 197, 400};
  CHECK(first_bad_item(good, 3, 96) == 3, "all long enough");
  CHECK(first_bad_item(good, 3, 97) == 0, "first too short");
  CHECK(first_bad_item(good, 3, 0) == 3, "non-decreasing");
  CHECK(first_bad_item(good, 0, 96) == 0, "empty batch");
  const uint64_t shortish[] = {0, 100, 195, 300, 390};
  CHECK(first_bad_item(shortish, 4, 96) == 1, "first of two short items");
  const uint64_t down[] = {0, 100, 90, 290, 280};
  CHECK(first_bad_item(down, 4, 0) == 1, "first decrease");
  CHECK(first_bad_item(down, 4, 96) == 1, "a decrease is not a huge length");
  CHECK(first_bad_item(down, 1, 96) == 1, "only the first n items are looked at");
  const uint64_t zeros[] = {7, 7, 7, 7};
  CHECK(first_bad_item(zeros, 3, 0) == 3, "empty items are fine at min_len 0");
  CHECK(first_bad_item(zeros, 3, 1) == 0, "empty items are too short at min_len 1");
  for (int round = 0; round < 200; ++round) {
    const size_t n = 1 + rnd(30);
    const uint64_t min_len = rnd(3) ? 96 : 0;
    std::vector<uint64_t> offs(n + 1);
    offs[0] = 1000 + rnd(50);
    const bool clean = rnd(4) == 0;
    size_t want = n;  // the first item built bad
    for (size_t i = 0; i < n; ++i) {
      const uint64_t kind = clean ? 0 : rnd(8);
      if (kind == 1 && min_len) {  // too short
        offs[i + 1] = offs[i] + rnd(min_len);
      } else if (kind == 2) {  // decreasing (offs stays above 1000 - 30 * 20)
        offs[i + 1] = offs[i] - 1 - rnd(20);
      } else {
        offs[i + 1] = offs[i] + min_len + rnd(100);
        continue;
      }
      want = i < want ? i : want;
    }
    CHECK(first_bad_item(offs.data(), n, min_len) == want, "random batch: expected %zu", want);
  }
  return 0;
}

int main(int argc, char **argv) {
  int rc = 2;
  if (argc > 1 && strcmp(argv[1], "--walk") == 0) rc = run_walk();
  if (argc > 1 && strcmp(argv[1], "--validate") == 0) rc = run_validate();
  if (rc == 0) printf("ok %ld\n", g_checks);
  return rc;
}
