// The device walk of a serialized mempool batch (csrc/hsv_batchscan.hpp, the
// core of hsv_batchwire.hip's kernels) compiled for the host and held against
// the host parser hsvw::parse_batch (csrc/hsv_wire_parse.cpp) on the same
// bytes: statuses, counts and span pairs, at every misalignment 0..15 of the
// batch in its chunk stream and with three fill patterns around it.  Built with
// -fsanitize=address,undefined by tests/test_batch_wire_host.py; no GPU.
//
// Vectors: an empty batch, one transaction, ragged lengths including 0, 95 and
// 96; truncation at every byte, a count beyond the buffer, lengths of 2^64 - 1
// and with high bits set, tags 1 and 2, one trailing byte; and stepped batches
// of >= 3 windows whose transaction lengths step so that a length prefix lands
// on every residue mod 16 and straddles a window edge at every split (1..7
// bytes before the edge) -- checked here from the spans, not assumed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "batchscan_walk.hpp"
#include "hsv_wire_parse.h"

namespace {

using Bytes = std::vector<uint8_t>;

int failures = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      std::fprintf(stderr, "CHECK failed: %s: ", #c);  \
      std::fprintf(stderr, __VA_ARGS__);               \
      std::fprintf(stderr, "\n");                      \
      ++failures;                                      \
    }                                                  \
  } while (0)

void put_u32(Bytes &b, uint32_t v) {
  for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
void put_u64(Bytes &b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}

Bytes encode(const std::vector<size_t> &lens, uint32_t tag = 0) {
  Bytes b;
  put_u32(b, tag);
  put_u64(b, lens.size());
  uint8_t x = 1;
  for (size_t n : lens) {
    put_u64(b, n);
    for (size_t i = 0; i < n; ++i) b.push_back(x = (uint8_t)(x * 73 + 41));
  }
  return b;
}

// walker == parser on b, at every misalignment; returns the parser's verdict
bool same(const Bytes &b, const char *what, std::vector<uint64_t> *spans_out = nullptr) {
  std::vector<uint64_t> spans;
  size_t n = 0;
  std::string err;
  const bool ok = hsvw::parse_batch(b.data(), b.size(), 0, &spans, n, err);
  CHECK(ok || spans.empty(), "%s: spans left behind a failed parse", what);
  for (uint32_t mis = 0; mis < 16; ++mis)
    for (uint8_t fill : {(uint8_t)0x00, (uint8_t)0xff, (uint8_t)0xa5}) {
      const bsw::Walked w = bsw::walk(b.data(), b.size(), mis, fill);
      CHECK(w.windows != ~0ull, "%s: mis %u: the walk did not end within its windows", what, mis);
      CHECK(w.ok == ok, "%s: mis %u fill %02x: walker %d, parser %d (%s)", what, mis, fill, (int)w.ok, (int)ok,
            err.c_str());
      if (ok && w.ok) {
        CHECK(w.count == n, "%s: mis %u: count %llu != %zu", what, mis, (unsigned long long)w.count, n);
        CHECK(w.spans == spans, "%s: mis %u: spans differ", what, mis);
      }
    }
  if (spans_out) *spans_out = spans;
  return ok;
}

void set_u64(Bytes &b, size_t off, uint64_t v) {
  for (int i = 0; i < 8; ++i) b[off + i] = (uint8_t)(v >> (8 * i));
}

// A batch of at least `windows` windows whose length prefixes, with the batch
// at misalignment mis, land `split` bytes before window edge k for (k, split) =
// (1, 1), (2, 2), ... (7, 7), (8, 1), ...; between the edges the lengths step
// by one from 0, so the prefixes visit every residue mod 16.
std::vector<size_t> stepped_lengths(uint32_t mis, size_t windows) {
  std::vector<size_t> lens;
  size_t pos = mis + hsv::kBatchHeader, step = 0;  // stream position of the next prefix
  for (size_t k = 1; k <= windows; ++k) {
    const size_t target = k * hsv::kScanWindow - ((k - 1) % 7 + 1);
    while (pos + 8 + step + 8 + 120 <= target) {  // room for this one and a last one of >= 120 bytes
      lens.push_back(step);
      pos += 8 + step;
      step = (step + 1) % 200;
    }
    lens.push_back(target - pos - 8);  // the next prefix starts at target
    pos = target;
  }
  lens.push_back(97);  // the transaction behind the last straddling prefix
  return lens;
}

void check_stepped(uint32_t mis, size_t windows) {
  const Bytes b = encode(stepped_lengths(mis, windows));
  CHECK(b.size() >= 3 * hsv::kScanWindow, "stepped batch of %zu bytes", b.size());
  std::vector<uint64_t> spans;
  CHECK(same(b, "stepped batch", &spans), "stepped batch rejected");
  std::set<uint64_t> residues, splits;
  for (size_t i = 0; i < spans.size(); i += 2) {
    const uint64_t p = spans[i] - 8 + mis;  // stream position of the prefix
    residues.insert(p % 16);
    const uint64_t to_edge = hsv::kScanWindow - p % hsv::kScanWindow;
    if (to_edge < 8) splits.insert(to_edge);
  }
  CHECK(residues.size() == 16, "mis %u: prefixes on %zu residues mod 16", mis, residues.size());
  CHECK(splits.size() == 7, "mis %u: straddles at %zu of the 7 splits", mis, splits.size());
}

}  // namespace

int main() {
  CHECK(same(encode({}), "empty batch"), "empty batch rejected");
  CHECK(same(encode({136}), "one transaction"), "one transaction rejected");
  const std::vector<size_t> ragged = {0, 95, 96, 97, 1, 400, 0, 0, 1023, 1024, 1025, 96};
  const Bytes good = encode(ragged);
  CHECK(same(good, "ragged batch"), "ragged batch rejected");
  // truncation at every byte, one trailing byte
  for (size_t cut = 0; cut < good.size(); ++cut) {
    const Bytes t(good.begin(), good.begin() + cut);
    CHECK(!same(t, "truncated batch"), "prefix %zu accepted", cut);
  }
  Bytes ext = good;
  ext.push_back(0);
  CHECK(!same(ext, "trailing byte"), "a trailing byte accepted");
  // tags 1 (BatchRequest) and 2, and each tag byte alone
  CHECK(!same(encode(ragged, 1), "tag 1"), "tag 1 accepted");
  CHECK(!same(encode(ragged, 2), "tag 2"), "tag 2 accepted");
  CHECK(!same(encode(ragged, 0x01000000u), "tag high byte"), "tag 0x01000000 accepted");
  // counts beyond the buffer
  for (uint64_t c : std::vector<uint64_t>{ragged.size() + 1, good.size(), ~0ull, 1ull << 63, (~0ull) / 8 + 1}) {
    Bytes t = good;
    set_u64(t, 4, c);
    CHECK(!same(t, "count beyond the buffer"), "count %llu accepted", (unsigned long long)c);
  }
  // lengths: 2^64 - 1, high bits set, one past the end -- at the first, a middle and the last prefix
  std::vector<uint64_t> spans;
  (void)same(good, "ragged batch", &spans);
  for (size_t i : {(size_t)0, ragged.size() / 2, ragged.size() - 1})
    for (uint64_t add : std::vector<uint64_t>{~0ull, 1ull << 63, 1ull << 32, 1, ~0ull - 7}) {
      Bytes t = good;
      const size_t at = (size_t)spans[2 * i] - 8;
      set_u64(t, at, add == 1 ? good.size() - spans[2 * i] + 1 : add);
      CHECK(!same(t, "length past the end"), "transaction %zu with a length past the end accepted", i);
    }
  // a count one too small leaves trailing bytes; one too large truncates
  {
    Bytes t = good;
    set_u64(t, 4, ragged.size() - 1);
    CHECK(!same(t, "count one too small"), "count one too small accepted");
  }
  // stepped batches of 8 and 15 windows at every misalignment
  for (uint32_t mis = 0; mis < 16; ++mis) {
    check_stepped(mis, 8);
    check_stepped(mis, 15);
  }
  // a transaction much longer than a window: the walk skips windows without a prefix
  CHECK(same(encode({5000, 0, 96, 9000}), "long transactions"), "long transactions rejected");
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batchscan host ok\n");
  return 0;
}
