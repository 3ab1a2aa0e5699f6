// Fuzz harness for the serialized-batch parsers: hsvw::parse_batch
// (csrc/hsv_wire_parse.cpp), which hsv_batch*_bincode run on untrusted network
// bytes (a batch arrives as a TCP frame, mempool/src/mempool.rs, and is read
// back from the store by consensus/src/core.rs:113-142), and the device walk's
// core (csrc/hsv_batchscan.hpp) compiled for the host.  Built with
// -fsanitize=address,undefined by tests/test_batch_wire_fuzz.py and run as a
// program of its own (host only, no GPU).
//
// Checks: no sanitizer report; a valid encoding parses to exactly the encoded
// transactions; every strict prefix and every extension is rejected; on every
// input, mutated ones included, the walk (at a random misalignment, with a
// random fill around the batch) and the parser agree on the verdict, the count
// and every span, and every span lies inside the buffer.
//
// usage: batch_wire_fuzz [iterations] [seed]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

void put_u64(Bytes &b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}

Bytes encode(const std::vector<Bytes> &txs) {
  Bytes b(4, 0);
  put_u64(b, txs.size());
  for (const Bytes &t : txs) {
    put_u64(b, t.size());
    b.insert(b.end(), t.begin(), t.end());
  }
  return b;
}

// parser and walk on any bytes; true if they parse
bool parse_any(const Bytes &b, std::mt19937_64 &rng, std::vector<uint64_t> *spans_out = nullptr) {
  std::vector<uint64_t> spans = {7, 9};  // appended to, never cleared
  size_t n = 0;
  std::string err;
  // an exact-size copy, so that a read past the end is a sanitizer report
  const Bytes exact(b.begin(), b.end());
  const bool ok = hsvw::parse_batch(exact.data(), exact.size(), 0, &spans, n, err);
  CHECK(spans.size() == 2 + (ok ? 2 * n : 0) && spans[0] == 7 && spans[1] == 9, "span vector of %zu entries",
        spans.size());
  spans.erase(spans.begin(), spans.begin() + 2);
  uint64_t at = 12;
  for (size_t i = 0; i < spans.size(); i += 2) {
    CHECK(spans[i] == at + 8 && spans[i + 1] >= spans[i] && spans[i + 1] <= exact.size(), "span %zu", i / 2);
    at = spans[i + 1];
  }
  size_t n2 = 0;
  CHECK(hsvw::parse_batch(exact.data(), exact.size(), 0, nullptr, n2, err) == ok && n2 == n, "parse without spans");
  const bsw::Walked w = bsw::walk(exact.data(), exact.size(), (uint32_t)(rng() % 16), (uint8_t)rng());
  CHECK(w.windows != ~0ull, "the walk did not end within its windows");
  CHECK(w.ok == ok, "walker %d, parser %d (%s)", (int)w.ok, (int)ok, err.c_str());
  if (ok && w.ok) CHECK(w.count == n && w.spans == spans, "walker and parser differ on a well-formed batch");
  if (spans_out) *spans_out = spans;
  return ok;
}

void check_valid(const std::vector<Bytes> &txs, std::mt19937_64 &rng, std::vector<Bytes> &pool) {
  const Bytes enc = encode(txs);
  std::vector<uint64_t> spans;
  CHECK(parse_any(enc, rng, &spans), "valid batch rejected");
  CHECK(spans.size() == 2 * txs.size(), "transaction count");
  for (size_t i = 0; i < txs.size() && 2 * i + 1 < spans.size(); ++i)
    CHECK(Bytes(enc.begin() + spans[2 * i], enc.begin() + spans[2 * i + 1]) == txs[i], "transaction %zu", i);
  for (size_t cut = 0; cut < enc.size(); ++cut)
    CHECK(!parse_any(Bytes(enc.begin(), enc.begin() + cut), rng), "prefix %zu accepted", cut);
  for (int extra = 1; extra <= 9; ++extra) {
    Bytes ext = enc;
    for (int k = 0; k < extra; ++k) ext.push_back((uint8_t)rng());
    CHECK(!parse_any(ext, rng), "extension by %d accepted", extra);
  }
  for (uint32_t tag : {1u, 2u, 0x100u, 0x80000000u}) {
    Bytes t = enc;
    for (int k = 0; k < 4; ++k) t[k] = (uint8_t)(tag >> (8 * k));
    CHECK(!parse_any(t, rng), "tag %u accepted", tag);
  }
  pool.push_back(enc);
}

void set_u64(Bytes &b, size_t off, uint64_t v) {
  if (off + 8 > b.size()) return;
  for (int i = 0; i < 8; ++i) b[off + i] = (uint8_t)(v >> (8 * i));
}

Bytes mutate(const Bytes &in, std::mt19937_64 &rng, const std::vector<Bytes> &pool) {
  Bytes b = in;
  const int ops = 1 + (int)(rng() % 4);
  for (int k = 0; k < ops; ++k) {
    switch (rng() % 8) {
      case 0:  // bit flip
        if (!b.empty()) b[rng() % b.size()] ^= (uint8_t)(1u << (rng() % 8));
        break;
      case 1:  // random byte, often in the header
        if (!b.empty()) b[(rng() & 1) ? rng() % b.size() : rng() % (b.size() < 20 ? b.size() : 20)] = (uint8_t)rng();
        break;
      case 2:  // truncate
        if (!b.empty()) b.resize(rng() % b.size());
        break;
      case 3:  // insert
        b.insert(b.begin() + (b.empty() ? 0 : rng() % (b.size() + 1)), (uint8_t)rng());
        break;
      case 4:  // delete
        if (!b.empty()) b.erase(b.begin() + rng() % b.size());
        break;
      case 5: {  // oversized / boundary u64 at the count, or at a random offset
        const uint64_t vals[] = {~0ull, 1ull << 63, 1ull << 32, 0xffffffffull, 0, 1, 2, 95, 96, ~0ull / 8, ~0ull / 8 + 1,
                                 ~0ull - 7, (uint64_t)b.size(), (uint64_t)b.size() / 8, (uint64_t)b.size() - 12};
        set_u64(b, (rng() & 3) == 0 ? 4 : (b.empty() ? 0 : rng() % b.size()), vals[rng() % (sizeof(vals) / sizeof(vals[0]))]);
        break;
      }
      case 6: {  // splice with another input
        const Bytes &o = pool[rng() % pool.size()];
        if (!o.empty() && !b.empty()) {
          const size_t at = rng() % b.size(), from = rng() % o.size(), len = rng() % (o.size() - from + 1);
          b.resize(at);
          b.insert(b.end(), o.begin() + from, o.begin() + from + len);
        }
        break;
      }
      default:  // grow or shrink one length prefix by a little (walks off the chain)
        if (b.size() >= 20) set_u64(b, 12, (uint64_t)(rng() % 300));
    }
  }
  return b;
}

}  // namespace

int main(int argc, char **argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 100000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261021);
  std::vector<Bytes> pool;
  auto tx = [&](size_t n) {
    Bytes t(n);
    for (uint8_t &x : t) x = (uint8_t)rng();
    return t;
  };
  check_valid({}, rng, pool);
  check_valid({tx(136)}, rng, pool);
  check_valid({tx(0), tx(95), tx(96), tx(97), tx(0), tx(1)}, rng, pool);
  check_valid({tx(1000), tx(7), tx(1030)}, rng, pool);  // prefixes around the first two window edges
  {
    std::vector<Bytes> many;
    for (size_t i = 0; i < 40; ++i) many.push_back(tx(90 + i));
    check_valid(many, rng, pool);
  }
  pool.push_back(Bytes());
  for (long i = 0; i < iters; ++i) (void)parse_any(mutate(pool[rng() % pool.size()], rng, pool), rng);
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("batch wire fuzz ok: %ld mutated inputs, %zu seeds\n", iters, pool.size());
  return 0;
}
