// The arithmetic of hsv_seal_transactions* (csrc/hsv_seal.hpp) on the host,
// built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_seal_host.py: the greedy cut against a naive restatement of
// BatchMaker::run, the destination arithmetic against a naive serializer, the
// bound, and the byte-shifting copy for every pair of alignments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "hsv_seal.hpp"

using namespace hsv;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

namespace {

struct Tx {
  std::vector<uint8_t> bytes;
  uint32_t cls;
};

// BatchMaker::run, line by line (mempool/src/batch_maker.rs:87-105)
std::vector<std::vector<size_t>> naive_batches(const std::vector<Tx> &txs, uint64_t batch_size, bool flush,
                                               std::vector<size_t> &held) {
  std::vector<std::vector<size_t>> out;
  std::vector<size_t> cur;
  uint64_t size = 0;
  for (size_t i = 0; i < txs.size(); ++i) {
    if (txs[i].cls != kSealKept) continue;
    size += txs[i].bytes.size();
    cur.push_back(i);
    if (size >= batch_size) {
      out.push_back(cur);
      cur.clear();
      size = 0;
    }
  }
  if (flush && !cur.empty()) {
    out.push_back(cur);
    cur.clear();
  }
  held = cur;
  return out;
}

std::vector<uint8_t> naive_encode(const std::vector<Tx> &txs, const std::vector<std::vector<size_t>> &batches,
                                  std::vector<uint64_t> &starts) {
  std::vector<uint8_t> out;
  auto le = [&](uint64_t v, int n) {
    for (int k = 0; k < n; ++k) out.push_back((uint8_t)(v >> (8 * k)));
  };
  for (const auto &b : batches) {
    starts.push_back(out.size());
    le(0, 4);
    le(b.size(), 8);
    for (size_t i : b) {
      le(txs[i].bytes.size(), 8);
      out.insert(out.end(), txs[i].bytes.begin(), txs[i].bytes.end());
    }
  }
  starts.push_back(out.size());
  return out;
}

// the copy of hsv_seal.hip on host arrays whose first byte is 16-byte aligned
void copy_bytes(const uint8_t *sbase, uint64_t spos, uint8_t *dbase, uint64_t dpos, uint64_t len) {
  if (!len) return;
  SealCopy cp;
  cp.spos = spos;
  cp.dpos = dpos;
  cp.len = len;
  const uint64_t nc = cp.chunks();
  for (uint64_t c = nc; c-- > 0;)  // any order
    cp.chunk(
        c,
        [&](uint64_t k) {
          SealChunk v;
          std::memcpy(&v, sbase + 16 * k, 16);
          return v;
        },
        [&](uint64_t k, SealChunk v) { std::memcpy(dbase + 16 * k, &v, 16); },
        [&](uint64_t p, uint8_t b) { dbase[p] = b; });
}

void test_cut_and_layout() {
  std::mt19937_64 rng(7);
  std::vector<Tx> txs;
  uint64_t total = 0;
  for (int i = 0; i < 300; ++i) {
    Tx t;
    const size_t len = i % 37 == 0 ? 0 : 96 + rng() % 64;
    t.bytes.resize(len);
    for (auto &b : t.bytes) b = (uint8_t)rng();
    t.cls = rng() % 5 == 0 ? kSealRejected : rng() % 11 == 0 ? kSealMalformed : kSealKept;
    total += len;
    txs.push_back(t);
  }
  const size_t n = txs.size();
  // the records of the apply kernel
  std::vector<uint64_t> E(n), R(n);
  uint64_t e = 0, r = 0;
  for (size_t i = 0; i < n; ++i) {
    if (txs[i].cls == kSealKept) {
      e += txs[i].bytes.size();
      ++r;
    }
    E[i] = e;
    R[i] = r;
  }
  // the input, packed at an odd position of an aligned array
  const uint64_t imis = 5;
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + txs[i].bytes.size();
  uint8_t *in = static_cast<uint8_t *>(std::aligned_alloc(16, (imis + total + 15) / 16 * 16));
  for (size_t i = 0; i < n; ++i)
    if (!txs[i].bytes.empty()) std::memcpy(in + imis + off[i], txs[i].bytes.data(), txs[i].bytes.size());
  const uint64_t sizes[] = {1, 96, 97, 1000, total + 1, ~0ull};
  for (uint64_t bs : sizes)
    for (int flush = 0; flush < 2; ++flush) {
      std::vector<size_t> held;
      const auto want = naive_batches(txs, bs, flush, held);
      std::vector<uint64_t> want_starts;
      const auto want_bytes = naive_encode(txs, want, want_starts);
      // the walk of the cut kernel
      SealCut cut;
      cut.batch_size = bs;
      std::vector<uint64_t> brank{0}, starts{0};
      for (size_t i = 0; i < n; ++i)
        if (cut.closes(i, E[i])) {
          cut.close(i, E[i], R[i]);
          brank.push_back(R[i]);
          starts.push_back(seal_batch_start(cut.nb, R[i], E[i]));
        }
      if (flush && r > cut.cut_r) {
        cut.close(n, e, r);
        brank.push_back(r);
        starts.push_back(seal_batch_start(cut.nb, r, e));
      }
      CHECK(cut.nb == want.size());
      CHECK(starts == want_starts);
      CHECK(r - cut.cut_r == held.size());
      for (size_t b = 0; b < want.size(); ++b) CHECK(brank[b + 1] - brank[b] == want[b].size());
      uint64_t bound_bytes = 0, bound_batches = 0;
      CHECK(seal_bound(total, n, bs, &bound_bytes, &bound_batches));
      CHECK(bound_bytes >= want_bytes.size() && bound_batches >= want.size());
      // the copy kernel's places, into an output at an odd position between guards
      const uint64_t omis = 11;
      const size_t cap = (omis + want_bytes.size() + 15) / 16 * 16 + 16;
      uint8_t *out = static_cast<uint8_t *>(std::aligned_alloc(16, cap));
      std::memset(out, 0xEE, cap);
      for (size_t i = 0; i < n; ++i) {
        if (txs[i].cls != kSealKept || R[i] > cut.cut_r) continue;
        const uint64_t k = R[i] - 1, len = txs[i].bytes.size();
        size_t b = 0;
        while (!(brank[b] <= k && k < brank[b + 1])) ++b;
        const uint64_t dst = seal_dst(b, k, E[i] - len);
        for (int j = 0; j < 8; ++j) out[omis + dst - 8 + j] = (uint8_t)(len >> (8 * j));
        if (brank[b] == k) {
          for (int j = 0; j < 8; ++j) out[omis + dst - 16 + j] = (uint8_t)((brank[b + 1] - brank[b]) >> (8 * j));
          for (int j = 0; j < 4; ++j) out[omis + dst - 20 + j] = 0;
        }
        copy_bytes(in, imis + off[i], out, omis + dst, len);
      }
      CHECK(want_bytes.empty() || std::memcmp(out + omis, want_bytes.data(), want_bytes.size()) == 0);
      for (size_t p = 0; p < omis; ++p) CHECK(out[p] == 0xEE);
      for (size_t p = omis + want_bytes.size(); p < cap; ++p) CHECK(out[p] == 0xEE);
      std::free(out);
    }
  std::free(in);
  uint64_t a, b;
  CHECK(!seal_bound(~0ull - 7, 1, 1, &a, &b));
  CHECK(seal_bound(0, 0, 5, &a, &b) && a == 0 && b == 0);
  CHECK(seal_bound(1000, 3, 100, &a, &b) && b == 3 && a == 1000 + 24 + 36);
  CHECK(seal_extra_pieces(0) == 0 && seal_extra_pieces(kSealPiece) == 0 && seal_extra_pieces(kSealPiece + 1) == 1 &&
        seal_extra_pieces(3 * kSealPiece) == 2);
}

void test_copy_alignments() {
  for (uint32_t smis = 0; smis < 16; ++smis)
    for (uint32_t dmis = 0; dmis < 16; ++dmis)
      for (uint64_t len = 0; len <= 80; ++len) {
        // the source array ends with the chunk that holds the last source byte,
        // and starts 32 bytes (of another object's, in the kernel) before the first
        const uint64_t spos = 32 + smis, dpos = 48 + dmis;
        const size_t scap = (spos + (len ? len : 1) + 15) / 16 * 16;
        const size_t dcap = (dpos + len + 15) / 16 * 16 + 32;
        uint8_t *src = static_cast<uint8_t *>(std::aligned_alloc(16, scap));
        uint8_t *dst = static_cast<uint8_t *>(std::aligned_alloc(16, dcap));
        for (size_t i = 0; i < scap; ++i) src[i] = (uint8_t)(i * 7 + 3);
        std::memset(dst, 0xCD, dcap);
        copy_bytes(src, spos, dst, dpos, len);
        for (size_t p = 0; p < dcap; ++p) {
          const uint8_t want = p >= dpos && p < dpos + len ? src[spos + (p - dpos)] : 0xCD;
          if (dst[p] != want) {
            std::printf("copy smis %u dmis %u len %llu at %zu\n", smis, dmis, (unsigned long long)len, p);
            std::exit(1);
          }
        }
        std::free(src);
        std::free(dst);
      }
  // a source at the very start of its array: the chunk before it is never read
  uint8_t *src = static_cast<uint8_t *>(std::aligned_alloc(16, 48));
  uint8_t *dst = static_cast<uint8_t *>(std::aligned_alloc(16, 64));
  for (int i = 0; i < 48; ++i) src[i] = (uint8_t)(i + 1);
  std::memset(dst, 0, 64);
  copy_bytes(src, 1, dst, 15, 40);
  CHECK(std::memcmp(dst + 15, src + 1, 40) == 0);
  std::free(src);
  std::free(dst);
}

}  // namespace

int main() {
  test_cut_and_layout();
  test_copy_alignments();
  CHECK(seal_class(5, 4, false, 0xff) == kSealMalformed && seal_class(4, 4, false, 0) == kSealKept);
  CHECK(seal_class(0, 96, true, 0xfe) == kSealRejected && seal_class(0, 96, true, 0x01) == kSealKept);
  std::printf("seal host ok\n");
  return 0;
}
