// csrc/hsv_proposal.hpp compiled for the host with plain g++ (no HIP): the
// assembly of a proposal into one verification batch and the reduction of the
// batch's flags to the reference's verdict (tests/test_proposal_host.py).
//
//   proposal_host --check    item order, the genesis-QC skip, the empty QC, the
//                            verdict on synthetic flags; prints "ok <checks>"
//   proposal_host --digests  the block, QC / vote and timeout digests of fixed
//                            inputs as hex, one per line, for hashlib to match
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hsv_proposal.hpp"

namespace {

long checks = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    ++checks;                                                             \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

constexpr uint8_t kGood = HSV_STRICT_OK | HSV_EQ_OK | HSV_PARSE_OK | HSV_S_OK | HSV_A_OK | HSV_R_OK;
// what a small-order or non-canonical vote can carry: the batch rule's bits without the strict one
constexpr uint8_t kBatchOnly = HSV_EQ_OK | HSV_PARSE_OK | HSV_S_OK | HSV_A_OK | HSV_R_OK;

// a block whose every byte names its place: vote v of the QC has pk bytes
// 0x40 + v, R bytes 0x60 + v, s bytes 0x80 + v; of the TC 0xa0 / 0xc0 / 0xe0 + v
struct Fixture {
  hsv_proposal p{};
  std::vector<uint8_t> payload, qc, tc;
  Fixture(size_t n_payload, size_t n_qc, bool has_tc, size_t n_tc, bool genesis) {
    std::memset(p.author, 0x11, 32);
    std::memset(p.signature, 0x22, 64);
    p.round = 9;
    payload.assign(32 * n_payload, 0x33);
    if (!genesis) {
      std::memset(p.qc_hash, 0x44, 32);
      p.qc_round = 8;
    }
    qc.resize(96 * n_qc);
    for (size_t v = 0; v < n_qc; ++v) {
      std::memset(qc.data() + 96 * v, 0x40 + (int)v, 32);
      std::memset(qc.data() + 96 * v + 32, 0x60 + (int)v, 32);
      std::memset(qc.data() + 96 * v + 64, 0x80 + (int)v, 32);
    }
    tc.resize(104 * n_tc);
    for (size_t v = 0; v < n_tc; ++v) {
      std::memset(tc.data() + 104 * v, 0xa0 + (int)v, 32);
      std::memset(tc.data() + 104 * v + 32, 0xc0 + (int)v, 32);
      std::memset(tc.data() + 104 * v + 64, 0xe0 + (int)v, 32);
      hsvp::put_le64(tc.data() + 104 * v + 96, 5 + v % 2);  // two distinct high_qc_rounds
    }
    p.payload = payload.empty() ? nullptr : payload.data();
    p.n_payload = n_payload;
    p.qc_votes = qc.empty() ? nullptr : qc.data();
    p.n_qc = n_qc;
    p.has_tc = has_tc;
    p.tc_round = 9;
    p.tc_votes = tc.empty() ? nullptr : tc.data();
    p.n_tc = n_tc;
  }
};

bool all_bytes(const uint8_t *p, size_t n, uint8_t v) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] != v) return false;
  return true;
}

void check_order() {
  std::vector<uint8_t> pre;
  hsvp::Items it;
  // something already in the batch: the object's items follow it
  it.grow(2);
  Fixture f(3, 3, true, 4, false);
  const hsvp::Layout l = hsvp::append(hsvp::object_of(f.p, pre), it);
  CHECK(l.first == 2 && l.n_qc == 3 && l.qc_items == 3 && l.n_tc == 4 && l.items() == 8);
  CHECK(it.n == 10 && it.pk.size() == 320 && it.sig.size() == 640 && it.msg.size() == 320);
  uint8_t d[32];
  // author
  CHECK(all_bytes(it.pk.data() + 32 * 2, 32, 0x11) && all_bytes(it.sig.data() + 64 * 2, 64, 0x22));
  hsvp::block_digest(f.p.author, 9, f.payload.data(), 3, f.p.qc_hash, pre, d);
  CHECK(std::memcmp(it.msg.data() + 32 * 2, d, 32) == 0);
  // QC votes, one shared digest
  hsvp::qc_digest(f.p.qc_hash, 8, d);
  for (size_t v = 0; v < 3; ++v) {
    const size_t i = 3 + v;
    CHECK(all_bytes(it.pk.data() + 32 * i, 32, 0x40 + v));
    CHECK(all_bytes(it.sig.data() + 64 * i, 32, 0x60 + v) && all_bytes(it.sig.data() + 64 * i + 32, 32, 0x80 + v));
    CHECK(std::memcmp(it.msg.data() + 32 * i, d, 32) == 0);
  }
  // TC votes, a digest per high_qc_round
  for (size_t v = 0; v < 4; ++v) {
    const size_t i = 6 + v;
    CHECK(all_bytes(it.pk.data() + 32 * i, 32, 0xa0 + v));
    CHECK(all_bytes(it.sig.data() + 64 * i, 32, 0xc0 + v) && all_bytes(it.sig.data() + 64 * i + 32, 32, 0xe0 + v));
    hsvp::timeout_digest(9, 5 + v % 2, d);
    CHECK(std::memcmp(it.msg.data() + 32 * i, d, 32) == 0);
  }
  // has_tc == 0: the votes behind tc_votes are not items
  Fixture g(0, 2, false, 4, false);
  it.clear();
  const hsvp::Layout lg = hsvp::append(hsvp::object_of(g.p, pre), it);
  CHECK(lg.first == 0 && lg.n_tc == 0 && lg.items() == 3 && it.n == 3);
}

void check_genesis_and_empty() {
  std::vector<uint8_t> pre;
  hsvp::Items it;
  // the genesis QC (hash and round zero) is skipped, with or without votes
  for (size_t n_qc : {size_t(0), size_t(3)}) {
    Fixture f(1, n_qc, true, 2, true);
    it.clear();
    const hsvp::Layout l = hsvp::append(hsvp::object_of(f.p, pre), it);
    CHECK(l.n_qc == n_qc && l.qc_items == 0 && l.items() == 3 && it.n == 3);
    CHECK(all_bytes(it.pk.data() + 32, 32, 0xa0));  // the TC follows the author directly
    const uint8_t flags[3] = {kGood, kGood, kGood};
    CHECK(hsvp::reduce(l, flags).stage == HSV_STAGE_OK);
    std::vector<uint8_t> out(1 + n_qc + 2, 0xee);
    hsvp::scatter_flags(l, flags, out.data());
    CHECK(out[0] == kGood && out[1 + n_qc] == kGood && out[2 + n_qc] == kGood);
    for (size_t v = 0; v < n_qc; ++v) CHECK(out[1 + v] == 0);  // not verified: read 0
  }
  // a zero hash with a round, or a hash with round 0, is not genesis
  Fixture a(0, 1, false, 0, true);
  a.p.qc_round = 1;
  CHECK(!hsvp::qc_is_genesis(a.p.qc_hash, a.p.qc_round));
  it.clear();
  CHECK(hsvp::append(hsvp::object_of(a.p, pre), it).qc_items == 1);
  Fixture b(0, 1, false, 0, true);
  b.p.qc_hash[31] = 1;
  CHECK(!hsvp::qc_is_genesis(b.p.qc_hash, 0));
  // an empty QC that is not genesis: no items, and it passes
  Fixture e(2, 0, false, 0, false);
  it.clear();
  const hsvp::Layout le = hsvp::append(hsvp::object_of(e.p, pre), it);
  CHECK(le.qc_items == 0 && le.items() == 1);
  const uint8_t one[1] = {kGood};
  CHECK(hsvp::reduce(le, one).stage == HSV_STAGE_OK);
}

void check_verdicts() {
  hsvp::Layout l;
  l.first = 1;  // one foreign item in front
  l.n_qc = l.qc_items = 3;
  l.n_tc = 3;
  auto verdict = [&](std::vector<uint8_t> f) {
    f.insert(f.begin(), 0);  // the foreign item's flags must not matter
    return hsvp::reduce(l, f.data());
  };
  auto is = [](hsv_proposal_result r, uint32_t stage, uint32_t index) { return r.stage == stage && r.index == index; };
  const std::vector<uint8_t> good(7, kGood);
  CHECK(is(verdict(good), HSV_STAGE_OK, 0));
  // PARSE_OK | EQ_OK without STRICT_OK: passes in the QC, fails in the TC and as author
  for (size_t v = 0; v < 3; ++v) {
    std::vector<uint8_t> f = good;
    f[1 + v] = kBatchOnly;
    CHECK(is(verdict(f), HSV_STAGE_OK, 0));
    f = good;
    f[4 + v] = kBatchOnly;
    CHECK(is(verdict(f), HSV_STAGE_TC, (uint32_t)v));
  }
  {
    std::vector<uint8_t> f = good;
    f[0] = kBatchOnly;
    CHECK(is(verdict(f), HSV_STAGE_AUTHOR, 0));
  }
  // a QC vote needs both bits; STRICT_OK alone is no pass (it cannot occur, but the rule is the batch one)
  for (uint8_t bad : {(uint8_t)0, (uint8_t)HSV_PARSE_OK, (uint8_t)HSV_EQ_OK, (uint8_t)HSV_STRICT_OK,
                      (uint8_t)(kGood & ~HSV_EQ_OK), (uint8_t)(kGood & ~HSV_PARSE_OK)}) {
    std::vector<uint8_t> f = good;
    f[2] = bad;
    CHECK(is(verdict(f), HSV_STAGE_QC, 1));
  }
  // the first failing stage in the reference's order, whatever else fails
  {
    std::vector<uint8_t> f = good;
    f[0] = 0;
    f[2] = 0;
    f[5] = 0;
    CHECK(is(verdict(f), HSV_STAGE_AUTHOR, 0));
    f[0] = kGood;
    CHECK(is(verdict(f), HSV_STAGE_QC, 1));
    f[2] = kGood;
    CHECK(is(verdict(f), HSV_STAGE_TC, 1));
  }
  // the lowest failing vote of the stage
  {
    std::vector<uint8_t> f = good;
    f[3] = 0;
    f[1] = 0;
    CHECK(is(verdict(f), HSV_STAGE_QC, 0));
    f = good;
    f[6] = 0;
    f[5] = kBatchOnly;
    CHECK(is(verdict(f), HSV_STAGE_TC, 1));
    f = good;
    f[6] = 0;
    CHECK(is(verdict(f), HSV_STAGE_TC, 2));
  }
  // flags as the caller sees them, QC checked
  std::vector<uint8_t> f = {0, 1, 2, 3, 4, 5, 6, 7}, out(7, 0xee);
  hsvp::scatter_flags(l, f.data(), out.data());
  for (int i = 0; i < 7; ++i) CHECK(out[i] == i + 1);
}

void check_memo() {
  // more distinct rounds than the memo holds, revisited: every digest is the direct one
  hsvp::TcDigestMemo memo(77);
  uint8_t a[32], b[32];
  for (int pass = 0; pass < 2; ++pass)
    for (uint64_t r = 0; r < 50; ++r) {
      memo.digest(r * 3 % 50, a);
      hsvp::timeout_digest(77, r * 3 % 50, b);
      CHECK(std::memcmp(a, b, 32) == 0);
    }
}

void print_hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
  std::printf("\n");
}

// author = 00 01 .. 1f, round = 0x0102030405060708, payload k = 32 bytes of
// 0xa0 + k, qc.hash = 20 21 .. 3f; qc round 7; timeout (9, 8)
void print_digests() {
  uint8_t author[32], hash[32], d[32];
  for (int i = 0; i < 32; ++i) {
    author[i] = (uint8_t)i;
    hash[i] = (uint8_t)(0x20 + i);
  }
  std::vector<uint8_t> pre;
  for (size_t np : {size_t(0), size_t(3)}) {
    std::vector<uint8_t> payload(32 * np);
    for (size_t k = 0; k < np; ++k) std::memset(payload.data() + 32 * k, 0xa0 + (int)k, 32);
    hsvp::block_digest(author, 0x0102030405060708ull, payload.data(), np, hash, pre, d);
    print_hex(d, 32);
  }
  hsvp::qc_digest(hash, 7, d);
  print_hex(d, 32);
  hsvp::timeout_digest(9, 8, d);
  print_hex(d, 32);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--digests") {
    print_digests();
    return 0;
  }
  if (mode != "--check") {
    std::fprintf(stderr, "usage: proposal_host --check | --digests\n");
    return 2;
  }
  check_order();
  check_genesis_and_empty();
  check_verdicts();
  check_memo();
  std::printf("ok %ld\n", checks);
  return 0;
}
