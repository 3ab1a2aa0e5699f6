// Fuzz harness for the block, timeout and vote parsers (csrc/hsv_wire_parse.cpp)
// and the batch assembly behind them (csrc/hsv_proposal.hpp), built with
// -fsanitize=address,undefined by tests/test_proposal_fuzz.py and run as a
// program of its own (host only, no GPU).  The parsers read untrusted network
// bytes: the reference receives proposals, votes and timeouts as TCP frames
// (network/src/receiver.rs:47-60) and bincode-deserialises them
// (consensus/src/consensus.rs:32-39).
//
// Inputs: valid Block / Timeout / Vote encodings (bincode 1.3 defaults,
// PublicKey as its base64 string) with and without a TC, with a genesis QC,
// with empty and non-empty payloads; from each, every truncation, a trailing
// byte, every Option tag but 0 and 1, oversized counts and string lengths, and
// random byte flips / insertions / deletions / splices.  Checks: no sanitizer
// report; a valid input parses to exactly the encoded fields; every strict
// prefix and every extension is rejected; whatever parses assembles into a
// batch whose sizes agree with its layout.
//
// usage: proposal_fuzz [iterations] [seed]
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hsv_proposal.hpp"
#include "hsv_wire_parse.h"

namespace {

using Bytes = std::vector<uint8_t>;

void put_u64(Bytes &b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}

void put_key(Bytes &b, const uint8_t pk[32]) {
  static const char *A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string s;
  for (size_t i = 0; i < 30; i += 3) {
    const uint32_t v = (pk[i] << 16) | (pk[i + 1] << 8) | pk[i + 2];
    s += A[v >> 18];
    s += A[(v >> 12) & 63];
    s += A[(v >> 6) & 63];
    s += A[v & 63];
  }
  const uint32_t v = (pk[30] << 16) | (pk[31] << 8);
  s += A[v >> 18];
  s += A[(v >> 12) & 63];
  s += A[(v >> 6) & 63];
  s += '=';
  put_u64(b, s.size());
  b.insert(b.end(), s.begin(), s.end());
}

void fill(std::mt19937_64 &rng, uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)rng();
}

struct Qc {
  uint8_t hash[32] = {0};
  uint64_t round = 0;
  Bytes votes;  // n * 96
  size_t n = 0;
};

Qc make_qc(std::mt19937_64 &rng, size_t n, bool genesis) {
  Qc q;
  if (!genesis) {
    fill(rng, q.hash, 32);
    q.round = 1 + rng() % 1000000;
  }
  q.n = n;
  q.votes.resize(96 * n);
  fill(rng, q.votes.data(), q.votes.size());
  return q;
}

void put_qc(Bytes &b, const Qc &q) {
  b.insert(b.end(), q.hash, q.hash + 32);
  put_u64(b, q.round);
  put_u64(b, q.n);
  for (size_t i = 0; i < q.n; ++i) {
    put_key(b, q.votes.data() + 96 * i);
    b.insert(b.end(), q.votes.begin() + 96 * i + 32, q.votes.begin() + 96 * (i + 1));
  }
}

struct Block {
  Qc qc;
  bool has_tc = false;
  uint64_t tc_round = 0;
  Bytes tc_votes;  // n_tc * 104
  size_t n_tc = 0;
  uint8_t author[32], signature[64];
  uint64_t round = 0;
  Bytes payload;
  size_t tag_at = 0;  // offset of the Option tag in enc
  Bytes enc;
};

Block make_block(std::mt19937_64 &rng, size_t n_qc, bool genesis, bool has_tc, size_t n_tc, size_t n_payload) {
  Block k;
  k.qc = make_qc(rng, n_qc, genesis);
  k.has_tc = has_tc;
  k.n_tc = has_tc ? n_tc : 0;
  k.tc_round = 1000 + rng() % 1000;
  k.tc_votes.resize(104 * k.n_tc);
  fill(rng, k.tc_votes.data(), k.tc_votes.size());
  fill(rng, k.author, 32);
  fill(rng, k.signature, 64);
  k.round = rng() % 1000000;
  k.payload.resize(32 * n_payload);
  fill(rng, k.payload.data(), k.payload.size());
  put_qc(k.enc, k.qc);
  k.tag_at = k.enc.size();
  k.enc.push_back(has_tc ? 1 : 0);
  if (has_tc) {
    put_u64(k.enc, k.tc_round);
    put_u64(k.enc, k.n_tc);
    for (size_t i = 0; i < k.n_tc; ++i) {
      const uint8_t *v = k.tc_votes.data() + 104 * i;
      put_key(k.enc, v);
      k.enc.insert(k.enc.end(), v + 32, v + 104);  // R || s || high_qc_round_le
    }
  }
  put_key(k.enc, k.author);
  put_u64(k.enc, k.round);
  put_u64(k.enc, n_payload);
  k.enc.insert(k.enc.end(), k.payload.begin(), k.payload.end());
  k.enc.insert(k.enc.end(), k.signature, k.signature + 64);
  return k;
}

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

// what parses must assemble: sizes of the batch against the layout
void assemble(const hsvw::BlockParsed &b) {
  std::vector<uint8_t> pre;
  hsvp::Items it;
  const hsvp::Layout l = hsvp::append(hsvp::object_of(b.p, pre), it);
  CHECK(it.n == l.items() && it.pk.size() == 32 * it.n && it.sig.size() == 64 * it.n && it.msg.size() == 32 * it.n,
        "batch sizes");
  CHECK(l.n_qc == b.p.n_qc && l.n_tc == (b.p.has_tc ? b.p.n_tc : 0), "layout counts");
  std::vector<uint8_t> flags(it.n, 0x07), out(1 + l.n_qc + l.n_tc);
  CHECK(hsvp::reduce(l, flags.data()).stage == HSV_STAGE_OK, "verdict of all-good flags");
  hsvp::scatter_flags(l, flags.data(), out.data());
}

void check_valid_block(const Block &k) {
  hsvw::BlockParsed b;
  std::string err;
  CHECK(hsvw::parse_block(k.enc.data(), k.enc.size(), b, err), "valid block rejected: %s", err.c_str());
  const hsv_proposal &p = b.p;
  CHECK(std::memcmp(p.author, k.author, 32) == 0 && std::memcmp(p.signature, k.signature, 64) == 0 &&
            p.round == k.round,
        "block author / signature / round");
  CHECK(p.n_payload * 32 == k.payload.size() && b.payload == k.payload, "payload");
  CHECK(std::memcmp(p.qc_hash, k.qc.hash, 32) == 0 && p.qc_round == k.qc.round && p.n_qc == k.qc.n &&
            b.qc_votes == k.qc.votes,
        "embedded QC");
  CHECK((p.has_tc != 0) == k.has_tc, "Option tag");
  if (k.has_tc) CHECK(p.tc_round == k.tc_round && p.n_tc == k.n_tc && b.tc_votes == k.tc_votes, "embedded TC");
  assemble(b);
  // every strict prefix is truncated, every extension has trailing bytes
  for (size_t cut = 0; cut < k.enc.size(); ++cut) {
    hsvw::BlockParsed x;
    CHECK(!hsvw::parse_block(k.enc.data(), cut, x, err), "block prefix %zu accepted", cut);
  }
  Bytes ext = k.enc;
  ext.push_back(0);
  hsvw::BlockParsed x;
  CHECK(!hsvw::parse_block(ext.data(), ext.size(), x, err), "block with a trailing byte accepted");
  // any Option tag but 0 and 1
  for (int tag = 2; tag < 256; ++tag) {
    Bytes t = k.enc;
    t[k.tag_at] = (uint8_t)tag;
    CHECK(!hsvw::parse_block(t.data(), t.size(), x, err), "Option tag %d accepted", tag);
  }
}

Bytes make_timeout(std::mt19937_64 &rng, size_t n_qc, bool genesis) {
  const Qc q = make_qc(rng, n_qc, genesis);
  uint8_t author[32], sig[64];
  fill(rng, author, 32);
  fill(rng, sig, 64);
  const uint64_t round = rng() % 1000000;
  Bytes enc;
  put_qc(enc, q);
  put_u64(enc, round);
  put_key(enc, author);
  enc.insert(enc.end(), sig, sig + 64);
  hsvw::TimeoutParsed t;
  std::string err;
  CHECK(hsvw::parse_timeout(enc.data(), enc.size(), t, err), "valid timeout rejected: %s", err.c_str());
  CHECK(t.round == round && std::memcmp(t.author, author, 32) == 0 && std::memcmp(t.signature, sig, 64) == 0,
        "timeout fields");
  CHECK(t.n_qc == q.n && t.qc_votes == q.votes && t.qc_round == q.round && std::memcmp(t.qc_hash, q.hash, 32) == 0,
        "timeout high_qc");
  for (size_t cut = 0; cut < enc.size(); ++cut) {
    hsvw::TimeoutParsed x;
    CHECK(!hsvw::parse_timeout(enc.data(), cut, x, err), "timeout prefix %zu accepted", cut);
  }
  Bytes ext = enc;
  ext.push_back(7);
  CHECK(!hsvw::parse_timeout(ext.data(), ext.size(), t, err), "timeout with a trailing byte accepted");
  return enc;
}

Bytes make_vote(std::mt19937_64 &rng) {
  uint8_t hash[32], author[32], sig[64];
  fill(rng, hash, 32);
  fill(rng, author, 32);
  fill(rng, sig, 64);
  const uint64_t round = rng() % 1000000;
  Bytes enc(hash, hash + 32);
  put_u64(enc, round);
  put_key(enc, author);
  enc.insert(enc.end(), sig, sig + 64);
  hsvw::VoteParsed v;
  std::string err;
  CHECK(hsvw::parse_vote(enc.data(), enc.size(), v, err), "valid vote rejected: %s", err.c_str());
  uint8_t d[32];
  hsvp::qc_digest(hash, round, d);
  CHECK(v.round == round && std::memcmp(v.hash, hash, 32) == 0 && std::memcmp(v.author, author, 32) == 0 &&
            std::memcmp(v.signature, sig, 64) == 0 && std::memcmp(v.digest, d, 32) == 0,
        "vote fields");
  for (size_t cut = 0; cut < enc.size(); ++cut)
    CHECK(!hsvw::parse_vote(enc.data(), cut, v, err), "vote prefix %zu accepted", cut);
  Bytes ext = enc;
  ext.push_back(0);
  CHECK(!hsvw::parse_vote(ext.data(), ext.size(), v, err), "vote with a trailing byte accepted");
  return enc;
}

// parse anything; only the sanitizers judge (and a successful parse must be self-consistent)
void parse_any(const Bytes &b) {
  std::string err;
  hsvw::BlockParsed k;
  if (hsvw::parse_block(b.data(), b.size(), k, err)) {
    CHECK(k.qc_votes.size() == 96 * k.p.n_qc && k.payload.size() == 32 * k.p.n_payload &&
              (!k.p.has_tc || k.tc_votes.size() == 104 * k.p.n_tc),
          "block sizes");
    assemble(k);
  }
  hsvw::TimeoutParsed t;
  if (hsvw::parse_timeout(b.data(), b.size(), t, err)) CHECK(t.qc_votes.size() == 96 * t.n_qc, "timeout sizes");
  hsvw::VoteParsed v;
  (void)hsvw::parse_vote(b.data(), b.size(), v, err);
}

void set_u64(Bytes &b, size_t off, uint64_t v) {
  if (off + 8 > b.size()) return;
  for (int i = 0; i < 8; ++i) b[off + i] = (uint8_t)(v >> (8 * i));
}

Bytes mutate(const Bytes &in, std::mt19937_64 &rng, const std::vector<Bytes> &pool) {
  Bytes b = in;
  const int ops = 1 + (int)(rng() % 4);
  for (int k = 0; k < ops; ++k) {
    switch (rng() % 9) {
      case 0:  // bit flip
        if (!b.empty()) b[rng() % b.size()] ^= (uint8_t)(1u << (rng() % 8));
        break;
      case 1:  // random byte
        if (!b.empty()) b[rng() % b.size()] = (uint8_t)rng();
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
      case 5: {  // oversized / boundary u64 at a random offset
        static const uint64_t vals[] = {~0ull, 1ull << 63, 1ull << 32, 0xffffffffull, 44, 43, 45, 0, 1, 2,
                                        ~0ull / 32, ~0ull / 32 + 1, ~0ull / 96, ~0ull / 72 + 1, ~0ull / 80 + 1};
        set_u64(b, b.empty() ? 0 : rng() % b.size(), vals[rng() % (sizeof(vals) / sizeof(vals[0]))]);
        break;
      }
      case 6:  // bad base64 symbol / padding / Option tag inside the bytes
        if (!b.empty()) {
          static const uint8_t bad[] = {'=', '-', '_', ' ', '\n', 0, 1, 2, 0x80, '!', '/', '+'};
          b[rng() % b.size()] = bad[rng() % sizeof(bad)];
        }
        break;
      case 7: {  // splice with another input
        const Bytes &o = pool[rng() % pool.size()];
        if (!o.empty() && !b.empty()) {
          const size_t at = rng() % b.size(), from = rng() % o.size(), len = rng() % (o.size() - from + 1);
          b.resize(at);
          b.insert(b.end(), o.begin() + from, o.begin() + from + len);
        }
        break;
      }
      default:  // duplicate a chunk
        if (b.size() > 2) {
          const size_t a = rng() % b.size(), len = rng() % (b.size() - a);
          Bytes chunk(b.begin() + a, b.begin() + a + len);
          b.insert(b.begin() + a, chunk.begin(), chunk.end());
        }
    }
  }
  return b;
}

}  // namespace

int main(int argc, char **argv) {
  const long iters = argc > 1 ? std::atol(argv[1]) : 100000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261020);
  std::vector<Bytes> pool;
  struct Shape {
    size_t n_qc;
    bool genesis, has_tc;
    size_t n_tc, n_payload;
  };
  const Shape shapes[] = {{0, true, false, 0, 0}, {3, false, false, 0, 3}, {3, false, true, 3, 0},
                          {2, true, true, 1, 1},  {0, false, true, 0, 2},  {5, false, true, 4, 3}};
  for (const Shape &s : shapes) {
    const Block k = make_block(rng, s.n_qc, s.genesis, s.has_tc, s.n_tc, s.n_payload);
    check_valid_block(k);
    pool.push_back(k.enc);
  }
  for (size_t n : {0, 1, 3}) {
    pool.push_back(make_timeout(rng, n, false));
    pool.push_back(make_timeout(rng, n, true));
  }
  pool.push_back(make_vote(rng));
  pool.push_back(Bytes());
  for (long i = 0; i < iters; ++i) parse_any(mutate(pool[rng() % pool.size()], rng, pool));
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("proposal fuzz ok: %ld mutated inputs, %zu seeds\n", iters, pool.size());
  return 0;
}
