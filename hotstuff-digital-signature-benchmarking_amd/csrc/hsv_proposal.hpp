// A proposal (Block), a Timeout or a chain of blocks as ONE verification batch
// with mixed digests and mixed acceptance rules, and the batch's flags back
// into the reference's verdict (hsv_proposal_verify and the *_bincode calls
// around it, hsv_proposal.cpp).  Pure host code without a HIP include, like
// hsv_batch.hpp and hsv_keyindex.hpp: tests/native/proposal_host.cpp builds it
// with plain g++.
//
// Item order of one object: the author's signature, the embedded QC's votes
// (none when the QC equals QC::genesis(): hash and round both zero,
// consensus/src/messages.rs:216-220, whatever votes it carries), the embedded
// TC's votes.  Rules: author and TC votes HSV_STRICT_OK (Signature::verify),
// QC votes HSV_PARSE_OK and HSV_EQ_OK (Signature::verify_batch).  The first
// failing stage in that order is the verdict, with its lowest failing vote.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hsv.h"
#include "hsv_sha512.hpp"

namespace hsvp {

inline void put_le64(uint8_t *p, uint64_t v) {
  for (int b = 0; b < 8; ++b) p[b] = (uint8_t)(v >> (8 * b));
}

inline uint64_t get_le64(const uint8_t *p) {
  uint64_t v = 0;
  for (int b = 7; b >= 0; --b) v = (v << 8) | p[b];
  return v;
}

// Block::digest (messages.rs:80-89): SHA-512(author || round_le || payload... || qc.hash)[..32].
// `scratch` keeps its capacity from call to call.
inline void block_digest(const uint8_t author[32], uint64_t round, const uint8_t *payload, size_t n_payload,
                         const uint8_t qc_hash[32], std::vector<uint8_t> &scratch, uint8_t out[32]) {
  scratch.resize(72 + 32 * n_payload);
  uint8_t *p = scratch.data();
  std::memcpy(p, author, 32);
  put_le64(p + 32, round);
  if (n_payload) std::memcpy(p + 40, payload, 32 * n_payload);
  std::memcpy(p + 40 + 32 * n_payload, qc_hash, 32);
  uint8_t h[64];
  hsv::sha512_bytes(p, scratch.size(), h);
  std::memcpy(out, h, 32);
}

// QC::digest and Vote::digest (messages.rs:201-207, 149-156): SHA-512(hash || round_le)[..32]
inline void qc_digest(const uint8_t hash[32], uint64_t round, uint8_t out[32]) {
  uint8_t pre[40], h[64];
  std::memcpy(pre, hash, 32);
  put_le64(pre + 32, round);
  hsv::sha512_bytes(pre, sizeof(pre), h);
  std::memcpy(out, h, 32);
}

// Timeout::digest and a TC vote's digest (messages.rs:268-275, 306-313):
// SHA-512(round_le || high_qc_round_le)[..32]
inline void timeout_digest(uint64_t round, uint64_t high_qc_round, uint8_t out[32]) {
  uint8_t pre[16], h[64];
  put_le64(pre, round);
  put_le64(pre + 8, high_qc_round);
  hsv::sha512_bytes(pre, sizeof(pre), h);
  std::memcpy(out, h, 32);
}

// The digests of one TC's votes depend only on (round, high_qc_round), and a
// TC's high_qc_rounds take few distinct values (the last rounds before a
// timeout): each is hashed once.  A small array searched from the last hit,
// not a hash map -- no allocation per call, and a C3 TC's 667 lookups cost a
// few compares each (the map made the parse ~28 us of a 0.092 ms bincode TC on
// the GPU box, profiles/r05e_bench_detail.json).  Beyond kSlots distinct values
// every new one is hashed.
class TcDigestMemo {
 public:
  explicit TcDigestMemo(uint64_t round) : round_(round) {}
  void digest(uint64_t high_qc_round, uint8_t out[32]) {
    size_t k = last_;
    if (n_ == 0 || key_[k] != high_qc_round) {
      for (k = 0; k < n_ && key_[k] != high_qc_round; ++k) {
      }
    }
    if (k < n_) {
      last_ = k;
      std::memcpy(out, dig_[k], 32);
      return;
    }
    timeout_digest(round_, high_qc_round, out);
    if (n_ < kSlots) {
      key_[n_] = high_qc_round;
      std::memcpy(dig_[n_], out, 32);
      last_ = n_++;
    }
  }

 private:
  static constexpr size_t kSlots = 32;
  uint64_t round_;
  uint64_t key_[kSlots];
  uint8_t dig_[kSlots][32];
  size_t n_ = 0, last_ = 0;
};

inline bool qc_is_genesis(const uint8_t hash[32], uint64_t round) {
  uint8_t acc = 0;
  for (int i = 0; i < 32; ++i) acc |= hash[i];
  return acc == 0 && round == 0;
}

// One verification batch: parallel arrays as hsv_verify takes them (msg_stride 32).
struct Items {
  std::vector<uint8_t> pk, sig, msg;  // n * 32, n * 64, n * 32
  size_t n = 0;
  void clear() {
    pk.clear();
    sig.clear();
    msg.clear();
    n = 0;
  }
  // room for k more items; returns the index of the first
  size_t grow(size_t k) {
    const size_t first = n;
    n += k;
    pk.resize(n * 32);
    sig.resize(n * 64);
    msg.resize(n * 32);
    return first;
  }
  void set(size_t i, const uint8_t *key, const uint8_t *rs, const uint8_t *digest) {
    std::memcpy(pk.data() + 32 * i, key, 32);
    std::memcpy(sig.data() + 64 * i, rs, 64);
    std::memcpy(msg.data() + 32 * i, digest, 32);
  }
};

// Where one object's items lie in the batch.  n_qc and n_tc are the vote
// counts the object carries; qc_items is 0 for a skipped (genesis) QC.
struct Layout {
  size_t first = 0;  // the author's item
  size_t n_qc = 0, n_tc = 0;
  size_t qc_items = 0;
  size_t items() const { return 1 + qc_items + n_tc; }
};

// The author item and the embedded certificates of one object.  Block: the
// author's digest is block_digest and has_tc as the block says; Timeout: the
// author's digest is timeout_digest(round, high_qc.round) and there is no TC.
struct Object {
  const uint8_t *author = nullptr;     // 32
  const uint8_t *signature = nullptr;  // 64
  uint8_t author_digest[32];
  const uint8_t *qc_hash = nullptr;  // 32
  uint64_t qc_round = 0;
  const uint8_t *qc_votes = nullptr;  // n_qc * 96: pk || R || s
  size_t n_qc = 0;
  bool has_tc = false;
  uint64_t tc_round = 0;
  const uint8_t *tc_votes = nullptr;  // n_tc * 104: pk || R || s || high_qc_round_le
  size_t n_tc = 0;
};

inline Object object_of(const hsv_proposal &p, std::vector<uint8_t> &scratch) {
  Object o;
  o.author = p.author;
  o.signature = p.signature;
  block_digest(p.author, p.round, p.payload, p.n_payload, p.qc_hash, scratch, o.author_digest);
  o.qc_hash = p.qc_hash;
  o.qc_round = p.qc_round;
  o.qc_votes = p.qc_votes;
  o.n_qc = p.n_qc;
  o.has_tc = p.has_tc != 0;
  o.tc_round = p.tc_round;
  o.tc_votes = o.has_tc ? p.tc_votes : nullptr;
  o.n_tc = o.has_tc ? p.n_tc : 0;
  return o;
}

// Appends the object's items to the batch.
inline Layout append(const Object &o, Items &it) {
  Layout l;
  l.n_qc = o.n_qc;
  l.n_tc = o.n_tc;
  l.qc_items = qc_is_genesis(o.qc_hash, o.qc_round) ? 0 : o.n_qc;
  l.first = it.grow(l.items());
  size_t i = l.first;
  it.set(i++, o.author, o.signature, o.author_digest);
  if (l.qc_items) {
    uint8_t d[32];
    qc_digest(o.qc_hash, o.qc_round, d);
    for (size_t v = 0; v < o.n_qc; ++v, ++i) it.set(i, o.qc_votes + 96 * v, o.qc_votes + 96 * v + 32, d);
  }
  if (o.n_tc) {
    TcDigestMemo memo(o.tc_round);
    uint8_t d[32];
    for (size_t v = 0; v < o.n_tc; ++v, ++i) {
      const uint8_t *r = o.tc_votes + 104 * v;
      memo.digest(get_le64(r + 96), d);
      it.set(i, r, r + 32, d);
    }
  }
  return l;
}

inline bool strict_ok(uint8_t f) { return (f & HSV_STRICT_OK) != 0; }
inline bool batch_ok(uint8_t f) { return (f & (HSV_PARSE_OK | HSV_EQ_OK)) == (HSV_PARSE_OK | HSV_EQ_OK); }

// The reference's verdict from the batch's flags (flags[l.first ..] are the
// object's): first failing stage, lowest failing vote in it.
inline hsv_proposal_result reduce(const Layout &l, const uint8_t *flags) {
  const uint8_t *f = flags + l.first;
  if (!strict_ok(f[0])) return {HSV_STAGE_AUTHOR, 0};
  for (size_t v = 0; v < l.qc_items; ++v)
    if (!batch_ok(f[1 + v])) return {HSV_STAGE_QC, (uint32_t)v};
  for (size_t v = 0; v < l.n_tc; ++v)
    if (!strict_ok(f[1 + l.qc_items + v])) return {HSV_STAGE_TC, (uint32_t)v};
  return {HSV_STAGE_OK, 0};
}

// The object's raw flags as the caller sees them: 1 + n_qc + n_tc bytes in the
// order author, QC votes, TC votes; a skipped QC's votes read 0.
inline void scatter_flags(const Layout &l, const uint8_t *flags, uint8_t *out) {
  const uint8_t *f = flags + l.first;
  out[0] = f[0];
  if (l.qc_items) std::memcpy(out + 1, f + 1, l.n_qc);
  else if (l.n_qc) std::memset(out + 1, 0, l.n_qc);
  if (l.n_tc) std::memcpy(out + 1 + l.n_qc, f + 1 + l.qc_items, l.n_tc);
}

}  // namespace hsvp
