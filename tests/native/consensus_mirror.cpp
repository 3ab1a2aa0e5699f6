// The consensus half of the C++ mirror (include/hsv_crypto.hpp, namespace
// consensus): Block, Vote and Timeout whose signature checks make one
// verification call each (tests/test_consensus_mirror.py).  Keys and
// signatures are made here with the crate mirror's own signer; the digests
// come from csrc/hsv_proposal.hpp.  Without a GPU the first verify throws
// crypto::InfrastructureError, which is reported on stderr (exit status 3).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hsv_crypto.hpp"
#include "hsv_proposal.hpp"

namespace {

int failures = 0;
#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                                                  \
    }                                                                              \
  } while (0)

struct Key {
  crypto::PublicKey pk;
  crypto::SecretKey sk;
};

Key make_key(uint8_t tag) {
  auto kp = crypto::generate_keypair([tag](uint8_t *p, size_t n) { std::memset(p, tag, n); });
  return Key{kp.first, kp.second};
}

crypto::Signature sign(const Key &k, const uint8_t digest[32]) {
  crypto::Digest d;
  std::memcpy(d.bytes.data(), digest, 32);
  return crypto::Signature::sign(d, k.sk);
}

bool at(const consensus::Verdict &v, uint32_t stage, uint32_t index) {
  return v.is_ok() == (stage == HSV_STAGE_OK) && v.where.stage == stage && v.where.index == index;
}

void run(const std::vector<Key> &keys, hsv_committee *c) {
  const Key &author = keys[3];
  uint8_t d[32];
  std::vector<uint8_t> pre;

  consensus::Block b;
  std::memset(b.qc.hash.bytes.data(), 0x5a, 32);
  b.qc.round = 8;
  hsvp::qc_digest(b.qc.hash.bytes.data(), b.qc.round, d);
  for (int i = 0; i < 3; ++i) b.qc.votes.emplace_back(keys[i].pk, sign(keys[i], d));
  b.has_tc = true;
  b.tc.round = 8;
  for (int i = 0; i < 3; ++i) {
    hsvp::timeout_digest(b.tc.round, 6 + i % 2, d);
    b.tc.votes.push_back({keys[i].pk, sign(keys[i], d), (consensus::Round)(6 + i % 2)});
  }
  b.author = author.pk;
  b.round = 9;
  b.payload.resize(2);
  std::memset(b.payload[0].bytes.data(), 1, 32);
  std::memset(b.payload[1].bytes.data(), 2, 32);
  std::vector<uint8_t> pay(64);
  std::memset(pay.data(), 1, 32);
  std::memset(pay.data() + 32, 2, 32);
  hsvp::block_digest(b.author.bytes.data(), b.round, pay.data(), 2, b.qc.hash.bytes.data(), pre, d);
  b.signature = sign(author, d);

  CHECK(at(b.verify_signatures(c), HSV_STAGE_OK, 0));  // without a GPU this throws
  {
    consensus::Block x = b;
    x.round ^= 1;
    CHECK(at(x.verify_signatures(c), HSV_STAGE_AUTHOR, 0));
    x = b;
    x.qc.votes[2].second.part2[3] ^= 4;
    CHECK(at(x.verify_signatures(c), HSV_STAGE_QC, 2));
    x.tc.votes[0].signature.part1[0] ^= 1;  // the QC still fails first
    CHECK(at(x.verify_signatures(c), HSV_STAGE_QC, 2));
    x = b;
    x.tc.votes[1].high_qc_round += 1;
    CHECK(at(x.verify_signatures(c), HSV_STAGE_TC, 1));
    x.has_tc = false;  // tc: None -- its votes are not looked at
    CHECK(at(x.verify_signatures(c), HSV_STAGE_OK, 0));
  }
  {  // the genesis QC is skipped whatever votes it carries
    consensus::Block g = b;
    g.qc.hash = crypto::Digest();
    g.qc.round = 0;
    g.qc.votes[1].second.part2[0] ^= 1;
    hsvp::block_digest(g.author.bytes.data(), g.round, pay.data(), 2, g.qc.hash.bytes.data(), pre, d);
    g.signature = sign(author, d);
    CHECK(at(g.verify_signatures(c), HSV_STAGE_OK, 0));
  }

  consensus::Vote v;
  v.hash = b.qc.hash;
  v.round = 9;
  v.author = keys[1].pk;
  hsvp::qc_digest(v.hash.bytes.data(), v.round, d);
  v.signature = sign(keys[1], d);
  CHECK(v.verify_signature(c).is_ok());
  v.round = 10;
  CHECK(v.verify_signature(c).is_err());

  consensus::Timeout t;
  t.high_qc = b.qc;
  t.round = 12;
  t.author = author.pk;
  hsvp::timeout_digest(t.round, t.high_qc.round, d);
  t.signature = sign(author, d);
  CHECK(at(t.verify_signatures(c), HSV_STAGE_OK, 0));
  t.high_qc.votes[0].second.part1[5] ^= 2;
  CHECK(at(t.verify_signatures(c), HSV_STAGE_QC, 0));
  t.signature.part2[1] ^= 1;
  CHECK(at(t.verify_signatures(c), HSV_STAGE_AUTHOR, 0));
}

}  // namespace

int main() {
  try {
    std::vector<Key> keys;
    std::vector<crypto::PublicKey> pks;
    for (uint8_t i = 0; i < 4; ++i) {
      keys.push_back(make_key((uint8_t)(0x10 + i)));
      pks.push_back(keys.back().pk);
    }
    run(keys, nullptr);
    hsv::Committee committee(pks);
    run(keys, committee.handle());
  } catch (const crypto::InfrastructureError &e) {
    std::fprintf(stderr, "InfrastructureError: %s\n", e.what());
    return 3;
  }
  if (failures) return 1;
  std::printf("consensus mirror ok\n");
  return 0;
}
