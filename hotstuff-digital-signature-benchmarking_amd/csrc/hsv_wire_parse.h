// Parsers of the consensus messages' bincode bytes (no GPU code): the part of
// hsv_qc_verify_bincode / hsv_tc_verify_bincode and of the block, timeout and
// vote calls (hsv_proposal.cpp) that reads untrusted network bytes (the
// reference receives them as TCP frames, network/src/receiver.rs:47-60,
// consensus/src/consensus.rs:32-39).  Kept in its own translation unit so
// tests/native/wire_fuzz.cpp and tests/native/proposal_fuzz.cpp can build it
// alone under AddressSanitizer / UndefinedBehaviorSanitizer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "hsv.h"

namespace hsvw {

// consensus::QC (consensus/src/messages.rs:162-167) -> packed pk||R||s votes
// and qc.digest() = SHA-512(hash || round_le)[..32] (messages.rs:201-207).
struct QcParsed {
  uint8_t digest[32];
  uint64_t round = 0;
  std::vector<uint8_t> votes;  // n * 96
  size_t n = 0;
};

// consensus::TC (messages.rs:281-285) -> per-vote pk, sig and digest
// SHA-512(round_le || high_qc_round_le)[..32] (messages.rs:306-313).
struct TcParsed {
  uint64_t round = 0;
  std::vector<uint8_t> pks, sigs, digests;  // n * 32, n * 64, n * 32
  size_t n = 0;
};

// consensus::Block (messages.rs:16-24) as the plain-data proposal of hsv.h;
// p's pointers point into the vectors beside it (valid until the next parse
// into this object).
struct BlockParsed {
  hsv_proposal p{};
  std::vector<uint8_t> payload, qc_votes, tc_votes;  // n_payload * 32, n_qc * 96, n_tc * 104
};

// consensus::Timeout (messages.rs:222-228)
struct TimeoutParsed {
  uint8_t author[32], signature[64];
  uint64_t round = 0;
  uint8_t qc_hash[32];
  uint64_t qc_round = 0;
  std::vector<uint8_t> qc_votes;  // n_qc * 96
  size_t n_qc = 0;
};

// consensus::Vote (messages.rs:112-118) and vote.digest() =
// SHA-512(hash || round_le)[..32] (messages.rs:149-156)
struct VoteParsed {
  uint8_t hash[32], author[32], signature[64], digest[32];
  uint64_t round = 0;
};

// true on success; on failure `err` says what was malformed
bool parse_qc(const uint8_t *buf, size_t len, QcParsed &out, std::string &err);
bool parse_tc(const uint8_t *buf, size_t len, TcParsed &out, std::string &err);
bool parse_block(const uint8_t *buf, size_t len, BlockParsed &out, std::string &err);
bool parse_timeout(const uint8_t *buf, size_t len, TimeoutParsed &out, std::string &err);
bool parse_vote(const uint8_t *buf, size_t len, VoteParsed &out, std::string &err);

// mempool::MempoolMessage::Batch(Vec<Vec<u8>>) as BatchMaker::seal serializes it
// (mempool/src/batch_maker.rs:127-131) and Core::make_vote reads it back
// (consensus/src/core.rs:113-142): u32 LE variant tag (0 = Batch) | u64 count |
// count x (u64 length, bytes).  n_tx: the count; spans (optional): transaction
// i is buf[s[2i] - base, s[2i+1] - base) for the 2 * n_tx entries s appended to
// it (nothing is appended on failure).  Malformed: a tag other than 0 (a
// BatchRequest is tag 1), truncation, a count above the remaining bytes / 8, a
// length past the buffer's end, trailing bytes -- the rules of the device walk
// (hsv_batchscan.hpp), which tests/native/batchscan_host.cpp holds against
// this function.
bool parse_batch(const uint8_t *buf, size_t len, uint64_t base, std::vector<uint64_t> *spans, size_t &n_tx,
                 std::string &err);

// base64 0.13 standard decoding (PublicKey::decode_base64, crypto/src/lib.rs:73-79)
bool b64_decode(const uint8_t *s, size_t n, std::vector<uint8_t> &out);

}  // namespace hsvw
