// hsv_crypto.hpp -- C++ mirror of the reference's `crypto` crate over the C ABI.
//
// The reference (mwaurawakati/hotstuff-digital-signature-benchmarking) is Rust;
// no Rust toolchain exists in this image, so the host side above libhsv's C
// ABI is written in C++ with the crate's names, byte layouts, argument meaning
// and error behaviour (reference crypto/src/lib.rs):
//
//   Digest(pub [u8;32])                       lib.rs:22      -> crypto::Digest
//   PublicKey(pub [u8;32]) + base64 serde     lib.rs:66-118  -> crypto::PublicKey
//   SecretKey([u8;64]), zeroed on drop        lib.rs:121-161 -> crypto::SecretKey
//   generate_keypair(csprng)                  lib.rs:167-175 -> crypto::generate_keypair
//   Signature{part1, part2}                   lib.rs:179-182 -> crypto::Signature
//   Signature::new / from_bytes / flatten     lib.rs:185-202
//   Signature::verify        -> Result        lib.rs:204-208 (verify_strict semantics)
//   Signature::verify_batch  -> Result        lib.rs:210-223
//   SignatureService::request_signature       lib.rs:229-254 -> crypto::SignatureService
// and, of consensus/src/messages.rs, the signature half of
//   Block::verify / Vote::verify / Timeout::verify   55-76, 136-146, 250-265
//                                              -> consensus::Block / Vote / Timeout
// (one verification call per object: hsv_proposal_verify,
// hsv_vote_verify_bincode, hsv_timeout_verify_bincode).
//
// `Result` carries Ok or Err(CryptoError) exactly like Result<(), CryptoError>.
// An infrastructure failure (no GPU, HIP error) is NOT an Err: by default it
// throws crypto::InfrastructureError, so a broken device can never look like a
// rejected signature.  A deployment that must keep running through a device
// fault installs an InfrastructureFallback (set_infrastructure_fallback): a
// host verifier with the same semantics (ed25519-dalek in the Rust shim,
// INTEGRATION.md section 2) that is consulted ONLY for calls libhsv could not
// run, never to second-guess a rejection; every use is counted.  libhsv itself
// has no CPU path.
#ifndef HSV_CRYPTO_HPP_
#define HSV_CRYPTO_HPP_

#include <array>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "hsv.h"

namespace crypto {

class InfrastructureError : public std::runtime_error {
 public:
  explicit InfrastructureError(const std::string &what) : std::runtime_error(what) {}
};

inline int check_infra(int rc, const char *what) {
  if (rc < 0) throw InfrastructureError(std::string(what) + ": " + hsv_last_error());
  return rc;
}

// Infrastructure-failure policy of the caller (see the header comment).
// Install once at startup, before verify calls run on other threads.
struct InfrastructureFallback {
  // verify_strict over one 32-byte digest; true = Ok
  std::function<bool(const uint8_t *digest, const uint8_t *pk, const uint8_t *sig)> verify_strict;
  // the deterministic verify_batch rule over packed 96-byte pk || R || s votes
  std::function<bool(const uint8_t *digest, const uint8_t *votes, size_t n)> verify_batch;
};

inline InfrastructureFallback &infrastructure_fallback() {
  static InfrastructureFallback f;
  return f;
}
inline std::atomic<uint64_t> &infrastructure_fallback_uses() {
  static std::atomic<uint64_t> n{0};
  return n;
}
inline void set_infrastructure_fallback(InfrastructureFallback f) { infrastructure_fallback() = std::move(f); }

// Latency routing of the caller.
// One signature on the GPU costs a launch plus one dependent root chain
// (0.0395 ms for a cached committee key, 0.0357 ms through the resident
// service), one host core 0.037 ms (dalek port); a 3-vote QC is 0.04 ms on the
// GPU against 0.077 ms on the host.  A
// deployment installs a host verifier with the same semantics (dalek in the
// Rust shim) and a size limit: verify calls and verify_batch calls of at most
// max_batch votes go to it, everything larger to libhsv.  Unlike the
// infrastructure fallback this is a routing choice made before the call --
// libhsv's verdicts are never second-guessed.  Every routed call is counted.
struct HostRoute {
  size_t max_batch = 0;  // verify_batch calls of at most this many votes go to the host
  bool single = false;   // Signature::verify goes to the host
  std::function<bool(const uint8_t *digest, const uint8_t *pk, const uint8_t *sig)> verify_strict;
  std::function<bool(const uint8_t *digest, const uint8_t *votes, size_t n)> verify_batch;
};

inline HostRoute &host_route() {
  static HostRoute r;
  return r;
}
inline std::atomic<uint64_t> &host_route_uses() {
  static std::atomic<uint64_t> n{0};
  return n;
}
// Install once at startup, before verify calls run on other threads.
inline void set_host_route(HostRoute r) { host_route() = std::move(r); }

// The single-verify routing default (the Rust
// shim's hsv_single_on_host): a lone signature goes to libhsv, whose resident
// latency service is on by default (one cached-key verify_strict 0.034 ms
// against 0.036-0.037 ms for the dalek port on one host core,
// profiles/r05ah_bench.json).  It stays on the host only when the service is
// turned off (HSV_QC_RESIDENT=0: launched, 0.039 ms).  HSV_ROUTE_SINGLE =
// "gpu" / "host" overrides it.
inline bool single_verify_on_host_default() {
  if (const char *v = std::getenv("HSV_ROUTE_SINGLE")) return std::strcmp(v, "gpu") != 0;
  const char *r = std::getenv("HSV_QC_RESIDENT");
  return r && r[0] == '0';
}

// ed25519::Error: opaque.
struct CryptoError {
  std::string message = "signature error";
};

// Result<(), CryptoError>
class Result {
 public:
  static Result ok() { return Result(true); }
  static Result err() { return Result(false); }
  bool is_ok() const { return ok_; }
  bool is_err() const { return !ok_; }
  CryptoError unwrap_err() const { return CryptoError{}; }

 private:
  explicit Result(bool ok) : ok_(ok) {}
  bool ok_;
};

namespace detail {
inline std::string b64encode(const uint8_t *p, size_t n) {
  static const char *tbl = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  std::string out;
  for (size_t i = 0; i < n; i += 3) {
    uint32_t v = (uint32_t)p[i] << 16;
    if (i + 1 < n) v |= (uint32_t)p[i + 1] << 8;
    if (i + 2 < n) v |= p[i + 2];
    out += tbl[(v >> 18) & 63];
    out += tbl[(v >> 12) & 63];
    out += i + 1 < n ? tbl[(v >> 6) & 63] : '=';
    out += i + 2 < n ? tbl[v & 63] : '=';
  }
  return out;
}

inline std::vector<uint8_t> b64decode(const std::string &s) {
  auto val = [](char c) -> int {
    if (c >= 'A' && c <= 'Z') return c - 'A';
    if (c >= 'a' && c <= 'z') return c - 'a' + 26;
    if (c >= '0' && c <= '9') return c - '0' + 52;
    if (c == '+') return 62;
    if (c == '/') return 63;
    return -1;
  };
  std::vector<uint8_t> out;
  uint32_t buf = 0;
  int bits = 0;
  for (char c : s) {
    if (c == '=') break;
    const int v = val(c);
    if (v < 0) throw std::invalid_argument("base64: invalid symbol");
    buf = (buf << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      out.push_back((uint8_t)(buf >> bits));
    }
  }
  return out;
}
}  // namespace detail

struct Digest {
  std::array<uint8_t, 32> bytes{};
  std::vector<uint8_t> to_vec() const { return {bytes.begin(), bytes.end()}; }
  size_t size() const { return bytes.size(); }
  bool operator==(const Digest &o) const { return bytes == o.bytes; }
};

struct PublicKey {
  std::array<uint8_t, 32> bytes{};
  std::string encode_base64() const { return detail::b64encode(bytes.data(), 32); }
  static PublicKey decode_base64(const std::string &s) {
    const std::vector<uint8_t> raw = detail::b64decode(s);
    if (raw.size() < 32) throw std::invalid_argument("InvalidLength");
    PublicKey k;
    std::memcpy(k.bytes.data(), raw.data(), 32);
    return k;
  }
  bool operator==(const PublicKey &o) const { return bytes == o.bytes; }
  bool operator<(const PublicKey &o) const { return bytes < o.bytes; }
};

// 64 bytes: secret seed (32) || public key (32); zeroed on destruction.
class SecretKey {
 public:
  SecretKey() = default;
  explicit SecretKey(const std::array<uint8_t, 64> &b) : bytes_(b) {}
  SecretKey(const SecretKey &) = default;
  SecretKey &operator=(const SecretKey &) = default;
  ~SecretKey() {
    volatile uint8_t *p = bytes_.data();
    for (size_t i = 0; i < bytes_.size(); ++i) p[i] = 0;
  }
  std::string encode_base64() const { return detail::b64encode(bytes_.data(), 64); }
  static SecretKey decode_base64(const std::string &s) {
    const std::vector<uint8_t> raw = detail::b64decode(s);
    if (raw.size() < 64) throw std::invalid_argument("InvalidLength");
    std::array<uint8_t, 64> b{};
    std::memcpy(b.data(), raw.data(), 64);
    return SecretKey(b);
  }
  const uint8_t *seed() const { return bytes_.data(); }
  bool operator==(const SecretKey &o) const { return bytes_ == o.bytes_; }

 private:
  std::array<uint8_t, 64> bytes_{};
};

// generate_keypair(csprng): `fill` writes 32 secret bytes (dalek SecretKey::generate).
inline std::pair<PublicKey, SecretKey> generate_keypair(const std::function<void(uint8_t *, size_t)> &fill) {
  std::array<uint8_t, 64> sk{};
  fill(sk.data(), 32);
  PublicKey pk;
  check_infra(hsv_public_key(sk.data(), pk.bytes.data()), "hsv_public_key");
  std::memcpy(sk.data() + 32, pk.bytes.data(), 32);
  return {pk, SecretKey(sk)};
}

class Signature {
 public:
  std::array<uint8_t, 32> part1{};  // R
  std::array<uint8_t, 32> part2{};  // s

  Signature() = default;  // Signature::default(): 64 zero bytes

  // Signature::new (lib.rs:185-191): RFC 8032 over digest.0
  static Signature sign(const Digest &digest, const SecretKey &secret) {
    uint8_t out[64];
    check_infra(hsv_sign(secret.seed(), digest.bytes.data(), 32, out), "hsv_sign");
    Signature s;
    std::memcpy(s.part1.data(), out, 32);
    std::memcpy(s.part2.data(), out + 32, 32);
    return s;
  }

  static Signature from_bytes(const std::array<uint8_t, 32> &p1, const std::array<uint8_t, 32> &p2) {
    Signature s;
    s.part1 = p1;
    s.part2 = p2;
    return s;
  }

  std::array<uint8_t, 64> flatten() const {
    std::array<uint8_t, 64> f{};
    std::memcpy(f.data(), part1.data(), 32);
    std::memcpy(f.data() + 32, part2.data(), 32);
    return f;
  }

  // Signature::verify (lib.rs:204-208): ed25519-dalek verify_strict semantics.
  Result verify(const Digest &digest, const PublicKey &public_key) const {
    const std::array<uint8_t, 64> f = flatten();
    const HostRoute &route = host_route();
    if (route.single && route.verify_strict) {
      ++host_route_uses();
      return route.verify_strict(digest.bytes.data(), public_key.bytes.data(), f.data()) ? Result::ok()
                                                                                         : Result::err();
    }
    int rc = hsv_verify_strict(digest.bytes.data(), public_key.bytes.data(), f.data());
    if (rc < 0 && infrastructure_fallback().verify_strict) {
      ++infrastructure_fallback_uses();
      rc = infrastructure_fallback().verify_strict(digest.bytes.data(), public_key.bytes.data(), f.data()) ? 1 : 0;
    }
    check_infra(rc, "hsv_verify_strict");
    return rc == 1 ? Result::ok() : Result::err();
  }

  // Signature::verify_batch (lib.rs:210-223): every vote signs the same digest.
  static Result verify_batch(const Digest &digest, const std::vector<std::pair<PublicKey, Signature>> &votes) {
    std::vector<uint8_t> packed(votes.size() * 96);
    for (size_t i = 0; i < votes.size(); ++i) {
      std::memcpy(packed.data() + 96 * i, votes[i].first.bytes.data(), 32);
      std::memcpy(packed.data() + 96 * i + 32, votes[i].second.part1.data(), 32);
      std::memcpy(packed.data() + 96 * i + 64, votes[i].second.part2.data(), 32);
    }
    const HostRoute &route = host_route();
    if (votes.size() <= route.max_batch && route.verify_batch) {
      ++host_route_uses();
      return route.verify_batch(digest.bytes.data(), packed.data(), votes.size()) ? Result::ok() : Result::err();
    }
    int rc = hsv_verify_batch_packed(digest.bytes.data(), packed.data(), votes.size());
    if (rc < 0 && infrastructure_fallback().verify_batch) {
      ++infrastructure_fallback_uses();
      rc = infrastructure_fallback().verify_batch(digest.bytes.data(), packed.data(), votes.size()) ? 1 : 0;
    }
    check_infra(rc, "hsv_verify_batch_packed");
    return rc == 1 ? Result::ok() : Result::err();
  }

  // Signatures over whole messages of any length (hsv_verify_msgs; RFC 8032
  // PureEdDSA, what hsv::Signer::sign produces): item i is items[i] over
  // msgs[i].  Returns the per-item HSV_* flag bytes (HSV_STRICT_OK = dalek's
  // verify_strict Ok).  GPU only: no host route and no fallback.
  static std::vector<uint8_t> verify_msgs(const std::vector<std::pair<PublicKey, Signature>> &items,
                                          const std::vector<std::vector<uint8_t>> &msgs) {
    if (msgs.size() != items.size()) throw std::invalid_argument("verify_msgs: one message per item");
    const size_t n = items.size();
    std::vector<uint8_t> pk(n * 32), sig(n * 64), buf, flags(n);
    std::vector<uint64_t> offsets(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(pk.data() + 32 * i, items[i].first.bytes.data(), 32);
      std::memcpy(sig.data() + 64 * i, items[i].second.part1.data(), 32);
      std::memcpy(sig.data() + 64 * i + 32, items[i].second.part2.data(), 32);
      buf.insert(buf.end(), msgs[i].begin(), msgs[i].end());
      offsets[i + 1] = buf.size();
    }
    check_infra(hsv_verify_msgs(pk.data(), sig.data(), buf.data(), offsets.data(), 0, 0, n, flags.data()),
                "hsv_verify_msgs");
    return flags;
  }
};

// SignatureService (lib.rs:229-254): a worker owns the secret key and answers
// signature requests in order (tokio task + mpsc(100) in the reference).
class SignatureService {
 public:
  explicit SignatureService(SecretKey secret) : secret_(std::move(secret)), worker_([this] { run(); }) {}
  ~SignatureService() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    worker_.join();
  }
  std::future<Signature> request_signature(const Digest &digest) {
    std::promise<Signature> p;
    std::future<Signature> f = p.get_future();
    {
      std::lock_guard<std::mutex> lk(mu_);
      queue_.emplace_back(digest, std::move(p));
    }
    cv_.notify_one();
    return f;
  }

 private:
  void run() {
    for (;;) {
      std::pair<Digest, std::promise<Signature>> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
        if (queue_.empty()) return;
        job = std::move(queue_.front());
        queue_.pop_front();
      }
      try {
        job.second.set_value(Signature::sign(job.first, secret_));
      } catch (...) {
        job.second.set_exception(std::current_exception());
      }
    }
  }
  SecretKey secret_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<Digest, std::promise<Signature>>> queue_;
  bool stop_ = false;
  std::thread worker_;
};

}  // namespace crypto

// The signature half of the reference's consensus messages
// (consensus/src/messages.rs): Block::verify, Vote::verify and Timeout::verify
// with every signature of the object in ONE verification call
// (hsv_proposal_verify and the calls around it, hsv.h) instead of one call per
// embedded certificate.  The stake, quorum and authority-reuse checks of the
// reference stay with the caller and run before these, as in the reference.
// GPU only: no host route and no fallback, errors throw
// crypto::InfrastructureError.  `committee` (optional): an hsv_committee whose
// members the signers are; votes are then verified by member index.
namespace consensus {

using Round = uint64_t;

// messages.rs:164-169
struct QC {
  crypto::Digest hash;
  Round round = 0;
  std::vector<std::pair<crypto::PublicKey, crypto::Signature>> votes;
};

// messages.rs:283-287
struct TC {
  Round round = 0;
  struct Vote {
    crypto::PublicKey author;
    crypto::Signature signature;
    Round high_qc_round = 0;
  };
  std::vector<Vote> votes;
};

// Where a rejected object fails: the first failing stage in the reference's
// order (HSV_STAGE_AUTHOR, HSV_STAGE_QC, HSV_STAGE_TC) and its lowest failing vote.
struct Verdict {
  crypto::Result result = crypto::Result::ok();
  hsv_proposal_result where{HSV_STAGE_OK, 0};
  bool is_ok() const { return result.is_ok(); }
};

namespace detail {
inline void put_u64(std::vector<uint8_t> &b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
// bincode of PublicKey: its base64 string
inline void put_key(std::vector<uint8_t> &b, const crypto::PublicKey &pk) {
  const std::string s = pk.encode_base64();
  put_u64(b, s.size());
  b.insert(b.end(), s.begin(), s.end());
}
inline void put_signature(std::vector<uint8_t> &b, const crypto::Signature &s) {
  b.insert(b.end(), s.part1.begin(), s.part1.end());
  b.insert(b.end(), s.part2.begin(), s.part2.end());
}
inline void put_qc(std::vector<uint8_t> &b, const QC &qc) {
  b.insert(b.end(), qc.hash.bytes.begin(), qc.hash.bytes.end());
  put_u64(b, qc.round);
  put_u64(b, qc.votes.size());
  for (const auto &v : qc.votes) {
    put_key(b, v.first);
    put_signature(b, v.second);
  }
}
inline Verdict verdict(int rc, const hsv_proposal_result &where, const char *what) {
  crypto::check_infra(rc, what);
  Verdict v;
  v.result = rc == 1 ? crypto::Result::ok() : crypto::Result::err();
  v.where = where;
  return v;
}
}  // namespace detail

// messages.rs:16-24
struct Block {
  QC qc;
  bool has_tc = false;  // tc: Option<TC>
  TC tc;
  crypto::PublicKey author;
  Round round = 0;
  std::vector<crypto::Digest> payload;
  crypto::Signature signature;

  // Block::verify's signature checks (messages.rs:63-74): fills an
  // hsv_proposal and makes one call.
  Verdict verify_signatures(hsv_committee *committee = nullptr) const {
    std::vector<uint8_t> pay(payload.size() * 32), qv(qc.votes.size() * 96), tv(has_tc ? tc.votes.size() * 104 : 0);
    for (size_t i = 0; i < payload.size(); ++i) std::memcpy(pay.data() + 32 * i, payload[i].bytes.data(), 32);
    for (size_t i = 0; i < qc.votes.size(); ++i) {
      std::memcpy(qv.data() + 96 * i, qc.votes[i].first.bytes.data(), 32);
      std::memcpy(qv.data() + 96 * i + 32, qc.votes[i].second.flatten().data(), 64);
    }
    for (size_t i = 0; i * 104 < tv.size(); ++i) {
      uint8_t *r = tv.data() + 104 * i;
      std::memcpy(r, tc.votes[i].author.bytes.data(), 32);
      std::memcpy(r + 32, tc.votes[i].signature.flatten().data(), 64);
      for (int b = 0; b < 8; ++b) r[96 + b] = (uint8_t)(tc.votes[i].high_qc_round >> (8 * b));
    }
    hsv_proposal p{};
    std::memcpy(p.author, author.bytes.data(), 32);
    std::memcpy(p.signature, signature.flatten().data(), 64);
    p.round = round;
    p.payload = pay.data();
    p.n_payload = payload.size();
    std::memcpy(p.qc_hash, qc.hash.bytes.data(), 32);
    p.qc_round = qc.round;
    p.qc_votes = qv.data();
    p.n_qc = qc.votes.size();
    p.has_tc = has_tc ? 1 : 0;
    p.tc_round = tc.round;
    p.tc_votes = tv.data();
    p.n_tc = has_tc ? tc.votes.size() : 0;
    hsv_proposal_result where{HSV_STAGE_OK, 0};
    return detail::verdict(hsv_proposal_verify(committee, &p, &where, nullptr), where, "hsv_proposal_verify");
  }
};

// messages.rs:112-118
struct Vote {
  crypto::Digest hash;
  Round round = 0;
  crypto::PublicKey author;
  crypto::Signature signature;

  // Vote::verify's signature check (messages.rs:143-145), from the vote's bincode bytes
  crypto::Result verify_signature(hsv_committee *committee = nullptr) const {
    std::vector<uint8_t> b(hash.bytes.begin(), hash.bytes.end());
    detail::put_u64(b, round);
    detail::put_key(b, author);
    detail::put_signature(b, signature);
    const int rc = crypto::check_infra(hsv_vote_verify_bincode(committee, b.data(), b.size()), "hsv_vote_verify_bincode");
    return rc == 1 ? crypto::Result::ok() : crypto::Result::err();
  }
};

// messages.rs:222-228
struct Timeout {
  QC high_qc;
  Round round = 0;
  crypto::PublicKey author;
  crypto::Signature signature;

  // Timeout::verify's signature checks (messages.rs:257-263) in one call,
  // from the timeout's bincode bytes; the TC stage is never reported
  Verdict verify_signatures(hsv_committee *committee = nullptr) const {
    std::vector<uint8_t> b;
    detail::put_qc(b, high_qc);
    detail::put_u64(b, round);
    detail::put_key(b, author);
    detail::put_signature(b, signature);
    hsv_proposal_result where{HSV_STAGE_OK, 0};
    return detail::verdict(hsv_timeout_verify_bincode(committee, b.data(), b.size(), &where, nullptr, nullptr), where,
                           "hsv_timeout_verify_bincode");
  }
};

}  // namespace consensus

// Batch key derivation and signing on the GPU (hsv_signer_*, hsv.h): the form
// of generate_keypair / Signature::new a load generator uses.  Not constant
// time -- never a home for a validator's key.  Owns the signer handle; errors
// throw crypto::InfrastructureError (there is no CPU fallback).
namespace hsv {

class Signer {
 public:
  // seeds: nkeys * 32 bytes
  Signer(const uint8_t *seeds, size_t nkeys) {
    crypto::check_infra(hsv_signer_create(seeds, nkeys, &h_), "hsv_signer_create");
  }
  explicit Signer(const std::vector<std::array<uint8_t, 32>> &seeds)
      : Signer(seeds.empty() ? nullptr : seeds[0].data(), seeds.size()) {}
  ~Signer() { hsv_signer_destroy(h_); }
  Signer(const Signer &) = delete;
  Signer &operator=(const Signer &) = delete;
  Signer(Signer &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Signer &operator=(Signer &&o) noexcept {
    if (this != &o) {
      hsv_signer_destroy(h_);
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }

  size_t size() const { return hsv_signer_size(h_); }
  std::vector<crypto::PublicKey> public_keys() const {
    std::vector<uint8_t> raw(size() * 32);
    crypto::check_infra(hsv_signer_public_keys(h_, raw.data()), "hsv_signer_public_keys");
    std::vector<crypto::PublicKey> out(size());
    for (size_t i = 0; i < out.size(); ++i) std::memcpy(out[i].bytes.data(), raw.data() + 32 * i, 32);
    return out;
  }
  // m messages of msg_len bytes at msg_stride (0: one shared message), key
  // key_idx[i] for item i (nullptr: key i); returns m * 64 bytes, R || s
  std::vector<uint8_t> sign(const uint32_t *key_idx, const uint8_t *msgs, size_t msg_len, size_t msg_stride,
                            size_t m) {
    std::vector<uint8_t> sig(m * 64);
    crypto::check_infra(hsv_signer_sign(h_, key_idx, msgs, msg_len, msg_stride, m, sig.data()), "hsv_signer_sign");
    return sig;
  }
  // every key signs one digest: the votes of a QC
  std::vector<uint8_t> sign_all(const crypto::Digest &digest) {
    return sign(nullptr, digest.bytes.data(), 32, 0, size());
  }
  // device-resident, stream-ordered form (hsv_signer_sign_device)
  void sign_device(const uint32_t *d_key_idx, const uint8_t *d_msg, size_t msg_len, size_t msg_stride, size_t m,
                   uint8_t *d_sig, size_t sig_stride, uint32_t *d_fault = nullptr, void *stream = nullptr) const {
    crypto::check_infra(hsv_signer_sign_device(h_, d_key_idx, d_msg, msg_len, msg_stride, m, d_sig, sig_stride,
                                               d_fault, stream),
                        "hsv_signer_sign_device");
  }
  // Mempool transactions message || pk || R || s, signed in place
  // (hsv_signer_sign_transactions): n transactions at txs[offsets[i] ..
  // offsets[i+1]) (n + 1 offsets), or of tx_size bytes each when offsets is
  // nullptr; key key_idx[i] for item i (nullptr: key i).  The last 96 bytes of
  // each become pk and the signature over SHA-512(message)[..32]; a
  // transaction shorter than 96 bytes throws before anything is written.
  void sign_transactions(const uint32_t *key_idx, uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t n) {
    crypto::check_infra(hsv_signer_sign_transactions(h_, key_idx, txs, offsets, tx_size, n),
                        "hsv_signer_sign_transactions");
  }
  // equal transactions of tx_size bytes, item i with key i
  void sign_transactions(std::vector<uint8_t> &txs, size_t tx_size) {
    sign_transactions(nullptr, txs.data(), nullptr, tx_size, tx_size ? txs.size() / tx_size : 0);
  }
  // device-resident, stream-ordered form (hsv_signer_sign_transactions_device)
  void sign_transactions_device(const uint32_t *d_key_idx, uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size,
                                size_t n, uint32_t *d_fault = nullptr, void *stream = nullptr) const {
    crypto::check_infra(hsv_signer_sign_transactions_device(h_, d_key_idx, d_txs, d_offsets, tx_size, n, d_fault,
                                                            stream),
                        "hsv_signer_sign_transactions_device");
  }
  // Whole messages of differing lengths (hsv_signer_sign_msgs, the signing
  // mirror of hsv_verify_msgs): message i is msgs[offsets[i] .. offsets[i+1])
  // (m + 1 offsets), or msg_len bytes at msgs + i * msg_stride when offsets is
  // nullptr; key key_idx[i] for item i (nullptr: key i).  Returns m * 64
  // bytes, R || s; decreasing offsets throw before anything is signed.
  std::vector<uint8_t> sign_msgs(const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *offsets,
                                 size_t msg_len, size_t msg_stride, size_t m) {
    std::vector<uint8_t> sig(m * 64);
    crypto::check_infra(hsv_signer_sign_msgs(h_, key_idx, msgs, offsets, msg_len, msg_stride, m, sig.data()),
                        "hsv_signer_sign_msgs");
    return sig;
  }
  // one message per item, item i with key i
  std::vector<uint8_t> sign_msgs(const std::vector<std::vector<uint8_t>> &msgs) {
    std::vector<uint64_t> offsets(msgs.size() + 1, 0);
    std::vector<uint8_t> buf;
    for (size_t i = 0; i < msgs.size(); ++i) {
      buf.insert(buf.end(), msgs[i].begin(), msgs[i].end());
      offsets[i + 1] = buf.size();
    }
    return sign_msgs(nullptr, buf.empty() ? nullptr : buf.data(), offsets.data(), 0, 0, msgs.size());
  }
  // device-resident, stream-ordered form (hsv_signer_sign_msgs_device)
  void sign_msgs_device(const uint32_t *d_key_idx, const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len,
                        size_t msg_stride, size_t m, uint8_t *d_sig, size_t sig_stride, uint32_t *d_fault = nullptr,
                        void *stream = nullptr) const {
    crypto::check_infra(hsv_signer_sign_msgs_device(h_, d_key_idx, d_msgs, d_offsets, msg_len, msg_stride, m, d_sig,
                                                    sig_stride, d_fault, stream),
                        "hsv_signer_sign_msgs_device");
  }
  hsv_signer *handle() const { return h_; }

 private:
  hsv_signer *h_ = nullptr;
};

// A committee's keys with their comb tables on the GPU (hsv_committee_*,
// hsv.h), for a QC or TC whose votes sign whole messages: the caller looks each
// vote's author up once (index) and verifies the votes by member index, the
// committee form of crypto::Signature::verify_msgs.  Owns the handle; errors
// throw crypto::InfrastructureError (there is no CPU fallback).
class Committee {
 public:
  explicit Committee(const std::vector<crypto::PublicKey> &keys, bool compact = false) {
    std::vector<uint8_t> raw(keys.size() * 32);
    for (size_t i = 0; i < keys.size(); ++i) std::memcpy(raw.data() + 32 * i, keys[i].bytes.data(), 32);
    crypto::check_infra(hsv_committee_create_ex(raw.data(), keys.size(),
                                                compact ? HSV_COMMITTEE_DIGITS_COMPACT : HSV_COMMITTEE_DIGITS_FULL,
                                                &h_),
                        "hsv_committee_create_ex");
  }
  ~Committee() { hsv_committee_destroy(h_); }
  Committee(const Committee &) = delete;
  Committee &operator=(const Committee &) = delete;

  size_t size() const { return hsv_committee_size(h_); }
  // the member index of pk, or -1 for a stranger
  int64_t index(const crypto::PublicKey &pk) const { return hsv_committee_index(h_, pk.bytes.data()); }
  // Votes over whole messages by member index (hsv_committee_verify_msgs_indexed):
  // item i is sigs[i] over msgs[i] under member key_idx[i].  Returns the
  // per-item HSV_* flag bytes, those of Signature::verify_msgs for the member's
  // key; an index >= size() gives flags 0.
  std::vector<uint8_t> verify_msgs_indexed(const std::vector<uint32_t> &key_idx,
                                           const std::vector<crypto::Signature> &sigs,
                                           const std::vector<std::vector<uint8_t>> &msgs) {
    const size_t m = key_idx.size();
    if (sigs.size() != m || msgs.size() != m)
      throw std::invalid_argument("verify_msgs_indexed: one signature and one message per index");
    std::vector<uint8_t> sig(m * 64), buf, flags(m);
    std::vector<uint64_t> offsets(m + 1, 0);
    for (size_t i = 0; i < m; ++i) {
      std::memcpy(sig.data() + 64 * i, sigs[i].part1.data(), 32);
      std::memcpy(sig.data() + 64 * i + 32, sigs[i].part2.data(), 32);
      buf.insert(buf.end(), msgs[i].begin(), msgs[i].end());
      offsets[i + 1] = buf.size();
    }
    crypto::check_infra(hsv_committee_verify_msgs_indexed(h_, key_idx.data(), sig.data(), buf.data(), offsets.data(), 0,
                                                          0, m, flags.data()),
                        "hsv_committee_verify_msgs_indexed");
    return flags;
  }
  // device-resident, stream-ordered form (hsv_committee_verify_msgs_indexed_device)
  void verify_msgs_indexed_device(const uint32_t *d_key_idx, const uint8_t *d_sig, size_t sig_stride,
                                  const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                                  size_t m, uint8_t *d_flags, uint32_t *d_fault = nullptr,
                                  void *stream = nullptr) const {
    crypto::check_infra(hsv_committee_verify_msgs_indexed_device(h_, d_key_idx, d_sig, sig_stride, d_msgs, d_offsets,
                                                                 msg_len, msg_stride, m, d_flags, d_fault, stream),
                        "hsv_committee_verify_msgs_indexed_device");
  }
  hsv_committee *handle() const { return h_; }

 private:
  hsv_committee *h_ = nullptr;
};

}  // namespace hsv

// Core::make_vote's payload check from the stored bytes
// (consensus/src/core.rs:113-142; hsv_batch*_verify_bincode, hsv.h): the bincode
// of MempoolMessage::Batch(Vec<Vec<u8>>) verified where it lies.
namespace mempool {

// BatchMaker::seal's serialization (mempool/src/batch_maker.rs:127-131)
inline std::vector<uint8_t> encode_batch(const std::vector<std::vector<uint8_t>> &txs) {
  std::vector<uint8_t> out(12, 0);
  auto put_u64 = [&](size_t at, uint64_t v) {
    for (int i = 0; i < 8; ++i) out[at + i] = (uint8_t)(v >> (8 * i));
  };
  put_u64(4, txs.size());
  for (const std::vector<uint8_t> &t : txs) {
    out.resize(out.size() + 8);
    put_u64(out.size() - 8, t.size());
    out.insert(out.end(), t.begin(), t.end());
  }
  return out;
}

// True iff buf is a well-formed Batch whose transactions all verify; false for a
// failing transaction (res, optional, says which) and for malformed bytes or a
// BatchRequest, which make_vote rejects alike (res->status == HSV_BATCH_PARSE).
// Infrastructure errors throw.  committee (optional): the known clients' keys.
inline bool verify_serialized_batch(const uint8_t *buf, size_t len, hsv_committee *committee = nullptr,
                                    hsv_batch_result *res = nullptr) {
  hsv_batch_result r{};
  const int rc = hsv_batch_verify_bincode(committee, buf, len, &r);
  if (rc == HSV_ERR_PARSE) r.status = HSV_BATCH_PARSE;
  else crypto::check_infra(rc, "hsv_batch_verify_bincode");
  if (res) *res = r;
  return rc == 1;
}
inline bool verify_serialized_batch(const std::vector<uint8_t> &buf, hsv_committee *committee = nullptr,
                                    hsv_batch_result *res = nullptr) {
  return verify_serialized_batch(buf.data(), buf.size(), committee, res);
}

// Several stored batches in one call (hsv_batches_verify_bincode): one verdict
// per batch, a malformed one HSV_BATCH_PARSE.
inline std::vector<hsv_batch_result> verify_serialized_batches(const std::vector<std::vector<uint8_t>> &batches,
                                                               hsv_committee *committee = nullptr) {
  std::vector<uint8_t> bufs;
  std::vector<uint64_t> offsets(batches.size() + 1, 0);
  for (size_t i = 0; i < batches.size(); ++i) {
    bufs.insert(bufs.end(), batches[i].begin(), batches[i].end());
    offsets[i + 1] = bufs.size();
  }
  std::vector<hsv_batch_result> res(batches.size());
  crypto::check_infra(hsv_batches_verify_bincode(committee, bufs.data(), offsets.data(), batches.size(), res.data(),
                                                 nullptr, 0),
                      "hsv_batches_verify_bincode");
  return res;
}

// What the `benchmark` block of BatchMaker::seal logs about a batch
// (mempool/src/batch_maker.rs:118-125, 133-153; hsv_batch_samples_bincode, no
// GPU): the ids of its sample transactions in order (ids, optional) and, in the
// result, their number and the batch's size.  A malformed batch has status
// HSV_BATCH_PARSE and no ids.  Infrastructure errors throw.
inline hsv_batch_samples batch_samples(const uint8_t *buf, size_t len, std::vector<uint64_t> *ids = nullptr) {
  hsv_batch_samples r{};
  if (ids) ids->clear();
  int rc = hsv_batch_samples_bincode(buf, len, &r, nullptr, 0);
  if (rc == 1 && ids && r.n_samples) {
    ids->resize((size_t)r.n_samples);
    rc = hsv_batch_samples_bincode(buf, len, &r, ids->data(), ids->size());
  }
  if (rc == HSV_ERR_PARSE) {
    r = hsv_batch_samples{};
    r.status = HSV_BATCH_PARSE;
  } else {
    crypto::check_infra(rc, "hsv_batch_samples_bincode");
  }
  return r;
}
inline hsv_batch_samples batch_samples(const std::vector<uint8_t> &buf, std::vector<uint64_t> *ids = nullptr) {
  return batch_samples(buf.data(), buf.size(), ids);
}

}  // namespace mempool

// The benchmark client's transactions (node/src/client.rs:106-148;
// hsv_client_bursts, no GPU).
namespace client {

// n transactions of tx_size bytes in bursts of `burst`, one sample 00 || BE64(counter)
// per burst among 01 || BE64(r) fillers, zero-padded up to the last `trailer`
// bytes (96: room for hsv::Signer::sign_transactions; 0: the reference's
// unsigned filler), which stay zero here.  r (optional): in, the r before the
// first transaction; out, the r to continue with.
inline std::vector<uint8_t> bursts(size_t n, size_t tx_size, uint64_t burst, uint64_t counter0 = 0,
                                   uint64_t *r = nullptr, size_t trailer = 96) {
  std::vector<uint8_t> txs(n * tx_size, 0);
  uint64_t r_next = 0;
  crypto::check_infra(hsv_client_bursts(txs.data(), tx_size, trailer, counter0, burst, r ? *r : 0, n, &r_next),
                      "hsv_client_bursts");
  if (r) *r = r_next;
  return txs;
}

}  // namespace client

#endif  // HSV_CRYPTO_HPP_
