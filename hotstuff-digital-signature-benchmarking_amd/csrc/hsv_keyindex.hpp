// Member index by key, on the host: the lookup of the QC paths (the explicit
// committee, hsv_committee_api.cpp, and the automatic cache,
// hsv_auto_committee.cpp).  Its device form is hsv_keytab.hpp, whose keyed mix
// KeyHash uses.
//
// Pure host code without a HIP include, like hsv_batch.hpp:
// tests/native/keyindex_host.cpp builds it with plain g++.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "hsv_keytab.hpp"

namespace hsvh {

using Key32 = std::array<uint8_t, 32>;

inline Key32 key_of(const uint8_t *p) {
  Key32 k;
  std::memcpy(k.data(), p, 32);
  return k;
}

// Keys are attacker-chosen bytes (they arrive in certificates from the
// network), so the hash is keyed with a per-process random seed.
struct KeyHash {
  static uint64_t seed() {
    static const uint64_t s = [] {
      std::random_device rd;
      return ((uint64_t)rd() << 32) ^ rd() ^ 0x9e3779b97f4a7c15ull;
    }();
    return s;
  }
  // hsv::keytab_hash over the key's eight 32-bit words as they lie in memory:
  // on the little-endian hosts this builds for, the values of the mix over
  // four 8-byte loads that stood here before.
  size_t operator()(const Key32 &k) const {
    uint32_t w[8];
    std::memcpy(w, k.data(), 32);
    return (size_t)hsv::keytab_hash(seed(), w);
  }
};

// Member index by key, on the QC hot path (a C3 QC looks up 667 keys): an
// open-addressing table, load <= 1/2, linear probing, the keys kept
// contiguously.  A probe compares the key's first 8 bytes from the slot's tag
// before the full 32; no node chasing as in std::unordered_map (3.2 us per
// C3 lookup on the GPU box's host with it).  Copyable, so a new cache view
// starts from its base's index.
class KeyIndex {
 public:
  // the member index of pk, or -1
  int64_t find(const uint8_t *pk) const {
    if (count_ == 0) return -1;
    uint64_t w0;
    std::memcpy(&w0, pk, 8);
    for (size_t h = slot_of(pk);; h = (h + 1) & mask_) {
      const uint32_t e = slot_[h];
      if (e == 0) return -1;
      if (tag_[h] == w0 && std::memcmp(keys_.data() + (size_t)(e - 1) * 32, pk, 32) == 0) return val_[e - 1];
    }
  }
  // first insertion of a key wins (as unordered_map::emplace)
  void emplace(const Key32 &k, uint32_t v) {
    if (find(k.data()) >= 0) return;
    if (2 * (count_ + 1) > slot_.size()) grow();
    keys_.insert(keys_.end(), k.begin(), k.end());
    val_.push_back(v);
    ++count_;
    place(count_ - 1);
  }
  size_t size() const { return count_; }

 private:
  size_t slot_of(const uint8_t *pk) const { return KeyHash()(key_of(pk)) & mask_; }
  void place(size_t e) {
    const uint8_t *pk = keys_.data() + e * 32;
    size_t h = slot_of(pk);
    while (slot_[h] != 0) h = (h + 1) & mask_;
    slot_[h] = (uint32_t)e + 1;
    std::memcpy(&tag_[h], pk, 8);
  }
  void grow() {
    const size_t cap = std::max<size_t>(64, slot_.size() * 2);
    slot_.assign(cap, 0u);
    tag_.assign(cap, 0u);
    mask_ = cap - 1;
    for (size_t e = 0; e < count_; ++e) place(e);
  }
  std::vector<uint8_t> keys_;   // count_ * 32, in insertion order
  std::vector<uint32_t> val_;   // member index of each key
  std::vector<uint32_t> slot_;  // 1 + position in keys_, 0 = empty
  std::vector<uint64_t> tag_;   // first 8 bytes of the slot's key
  size_t mask_ = 0, count_ = 0;
};

}  // namespace hsvh
