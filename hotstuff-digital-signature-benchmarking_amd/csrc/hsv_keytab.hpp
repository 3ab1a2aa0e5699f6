// Member index by key, on the device: the lookup of the committee
// transaction path (hsv_committee_verify_transactions*, hsv_mempool.hip) and
// of the committee message path (hsv_committee_verify_msgs*,
// hsv_committee_msgs.hip).
//
// A transaction carries its signer's 32 raw key bytes; whether they are a
// committee member's decides which kernels verify it.  The table is the
// device form of KeyIndex (hsv_keyindex.hpp): open addressing in HBM,
// capacity a power of two >= 2 x keys, linear probing, slot = 1 + member
// index, 0 = empty.  A probe compares all 32 bytes against the committee's key
// array (d_pks, 32 bytes per member), so a hit is exact; of a key listed twice
// the first index wins, as KeyIndex::emplace.  The slot hash is KeyHash's keyed
// mix: transaction keys are attacker-chosen bytes, so the per-process seed is
// an argument of the lookup and never a constant of the code.
//
// Host-compilable like hsv_comb.hpp: keytab_build (host only) fills the slots,
// keytab_find is shared by the route kernel and tests/native/keytab_host.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hsv_field.hpp"  // HSV_INL

#include <vector>

namespace hsv {

constexpr uint32_t kKeytabMiss = 0xffffffffu;

// the keyed mix, also KeyHash's (hsv_keyindex.hpp), over the key's eight
// little-endian words
HSV_INL uint64_t keytab_hash(uint64_t seed, const uint32_t pkw[8]) {
  uint64_t h = seed;
  for (int i = 0; i < 4; ++i) {
    const uint64_t w = (uint64_t)pkw[2 * i] | ((uint64_t)pkw[2 * i + 1] << 32);
    h = (h ^ w) * 0xbf58476d1ce4e5b9ull;
    h ^= h >> 31;
  }
  return h;
}

// member `idx`'s 32 bytes in pks against pkw
HSV_INL bool keytab_key_eq(const uint8_t *pks, uint32_t idx, const uint32_t pkw[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 *p = reinterpret_cast<const uint4 *>(pks + (uint64_t)idx * 32);  // d_pks: 32-byte entries of a hipMalloc block
  const uint4 a = p[0], b = p[1];
  return ((a.x ^ pkw[0]) | (a.y ^ pkw[1]) | (a.z ^ pkw[2]) | (a.w ^ pkw[3]) | (b.x ^ pkw[4]) | (b.y ^ pkw[5]) |
          (b.z ^ pkw[6]) | (b.w ^ pkw[7])) == 0u;
#else
  uint32_t w[8];
  memcpy(w, pks + (size_t)idx * 32, 32);
  uint32_t d = 0;
  for (int i = 0; i < 8; ++i) d |= w[i] ^ pkw[i];
  return d == 0u;
#endif
}

// The member index of the key pkw (its 32 bytes as little-endian words), or
// kKeytabMiss.  table: mask + 1 slots.  The walk ends at the first empty slot;
// it is also bounded by the capacity, so a table without one (never built by
// keytab_build) still ends.
HSV_INL uint32_t keytab_find(const uint32_t *table, uint32_t mask, uint64_t seed, const uint8_t *d_pks,
                             const uint32_t pkw[8]) {
  uint32_t h = (uint32_t)keytab_hash(seed, pkw) & mask;
  for (uint32_t probes = 0; probes <= mask; ++probes) {
    const uint32_t e = table[h];
    if (e == 0u) return kKeytabMiss;
    if (keytab_key_eq(d_pks, e - 1u, pkw)) return e - 1u;
    h = (h + 1u) & mask;
  }
  return kKeytabMiss;
}

// ---- host: the builder ----
// slots of a table for n keys: a power of two, at least 2 n (and 2)
inline uint32_t keytab_capacity(size_t n) {
  uint32_t cap = 2;
  while ((size_t)cap < 2 * n) cap <<= 1;
  return cap;
}

// The table of pks[0 .. 32 n) under `seed` (n <= 2^20, hsv_committee_create's
// bound); a key already placed keeps its first index.
inline std::vector<uint32_t> keytab_build(const uint8_t *pks, size_t n, uint64_t seed) {
  const uint32_t cap = keytab_capacity(n), mask = cap - 1u;
  std::vector<uint32_t> slots(cap, 0u);
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8];
    memcpy(w, pks + 32 * i, 32);
    uint32_t h = (uint32_t)keytab_hash(seed, w) & mask;
    bool dup = false;
    while (slots[h] != 0u) {
      if (keytab_key_eq(pks, slots[h] - 1u, w)) {
        dup = true;
        break;
      }
      h = (h + 1u) & mask;
    }
    if (!dup) slots[h] = (uint32_t)i + 1u;
  }
  return slots;
}

}  // namespace hsv
