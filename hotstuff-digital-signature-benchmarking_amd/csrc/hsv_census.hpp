// The signer census (hsv_census_keys*, hsv_census_transactions*): the insert
// step of its table, shared by hsv_census_count_kernel (hsv_census.hip) and
// tests/native/census_host.cpp.
//
// The table is open addressing with linear probing over `slots` (a power of
// two) 32-bit words, 0 = empty.  An occupied slot holds 1 + the index of the
// item that claimed it, and a probe compares the probing key against the
// claimer's 32 key bytes where they lie in the call's INPUT, as hsv_keytab.hpp
// compares against d_pks: the input was written before the launch and nothing
// writes it during the call, so no key bytes pass from one workgroup to
// another inside the kernel.  A parallel array holds the slot's count.
//
// What other workgroups do see of each other are the slot words and the
// counts, and both are touched by agent-scope atomics only (relaxed: nothing
// is ordered against them).
//   * A slot goes from 0 to nonzero once, by a compare-and-swap against 0, and
//     never changes again.  The load that precedes the swap may therefore be
//     stale in one way only: it shows 0 where a claim has landed.  Then the
//     swap fails and returns the claimer, the truth.  A nonzero value, from
//     the load or from the swap, is final, whichever cache served it.
//   * Counts only grow by atomic adds, performed where the atomics of every
//     workgroup meet; nobody reads them before the launch has ended.
// The gather kernel and the summary read slots, counts and totals after that
// launch: a kernel boundary, no ready word, no polling.
//
// A walk is bounded by min(slots, kCensusProbeBound) slots.  A key that finds
// neither itself nor an empty slot in that many is not recorded (the caller
// adds its items to `overflow`); slots never empty, so a key is either
// recorded with its exact count or not recorded at all.  The slot hash is
// keytab_hash under a seed the caller passes: keys are attacker-chosen bytes.
//
// On the device the lanes of a wave insert side by side, each the one key it
// leads (the wave has already folded equal keys into one lane and a count,
// hsv_census.hip): every lane calls census_insert, `active` says whether it has
// a key to insert, and the walk goes on while ANY lane of the wave is still
// open, so the loop's back edge is wave-uniform (a scalar branch on a ballot)
// and only its body is masked.  Lanes of one wave that meet in a slot are
// serialised by the atomics like lanes of different waves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hsv_keytab.hpp"  // keytab_hash, HSV_INL

namespace hsv {

constexpr uint32_t kCensusMinSlots = 16u, kCensusMaxSlots = 1u << 22;
constexpr uint32_t kCensusProbeBound = 256u;

// the outcome of an insert (kCensusIdle: the caller had nothing to insert)
constexpr uint32_t kCensusOverflow = 0u, kCensusMatched = 1u, kCensusClaimed = 2u, kCensusIdle = 3u;

// The three memory operations and the wave vote.  Host builds
// (tests/native/census_host.cpp, threads in the place of lanes) use the
// __atomic builtins, as hsv_comb.hpp and hsv_keytab.hpp keep one text for both.
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(1))) uint32_t census_gu32;
#define HSV_CENSUS_LOAD(p) __hip_atomic_load((hsv::census_gu32 *)(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define HSV_CENSUS_ADD(p, v) \
  (void)__hip_atomic_fetch_add((hsv::census_gu32 *)(p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define HSV_CENSUS_ANY(x) (__ballot(x) != 0ull)
// 0 -> want; returns what the slot held before
HSV_INL uint32_t census_claim(uint32_t *p, uint32_t want) {
  uint32_t seen = 0u;
  (void)__hip_atomic_compare_exchange_strong((census_gu32 *)p, &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
  return seen;
}
#else
#define HSV_CENSUS_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define HSV_CENSUS_ADD(p, v) (void)__atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define HSV_CENSUS_ANY(x) (x)
HSV_INL uint32_t census_claim(uint32_t *p, uint32_t want) {
  uint32_t seen = 0u;
  (void)__atomic_compare_exchange_n(p, &seen, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  return seen;
}
#endif

// slots of a census table: a power of two in [kCensusMinSlots, kCensusMaxSlots]
HSV_INL bool census_slots_ok(uint64_t slots) {
  return slots >= kCensusMinSlots && slots <= kCensusMaxSlots && (slots & (slots - 1u)) == 0u;
}

HSV_INL bool census_key_eq(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
  for (int i = 0; i < 8; ++i) d |= a[i] ^ b[i];
  return d == 0u;
}

// Adds `count` occurrences of the key pkw, one of which is item `item` of the
// input: hash, bounded walk, claim an empty slot or match the claimer's key,
// add.  tab, counts: mask + 1 words each.  keys.load(j, w) fills w with the
// key words of input item j (a claimer: well-formed).  active: this caller has
// a key to insert (a lane without one still runs the loop with its wave and
// touches nothing).  Returns kCensusClaimed (a slot newly taken),
// kCensusMatched, kCensusOverflow (nothing recorded) or kCensusIdle (!active).
template <class Keys>
HSV_INL uint32_t census_insert(uint32_t *tab, uint32_t *counts, uint32_t mask, uint64_t seed, const Keys &keys,
                               uint32_t item, const uint32_t pkw[8], uint32_t count, bool active) {
  const uint32_t bound = mask + 1u < kCensusProbeBound ? mask + 1u : kCensusProbeBound;
  uint32_t h = (uint32_t)keytab_hash(seed, pkw) & mask;
  uint32_t r = active ? kCensusOverflow : kCensusIdle;
  bool open = active;
  for (uint32_t probes = 0; probes < bound && HSV_CENSUS_ANY(open); ++probes) {
    if (open) {
      uint32_t e = HSV_CENSUS_LOAD(tab + h);
      bool mine = false;
      if (e == 0u) {
        e = census_claim(tab + h, item + 1u);
        mine = e == 0u;
      }
      bool same = mine;
      if (!mine) {
        uint32_t cw[8];
        keys.load(e - 1u, cw);
        same = census_key_eq(cw, pkw);
      }
      if (same) {
        HSV_CENSUS_ADD(counts + h, count);
        r = mine ? kCensusClaimed : kCensusMatched;
        open = false;
      } else {
        h = (h + 1u) & mask;
      }
    }
  }
  return r;
}

}  // namespace hsv
