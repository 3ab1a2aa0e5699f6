// What the two routed rounds share: hsv_committee_verify_transactions*
// (hsv_mempool.hip) and hsv_committee_verify_msgs* (hsv_committee_msgs.hip).
// In both a route kernel deals the items of a batch to a hit list (signers
// that are committee members), a miss list and a fallback list; a persistent
// comb pass takes the hit list, a persistent generic pass the fallback list and
// then the miss list.  Here: the counters, the small device helpers and the
// host side of a round.
//
// The pass bodies and the route kernels' list compaction stay in the two
// files: as one function template each they compiled to other code (DESIGN.md
// 4j).  The rules those bodies keep, said here once:
//   * a route kernel compacts its lists per wave: one ballot, one atomic add
//     by one lane per list (lane 0 the hits, lane 1 the misses), a prefix rank
//     -- entries keep their order inside a wave, a list costs one atomic per
//     wave;
//   * a work loop's exit is wave-uniform (the batch base comes from lane 0's
//     atomic through readfirstlane) and no store inside it sits in a region
//     that depends on the lane's place in a list: nested lane-dependent stores
//     made hipcc compile a divergent back edge, the round-1 hang
//     (tests/test_kernel_isa.py);
//   * so a lane past a list's end redoes the batch's first entry: in a comb
//     pass it stores the same byte and bit again, in a generic pass `valid`
//     keeps it from storing;
//   * an item that the prepass sent to the fallback list is on the miss list
//     too: `own` keeps the miss-list lane from storing it a second time;
//   * a route kernel's list stores sit in lane-dependent regions, so no loop
//     may surround them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

#include "hsv_internal.h"
#include "hsv_verify_hc.hpp"
#include "hsv_pointpass.hpp"

namespace hsv {

struct RoutedCounters {  // zeroed before the route launch (32 bytes)
  uint32_t hits, misses, fb_count;  // list lengths, written by the route kernel
  uint32_t hit_next, gen_next;      // work counters of the comb and the generic pass
  uint32_t pad[3];
};

// this lane's place among the set bits of a wave mask
__device__ __forceinline__ uint32_t mask_rank(uint64_t mask, uint32_t lane) {
  return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// (load_words8 and store_verdict, which the pass bodies use, are in hsv_pointpass.hpp)

// ---- the host side of a round ----------------------------------------------------
// (internal linkage: each of the two files caches the occupancy of its own
// three kernels)
namespace {

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// blocks per CU of the persistent passes and the device's CUs, cached per device
struct RoutedGrids {
  int comb_bpc, comb4_bpc, generic_bpc, cus;  // (the compact comb pass from its own occupancy query)
};
hipError_t routed_grids(int dev, const void *comb, const void *comb4, const void *generic, RoutedGrids *out) {
  static std::mutex mu;
  static std::unordered_map<int, RoutedGrids> per_dev;
  std::lock_guard<std::mutex> lk(mu);
  auto it = per_dev.find(dev);
  if (it == per_dev.end()) {
    int bc = 0, bc4 = 0, bg = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&bc, comb, 256, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&bc4, comb4, 256, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&bg, generic, kBlock, 0);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    it = per_dev.emplace(dev, RoutedGrids{std::max(1, bc), std::max(1, bc4), std::max(1, bg), std::max(1, cus)}).first;
  }
  *out = it->second;
  return hipSuccess;
}

// One round of n <= 2^22 items on the current device, no synchronisation.
// Both persistent grids fit the device at once (occupancy x CUs, one CU left
// free once the resident service has run, as launch_hp) and are capped by
// ceil(n / 256): the host knows n, not the split.  The workspace starts
// per-lane tables | counters | canaries; what follows is the launcher's.
struct RoutedRound {
  bool compact;  // the committee's table width decides the comb pass, nothing else
  uint32_t blocks_needed, grid_c, grid_g;
  size_t vt_bytes, canary_bytes;

  hipError_t size(uint32_t n, int digit_bits, const void *comb, const void *comb4, const void *generic) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    RoutedGrids g;
    e = routed_grids(dev, comb, comb4, generic, &g);
    if (e != hipSuccess) return e;
    compact = digit_bits == 4;
    const int cus = hsvi_resident_started() && g.cus > 1 ? g.cus - 1 : g.cus;
    blocks_needed = (n + kBlock - 1) / kBlock;
    grid_c = std::min<uint32_t>(blocks_needed, (uint32_t)((compact ? g.comb4_bpc : g.comb_bpc) * cus));
    grid_g = std::min<uint32_t>(blocks_needed, (uint32_t)(g.generic_bpc * cus));
    vt_bytes = (size_t)grid_g * kBlock * vt_lane_uint4<4>() * sizeof(uint4);
    canary_bytes = up256((size_t)grid_g * kBlock * sizeof(uint32_t));
    return hipSuccess;
  }
  // a round without a generic pass (items addressed by member index have no
  // miss side): no per-lane tables and no canaries, the workspace starts at the
  // counters
  void comb_only() {
    grid_g = 0;
    vt_bytes = canary_bytes = 0;
  }
  size_t head_bytes() const { return vt_bytes + 256 + canary_bytes; }
  // the counters and the strict words zeroed on the stream, before the route launch
  static hipError_t zero(RoutedCounters *ctr, uint32_t *strict_bits, uint32_t n, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(ctr, 0, sizeof(RoutedCounters), stream);
    if (e == hipSuccess && strict_bits) e = hipMemsetAsync(strict_bits, 0, (size_t)((n + 31u) / 32u) * 4u, stream);
    return e;
  }
  // the comb pass's kernel, or its table of B, by the table width
  template <class T>
  T pick(T full, T compact_form) const { return compact ? compact_form : full; }
};

}  // namespace
}  // namespace hsv
