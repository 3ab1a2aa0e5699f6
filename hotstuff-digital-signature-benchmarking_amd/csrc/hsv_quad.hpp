// The geometry of the committee latency forms, shared by the kernels that run
// it: hsv_comb_verify_quad_fused_kernel and hsv_comb_resident_kernel over
// 32-byte digests (hsv_committee.hip, where the measurements behind these
// values are told) and hsv_cmsg_quad_kernel over whole messages
// (hsv_committee_msgs.hip).  A block takes kFusedVotes votes: wave 0 adds the
// comb entries over kCombLanes lanes per vote, kFusedRWaves waves decompress
// R, the last wave hashes.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "hsv_comb.hpp"
#include "hsv_fe16x16.hpp"

namespace hsv {

// batches up to this many votes take the latency form
constexpr uint32_t kCombQuadMax = 1u << 12;

// lanes per vote of the comb wave: one DPP row
constexpr int kCombLanes = 16;
constexpr int kCombPosPerLane = kCombPos / kCombLanes;

// the swap rounds' partner: lane ^ m of the wave
__device__ __forceinline__ ge_ext ge_swap_xor(const ge_ext &p, int m) {
  ge_ext r;
  HSV_UNROLL
  for (int i = 0; i < kFeLimbs; ++i) {
    r.X.v[i] = (uint32_t)__shfl_xor((int)p.X.v[i], m, 64);
    r.Y.v[i] = (uint32_t)__shfl_xor((int)p.Y.v[i], m, 64);
    r.Z.v[i] = (uint32_t)__shfl_xor((int)p.Z.v[i], m, 64);
    r.T.v[i] = (uint32_t)__shfl_xor((int)p.T.v[i], m, 64);
  }
  return r;
}

// the R waves: one vote per kRRows 16-lane rows (RowLane2, hsv_fe16x16.hpp)
constexpr int kRRows = 2;
using RLane = RowLane2;
constexpr int kRVotesPerWave = 4 / kRRows;
constexpr int kFusedVotes = 64 / kCombLanes;
constexpr int kFusedRWaves = (kFusedVotes + kRVotesPerWave - 1) / kRVotesPerWave;
// the hash wave is the block's last
constexpr uint32_t kHashWaveIdx = 1 + kFusedRWaves;
constexpr int kFusedThreads = 64 * (2 + kFusedRWaves);

// lane g's 8 P digit bits of a recoded scalar, starting at bit 8 g P
__device__ __forceinline__ uint64_t lane_digits(const uint32_t r[9], uint32_t g) {
  constexpr int kBits = 8 * kCombPosPerLane;
  uint64_t d = 0;
  HSV_UNROLL
  for (int q = 0; q < kCombLanes; ++q) {
    const int w = (q * kBits) / 32, sh = (q * kBits) % 32;
    const uint64_t v = ((((uint64_t)r[w + 1] << 32) | r[w]) >> sh) & (kBits == 64 ? ~0ull : ((1ull << kBits) - 1));
    d = g == (uint32_t)q ? v : d;
  }
  return d;
}

}  // namespace hsv
