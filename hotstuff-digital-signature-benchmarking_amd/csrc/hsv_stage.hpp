// Wave-cooperative staging of ragged byte ranges through LDS, shared by the
// kernels that hash caller bytes at arbitrary addresses: the mempool record
// kernels (hsv_mempool.hip) and the any-length message prepass
// (hsv_msgs.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "hsv_field.hpp"

namespace hsv {

constexpr uint64_t kNoChunk = ~0ull;      // lane without a transaction: loads nothing

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// The wave's NQ chunks starting at chunk first(t) (clamped to last(t)) for each
// of its 64 transactions t, staged through LDS with consecutive lanes reading
// consecutive chunks of one transaction (one load instruction covers about
// 64/NQ transactions' runs instead of 64 scattered lines); lane l gets the raw
// words of its own transaction.
template <int NQ>
__device__ __forceinline__ void tx_stage_chunks(const uint4 *__restrict__ q, uint4 *stage, uint32_t lane,
                                                uint64_t first, uint64_t last, uint32_t raw[4 * NQ + 1]) {
  HSV_UNROLL
  for (int it = 0; it < NQ; ++it) {
    const uint32_t e = (uint32_t)it * 64u + lane;  // = t * NQ + c
    const uint32_t t = e / NQ, c = e - t * NQ;
    const uint64_t f = shfl_u64(first, (int)t), l = shfl_u64(last, (int)t);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (l != kNoChunk) {
      const uint64_t k = f + c;
      v = q[k < l ? k : l];
    }
    stage[e] = v;
  }
  __builtin_amdgcn_wave_barrier();
  HSV_UNROLL
  for (int k = 0; k < NQ; ++k) {
    const uint4 v = stage[lane * NQ + k];
    raw[4 * k] = v.x;
    raw[4 * k + 1] = v.y;
    raw[4 * k + 2] = v.z;
    raw[4 * k + 3] = v.w;
  }
  raw[4 * NQ] = 0u;
  __builtin_amdgcn_wave_barrier();  // every lane has read before the next staging round
}

}  // namespace hsv
