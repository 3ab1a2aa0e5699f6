// What the signer's launches share (hsv_signer.hip, hsv_msgsign.hip): the
// block size, the lane's view of the launch workspace, the grid of a batch and
// the dispatch over the built group sizes G.  Device translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hsv_sign_core.hpp"

namespace hsv {

constexpr int kSignBlock = 256;

// Slot g, word w of this lane: base[(g * kSignWsWords + w) * 64] -- one word of
// all 64 lanes is one 256-byte line.
struct LaneStore {
  uint32_t *base;
  __device__ __forceinline__ void put(int g, int w, uint32_t v) { base[(uint32_t)(g * kSignWsWords + w) * 64u] = v; }
  __device__ __forceinline__ uint32_t get(int g, int w) const { return base[(uint32_t)(g * kSignWsWords + w) * 64u]; }
};

struct SignGrid {
  uint32_t blocks;
  size_t ws_bytes;
};
inline SignGrid sign_grid_for(uint64_t n, int group) {
  const uint64_t per_block = (uint64_t)kSignBlock * group;
  const uint64_t blocks = (n + per_block - 1) / per_block;
  return {(uint32_t)blocks, (size_t)(blocks * per_block * kSignWsWords * sizeof(uint32_t))};
}

// fn(std::integral_constant<int, G>) for the built G that `group` names
template <class Fn>
void sign_with_group(int group, Fn &&fn) {
  switch (group) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 8: fn(std::integral_constant<int, 8>{}); break;
    default: fn(std::integral_constant<int, 16>{}); break;
  }
}

}  // namespace hsv
