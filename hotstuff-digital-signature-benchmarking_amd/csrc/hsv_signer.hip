// gfx950 kernels of the batch signer (hsv_signer_*, include/hsv.h).
//
//  hsv_keygen_kernel  seeds -> 96-byte expanded key records a | prefix | pk
//  hsv_sign_kernel    (key record, message) -> R || s
//  hsv_tx_sign_kernel (key record, digest of a transaction's message) -> pk || R || s
//                     at the end of the transaction, at any byte address
//                     (hsv_txsign.hpp; its digests come from hsv_tx_digest_kernel,
//                     hsv_txsign.hip, the launch before it)
//
// All run csrc/hsv_sign_core.hpp's lane functions on a plain grid: a wave
// takes 64 * G consecutive items, lane l the items base + g * 64 + l (g < G),
// so every load and store of a wave is coalesced.  The state an item keeps
// between the two phases (its point, the prefix product before it, r: 49
// words) sits in a launch workspace from the library pool, word by word across
// the wave's lanes; nothing is handed between waves, so there is no work
// counter and no persistent loop.  [r]B reads the wide comb of B the device
// context already holds (16 reads of 96 bytes per item, MALL-resident).
#include <hip/hip_runtime.h>

#include <atomic>

#include "hsv_internal.h"
#include "hsv_sign_launch.hpp"
#include "hsv_txsign.hpp"

namespace hsv {

template <int G>
__global__ void __launch_bounds__(kSignBlock) hsv_keygen_kernel(KeygenArgs a, uint32_t *__restrict__ ws,
                                                                uint32_t *__restrict__ fault) {
  const uint32_t wave = blockIdx.x * (kSignBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint64_t base = (uint64_t)wave * 64u * G;
  if (base >= a.n) return;  // the whole wave is past the end
  LaneStore st{ws + (uint64_t)wave * G * kSignWsWords * 64u + lane};
  a.inject = kInjectNone;
  if (keygen_lane<16, G>(a, base + lane, 64u, st)) fault[0] = 1u;  // device self-check (hsv_pointpass.hpp report_faults)
}

template <int G, bool FAST>
__global__ void __launch_bounds__(kSignBlock) hsv_sign_kernel(SignArgs a, uint32_t *__restrict__ ws,
                                                              uint32_t *__restrict__ fault) {
  const uint32_t wave = blockIdx.x * (kSignBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint64_t base = (uint64_t)wave * 64u * G;
  if (base >= a.m) return;  // the whole wave is past the end
  LaneStore st{ws + (uint64_t)wave * G * kSignWsWords * 64u + lane};
  a.inject = kInjectNone;
  if (sign_lane<16, G, FAST>(a, base + lane, 64u, st)) fault[0] = 1u;
}

// The one-block fast path over the digests of the launch workspace (a.msg,
// stride 32); status and store through TxSignIo.
template <int G>
__global__ void __launch_bounds__(kSignBlock) hsv_tx_sign_kernel(SignArgs a, TxSignIo io, uint32_t *__restrict__ ws,
                                                                 uint32_t *__restrict__ fault) {
  const uint32_t wave = blockIdx.x * (kSignBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint64_t base = (uint64_t)wave * 64u * G;
  if (base >= a.m) return;  // the whole wave is past the end
  LaneStore st{ws + (uint64_t)wave * G * kSignWsWords * 64u + lane};
  a.inject = kInjectNone;
  if (sign_lane<16, G, true>(a, base + lane, 64u, st, io)) fault[0] = 1u;
}

}  // namespace hsv

namespace {

constexpr int kGroups[] = {1, 2, 4, 8, 16};
std::atomic<int> g_group{hsv::kSignGroup};

}  // namespace

// G of the following launches (measurement hook, csrc/hsv_test_hooks.h):
// 0 restores the product's; returns the previous value, or -1 for a value
// that is not built.
extern "C" int hsvi_signer_group(void) { return g_group.load(); }

extern "C" int hsvi_set_signer_group(int g) {
  if (g == 0) g = hsv::kSignGroup;
  for (int b : kGroups)
    if (b == g) return g_group.exchange(g);
  return -1;
}

extern "C" hipError_t hsv_launch_keygen(const uint8_t *seeds, uint32_t n, uint8_t *keys, const uint32_t *comb16,
                                        uint32_t *fault, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > (1u << 22)) return hipErrorInvalidValue;
  const int group = g_group.load();
  const hsv::SignGrid gr = hsv::sign_grid_for(n, group);
  hsv::Workspace ws(nullptr, 0, gr.ws_bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  const hsv::KeygenArgs a{seeds, n, keys, comb16, hsv::kInjectNone, 0u};
  uint32_t *w = reinterpret_cast<uint32_t *>(ws.get());
  hsv::sign_with_group(group, [&](auto g) {
    hipLaunchKernelGGL((hsv::hsv_keygen_kernel<decltype(g)::value>), dim3(gr.blocks), dim3(hsv::kSignBlock), 0, stream,
                       a, w, fault);
  });
  return ws.done(hipGetLastError());
}

extern "C" hipError_t hsv_launch_sign(const uint8_t *keys, uint32_t nkeys, const uint32_t *key_idx, const uint8_t *msg,
                                      uint64_t msg_len, uint64_t msg_stride, uint32_t m, uint8_t *sig,
                                      uint64_t sig_stride, const uint32_t *comb16, uint32_t *fault,
                                      hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (m > (1u << 22)) return hipErrorInvalidValue;
  const int group = g_group.load();
  const hsv::SignGrid gr = hsv::sign_grid_for(m, group);
  hsv::Workspace ws(nullptr, 0, gr.ws_bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  const hsv::SignArgs a{keys, nkeys, key_idx, msg, msg_len, msg_stride, m, sig, sig_stride, comb16, hsv::kInjectNone, 0u};
  uint32_t *w = reinterpret_cast<uint32_t *>(ws.get());
  hsv::sign_with_group(group, [&](auto g) {
    constexpr int G = decltype(g)::value;
    if (a.msg_len == 32)
      hipLaunchKernelGGL((hsv::hsv_sign_kernel<G, true>), dim3(gr.blocks), dim3(hsv::kSignBlock), 0, stream, a, w, fault);
    else
      hipLaunchKernelGGL((hsv::hsv_sign_kernel<G, false>), dim3(gr.blocks), dim3(hsv::kSignBlock), 0, stream, a, w, fault);
  });
  return ws.done(hipGetLastError());
}

// Two launches on `stream`: the digests and slot statuses of the m transactions
// (hsv_txsign.hip) into the workspace, then the signing launch over them.
extern "C" hipError_t hsv_launch_tx_sign(const uint8_t *keys, uint32_t nkeys, const uint32_t *key_idx, uint8_t *txs,
                                         const uint64_t *offsets, uint64_t tx_size, uint32_t m,
                                         const uint32_t *comb16, uint32_t *fault, hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (m > (1u << 22)) return hipErrorInvalidValue;
  const int group = g_group.load();
  const hsv::SignGrid gr = hsv::sign_grid_for(m, group);
  // the signing workspace | m digests of 32 B | m status words
  const size_t off_dig = gr.ws_bytes, off_status = off_dig + (size_t)m * 32;
  hsv::Workspace ws(nullptr, 0, off_status + (size_t)m * 4, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *d = ws.get();
  uint32_t *status = reinterpret_cast<uint32_t *>(d + off_status);
  hipError_t e = hsv_launch_tx_digest(txs, offsets, tx_size, key_idx, nkeys, m, d + off_dig, status, stream);
  if (e == hipSuccess) {
    const hsv::SignArgs a{keys, nkeys, key_idx, d + off_dig, 32, 32, m, nullptr, 0, comb16, hsv::kInjectNone, 0u};
    const hsv::TxSignIo io{status, txs, offsets, tx_size};
    uint32_t *w = reinterpret_cast<uint32_t *>(d);
    hsv::sign_with_group(group, [&](auto g) {
      hipLaunchKernelGGL((hsv::hsv_tx_sign_kernel<decltype(g)::value>), dim3(gr.blocks), dim3(hsv::kSignBlock), 0,
                         stream, a, io, w, fault);
    });
    e = hipGetLastError();
  }
  return ws.done(e);
}
