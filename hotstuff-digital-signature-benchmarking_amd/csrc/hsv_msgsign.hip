// The three launches of a round of hsv_signer_sign_msgs* (include/hsv.h; the
// lane code and the layout are csrc/hsv_msgsign.hpp's):
//
//  hsv_msg_nonce_kernel     status, r = SHA-512(prefix || M) mod l  -> workspace
//  hsv_msg_point_kernel     R = [r]B, enc(R) -> sig slot bytes 0..32 (sign_lane
//                           with MsgSignIo: G items per lane, one fe_invert)
//  hsv_msg_response_kernel  k = SHA-512(R || pk || M) mod l, s = r + k a
//                           -> sig slot bytes 32..64; zeros for a dead item
//
// The two hashing kernels run one lane per item as hsv_msg_prep_kernel
// (hsv_msgs.hip): the wave's message loads are staged through LDS
// (msg_hash_wave, hsv_msgwave.hpp), the trip count is the wave's longest
// message, a lane past m redoes item m - 1 and stores nothing, and every
// global store comes after the hash loop.  They are ordinary launches, one
// after the other on the caller's stream: nothing waits between workgroups.
#include <hip/hip_runtime.h>

#define HSV_SHA_BITOP3 1  // v_bitop3_b32 in the message hash, as hsv_msgs.hip
#include "hsv_internal.h"
#include "hsv_msgwave.hpp"
#include "hsv_msgsign.hpp"
#include "hsv_sign_launch.hpp"

namespace hsv {

struct MsgSignArgs {
  const uint8_t *keys;      // nkeys expanded records of 96 B
  uint32_t nkeys;
  const uint32_t *key_idx;  // m indices, or NULL: item i uses key i
  const uint8_t *msgs;      // any alignment
  const uint64_t *offsets;  // m + 1, or NULL: msg_len bytes at msgs + i * msg_stride
  uint64_t msg_len, msg_stride;
  uint32_t m;
  uint8_t *sig;             // item i's R || s at sig + i * sig_stride, multiples of 16
  uint64_t sig_stride;
  uint8_t *nonce;           // workspace: m * 32 B, 16-byte aligned
  uint32_t *status;         // workspace: m words
};

__global__ void __launch_bounds__(kMsgBlock) hsv_msg_nonce_kernel(MsgSignArgs a) {
  __shared__ uint4 stage_all[kMsgWaves][64 * kMsgQ];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kMsgBlock + wv * 64u >= a.m) return;  // whole wave past the end
  const uint32_t i_in = blockIdx.x * kMsgBlock + threadIdx.x;
  const uint32_t i = i_in < a.m ? i_in : a.m - 1u;
  uint64_t lo, mlen;
  const bool span_ok = msg_sign_span(a.offsets, a.msg_len, a.msg_stride, i, lo, mlen);
  const uint32_t ki = a.key_idx ? a.key_idx[i] : i;
  const uint32_t st = msg_sign_status(span_ok, ki, a.nkeys);
  if (st != kSlotOk) mlen = 0;  // nothing of a dead item is read
  uint32_t head[8], hw[16], r[8];
  msg_nonce_head(a.keys, ki, st, head);
  msg_hash_wave<32>(head, a.msgs, lo, mlen, lane, stage_all[wv], hw);
  msg_nonce_finish(hw, st, r);
  if (i_in < a.m) {
    sign_store16<8>(a.nonce + (uint64_t)i * 32u, r);
    a.status[i] = st;
  }
}

template <int G>
__global__ void __launch_bounds__(kSignBlock) hsv_msg_point_kernel(SignArgs a, MsgSignIo io, uint32_t *__restrict__ ws,
                                                                   uint32_t *__restrict__ fault) {
  const uint32_t wave = blockIdx.x * (kSignBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint64_t base = (uint64_t)wave * 64u * G;
  if (base >= a.m) return;  // the whole wave is past the end
  LaneStore st{ws + (uint64_t)wave * G * kSignWsWords * 64u + lane};
  a.inject = kInjectNone;
  if (sign_lane<16, G, false>(a, base + lane, 64u, st, io)) fault[0] = 1u;
}

__global__ void __launch_bounds__(kMsgBlock) hsv_msg_response_kernel(MsgSignArgs a) {
  __shared__ uint4 stage_all[kMsgWaves][64 * kMsgQ];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kMsgBlock + wv * 64u >= a.m) return;  // whole wave past the end
  const uint32_t i_in = blockIdx.x * kMsgBlock + threadIdx.x;
  const uint32_t i = i_in < a.m ? i_in : a.m - 1u;
  const uint32_t st = a.status[i];
  uint64_t lo, mlen;
  msg_sign_span(a.offsets, a.msg_len, a.msg_stride, i, lo, mlen);
  if (st != kSlotOk) mlen = 0;
  const uint32_t ki = a.key_idx ? a.key_idx[i] : i;
  uint8_t *slot = a.sig + (uint64_t)i * a.sig_stride;
  uint32_t head[16], hw[16], sigw[16];
  msg_response_head(a.keys, ki, st, slot, head);
  msg_hash_wave<64>(head, a.msgs, lo, mlen, lane, stage_all[wv], hw);
  msg_response_finish(hw, head, a.keys, ki, st, a.nonce + (uint64_t)i * 32u, sigw);
  if (i_in < a.m) sign_store16<16>(slot, sigw);
}

}  // namespace hsv

extern "C" hipError_t hsv_launch_msg_sign(const uint8_t *keys, uint32_t nkeys, const uint32_t *key_idx,
                                          const uint8_t *msgs, const uint64_t *offsets, uint64_t msg_len,
                                          uint64_t msg_stride, uint32_t m, uint8_t *sig, uint64_t sig_stride,
                                          const uint32_t *comb16, uint32_t *fault, hipStream_t stream) {
  if (m == 0) return hipSuccess;
  if (m > (1u << 22)) return hipErrorInvalidValue;
  const int group = hsvi_signer_group();
  const hsv::SignGrid gr = hsv::sign_grid_for(m, group);
  // the point launch's workspace | m nonces of 32 B | m status words
  const size_t off_nonce = gr.ws_bytes, off_status = off_nonce + (size_t)m * 32;
  hsv::Workspace ws(nullptr, 0, off_status + (size_t)m * 4, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *d = ws.get();
  uint32_t *status = reinterpret_cast<uint32_t *>(d + off_status);
  const hsv::MsgSignArgs ma{keys, nkeys, key_idx, msgs, offsets, msg_len, msg_stride, m,
                            sig,  sig_stride, d + off_nonce, status};
  const uint32_t grid = (m + hsv::kMsgBlock - 1) / hsv::kMsgBlock;
  hipLaunchKernelGGL(hsv::hsv_msg_nonce_kernel, dim3(grid), dim3(hsv::kMsgBlock), 0, stream, ma);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    const hsv::SignArgs a{keys, nkeys, key_idx, nullptr, 0, 0, m, sig, sig_stride, comb16, hsv::kInjectNone, 0u};
    const hsv::MsgSignIo io{status, d + off_nonce};
    uint32_t *w = reinterpret_cast<uint32_t *>(d);
    hsv::sign_with_group(group, [&](auto g) {
      hipLaunchKernelGGL((hsv::hsv_msg_point_kernel<decltype(g)::value>), dim3(gr.blocks), dim3(hsv::kSignBlock), 0,
                         stream, a, io, w, fault);
    });
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hsv::hsv_msg_response_kernel, dim3(grid), dim3(hsv::kMsgBlock), 0, stream, ma);
    e = hipGetLastError();
  }
  return ws.done(e);
}
