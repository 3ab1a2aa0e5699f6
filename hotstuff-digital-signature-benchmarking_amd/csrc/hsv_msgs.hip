// Ed25519 over messages of any length (hsv_verify_msgs*, include/hsv.h):
// the scalar prepass that hashes each whole message.
//
// RFC 8032 5.1.7 PureEdDSA: k = SHA-512(R || A || M) over all of M, then the
// rules of dalek's verify_strict as everywhere else.  The point pass needs
// only k, so the work splits as the two-pass form of hsv_verify_device does:
//   hsv_msg_prep_kernel   one lane per item: SHA-512(R || A || M) block by
//                         block (hsv_msghash.hpp), k mod l, lattice reduction,
//                         recoding; the same kPrepWords SoA record as
//                         hsv_prep_kernel, fallback items appended to fb_list
//                         with k mod l in their b words, the others to their
//                         column class's list (deal_append);
//   hsv_verify_hp_kernel  (hsv_kernels.hip, KREC instantiation) the point
//                         pass; it never reads a message byte.
// Two ordinary launches above 2^13 items and no inter-workgroup waiting: a
// message of many megabytes keeps one wave of the prepass busy and nothing
// polls for it.  At or below 2^13 items the small forms of
// hsv_small.hip run instead, one launch, their prepass wave hashing through
// the same msg_hash_lane.
#include <hip/hip_runtime.h>

#define HSV_SHA_BITOP3 1  // v_bitop3_b32 in the message hash, as hsv_mempool.hip
#include "hsv_internal.h"
#include "hsv_msgwave.hpp"
#include "hsv_pointpass.hpp"
#include "hsv_verify_hc.hpp"

namespace hsv {

// One lane per item i of its wave; the wave's message loads are cooperative
// (tx_stage_chunks, hsv_stage.hpp).  Each lane hashes its own blocks, the wave
// loops over its longest message, so the trip count is wave-uniform.  A lane
// past n redoes item n - 1 and stores nothing; every store sits after the
// loop (no store in a lane-dependent region of it, see tx_record_lane in
// hsv_mempool.hip).
__global__ void __launch_bounds__(kMsgBlock)
hsv_msg_prep_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                    uint64_t sig_stride, const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ offsets,
                    uint64_t msg_len, uint64_t msg_stride, uint32_t n, uint32_t *__restrict__ prep,
                    HcCounters *__restrict__ ctr, uint32_t *__restrict__ fb_list, uint32_t *__restrict__ cls_list,
                    int lat_bits) {
  __shared__ uint4 stage_all[kMsgWaves][64 * kMsgQ];
  __builtin_amdgcn_s_setprio(3);  // as hsv_prep_kernel: ahead of a running point pass
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const bool live = blockIdx.x * kMsgBlock + wv * 64u < n;  // false: the whole wave is past the end
  bool listed = false;
  uint32_t cls = 0, i = 0;
  if (live) {
    uint4 *stage = stage_all[wv];
    const uint32_t i_in = blockIdx.x * kMsgBlock + threadIdx.x;
    i = i_in < n ? i_in : n - 1u;
    uint32_t hw[16], s[8];
    const bool ok =
        msg_hash_lane(pk, pk_stride, sig, sig_stride, msgs, offsets, msg_len, msg_stride, i, lane, stage, hw);
    {
      const uint4 *sigq = reinterpret_cast<const uint4 *>(sig + (uint64_t)i * sig_stride);
      const uint4 s0 = sigq[2], s1 = sigq[3];
      s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w;
      s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w;
    }
    if (i_in < n) {
      const bool fallback =
          prep_from_hash<4, PutPlain, true, pointpass_digit_bits<4>()>(hw, s, prep + i, n, lat_bits, !ok, &cls);
      if (fallback) fb_list[atomicAdd(&ctr->fb_count, 1u)] = i;
      listed = !fallback;
    }
  }
  if (cls_list) deal_append(ctr, cls_list, n, listed, cls, i);  // the whole block: barriers inside
}

}  // namespace hsv

extern "C" hipError_t hsv_launch_msg_prep(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                          uint64_t sig_stride, const uint8_t *msgs, const uint64_t *offsets,
                                          uint64_t msg_len, uint64_t msg_stride, uint32_t n, uint32_t *prep,
                                          void *ctr, uint32_t *fb_list, uint32_t *cls_list, int lat_bits,
                                          hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = (n + hsv::kMsgBlock - 1) / hsv::kMsgBlock;
  hipLaunchKernelGGL(hsv::hsv_msg_prep_kernel, dim3(grid), dim3(hsv::kMsgBlock), 0, stream, pk, pk_stride, sig,
                     sig_stride, msgs, offsets, msg_len, msg_stride, n, prep, static_cast<hsv::HcCounters *>(ctr),
                     fb_list, cls_list, lat_bits);
  return hipGetLastError();
}
