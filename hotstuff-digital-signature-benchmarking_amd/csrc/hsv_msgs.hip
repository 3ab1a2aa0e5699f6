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
//                         with k mod l in their b words;
//   hsv_verify_hp_kernel  (hsv_kernels.hip, KREC instantiation) the point
//                         pass; it never reads a message byte.
// Two ordinary launches at every n and no inter-workgroup waiting: a message of
// many megabytes keeps one wave of the prepass busy and nothing polls for it
// (DESIGN.md 4e).
#include <hip/hip_runtime.h>

#define HSV_SHA_BITOP3 1  // v_bitop3_b32 in the message hash, as hsv_mempool.hip
#include "hsv_internal.h"
#include "hsv_stage.hpp"
#include "hsv_msghash.hpp"
#include "hsv_verify_hc.hpp"

namespace hsv {

constexpr int kMsgBlock = 256;
constexpr int kMsgWaves = kMsgBlock / 64;
constexpr int kMsgQ0 = 5;  // 16-B chunks under the 64-B window of block 0 at any offset
constexpr int kMsgQ = 9;   // ... under a 128-B window

template <int NW>
__device__ __forceinline__ void msg_words(const uint32_t *raw, bool wave_aligned, uint32_t sh16, uint32_t words[NW]) {
  if (wave_aligned) {
    HSV_UNROLL
    for (int j = 0; j < NW; ++j) words[j] = raw[j];
  } else {
    tx_realign<NW>(raw, sh16, words);
  }
}

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
                    uint32_t *__restrict__ fb_count, uint32_t *__restrict__ fb_list, int lat_bits) {
  __shared__ uint4 stage_all[kMsgWaves][64 * kMsgQ];
  __builtin_amdgcn_s_setprio(3);  // as hsv_prep_kernel: ahead of a running point pass
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kMsgBlock + wv * 64u >= n) return;  // whole wave past the end
  uint4 *stage = stage_all[wv];
  const uint32_t i_in = blockIdx.x * kMsgBlock + threadIdx.x;
  const uint32_t i = i_in < n ? i_in : n - 1u;
  uint64_t lo, hi;
  if (offsets) {
    lo = offsets[i];
    hi = offsets[i + 1];
  } else {
    lo = (uint64_t)i * msg_stride;
    hi = lo + msg_len;
  }
  const bool ok = hi >= lo;  // a decreasing pair: hashed as an empty message, marked void
  const uint64_t mlen = ok ? hi - lo : 0;
  const uintptr_t base = reinterpret_cast<uintptr_t>(msgs);
  const uint4 *q = reinterpret_cast<const uint4 *>(base & ~uintptr_t(15));
  const uint64_t start = (uint64_t)(base & 15u) + lo;
  const uint64_t q_last = mlen ? (start + mlen - 1) >> 4 : kNoChunk;  // an empty message loads nothing
  const uint4 *pkq = reinterpret_cast<const uint4 *>(pk + (uint64_t)i * pk_stride);
  const uint4 *sigq = reinterpret_cast<const uint4 *>(sig + (uint64_t)i * sig_stride);

  uint64_t h[8];
  sha512_init(h);
  const uint64_t nblocks = msg_num_blocks(mlen);
  uint32_t wave_blocks = (uint32_t)nblocks;
  HSV_UNROLL
  for (int m = 1; m < 64; m <<= 1) wave_blocks = max(wave_blocks, (uint32_t)__shfl_xor((int)wave_blocks, m, 64));
  const uint32_t sh16 = (uint32_t)(start & 15u);
  // wave-uniform fast paths: every message of the wave starts on a 16-byte
  // boundary (no realignment), and block b lies wholly inside every message
  // (no padding selects)
  const bool wave_aligned = __all(sh16 == 0u || mlen == 0);
  HSV_NOUNROLL
  for (uint32_t b = 0; b < wave_blocks; ++b) {
    uint64_t w[16];
    const uint64_t off = msg_block_offset(b);
    const uint64_t last = off < mlen ? q_last : kNoChunk;  // a window without a message byte is not loaded
    if (b == 0) {
      uint32_t raw[4 * kMsgQ0 + 1], words[16], head[16];
      tx_stage_chunks<kMsgQ0>(q, stage, lane, start >> 4, last, raw);
      msg_words<16>(raw, wave_aligned, sh16, words);
      {  // R || A
        const uint4 r0 = sigq[0], r1 = sigq[1], a0 = pkq[0], a1 = pkq[1];
        head[0] = r0.x; head[1] = r0.y; head[2] = r0.z; head[3] = r0.w;
        head[4] = r1.x; head[5] = r1.y; head[6] = r1.z; head[7] = r1.w;
        head[8] = a0.x; head[9] = a0.y; head[10] = a0.z; head[11] = a0.w;
        head[12] = a1.x; head[13] = a1.y; head[14] = a1.z; head[15] = a1.w;
      }
      msg_block0_words(head, words, mlen, w);
    } else {
      uint32_t raw[4 * kMsgQ + 1], words[32];
      tx_stage_chunks<kMsgQ>(q, stage, lane, (start + off) >> 4, last, raw);
      msg_words<32>(raw, wave_aligned, sh16, words);
      const bool wave_full = __all(off + 128u <= mlen);
      if (wave_full) msg_block_words_full(words, w);
      else msg_block_words(words, mlen, b, w);
    }
    if (b < nblocks) {
      if (b + 1 == nblocks) msg_length_field(w, mlen);
      sha512_compress(h, w);
    }
  }
  uint32_t hw[16], s[8];
  msg_digest_words(h, hw);
  {
    const uint4 s0 = sigq[2], s1 = sigq[3];
    s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w;
    s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w;
  }
  if (i_in < n) {
    const bool fallback = prep_from_hash<4, PutPlain, true>(hw, s, prep + i, n, lat_bits, !ok);
    if (fallback) fb_list[atomicAdd(fb_count, 1u)] = i;
  }
}

}  // namespace hsv

extern "C" hipError_t hsv_launch_msg_prep(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                          uint64_t sig_stride, const uint8_t *msgs, const uint64_t *offsets,
                                          uint64_t msg_len, uint64_t msg_stride, uint32_t n, uint32_t *prep,
                                          uint32_t *fb_count, uint32_t *fb_list, int lat_bits, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = (n + hsv::kMsgBlock - 1) / hsv::kMsgBlock;
  hipLaunchKernelGGL(hsv::hsv_msg_prep_kernel, dim3(grid), dim3(hsv::kMsgBlock), 0, stream, pk, pk_stride, sig,
                     sig_stride, msgs, offsets, msg_len, msg_stride, n, prep, fb_count, fb_list, lat_bits);
  return hipGetLastError();
}
