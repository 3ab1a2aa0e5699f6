// The wave's hash loop over whole messages, shared by the kernels that hash
// R || A || M one lane per item: the any-length message prepass (hsv_msgs.hip)
// and the route kernel of the committee message path
// (hsv_committee_msgs.hip).  Device code only; the block arithmetic is
// hsv_msghash.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include "hsv_stage.hpp"
#include "hsv_msghash.hpp"

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

// hw = SHA-512(R || A || M) of item i (i < n) as 16 little-endian words; R from
// sig + i * sig_stride, A from pk + i * pk_stride (multiples of 16), M =
// msgs[offsets[i], offsets[i+1]) or msg_len bytes at msgs + i * msg_stride.
// Every lane of the wave calls this: the wave's message loads are cooperative
// (tx_stage_chunks, stage: 64 * kMsgQ uint4 of LDS per wave), each lane hashes
// its own blocks and the wave loops over its longest message, so the trip
// count is wave-uniform.  Nothing is stored to global
// memory here: a caller's stores and atomics come after this loop, never in a
// lane-dependent region of it (see tx_record_lane in hsv_mempool.hip).
// Returns false for a decreasing pair of offsets: hashed as an empty message,
// for the caller to mark void.
__device__ __forceinline__ bool msg_hash_lane(const uint8_t *__restrict__ pk, uint64_t pk_stride,
                                              const uint8_t *__restrict__ sig, uint64_t sig_stride,
                                              const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ offsets,
                                              uint64_t msg_len, uint64_t msg_stride, uint32_t i, uint32_t lane,
                                              uint4 *stage, uint32_t hw[16]) {
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
  msg_digest_words(h, hw);
  return ok;
}

// hw = SHA-512(head || M) with the HB / 4 head words from the caller (the
// signer's launches, hsv_msgsign.hip: the prefix, or R || pk gathered through
// key_idx, which a pointer and a stride do not describe); M = mlen bytes at
// msgs + lo.  HB = 32: the window of block 0 is 96 bytes at any offset, 7
// chunks; HB = 64: 64 bytes, 5 chunks; later windows 9, as above.  The
// conventions are msg_hash_lane's: every lane of the wave calls this, the trip
// count is the wave's longest message, nothing is stored to global memory, a
// window without a message byte and an empty message load nothing.
template <int HB>
__device__ __forceinline__ void msg_hash_wave(const uint32_t head[HB / 4], const uint8_t *__restrict__ msgs,
                                              uint64_t lo, uint64_t mlen, uint32_t lane, uint4 *stage,
                                              uint32_t hw[16]) {
  constexpr int NW0 = (128 - HB) / 4;  // message words of block 0
  constexpr int Q0 = NW0 / 4 + 1;
  static_assert(Q0 <= kMsgQ, "block 0 stages through the same LDS");
  const uintptr_t base = reinterpret_cast<uintptr_t>(msgs);
  const uint4 *q = reinterpret_cast<const uint4 *>(base & ~uintptr_t(15));
  const uint64_t start = (uint64_t)(base & 15u) + lo;
  const uint64_t q_last = mlen ? (start + mlen - 1) >> 4 : kNoChunk;  // an empty message loads nothing

  uint64_t h[8];
  sha512_init(h);
  const uint64_t nblocks = head_num_blocks<HB>(mlen);
  uint32_t wave_blocks = (uint32_t)nblocks;
  HSV_UNROLL
  for (int m = 1; m < 64; m <<= 1) wave_blocks = max(wave_blocks, (uint32_t)__shfl_xor((int)wave_blocks, m, 64));
  const uint32_t sh16 = (uint32_t)(start & 15u);
  const bool wave_aligned = __all(sh16 == 0u || mlen == 0);
  HSV_NOUNROLL
  for (uint32_t b = 0; b < wave_blocks; ++b) {
    uint64_t w[16];
    const uint64_t off = head_block_offset<HB>(b);
    const uint64_t last = off < mlen ? q_last : kNoChunk;  // a window without a message byte is not loaded
    if (b == 0) {
      uint32_t raw[4 * Q0 + 1], words[NW0];
      tx_stage_chunks<Q0>(q, stage, lane, start >> 4, last, raw);
      msg_words<NW0>(raw, wave_aligned, sh16, words);
      head_block0_words<HB>(head, words, mlen, w);
    } else {
      uint32_t raw[4 * kMsgQ + 1], words[32];
      tx_stage_chunks<kMsgQ>(q, stage, lane, (start + off) >> 4, last, raw);
      msg_words<32>(raw, wave_aligned, sh16, words);
      const bool wave_full = __all(off + 128u <= mlen);
      if (wave_full) msg_block_words_full(words, w);
      else head_block_words<HB>(words, mlen, b, w);
    }
    if (b < nblocks) {
      if (b + 1 == nblocks) head_length_field<HB>(w, mlen);
      sha512_compress(h, w);
    }
  }
  msg_digest_words(h, hw);
}

}  // namespace hsv
