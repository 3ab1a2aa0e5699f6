// Ed25519 challenge hash over a message of any length (RFC 8032 5.1.7):
//     h = SHA-512(R || A || M),  M = mlen bytes at an arbitrary byte address.
//
// The hashed stream is the 64-byte head R || A followed by the message, so
//     block 0      = the 16 head words, then message bytes [0, 64)
//     block b >= 1 = message bytes [128 b - 64, 128 b + 64)
//     nblocks      = (64 + mlen + 17 + 127) >> 7,  length field (64 + mlen) * 8.
// One lane hashes one message.  As in hsv_txhash.hpp the lane reads the
// 16-byte-aligned chunks that contain its bytes and realigns them in registers
// (tx_load_words / tx_realign), and bytes past the end are replaced by the
// SHA-512 padding with selects (tx_pad_word).  Every load is clamped to the
// chunk holding the message's last byte, a window that holds no message byte
// is not loaded, and an empty message issues no load at all: its pointer may
// be one past an allocation.
//
// The routines take a chunk loader `ld(q, out[4])` so that the same code runs
// in the gfx950 kernel (hsv_msgs.hip, which stages the chunks through LDS) and
// in the host test build (tests/native/msg_host.cpp).
#pragma once
#include "hsv_txhash.hpp"

namespace hsv {

constexpr uint64_t kMsgHeadBytes = 64;  // R || A

HSV_INL uint64_t msg_num_blocks(uint64_t mlen) { return (kMsgHeadBytes + mlen + 1 + 16 + 127) >> 7; }

// message offset of the first byte block b hashes (block 0: after the head)
HSV_INL uint64_t msg_block_offset(uint64_t b) { return b ? 128u * b - kMsgHeadBytes : 0u; }

// Block 0: head = R || A as 16 little-endian words, words = message bytes
// [0, 64) as 16 little-endian words (anything past mlen is ignored).
HSV_INL void msg_block0_words(const uint32_t head[16], const uint32_t words[16], uint64_t mlen, uint64_t w[16]) {
  HSV_UNROLL
  for (int j = 0; j < 8; ++j) w[j] = be64_from_le32(head[2 * j], head[2 * j + 1]);
  HSV_UNROLL
  for (int j = 0; j < 8; ++j)
    w[8 + j] = tx_pad_word(be64_from_le32(words[2 * j], words[2 * j + 1]), (int64_t)mlen - (int64_t)(8 * j));
}

// Block b >= 1: words = message bytes [128 b - 64, 128 b + 64).
HSV_INL void msg_block_words(const uint32_t words[32], uint64_t mlen, uint64_t b, uint64_t w[16]) {
  HSV_UNROLL
  for (int j = 0; j < 16; ++j) {
    const int64_t rem = (int64_t)mlen - (int64_t)(msg_block_offset(b) + 8 * (uint64_t)j);
    w[j] = tx_pad_word(be64_from_le32(words[2 * j], words[2 * j + 1]), rem);
  }
}

// The same for a block wholly inside the message (128 b + 64 <= mlen): no
// padding selects.  The kernel takes it when every lane of the wave is there.
HSV_INL void msg_block_words_full(const uint32_t words[32], uint64_t w[16]) {
  HSV_UNROLL
  for (int j = 0; j < 16; ++j) w[j] = be64_from_le32(words[2 * j], words[2 * j + 1]);
}

// The 128-bit big-endian bit length of the stream, into the last block.
HSV_INL void msg_length_field(uint64_t w[16], uint64_t mlen) {
  const uint64_t total = kMsgHeadBytes + mlen;
  w[14] = total >> 61;
  w[15] = total << 3;
}

// The 64 digest bytes as 16 little-endian words (the integer sc_reduce512 reads).
HSV_INL void msg_digest_words(const uint64_t h[8], uint32_t out[16]) {
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) {
    out[2 * i] = bswap32((uint32_t)(h[i] >> 32));
    out[2 * i + 1] = bswap32((uint32_t)h[i]);
  }
}

// out = SHA-512(head || M) for the message of mlen bytes at stream byte
// address `start` (chunk q of the loader holds stream bytes [16 q, 16 q + 16)).
template <class LoadChunk>
HSV_INL void msg_hash(LoadChunk &ld, const uint32_t head[16], uint64_t start, uint64_t mlen, uint32_t out[16]) {
  uint64_t h[8];
  sha512_init(h);
  const uint64_t nblocks = msg_num_blocks(mlen);
  const uint64_t q_last = mlen ? (start + mlen - 1) >> 4 : 0;
  const uint32_t sh16 = (uint32_t)(start & 15u);
  HSV_NOUNROLL
  for (uint64_t b = 0; b < nblocks; ++b) {
    uint64_t w[16];
    const uint64_t off = msg_block_offset(b);
    uint32_t words[32];
    HSV_UNROLL
    for (int j = 0; j < 32; ++j) words[j] = 0u;
    if (b == 0) {
      if (off < mlen) tx_load_words<16>(ld, start >> 4, sh16, q_last, words);
      msg_block0_words(head, words, mlen, w);
    } else {
      if (off < mlen) tx_load_words<32>(ld, (start + off) >> 4, sh16, q_last, words);
      msg_block_words(words, mlen, b, w);
    }
    if (b + 1 == nblocks) msg_length_field(w, mlen);
    sha512_compress(h, w);
  }
  msg_digest_words(h, out);
}

// ---- a head of HB bytes (the signer's two hashes, hsv_msgsign.hpp) --------------
// The same stream with a head of HB bytes, HB = 32 (prefix || M, the nonce) or
// 64 (R || pk || M, the challenge):
//     block 0      = the HB / 4 head words, then message bytes [0, 128 - HB)
//     block b >= 1 = message bytes [128 b - HB, 128 b - HB + 128)
//     nblocks      = (HB + mlen + 17 + 127) >> 7,  length field (HB + mlen) * 8.
// HB = 64 is the arithmetic above under other names.
template <int HB>
HSV_INL uint64_t head_num_blocks(uint64_t mlen) {
  static_assert(HB == 32 || HB == 64, "head of 32 or 64 bytes");
  return ((uint64_t)HB + mlen + 1 + 16 + 127) >> 7;
}

template <int HB>
HSV_INL uint64_t head_block_offset(uint64_t b) { return b ? 128u * b - (uint64_t)HB : 0u; }

// Block 0: head = HB / 4 little-endian words, words = message bytes
// [0, 128 - HB) as little-endian words (anything past mlen is ignored).
template <int HB>
HSV_INL void head_block0_words(const uint32_t head[HB / 4], const uint32_t words[(128 - HB) / 4], uint64_t mlen,
                               uint64_t w[16]) {
  constexpr int HQ = HB / 8;
  HSV_UNROLL
  for (int j = 0; j < HQ; ++j) w[j] = be64_from_le32(head[2 * j], head[2 * j + 1]);
  HSV_UNROLL
  for (int j = 0; j < 16 - HQ; ++j)
    w[HQ + j] = tx_pad_word(be64_from_le32(words[2 * j], words[2 * j + 1]), (int64_t)mlen - (int64_t)(8 * j));
}

// Block b >= 1: words = message bytes [128 b - HB, 128 b - HB + 128).
template <int HB>
HSV_INL void head_block_words(const uint32_t words[32], uint64_t mlen, uint64_t b, uint64_t w[16]) {
  HSV_UNROLL
  for (int j = 0; j < 16; ++j) {
    const int64_t rem = (int64_t)mlen - (int64_t)(head_block_offset<HB>(b) + 8 * (uint64_t)j);
    w[j] = tx_pad_word(be64_from_le32(words[2 * j], words[2 * j + 1]), rem);
  }
}

template <int HB>
HSV_INL void head_length_field(uint64_t w[16], uint64_t mlen) {
  const uint64_t total = (uint64_t)HB + mlen;
  w[14] = total >> 61;
  w[15] = total << 3;
}

// out = SHA-512(head || M), one lane end to end: msg_hash for a head of HB
// bytes.  The kernels' form is msg_hash_wave (hsv_msgwave.hpp).
template <int HB, class LoadChunk>
HSV_INL void head_msg_hash(LoadChunk &ld, const uint32_t head[HB / 4], uint64_t start, uint64_t mlen,
                           uint32_t out[16]) {
  constexpr int NW0 = (128 - HB) / 4;
  uint64_t h[8];
  sha512_init(h);
  const uint64_t nblocks = head_num_blocks<HB>(mlen);
  const uint64_t q_last = mlen ? (start + mlen - 1) >> 4 : 0;
  const uint32_t sh16 = (uint32_t)(start & 15u);
  HSV_NOUNROLL
  for (uint64_t b = 0; b < nblocks; ++b) {
    uint64_t w[16];
    const uint64_t off = head_block_offset<HB>(b);
    uint32_t words[32];
    HSV_UNROLL
    for (int j = 0; j < 32; ++j) words[j] = 0u;
    if (b == 0) {
      if (off < mlen) tx_load_words<NW0>(ld, start >> 4, sh16, q_last, words);
      head_block0_words<HB>(head, words, mlen, w);
    } else {
      if (off < mlen) tx_load_words<32>(ld, (start + off) >> 4, sh16, q_last, words);
      head_block_words<HB>(words, mlen, b, w);
    }
    if (b + 1 == nblocks) head_length_field<HB>(w, mlen);
    sha512_compress(h, w);
  }
  msg_digest_words(h, out);
}

}  // namespace hsv
