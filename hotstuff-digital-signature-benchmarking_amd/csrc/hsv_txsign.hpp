// Signing mempool transactions in place (hsv_signer_sign_transactions*,
// include/hsv.h): the signing mirror of hsv_verify_transactions*.
//
// A client transaction is  message || pk (32) || R || s (64)  with the
// signature over Digest(SHA-512(message)[..32]) (hsv_txhash.hpp; reference
// mempool/src/batch_maker.rs:79-85).  The signer fills in the last 96 bytes:
//   1. the digest launch: one lane per transaction hashes the message and
//      writes the 8 digest words and the item's slot status (sign / zero /
//      skip) into the launch workspace;
//   2. the signing launch: sign_lane's one-block fast path over those digests
//      (hsv_sign_core.hpp), with TxSignIo below for the status and the store.
//
// The store is the one new device routine.  A transaction starts and ends at
// any byte, so in a batch of equal transactions whose size is no multiple of 4
// the signature of transaction i and the message of transaction i + 1 share a
// 32-bit word, and neighbouring lanes write neighbouring transactions at the
// same time: tx_store_tail never reads a word back and never writes a byte
// outside [p, p + 96) -- byte stores up to the first 4-byte boundary, aligned
// word stores (realigned in registers) between, byte stores after the last.
//
// Everything here also builds for the host (tests/native/txsign_host.cpp).
#pragma once
#include "hsv_sign_core.hpp"
#include "hsv_txhash.hpp"

namespace hsv {

constexpr int kTxTailBytes = 96;  // pk || R || s

// Transaction i spans [lo, hi) bytes of txs, by the convention of
// hsv_verify_transactions_device (tx_span, hsv_mempool.hip); false for a
// transaction shorter than 96 bytes or a decreasing pair of offsets.
HSV_INL bool tx_sign_span(const uint64_t *offsets, uint64_t tx_size, uint64_t i, uint64_t &lo, uint64_t &hi) {
  if (offsets) {
    lo = offsets[i];
    hi = offsets[i + 1];
  } else {
    lo = i * tx_size;
    hi = lo + tx_size;
  }
  return hi >= lo && hi - lo >= (uint64_t)kTxTailBytes;
}

// The slot status the digest launch records for an item: a span that holds no
// tail is skipped (nothing of it is written), a key index out of range gets
// 96 zero bytes, every other item is hashed and signed.
HSV_INL uint32_t tx_sign_status(bool span_ok, uint32_t ki, uint32_t nkeys) {
  return !span_ok ? (uint32_t)kSlotDead : ki < nkeys ? (uint32_t)kSlotOk : (uint32_t)kSlotZero;
}

// One item of the digest launch without the wave's staging (the kernel's form
// is hsv_tx_digest_kernel, hsv_txsign.hip): status, and for kSlotOk the digest.
// base16: the low four address bits of txs; ld: the chunk loader of
// hsv_txhash.hpp over txs rounded down to 16 bytes.
template <class LoadChunk>
HSV_INL uint32_t tx_digest_item(LoadChunk &ld, uint32_t base16, const uint64_t *offsets, uint64_t tx_size,
                                const uint32_t *key_idx, uint32_t nkeys, uint64_t i, uint32_t dig[8]) {
  uint64_t lo = 0, hi = 0;
  const bool ok = tx_sign_span(offsets, tx_size, i, lo, hi);
  const uint32_t status = tx_sign_status(ok, key_idx ? key_idx[i] : (uint32_t)i, nkeys);
  HSV_UNROLL
  for (int j = 0; j < 8; ++j) dig[j] = 0u;
  if (status == kSlotOk) {
    const uint64_t start = (uint64_t)base16 + lo;
    tx_message_digest(ld, start, hi - lo - kTxTailBytes, (start + (hi - lo) - 1) >> 4, dig);
  }
  return status;
}

// ---- the unaligned tail store -------------------------------------------------
HSV_INL void tx_store_u32(uint8_t *p, uint32_t v) {  // p 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint32_t *>(p) = v;
#else
  if (reinterpret_cast<uintptr_t>(p) & 3u) __builtin_trap();  // host test build: a word store off its boundary
  HSV_UNROLL
  for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
#endif
}

// The 96 bytes of w (24 little-endian words) to [p, p + 96), p at any byte.
// No byte outside that range is written and none is read.
HSV_INL void tx_store_tail(uint8_t *p, const uint32_t w[24]) {
  const uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u)) & 3u;  // bytes before the first boundary
  HSV_UNROLL
  for (uint32_t k = 0; k < 3; ++k)
    if (k < head) p[k] = (uint8_t)(w[0] >> (8u * k));
  uint8_t *q = p + head;  // 4-byte aligned
  HSV_UNROLL
  for (int j = 0; j < 23; ++j) tx_store_u32(q + 4 * j, tx_funnel(w[j], w[j + 1], head));
  // 4 - head bytes are left, bytes head.. of w[23]: one word when p is aligned
  if (head == 0) {
    tx_store_u32(q + 92, w[23]);
  } else {
    HSV_UNROLL
    for (uint32_t k = 0; k < 3; ++k)
      if (k < 4u - head) q[92 + k] = (uint8_t)(w[23] >> (8u * (head + k)));
  }
}

// ---- sign_lane's status and store for transactions ------------------------------
struct TxSignIo {
  static constexpr bool kPointOnly = false;
  const uint32_t *status;   // per item, from the digest launch
  uint8_t *txs;
  const uint64_t *offsets;  // or NULL: fixed tx_size
  uint64_t tx_size;
  HSV_MEMBER uint32_t slot(const SignArgs &, uint64_t i, uint32_t) const { return status[i]; }
  // pk || R || s; pk || 0 for an item that failed the self-check; 0 for a key out of range
  HSV_MEMBER void store(const SignArgs &a, uint64_t i, uint32_t st, const uint32_t sigw[16]) const {
    uint32_t w[24];
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) w[j] = 0u;
    if (st != kSlotZero) {
      const uint32_t ki = a.key_idx ? a.key_idx[i] : (uint32_t)i;
      sign_load16<8>(a.keys + (uint64_t)ki * kSignKeyBytes + 64, w);
    }
    HSV_UNROLL
    for (int j = 0; j < 16; ++j) w[8 + j] = sigw[j];
    uint64_t lo = 0, hi = 0;
    tx_sign_span(offsets, tx_size, i, lo, hi);  // holds: the digest launch skips every other item
    tx_store_tail(txs + (hi - kTxTailBytes), w);
  }
};

}  // namespace hsv
