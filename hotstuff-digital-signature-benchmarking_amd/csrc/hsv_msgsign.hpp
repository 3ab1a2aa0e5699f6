// Signing whole messages of any lengths (hsv_signer_sign_msgs*, include/hsv.h):
// the signing mirror of hsv_verify_msgs*.  Message i is msgs[offsets[i],
// offsets[i+1]) or msg_len bytes at msgs + i * msg_stride, at any byte address,
// possibly empty; the output is R || s of RFC 8032 in the item's 64-byte slot.
//
// A round is three launches on one stream (kernels: hsv_msgsign.hip):
//   1. nonce:    one lane per item.  Slot status (sign / zero), r =
//                SHA-512(prefix || M) mod l.  Writes r (8 words) and the status
//                (1 word) into the launch workspace.
//   2. point:    sign_lane's group structure (hsv_sign_core.hpp) with
//                MsgSignIo below: r is read from the workspace instead of
//                hashed, G items per lane share one fe_invert, enc(R) goes to
//                the first 32 bytes of the item's slot, a failed self-check
//                turns the status into kSlotFault.
//   3. response: one lane per item.  k = SHA-512(R || pk || M) mod l with R
//                read back from the slot, s = r + k a to bytes 32..64; an item
//                that is not kSlotOk gets its 64 bytes zeroed here.
// Both hashes are the verifier's staged message hash with the head generalised
// to HB = 32 and 64 bytes (hsv_msghash.hpp, hsv_msgwave.hpp).
//
// This header holds what a lane does around its hash, so that it also builds
// for the host (tests/native/msgsign_host.cpp), where head_msg_hash stands in
// for the wave's staged loop.  As all of the signer: NOT constant time.
#pragma once
#include "hsv_msghash.hpp"
#include "hsv_sign_core.hpp"

namespace hsv {

constexpr int kMsgSignWsWords = 9;  // r (8) and the status, on top of the point launch's kSignWsWords

// Message i spans [lo, lo + mlen) of msgs; false for a decreasing pair of
// offsets (lo = mlen = 0 then: nothing of it is read).
HSV_INL bool msg_sign_span(const uint64_t *offsets, uint64_t msg_len, uint64_t msg_stride, uint64_t i, uint64_t &lo,
                           uint64_t &mlen) {
  uint64_t hi;
  if (offsets) {
    lo = offsets[i];
    hi = offsets[i + 1];
  } else {
    lo = i * msg_stride;
    hi = lo + msg_len;
  }
  const bool ok = hi >= lo;
  mlen = ok ? hi - lo : 0;
  if (!ok) lo = 0;
  return ok;
}

// The status the nonce launch records: a key index out of range or a
// decreasing pair of offsets gets 64 zero bytes and no fault.
HSV_INL uint32_t msg_sign_status(bool span_ok, uint32_t ki, uint32_t nkeys) {
  return span_ok && ki < nkeys ? (uint32_t)kSlotOk : (uint32_t)kSlotZero;
}

// ---- nonce launch ------------------------------------------------------------
// The head of the nonce hash: the key's prefix, or zeros for an item that is
// not signed (its hash is computed and dropped; its message length is 0).
HSV_INL void msg_nonce_head(const uint8_t *keys, uint32_t ki, uint32_t status, uint32_t head[8]) {
  HSV_UNROLL
  for (int j = 0; j < 8; ++j) head[j] = 0u;
  if (status == kSlotOk) sign_load16<8>(keys + (uint64_t)ki * kSignKeyBytes + 32, head);
}

// hw = SHA-512(prefix || M) -> r, 8 words (zeros for an item that is not signed)
HSV_INL void msg_nonce_finish(const uint32_t hw[16], uint32_t status, uint32_t r[8]) {
  const sc x = sc_reduce512(hw);
  HSV_UNROLL
  for (int j = 0; j < 8; ++j) r[j] = status == kSlotOk ? x.v[j] : 0u;
}

// ---- point launch: sign_lane's status, nonce and store ----------------------------
struct MsgSignIo {
  static constexpr bool kPointOnly = true;  // sign_lane hashes nothing: r comes from nonce(), only enc(R) is stored
  uint32_t *status;      // per item, from the nonce launch
  const uint8_t *nonce;  // per item 32 B, 16-byte aligned
  HSV_MEMBER uint32_t slot(const SignArgs &, uint64_t i, uint32_t) const { return status[i]; }
  HSV_MEMBER void nonce_words(uint64_t i, uint32_t r[8]) const { sign_load16<8>(nonce + i * 32u, r); }
  // kSlotOk: sigw[0..8) = enc(R); kSlotFault: recorded for the response launch, which zeroes the slot
  HSV_MEMBER void store(const SignArgs &a, uint64_t i, uint32_t st, const uint32_t sigw[16]) const {
    if (st == kSlotOk) sign_store16<8>(a.sig + i * a.sig_stride, sigw);
    else if (st == kSlotFault) status[i] = kSlotFault;
  }
};

// ---- response launch ---------------------------------------------------------
// The head of the challenge hash: enc(R) from the item's slot, pk from its key
// record; zeros for an item that is not kSlotOk.
HSV_INL void msg_response_head(const uint8_t *keys, uint32_t ki, uint32_t status, const uint8_t *slot,
                               uint32_t head[16]) {
  HSV_UNROLL
  for (int j = 0; j < 16; ++j) head[j] = 0u;
  if (status == kSlotOk) {
    sign_load16<8>(slot, head);
    sign_load16<8>(keys + (uint64_t)ki * kSignKeyBytes + 64, head + 8);
  }
}

// hw = SHA-512(R || pk || M) -> the slot's 16 words R || s, or zeros
HSV_INL void msg_response_finish(const uint32_t hw[16], const uint32_t head[16], const uint8_t *keys, uint32_t ki,
                                 uint32_t status, const uint8_t *nonce, uint32_t sigw[16]) {
  HSV_UNROLL
  for (int j = 0; j < 16; ++j) sigw[j] = 0u;
  if (status == kSlotOk) {
    const sc k = sc_reduce512(hw);
    sc sa, r;
    sign_load16<8>(keys + (uint64_t)ki * kSignKeyBytes, sa.v);
    sign_load16<8>(nonce, r.v);
    const sc s = sc_muladd(k, sa, r);
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) {
      sigw[j] = head[j];
      sigw[8 + j] = s.v[j];
    }
  }
}

// ---- one item without the wave's staging (the host build) ---------------------------
// base16: the low four address bits of msgs; ld: the chunk loader of
// hsv_txhash.hpp over msgs rounded down to 16 bytes.
template <class LoadChunk>
HSV_INL void msg_nonce_item(LoadChunk &ld, uint32_t base16, const uint8_t *keys, uint32_t nkeys,
                            const uint32_t *key_idx, const uint64_t *offsets, uint64_t msg_len, uint64_t msg_stride,
                            uint64_t i, uint32_t r[8], uint32_t &status) {
  uint64_t lo, mlen;
  const bool ok = msg_sign_span(offsets, msg_len, msg_stride, i, lo, mlen);
  const uint32_t ki = key_idx ? key_idx[i] : (uint32_t)i;
  status = msg_sign_status(ok, ki, nkeys);
  if (status != kSlotOk) mlen = 0;
  uint32_t head[8], hw[16];
  msg_nonce_head(keys, ki, status, head);
  head_msg_hash<32>(ld, head, (uint64_t)base16 + lo, mlen, hw);
  msg_nonce_finish(hw, status, r);
}

template <class LoadChunk>
HSV_INL void msg_response_item(LoadChunk &ld, uint32_t base16, const uint8_t *keys, const uint32_t *key_idx,
                               const uint64_t *offsets, uint64_t msg_len, uint64_t msg_stride, uint64_t i,
                               const uint8_t *nonce, const uint32_t *status, uint8_t *sig, uint64_t sig_stride) {
  const uint32_t st = status[i];
  uint64_t lo, mlen;
  msg_sign_span(offsets, msg_len, msg_stride, i, lo, mlen);
  if (st != kSlotOk) mlen = 0;
  const uint32_t ki = key_idx ? key_idx[i] : (uint32_t)i;
  uint32_t head[16], hw[16], sigw[16];
  msg_response_head(keys, ki, st, sig + i * sig_stride, head);
  head_msg_hash<64>(ld, head, (uint64_t)base16 + lo, mlen, hw);
  msg_response_finish(hw, head, keys, ki, st, nonce + i * 32u, sigw);
  sign_store16<16>(sig + i * sig_stride, sigw);
}

}  // namespace hsv
