// C ABI of the batch signer (include/hsv.h, hsv_signer_*): the GPU form of
//   crypto::generate_keypair  (reference crypto/src/lib.rs:167-175)
//   crypto::Signature::new    (reference crypto/src/lib.rs:185-191)
// A signer holds, in HBM of the device bound at creation, one 96-byte
// expanded record a | prefix | pk per key (hsv_keygen_kernel) and signs from
// them with hsv_sign_kernel (csrc/hsv_signer.hip).  There is no CPU fallback:
// hsv_sign_many is the host signer.
// hsv_signer_sign_transactions* is the signing mirror of hsv_verify_transactions*
// (the client's half of mempool/src/batch_maker.rs:79-85): pk || R || s into the
// last 96 bytes of every transaction, in place (csrc/hsv_txsign.hpp).
// hsv_signer_sign_msgs* is the signing mirror of hsv_verify_msgs*: whole
// messages of any lengths, by offsets or at a fixed stride, in three launches
// per round (csrc/hsv_msgsign.hpp).
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "hsv_host.h"

using namespace hsvh;

struct hsv_signer {
  int device = 0;
  size_t n = 0;
  uint8_t *d_keys = nullptr;   // n records of 96 B
  std::vector<uint8_t> h_pks;  // n * 32 B
};

namespace {

// launches of at most kChunk items, one after the other on `stream`
hipError_t sign_chunks(const hsv_signer &s, const uint32_t *d_key_idx, const uint8_t *d_msg, size_t msg_len,
                       size_t msg_stride, size_t m, uint8_t *d_sig, size_t sig_stride, const uint32_t *comb16,
                       uint32_t *fault, hipStream_t stream) {
  hipError_t e = hipSuccess;
  for (size_t base = 0; base < m && e == hipSuccess; base += kChunk) {
    const size_t k = std::min(kChunk, m - base);
    // key_idx == NULL: item i uses key i, so a chunk's records start at its base
    e = hsv_launch_sign(s.d_keys + (d_key_idx ? 0 : base * 96), (uint32_t)(d_key_idx ? s.n : s.n - base),
                        d_key_idx ? d_key_idx + base : nullptr, d_msg + base * msg_stride, msg_len, msg_stride,
                        (uint32_t)k, d_sig + base * sig_stride, sig_stride, comb16, fault, stream);
  }
  return e;
}

int sign_args_ok(const hsv_signer *s, const uint32_t *key_idx, const void *msg, size_t msg_len, size_t msg_stride,
                 size_t m, const void *sig) {
  if (!s || !sig || (!msg && msg_len)) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (msg_stride != 0 && msg_stride < msg_len) return fail(HSV_ERR_INVALID_ARG, "messages overlap");
  if (m > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if (!key_idx && m > s->n) return fail(HSV_ERR_INVALID_ARG, "more items than keys and no key_idx");
  return HSV_OK;
}

// ---- transactions (hsv_signer_sign_transactions*) -------------------------------
std::atomic<size_t> g_tx_chunk{kChunk};  // items per launch (hsvi_set_tx_sign_chunk: tests)

// launches of at most g_tx_chunk items, one after the other on `stream`;
// d_offsets are relative to d_txs, so a chunk only moves along the offsets
hipError_t tx_sign_chunks(const hsv_signer &s, const uint32_t *d_key_idx, uint8_t *d_txs, const uint64_t *d_offsets,
                          size_t tx_size, size_t n, const uint32_t *comb16, uint32_t *fault, hipStream_t stream) {
  const size_t per = g_tx_chunk.load();
  hipError_t e = hipSuccess;
  for (size_t base = 0; base < n && e == hipSuccess; base += per) {
    const size_t k = std::min(per, n - base);
    // key_idx == NULL: item i uses key i (n <= s.n), so a chunk's records start at its base
    const size_t kb = std::min(base, s.n);
    e = hsv_launch_tx_sign(s.d_keys + (d_key_idx ? 0 : kb * 96), (uint32_t)(d_key_idx ? s.n : s.n - kb),
                           d_key_idx ? d_key_idx + base : nullptr, d_offsets ? d_txs : d_txs + base * tx_size,
                           d_offsets ? d_offsets + base : nullptr, tx_size, (uint32_t)k, comb16, fault, stream);
  }
  return e;
}

// ---- whole messages (hsv_signer_sign_msgs*) --------------------------------------
std::atomic<size_t> g_msg_chunk{kChunk};  // items per round (hsvi_set_msg_sign_chunk: tests)

// One round: items [base, base + k) of a batch whose keys, when key_idx is
// NULL, are those of items first.. (item i uses key i).
hipError_t msg_sign_round(const hsv_signer &s, size_t first, const uint32_t *d_key_idx, const uint8_t *d_msgs,
                          const uint64_t *d_offsets, size_t msg_len, size_t msg_stride, size_t k, uint8_t *d_sig,
                          size_t sig_stride, const uint32_t *comb16, uint32_t *fault, hipStream_t stream) {
  const size_t kb = std::min(first, s.n);
  return hsv_launch_msg_sign(s.d_keys + (d_key_idx ? 0 : kb * 96), (uint32_t)(d_key_idx ? s.n : s.n - kb), d_key_idx,
                             d_msgs, d_offsets, msg_len, msg_stride, (uint32_t)k, d_sig, sig_stride, comb16, fault,
                             stream);
}

}  // namespace

extern "C" size_t hsvi_set_tx_sign_chunk(size_t items) {
  return g_tx_chunk.exchange(items == 0 || items > kChunk ? kChunk : items);
}

extern "C" size_t hsvi_set_msg_sign_chunk(size_t items) {
  return g_msg_chunk.exchange(items == 0 || items > kChunk ? kChunk : items);
}

extern "C" {

int hsv_signer_create(const uint8_t *seeds, size_t nkeys, hsv_signer **out) {
  if (!out || (!seeds && nkeys)) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (nkeys > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "too many keys");
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  const int dev = home_device();
  DeviceGuard guard(dev);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  DevCtx &c = ctx(dev);
  rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  std::unique_ptr<hsv_signer> s(new hsv_signer());
  s->device = dev;
  s->n = nkeys;
  s->h_pks.resize(nkeys * 32);
  if (nkeys) {
    uint8_t *d_seeds = nullptr;
    uint32_t *d_fault = nullptr;
    hipStream_t st = nullptr;
    uint8_t words[kFaultBytes] = {0};
    hipError_t e = hipMalloc(&s->d_keys, nkeys * 96);
    if (e == hipSuccess) e = hipMalloc(&d_seeds, nkeys * 32);
    if (e == hipSuccess) e = hipMalloc(&d_fault, 256);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(d_seeds, seeds, nkeys * 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_fault, 0, kFaultBytes, st);
    for (size_t base = 0; base < nkeys && e == hipSuccess; base += kChunk)
      e = hsv_launch_keygen(d_seeds + base * 32, (uint32_t)std::min(kChunk, nkeys - base), s->d_keys + base * 96,
                            c.d_btable16, d_fault, st);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(s->h_pks.data(), 32, s->d_keys + 64, 96, 32, nkeys, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(words, d_fault, kFaultBytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (st) (void)hipStreamDestroy(st);
    {
      ResidentPause pause;  // hipFree waits for every grid on the device
      if (d_seeds) (void)hipFree(d_seeds);
      if (d_fault) (void)hipFree(d_fault);
    }
    if (e == hipSuccess) rc = check_faults(words, "hsv_signer_create");
    if (e != hipSuccess || rc != HSV_OK) {
      hsv_signer_destroy(s.release());
      return e != hipSuccess ? hip_fail("expanding the signer's keys", e) : rc;
    }
  }
  *out = s.release();
  return HSV_OK;
}

void hsv_signer_destroy(hsv_signer *s) {
  if (!s) return;
  if (s->d_keys) {
    ResidentPause pause;  // hipFree waits for every grid on the device
    DeviceGuard guard(s->device);
    (void)hipFree(s->d_keys);
  }
  delete s;
}

size_t hsv_signer_size(const hsv_signer *s) { return s ? s->n : 0; }

int hsv_signer_public_keys(const hsv_signer *s, uint8_t *pk_out) {
  if (!s || (!pk_out && s->n)) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (s->n) std::memcpy(pk_out, s->h_pks.data(), s->n * 32);
  return HSV_OK;
}

int hsv_signer_sign_device(const hsv_signer *s, const uint32_t *d_key_idx, const uint8_t *d_msg, size_t msg_len,
                           size_t msg_stride, size_t m, uint8_t *d_sig, size_t sig_stride, uint32_t *d_fault,
                           void *stream) {
  if (m == 0) return HSV_OK;
  // misaligned pointers are rejected before anything is looked at (as hsv_verify_device)
  if (((reinterpret_cast<uintptr_t>(d_sig) | sig_stride) & 15u) != 0)
    return fail(HSV_ERR_ALIGN, "d_sig and sig_stride must be multiples of 16");
  if (reinterpret_cast<uintptr_t>(d_key_idx) & 3u) return fail(HSV_ERR_ALIGN, "d_key_idx must be 4-byte aligned");
  int rc = sign_args_ok(s, d_key_idx, d_msg, msg_len, msg_stride, m, d_sig);
  if (rc != HSV_OK) return rc;
  if (sig_stride < 64) return fail(HSV_ERR_INVALID_ARG, "signatures overlap");
  DeviceCall call;
  rc = call.begin(d_sig, stream, d_fault, DeviceCall::kWide, "signer", s->device);
  if (rc != HSV_OK) return rc;
  const hipError_t e = sign_chunks(*s, d_key_idx, d_msg, msg_len, msg_stride, m, d_sig, sig_stride, call.comb,
                                   call.fault, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("sign kernel launch", e);
}

int hsv_signer_sign(hsv_signer *s, const uint32_t *key_idx, const uint8_t *msgs, size_t msg_len, size_t msg_stride,
                    size_t m, uint8_t *sig_out) {
  if (m == 0) return HSV_OK;
  int rc = sign_args_ok(s, key_idx, msgs, msg_len, msg_stride, m, sig_out);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(s->device);
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  SlotLease lease(c);
  Slot &slot = lease.slot();
  rc = slot_prepare(slot, 0, 0);
  if (rc != HSV_OK) return rc;
  const size_t msg_bytes = BatchSpan{nullptr, msg_stride, msg_len}.span_bytes(0, m);
  StagedBlock blk(slot.stream);
  const size_t off_sig = blk.add(m * 64), off_idx = blk.add(key_idx ? m * 4 : 0), off_msg = blk.add(msg_bytes);
  rc = blk.alloc("allocating the signing buffers");
  if (rc != HSV_OK) return rc;
  uint32_t *d_idx = key_idx ? reinterpret_cast<uint32_t *>(blk.at(off_idx)) : nullptr;
  if (key_idx) blk.in(off_idx, key_idx, m * 4);
  blk.in(off_msg, msgs, msg_bytes);
  if (blk.ok())
    blk.step(sign_chunks(*s, d_idx, blk.at(off_msg), msg_len, msg_stride, m, blk.at(off_sig), 64, c.d_btable16,
                         blk.fault(), slot.stream));
  blk.out(sig_out, off_sig, m * 64);
  return blk.finish("hsv_signer_sign");
}

int hsv_signer_sign_transactions_device(const hsv_signer *s, const uint32_t *d_key_idx, uint8_t *d_txs,
                                        const uint64_t *d_offsets, size_t tx_size, size_t n, uint32_t *d_fault,
                                        void *stream) {
  if (n == 0) return HSV_OK;
  if (!s || !d_txs) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (reinterpret_cast<uintptr_t>(d_key_idx) & 3u) return fail(HSV_ERR_ALIGN, "d_key_idx must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return fail(HSV_ERR_ALIGN, "d_offsets must be 8-byte aligned");
  if (!d_offsets && tx_size < 96) return fail(HSV_ERR_INVALID_ARG, "transactions are shorter than 96 bytes");
  if (n > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  DeviceCall call;
  const int rc = call.begin(d_txs, stream, d_fault, DeviceCall::kWide, "signer", s->device);
  if (rc != HSV_OK) return rc;
  if (!d_key_idx && n > s->n) return fail(HSV_ERR_INVALID_ARG, "more items than keys and no key_idx");
  const hipError_t e = tx_sign_chunks(*s, d_key_idx, d_txs, d_offsets, tx_size, n, call.comb, call.fault, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("transaction sign launch", e);
}

int hsv_signer_sign_transactions(hsv_signer *s, const uint32_t *key_idx, uint8_t *txs, const uint64_t *offsets,
                                 size_t tx_size, size_t n) {
  if (n == 0) return HSV_OK;
  if (!s || !txs) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (n > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  int rc = tx_lengths_ok(offsets, tx_size, n);  // the length check of hsv_verify_transactions
  if (rc != HSV_OK) return rc;
  rc = ensure_init();
  if (rc != HSV_OK) return rc;
  if (!key_idx && n > s->n) return fail(HSV_ERR_INVALID_ARG, "more items than keys and no key_idx");
  DevCtx &c = ctx(s->device);
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  SlotLease lease(c);
  Slot &slot = lease.slot();
  rc = slot_prepare(slot, 0, 0);
  if (rc != HSV_OK) return rc;
  hipStream_t st = slot.stream;
  const BatchSpan span{offsets, tx_size, tx_size};
  std::vector<uint64_t> rel;  // a chunk's offsets, relative to its first byte
  std::vector<uint8_t> back;  // a ragged chunk as the device left it
  for (size_t a = 0, b; a < n; a = b) {
    b = span.chunk_end(a, n, g_tx_chunk.load(), g_stage_bytes.load());  // one launch
    const size_t m = b - a, first = span.first_byte(a), bytes = span.span_bytes(a, b);
    StagedBlock blk(st);
    const size_t off_idx = blk.add(key_idx ? m * 4 : 0), off_offs = blk.add(offsets ? (m + 1) * 8 : 0);
    const size_t off_tx = blk.add(bytes);
    rc = blk.alloc("allocating the transaction signing buffers");
    if (rc != HSV_OK) return rc;
    uint32_t *d_idx = key_idx ? reinterpret_cast<uint32_t *>(blk.at(off_idx)) : nullptr;
    uint64_t *d_offs = offsets ? reinterpret_cast<uint64_t *>(blk.at(off_offs)) : nullptr;
    if (key_idx) blk.in(off_idx, key_idx + a, m * 4);
    if (offsets) {
      rel.resize(m + 1);
      span.rel_offsets(a, b, rel.data());
      blk.in(off_offs, rel.data(), (m + 1) * 8);
    }
    blk.in(off_tx, txs + first, bytes);
    if (blk.ok()) {
      const size_t kb = std::min(a, s->n);  // key_idx == NULL: item i uses key i
      blk.step(hsv_launch_tx_sign(s->d_keys + (key_idx ? 0 : kb * 96), (uint32_t)(key_idx ? s->n : s->n - kb), d_idx,
                                  blk.at(off_tx), d_offs, tx_size, (uint32_t)m, c.d_btable16, blk.fault(), st));
    }
    // only the tails come back: the caller's message bytes are never written
    if (blk.ok() && !offsets)
      blk.step(hipMemcpy2DAsync(txs + first + (tx_size - 96), tx_size, blk.at(off_tx) + (tx_size - 96), tx_size, 96, m,
                                hipMemcpyDeviceToHost, st));
    if (offsets) {
      back.resize(bytes);
      blk.out(back.data(), off_tx, bytes);
    }
    const bool copied = blk.ok();
    rc = blk.finish("hsv_signer_sign_transactions");
    if (offsets && copied && (rc == HSV_OK || rc == HSV_ERR_DEVICE_FAULT))
      for (size_t k = 0; k < m; ++k) std::memcpy(txs + first + rel[k + 1] - 96, back.data() + rel[k + 1] - 96, 96);
    if (rc != HSV_OK) return rc;
  }
  return HSV_OK;
}

int hsv_signer_sign_msgs_device(const hsv_signer *s, const uint32_t *d_key_idx, const uint8_t *d_msgs,
                                const uint64_t *d_offsets, size_t msg_len, size_t msg_stride, size_t m,
                                uint8_t *d_sig, size_t sig_stride, uint32_t *d_fault, void *stream) {
  if (m == 0) return HSV_OK;
  // misaligned pointers are rejected before anything is looked at (as hsv_signer_sign_device)
  if (((reinterpret_cast<uintptr_t>(d_sig) | sig_stride) & 15u) != 0)
    return fail(HSV_ERR_ALIGN, "d_sig and sig_stride must be multiples of 16");
  if (reinterpret_cast<uintptr_t>(d_key_idx) & 3u) return fail(HSV_ERR_ALIGN, "d_key_idx must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return fail(HSV_ERR_ALIGN, "d_offsets must be 8-byte aligned");
  if (!s || !d_sig || (!d_msgs && !d_offsets && msg_len)) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (!d_offsets && msg_stride != 0 && msg_stride < msg_len) return fail(HSV_ERR_INVALID_ARG, "messages overlap");
  if (sig_stride < 64) return fail(HSV_ERR_INVALID_ARG, "signatures overlap");
  if (m > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  DeviceCall call;
  const int rc = call.begin(d_sig, stream, d_fault, DeviceCall::kWide, "signer", s->device);
  if (rc != HSV_OK) return rc;
  if (!d_key_idx && m > s->n) return fail(HSV_ERR_INVALID_ARG, "more items than keys and no key_idx");
  const size_t per = g_msg_chunk.load();
  hipError_t e = hipSuccess;
  // d_offsets are relative to d_msgs, so a round only moves along the offsets
  for (size_t base = 0; base < m && e == hipSuccess; base += per)
    e = msg_sign_round(*s, base, d_key_idx ? d_key_idx + base : nullptr,
                       d_offsets ? d_msgs : d_msgs + base * msg_stride, d_offsets ? d_offsets + base : nullptr, msg_len,
                       msg_stride, std::min(per, m - base), d_sig + base * sig_stride, sig_stride, call.comb,
                       call.fault, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("message sign launch", e);
}

int hsv_signer_sign_msgs(hsv_signer *s, const uint32_t *key_idx, const uint8_t *msgs, const uint64_t *offsets,
                         size_t msg_len, size_t msg_stride, size_t m, uint8_t *sig_out) {
  if (m == 0) return HSV_OK;
  if (!s || !sig_out) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = msgs_host_args_ok(msgs, offsets, msg_len, msg_stride, m);  // the checks of hsv_verify_msgs
  if (rc != HSV_OK) return rc;
  rc = ensure_init();
  if (rc != HSV_OK) return rc;
  if (!key_idx && m > s->n) return fail(HSV_ERR_INVALID_ARG, "more items than keys and no key_idx");
  DevCtx &c = ctx(s->device);
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  SlotLease lease(c);
  Slot &slot = lease.slot();
  rc = slot_prepare(slot, 0, 0);
  if (rc != HSV_OK) return rc;
  hipStream_t st = slot.stream;
  const BatchSpan span{offsets, msg_stride, msg_len};
  std::vector<uint64_t> rel;  // a round's offsets, relative to its first byte
  for (size_t a = 0, b; a < m; a = b) {
    b = span.chunk_end(a, m, g_msg_chunk.load(), g_stage_bytes.load());  // one round
    const size_t k = b - a, bytes = span.span_bytes(a, b);
    StagedBlock blk(st);
    const size_t off_sig = blk.add(k * 64), off_idx = blk.add(key_idx ? k * 4 : 0);
    const size_t off_offs = blk.add(offsets ? (k + 1) * 8 : 0), off_msg = blk.add(bytes);
    rc = blk.alloc("allocating the message signing buffers");
    if (rc != HSV_OK) return rc;
    uint32_t *d_idx = key_idx ? reinterpret_cast<uint32_t *>(blk.at(off_idx)) : nullptr;
    uint64_t *d_offs = offsets ? reinterpret_cast<uint64_t *>(blk.at(off_offs)) : nullptr;
    if (key_idx) blk.in(off_idx, key_idx + a, k * 4);
    if (offsets) {
      rel.resize(k + 1);
      span.rel_offsets(a, b, rel.data());
      blk.in(off_offs, rel.data(), (k + 1) * 8);
    }
    if (msgs) blk.in(off_msg, msgs + span.first_byte(a), bytes);  // NULL: every message is empty
    if (blk.ok())
      blk.step(msg_sign_round(*s, a, d_idx, blk.at(off_msg), d_offs, msg_len, msg_stride, k, blk.at(off_sig), 64,
                              c.d_btable16, blk.fault(), st));
    blk.out(sig_out + a * 64, off_sig, k * 64);
    rc = blk.finish("hsv_signer_sign_msgs");
    if (rc != HSV_OK) return rc;
  }
  return HSV_OK;
}

}  // extern "C"
