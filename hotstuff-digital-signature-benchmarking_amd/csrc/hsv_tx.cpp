// Mempool transactions behind the C ABI.
// tx = message || pk (32) || sig (64); the signature is checked over
// Digest(SHA-512(message)[..32]) with Signature::verify, as in
// mempool/src/batch_maker.rs:79-85 and consensus/src/core.rs:121-127.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hsv.h"
#include "hsv_host.h"
#include "hsv_internal.h"

namespace hsvh {
namespace {

// records, verification and the short-transaction mask for m <= kChunk
// transactions already in HBM (d_offsets relative to d_txs, or NULL = fixed size)
int tx_enqueue(int v, const uint32_t *comb_b, const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size,
               size_t m, uint8_t *d_rec, uint8_t *d_flags, uint32_t *d_bits, uint32_t *d_fault, hipStream_t s) {
  hipError_t e = hsv_launch_verify_tx(v, d_txs, d_offsets, tx_size, (uint32_t)m, d_rec, d_flags, d_bits, comb_b,
                                      d_fault, s);
  if (e != hipSuccess) return hip_fail("transaction verify launch", e);
  e = hsv_launch_tx_mask(d_offsets, (uint32_t)m, d_flags, d_bits, s);
  if (e != hipSuccess) return hip_fail("transaction mask kernel launch", e);
  return HSV_OK;
}

}  // namespace

// "transaction i is shorter than 96 bytes" for the first such i of a ragged
// batch (or one whose offsets decrease), or for a fixed size below 96
int tx_lengths_ok(const uint64_t *offsets, size_t tx_size, size_t n) {
  if (!offsets)
    return tx_size < 96 ? fail(HSV_ERR_INVALID_ARG, "transactions are shorter than 96 bytes") : HSV_OK;
  const size_t bad = first_bad_item(offsets, n, 96);
  return bad == n ? HSV_OK
                  : fail(HSV_ERR_INVALID_ARG, "transaction " + std::to_string(bad) + " is shorter than 96 bytes");
}

// The one walk of the staged transaction host forms (hsv_host.h).  With
// rec_bytes = 0 the record region is empty and the device and host layouts
// coincide: byte for byte the layout the committee form had while it was a
// copy of this walk (tx bytes | offsets | flags | self-check words).
int staged_tx_host(DevCtx &c, const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t lo, size_t hi,
                   uint8_t *flags_out, size_t rec_bytes, const StagedBegin &begin, const TxLaunch &launch,
                   const char *where) {
  const BatchSpan span{offsets, tx_size, tx_size};
  std::vector<size_t> ends;  // the chunks' ends, in order from lo
  size_t max_items = 0, max_bytes = 0;
  for (size_t a = lo; a < hi; a = ends.back()) {
    ends.push_back(span.chunk_end(a, hi, kChunk, g_stage_bytes.load()));
    max_items = std::max(max_items, ends.back() - a);
    max_bytes = std::max(max_bytes, span.span_bytes(a, ends.back()));
  }
  // device: tx bytes | offsets | records | flags | self-check words;
  // host: tx bytes | offsets | flags | self-check words
  const size_t off_off = round_up(max_bytes, kAlign);
  const size_t rec_off = off_off + round_up((max_items + 1) * 8, kAlign);
  const size_t flag_off = rec_off + round_up(max_items * rec_bytes, kAlign);
  const size_t fault_off = flag_off + round_up(max_items, kAlign);
  const size_t d_total = fault_off + kAlign;
  const size_t h_flag_off = rec_off;
  const size_t h_fault_off = h_flag_off + round_up(max_items, kAlign);
  const size_t h_total = h_fault_off + kAlign;
  SlotLease lease(c);
  Slot &s = lease.slot();
  int rc = slot_prepare(s, d_total, h_total);
  if (rc == HSV_OK && begin) rc = begin(s.stream);
  if (rc != HSV_OK) return rc;
  size_t a = lo;
  for (const size_t b : ends) {
    const size_t m = b - a, bytes = span.span_bytes(a, b);
    uint8_t *h = s.h_buf;
    stage_copy(h, txs + span.first_byte(a), bytes);
    size_t in_bytes = bytes;
    if (offsets) {
      span.rel_offsets(a, b, reinterpret_cast<uint64_t *>(h + off_off));
      in_bytes = off_off + (m + 1) * 8;
    }
    hipError_t e = hipMemcpyAsync(s.d_buf, h, in_bytes, hipMemcpyHostToDevice, s.stream);
    // unwritten flags read as rejections; self-check words start at zero
    if (e == hipSuccess) e = hipMemsetAsync(s.d_buf + flag_off, 0, fault_off + kFaultBytes - flag_off, s.stream);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s.stream);
      return hip_fail("hipMemcpyAsync H2D", e);
    }
    rc = launch(s.d_buf, offsets ? reinterpret_cast<const uint64_t *>(s.d_buf + off_off) : nullptr, m,
                s.d_buf + rec_off, s.d_buf + flag_off, reinterpret_cast<uint32_t *>(s.d_buf + fault_off), s.stream);
    if (rc == HSV_OK) {
      e = hipMemcpyAsync(h + h_flag_off, s.d_buf + flag_off, fault_off + kFaultBytes - flag_off,
                         hipMemcpyDeviceToHost, s.stream);
      if (e != hipSuccess) rc = hip_fail("hipMemcpyAsync D2H", e);
    }
    e = hipStreamSynchronize(s.stream);  // nothing of this call stays in flight
    if (rc != HSV_OK) return rc;
    if (e != hipSuccess) return hip_fail("hipStreamSynchronize", e);
    rc = check_faults(h + h_fault_off, where);
    if (rc != HSV_OK) return rc;
    std::memcpy(flags_out + (a - lo), h + h_flag_off, m);
    a = b;
  }
  return HSV_OK;
}

int tx_device_args_ok(const uint64_t *d_offsets, size_t tx_size, const uint8_t *d_flags,
                      const uint32_t *d_strict_bits) {
  if (!d_flags && !d_strict_bits) return fail(HSV_ERR_INVALID_ARG, "no output");
  if (!d_offsets && tx_size < 96) return fail(HSV_ERR_INVALID_ARG, "transactions are shorter than 96 bytes");
  return HSV_OK;
}

namespace {

// transactions [lo, hi) of the caller's arrays on device c: the generic
// kernels, with their 128-byte record per item
int run_tx_on_device(DevCtx &c, const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t lo, size_t hi,
                     uint8_t *flags_out) {
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  const int v = variant();
  const uint32_t *comb_b = nullptr;
  const int rc = comb_table_for(c, v, &comb_b);
  if (rc != HSV_OK) return rc;
  return staged_tx_host(
      c, txs, offsets, tx_size, lo, hi, flags_out, 128, nullptr,
      [&](const uint8_t *d_txs, const uint64_t *d_offsets, size_t m, uint8_t *d_rec, uint8_t *d_flags,
          uint32_t *d_fault, hipStream_t s) {
        return tx_enqueue(v, comb_b, d_txs, d_offsets, tx_size, m, d_rec, d_flags, nullptr, d_fault, s);
      },
      "transaction verify");
}

int run_tx_host(const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t n, uint8_t *flags_out) {
  if (n == 0) return HSV_OK;
  if (!txs || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null pointer");
  int rc = tx_lengths_ok(offsets, tx_size, n);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();
  if (rc != HSV_OK) return rc;
  const int k = shard_count(n);
  if (k <= 1) return run_tx_on_device(ctx(home_device()), txs, offsets, tx_size, 0, n, flags_out);
  // contiguous shards, each on the shard worker of its GPU's node
  return run_sharded(k, [&](int d, int dev) {
    const size_t lo = n * d / k, hi = n * (d + 1) / k;
    return hi > lo ? run_tx_on_device(ctx(dev), txs, offsets, tx_size, lo, hi, flags_out + lo) : HSV_OK;
  });
}

}  // namespace
}  // namespace hsvh

using namespace hsvh;

extern "C" {

int hsv_verify_transactions(const uint8_t *txs, const uint64_t *offsets, size_t n, uint8_t *flags_out) {
  CallScope call;
  if (n && !offsets) return fail(HSV_ERR_INVALID_ARG, "null offsets");
  return run_tx_host(txs, offsets, 0, n, flags_out);
}

int hsv_verify_transactions_fixed(const uint8_t *txs, size_t tx_size, size_t n, uint8_t *flags_out) {
  CallScope call;
  return run_tx_host(txs, nullptr, tx_size, n, flags_out);
}

int hsv_verify_transactions_device(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                                   uint8_t *d_flags, uint32_t *d_strict_bits, uint32_t *d_fault, void *stream) {
  if (n == 0) return HSV_OK;
  if (!d_txs) return fail(HSV_ERR_INVALID_ARG, "null d_txs");
  int rc = tx_device_args_ok(d_offsets, tx_size, d_flags, d_strict_bits);
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  rc = call.begin(d_txs, stream, d_fault, DeviceCall::kVariant);
  if (rc != HSV_OK) return rc;
  hipStream_t s = call.stream;
  const size_t per = std::min(n, kChunk);
  void *rec = nullptr;
  hipError_t e = hsv_ws_malloc(reinterpret_cast<void **>(&rec), per * 128, s);
  if (e != hipSuccess) return hip_fail("workspace allocation (transaction records)", e);
  for (size_t base = 0; base < n && rc == HSV_OK; base += per) {
    const size_t m = std::min(per, n - base);
    rc = tx_enqueue(call.v, call.comb, d_offsets ? d_txs : d_txs + base * tx_size, d_offsets ? d_offsets + base : nullptr,
                    tx_size, m, static_cast<uint8_t *>(rec), d_flags ? d_flags + base : nullptr,
                    d_strict_bits ? d_strict_bits + base / 32 : nullptr, call.fault, s);
  }
  e = hipFreeAsync(rec, s);
  if (rc != HSV_OK) return rc;
  return e == hipSuccess ? HSV_OK : hip_fail("hipFreeAsync", e);
}

}  // extern "C"
