// Sealing verified transactions into MempoolMessage::Batch messages behind the
// C ABI (hsv_seal_bound, hsv_seal_transactions*): BatchMaker::run / seal
// (mempool/src/batch_maker.rs:78-131) with the check enabled, on the device
// (hsv_seal.hip).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "hsv.h"
#include "hsv_committee_host.h"
#include "hsv_host.h"
#include "hsv_internal.h"
#include "hsv_seal.hpp"

namespace hsvh {
namespace {

// the checks of the device form, all before any device work
int device_args_ok(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n, uint64_t batch_size,
                   const uint8_t *d_out, size_t out_cap, const uint64_t *d_batch_offsets,
                   const hsv_seal_summary *d_summary) {
  if (batch_size == 0) return fail(HSV_ERR_INVALID_ARG, "batch_size is 0");
  if (n > 0xffffffffull) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if (!d_batch_offsets || !d_summary) return fail(HSV_ERR_INVALID_ARG, "null output");
  if (out_cap && !d_out) return fail(HSV_ERR_INVALID_ARG, "null d_out");
  if (n && !d_txs) return fail(HSV_ERR_INVALID_ARG, "null d_txs");
  if (n && !d_offsets && tx_size == 0) return fail(HSV_ERR_INVALID_ARG, "tx_size is 0");
  if ((reinterpret_cast<uintptr_t>(d_offsets) | reinterpret_cast<uintptr_t>(d_batch_offsets) |
       reinterpret_cast<uintptr_t>(d_summary)) & 7u)
    return fail(HSV_ERR_ALIGN, "d_offsets, d_batch_offsets and d_summary must be 8-byte aligned");
  if (n && !d_offsets) {
    if (tx_size > ~size_t(0) / n) return fail(HSV_ERR_INVALID_ARG, "n * tx_size does not fit");
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_txs), b = reinterpret_cast<uintptr_t>(d_out);
    if (out_cap && a < b + out_cap && b < a + n * tx_size)
      return fail(HSV_ERR_INVALID_ARG, "d_out overlaps the transactions");
  }
  return HSV_OK;
}

int seal_enqueue(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n, const uint8_t *d_flags,
                 uint64_t batch_size, int flush, uint8_t *d_out, size_t out_cap, uint64_t *d_batch_offsets,
                 size_t batches_cap, uint8_t *d_digests, hsv_seal_summary *d_summary, hipEvent_t *marks,
                 hipStream_t s) {
  const hipError_t e = hsv_launch_seal(d_txs, d_offsets, tx_size, (uint32_t)n, d_flags, batch_size, flush, d_out,
                                       out_cap, d_batch_offsets, batches_cap, d_digests, d_summary, marks, s);
  return e == hipSuccess ? HSV_OK : hip_fail("seal launch", e);
}

}  // namespace

int seal_stage_times(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n, const uint8_t *d_flags,
                     uint64_t batch_size, int flush, uint8_t *d_out, size_t out_cap, uint64_t *d_batch_offsets,
                     size_t batches_cap, uint8_t *d_digests, hsv_seal_summary *d_summary, float ms_out[4]) {
  int rc = device_args_ok(d_txs, d_offsets, tx_size, n, batch_size, d_out, out_cap, d_batch_offsets, d_summary);
  if (rc != HSV_OK) return rc;
  if (!ms_out) return fail(HSV_ERR_INVALID_ARG, "null ms_out");
  DeviceCall call;
  rc = call.begin(d_txs ? static_cast<const void *>(d_txs) : d_summary, nullptr, nullptr, DeviceCall::kNone);
  if (rc != HSV_OK) return rc;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  if (e == hipSuccess) {
    rc = seal_enqueue(d_txs, d_offsets, tx_size, n, d_flags, batch_size, flush, d_out, out_cap, d_batch_offsets,
                      batches_cap, d_digests, d_summary, ev, call.stream);
    e = hipStreamSynchronize(call.stream);
    for (int k = 0; k < 4 && e == hipSuccess && rc == HSV_OK; ++k) e = hipEventElapsedTime(&ms_out[k], ev[k], ev[k + 1]);
  }
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  if (rc != HSV_OK) return rc;
  return e == hipSuccess ? HSV_OK : hip_fail("hsv_test_seal_stages", e);
}

}  // namespace hsvh

using namespace hsvh;

extern "C" {

int hsv_seal_bound(uint64_t total_tx_bytes, uint64_t n, uint64_t batch_size, uint64_t *bytes_out,
                   uint64_t *batches_out) {
  if (batch_size == 0) return fail(HSV_ERR_INVALID_ARG, "batch_size is 0");
  uint64_t bytes = 0, batches = 0;
  if (!hsv::seal_bound(total_tx_bytes, n, batch_size, &bytes, &batches))
    return fail(HSV_ERR_INVALID_ARG, "the bound does not fit 64 bits");
  if (bytes_out) *bytes_out = bytes;
  if (batches_out) *batches_out = batches;
  return HSV_OK;
}

int hsv_seal_transactions_device(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                                 const uint8_t *d_flags, uint64_t batch_size, int flush, uint8_t *d_out,
                                 size_t out_cap, uint64_t *d_batch_offsets, size_t batches_cap, uint8_t *d_digests,
                                 hsv_seal_summary *d_summary, void *stream) {
  int rc = device_args_ok(d_txs, d_offsets, tx_size, n, batch_size, d_out, out_cap, d_batch_offsets, d_summary);
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  // n == 0: the inputs may be NULL
  rc = call.begin(d_txs ? static_cast<const void *>(d_txs) : d_summary, stream, nullptr, DeviceCall::kNone);
  if (rc != HSV_OK) return rc;
  return seal_enqueue(d_txs, d_offsets, tx_size, n, d_flags, batch_size, flush, d_out, out_cap, d_batch_offsets,
                      batches_cap, d_digests, d_summary, nullptr, call.stream);
}

int hsv_seal_transactions(hsv_committee *cm, const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t n,
                          uint64_t batch_size, int flush, uint8_t *out, size_t out_cap, uint64_t *batch_offsets_out,
                          size_t batches_cap, uint8_t *digests_out, uint8_t *flags_out, hsv_seal_summary *summary) {
  CallScope scope;
  if (batch_size == 0) return fail(HSV_ERR_INVALID_ARG, "batch_size is 0");
  if (!batch_offsets_out || !summary || (out_cap && !out)) return fail(HSV_ERR_INVALID_ARG, "null output");
  if (n && !txs) return fail(HSV_ERR_INVALID_ARG, "null txs");
  if (n && !offsets && tx_size == 0) return fail(HSV_ERR_INVALID_ARG, "tx_size is 0");
  if (n > kChunk) return fail(HSV_ERR_INVALID_ARG, "more than 2^22 transactions");
  const BatchSpan span{offsets, tx_size, tx_size};
  if (offsets && first_bad_item(offsets, n, 0) != n) return fail(HSV_ERR_INVALID_ARG, "offsets decrease");
  if (!offsets && n && tx_size > kStageBytes / n) return fail(HSV_ERR_INVALID_ARG, "more than 2^29 bytes");
  const size_t total = n ? span.span_bytes(0, n) : 0, first = n ? span.first_byte(0) : 0;
  if (total > kStageBytes) return fail(HSV_ERR_INVALID_ARG, "more than 2^29 bytes");
  uint64_t need_bytes = 0, need_batches = 0;
  (void)hsv::seal_bound(total, n, batch_size, &need_bytes, &need_batches);  // (fits: the limits above)
  int rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(cm ? committee_device_of(cm) : home_device());
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  SlotLease lease(c);
  Slot &s = lease.slot();
  rc = slot_prepare(s, 0, kAlign);
  if (rc != HSV_OK) return rc;
  StagedBlock blk(s.stream);
  const size_t off_flags = blk.add(std::max<size_t>(n, 1)), off_txs = blk.add(total + 16);
  const size_t off_offs = blk.add((n + 1) * 8), off_out = blk.add(need_bytes + 16);
  const size_t off_boff = blk.add((need_batches + 1) * 8), off_dig = blk.add(need_batches * 32 + 16);
  const size_t off_sum = blk.add(sizeof(hsv_seal_summary));
  rc = blk.alloc("allocating the seal buffers", std::max<size_t>(n, 1));  // unwritten flags read as rejections
  if (rc != HSV_OK) return rc;
  std::vector<uint64_t> rel;
  if (n) {
    blk.in(off_txs, txs + first, total);
    if (offsets) {
      rel.resize(n + 1);
      span.rel_offsets(0, n, rel.data());
      blk.in(off_offs, rel.data(), (n + 1) * 8);
    }
  }
  const uint64_t *d_offs = offsets ? reinterpret_cast<const uint64_t *>(blk.at(off_offs)) : nullptr;
  if (blk.ok() && n) {
    rc = cm ? hsv_committee_verify_transactions_device(cm, blk.at(off_txs), d_offs, tx_size, n, blk.at(off_flags),
                                                       nullptr, blk.fault(), s.stream)
            : hsv_verify_transactions_device(blk.at(off_txs), d_offs, tx_size, n, blk.at(off_flags), nullptr,
                                             blk.fault(), s.stream);
  }
  if (blk.ok() && rc == HSV_OK)
    rc = seal_enqueue(blk.at(off_txs), d_offs, tx_size, n, blk.at(off_flags), batch_size, flush, blk.at(off_out),
                      need_bytes, reinterpret_cast<uint64_t *>(blk.at(off_boff)), need_batches,
                      digests_out ? blk.at(off_dig) : nullptr,
                      reinterpret_cast<hsv_seal_summary *>(blk.at(off_sum)), nullptr, s.stream);
  hsv_seal_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  std::vector<uint64_t> boff;
  if (blk.ok() && rc == HSV_OK) {
    blk.out(&sum, off_sum, sizeof(sum));
    if (flags_out) blk.out(flags_out, off_flags, n);
    if (blk.ok()) blk.step(hipStreamSynchronize(s.stream));
    if (blk.ok() && sum.status == HSV_SEAL_OK && sum.bytes <= need_bytes && sum.n_batches <= need_batches) {
      if (sum.bytes > out_cap || sum.n_batches > batches_cap) {
        sum.status = HSV_SEAL_OVERFLOW;
      } else {
        boff.resize((size_t)sum.n_batches + 1);
        blk.out(out, off_out, sum.bytes);
        blk.out(boff.data(), off_boff, boff.size() * 8);
        if (digests_out) blk.out(digests_out, off_dig, (size_t)sum.n_batches * 32);
      }
    }
  }
  const int frc = blk.finish("hsv_seal_transactions");  // frees the block and drains the stream
  if (rc != HSV_OK) return rc;
  if (frc != HSV_OK) return frc;
  if (sum.bytes > need_bytes || sum.n_batches > need_batches || (boff.empty() && sum.status == HSV_SEAL_OK))
    return fail(HSV_ERR_HIP, "seal summary out of range");
  if (!boff.empty()) {
    std::copy(boff.begin(), boff.end(), batch_offsets_out);
    std::fill(batch_offsets_out + boff.size(), batch_offsets_out + batches_cap + 1, sum.bytes);
  }
  *summary = sum;
  return HSV_OK;
}

}  // extern "C"
