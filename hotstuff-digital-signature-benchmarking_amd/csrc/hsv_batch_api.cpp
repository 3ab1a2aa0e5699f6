// C ABI of the serialized mempool batches (include/hsv.h,
// hsv_batch*_bincode*): Core::make_vote's payload check
// (consensus/src/core.rs:113-142) from the stored bincode bytes of
// MempoolMessage::Batch.  The transactions are verified where they lie: the
// transaction kernels address them through a span table (hsv_mempool.hip,
// SPANS) that the host parser (hsv_wire_parse.cpp, parse_batch) or the device
// parse (hsv_batchwire.hip) writes.  Records -> the generic verification
// launch -> the short-transaction mask at every size (the route transactions
// take at <= 2^13 items; the fused launch is left alone), or the committee's
// route, comb and generic passes.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "hsv_committee_host.h"
#include "hsv_wire_parse.h"

using namespace hsvh;

namespace {

int parse_error(const std::string &what) { return fail(HSV_ERR_PARSE, "bincode: " + what); }

// n transactions in HBM through the generic kernels, rounds of kChunk in order
// on `s`: d_rec holds min(n, kChunk) records
int generic_spans_enqueue(int v, const uint32_t *comb_b, const uint8_t *d_bufs, const uint64_t *d_spans, size_t n,
                          uint8_t *d_rec, uint8_t *d_flags, uint32_t *d_fault, hipStream_t s) {
  for (size_t base = 0; base < n; base += kChunk) {
    const uint32_t m = (uint32_t)std::min(kChunk, n - base);
    const uint64_t *sp = d_spans + 2 * base;
    hipError_t e = hsv_launch_tx_records_spans(d_bufs, sp, m, d_rec, s);
    if (e != hipSuccess) return hip_fail("transaction record kernel launch", e);
    e = hsv_launch_verify(v, d_rec, 128, d_rec + 32, 128, d_rec + 96, 128, m, d_flags + base, nullptr, comb_b, d_fault, s);
    if (e != hipSuccess) return hip_fail("transaction verify launch", e);
    e = hsv_launch_tx_mask_spans(sp, m, d_flags + base, nullptr, s);
    if (e != hipSuccess) return hip_fail("transaction mask kernel launch", e);
  }
  return HSV_OK;
}

struct HostBatch {
  bool ok = false;
  size_t n = 0, first = 0;
};

// verdict of a well-formed batch from its transactions' flags
hsv_batch_result batch_verdict_of(const HostBatch &b, const uint8_t *flags) {
  hsv_batch_result r{HSV_BATCH_OK, 0, b.n, b.first};
  for (size_t i = 0; i < b.n; ++i)
    if (!(flags[b.first + i] & HSV_STRICT_OK)) {
      r.status = HSV_BATCH_TX;
      r.index = (uint32_t)i;
      break;
    }
  return r;
}

// The host form after the argument checks and the parse: well-formed batches
// staged in rounds of whole batches, at most g_stage_bytes bytes and (but for
// a single larger batch) kChunk transactions each, through a slot's pinned
// staging as staged_tx_host does: per round one H2D copy (batch bytes | span
// pairs), the memset of flags and self-check words, the launches, one D2H, the
// drain.  spans: absolute in bufs.
struct Round {
  size_t b0, b1, bytes, m;
};

int run_batches_host(hsv_committee *cm, const uint8_t *bufs, const uint64_t *offsets, size_t nb,
                     const std::vector<HostBatch> &hb, const std::vector<uint64_t> &spans, uint8_t *flags) {
  DevCtx &c = ctx(cm ? committee_device_of(cm) : home_device());
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  const int v = variant();
  const uint32_t *comb_b = nullptr;
  int rc = cm ? ensure_btable(c) : comb_table_for(c, v, &comb_b);
  if (rc == HSV_OK && cm) rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  const size_t limit = g_stage_bytes.load();
  std::vector<Round> rounds;
  size_t max_bytes = 0, max_items = 0;
  for (size_t b0 = 0; b0 < nb;) {
    Round r{b0, b0, 0, 0};
    for (; r.b1 < nb; ++r.b1) {
      const HostBatch &h = hb[r.b1];
      if (!h.ok || h.n == 0) continue;  // no device work
      const size_t len = (size_t)(offsets[r.b1 + 1] - offsets[r.b1]);
      if (r.m && (r.bytes + len > limit || r.m + h.n > kChunk)) break;
      r.bytes += len;
      r.m += h.n;
    }
    if (r.m == 0) break;  // nothing left to verify
    rounds.push_back(r);
    max_bytes = std::max(max_bytes, r.bytes);
    max_items = std::max(max_items, r.m);
    b0 = r.b1;
  }
  // device: batch bytes | span pairs | records | flags | self-check words;
  // host: batch bytes | span pairs | flags | self-check words
  const size_t span_off = round_up(max_bytes, kAlign), rec_off = span_off + round_up(max_items * 16, kAlign);
  const size_t flag_off = rec_off + round_up(cm ? 0 : std::min(max_items, kChunk) * 128, kAlign);
  const size_t fault_off = flag_off + round_up(max_items, kAlign), d_total = fault_off + kAlign;
  const size_t h_flag_off = rec_off, h_fault_off = h_flag_off + round_up(max_items, kAlign);
  SlotLease lease(c);
  Slot &s = lease.slot();
  rc = slot_prepare(s, d_total, h_fault_off + kAlign);
  if (rc != HSV_OK) return rc;
  for (const Round &r : rounds) {
    uint8_t *h = s.h_buf;
    uint64_t *rel = reinterpret_cast<uint64_t *>(h + span_off);
    // batches packed in order; adjacent ones travel in one copy
    size_t first = 0, doff = 0, k = 0, run_src = 0, run_dst = 0, run_len = 0;
    bool have_first = false;
    for (size_t b = r.b0; b < r.b1; ++b) {
      if (!hb[b].ok || hb[b].n == 0) continue;
      if (!have_first) first = hb[b].first, have_first = true;
      const size_t src = (size_t)offsets[b], len = (size_t)(offsets[b + 1] - offsets[b]);
      for (size_t i = 0; i < 2 * hb[b].n; ++i) rel[k++] = spans[2 * hb[b].first + i] - src + doff;
      if (run_len && run_src + run_len == src) {
        run_len += len;
      } else {
        if (run_len) stage_copy(h + run_dst, bufs + run_src, run_len);
        run_src = src, run_dst = doff, run_len = len;
      }
      doff += len;
    }
    if (run_len) stage_copy(h + run_dst, bufs + run_src, run_len);
    hipError_t e = hipMemcpyAsync(s.d_buf, h, span_off + r.m * 16, hipMemcpyHostToDevice, s.stream);
    // unwritten flags read as rejections; self-check words start at zero
    if (e == hipSuccess) e = hipMemsetAsync(s.d_buf + flag_off, 0, fault_off + kFaultBytes - flag_off, s.stream);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s.stream);
      return hip_fail("hipMemcpyAsync H2D", e);
    }
    const uint64_t *d_spans = reinterpret_cast<const uint64_t *>(s.d_buf + span_off);
    uint32_t *d_fault = reinterpret_cast<uint32_t *>(s.d_buf + fault_off);
    rc = cm ? committee_tx_spans_enqueue(cm, c, c.d_btable, c.d_btable16, s.d_buf, d_spans, r.m, s.d_buf + flag_off,
                                         d_fault, s.stream)
            : generic_spans_enqueue(v, comb_b, s.d_buf, d_spans, r.m, s.d_buf + rec_off, s.d_buf + flag_off, d_fault,
                                    s.stream);
    if (rc == HSV_OK) {
      e = hipMemcpyAsync(h + h_flag_off, s.d_buf + flag_off, fault_off + kFaultBytes - flag_off, hipMemcpyDeviceToHost,
                         s.stream);
      if (e != hipSuccess) rc = hip_fail("hipMemcpyAsync D2H", e);
    }
    e = hipStreamSynchronize(s.stream);  // nothing of this call stays in flight
    if (rc != HSV_OK) return rc;
    if (e != hipSuccess) return hip_fail("hipStreamSynchronize", e);
    rc = check_faults(h + h_fault_off, "hsv_batches_verify_bincode");
    if (rc != HSV_OK) return rc;
    // well-formed batches are numbered in order, so the round's flags are contiguous
    std::memcpy(flags + first, h + h_flag_off, r.m);
  }
  return HSV_OK;
}

int batches_host(hsv_committee *cm, const uint8_t *bufs, const uint64_t *offsets, size_t nb,
                 hsv_batch_result *results, uint8_t *flags_out, size_t flags_cap, bool parse_is_error) {
  if (nb == 0) return 0;
  if (!offsets) return fail(HSV_ERR_INVALID_ARG, "null offsets");
  for (size_t i = 0; i < nb; ++i)
    if (offsets[i + 1] < offsets[i])
      return fail(HSV_ERR_INVALID_ARG, "batch " + std::to_string(i) + ": offsets decrease");
  if (!bufs && offsets[nb] != offsets[0]) return fail(HSV_ERR_INVALID_ARG, "null buffer");
  std::vector<HostBatch> hb(nb);
  std::vector<uint64_t> spans;
  std::string err;
  size_t total = 0;
  const size_t limit = g_stage_bytes.load();
  for (size_t b = 0; b < nb; ++b) {
    const size_t len = (size_t)(offsets[b + 1] - offsets[b]);
    hb[b].first = total;
    hb[b].ok = hsvw::parse_batch(len ? bufs + offsets[b] : nullptr, len, offsets[b], &spans, hb[b].n, err);
    if (!hb[b].ok && parse_is_error) return parse_error(err);
    if (hb[b].ok && hb[b].n && len > limit)
      return fail(HSV_ERR_INVALID_ARG, "batch " + std::to_string(b) + " is larger than a staging round");
    total += hb[b].n;
  }
  if (flags_out && flags_cap < total) return fail(HSV_ERR_INVALID_ARG, "flags_cap is below the transaction count");
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  std::vector<uint8_t> own;
  uint8_t *flags = flags_out;
  if (!flags) {
    own.assign(total, 0);
    flags = own.data();
  }
  if (total) {
    rc = run_batches_host(cm, bufs, offsets, nb, hb, spans, flags);
    if (rc != HSV_OK) return rc;
  }
  int good = 0;
  for (size_t b = 0; b < nb; ++b) {
    const hsv_batch_result r =
        hb[b].ok ? batch_verdict_of(hb[b], flags) : hsv_batch_result{HSV_BATCH_PARSE, 0, 0, hb[b].first};
    if (results) results[b] = r;
    good += r.status == HSV_BATCH_OK;
  }
  return good;
}

}  // namespace

// Measurement (hsv_test_batch_stages, tools/batch_wire_probe.py): the stages of
// the generic device form one after the other on the current device's null
// stream, each between two events: ms_out = {parse (count, index, spans),
// record kernel, verification launch and mask, verdict kernel}.  Synchronises.
namespace hsvh {
int batch_stage_times(const uint8_t *d_bufs, const uint64_t *d_offsets, size_t n_batches, size_t tx_cap,
                      hsv_batch_result *d_results, float ms_out[4]) {
  if (!d_bufs || !d_offsets || !d_results || !ms_out || !n_batches || !tx_cap || n_batches > 0xffffffffu ||
      tx_cap > kChunk)
    return fail(HSV_ERR_INVALID_ARG, "bad argument");
  DeviceCall call;
  int rc = call.begin(d_bufs, nullptr, nullptr, DeviceCall::kVariant);
  if (rc != HSV_OK) return rc;
  hipStream_t s = call.stream;
  const uint32_t nb = (uint32_t)n_batches;
  const size_t off_count = round_up((size_t)nb * 4, kAlign), off_first = off_count + round_up((size_t)nb * 8, kAlign);
  const size_t off_spans = off_first + round_up(((size_t)nb + 1) * 8, kAlign);
  const size_t off_flags = off_spans + round_up(tx_cap * 16, kAlign), off_rec = off_flags + round_up(tx_cap, kAlign);
  uint8_t *ws = nullptr;
  hipError_t e = hsv_ws_malloc(reinterpret_cast<void **>(&ws), off_rec + tx_cap * 128 + kAlign, s);
  if (e != hipSuccess) return hip_fail("workspace allocation (batch parse)", e);
  uint32_t *status = reinterpret_cast<uint32_t *>(ws);
  uint64_t *count = reinterpret_cast<uint64_t *>(ws + off_count), *first = reinterpret_cast<uint64_t *>(ws + off_first);
  uint64_t *spans = reinterpret_cast<uint64_t *>(ws + off_spans);
  uint8_t *flags = ws + off_flags, *rec = ws + off_rec;
  hipEvent_t ev[5] = {};
  for (hipEvent_t &x : ev)
    if (e == hipSuccess) e = hipEventCreate(&x);
  const uint32_t m = (uint32_t)tx_cap;
  if (e == hipSuccess) e = hipMemsetAsync(spans, 0, tx_cap * 16, s);
  if (e == hipSuccess) e = hipEventRecord(ev[0], s);
  if (e == hipSuccess) e = hsv_launch_batch_scan(d_bufs, d_offsets, nb, tx_cap, status, count, first, spans, s);
  if (e == hipSuccess) e = hipEventRecord(ev[1], s);
  if (e == hipSuccess) e = hsv_launch_tx_records_spans(d_bufs, spans, m, rec, s);
  if (e == hipSuccess) e = hipEventRecord(ev[2], s);
  if (e == hipSuccess)
    e = hsv_launch_verify(call.v, rec, 128, rec + 32, 128, rec + 96, 128, m, flags, nullptr, call.comb, call.fault, s);
  if (e == hipSuccess) e = hsv_launch_tx_mask_spans(spans, m, flags, nullptr, s);
  if (e == hipSuccess) e = hipEventRecord(ev[3], s);
  if (e == hipSuccess) e = hsv_launch_batch_reduce(status, count, first, flags, nb, d_results, s);
  if (e == hipSuccess) e = hipEventRecord(ev[4], s);
  if (e == hipSuccess) e = hipEventSynchronize(ev[4]);
  for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  const hipError_t ef = hipFreeAsync(ws, s);
  if (e != hipSuccess) return hip_fail("batch stage timing", e);
  return ef == hipSuccess ? HSV_OK : hip_fail("hipFreeAsync", ef);
}
}  // namespace hsvh

extern "C" {

int hsv_batch_parse_bincode(const uint8_t *buf, size_t len, size_t *n_tx_out, uint64_t *spans_out, size_t spans_cap) {
  if (!buf && len) return fail(HSV_ERR_INVALID_ARG, "null buffer");
  std::vector<uint64_t> spans;
  std::string err;
  size_t n = 0;
  if (!hsvw::parse_batch(buf, len, 0, spans_out ? &spans : nullptr, n, err)) return parse_error(err);
  if (spans_out) {
    if (spans_cap < 2 * n) return fail(HSV_ERR_INVALID_ARG, "spans_cap is below twice the transaction count");
    std::copy(spans.begin(), spans.end(), spans_out);
  }
  if (n_tx_out) *n_tx_out = n;
  return 1;
}

int hsv_batches_verify_bincode(hsv_committee *c, const uint8_t *bufs, const uint64_t *offsets, size_t n_batches,
                               hsv_batch_result *results, uint8_t *flags_out, size_t flags_cap) {
  CallScope call;  // the host timeline includes the parse
  return batches_host(c, bufs, offsets, n_batches, results, flags_out, flags_cap, false);
}

int hsv_batch_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len, hsv_batch_result *res) {
  CallScope call;
  if (!buf && len) return fail(HSV_ERR_INVALID_ARG, "null buffer");
  const uint64_t offsets[2] = {0, len};
  hsv_batch_result r{};
  const int rc = batches_host(c, buf, offsets, 1, &r, nullptr, 0, true);
  if (rc < 0) return rc;
  if (res) *res = r;
  return rc;
}

int hsv_batches_verify_bincode_device(const hsv_committee *c, const uint8_t *d_bufs, const uint64_t *d_offsets,
                                      size_t n_batches, size_t tx_cap, hsv_batch_result *d_results, uint8_t *d_flags,
                                      uint32_t *d_fault, void *stream) {
  if (n_batches == 0 && (tx_cap == 0 || !d_flags)) return HSV_OK;
  if (!d_bufs || (n_batches && (!d_offsets || !d_results))) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (n_batches > 0xffffffffu || tx_cap > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if ((reinterpret_cast<uintptr_t>(d_offsets) | reinterpret_cast<uintptr_t>(d_results)) & 7u)
    return fail(HSV_ERR_ALIGN, "d_offsets and d_results must be 8-byte aligned");
  int rc = HSV_OK;
  if (c) rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  rc = c ? call.begin(d_bufs, stream, d_fault, DeviceCall::kBoth, "committee", committee_device_of(c))
         : call.begin(d_bufs, stream, d_fault, DeviceCall::kVariant);
  if (rc != HSV_OK) return rc;
  hipStream_t s = call.stream;
  if (n_batches == 0) {
    const hipError_t e = hipMemsetAsync(d_flags, 0, tx_cap, s);
    return e == hipSuccess ? HSV_OK : hip_fail("hipMemsetAsync", e);
  }
  // status | count | first | spans | flags (when the caller keeps none) | records
  const uint32_t nb = (uint32_t)n_batches;
  const size_t off_status = 0, off_count = off_status + round_up((size_t)nb * 4, kAlign);
  const size_t off_first = off_count + round_up((size_t)nb * 8, kAlign);
  const size_t off_spans = off_first + round_up(((size_t)nb + 1) * 8, kAlign);
  const size_t off_flags = off_spans + round_up(tx_cap * 16, kAlign);
  const size_t off_rec = off_flags + (d_flags ? 0 : round_up(tx_cap, kAlign));
  const size_t bytes = off_rec + (c ? 0 : std::min(tx_cap, kChunk) * 128) + kAlign;
  uint8_t *ws = nullptr;
  hipError_t e = hsv_ws_malloc(reinterpret_cast<void **>(&ws), bytes, s);
  if (e != hipSuccess) return hip_fail("workspace allocation (batch parse)", e);
  uint32_t *status = reinterpret_cast<uint32_t *>(ws + off_status);
  uint64_t *count = reinterpret_cast<uint64_t *>(ws + off_count), *first = reinterpret_cast<uint64_t *>(ws + off_first);
  uint64_t *spans = reinterpret_cast<uint64_t *>(ws + off_spans);
  uint8_t *flags = d_flags ? d_flags : ws + off_flags;
  // an entry no batch writes reads as an empty span: flags 0
  if (tx_cap) e = hipMemsetAsync(spans, 0, tx_cap * 16, s);
  if (e == hipSuccess) e = hsv_launch_batch_scan(d_bufs, d_offsets, nb, tx_cap, status, count, first, spans, s);
  if (e != hipSuccess) rc = hip_fail("batch parse launch", e);
  if (rc == HSV_OK && tx_cap)
    rc = c ? committee_tx_spans_enqueue(c, *call.c, call.comb, call.comb16, d_bufs, spans, tx_cap, flags, call.fault, s)
           : generic_spans_enqueue(call.v, call.comb, d_bufs, spans, tx_cap, ws + off_rec, flags, call.fault, s);
  if (rc == HSV_OK) {
    e = hsv_launch_batch_reduce(status, count, first, flags, nb, d_results, s);
    if (e != hipSuccess) rc = hip_fail("batch verdict launch", e);
  }
  e = hipFreeAsync(ws, s);
  if (rc != HSV_OK) return rc;
  return e == hipSuccess ? HSV_OK : hip_fail("hipFreeAsync", e);
}

}  // extern "C"
