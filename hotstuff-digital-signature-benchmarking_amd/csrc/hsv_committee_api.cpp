// The explicit committee behind the C ABI:
// hsv_committee_*, tables for a given key list, with its transaction and
// message calls; and committee_run, the launch path of every vote batch by
// member index, which the automatic cache (hsv_auto_committee.cpp) shares and
// which tries the resident latency service (hsv_resident.cpp) first.
//
// The committee kernels (hsv_committee.hip) take a device array of per-key
// table pointers, so the automatic cache can grow by appending table blocks.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "hsv_committee_host.h"
#include "hsv_keyindex.hpp"
#include "hsv_keytab.hpp"

namespace hsvh {

// Votes by member index on the committee's device, through a slot of that
// device: the kernels read the pinned staging buffer directly for batches of
// at most kZeroCopyMax votes (the latency path), otherwise via copies.
int committee_run(const CommitteeDev &cd, const uint32_t *key_idx, const uint8_t *sig, size_t sig_stride,
                  const uint8_t *msg, size_t msg_stride, size_t m, uint8_t *flags_out) {
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(cd.device);
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  rc = ensure_btable(c);  // also after an hsv_shutdown
  // compact tables have no latency form: no resident request, no zero-copy
  // launch; their kernel takes [s]B from the wide comb of B
  const bool compact = cd.digit_bits == 4;
  if (rc == HSV_OK && compact) rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  if (!compact && resident_enabled() && m <= hsv_comb_resident_votes()) {
    rc = resident_run(cd, key_idx, sig, sig_stride, msg, msg_stride, m, flags_out, c.d_btable);
    if (rc != kResidentUnavailable) return rc;
  }
  SlotLease lease(c);
  Slot &s = lease.slot();
  call_mark(HSV_MARK_SLOT);
  for (size_t base = 0; base < m; base += kChunk) {
    const size_t k = std::min(kChunk, m - base);
    const size_t idx_off = 0;
    const size_t sig_off = round_up(k * 4, kAlign);
    const size_t msg_off = sig_off + round_up(k * 64, kAlign);
    const size_t msg_bytes = msg_stride ? k * 32 : 32;
    const size_t flag_off = msg_off + round_up(msg_bytes, kAlign);
    const size_t fault_off = flag_off + round_up(k, kAlign);
    const size_t total = fault_off + kAlign;
    rc = slot_prepare(s, total, total);
    if (rc != HSV_OK) return rc;
    uint8_t *h = s.h_buf;
    // only the indices go out in streaming stores; the signature and message
    // copies are stage_copy, a cached memcpy below 64 KiB (hsv_host.h)
    stage_stream(h + idx_off, key_idx + base, k * 4);
    if (sig_stride == 64) {
      stage_copy(h + sig_off, sig + base * 64, k * 64);
    } else {  // signatures inside packed votes: gathered straight into the staging
      for (size_t i = 0; i < k; ++i) stage_copy(h + sig_off + i * 64, sig + (base + i) * sig_stride, 64);
    }
    stage_copy(h + msg_off, msg + base * msg_stride, msg_bytes);
    stage_fence();
    // The zero-copy latency form (<= kZeroCopyMax votes) reads the inputs from
    // the pinned staging through its device mapping (copying them to HBM first
    // made C1 0.0444 -> 0.0498 ms and C3 0.0592 -> 0.0689 ms,
    // profiles/r03zz7_qc_ab_zc.txt) and writes its flags, self-check words and
    // one completion marker per block into the slot's coherent sync region;
    // the host spins on the markers instead of hipStreamSynchronize: the flags
    // are final once every block has released them, several microseconds
    // before the kernel's completion signal (same box, alternating processes,
    // profiles/r04b_qc_ab_marker.txt: C1 0.0444 -> 0.0394 ms, C3 0.0587 ->
    // 0.0559 ms, one verify_strict 0.0443 -> 0.0395 ms).
    const bool zero_copy = !compact && k <= kZeroCopyMax && s.h_buf_dev != nullptr;
    uint8_t *flags_h, *flags_d, *fault_h, *fault_d;
    uint32_t nmark = 0;
    volatile uint32_t *marks = nullptr;
    uint32_t *marks_d = nullptr;
    if (zero_copy) {
      nmark = hsv_comb_marker_blocks((uint32_t)k);
      const size_t sf = round_up(k, kAlign), sm = sf + kAlign, need = sm + round_up((size_t)nmark * 4 + 4, kAlign);
      rc = slot_sync_region(s, need);
      if (rc != HSV_OK) return rc;
      flags_h = s.h_sync;
      flags_d = s.h_sync_dev;
      fault_h = s.h_sync + sf;
      fault_d = s.h_sync_dev + sf;
      marks = reinterpret_cast<volatile uint32_t *>(s.h_sync + sm);
      marks_d = reinterpret_cast<uint32_t *>(s.h_sync_dev + sm);
      for (uint32_t b = 0; b < nmark; ++b) marks[b] = 0u;
    } else {
      flags_h = h + flag_off;
      flags_d = s.d_buf + flag_off;
      fault_h = h + fault_off;
      fault_d = s.d_buf + fault_off;
    }
    // unwritten flags read as rejections; self-check words start at zero
    std::memset(flags_h, 0, k);
    std::memset(fault_h, 0, kFaultBytes);
    call_mark(HSV_MARK_STAGED);
    const uint8_t *dbuf = zero_copy ? s.h_buf_dev : s.d_buf;
    hipError_t e = hipSuccess;
    if (!zero_copy) e = hipMemcpyAsync(s.d_buf, h, fault_off + kFaultBytes, hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess)
      e = hsv_launch_comb_verify(reinterpret_cast<const uint32_t *>(dbuf + idx_off), dbuf + sig_off, 64,
                                 dbuf + msg_off, msg_stride ? 32 : 0, (uint32_t)k, cd.d_pks, cd.d_kflags, cd.n,
                                 cd.d_tabptr, cd.digit_bits, compact ? c.d_btable16 : c.d_btable, flags_d, reinterpret_cast<uint32_t *>(fault_d), marks_d,
                                 s.stream);
    if (e == hipSuccess && !zero_copy)
      e = hipMemcpyAsync(h + flag_off, s.d_buf + flag_off, fault_off + kFaultBytes - flag_off, hipMemcpyDeviceToHost,
                         s.stream);
    call_mark(HSV_MARK_LAUNCH);
    hipError_t es = hipSuccess;
    bool marked = false;
    if (nmark && e == hipSuccess) {
      // every block past its reads and its stores released: the flags are
      // final, and nothing of this call reads the staging any more (the next
      // call on this slot is ordered behind the kernel on the stream); a
      // kernel that never marks (a device fault) falls back to the stream sync
      const auto t0 = std::chrono::steady_clock::now();
      for (uint32_t b = 0;;) {
        while (b < nmark && marks[b] == 1u) ++b;
        if (b == nmark) {
          marked = true;
          break;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
      }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!marked) es = hipStreamSynchronize(s.stream);  // nothing of this call stays in flight
    call_mark(HSV_MARK_SYNC);
    if (e != hipSuccess) return hip_fail("committee verify launch", e);
    if (es != hipSuccess) return hip_fail("hipStreamSynchronize", es);
    rc = check_faults(fault_h, "committee verify");
    if (rc != HSV_OK) return rc;
    std::memcpy(flags_out + base, flags_h, k);
    call_mark(HSV_MARK_DONE);
  }
  return HSV_OK;
}

// Builds comb tables for `nkeys` encodings already in HBM at d_encs into
// tables[i] (device pointers, host array), flags into d_kflags, on stream st.
// Keys are built in runs of contiguous table memory.  digit_bits: 8, or 4 for
// compact tables (d_tmp sized by the matching hsv_comb*_tmp_bytes(tmp_keys)).
hipError_t build_tables(const uint8_t *d_encs, uint32_t nkeys, uint32_t *const *tables, uint8_t *d_kflags,
                        uint32_t *d_tmp, uint32_t tmp_keys, hipStream_t st, int digit_bits) {
  const bool compact = digit_bits == 4;
  const uint64_t words = (compact ? hsv_comb4_table_bytes() : hsv_comb_table_bytes()) / 4;
  uint32_t i = 0;
  while (i < nkeys) {
    uint32_t j = i + 1;
    while (j < nkeys && j - i < tmp_keys && tables[j] == tables[j - 1] + words) ++j;
    const hipError_t e = (compact ? hsv_launch_comb4_build : hsv_launch_comb_build)(d_encs + (size_t)i * 32, j - i, 1,
                                                                                    tables[i], d_tmp, d_kflags + i, st);
    if (e != hipSuccess) return e;
    i = j;
  }
  return hipSuccess;
}

}  // namespace hsvh

using namespace hsvh;

// ---- explicit committee ------------------------------------------------------------
struct hsv_committee {
  CommitteeDev dev;
  std::vector<uint8_t> h_pks;
  uint8_t *d_pks = nullptr;
  uint8_t *d_kflags = nullptr;
  uint32_t *d_tables = nullptr;
  uint32_t **d_tabptr = nullptr;
  // member index by key bytes on the device (hsv_keytab.hpp), built with the
  // tables; read by hsv_committee_verify_transactions* only
  uint32_t *d_keytab = nullptr;
  uint32_t keymask = 0;
  KeyIndex index;
};

extern "C" {

int hsv_committee_create(const uint8_t *pks, size_t n, hsv_committee **out) {
  return hsv_committee_create_ex(pks, n, HSV_COMMITTEE_DIGITS_FULL, out);
}

int hsv_committee_digit_bits(const hsv_committee *cm) { return cm ? cm->dev.digit_bits : 0; }

uint64_t hsv_committee_table_bytes(const hsv_committee *cm) {
  if (!cm) return 0;
  return (uint64_t)cm->dev.n * (cm->dev.digit_bits == 4 ? hsv_comb4_table_bytes() : hsv_comb_table_bytes());
}

int hsv_committee_create_ex(const uint8_t *pks, size_t n, int digit_bits, hsv_committee **out) {
  if (!out || (!pks && n)) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (n > (1u << 20)) return fail(HSV_ERR_INVALID_ARG, "committee too large");
  if (digit_bits != HSV_COMMITTEE_DIGITS_FULL && digit_bits != HSV_COMMITTEE_DIGITS_COMPACT)
    return fail(HSV_ERR_INVALID_ARG, "digit_bits must be 8 or 4");
  const bool compact = digit_bits == HSV_COMMITTEE_DIGITS_COMPACT;
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  const int dev = home_device();
  DeviceGuard guard(dev);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  rc = ensure_btable(ctx(dev));
  if (rc != HSV_OK) return rc;
  std::unique_ptr<hsv_committee> cm(new hsv_committee());
  cm->dev.device = dev;
  cm->dev.n = (uint32_t)n;
  cm->dev.digit_bits = digit_bits;
  cm->h_pks.assign(pks, pks + 32 * n);
  cm->dev.h_pks = cm->h_pks.data();
  for (size_t i = 0; i < n; ++i) cm->index.emplace(key_of(pks + 32 * i), (uint32_t)i);
  if (n) {
    const uint64_t table_bytes = compact ? hsv_comb4_table_bytes() : hsv_comb_table_bytes();
    const uint64_t words = table_bytes / 4;
    const uint32_t run_keys = std::min<uint32_t>((uint32_t)n, 1024);  // keys per build launch
    uint32_t *d_tmp = nullptr;
    hipStream_t st = nullptr;
    std::vector<uint32_t *> ptrs(n);
    const std::vector<uint32_t> keytab = hsv::keytab_build(pks, n, KeyHash::seed());
    cm->keymask = (uint32_t)keytab.size() - 1u;
    hipError_t e = hipMalloc(&cm->d_pks, n * 32);
    if (e == hipSuccess) e = hipMalloc(&cm->d_keytab, keytab.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&cm->d_kflags, n);
    if (e == hipSuccess) e = hipMalloc(&cm->d_tables, n * table_bytes);
    if (e == hipSuccess) e = hipMalloc(&cm->d_tabptr, n * sizeof(uint32_t *));
    if (e == hipSuccess) e = hipMalloc(&d_tmp, compact ? hsv_comb4_tmp_bytes(run_keys) : hsv_comb_tmp_bytes(run_keys));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (size_t i = 0; e == hipSuccess && i < n; ++i) ptrs[i] = cm->d_tables + i * words;
    if (e == hipSuccess) e = hipMemcpyAsync(cm->d_pks, pks, n * 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(cm->d_tabptr, ptrs.data(), n * sizeof(uint32_t *), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(cm->d_keytab, keytab.data(), keytab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      e = build_tables(cm->d_pks, (uint32_t)n, ptrs.data(), cm->d_kflags, d_tmp, run_keys, st, digit_bits);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (st) (void)hipStreamDestroy(st);
    if (d_tmp) {
      ResidentPause pause;  // hipFree waits for every grid on the device
      (void)hipFree(d_tmp);
    }
    if (e != hipSuccess) {
      hsv_committee_destroy(cm.release());
      return hip_fail("building committee tables", e);
    }
    cm->dev.d_pks = cm->d_pks;
    cm->dev.d_kflags = cm->d_kflags;
    cm->dev.d_tabptr = cm->d_tabptr;
  }
  *out = cm.release();
  return HSV_OK;
}

void hsv_committee_destroy(hsv_committee *cm) {
  if (!cm) return;
  ResidentPause pause;  // hipFree waits for every grid on the device
  DeviceGuard guard(cm->dev.device);
  if (cm->d_pks) (void)hipFree(cm->d_pks);
  if (cm->d_kflags) (void)hipFree(cm->d_kflags);
  if (cm->d_tables) (void)hipFree(cm->d_tables);
  if (cm->d_tabptr) (void)hipFree(cm->d_tabptr);
  if (cm->d_keytab) (void)hipFree(cm->d_keytab);
  delete cm;
}

size_t hsv_committee_size(const hsv_committee *cm) { return cm ? cm->dev.n : 0; }

int64_t hsv_committee_index(const hsv_committee *cm, const uint8_t pk[32]) {
  if (!cm || !pk) return -1;
  return cm->index.find(pk);
}

int hsv_committee_verify_device(const hsv_committee *cm, const uint32_t *d_key_idx, const uint8_t *d_sig,
                                size_t sig_stride, const uint8_t *d_msg, size_t msg_stride, size_t m, uint8_t *d_flags,
                                uint32_t *d_fault, void *stream) {
  if (m == 0) return HSV_OK;
  if (!cm || !d_key_idx || !d_sig || !d_msg || !d_flags) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (((reinterpret_cast<uintptr_t>(d_sig) | reinterpret_cast<uintptr_t>(d_msg) | sig_stride | msg_stride) & 15u) != 0)
    return fail(HSV_ERR_ALIGN, "device pointers and strides must be multiples of 16");
  if (sig_stride < 64 || (msg_stride != 0 && msg_stride < 32)) return fail(HSV_ERR_INVALID_ARG, "record strides overlap");
  if (m > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  DeviceCall call;
  const bool compact = cm->dev.digit_bits == 4;  // its kernel reads the wide comb of B
  const int rc = call.begin(d_sig, stream, d_fault, compact ? DeviceCall::kWide : DeviceCall::kNarrow, "committee",
                            cm->dev.device);
  if (rc != HSV_OK) return rc;
  const hipError_t e = hsv_launch_comb_verify(d_key_idx, d_sig, sig_stride, d_msg, msg_stride, (uint32_t)m, cm->dev.d_pks,
                                              cm->dev.d_kflags, cm->dev.n, cm->dev.d_tabptr, cm->dev.digit_bits, call.comb, d_flags,
                                              call.fault, nullptr, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("committee verify launch", e);
}

int hsv_committee_verify(hsv_committee *cm, const uint32_t *key_idx, const uint8_t *sig, const uint8_t *msg,
                         size_t msg_stride, size_t m, uint8_t *flags_out) {
  CallScope call;
  if (m == 0) return HSV_OK;
  if (!cm || !key_idx || !sig || !msg || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (msg_stride != 0 && msg_stride != 32) return fail(HSV_ERR_INVALID_ARG, "msg_stride must be 0 or 32");
  return committee_run(cm->dev, key_idx, sig, 64, msg, msg_stride, m, flags_out);
}

int hsv_committee_verify_batch_packed(hsv_committee *cm, const uint8_t digest[32], const uint8_t *votes, size_t m) {
  CallScope call;
  if (m == 0) return 1;
  if (!cm || !digest || !votes) return fail(HSV_ERR_INVALID_ARG, "null argument");
  thread_local std::vector<uint32_t> idx;  // per-call scratch kept by the thread
  thread_local std::vector<uint8_t> flags;
  idx.resize(m);
  flags.resize(m);
  for (size_t i = 0; i < m; ++i) {
    const int64_t k = cm->index.find(votes + 96 * i);
    if (k < 0) {  // a non-member key: the generic kernels
      const int rc = run_host(votes, 96, votes + 32, 96, digest, 0, m, flags.data());
      return rc != HSV_OK ? rc : batch_verdict(flags.data(), m);
    }
    idx[i] = (uint32_t)k;
  }
  const int rc = committee_run(cm->dev, idx.data(), votes + 32, 96, digest, 0, m, flags.data());
  return rc != HSV_OK ? rc : batch_verdict(flags.data(), m);
}

}  // extern "C"

// ---- mempool transactions of known signers -------------------------------------------
// hsv_committee_verify_transactions*: the transaction layout and scheme of
// hsv_verify_transactions* (hsv_tx.cpp), with the signer looked up on the
// device (hsv_keytab.hpp): a member's transaction takes its comb table, any
// other the generic point pass -- three launches per round of at most kChunk
// transactions (hsv_launch_committee_tx, hsv_mempool.hip), no host round trip.
namespace hsvh {
namespace {

// the list-length slot of the calling thread's last call (committee_tx_counts)
struct TxCountRef {
  int device = -1;
  unsigned slot = 0;
};
thread_local TxCountRef t_tx_counts;
thread_local TxCountRef t_msg_counts;  // the same of the message calls (committee_msgs_counts)

// Takes the next slot (of those at byte `off` of the device's self-check
// block, dealt by `rr`) of device c (current) for this call and zeroes it on
// `stream`; out: the slot's three 64-bit words.
int counts_begin(DevCtx &c, hipStream_t stream, size_t off, std::atomic<unsigned> &rr, TxCountRef &ref,
                 uint64_t **out) {
  uint32_t *words = nullptr;
  const int rc = device_fault_words(c, &words);
  if (rc != HSV_OK) return rc;
  const unsigned slot = rr.fetch_add(1) % kTxCountSlots;
  uint8_t *p = reinterpret_cast<uint8_t *>(words) + off + slot * kTxCountBytes;
  const hipError_t e = hipMemsetAsync(p, 0, kTxCountBytes, stream);
  if (e != hipSuccess) return hip_fail("zeroing the call's list lengths", e);
  ref.device = c.device;
  ref.slot = slot;
  *out = reinterpret_cast<uint64_t *>(p);
  return HSV_OK;
}
int tx_counts_begin(DevCtx &c, hipStream_t stream, uint64_t **out) {
  return counts_begin(c, stream, kTxCountOff, c.tx_count_rr, t_tx_counts, out);
}

// the three words of the slot `ref` names
int counts_read(const TxCountRef &ref, size_t off, const char *none, uint64_t out[3]) {
  if (!out) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (ref.device < 0) return fail(HSV_ERR_INVALID_ARG, none);
  DevCtx &c = ctx(ref.device);
  DeviceGuard guard(c.device);
  uint32_t *words = nullptr;
  const int rc = device_fault_words(c, &words);
  if (rc != HSV_OK) return rc;
  const hipError_t e = hipMemcpy(out, reinterpret_cast<uint8_t *>(words) + off + ref.slot * kTxCountBytes,
                                 3 * sizeof(uint64_t), hipMemcpyDeviceToHost);
  return e == hipSuccess ? HSV_OK : hip_fail("hipMemcpy", e);
}

// n transactions already in HBM, in rounds of kChunk in order on `stream`
// (d_offsets relative to d_txs, or NULL = fixed size)
int committee_tx_enqueue(const hsv_committee &cm, const uint32_t *btable, const uint32_t *comb16, const uint8_t *d_txs,
                         const uint64_t *d_offsets, size_t tx_size, size_t n, uint8_t *d_flags, uint32_t *d_bits,
                         uint32_t *d_fault, uint64_t *d_totals, hipStream_t s) {
  for (size_t base = 0; base < n; base += kChunk) {
    const size_t m = std::min(kChunk, n - base);
    const hipError_t e = hsv_launch_committee_tx(
        d_offsets ? d_txs : d_txs + base * tx_size, d_offsets ? d_offsets + base : nullptr, tx_size, (uint32_t)m,
        cm.d_keytab, cm.keymask, KeyHash::seed(), cm.dev.d_pks, cm.dev.d_kflags, cm.dev.n, cm.dev.d_tabptr,
        cm.dev.digit_bits, btable, comb16, d_flags ? d_flags + base : nullptr, d_bits ? d_bits + base / 32 : nullptr, d_fault, d_totals, s);
    if (e != hipSuccess) return hip_fail("committee transaction launch", e);
  }
  return HSV_OK;
}

// The host form: the staged walk of the generic one (staged_tx_host,
// hsv_tx.cpp) without a record region, through a slot of the committee's
// device; neither pipelined nor sharded, the tables live on one device.
int committee_tx_host(const hsv_committee &cm, const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t n,
                      uint8_t *flags_out) {
  DevCtx &c = ctx(cm.dev.device);
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  int rc = ensure_btable(c);
  if (rc == HSV_OK) rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  uint64_t *d_totals = nullptr;
  return staged_tx_host(
      c, txs, offsets, tx_size, 0, n, flags_out, 0,
      [&](hipStream_t s) { return tx_counts_begin(c, s, &d_totals); },
      [&](const uint8_t *d_txs, const uint64_t *d_offsets, size_t m, uint8_t *, uint8_t *d_flags, uint32_t *d_fault,
          hipStream_t s) {
        return committee_tx_enqueue(cm, c.d_btable, c.d_btable16, d_txs, d_offsets, tx_size, m, d_flags, nullptr,
                                    d_fault, d_totals, s);
      },
      "committee transaction verify");
}

// ---- whole messages of known signers ---------------------------------------------------
// hsv_committee_verify_msgs*: the message addressing and scheme of
// hsv_verify_msgs* (hsv_msgs_api.cpp), routed per item on the device as the
// transaction calls above -- three launches per round of at most kChunk items
// (hsv_launch_committee_msgs, hsv_committee_msgs.hip), no host round trip.

// n items already in HBM, in rounds of kChunk in order on `s` (d_offsets
// relative to d_msgs, so a round only moves along the offsets)
int committee_msgs_enqueue(const hsv_committee &cm, const uint32_t *btable, const uint32_t *comb16, const uint8_t *d_pk,
                           size_t pk_stride, const uint8_t *d_sig, size_t sig_stride, const uint8_t *d_msgs,
                           const uint64_t *d_offsets, size_t msg_len, size_t msg_stride, size_t n, uint8_t *d_flags,
                           uint32_t *d_bits, uint32_t *d_fault, uint64_t *d_totals, hipStream_t s) {
  for (size_t base = 0; base < n; base += kChunk) {
    const size_t m = std::min(kChunk, n - base);
    const hipError_t e = hsv_launch_committee_msgs(
        d_pk + base * pk_stride, pk_stride, d_sig + base * sig_stride, sig_stride,
        d_offsets ? d_msgs : d_msgs + base * msg_stride, d_offsets ? d_offsets + base : nullptr, msg_len, msg_stride,
        (uint32_t)m, cm.d_keytab, cm.keymask, KeyHash::seed(), cm.dev.d_pks, cm.dev.d_kflags, cm.dev.n,
        cm.dev.d_tabptr, cm.dev.digit_bits, btable, comb16, d_flags ? d_flags + base : nullptr,
        d_bits ? d_bits + base / 32 : nullptr, d_fault, d_totals, s);
    if (e != hipSuccess) return hip_fail("committee message launch", e);
  }
  return HSV_OK;
}

// The host form: the staged walk of hsv_verify_msgs (staged_msgs_host,
// hsv_msgs_api.cpp) on the committee's device; neither pipelined nor sharded,
// the tables live on one device.
int committee_msgs_host(const hsv_committee &cm, const uint8_t *pk, const uint8_t *sig, const uint8_t *msgs,
                        const uint64_t *offsets, size_t msg_len, size_t msg_stride, size_t n, uint8_t *flags_out) {
  DevCtx &c = ctx(cm.dev.device);
  uint64_t *d_totals = nullptr;
  return staged_msgs_host(
      c,
      [&] {
        const int rc = ensure_btable(c);
        return rc == HSV_OK ? ensure_btable16(c) : rc;
      },
      [&](hipStream_t st) { return counts_begin(c, st, kMsgCountOff, c.msg_count_rr, t_msg_counts, &d_totals); },
      [&](const uint8_t *d_pk, const uint8_t *d_sig, const uint8_t *d_msgs, const uint64_t *d_offsets, size_t m,
          uint8_t *d_flags, uint32_t *d_fault, hipStream_t st) {
        return hsv_launch_committee_msgs(d_pk, 32, d_sig, 64, d_msgs, d_offsets, msg_len, msg_stride, (uint32_t)m,
                                         cm.d_keytab, cm.keymask, KeyHash::seed(), cm.dev.d_pks, cm.dev.d_kflags,
                                         cm.dev.n, cm.dev.d_tabptr, cm.dev.digit_bits, c.d_btable, c.d_btable16,
                                         d_flags, nullptr, d_fault, d_totals, st);
      },
      "allocating the committee message buffers", "hsv_committee_verify_msgs", StagedColumn{pk, 32}, sig, msgs, offsets,
      msg_len, msg_stride, n, flags_out);
}

// ---- whole messages by member index ------------------------------------------------------
// hsv_committee_verify_msgs_indexed*: the messages of the calls above, the
// signer named by its member index as hsv_committee_verify* names it -- no
// lookup, no miss side, no list lengths to report
// (hsv_launch_committee_msgs_indexed, hsv_committee_msgs.hip).

// the quad form forced by the test hook needs 8-bit tables
int indexed_form_ok(const hsv_committee &cm) {
  if (hsvi_cmsg_indexed_form() == 1 && cm.dev.digit_bits != 8)
    return fail(HSV_ERR_INVALID_ARG, "the quad form needs a committee with 8-bit tables");
  return HSV_OK;
}

// n items already in HBM, in rounds of kChunk in order on `s`
int committee_msgs_indexed_enqueue(const hsv_committee &cm, const uint32_t *btable, const uint32_t *comb16,
                                   const uint32_t *d_key_idx, const uint8_t *d_sig, size_t sig_stride,
                                   const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                                   size_t n, uint8_t *d_flags, uint32_t *d_fault, hipStream_t s) {
  for (size_t base = 0; base < n; base += kChunk) {
    const size_t m = std::min(kChunk, n - base);
    const hipError_t e = hsv_launch_committee_msgs_indexed(
        d_key_idx + base, d_sig + base * sig_stride, sig_stride, d_offsets ? d_msgs : d_msgs + base * msg_stride,
        d_offsets ? d_offsets + base : nullptr, msg_len, msg_stride, (uint32_t)m, cm.dev.d_pks, cm.dev.d_kflags,
        cm.dev.n, cm.dev.d_tabptr, cm.dev.digit_bits, btable, comb16, d_flags + base, d_fault, s);
    if (e != hipSuccess) return hip_fail("committee indexed message launch", e);
  }
  return HSV_OK;
}

// The host form: staged_msgs_host with the member indices staged where the
// other calls stage pk.
int committee_msgs_indexed_host(const hsv_committee &cm, const uint32_t *key_idx, const uint8_t *sig,
                                const uint8_t *msgs, const uint64_t *offsets, size_t msg_len, size_t msg_stride,
                                size_t n, uint8_t *flags_out) {
  DevCtx &c = ctx(cm.dev.device);
  return staged_msgs_host(
      c,
      [&] {
        const int rc = ensure_btable(c);
        return rc == HSV_OK ? ensure_btable16(c) : rc;
      },
      nullptr,
      [&](const uint8_t *d_col, const uint8_t *d_sig, const uint8_t *d_msgs, const uint64_t *d_offsets, size_t m,
          uint8_t *d_flags, uint32_t *d_fault, hipStream_t st) {
        return hsv_launch_committee_msgs_indexed(reinterpret_cast<const uint32_t *>(d_col), d_sig, 64, d_msgs, d_offsets,
                                                 msg_len, msg_stride, (uint32_t)m, cm.dev.d_pks, cm.dev.d_kflags,
                                                 cm.dev.n, cm.dev.d_tabptr, cm.dev.digit_bits, c.d_btable,
                                                 c.d_btable16, d_flags, d_fault, st);
      },
      "allocating the committee message buffers", "hsv_committee_verify_msgs_indexed",
      StagedColumn{reinterpret_cast<const uint8_t *>(key_idx), 4}, sig, msgs, offsets, msg_len, msg_stride, n,
      flags_out);
}

}  // namespace

// The committee routes of the serialized-batch calls (hsv_batch_api.cpp), which
// cannot see into the handle: its device, and committee_tx_enqueue over a span
// table (n transactions in HBM, transaction i = d_bufs[d_spans[2i], d_spans[2i+1]),
// rounds of kChunk in order on `s`, every flag byte written; device c current).
int committee_device_of(const hsv_committee *cm) { return cm->dev.device; }

CommitteeKeys committee_keys_of(const hsv_committee *cm) {
  CommitteeKeys k;
  k.device = cm->dev.device;
  k.n = cm->dev.n;
  k.d_keytab = cm->d_keytab;
  k.keymask = cm->keymask;
  k.d_pks = cm->dev.d_pks;
  return k;
}

int committee_tx_spans_enqueue(const hsv_committee *cm, DevCtx &c, const uint32_t *btable, const uint32_t *comb16,
                               const uint8_t *d_bufs, const uint64_t *d_spans, size_t n, uint8_t *d_flags,
                               uint32_t *d_fault, hipStream_t s) {
  uint64_t *d_totals = nullptr;
  const int rc = tx_counts_begin(c, s, &d_totals);
  if (rc != HSV_OK) return rc;
  for (size_t base = 0; base < n; base += kChunk) {
    const size_t m = std::min(kChunk, n - base);
    const hipError_t e = hsv_launch_committee_tx_spans(
        d_bufs, d_spans + 2 * base, (uint32_t)m, cm->d_keytab, cm->keymask, KeyHash::seed(), cm->dev.d_pks,
        cm->dev.d_kflags, cm->dev.n, cm->dev.d_tabptr, cm->dev.digit_bits, btable, comb16, d_flags + base, nullptr,
        d_fault, d_totals, s);
    if (e != hipSuccess) return hip_fail("committee transaction launch", e);
  }
  return HSV_OK;
}

int committee_tx_counts(uint64_t out[3]) {
  return counts_read(t_tx_counts, kTxCountOff, "no committee transaction call on this thread", out);
}

int committee_msgs_counts(uint64_t out[3]) {
  return counts_read(t_msg_counts, kMsgCountOff, "no committee message call on this thread", out);
}

}  // namespace hsvh

extern "C" {

int hsv_committee_verify_transactions(hsv_committee *cm, const uint8_t *txs, const uint64_t *offsets, size_t tx_size,
                                      size_t n, uint8_t *flags_out) {
  CallScope call;
  if (n == 0) return HSV_OK;
  if (!cm || !txs || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = tx_lengths_ok(offsets, tx_size, n);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();
  if (rc != HSV_OK) return rc;
  return committee_tx_host(*cm, txs, offsets, tx_size, n, flags_out);
}

int hsv_committee_verify_transactions_device(const hsv_committee *cm, const uint8_t *d_txs, const uint64_t *d_offsets,
                                             size_t tx_size, size_t n, uint8_t *d_flags, uint32_t *d_strict_bits,
                                             uint32_t *d_fault, void *stream) {
  if (n == 0) return HSV_OK;
  if (!cm || !d_txs) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = tx_device_args_ok(d_offsets, tx_size, d_flags, d_strict_bits);
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  rc = call.begin(d_txs, stream, d_fault, DeviceCall::kBoth, "committee", cm->dev.device);
  if (rc != HSV_OK) return rc;
  uint64_t *d_totals = nullptr;
  rc = tx_counts_begin(*call.c, call.stream, &d_totals);
  if (rc != HSV_OK) return rc;
  return committee_tx_enqueue(*cm, call.comb, call.comb16, d_txs, d_offsets, tx_size, n, d_flags, d_strict_bits,
                              call.fault, d_totals, call.stream);
}

int hsv_committee_verify_msgs(hsv_committee *cm, const uint8_t *pk, const uint8_t *sig, const uint8_t *msgs,
                              const uint64_t *offsets, size_t msg_len, size_t msg_stride, size_t n,
                              uint8_t *flags_out) {
  CallScope call;
  if (n == 0) return HSV_OK;
  if (!cm || !pk || !sig || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = msgs_host_args_ok(msgs, offsets, msg_len, msg_stride, n);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  return committee_msgs_host(*cm, pk, sig, msgs, offsets, msg_len, msg_stride, n, flags_out);
}

int hsv_committee_verify_msgs_device(const hsv_committee *cm, const uint8_t *d_pk, size_t pk_stride,
                                     const uint8_t *d_sig, size_t sig_stride, const uint8_t *d_msgs,
                                     const uint64_t *d_offsets, size_t msg_len, size_t msg_stride, size_t n,
                                     uint8_t *d_flags, uint32_t *d_strict_bits, uint32_t *d_fault, void *stream) {
  if (n == 0) return HSV_OK;
  if (!cm || !d_pk || !d_sig) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = msgs_device_args_ok(d_pk, pk_stride, d_sig, sig_stride, d_msgs, d_offsets, msg_len, msg_stride, d_flags,
                               d_strict_bits);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  rc = call.begin(d_pk, stream, d_fault, DeviceCall::kBoth, "committee", cm->dev.device);
  if (rc != HSV_OK) return rc;
  uint64_t *d_totals = nullptr;
  rc = counts_begin(*call.c, call.stream, kMsgCountOff, call.c->msg_count_rr, t_msg_counts, &d_totals);
  if (rc != HSV_OK) return rc;
  return committee_msgs_enqueue(*cm, call.comb, call.comb16, d_pk, pk_stride, d_sig, sig_stride, d_msgs, d_offsets,
                                msg_len, msg_stride, n, d_flags, d_strict_bits, call.fault, d_totals, call.stream);
}

int hsv_committee_verify_msgs_indexed(hsv_committee *cm, const uint32_t *key_idx, const uint8_t *sig,
                                      const uint8_t *msgs, const uint64_t *offsets, size_t msg_len, size_t msg_stride,
                                      size_t m, uint8_t *flags_out) {
  CallScope call;
  if (m == 0) return HSV_OK;
  if (!cm || !key_idx || !sig || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = msgs_host_args_ok(msgs, offsets, msg_len, msg_stride, m);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  rc = indexed_form_ok(*cm);
  if (rc != HSV_OK) return rc;
  return committee_msgs_indexed_host(*cm, key_idx, sig, msgs, offsets, msg_len, msg_stride, m, flags_out);
}

int hsv_committee_verify_msgs_indexed_device(const hsv_committee *cm, const uint32_t *d_key_idx, const uint8_t *d_sig,
                                             size_t sig_stride, const uint8_t *d_msgs, const uint64_t *d_offsets,
                                             size_t msg_len, size_t msg_stride, size_t m, uint8_t *d_flags,
                                             uint32_t *d_fault, void *stream) {
  if (m == 0) return HSV_OK;
  if (!cm || !d_key_idx || !d_sig || !d_flags) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (m > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if (reinterpret_cast<uintptr_t>(d_key_idx) & 3u) return fail(HSV_ERR_ALIGN, "d_key_idx must be 4-byte aligned");
  // the checks of the pk-addressed call from "null d_msgs" on; there is no pk column to check
  int rc = msgs_device_args_ok(nullptr, 32, d_sig, sig_stride, d_msgs, d_offsets, msg_len, msg_stride, d_flags, nullptr);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  rc = indexed_form_ok(*cm);
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  rc = call.begin(d_sig, stream, d_fault, DeviceCall::kBoth, "committee", cm->dev.device);
  if (rc != HSV_OK) return rc;
  return committee_msgs_indexed_enqueue(*cm, call.comb, call.comb16, d_key_idx, d_sig, sig_stride, d_msgs, d_offsets,
                                        msg_len, msg_stride, m, d_flags, call.fault, call.stream);
}

}  // extern "C"
