// C ABI of Ed25519 verification over messages of any length (include/hsv.h,
// hsv_verify_msgs*): RFC 8032 5.1.7, k = SHA-512(R || A || M) over the whole
// message, everything else as hsv_verify (dalek's verify_strict).  The verifying
// half of hsv_signer_sign* / hsv_sign_many.  Kernels: csrc/hsv_msgs.hip (the
// message prepass) and the point pass of csrc/hsv_kernels.hip.  The host form
// is plain staged copies on one device: no pipelining, no multi-GPU sharding.
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "hsv_host.h"

using namespace hsvh;

namespace {

// launches of at most kChunk items, one after the other on `stream`
hipError_t msgs_chunks(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig, size_t sig_stride,
                       const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride, size_t n,
                       uint8_t *d_flags, uint32_t *d_bits, const uint32_t *comb16, uint32_t *fault,
                       hipStream_t stream) {
  hipError_t e = hipSuccess;
  for (size_t base = 0; base < n && e == hipSuccess; base += kChunk) {
    const size_t m = std::min(kChunk, n - base);
    // offsets are relative to d_msgs, so a chunk only moves along the offsets
    e = hsv_launch_verify_msgs(d_pk + base * pk_stride, pk_stride, d_sig + base * sig_stride, sig_stride,
                               d_offsets ? d_msgs : d_msgs + base * msg_stride, d_offsets ? d_offsets + base : nullptr,
                               msg_len, msg_stride, (uint32_t)m, d_flags ? d_flags + base : nullptr,
                               d_bits ? d_bits + base / 32 : nullptr, comb16, fault, stream);
  }
  return e;
}

}  // namespace

namespace hsvh {

int msgs_host_args_ok(const uint8_t *msgs, const uint64_t *offsets, size_t msg_len, size_t msg_stride, size_t n) {
  if (n > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  bool any_bytes = msg_len != 0;
  if (offsets) {
    const size_t bad = first_bad_item(offsets, n, 0);
    if (bad != n) return fail(HSV_ERR_INVALID_ARG, "offsets decrease at message " + std::to_string(bad));
    any_bytes = offsets[n] != offsets[0];
  } else if (msg_stride != 0 && msg_stride < msg_len) {
    return fail(HSV_ERR_INVALID_ARG, "messages overlap");
  }
  if (any_bytes && !msgs) return fail(HSV_ERR_INVALID_ARG, "null msgs");
  return HSV_OK;
}

int msgs_device_args_ok(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig, size_t sig_stride,
                        const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                        const uint8_t *d_flags, const uint32_t *d_strict_bits) {
  if (!d_msgs && (d_offsets || msg_len)) return fail(HSV_ERR_INVALID_ARG, "null d_msgs");
  if (!d_flags && !d_strict_bits) return fail(HSV_ERR_INVALID_ARG, "no output");
  const uintptr_t mis =
      (reinterpret_cast<uintptr_t>(d_pk) | reinterpret_cast<uintptr_t>(d_sig) | pk_stride | sig_stride) & 15u;
  if (mis) return fail(HSV_ERR_ALIGN, "d_pk, d_sig and their strides must be multiples of 16");
  if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return fail(HSV_ERR_ALIGN, "d_offsets must be 8-byte aligned");
  if (pk_stride < 32 || sig_stride < 64) return fail(HSV_ERR_INVALID_ARG, "record strides overlap");
  if (!d_offsets && msg_stride != 0 && msg_stride < msg_len) return fail(HSV_ERR_INVALID_ARG, "messages overlap");
  return HSV_OK;
}

// The one walk of the staged message host forms (hsv_host.h).
int staged_msgs_host(DevCtx &c, const std::function<int()> &tables, const StagedBegin &begin,
                     const MsgsLaunch &launch, const char *alloc_what, const char *finish_where,
                     const StagedColumn &col, const uint8_t *sig, const uint8_t *msgs, const uint64_t *offsets,
                     size_t msg_len, size_t msg_stride, size_t n, uint8_t *flags_out) {
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  int rc = tables();
  if (rc != HSV_OK) return rc;
  SlotLease lease(c);
  Slot &slot = lease.slot();
  rc = slot_prepare(slot, 0, 0);
  if (rc != HSV_OK) return rc;
  hipStream_t st = slot.stream;
  if (begin) rc = begin(st);
  if (rc != HSV_OK) return rc;
  const BatchSpan span{offsets, msg_stride, msg_len};
  std::vector<uint64_t> rel;  // a chunk's offsets, relative to its first byte
  for (size_t a = 0, b; a < n; a = b) {
    b = span.chunk_end(a, n, kChunk, g_stage_bytes.load());
    const size_t m = b - a, bytes = span.span_bytes(a, b);
    StagedBlock blk(st);
    const size_t off_flags = blk.add(m), off_col = blk.add(m * col.item_bytes), off_sig = blk.add(m * 64);
    const size_t off_offs = blk.add(offsets ? (m + 1) * 8 : 0), off_msg = blk.add(bytes);
    // unwritten flags read as rejections
    rc = blk.alloc(alloc_what, m);
    if (rc != HSV_OK) return rc;
    blk.in(off_col, col.src + a * col.item_bytes, m * col.item_bytes);
    blk.in(off_sig, sig + a * 64, m * 64);
    if (offsets) {
      rel.resize(m + 1);
      span.rel_offsets(a, b, rel.data());
      blk.in(off_offs, rel.data(), (m + 1) * 8);
    }
    blk.in(off_msg, msgs + span.first_byte(a), bytes);
    if (blk.ok())
      blk.step(launch(blk.at(off_col), blk.at(off_sig), blk.at(off_msg),
                      offsets ? reinterpret_cast<uint64_t *>(blk.at(off_offs)) : nullptr, m, blk.at(off_flags),
                      blk.fault(), st));
    blk.out(flags_out + a, off_flags, m);
    rc = blk.finish(finish_where);
    if (rc != HSV_OK) return rc;
  }
  return HSV_OK;
}

}  // namespace hsvh

extern "C" {

int hsv_verify_msgs_device(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig, size_t sig_stride,
                           const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                           size_t n, uint8_t *d_flags, uint32_t *d_strict_bits, uint32_t *d_fault, void *stream) {
  if (n == 0) return HSV_OK;
  if (!d_pk || !d_sig) return fail(HSV_ERR_INVALID_ARG, "null input pointer");
  int rc = msgs_device_args_ok(d_pk, pk_stride, d_sig, sig_stride, d_msgs, d_offsets, msg_len, msg_stride, d_flags,
                               d_strict_bits);
  if (rc != HSV_OK) return rc;
  DeviceCall call;
  rc = call.begin(d_pk, stream, d_fault, DeviceCall::kWide);
  if (rc != HSV_OK) return rc;
  const hipError_t e = msgs_chunks(d_pk, pk_stride, d_sig, sig_stride, d_msgs, d_offsets, msg_len, msg_stride, n,
                                   d_flags, d_strict_bits, call.comb, call.fault, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("message verify launch", e);
}

int hsv_verify_msgs(const uint8_t *pk, const uint8_t *sig, const uint8_t *msgs, const uint64_t *offsets,
                    size_t msg_len, size_t msg_stride, size_t n, uint8_t *flags_out) {
  CallScope call;
  if (n == 0) return HSV_OK;
  if (!pk || !sig || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null pointer");
  int rc = msgs_host_args_ok(msgs, offsets, msg_len, msg_stride, n);
  if (rc != HSV_OK) return rc;
  rc = ensure_init();
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(home_device());
  return staged_msgs_host(
      c, [&] { return ensure_btable16(c); }, nullptr,
      [&](const uint8_t *d_pk, const uint8_t *d_sig, const uint8_t *d_msgs, const uint64_t *d_offsets, size_t m,
          uint8_t *d_flags, uint32_t *d_fault, hipStream_t st) {
        return hsv_launch_verify_msgs(d_pk, 32, d_sig, 64, d_msgs, d_offsets, msg_len, msg_stride, (uint32_t)m,
                                      d_flags, nullptr, c.d_btable16, d_fault, st);
      },
      "allocating the message verification buffers", "hsv_verify_msgs", StagedColumn{pk, 32}, sig, msgs, offsets,
      msg_len, msg_stride, n, flags_out);
}

}  // extern "C"
