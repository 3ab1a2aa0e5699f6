// C ABI of Ed25519 verification over messages of any length (include/hsv.h,
// hsv_verify_msgs*): RFC 8032 5.1.7, k = SHA-512(R || A || M) over the whole
// message, everything else as hsv_verify (dalek's verify_strict).  The verifying
// half of hsv_signer_sign* / hsv_sign_many.  Kernels: csrc/hsv_msgs.hip (the
// message prepass) and the point pass of csrc/hsv_kernels.hip.  The host form
// is plain staged copies on one device: no pipelining, no multi-GPU sharding.
#include <algorithm>
#include <string>
#include <vector>

#include "hsv_host.h"

using namespace hsvh;

namespace {

constexpr size_t kMsgChunkBytes = size_t(1) << 29;  // message bytes staged per launch (one longer message: alone)

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

// bytes of the caller's buffer that items [a, b) span, from byte *first
size_t span_bytes(const uint64_t *offsets, size_t msg_len, size_t msg_stride, size_t a, size_t b, size_t *first) {
  if (offsets) {
    *first = (size_t)offsets[a];
    return (size_t)(offsets[b] - offsets[a]);
  }
  *first = a * msg_stride;
  return msg_stride ? (b - a - 1) * msg_stride + msg_len : msg_len;
}

}  // namespace

extern "C" {

int hsv_verify_msgs_device(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig, size_t sig_stride,
                           const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                           size_t n, uint8_t *d_flags, uint32_t *d_strict_bits, uint32_t *d_fault, void *stream) {
  if (n == 0) return HSV_OK;
  if (!d_pk || !d_sig) return fail(HSV_ERR_INVALID_ARG, "null input pointer");
  if (!d_msgs && (d_offsets || msg_len)) return fail(HSV_ERR_INVALID_ARG, "null d_msgs");
  if (!d_flags && !d_strict_bits) return fail(HSV_ERR_INVALID_ARG, "no output");
  const uintptr_t mis =
      (reinterpret_cast<uintptr_t>(d_pk) | reinterpret_cast<uintptr_t>(d_sig) | pk_stride | sig_stride) & 15u;
  if (mis) return fail(HSV_ERR_ALIGN, "d_pk, d_sig and their strides must be multiples of 16");
  if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return fail(HSV_ERR_ALIGN, "d_offsets must be 8-byte aligned");
  if (pk_stride < 32 || sig_stride < 64) return fail(HSV_ERR_INVALID_ARG, "record strides overlap");
  if (!d_offsets && msg_stride != 0 && msg_stride < msg_len) return fail(HSV_ERR_INVALID_ARG, "messages overlap");
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  int dev = 0;
  rc = device_for_call(d_pk, stream, &dev);
  if (rc != HSV_OK) return rc;
  DeviceGuard guard(dev);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  DevCtx &c = ctx(dev);
  rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint32_t *fault = nullptr;
  rc = call_fault_words(c, d_fault, s, &fault);
  if (rc != HSV_OK) return rc;
  const hipError_t e = msgs_chunks(d_pk, pk_stride, d_sig, sig_stride, d_msgs, d_offsets, msg_len, msg_stride, n,
                                   d_flags, d_strict_bits, c.d_btable16, fault, s);
  return e == hipSuccess ? HSV_OK : hip_fail("message verify launch", e);
}

int hsv_verify_msgs(const uint8_t *pk, const uint8_t *sig, const uint8_t *msgs, const uint64_t *offsets,
                    size_t msg_len, size_t msg_stride, size_t n, uint8_t *flags_out) {
  CallScope call;
  if (n == 0) return HSV_OK;
  if (!pk || !sig || !flags_out) return fail(HSV_ERR_INVALID_ARG, "null pointer");
  if (n > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  bool any_bytes = !offsets && msg_len != 0;
  if (offsets) {
    for (size_t i = 0; i < n; ++i) {
      if (offsets[i + 1] < offsets[i])
        return fail(HSV_ERR_INVALID_ARG, "offsets decrease at message " + std::to_string(i));
      any_bytes |= offsets[i + 1] != offsets[i];
    }
  } else if (msg_stride != 0 && msg_stride < msg_len) {
    return fail(HSV_ERR_INVALID_ARG, "messages overlap");
  }
  if (any_bytes && !msgs) return fail(HSV_ERR_INVALID_ARG, "null msgs");
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(home_device());
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  rc = ensure_btable16(c);
  if (rc != HSV_OK) return rc;
  SlotLease lease(c);
  Slot &slot = lease.slot();
  rc = slot_prepare(slot, 0, 0);
  if (rc != HSV_OK) return rc;
  hipStream_t st = slot.stream;
  std::vector<uint64_t> rel;  // a chunk's offsets, relative to its first byte
  for (size_t a = 0; a < n;) {
    // items [a, b): at most kChunk, and at most kMsgChunkBytes of messages unless one message is longer
    size_t b = a + 1, first = 0;
    if (!offsets) {
      const size_t per = msg_stride ? std::max<size_t>(1, kMsgChunkBytes / msg_stride) : kChunk;
      b = std::min(n, a + std::min(kChunk, per));
    } else {
      while (b < n && b - a < kChunk && offsets[b + 1] - offsets[a] <= kMsgChunkBytes) ++b;
    }
    const size_t m = b - a;
    const size_t bytes = span_bytes(offsets, msg_len, msg_stride, a, b, &first);
    // one stream-ordered block from the library pool:
    // pk | sig | flags | fault words | offsets | message bytes
    const size_t off_sig = round_up(m * 32, kAlign), off_flags = off_sig + round_up(m * 64, kAlign);
    const size_t off_fault = off_flags + round_up(m, kAlign), off_offs = off_fault + kAlign;
    const size_t off_msg = off_offs + round_up(offsets ? (m + 1) * 8 : 0, kAlign);
    void *blk = nullptr;
    hipError_t e = hsv_ws_malloc(&blk, off_msg + bytes + kAlign, st);
    if (e != hipSuccess) return hip_fail("allocating the message verification buffers", e);
    uint8_t *d = static_cast<uint8_t *>(blk);
    uint32_t *d_fault = reinterpret_cast<uint32_t *>(d + off_fault);
    uint64_t *d_offs = offsets ? reinterpret_cast<uint64_t *>(d + off_offs) : nullptr;
    uint8_t words[kFaultBytes] = {0};
    // unwritten flags read as rejections; self-check words start at zero
    e = hipMemsetAsync(d + off_flags, 0, off_fault + kFaultBytes - off_flags, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d, pk + a * 32, m * 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + off_sig, sig + a * 64, m * 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && offsets) {
      rel.resize(m + 1);
      for (size_t k = 0; k <= m; ++k) rel[k] = offsets[a + k] - offsets[a];
      e = hipMemcpyAsync(d_offs, rel.data(), (m + 1) * 8, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(d + off_msg, msgs + first, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      e = hsv_launch_verify_msgs(d, 32, d + off_sig, 64, d + off_msg, d_offs, msg_len, msg_stride, (uint32_t)m,
                                 d + off_flags, nullptr, c.d_btable16, d_fault, st);
    if (e == hipSuccess) e = hipMemcpyAsync(flags_out + a, d + off_flags, m, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(words, d_fault, kFaultBytes, hipMemcpyDeviceToHost, st);
    const hipError_t ef = hipFreeAsync(blk, st);
    const hipError_t es = hipStreamSynchronize(st);  // nothing of this call stays in flight
    if (e == hipSuccess) e = ef;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail("hsv_verify_msgs", e);
    rc = check_faults(words, "hsv_verify_msgs");
    if (rc != HSV_OK) return rc;
    a = b;
  }
  return HSV_OK;
}

}  // extern "C"
