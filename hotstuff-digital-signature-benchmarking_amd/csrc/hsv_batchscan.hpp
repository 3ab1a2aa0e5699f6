// The walk over a serialized MempoolMessage::Batch (bincode 1.3 defaults:
//     u32 LE variant tag (0 = Batch) | u64 LE count | count x (u64 LE length, bytes)
// mempool/src/batch_maker.rs:127-131, read back by consensus/src/core.rs:113-142),
// window by window.  Host and device: hsv_batchwire.hip runs it from an LDS
// window one wave per batch, tests/native/batchscan_host.cpp from a host array
// against hsvw::parse_batch.
//
// The batch is read as a stream of 16-byte chunks that starts at the chunk
// holding its first byte: stream byte s is batch byte s - mis, mis = the batch
// address mod 16.  Window k holds stream bytes [k * kScanWindow, (k + 1) *
// kScanWindow) as 32-bit words, followed by kScanSlackWords words of any
// content (a read near the window's end may run into them; what it reads there
// is masked off).  The caller hands the windows over in order, 0, 1, ..., until
// done() -- at most windows() of them; bytes past the batch's end are never
// interpreted.  A length prefix that straddles a window edge is finished from
// the next window (carry).
//
// Malformed (kBatchParse), the rules of hsvw::parse_batch: a tag other than 0,
// truncation anywhere, a count above the remaining bytes / 8, a length that
// runs past the batch's own end (compared against the bytes left, so no
// addition can overflow), trailing bytes after the last transaction.
//
// Every step of the loop in window() consumes a prefix of 8 bytes or leaves
// the window, so a batch of len bytes costs at most len / 8 steps and
// windows() windows whatever its bytes say.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HSV_BS_FN __host__ __device__ __forceinline__
#else
#define HSV_BS_FN inline
#endif

namespace hsv {

// hsv_batch_result.status (include/hsv.h)
constexpr uint32_t kBatchOk = 0, kBatchTx = 1, kBatchParse = 2, kBatchOverflow = 3;

constexpr uint32_t kScanWindow = 1024;   // W: one 16-byte chunk per lane of a wave
constexpr uint32_t kScanSlackWords = 4;  // readable words behind a window
constexpr uint32_t kBatchHeader = 12;    // tag + count

// On the device every lane of the wave reads the same words, so what it read
// is wave-uniform; saying so keeps the whole walk -- positions, counts,
// comparisons, branches -- in scalar registers (DESIGN.md 4o has what the
// walk costs per length prefix).
#if defined(__HIP_DEVICE_COMPILE__)
#define HSV_BS_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define HSV_BS_UNIFORM(x) (x)
#endif

// the 8 bytes at byte `off` of the little-endian words w (reads w[off/4 .. off/4 + 2])
HSV_BS_FN uint64_t scan_rd64(const uint32_t *w, uint32_t off) {
  const uint32_t i = off >> 2, sh = (off & 3u) * 8u;
  const uint32_t w0 = HSV_BS_UNIFORM(w[i]), w1 = HSV_BS_UNIFORM(w[i + 1]);
  const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32);
  const uint64_t hi = HSV_BS_UNIFORM(w[i + 2]);
  return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

struct BatchWalk {
  uint64_t send;   // stream position of the batch's end: mis + len
  uint64_t spos;   // stream position of the next length prefix
  uint64_t left;   // transactions whose prefix has not been read
  uint64_t count;  // the batch's count (valid once the header is read)
  uint64_t carry;  // the first carry_n bytes of the prefix at spos (from the window before)
  uint32_t carry_n;
  uint32_t mis;
  uint32_t state;  // kHeader, kPrefix, then kDone or kBad
  enum : uint32_t { kHeader, kPrefix, kDone, kBad };

  HSV_BS_FN void begin(uint64_t len, uint32_t mis_) {
    mis = mis_;
    send = len + mis_;
    spos = mis_;
    left = count = carry = 0;
    carry_n = 0;
    state = len < kBatchHeader ? kBad : kHeader;  // truncated header
  }
  HSV_BS_FN bool done() const { return state >= kDone; }
  HSV_BS_FN bool ok() const { return state == kDone; }
  // windows that hold the batch's bytes
  HSV_BS_FN uint64_t windows() const { return (send + kScanWindow - 1) / kScanWindow; }

  // Window k (the windows come in order).  emit(i, lo, hi): transaction i of the
  // batch is its bytes [lo, hi).
  template <class Emit>
  HSV_BS_FN void window(const uint32_t *w, uint64_t k, Emit &&emit) {
    const uint64_t wlo = k * kScanWindow, wend = wlo + kScanWindow;
    if (state == kHeader) {  // k == 0: mis + 12 <= 27, the header lies in the first window
      const uint32_t tag = (uint32_t)scan_rd64(w, mis);
      count = scan_rd64(w, mis + 4u);
      spos = (uint64_t)mis + kBatchHeader;
      if (tag != 0u || count > (send - spos) / 8u) {
        state = kBad;  // not a Batch, or a count beyond the buffer
        return;
      }
      left = count;
      state = kPrefix;
    }
    while (state == kPrefix) {
      if (left == 0) {
        state = spos == send ? kDone : kBad;  // trailing bytes
        return;
      }
      uint64_t v;
      if (carry_n) {  // the prefix began in the window before
        v = carry | (scan_rd64(w, 0) << (8u * carry_n));
        carry_n = 0;
      } else {
        if (send - spos < 8u) {  // (spos <= send always)
          state = kBad;  // truncated prefix
          return;
        }
        if (spos >= wend) return;  // the next prefix lies in a later window, which exists
        const uint32_t off = (uint32_t)(spos - wlo);
        v = scan_rd64(w, off);
        if (spos + 8u > wend) {  // 1..7 of its bytes are here
          carry_n = (uint32_t)(wend - spos);
          carry = v & ((1ull << (8u * carry_n)) - 1ull);
          return;
        }
      }
      const uint64_t body = spos + 8u;
      if (v > send - body) {
        state = kBad;  // runs past the batch's end
        return;
      }
      emit(count - left, body - mis, body - mis + v);
      spos = body + v;
      --left;
    }
  }
};

}  // namespace hsv
