// The arithmetic of sealing verified transactions into MempoolMessage::Batch
// messages (hsv_seal_transactions*, include/hsv.h), as plain functions for the
// kernels of hsv_seal.hip and for the host (tests/native/seal_host.cpp):
//
//   * the class of a transaction (kept, rejected, malformed) and its length;
//   * the greedy cut of BatchMaker::run (mempool/src/batch_maker.rs:87-92) over
//     the inclusive prefix sums of the kept lengths, one 64-entry piece at a
//     time (SealCut);
//   * where a sealed transaction's bytes go (seal_dst);
//   * the copy of one destination-aligned 16-byte chunk from a source of any
//     alignment (seal_copy_chunk).
//
// Layout of a batch (bincode 1.3 defaults, hsv_batchscan.hpp):
//     u32 LE 0 | u64 LE count | count x (u64 LE length, bytes)
// Batches lie end to end, so the k-th kept transaction (rank k, counted from
// 0) of batch b (from 0), with e kept bytes before it, has its bytes at
// 12 (b + 1) + 8 (k + 1) + e and its length prefix in the 8 bytes before them:
// every batch up to its own has laid down a header, every kept transaction up
// to itself a prefix.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HSV_SEAL_FN __host__ __device__ __forceinline__
#else
#define HSV_SEAL_FN inline
#endif

namespace hsv {

constexpr uint32_t kSealHeader = 12;          // tag + count
constexpr uint32_t kSealPrefix = 8;           // a transaction's length
constexpr uint32_t kSealTile = 256;           // transactions per workgroup of the scan
constexpr uint64_t kSealPiece = 16384;        // bytes of a transaction one lane group copies
constexpr uint32_t kSealKept = 0, kSealRejected = 1, kSealMalformed = 2;  // a transaction's class
constexpr uint8_t kSealStrictOk = 0x01;       // HSV_STRICT_OK

// Transaction [lo, hi) with flag byte `flag` (has_flags false: every
// transaction is kept, whatever its length).  Decreasing offsets: malformed,
// whatever the flags say.
HSV_SEAL_FN uint32_t seal_class(uint64_t lo, uint64_t hi, bool has_flags, uint8_t flag) {
  if (hi < lo) return kSealMalformed;
  return !has_flags || (flag & kSealStrictOk) ? kSealKept : kSealRejected;
}

// 16 KiB pieces of a kept transaction beyond its first
HSV_SEAL_FN uint32_t seal_extra_pieces(uint64_t len) {
  return len > kSealPiece ? (uint32_t)((len - 1) / kSealPiece) : 0u;
}

// first byte of the transaction's bytes in the output: batch b, kept rank k
// (both from 0), e kept bytes before it
HSV_SEAL_FN uint64_t seal_dst(uint64_t b, uint64_t k, uint64_t e) {
  return (uint64_t)kSealHeader * (b + 1) + (uint64_t)kSealPrefix * (k + 1) + e;
}
// first byte of batch b, whose first transaction has rank k and e kept bytes before it
HSV_SEAL_FN uint64_t seal_batch_start(uint64_t b, uint64_t k, uint64_t e) {
  return (uint64_t)kSealHeader * b + (uint64_t)kSealPrefix * k + e;
}

// hsv_seal_bound's arithmetic: never below the true need.  A batch closes at a
// kept transaction, so there are at most n; every closed batch but a flushed
// last one holds at least batch_size bytes.  false: the sums do not fit 64 bits.
HSV_SEAL_FN bool seal_bound(uint64_t total, uint64_t n, uint64_t batch_size, uint64_t *bytes, uint64_t *batches) {
  const uint64_t by_size = total / batch_size;  // (batch_size != 0: the caller's check)
  const uint64_t nb = n == 0 ? 0 : (by_size + 1 < n ? by_size + 1 : n);
  if (n > (~0ull - total) / 8u) return false;
  const uint64_t body = total + 8u * n;
  if (nb > (~0ull - body) / kSealHeader) return false;
  *bytes = body + (uint64_t)kSealHeader * nb;
  *batches = nb;
  return true;
}

// The greedy cut as a walk over entries (E, R): E the kept bytes, R the kept
// transactions up to and including entry i.  An entry closes a batch when the
// bytes since the last cut reach batch_size; a transaction that is not kept
// repeats the entry before it and so never closes one (batch_size >= 1), nor
// does a kept transaction of no bytes.  The differences E - cut_e never
// overflow, whatever batch_size is.
struct SealCut {
  uint64_t batch_size;
  uint64_t cut_e = 0, cut_r = 0;  // E and R at the last cut
  int64_t cut_i = -1;             // its index
  uint64_t nb = 0;                // batches closed
  HSV_SEAL_FN bool closes(uint64_t i, uint64_t e) const {
    return (int64_t)i > cut_i && e - cut_e >= batch_size;
  }
  HSV_SEAL_FN void close(uint64_t i, uint64_t e, uint64_t r) {
    cut_i = (int64_t)i;
    cut_e = e;
    cut_r = r;
    ++nb;
  }
};

// ---- the byte-shifting copy ---------------------------------------------------
struct SealChunk {
  uint64_t lo, hi;  // bytes 0..7 and 8..15, little-endian
};

// the 16 bytes at byte `sh` (0..15) of a || b
HSV_SEAL_FN SealChunk seal_shift(SealChunk a, SealChunk b, uint32_t sh) {
  uint64_t x0 = a.lo, x1 = a.hi, x2 = b.lo;
  if (sh & 8u) {
    x0 = a.hi;
    x1 = b.lo;
    x2 = b.hi;
  }
  const uint32_t s = (sh & 7u) * 8u;
  SealChunk r;
  r.lo = s ? (x0 >> s) | (x1 << (64u - s)) : x0;
  r.hi = s ? (x1 >> s) | (x2 << (64u - s)) : x1;
  return r;
}
HSV_SEAL_FN uint8_t seal_byte(SealChunk v, uint32_t k) {
  return (uint8_t)((k < 8u ? v.lo >> (8u * k) : v.hi >> (8u * (k - 8u))) & 0xffu);
}

// A copy of len > 0 bytes from stream position spos to stream position dpos.
// Positions are byte offsets from 16-byte aligned bases (the source's and the
// destination's own), so position p lies in the aligned chunk p >> 4 of its
// base.  The destination is written chunk by chunk: chunks() of them, each by
// one call of chunk(c, ...) in any order and by any lane.  A chunk that lies
// wholly inside the destination goes out as one 16-byte store (st16), the at
// most two others byte by byte (st1); nothing outside [dpos, dpos + len) is
// written.  The source is read in aligned chunks (ld), only chunks that hold a
// byte of [spos, spos + len), and shifted into place.
struct SealCopy {
  uint64_t spos, dpos, len;
  HSV_SEAL_FN uint64_t first_chunk() const { return dpos >> 4; }
  HSV_SEAL_FN uint64_t chunks() const { return ((dpos + len - 1) >> 4) - (dpos >> 4) + 1; }
  // ld(k) -> SealChunk k of the source base; st16(k, v): chunk k of the
  // destination base; st1(p, byte): destination position p
  template <class Load, class Store16, class Store1>
  HSV_SEAL_FN void chunk(uint64_t c, Load &&ld, Store16 &&st16, Store1 &&st1) const {
    const uint64_t dc = first_chunk() + c;           // destination chunk
    const int64_t d = (int64_t)spos - (int64_t)dpos;  // source position - destination position
    const uint32_t sh = (uint32_t)(d & 15);
    const int64_t k = (int64_t)dc + (d >> 4);  // the source chunk that holds the byte for the chunk's byte 0
    const int64_t k_first = (int64_t)(spos >> 4), k_last = (int64_t)((spos + len - 1) >> 4);
    SealChunk a = {0, 0}, b = {0, 0};
    if (k >= k_first && k <= k_last) a = ld((uint64_t)k);
    if (sh && k + 1 >= k_first && k + 1 <= k_last) b = ld((uint64_t)(k + 1));
    const SealChunk v = seal_shift(a, b, sh);
    const uint64_t base = dc << 4;
    const uint32_t lo = base < dpos ? (uint32_t)(dpos - base) : 0u;
    const uint32_t hi = base + 16u > dpos + len ? (uint32_t)(dpos + len - base) : 16u;
    if (lo == 0u && hi == 16u) {
      st16(dc, v);
    } else {
      for (uint32_t j = lo; j < hi; ++j) st1(base + j, seal_byte(v, j));
    }
  }
};

}  // namespace hsv
