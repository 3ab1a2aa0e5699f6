// The kernels of hsv_seal_transactions* (include/hsv.h): from n transactions in
// HBM and their flags to MempoolMessage::Batch messages laid end to end, as
// BatchMaker::run / seal build them (mempool/src/batch_maker.rs:78-131), and
// optionally each batch's store key SHA-512(batch)[..32] (processor.rs:30).
//
// Launches on the caller's stream, each after the one before has ended; the
// kernel boundary is the only hand-off, no workgroup ever waits for another:
//   1. hsv_seal_reduce_kernel<MODE>   one lane per transaction: its class and
//      length; a workgroup's sums (kept bytes, kept, malformed, extra pieces).
//   2. hsv_seal_blocks_kernel         one workgroup: the exclusive scan of the
//      workgroup sums, and the call's totals.
//   3. hsv_seal_apply_kernel<MODE>    the same lanes again: the scan inside the
//      workgroup plus its base gives every transaction its record
//      {E, R, class} -- kept bytes and kept transactions up to and including
//      it -- and the inclusive count of 16 KiB pieces beyond the first.
//   4. hsv_seal_cut_kernel            one wave streams the records, eight
//      64-entry pieces in registers with the next eight in flight, and follows
//      the greedy rule (SealCut, hsv_seal.hpp): a ballot of the entries that
//      reach the threshold, the first lane set closes a batch, again until no
//      lane is set.  It writes each batch's first rank and byte offset, the
//      repeats behind them and the summary.
//   5. hsv_seal_copy_kernel<MODE>     sixteen lanes per transaction: the batch
//      by a binary search over the batches' first ranks, the length prefix
//      (and the 12-byte header before a batch's first transaction) as byte
//      stores of lanes side by side, then the first piece of its bytes as
//      destination-aligned 16-byte stores, the source read in its own aligned
//      chunks and shifted into place (SealCopy).
//      hsv_seal_pieces_kernel<MODE>   the pieces beyond the first of long
//      transactions, one wave per piece, found by a binary search over the
//      piece counts: a multi-megabyte transaction is spread over the device.
//   6. hsv_seal_digest_kernel         (digests asked for) one wave per batch
//      streams the bytes just written through LDS in 1 KiB windows and runs the
//      SHA-512 block function over them; the chain is serial per batch.
// On HSV_SEAL_OVERFLOW the cut kernel says so in the head of the workspace and
// kernels 5 and 6 return at once: nothing is written past a cap.
//
// Stores are plain vector stores; no kernel here uses scratch.
#include <hip/hip_runtime.h>

#include "hsv.h"
#include "hsv_internal.h"
#include "hsv_seal.hpp"
#include "hsv_sha512.hpp"

namespace hsv {

constexpr int kSealOffsets = 0, kSealFixed = 1;  // MODE
constexpr int kSealBlock = 256;
static_assert(kSealBlock == (int)kSealTile, "one lane per transaction of a tile");
constexpr int kSealAhead = 8;        // 64-entry pieces of the cut wave in registers
constexpr uint32_t kSealGroup = 16;  // lanes per transaction of the copy kernel
constexpr uint32_t kSealPieceGrid = 4096;

// a workgroup's sums, then (after the blocks kernel) the sums before it
struct alignas(16) SealSums {
  uint64_t bytes;
  uint32_t kept, malformed, extra, pad[3];
};
// a transaction's record: kept bytes and kept transactions up to and including it
struct alignas(16) SealRec {
  uint64_t e;
  uint32_t r, cls;
};
// head of the workspace
struct SealHead {
  SealSums total;           // blocks kernel (all zero when n == 0: the launcher's memset)
  uint32_t nb, status;      // cut kernel: batches written (0 on overflow), HSV_SEAL_*
  uint64_t sealed;          // cut kernel: transactions in them
};
constexpr size_t kSealHeadBytes = 256;
static_assert(sizeof(SealHead) <= kSealHeadBytes, "the head fits its region");

template <int MODE>
struct SealInput {
  const uint8_t *base;
  const uint64_t *offsets;
  uint64_t stride;
  const uint8_t *flags;
  __device__ __forceinline__ void span(uint32_t i, uint64_t &lo, uint64_t &hi) const {
    if constexpr (MODE == kSealOffsets) {
      lo = offsets[i];
      hi = offsets[(uint64_t)i + 1];
    } else {
      lo = (uint64_t)i * stride;
      hi = lo + stride;
    }
  }
  // class and kept length of transaction i
  __device__ __forceinline__ uint32_t classify(uint32_t i, uint64_t &len) const {
    uint64_t lo, hi;
    span(i, lo, hi);
    const uint32_t cls = seal_class(lo, hi, flags != nullptr, flags ? flags[i] : (uint8_t)0);
    len = cls == kSealKept ? hi - lo : 0;
    return cls;
  }
};

struct SealVals {
  uint64_t bytes;
  uint32_t kept, malformed, extra;
};
__device__ __forceinline__ SealVals seal_add(SealVals a, SealVals b) {
  return {a.bytes + b.bytes, a.kept + b.kept, a.malformed + b.malformed, a.extra + b.extra};
}
__device__ __forceinline__ SealVals seal_shfl_up(SealVals v, int d) {
  SealVals r;
  r.bytes = __shfl_up((unsigned long long)v.bytes, d);
  r.kept = (uint32_t)__shfl_up((int)v.kept, d);
  r.malformed = (uint32_t)__shfl_up((int)v.malformed, d);
  r.extra = (uint32_t)__shfl_up((int)v.extra, d);
  return r;
}
// inclusive scan over the workgroup's kSealBlock lanes; part: 4 entries of LDS
__device__ __forceinline__ SealVals seal_block_scan(SealVals v, SealVals *part, SealVals &block_total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  HSV_UNROLL
  for (int d = 1; d < 64; d <<= 1) {
    const SealVals u = seal_shfl_up(v, d);
    if (lane >= (uint32_t)d) v = seal_add(v, u);
  }
  if (lane == 63u) part[wave] = v;
  __syncthreads();
  SealVals before = {0, 0, 0, 0}, all = {0, 0, 0, 0};
  HSV_UNROLL
  for (uint32_t w = 0; w < kSealBlock / 64; ++w) {
    const SealVals p = part[w];
    if (w < wave) before = seal_add(before, p);
    all = seal_add(all, p);
  }
  block_total = all;
  return seal_add(before, v);
}

template <int MODE>
__device__ __forceinline__ SealVals seal_item(const SealInput<MODE> &in, uint32_t n, uint32_t &cls) {
  const uint64_t i = (uint64_t)blockIdx.x * kSealBlock + threadIdx.x;
  SealVals v = {0, 0, 0, 0};
  cls = kSealRejected;
  if (i < n) {
    uint64_t len;
    cls = in.classify((uint32_t)i, len);
    v.bytes = len;
    v.kept = cls == kSealKept;
    v.malformed = cls == kSealMalformed;
    v.extra = cls == kSealKept ? seal_extra_pieces(len) : 0u;
  }
  return v;
}

template <int MODE>
__global__ void __launch_bounds__(kSealBlock)
hsv_seal_reduce_kernel(SealInput<MODE> in, uint32_t n, SealSums *__restrict__ sums) {
  __shared__ SealVals part[kSealBlock / 64];
  uint32_t cls;
  SealVals total;
  (void)seal_block_scan(seal_item(in, n, cls), part, total);
  if (threadIdx.x == 0) {
    SealSums s = {total.bytes, total.kept, total.malformed, total.extra, {0u, 0u, 0u}};
    sums[blockIdx.x] = s;
  }
}

// sums[b] <- the sums of the workgroups before b; head->total <- all of them.
// Each lane takes a run of workgroups, as hsv_batch_index_kernel does.
__global__ void __launch_bounds__(kSealBlock)
hsv_seal_blocks_kernel(SealSums *__restrict__ sums, uint32_t nblk, SealHead *__restrict__ head) {
  __shared__ SealVals part[kSealBlock / 64];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nblk + kSealBlock - 1u) / kSealBlock;
  const uint32_t lo = min(t * per, nblk), hi = min(lo + per, nblk);
  SealVals mine = {0, 0, 0, 0};
  for (uint32_t b = lo; b < hi; ++b) {
    const SealSums s = sums[b];
    mine = seal_add(mine, {s.bytes, s.kept, s.malformed, s.extra});
  }
  SealVals total;
  const SealVals incl = seal_block_scan(mine, part, total);
  SealVals run = {incl.bytes - mine.bytes, incl.kept - mine.kept, incl.malformed - mine.malformed,
                  incl.extra - mine.extra};
  for (uint32_t b = lo; b < hi; ++b) {
    const SealSums s = sums[b];
    SealSums w = {run.bytes, run.kept, run.malformed, run.extra, {0u, 0u, 0u}};
    sums[b] = w;
    run = seal_add(run, {s.bytes, s.kept, s.malformed, s.extra});
  }
  if (t == 0) {
    SealSums w = {total.bytes, total.kept, total.malformed, total.extra, {0u, 0u, 0u}};
    head->total = w;
  }
}

template <int MODE>
__global__ void __launch_bounds__(kSealBlock)
hsv_seal_apply_kernel(SealInput<MODE> in, uint32_t n, const SealSums *__restrict__ sums, SealRec *__restrict__ recs,
                      uint32_t *__restrict__ xincl) {
  __shared__ SealVals part[kSealBlock / 64];
  uint32_t cls;
  SealVals total;
  const SealVals v = seal_block_scan(seal_item(in, n, cls), part, total);
  const uint64_t i = (uint64_t)blockIdx.x * kSealBlock + threadIdx.x;
  if (i < n) {
    const SealSums base = sums[blockIdx.x];
    SealRec r = {base.bytes + v.bytes, base.kept + v.kept, cls};
    recs[i] = r;
    xincl[i] = base.extra + v.extra;
  }
}

__device__ __forceinline__ uint64_t seal_readlane64(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// One wave.  brank: bcap + 1 words of the workspace (bcap = min(batches_cap, n));
// offsets: batches_cap + 1 entries; summary: hsv_seal_summary as eight 8-byte words.
__global__ void __launch_bounds__(64)
hsv_seal_cut_kernel(const SealRec *__restrict__ recs, uint32_t n, uint64_t batch_size, uint32_t flush,
                    uint64_t out_cap, uint64_t batches_cap, uint32_t bcap, SealHead *__restrict__ head,
                    uint32_t *__restrict__ brank, unsigned long long *__restrict__ offsets,
                    unsigned long long *__restrict__ summary) {
  const uint32_t lane = threadIdx.x;
  const uint4 *q = reinterpret_cast<const uint4 *>(recs);
  SealCut cut;
  cut.batch_size = batch_size;
  uint64_t held_first = n;  // the first kept transaction after the last cut
  bool have_held = false;
  if (lane == 0) {
    brank[0] = 0u;
    offsets[0] = 0ull;
  }
  const uint64_t npieces = ((uint64_t)n + 63u) >> 6;
  auto entry = [q, n](uint64_t i) {  // (a load under a branch, not a select of two addresses)
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i < n) v = q[i];
    return v;
  };
  uint4 pf[kSealAhead];
  HSV_UNROLL
  for (int j = 0; j < kSealAhead; ++j) pf[j] = entry((uint64_t)j * 64u + lane);
  for (uint64_t p0 = 0; p0 < npieces; p0 += kSealAhead) {
    uint4 cur[kSealAhead];
    HSV_UNROLL
    for (int j = 0; j < kSealAhead; ++j) cur[j] = pf[j];
    HSV_UNROLL
    for (int j = 0; j < kSealAhead; ++j) pf[j] = entry((p0 + kSealAhead + (uint64_t)j) * 64u + lane);
    HSV_UNROLL
    for (int j = 0; j < kSealAhead; ++j) {
      const uint64_t i = (p0 + (uint64_t)j) * 64u + lane;
      const bool valid = i < n;
      const uint64_t e = ((uint64_t)cur[j].y << 32) | cur[j].x;
      const uint32_t r = cur[j].z;
      for (;;) {  // every turn closes a batch at a later entry: at most 64 turns
        const uint64_t m = __ballot(valid && cut.closes(i, e));
        if (!m) break;
        const int f = __ffsll((unsigned long long)m) - 1;
        const uint64_t ec = seal_readlane64(e, f);
        const uint32_t rc = (uint32_t)__builtin_amdgcn_readlane((int)r, f);
        cut.close((p0 + (uint64_t)j) * 64u + (uint64_t)f, ec, rc);
        have_held = false;
        if (lane == 0 && cut.nb <= bcap) {  // (bcap <= batches_cap)
          brank[cut.nb] = rc;
          offsets[cut.nb] = seal_batch_start(cut.nb, rc, ec);
        }
      }
      if (!have_held) {
        const uint64_t m = __ballot(valid && (uint64_t)r > cut.cut_r);
        if (m) {
          have_held = true;
          held_first = (p0 + (uint64_t)j) * 64u + (uint64_t)(__ffsll((unsigned long long)m) - 1);
        }
      }
    }
  }
  // the totals: the last record's (n == 0: the zeroed head's)
  const uint64_t kept_bytes = head->total.bytes, kept = head->total.kept, malformed = head->total.malformed;
  if (flush && kept > cut.cut_r) {  // the timer branch: a last batch that is not empty
    cut.close(n, kept_bytes, kept);
    have_held = false;
    if (lane == 0 && cut.nb <= bcap) {
      brank[cut.nb] = (uint32_t)kept;
      offsets[cut.nb] = seal_batch_start(cut.nb, kept, kept_bytes);
    }
  }
  const uint64_t sealed = cut.cut_r, bytes = seal_batch_start(cut.nb, cut.cut_r, cut.cut_e);
  const bool overflow = cut.nb > batches_cap || bytes > out_cap;
  // entries past n_batches repeat the end offset
  for (uint64_t b = cut.nb + 1 + lane; b <= batches_cap; b += 64u) offsets[b] = bytes;
  if (lane == 0) {
    head->nb = overflow ? 0u : (uint32_t)cut.nb;
    head->status = overflow ? HSV_SEAL_OVERFLOW : HSV_SEAL_OK;
    head->sealed = overflow ? 0ull : sealed;
    summary[0] = n;
    summary[1] = sealed;
    summary[2] = (uint64_t)n - kept - malformed;
    summary[3] = malformed;
    summary[4] = kept - sealed;
    summary[5] = have_held ? held_first : (uint64_t)n;
    summary[6] = bytes;
    summary[7] = (uint64_t)(uint32_t)cut.nb | ((uint64_t)(overflow ? HSV_SEAL_OVERFLOW : HSV_SEAL_OK) << 32);
  }
}

// the batch of kept rank k: the last b < nb with brank[b] <= k (k < brank[nb])
__device__ __forceinline__ uint32_t seal_find_batch(const uint32_t *__restrict__ brank, uint32_t nb, uint32_t k) {
  uint32_t lo = 0, hi = nb;  // brank[lo] <= k < brank[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (brank[mid] <= k) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What the copy kernels know of a sealed transaction.
struct SealPlace {
  uint64_t src, dst, len;  // byte offsets from the input's and the output's bases
  uint32_t batch, first_of_batch, count;
};
template <int MODE>
__device__ __forceinline__ bool seal_place(const SealInput<MODE> &in, const SealRec *__restrict__ recs,
                                           const uint32_t *__restrict__ brank, const SealHead *__restrict__ head,
                                           uint32_t i, SealPlace &p) {
  const SealRec rec = recs[i];
  if (rec.cls != kSealKept || (uint64_t)rec.r > head->sealed) return false;  // not kept, or held
  uint64_t lo, hi;
  in.span(i, lo, hi);
  const uint32_t k = rec.r - 1u, nb = head->nb;
  const uint32_t b = seal_find_batch(brank, nb, k);
  p.src = lo;
  p.len = hi - lo;
  p.dst = seal_dst(b, k, rec.e - p.len);
  p.batch = b;
  p.first_of_batch = brank[b] == k;
  p.count = brank[b + 1] - brank[b];
  return true;
}

// piece `piece` (bytes [piece * kSealPiece, ...)) of the transaction at p, by
// `lanes` lanes of which the caller is number `l`
__device__ __forceinline__ void seal_copy_piece(const uint8_t *__restrict__ in_base, uint8_t *__restrict__ out_base,
                                                const SealPlace &p, uint64_t piece, uint32_t l, uint32_t lanes) {
  const uint64_t at = piece * kSealPiece;
  if (at >= p.len) return;
  const uint32_t imis = (uint32_t)(reinterpret_cast<uintptr_t>(in_base) & 15u);
  const uint32_t omis = (uint32_t)(reinterpret_cast<uintptr_t>(out_base) & 15u);
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(__builtin_assume_aligned(in_base - imis, 16));
  ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(__builtin_assume_aligned(out_base - omis, 16));
  uint8_t *dst1 = out_base - omis;
  SealCopy cp;
  cp.spos = imis + p.src + at;
  cp.dpos = omis + p.dst + at;
  cp.len = min(p.len - at, kSealPiece);
  const uint64_t nc = cp.chunks();
  for (uint64_t c = l; c < nc; c += lanes)
    cp.chunk(
        c,
        [src](uint64_t k) {
          const ulonglong2 v = src[k];
          return SealChunk{v.x, v.y};
        },
        [dst](uint64_t k, SealChunk v) { dst[k] = make_ulonglong2(v.lo, v.hi); },
        [dst1](uint64_t pos, uint8_t byte) { dst1[pos] = byte; });
}

template <int MODE>
__global__ void __launch_bounds__(kSealBlock)
hsv_seal_copy_kernel(SealInput<MODE> in, uint32_t n, const SealRec *__restrict__ recs,
                     const uint32_t *__restrict__ brank, const SealHead *__restrict__ head,
                     uint8_t *__restrict__ out) {
  if (head->status != HSV_SEAL_OK) return;
  const uint64_t t = (uint64_t)blockIdx.x * kSealBlock + threadIdx.x;
  const uint64_t i = t / kSealGroup;
  const uint32_t l = (uint32_t)(t % kSealGroup);
  if (i >= n) return;
  SealPlace p;
  if (!seal_place(in, recs, brank, head, (uint32_t)i, p)) return;
  // the length prefix, and the header before a batch's first transaction:
  // lanes 0..7 and 8..15 (twice) write a byte each
  if (l < 8u) {
    out[p.dst - 8u + l] = (uint8_t)(p.len >> (8u * l));
  } else if (p.first_of_batch) {
    const uint32_t j = l - 8u;  // count byte j
    out[p.dst - 16u + j] = (uint8_t)((uint64_t)p.count >> (8u * j));
    if (j < 4u) out[p.dst - 20u + j] = 0;  // the variant tag
  }
  seal_copy_piece(in.base, out, p, 0, l, kSealGroup);
}

// the pieces beyond the first: piece x of the call belongs to the first
// transaction i with xincl[i] > x
template <int MODE>
__global__ void __launch_bounds__(64)
hsv_seal_pieces_kernel(SealInput<MODE> in, uint32_t n, const SealRec *__restrict__ recs,
                       const uint32_t *__restrict__ xincl, const uint32_t *__restrict__ brank,
                       const SealHead *__restrict__ head, uint8_t *__restrict__ out) {
  if (head->status != HSV_SEAL_OK) return;
  const uint32_t total = head->total.extra;
  for (uint32_t x = blockIdx.x; x < total; x += gridDim.x) {
    uint32_t lo = 0, hi = n - 1u;  // the answer lies in [lo, hi]: xincl[n - 1] = total > x
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (xincl[mid] > x) hi = mid;
      else lo = mid + 1u;
    }
    const uint32_t before = lo ? xincl[lo - 1u] : 0u;
    SealPlace p;
    if (seal_place(in, recs, brank, head, lo, p)) seal_copy_piece(in.base, out, p, (uint64_t)(x - before) + 1u, threadIdx.x, 64u);
  }
}

// ---- the batches' digests ----------------------------------------------------------
constexpr uint32_t kDigestWindow = 1024;                        // message bytes per window: 8 blocks
constexpr uint32_t kDigestWords = (kDigestWindow + 16) / 4 + 4;  // 65 chunks and a word of slack

// One wave per batch: SHA-512(out[offsets[b], offsets[b+1]))[..32] to digests + 32 b.
// The padded message is read as stream bytes from the 16-byte chunk that holds
// its first byte (stream byte s is message byte s - mis); window w holds the 65
// chunks from 64 w on, that is message bytes [1024 w, 1024 w + 1024) at LDS
// byte mis + ...; the padding is written into LDS over whatever the chunks
// held there.  Every lane runs the same compression on the same LDS words.
__global__ void __launch_bounds__(64)
hsv_seal_digest_kernel(const uint8_t *__restrict__ out, const unsigned long long *__restrict__ offsets,
                       const SealHead *__restrict__ head, uint8_t *__restrict__ digests) {
  __shared__ uint32_t win[kDigestWords];
  if (head->status != HSV_SEAL_OK) return;
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  if (b >= head->nb) return;
  const uint64_t lo = offsets[b], len = offsets[b + 1] - lo;
  const uint8_t *msg = out + lo;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(msg) & 15u);
  const uint4 *q = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(msg - mis, 16));
  const uint64_t padded = (len + 17u + 127u) / 128u * 128u;
  const uint64_t nchunks = (mis + len + 15u) >> 4;  // chunks that hold a message byte
  const uint64_t nwin = (padded + kDigestWindow - 1u) / kDigestWindow;
  // (a load under a branch, not a select of two values: the compiler turns the
  // select into a select of two addresses, one of them a zero in scratch)
  auto chunk = [q, nchunks](uint64_t c) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c < nchunks) v = q[c];
    return v;
  };
  uint64_t h[8];
  sha512_init(h);
  uint4 pf = chunk(lane);
  uint4 pfx = chunk(64u);
  if (lane < 4u) win[kDigestWords - 4u + lane] = 0u;
  for (uint64_t w = 0; w < nwin; ++w) {
    reinterpret_cast<uint4 *>(win)[lane] = pf;
    if (lane == 0) reinterpret_cast<uint4 *>(win)[64] = pfx;
    {
      pf = chunk((w + 1u) * 64u + lane);
      pfx = chunk((w + 2u) * 64u);
    }
    __builtin_amdgcn_wave_barrier();
    // the padding bytes that lie in this window's 1040 stream bytes
    const uint64_t wlo = w * kDigestWindow;  // stream position of the window's first byte
    for (uint64_t s = mis + len + lane; s < mis + padded; s += 64u) {
      if (s >= wlo && s < wlo + kDigestWindow + 16u) {
        const uint64_t m = s - mis;  // position in the padded message
        uint8_t v = m == len ? 0x80 : 0;
        if (m >= padded - 8u) v = (uint8_t)((len * 8u) >> (8u * (padded - 1u - m)));
        reinterpret_cast<uint8_t *>(win)[s - wlo] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t nblocks = (uint32_t)min((uint64_t)(kDigestWindow / 128u), (padded - wlo) / 128u);
    HSV_NOUNROLL
    for (uint32_t k = 0; k < nblocks; ++k) {
      const uint32_t at = mis + 128u * k, wi = at >> 2, sh = (at & 3u) * 8u;
      uint64_t ww[16];
      uint32_t prev = win[wi];
      HSV_UNROLL
      for (int j = 0; j < 16; ++j) {
        const uint32_t a = win[wi + 2 * j + 1], c = win[wi + 2 * j + 2];
        const uint32_t w0 = (uint32_t)((((uint64_t)a << 32) | prev) >> sh);
        const uint32_t w1 = (uint32_t)((((uint64_t)c << 32) | a) >> sh);
        ww[j] = be64_from_le32(w0, w1);
        prev = c;
      }
      sha512_compress(h, ww);
    }
    __builtin_amdgcn_wave_barrier();  // every lane has read before the next window lands
  }
  if (lane < 32u) {
    const uint32_t wsel = lane >> 3;
    const uint64_t hw = wsel == 0 ? h[0] : wsel == 1 ? h[1] : wsel == 2 ? h[2] : h[3];
    digests[32ull * b + lane] = (uint8_t)(hw >> (56u - 8u * (lane & 7u)));
  }
}

namespace {

template <int MODE>
hipError_t launch_seal(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n, const uint8_t *flags,
                       uint64_t batch_size, int flush, uint8_t *out, uint64_t out_cap, uint64_t *batch_offsets,
                       uint64_t batches_cap, uint8_t *digests, void *summary, hipEvent_t *marks, hipStream_t stream) {
  const uint32_t nblk = (uint32_t)(((uint64_t)n + kSealBlock - 1) / kSealBlock);
  const uint32_t bcap = (uint32_t)(batches_cap < n ? batches_cap : n);
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t off_sums = kSealHeadBytes, off_recs = off_sums + up((size_t)nblk * sizeof(SealSums));
  const size_t off_x = off_recs + up((size_t)n * sizeof(SealRec)), off_rank = off_x + up((size_t)n * 4);
  const size_t bytes = off_rank + up(((size_t)bcap + 1) * 4);
  Workspace ws(nullptr, 0, bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *p = ws.get();
  SealHead *head = reinterpret_cast<SealHead *>(p);
  SealSums *sums = reinterpret_cast<SealSums *>(p + off_sums);
  SealRec *recs = reinterpret_cast<SealRec *>(p + off_recs);
  uint32_t *xincl = reinterpret_cast<uint32_t *>(p + off_x);
  uint32_t *brank = reinterpret_cast<uint32_t *>(p + off_rank);
  const SealInput<MODE> input{txs, offsets, tx_size, flags};
  auto mark = [&](int k, hipError_t e) { return e == hipSuccess && marks ? hipEventRecord(marks[k], stream) : e; };
  hipError_t e = hipMemsetAsync(p, 0, kSealHeadBytes, stream);
  e = mark(0, e);
  if (e == hipSuccess && n) {
    hipLaunchKernelGGL(hsv_seal_reduce_kernel<MODE>, dim3(nblk), dim3(kSealBlock), 0, stream, input, n, sums);
    hipLaunchKernelGGL(hsv_seal_blocks_kernel, dim3(1), dim3(kSealBlock), 0, stream, sums, nblk, head);
    hipLaunchKernelGGL(hsv_seal_apply_kernel<MODE>, dim3(nblk), dim3(kSealBlock), 0, stream, input, n, sums, recs,
                       xincl);
    e = hipGetLastError();
  }
  e = mark(1, e);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hsv_seal_cut_kernel, dim3(1), dim3(64), 0, stream, recs, n, batch_size, flush ? 1u : 0u,
                       out_cap, batches_cap, bcap, head, brank, reinterpret_cast<unsigned long long *>(batch_offsets),
                       static_cast<unsigned long long *>(summary));
    e = hipGetLastError();
  }
  e = mark(2, e);
  if (e == hipSuccess && n) {
    const uint64_t lanes = (uint64_t)n * kSealGroup;
    hipLaunchKernelGGL(hsv_seal_copy_kernel<MODE>, dim3((uint32_t)((lanes + kSealBlock - 1) / kSealBlock)),
                       dim3(kSealBlock), 0, stream, input, n, recs, brank, head, out);
    hipLaunchKernelGGL(hsv_seal_pieces_kernel<MODE>, dim3(kSealPieceGrid), dim3(64), 0, stream, input, n, recs, xincl,
                       brank, head, out);
    e = hipGetLastError();
  }
  e = mark(3, e);
  if (e == hipSuccess && digests && bcap) {
    hipLaunchKernelGGL(hsv_seal_digest_kernel, dim3(bcap), dim3(64), 0, stream, out,
                       reinterpret_cast<const unsigned long long *>(batch_offsets), head, digests);
    e = hipGetLastError();
  }
  e = mark(4, e);
  return ws.done(e);
}

}  // namespace
}  // namespace hsv

static_assert(sizeof(hsv_seal_summary) == 64, "eight 8-byte words, as the cut kernel writes them");

// One seal of n transactions on `stream` (hsv_internal.h).
extern "C" hipError_t hsv_launch_seal(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                                      const uint8_t *flags, uint64_t batch_size, int flush, uint8_t *out,
                                      uint64_t out_cap, uint64_t *batch_offsets, uint64_t batches_cap, uint8_t *digests,
                                      void *summary, hipEvent_t *marks, hipStream_t stream) {
  if (!batch_size || !batch_offsets || !summary || (n && !txs) || (out_cap && !out)) return hipErrorInvalidValue;
  if (offsets)
    return hsv::launch_seal<hsv::kSealOffsets>(txs, offsets, 0, n, flags, batch_size, flush, out, out_cap,
                                               batch_offsets, batches_cap, digests, summary, marks, stream);
  return hsv::launch_seal<hsv::kSealFixed>(txs, nullptr, tx_size, n, flags, batch_size, flush, out, out_cap,
                                           batch_offsets, batches_cap, digests, summary, marks, stream);
}
