// The device-side parse of serialized mempool batches (hsv_batches_verify_bincode_device,
// include/hsv.h): from n_batches bincode MempoolMessage::Batch messages in HBM
// to the span table the transaction kernels address (hsv_mempool.hip, SPANS),
// and from the transactions' flags to one verdict per batch.  No transaction
// byte is copied: the parse writes 16 bytes per transaction, the two ends of
// its span.
//
// A batch's length prefixes form a chain -- the place of each is known only
// once the one before is read -- so a walk straight from HBM would pay one
// memory round trip per transaction.  Here one wave per batch streams the
// batch through LDS in windows of kScanWindow bytes (hsv_batchscan.hpp: each
// lane loads one 16-byte chunk per window), kScanAhead windows side by side
// with the loads of the next kScanAhead already in flight in registers, and
// walks the chain from LDS.  The count is not known before the walk has
// ended, so the walk runs twice: hsv_batch_count_kernel counts and validates,
// hsv_batch_index_kernel numbers the transactions in batch order (first[b] =
// the counts before b, so the numbering does not depend on which wave ran
// when), hsv_batch_spans_kernel writes the pairs.  hsv_batch_reduce_kernel
// turns the flags into verdicts.
//
// Every loop is bounded by the batch's byte length: hsv_batchscan.hpp's walk
// takes at most len / 8 steps and ceil((len + 15) / 1024) windows, whatever the
// bytes say; no wave waits for another.
#include <hip/hip_runtime.h>

#include "hsv.h"
#include "hsv_internal.h"
#include "hsv_batchscan.hpp"
#include "hsv_field.hpp"

namespace hsv {

constexpr int kScanAhead = 16;  // windows per group: 16 KiB per wave in LDS, and as much in flight
constexpr uint32_t kScanWinWords = kScanAhead * (kScanWindow / 4u) + kScanSlackWords;
static_assert(kScanWindow == 64u * 16u, "one 16-byte chunk per lane and window");

// The wave's walk of the batch at `base` (len bytes, any alignment) through
// the LDS windows `win`: the state after its last window.  Every lane runs the
// same walk on the same LDS words; emit is called by every lane.
// The windows come in groups of kScanAhead: a group's chunks are written to
// LDS side by side, the loads of the next group are issued, and only then is
// the group walked, so the loads fly while the chain is followed and the wait
// for them (at the next group's stores, the first use of those registers) is
// for all of them at once.  (With one register window ahead of every LDS write
// instead, the compiler's wait before each write also covered the load issued
// just before it: one memory round trip per window.)
template <class Emit>
__device__ __forceinline__ BatchWalk batch_walk_wave(const uint8_t *base, uint64_t len, uint32_t *win, uint32_t lane,
                                                     Emit &&emit) {
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u);
  // (pointer arithmetic, not an integer round trip: the loads stay global loads, which the LDS reads of the
  // walk do not wait for; a flat load counts against the LDS counter as well)
  const uint4 *q = reinterpret_cast<const uint4 *>(__builtin_assume_aligned(base - mis, 16));
  BatchWalk wk;
  wk.begin(len, mis);
  if (wk.done()) return wk;
  // only chunks that hold a byte of the batch are loaded
  const uint64_t nchunks = (wk.send + 15u) >> 4, nwin = wk.windows();
  uint4 pf[kScanAhead];
  HSV_UNROLL
  for (int j = 0; j < kScanAhead; ++j) {
    const uint64_t c = (uint64_t)j * 64u + lane;
    pf[j] = c < nchunks ? q[c] : make_uint4(0u, 0u, 0u, 0u);
  }
  for (uint64_t w0 = 0; w0 < nwin && !wk.done(); w0 += kScanAhead) {
    HSV_UNROLL
    for (int j = 0; j < kScanAhead; ++j) reinterpret_cast<uint4 *>(win)[j * 64 + lane] = pf[j];
    HSV_UNROLL
    for (int j = 0; j < kScanAhead; ++j) {
      const uint64_t c = (w0 + kScanAhead + (uint64_t)j) * 64u + lane;
      pf[j] = c < nchunks ? q[c] : make_uint4(0u, 0u, 0u, 0u);
    }
    __builtin_amdgcn_wave_barrier();
    HSV_NOUNROLL
    for (uint32_t j = 0; j < (uint32_t)kScanAhead; ++j) {
      const uint64_t w = w0 + j;
      if (w >= nwin || wk.done()) break;
      // (a read that runs past window j reads window j + 1 or the slack words; the walk masks it off)
      wk.window(win + j * (kScanWindow / 4u), w, emit);
    }
    __builtin_amdgcn_wave_barrier();  // every lane has read before the next group lands
  }
  return wk;
}

// First walk: status[b] = kBatchOk / kBatchParse, count[b] = its transactions
// (0 for a malformed batch).  One wave per batch.
__global__ void __launch_bounds__(64) hsv_batch_count_kernel(const uint8_t *__restrict__ bufs,
                                                             const uint64_t *__restrict__ offsets, uint32_t nb,
                                                             uint32_t *__restrict__ status,
                                                             uint64_t *__restrict__ count) {
  __shared__ uint32_t win[kScanWinWords];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  if (b >= nb) return;
  const uint64_t lo = offsets[b], hi = offsets[b + 1];
  uint32_t st = kBatchParse;
  uint64_t n = 0;
  if (hi >= lo) {  // (decreasing offsets: malformed)
    if (lane < kScanSlackWords) win[kScanWinWords - kScanSlackWords + lane] = 0u;
    const BatchWalk wk = batch_walk_wave(bufs + lo, hi - lo, win, lane, [](uint64_t, uint64_t, uint64_t) {});
    if (wk.ok()) {
      st = kBatchOk;
      n = wk.count;
    }
  }
  if (lane == 0) {
    status[b] = st;
    count[b] = n;
  }
}

// first[b] = count[0] + ... + count[b-1], first[nb] = the total; a batch that
// does not fit below tx_cap becomes kBatchOverflow.  One block.
constexpr int kIndexBlock = 256;
__global__ void __launch_bounds__(kIndexBlock) hsv_batch_index_kernel(uint32_t *__restrict__ status,
                                                                      const uint64_t *__restrict__ count, uint32_t nb,
                                                                      uint64_t tx_cap, uint64_t *__restrict__ first) {
  __shared__ uint64_t part[kIndexBlock];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nb + kIndexBlock - 1u) / kIndexBlock;
  const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
  uint64_t sum = 0;
  for (uint32_t b = lo; b < hi; ++b) sum += count[b];
  part[t] = sum;
  __syncthreads();
  uint64_t run = 0;
  for (uint32_t k = 0; k < t; ++k) run += part[k];
  if (t == kIndexBlock - 1) first[nb] = run + sum;
  for (uint32_t b = lo; b < hi; ++b) {
    const uint64_t n = count[b];
    first[b] = run;
    if (status[b] == kBatchOk && (run > tx_cap || n > tx_cap - run)) status[b] = kBatchOverflow;
    run += n;
  }
}

// Second walk, kBatchOk batches only: transaction i of batch b is
// bufs[spans[2 (first[b] + i)], spans[2 (first[b] + i) + 1]).  The index
// kernel left the batch kBatchOk only if first[b] + count[b] <= tx_cap, and no
// pair is written past count[b], so every store lies inside the table even if
// the bytes changed since the first walk.
__global__ void __launch_bounds__(64) hsv_batch_spans_kernel(const uint8_t *__restrict__ bufs,
                                                             const uint64_t *__restrict__ offsets, uint32_t nb,
                                                             const uint32_t *__restrict__ status,
                                                             const uint64_t *__restrict__ count,
                                                             const uint64_t *__restrict__ first,
                                                             ulonglong2 *__restrict__ spans) {
  __shared__ uint32_t win[kScanWinWords];
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  if (b >= nb || status[b] != kBatchOk) return;
  const uint64_t lo = offsets[b], hi = offsets[b + 1], n = count[b], f = first[b];
  if (hi < lo || n == 0) return;
  if (lane < kScanSlackWords) win[kScanWinWords - kScanSlackWords + lane] = 0u;
  (void)batch_walk_wave(bufs + lo, hi - lo, win, lane, [&](uint64_t i, uint64_t a, uint64_t e) {
    if (lane == 0 && i < n) spans[f + i] = make_ulonglong2(lo + a, lo + e);
  });
}

// results[b] from the batch's status and the flags of its transactions: the
// lowest index whose flags lack HSV_STRICT_OK makes it kBatchTx.  One wave per
// batch.
__global__ void __launch_bounds__(64) hsv_batch_reduce_kernel(const uint32_t *__restrict__ status,
                                                              const uint64_t *__restrict__ count,
                                                              const uint64_t *__restrict__ first,
                                                              const uint8_t *__restrict__ flags, uint32_t nb,
                                                              hsv_batch_result *__restrict__ results) {
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  if (b >= nb) return;
  uint32_t st = status[b];
  const uint64_t n = st == kBatchParse ? 0 : count[b], f = first[b];
  uint64_t idx = 0;
  if (st == kBatchOk) {
    for (uint64_t base = 0; base < n; base += 64u) {
      const uint64_t i = base + lane;
      const bool bad = i < n && !(flags[f + i] & HSV_STRICT_OK);
      const uint64_t m = __ballot(bad);
      if (m) {
        st = kBatchTx;
        idx = base + (uint64_t)__builtin_ctzll(m);
        break;
      }
    }
  }
  if (lane == 0) {
    hsv_batch_result r;
    r.status = st;
    r.index = (uint32_t)idx;
    r.n_tx = n;
    r.first = f;
    results[b] = r;
  }
}

}  // namespace hsv

extern "C" hipError_t hsv_launch_batch_scan(const uint8_t *bufs, const uint64_t *offsets, uint32_t n_batches,
                                            uint64_t tx_cap, uint32_t *status, uint64_t *count, uint64_t *first,
                                            uint64_t *spans, hipStream_t stream) {
  if (n_batches == 0) return hipSuccess;
  if (!offsets || !status || !count || !first || (tx_cap && !spans) || (reinterpret_cast<uintptr_t>(spans) & 15u))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hsv::hsv_batch_count_kernel, dim3(n_batches), dim3(64), 0, stream, bufs, offsets, n_batches,
                     status, count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hsv::hsv_batch_index_kernel, dim3(1), dim3(hsv::kIndexBlock), 0, stream, status, count, n_batches,
                     tx_cap, first);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hsv::hsv_batch_spans_kernel, dim3(n_batches), dim3(64), 0, stream, bufs, offsets, n_batches,
                     status, count, first, reinterpret_cast<ulonglong2 *>(spans));
  return hipGetLastError();
}

extern "C" hipError_t hsv_launch_batch_reduce(const uint32_t *status, const uint64_t *count, const uint64_t *first,
                                              const uint8_t *flags, uint32_t n_batches, void *results,
                                              hipStream_t stream) {
  if (n_batches == 0) return hipSuccess;
  if (!status || !count || !first || !results) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hsv::hsv_batch_reduce_kernel, dim3(n_batches), dim3(64), 0, stream, status, count, first, flags,
                     n_batches, static_cast<hsv_batch_result *>(results));
  return hipGetLastError();
}
