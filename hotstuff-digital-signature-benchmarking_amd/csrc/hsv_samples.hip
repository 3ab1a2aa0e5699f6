// The kernels of hsv_batches_samples_bincode_device and hsv_client_bursts_device
// (include/hsv.h): the benchmark's sample transactions at both ends of the
// device pipeline.
//
// The sample index of n_batches serialized MempoolMessage::Batch messages: what
// the `benchmark` block of BatchMaker::seal logs (mempool/src/batch_maker.rs:
// 118-125, 133-153), per batch the ids of its sample transactions and its size.
// The parse is hsv_launch_batch_scan's (hsv_batchwire.hip): status, count and
// first per batch and the span table, over a table the launcher zeroed, so an
// entry no batch writes reads as an empty span.  Then, each launch after the
// one before has ended and no workgroup ever waiting for another:
//   1. hsv_samples_reduce_kernel   one lane per span: is it a sample (longer
//      than 8 bytes, first byte 0); a workgroup's count.
//   2. hsv_samples_blocks_kernel   one workgroup: the exclusive scan of the
//      workgroups' counts.
//   3. hsv_samples_apply_kernel    the same lanes again: the scan inside the
//      workgroup plus its base is the span's position among the call's
//      samples, kept in pos[0 .. tx_cap]; a sample below ids_cap writes its id,
//      bytes 1..9 big-endian, there.  Positions follow the transaction
//      numbering, which is in batch order, so the ids are too.
//   4. hsv_samples_batches_kernel  one lane per batch: first_sample and
//      n_samples from pos at first[b] and first[b] + count[b], the size from
//      the batch's length and count.
// The bytes are read in passes 1 and 3; should they change in between, the ids
// may be any of the two readings', but every store stays below ids_cap.
//
// hsv_client_bursts_kernel writes the client's transactions (node/src/
// client.rs:121-135): sixteen lanes per transaction, the preamble and the zero
// padding as destination-aligned 16-byte stores with byte stores at the ragged
// ends, nothing outside [0, tx_size - trailer) of a transaction.
//
// Stores are plain vector stores; no kernel here uses scratch.
#include <hip/hip_runtime.h>

#include "hsv.h"
#include "hsv_internal.h"
#include "hsv_batchscan.hpp"
#include "hsv_field.hpp"
#include "hsv_samples.hpp"

namespace hsv {

constexpr int kSamplesBlock = 256;
static_assert(kSamplesBlock == (int)kSamplesTile, "one lane per transaction of a tile");
static_assert(kSamplesBlock % (int)kClientGroup == 0, "whole lane groups per workgroup");

__device__ __forceinline__ uint32_t samples_shfl_up(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d); }
__device__ __forceinline__ uint64_t samples_shfl_up(uint64_t v, int d) {
  return (uint64_t)__shfl_up((unsigned long long)v, d);
}
// inclusive scan over the workgroup's kSamplesBlock lanes (T: uint32_t inside a
// tile, uint64_t over the tiles' counts); part: 4 entries of LDS
template <class T>
__device__ __forceinline__ T samples_block_scan(T v, T *part, T &block_total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  HSV_UNROLL
  for (int d = 1; d < 64; d <<= 1) {
    const T u = samples_shfl_up(v, d);
    if (lane >= (uint32_t)d) v += u;
  }
  if (lane == 63u) part[wave] = v;
  __syncthreads();
  T before = 0, all = 0;
  HSV_UNROLL
  for (uint32_t w = 0; w < kSamplesBlock / 64; ++w) {
    const T p = part[w];
    if (w < wave) before += p;
    all += p;
  }
  block_total = all;
  return before + v;
}

// 1 when span i (i < ntx) is a sample; lo: where it begins
__device__ __forceinline__ uint32_t samples_item(const uint8_t *__restrict__ bufs, const ulonglong2 *__restrict__ spans,
                                                 uint64_t ntx, uint64_t &lo) {
  const uint64_t i = (uint64_t)blockIdx.x * kSamplesBlock + threadIdx.x;
  lo = 0;
  if (i >= ntx) return 0u;
  const ulonglong2 s = spans[i];
  if (s.y < s.x || s.y - s.x <= 8u) return 0u;  // (every sample has a first byte)
  lo = s.x;
  return is_sample(s.y - s.x, bufs[s.x]) ? 1u : 0u;
}

__global__ void __launch_bounds__(kSamplesBlock)
hsv_samples_reduce_kernel(const uint8_t *__restrict__ bufs, const ulonglong2 *__restrict__ spans, uint64_t ntx,
                          uint64_t *__restrict__ sums) {
  __shared__ uint32_t part[kSamplesBlock / 64];
  uint64_t lo;
  uint32_t total;
  (void)samples_block_scan(samples_item(bufs, spans, ntx, lo), part, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[b] <- the counts of the workgroups before b.  Each lane takes a run of
// workgroups, as hsv_batch_index_kernel does.
__global__ void __launch_bounds__(kSamplesBlock)
hsv_samples_blocks_kernel(uint64_t *__restrict__ sums, uint32_t nblk) {
  __shared__ uint64_t part[kSamplesBlock / 64];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nblk + kSamplesBlock - 1u) / kSamplesBlock;
  const uint32_t lo = min(t * per, nblk), hi = min(lo + per, nblk);
  uint64_t mine = 0;
  for (uint32_t b = lo; b < hi; ++b) mine += sums[b];
  uint64_t total;
  uint64_t run = samples_block_scan(mine, part, total) - mine;
  for (uint32_t b = lo; b < hi; ++b) {
    const uint64_t s = sums[b];
    sums[b] = run;
    run += s;
  }
}

// pos: ntx + 1 entries, pos[i] = the samples among spans [0, i)
__global__ void __launch_bounds__(kSamplesBlock)
hsv_samples_apply_kernel(const uint8_t *__restrict__ bufs, const ulonglong2 *__restrict__ spans, uint64_t ntx,
                         const uint64_t *__restrict__ sums, uint32_t *__restrict__ pos,
                         unsigned long long *__restrict__ ids, uint64_t ids_cap) {
  __shared__ uint32_t part[kSamplesBlock / 64];
  uint64_t lo;
  uint32_t total;
  const uint32_t flag = samples_item(bufs, spans, ntx, lo);
  const uint32_t incl = samples_block_scan(flag, part, total);
  const uint64_t i = (uint64_t)blockIdx.x * kSamplesBlock + threadIdx.x;
  if (i > ntx) return;
  const uint64_t at = sums[blockIdx.x] + (incl - flag);  // (at most ntx < 2^32)
  pos[i] = (uint32_t)at;
  if (flag && at < ids_cap) {
    uint64_t id = 0;
    HSV_UNROLL
    for (uint32_t k = 1; k <= 8u; ++k) id = (id << 8) | bufs[lo + k];
    ids[at] = id;
  }
}

// index: hsv_batch_samples as five 8-byte words
__global__ void __launch_bounds__(kSamplesBlock)
hsv_samples_batches_kernel(const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ status,
                           const uint64_t *__restrict__ count, const uint64_t *__restrict__ first,
                           const uint32_t *__restrict__ pos, uint32_t nb, uint64_t ntx,
                           unsigned long long *__restrict__ index) {
  const uint64_t b = (uint64_t)blockIdx.x * kSamplesBlock + threadIdx.x;
  if (b >= nb) return;
  const uint32_t st = status[b];
  uint64_t n = 0, size = 0, ns = 0, fs = 0;
  if (st != kBatchParse) {  // kBatchOk or kBatchOverflow: the walk ended at the batch's end
    n = count[b];
    size = offsets[b + 1] - offsets[b] - kBatchHeader - 8u * n;
    const uint64_t f = first[b];
    fs = pos[min(f, ntx)];  // an overflowed batch: where its ids would begin, at most the total
    if (st == kBatchOk) ns = pos[f + n] - fs;  // (f + n <= ntx, the index kernel's condition)
  }
  unsigned long long *w = index + 5u * b;
  w[0] = st;
  w[1] = n;
  w[2] = size;
  w[3] = ns;
  w[4] = fs;
}

// body: tx_size - trailer, at least kClientPreamble
__global__ void __launch_bounds__(kSamplesBlock)
hsv_client_bursts_kernel(uint8_t *__restrict__ txs, uint64_t tx_size, uint64_t body, uint64_t counter0,
                         uint64_t burst, uint64_t r0, uint64_t n) {
  const uint64_t t = (uint64_t)blockIdx.x * kSamplesBlock + threadIdx.x;
  const uint64_t i = t / kClientGroup;
  const uint32_t l = (uint32_t)(t % kClientGroup);
  if (i >= n) return;
  const ClientPreamble p = client_preamble(i, burst, counter0, r0);
  uint8_t *a = txs + i * tx_size;
  // [0, head) bytes up to the first 16-byte boundary, nmid whole chunks, [tail, body) bytes
  const uint32_t to_edge = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(a) & 15u)) & 15u;
  const uint64_t head = min(body, (uint64_t)to_edge);
  const uint64_t nmid = (body - head) >> 4, tail = head + 16u * nmid;
  if (l < head) a[l] = p.byte(l);
  ulonglong2 *mid = reinterpret_cast<ulonglong2 *>(__builtin_assume_aligned(a + to_edge, 16));  // (a + head when nmid > 0)
  for (uint64_t c = l; c < nmid; c += kClientGroup) {
    const uint64_t at = head + 16u * c;
    uint64_t x = 0, y = 0;
    if (at < 16u) p.from((uint32_t)at, x, y);
    mid[c] = make_ulonglong2(x, y);
  }
  if (tail + l < body) a[tail + l] = p.byte(tail + l);
}

}  // namespace hsv

static_assert(sizeof(hsv_batch_samples) == 40, "five 8-byte words, as the batches kernel writes them");
static_assert(HSV_BATCH_OK == hsv::kBatchOk && HSV_BATCH_PARSE == hsv::kBatchParse &&
                  HSV_BATCH_OVERFLOW == hsv::kBatchOverflow,
              "the parse's status words are the index's");

// The sample index of n_batches serialized batches on `stream` (hsv_internal.h).
extern "C" hipError_t hsv_launch_batch_samples(const uint8_t *bufs, const uint64_t *offsets, uint32_t n_batches,
                                               uint64_t tx_cap, void *index, uint64_t *ids, uint64_t ids_cap,
                                               hipStream_t stream) {
  using namespace hsv;
  if (n_batches == 0) return hipSuccess;
  if (!offsets || !index || (ids_cap && !ids) || tx_cap > 0xffffffffull) return hipErrorInvalidValue;
  const uint32_t nblk = (uint32_t)((tx_cap + 1u + kSamplesBlock - 1u) / kSamplesBlock);  // lanes 0 .. tx_cap
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  // status | count | first | spans | workgroup counts | pos
  const size_t off_count = up((size_t)n_batches * 4), off_first = off_count + up((size_t)n_batches * 8);
  const size_t off_spans = off_first + up(((size_t)n_batches + 1) * 8);
  const size_t off_sums = off_spans + up((size_t)tx_cap * 16), off_pos = off_sums + up((size_t)nblk * 8);
  const size_t bytes = off_pos + up(((size_t)tx_cap + 1) * 4);
  Workspace ws(nullptr, 0, bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *p = ws.get();
  uint32_t *status = reinterpret_cast<uint32_t *>(p);
  uint64_t *count = reinterpret_cast<uint64_t *>(p + off_count), *first = reinterpret_cast<uint64_t *>(p + off_first);
  uint64_t *spans = reinterpret_cast<uint64_t *>(p + off_spans), *sums = reinterpret_cast<uint64_t *>(p + off_sums);
  uint32_t *pos = reinterpret_cast<uint32_t *>(p + off_pos);
  hipError_t e = tx_cap ? hipMemsetAsync(spans, 0, (size_t)tx_cap * 16, stream) : hipSuccess;
  if (e == hipSuccess) e = hsv_launch_batch_scan(bufs, offsets, n_batches, tx_cap, status, count, first, spans, stream);
  if (e == hipSuccess) {
    const ulonglong2 *sp = reinterpret_cast<const ulonglong2 *>(spans);
    hipLaunchKernelGGL(hsv_samples_reduce_kernel, dim3(nblk), dim3(kSamplesBlock), 0, stream, bufs, sp, tx_cap, sums);
    hipLaunchKernelGGL(hsv_samples_blocks_kernel, dim3(1), dim3(kSamplesBlock), 0, stream, sums, nblk);
    hipLaunchKernelGGL(hsv_samples_apply_kernel, dim3(nblk), dim3(kSamplesBlock), 0, stream, bufs, sp, tx_cap, sums,
                       pos, reinterpret_cast<unsigned long long *>(ids), ids_cap);
    hipLaunchKernelGGL(hsv_samples_batches_kernel, dim3((n_batches + kSamplesBlock - 1u) / kSamplesBlock),
                       dim3(kSamplesBlock), 0, stream, offsets, status, count, first, pos, n_batches, tx_cap,
                       static_cast<unsigned long long *>(index));
    e = hipGetLastError();
  }
  return ws.done(e);
}

// n client transactions of tx_size bytes at txs on `stream` (hsv_internal.h):
// n * kClientGroup lanes, n <= 2^32 - 1.
extern "C" hipError_t hsv_launch_client_bursts(uint8_t *txs, uint64_t tx_size, uint64_t trailer, uint64_t counter0,
                                               uint64_t burst, uint64_t r0, uint64_t n, hipStream_t stream) {
  using namespace hsv;
  if (n == 0) return hipSuccess;
  if (!txs || !burst || trailer > tx_size || tx_size - trailer < kClientPreamble || n > 0xffffffffull)
    return hipErrorInvalidValue;
  const uint64_t lanes = n * kClientGroup;
  hipLaunchKernelGGL(hsv_client_bursts_kernel, dim3((uint32_t)((lanes + kSamplesBlock - 1) / kSamplesBlock)),
                     dim3(kSamplesBlock), 0, stream, txs, tx_size, tx_size - trailer, counter0, burst, r0, n);
  return hipGetLastError();
}
