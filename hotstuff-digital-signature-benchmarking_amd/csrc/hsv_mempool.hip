// Mempool transaction verification kernels.
//
// Reference: the client-transaction check in mempool/src/batch_maker.rs:79-85
// (and the batch re-check in consensus/src/core.rs:121-127):
//     message = tx[..len-96], pk = tx[len-96..len-64], sig = tx[len-64..]
//     digest  = Digest(SHA-512(message)[..32])
//     Signature::from_bytes(sig[..32], sig[32..64]).verify(&digest, &PublicKey(pk))
//
// The record work (tx_record_lane, one lane per transaction, loads staged
// through LDS by the whole wave) hashes the message and writes the 128-byte
// record pk || R || s || digest, then runs the point pass's prepass on it.
// Above 2^13 transactions it is phase 1 of ONE fused launch whose waves then
// take the point batches (hsv_verify_tx_fused_kernel, below); otherwise, and
// with HSV_TX_FUSED=0, the record kernel is followed by the generic
// verification launch over the records (strides 128, the same kernels and
// flags as hsv_verify_device).  The record work is a small fraction of a
// verification: a 512-byte transaction is 4 SHA-512 blocks (about 4 x 80
// rounds) against ~2,300 field operations for the signature.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

// The message hash in this file runs gfx950's v_bitop3_b32 for the sigma XOR
// triples, the majority and the choice (hsv_sha512.hpp): with the bitop3
// results kept as opaque 64-bit pairs that is 754 instead of 991 instructions
// per 16 rounds, and the record kernel went from 0.99 to 0.82 ms per 2^20
// transactions together with the full-block fast path below
// (profiles/r06/r06k_*).  The latency kernels keep the XOR form (their lone
// waves measured no faster with it).
#define HSV_SHA_BITOP3 1
#include "hsv_internal.h"
#include "hsv_keytab.hpp"
#include "hsv_stage.hpp"
#include "hsv_txhash.hpp"
#include "hsv_verify_hc.hpp"
#include "hsv_pointpass.hpp"
#include "hsv_routed.hpp"

namespace hsv {

constexpr int kTxBlock = 256;

// Transaction i spans [lo, hi) bytes of txs: offsets[i], offsets[i+1] when
// offsets is given, else i*tx_size, (i+1)*tx_size.  A transaction shorter
// than 96 bytes (the reference's slice would panic) gets an all-zero record
// here and flags 0 from hsv_tx_mask_kernel.
// SPANS (the serialized batches of hsv_batches_verify_bincode*, whose
// transactions are separated by length prefixes and batch headers): offsets
// is a span table, transaction i is [offsets[2i], offsets[2i+1]).
template <bool SPANS = false>
__device__ __forceinline__ bool tx_span(const uint64_t *offsets, uint64_t tx_size, uint32_t i, uint64_t &lo,
                                        uint64_t &hi) {
  if constexpr (SPANS) {
    lo = offsets[2ull * i];
    hi = offsets[2ull * i + 1];
  } else if (offsets) {
    lo = offsets[i];
    hi = offsets[i + 1];
  } else {
    lo = (uint64_t)i * tx_size;
    hi = lo + tx_size;
  }
  return hi >= lo && hi - lo >= 96;
}

constexpr int kTxWaves = kTxBlock / 64;
constexpr int kTxQ = 9;                   // 16-B chunks under a 128-B window at any offset
// (kNoChunk, shfl_u64 and tx_stage_chunks, the wave's staged loads: hsv_stage.hpp)

// Stores of a record batch.  Plain for the record kernels (the point pass is
// a later launch); write-through (sc1) for the fused launch below, where
// other workgroups of the same launch read them: 16-B buffer stores for the
// 128-B records, 4-B agent-scope relaxed stores for the prepass words and the
// fallback list (MI355X_MICROARCH.md, inter-workgroup visibility: sc1
// payload, a drained wave, then one flag).
typedef __attribute__((address_space(1))) uint32_t gu32;
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));

struct TxRecPlain {
  uint4 *rec;
  __device__ __forceinline__ void put(uint32_t i, int j, const uint32_t r[32]) const {
    rec[(size_t)i * 8 + j] = make_uint4(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
  }
};
struct TxRecWriteThrough {
  __amdgpu_buffer_rsrc_t rsrc;  // the records, n * 128 bytes (< 2^32: hsv_launch_tx_fused)
  __device__ __forceinline__ void put(uint32_t i, int j, const uint32_t r[32]) const {
    const v4u32 v = {r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]};
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)(i * 128u + 16u * (uint32_t)j), 0, 16 /* sc1 */);
  }
};
struct PutWriteThrough {
  static __device__ __forceinline__ void u32(uint32_t *p, uint32_t v) {
    __hip_atomic_store((gu32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// The record words of transaction i (i < n, or past n: nothing is loaded):
// r = pk || R || s || SHA-512(message)[..32], all zero for a transaction
// shorter than 96 bytes or with decreasing offsets; returns whether it is
// well-formed.  Every lane of the wave calls this: the wave's loads are
// cooperative (tx_stage_chunks), each lane loops over its own blocks, the wave
// over its longest message.
template <bool SPANS = false>
__device__ __forceinline__ bool tx_record_words(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ offsets,
                                                uint64_t tx_size, uint32_t n, uint32_t i, uint32_t lane,
                                                uint4 *stage, uint32_t r[32]) {
  uint64_t lo = 0, hi = 0;
  const bool ok = i < n && tx_span<SPANS>(offsets, tx_size, i, lo, hi);
  const uintptr_t base = reinterpret_cast<uintptr_t>(txs);
  const uint4 *q = reinterpret_cast<const uint4 *>(base & ~uintptr_t(15));
  const uint64_t start = (uint64_t)(base & 15u) + lo;
  const uint64_t mlen = ok ? hi - lo - 96 : 0;
  const uint64_t q_last = ok ? (start + (hi - lo) - 1) >> 4 : kNoChunk;
  // SHA-512 of the message, block by block
  uint64_t h[8];
  sha512_init(h);
  const uint64_t nblocks = tx_num_blocks(mlen);
  uint32_t wave_blocks = (uint32_t)nblocks;
  HSV_UNROLL
  for (int m = 1; m < 64; m <<= 1) wave_blocks = max(wave_blocks, (uint32_t)__shfl_xor((int)wave_blocks, m, 64));
  const uint32_t sh16 = (uint32_t)(start & 15u);
  // wave-uniform fast paths: every transaction of the wave starts on a 16-byte
  // boundary (no realignment), and block b lies wholly inside every message
  // (no padding selects) -- the common case of equal-sized transactions
  const bool wave_aligned = __all(sh16 == 0u);
  HSV_NOUNROLL
  for (uint32_t b = 0; b < wave_blocks; ++b) {
    uint32_t raw[4 * kTxQ + 1];
    tx_stage_chunks<kTxQ>(q, stage, lane, (start >> 4) + 8ull * b, q_last, raw);
    const bool wave_full = __all((uint64_t)(b + 1u) * 128u <= mlen);
    if (b < nblocks) {
      uint32_t words[32];
      if (wave_aligned) {
        HSV_UNROLL
        for (int j = 0; j < 32; ++j) words[j] = raw[j];
      } else {
        tx_realign<32>(raw, sh16, words);
      }
      if (wave_full) tx_compress_full_block(h, words);
      else tx_compress_block(h, words, mlen, b, nblocks);
    }
  }
  // pk || R || s: the last 96 bytes (7 chunks at any offset), staged after
  // the hash so that its 24 words are not live across the message loop
  {
    const uint64_t tail = start + mlen;
    uint32_t raw[4 * 7 + 1];
    tx_stage_chunks<7>(q, stage, lane, tail >> 4, q_last, raw);
    tx_realign<24>(raw, (uint32_t)(tail & 15u), r);
  }
  tx_digest_words(h, r + 24);
  if (!ok) {
    HSV_UNROLL
    for (int j = 0; j < 32; ++j) r[j] = 0u;
  }
  return ok;
}

// One lane per transaction i of its wave (tx_record_words; every lane of the
// wave calls this, lanes past n load nothing and store nothing).  PREP: the
// same lane then runs the scalar prepass of the point pass on the record it
// holds in registers (SHA-512(R || A || digest), k mod l, lattice reduction,
// recoding; prep_scalars, hsv_verify_hc.hpp) and writes its SoA record, so a
// transaction's bytes are read once and no separate prepass reads the records
// back (round-2 VERDICT item 8).
// CLAMP (the fused launch's work loop): a lane past n redoes transaction
// n - 1 and stores the same bytes again, so no store sits in a lane-dependent
// region -- nested conditional stores inside the loop made hipcc compile the
// loop's back edge divergent (the round-1 hang pattern, tests/test_kernel_isa.py).
template <bool PREP, bool CLAMP, class Rec, class Put, bool SPANS = false>
__device__ __forceinline__ void tx_record_lane(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ offsets,
                                               uint64_t tx_size, uint32_t n, uint32_t i_in, uint32_t lane,
                                               uint4 *stage, const Rec &out, uint32_t *__restrict__ prep,
                                               uint32_t *__restrict__ fb_count, uint32_t *__restrict__ fb_list,
                                               int lat_bits) {
  const uint32_t i = CLAMP && i_in >= n ? n - 1u : i_in;
  uint32_t r[32];
  (void)tx_record_words<SPANS>(txs, offsets, tx_size, n, i, lane, stage, r);
  if (CLAMP || i < n) {
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) out.put(i, j, r);
    if constexpr (PREP) {
      // pk = r[0..8), R || s = r[8..24), digest = r[24..32)
      const bool fallback = prep_scalars<4, Put, pointpass_digit_bits<4>()>(r, r + 8, r + 24, prep + i, n, lat_bits);
      if (fallback && i == i_in) Put::u32(fb_list + atomicAdd(fb_count, 1u), i);  // once per transaction
    }
  }
}

// The record kernels: one lane per transaction (PREP: with the prepass; the
// point pass is the next launch on the stream).  SPANS: tx_span's span table.
template <bool PREP, bool SPANS = false>
__global__ void __launch_bounds__(kTxBlock) hsv_tx_record_kernel(const uint8_t *__restrict__ txs,
                                                                  const uint64_t *__restrict__ offsets,
                                                                  uint64_t tx_size, uint32_t n,
                                                                  uint4 *__restrict__ rec,
                                                                  uint32_t *__restrict__ prep,
                                                                  uint32_t *__restrict__ fb_count,
                                                                  uint32_t *__restrict__ fb_list, int lat_bits) {
  __shared__ uint4 stage_all[kTxWaves][64 * kTxQ];
  if constexpr (PREP) __builtin_amdgcn_s_setprio(3);  // as hsv_prep_kernel: ahead of a running point pass
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kTxBlock + wv * 64u >= n) return;  // whole wave past the end
  tx_record_lane<PREP, false, TxRecPlain, PutPlain, SPANS>(txs, offsets, tx_size, n, blockIdx.x * kTxBlock + threadIdx.x, lane,
                                             stage_all[wv], TxRecPlain{rec}, prep, fb_count, fb_list, lat_bits);
}

// ---- fused transaction launch (round 6) --------------------------------------
// Record batches and point batches in ONE persistent launch, so no kernel
// boundary falls between a batch's message hash and its point pass.  With two
// launches the point pass of step k can start only once the record kernel of
// step k has ended, and that kernel (0.8 ms per 2^20, 2.5x the C4 prepass)
// spends its end in the previous step's grid end: the mempool line ran 6-7 %
// behind the C4 line.  Here each wave
//   1. takes 64-transaction record batches from ctr->rnext until they run out:
//      hash, record, prepass, all stores write-through, then (after its own
//      vmcnt(0) drain) it publishes the batch: ready[batch] += 1 and
//      ctr->rdone += 1, agent-scope relaxed atomics;
//   2. takes point batches from ctr->next: polls ready[batch] (relaxed, one
//      word, s_sleep between polls, bounded), one agent-scope acquire, then
//      the point pass of hsv_verify_hp_kernel's regular range on the records;
//   3. runs the full-length path over the fallback list once every record
//      batch is published (the point pass's fallback-first order needs the
//      whole list up front; at 2^20 with the 138-bit bound the list is empty).
// Every record batch is handed out before any point batch (a wave moves on
// only when rnext has run out) and only to a running wave, so every poll
// ends.  A poll that still times out (0.5 s of the wall clock) is a device
// fault (fault[0]), never a verdict, and the wave waits no more.  Zeroed
// before the launch: ctr, ready.
constexpr uint64_t kTxFusedWaitTicks = 50000000ull;  // 0.5 s of the 100 MHz clock, far beyond any batch

// Wave-uniform bounded poll of one word; true once it reaches `want`.
__device__ __forceinline__ bool tx_wait_word(uint32_t *w, uint32_t want) {
  const uint64_t t0 = wall_clock64();
  for (;;) {
    const uint32_t v = __builtin_amdgcn_readfirstlane(__hip_atomic_load((gu32 *)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (v >= want) return true;
    if (wall_clock64() - t0 > kTxFusedWaitTicks) return false;
    __builtin_amdgcn_s_sleep(8);
  }
}

template <int WA, int WAVES, int CB>
__global__ void __launch_bounds__(kBlock, WAVES)
hsv_verify_tx_fused_kernel(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ offsets, uint64_t tx_size,
                           uint32_t n, uint8_t *__restrict__ records,
                           uint32_t *__restrict__ rec, HcCounters *__restrict__ ctr, uint32_t *__restrict__ fb_list,
                           uint32_t *__restrict__ ready, int lat_bits, uint8_t *__restrict__ flags_out,
                           uint32_t *__restrict__ strict_bits, uint4 *__restrict__ vt_ws,
                           const uint32_t *__restrict__ comb_b, uint32_t *__restrict__ canary, uint32_t nonce,
                           uint32_t inject, uint32_t *__restrict__ fault) {
  static_assert(kBlock == kTxBlock, "one staging slot per wave");
  __shared__ uint4 stage_all[kBlock / 64][64 * kTxQ];
  const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
  PointPassTab<WA> vt{vt_ws + (uint64_t)slot * pointpass_lane_uint4<WA>(), inject};
  const uint32_t lane = threadIdx.x & 63u;
  uint4 *stage = stage_all[threadIdx.x >> 6];
  canary[slot] = nonce;
  uint32_t bad = 0;
  const uint32_t nbatch = (n + 63u) / 64u;
  // the records' descriptor: n * 128 bytes, under 2^32 (hsv_launch_tx_fused)
  const __amdgpu_buffer_rsrc_t rec_rsrc = __builtin_amdgcn_make_buffer_rsrc(records, 0, (int)(n * 128u), 0x00020000);
  // 1. record batches, at the top wave priority (as the record kernel: they
  // run beside the previous launch's last point batches)
  __builtin_amdgcn_s_setprio(3);
  for (;;) {
    uint32_t rb = 0;
    if (lane == 0) rb = atomicAdd(&ctr->rnext, 1u);
    rb = __builtin_amdgcn_readfirstlane(__shfl(rb, 0));
    if (rb >= nbatch) break;
    tx_record_lane<true, true, TxRecWriteThrough, PutWriteThrough>(txs, offsets, tx_size, n, rb * 64u + lane, lane, stage,
                                                             TxRecWriteThrough{rec_rsrc}, rec, &ctr->fb_count,
                                                             fb_list, lat_bits);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's write-through stores have landed
    // lane 0 marks the batch, lane 1 counts it: ONE atomic add in ONE
    // region (two lane-0 operations made the loop's back edge divergent,
    // tests/test_kernel_isa.py)
    if (lane < 2u && !(inject == kInjectNoPublish && rb == 0u))  // (the test hook leaves batch 0 unpublished)
      __hip_atomic_fetch_add((gu32 *)(lane ? &ctr->rdone : ready + rb), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __builtin_amdgcn_s_setprio(0);
  // 2. point batches (hsv_verify_hp_kernel's regular range, records at stride 128)
  const uint32_t words = (n + 31u) / 32u;
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr->next, 64u);
    base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
    if (base >= n) break;
    if (inject == kInjectCanary) canary[slot] = ~nonce;
    if ((bad & 4u) || !tx_wait_word(ready + base / 64u, 1u)) {
      bad |= 5u;  // never published: a device fault, the batch's flags stay 0; the wave waits no more
      continue;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t idx = base + lane;
    const bool valid = idx < n;
    const uint32_t li = valid ? idx : n - 1u;
    uint32_t pkw[8], rw[8];
    {
      const uint4 *p = reinterpret_cast<const uint4 *>(records + (uint64_t)li * 128u);
      const uint4 p0 = p[0], p1 = p[1], r0 = p[2], r1 = p[3];
      pkw[0] = p0.x; pkw[1] = p0.y; pkw[2] = p0.z; pkw[3] = p0.w;
      pkw[4] = p1.x; pkw[5] = p1.y; pkw[6] = p1.z; pkw[7] = p1.w;
      rw[0] = r0.x; rw[1] = r0.y; rw[2] = r0.z; rw[3] = r0.w;
      rw[4] = r1.x; rw[5] = r1.y; rw[6] = r1.z; rw[7] = r1.w;
    }
    const uint32_t meta = rec[18ull * n + li];
    const bool own = valid && !(meta & kPrepFallback);
    const uint32_t f = verify_one_prepped<WA, CB, joint_pointpass<WA>()>(pkw, rw, rec + li, n, meta, comb_b, vt);
    bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
    if (own && flags_out) flags_out[idx] = (uint8_t)f;
    if (strict_bits) {
      const uint64_t mask = __ballot(own && (f & kStrictOk));
      const uint32_t w = base / 32u + lane;
      const uint32_t part = lane ? (uint32_t)(mask >> 32) : (uint32_t)mask;
      if (lane < 2u && w < words && part) atomicOr(&strict_bits[w], part);
    }
  }
  // 3. the fallback list, complete once every record batch is published
  if (!(bad & 4u) && tx_wait_word(&ctr->rdone, nbatch)) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const uint32_t nfb =
        __builtin_amdgcn_readfirstlane(__hip_atomic_load((gu32 *)&ctr->fb_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    for (;;) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&ctr->fb_next, 64u);
      base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
      if (base >= nfb) break;
      const uint32_t j = base + lane;
      const bool valid = j < nfb;
      const uint32_t idx = fb_list[valid ? j : base];
      uint32_t pkw[8], sigw[16], msgw[8];
      load_triple(records, 128, records + 32, 128, records + 96, 128, idx, pkw, sigw, msgw);
      const uint32_t f = verify_one_full_comb<WA, false, CB>(pkw, sigw, msgw, comb_b, vt);
      bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
      if (valid) {  // store_verdict written out: through the call this kernel came out 3 instructions longer
        if (flags_out) flags_out[idx] = (uint8_t)f;
        if (strict_bits && (f & kStrictOk)) atomicOr(&strict_bits[idx >> 5], 1u << (idx & 31u));
      }
    }
  } else {
    bad |= 1u;
  }
  report_faults(fault, bad & 3u);
}

// Zero the flags (and the STRICT_OK bit) of transactions shorter than 96 bytes.
template <bool SPANS>
__global__ void __launch_bounds__(kTxBlock) hsv_tx_mask_kernel(const uint64_t *__restrict__ offsets, uint32_t n,
                                                                uint8_t *flags, uint32_t *strict_bits) {
  const uint32_t i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t lo, hi;
  if (tx_span<SPANS>(offsets, 0, i, lo, hi)) return;
  if (flags) flags[i] = 0;
  if (strict_bits) atomicAnd(strict_bits + (i >> 5), ~(1u << (i & 31u)));
}

// ---- transactions of known signers (hsv_committee_verify_transactions*) ----------
// A batch whose signers are mostly members of a committee: a member's
// transaction is verified against its comb table (verify_one_comb: 64 mixed
// additions and one decompression), any other by the generic point pass.
// Which it is, is decided on the device from the transaction's own pk bytes
// (keytab_find, hsv_keytab.hpp), so a round of at most 2^22 transactions is
// three launches on the caller's stream and no host round trip:
//   1. hsv_ctx_route_kernel    one lane per transaction: hash, record, lookup;
//      members to the hit list as (i, member index), the others to the miss
//      list as i -- those lanes also run the point pass's prepass on the
//      record they hold; a malformed transaction gets flags 0 here;
//   2. hsv_ctx_comb_kernel     persistent, 64 hit-list entries per batch;
//   3. hsv_ctx_generic_kernel  persistent, the fallback list and then the miss
//      list, as hsv_verify_hp_kernel over the records.
// The list lengths are known on the device only; each pass reads them once,
// after the launch that wrote them has ended.  Every hand-off is a kernel
// boundary: no ready words, no polling, nothing a pass could wait for.
// Flags are those of hsv_verify_transactions* bit for bit: verify_one_comb and
// the point pass return the same byte for the same (pk, sig, digest), and a
// hit means the 32 pk bytes equal the member's.
// The passes' and the list compaction's rules: hsv_routed.hpp.
// One lane per transaction, so no loop surrounds the list stores.
template <bool SPANS>
__global__ void __launch_bounds__(kTxBlock)
hsv_ctx_route_kernel(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ offsets, uint64_t tx_size, uint32_t n,
                     uint4 *__restrict__ rec, const uint32_t *__restrict__ keytab, uint32_t keymask, uint64_t seed,
                     const uint8_t *__restrict__ pks, uint32_t nkeys, RoutedCounters *__restrict__ ctr,
                     uint2 *__restrict__ hit_list, uint32_t *__restrict__ miss_list, uint32_t *__restrict__ prep,
                     uint32_t *__restrict__ fb_list, int lat_bits, uint8_t *__restrict__ flags_out) {
  __shared__ uint4 stage_all[kTxWaves][64 * kTxQ];
  __builtin_amdgcn_s_setprio(3);  // as the record kernel: ahead of an earlier call's running passes
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kTxBlock + wv * 64u >= n) return;  // whole wave past the end
  const uint32_t i = blockIdx.x * kTxBlock + threadIdx.x;
  uint32_t r[32];
  const bool ok = tx_record_words<SPANS>(txs, offsets, tx_size, n, i, lane, stage_all[wv], r);
  if (i < n) {
    const TxRecPlain out{rec};
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) out.put(i, j, r);
    if (!ok && flags_out) flags_out[i] = 0;  // on neither list (its strict bit: zeroed by the host)
  }
  uint32_t kidx = kKeytabMiss;
  if (ok && nkeys) kidx = keytab_find(keytab, keymask, seed, pks, r);
  const bool hit = ok && kidx < nkeys, miss = ok && !hit;
  const uint64_t hm = __ballot(hit), mm = __ballot(miss);
  // lane 0 reserves the wave's hit entries, lane 1 its miss entries
  uint32_t base = 0;
  const uint32_t cnt = (uint32_t)__popcll(lane ? mm : hm);
  if (lane < 2u && cnt) base = atomicAdd(lane ? &ctr->misses : &ctr->hits, cnt);
  const uint32_t hb = (uint32_t)__shfl((int)base, 0), mb = (uint32_t)__shfl((int)base, 1);
  if (hit) hit_list[hb + mask_rank(hm, lane)] = make_uint2(i, kidx);
  bool fb = false;
  if (miss) {
    miss_list[mb + mask_rank(mm, lane)] = i;
    // pk = r[0..8), R || s = r[8..24), digest = r[24..32)
    fb = prep_scalars<4, PutPlain>(r, r + 8, r + 24, prep + i, n, lat_bits);
  }
  const uint64_t fm = __ballot(fb);
  if (fm) {
    uint32_t fbase = 0;
    if (lane == 0u) fbase = atomicAdd(&ctr->fb_count, (uint32_t)__popcll(fm));
    fbase = (uint32_t)__shfl((int)fbase, 0);
    if (fb) fb_list[fbase + mask_rank(fm, lane)] = i;
  }
}

// The comb pass over the hit list (its work loop's rules: hsv_routed.hpp).
__global__ void __launch_bounds__(256, 2)
hsv_ctx_comb_kernel(const uint8_t *__restrict__ records, uint32_t n, RoutedCounters *__restrict__ ctr,
                    const uint2 *__restrict__ hit_list, const uint8_t *__restrict__ pks,
                    const uint8_t *__restrict__ key_flags, uint32_t nkeys,
                    const uint32_t *const *__restrict__ key_tables, const uint32_t *__restrict__ btable,
                    uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits, uint32_t inject,
                    uint32_t *__restrict__ fault) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nh = min((uint32_t)__builtin_amdgcn_readfirstlane(ctr->hits), n);
  uint32_t bad = 0;
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr->hit_next, 64u);
    base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
    if (base >= nh) break;
    const uint32_t j = base + lane;
    const uint2 e = hit_list[j < nh ? j : base];
    const uint32_t i = min(e.x, n - 1u), kk = e.y < nkeys ? e.y : 0u;  // (the route kernel wrote both in range)
    uint32_t pkw[8], sigw[16], msgw[8];
    {  // the member's key bytes (the record's are equal), R || s and the digest from the record
      const uint8_t *t = records + (uint64_t)i * 128u;
      load_triple(pks + (uint64_t)kk * 32u, 0, t + 32, 0, t + 96, 0, 0, pkw, sigw, msgw);
    }
    const uint32_t f = verify_one_comb(pkw, key_flags[kk], sigw, msgw, key_tables[kk], btable, inject);
    bad |= (f & kFault) ? 1u : 0u;
    store_verdict(flags_out, strict_bits, i, f);
  }
  report_faults(fault, bad);
}

// hsv_ctx_comb_kernel for a committee with compact (4-bit digit) tables
// (verify_one_comb4: 80 mixed additions and one decompression; comb16: the
// wide comb of B, where hsv_ctx_comb_kernel reads the narrow one).  A twin,
// not a template of the width: as one body both compiled 10 instructions
// longer.
__global__ void __launch_bounds__(256, 2)
hsv_ctx_comb4_kernel(const uint8_t *__restrict__ records, uint32_t n, RoutedCounters *__restrict__ ctr,
                     const uint2 *__restrict__ hit_list, const uint8_t *__restrict__ pks,
                     const uint8_t *__restrict__ key_flags, uint32_t nkeys,
                     const uint32_t *const *__restrict__ key_tables, const uint32_t *__restrict__ comb16,
                     uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits, uint32_t inject,
                     uint32_t *__restrict__ fault) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nh = min((uint32_t)__builtin_amdgcn_readfirstlane(ctr->hits), n);
  uint32_t bad = 0;
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr->hit_next, 64u);
    base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
    if (base >= nh) break;
    const uint32_t j = base + lane;
    const uint2 e = hit_list[j < nh ? j : base];
    const uint32_t i = min(e.x, n - 1u), kk = e.y < nkeys ? e.y : 0u;  // (the route kernel wrote both in range)
    uint32_t pkw[8], sigw[16], msgw[8];
    {  // the member's key bytes (the record's are equal), R || s and the digest from the record
      const uint8_t *t = records + (uint64_t)i * 128u;
      load_triple(pks + (uint64_t)kk * 32u, 0, t + 32, 0, t + 96, 0, 0, pkw, sigw, msgw);
    }
    const uint32_t f = verify_one_comb4(pkw, key_flags[kk], sigw, msgw, key_tables[kk], comb16, inject);
    bad |= (f & kFault) ? 1u : 0u;
    store_verdict(flags_out, strict_bits, i, f);
  }
  report_faults(fault, bad);
}

// hsv_verify_hp_kernel over the miss list: the fallback list first (the
// full-length path), then 64 miss-list entries per batch through
// verify_one_prepped; pk / R (fallback items: s and the digest too) from the
// records at stride 128, the prepass words at rec + i, row stride n.
// totals (diagnostics, hsv_test_committee_tx_counts): one lane adds the
// round's list lengths {hits, misses, fallback items}.
// (hsv_cmsg_generic_kernel is the same loop with other loads; its rules are
// hsv_routed.hpp's, and DESIGN.md 4j says why the two stay apart.)
template <int WA, int WAVES, int CB>
__global__ void __launch_bounds__(kBlock, WAVES)
hsv_ctx_generic_kernel(const uint8_t *__restrict__ records, uint32_t n, uint8_t *__restrict__ flags_out,
                       uint32_t *__restrict__ strict_bits, uint4 *__restrict__ vt_ws,
                       const uint32_t *__restrict__ comb_b, const uint32_t *__restrict__ rec,
                       RoutedCounters *__restrict__ ctr, const uint32_t *__restrict__ miss_list,
                       const uint32_t *__restrict__ fb_list, uint32_t *__restrict__ canary, uint32_t nonce,
                       uint32_t inject, uint32_t *__restrict__ fault, uint64_t *__restrict__ totals) {
  constexpr int kEnt = (1 << (WA - 1)) + 1;
  const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
  GlobalVarTab<kEnt> vt{vt_ws + (uint64_t)slot * vt_lane_uint4<WA>(), inject};
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nfb = min((uint32_t)__builtin_amdgcn_readfirstlane(ctr->fb_count), n);
  const uint32_t nm = min((uint32_t)__builtin_amdgcn_readfirstlane(ctr->misses), n);
  if (totals && slot == 0u) {
    totals[0] += ctr->hits;
    totals[1] += nm;
    totals[2] += nfb;
  }
  const uint32_t fb_end = (nfb + 63u) & ~63u;
  if (fb_end + nm == 0u) return;  // every transaction was a member's (or malformed)
  canary[slot] = nonce;
  uint32_t bad = 0;
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr->gen_next, 64u);
    base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
    if (base >= fb_end + nm) break;
    if (inject == kInjectCanary) canary[slot] = ~nonce;
    if (base < fb_end) {
      const uint32_t j = base + lane;
      const bool valid = j < nfb;
      const uint32_t idx = min(fb_list[valid ? j : base], n - 1u);
      uint32_t pkw[8], sigw[16], msgw[8];
      load_triple(records, 128, records + 32, 128, records + 96, 128, idx, pkw, sigw, msgw);
      const uint32_t f = verify_one_full_comb<WA, false, CB>(pkw, sigw, msgw, comb_b, vt);
      bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
      if (valid) store_verdict(flags_out, strict_bits, idx, f);
      continue;
    }
    const uint32_t b0 = base - fb_end;
    const bool valid = b0 + lane < nm;
    const uint32_t li = min(miss_list[valid ? b0 + lane : b0], n - 1u);
    uint32_t pkw[8], rw[8];
    {
      const uint4 *p = reinterpret_cast<const uint4 *>(records + (uint64_t)li * 128u);
      const uint4 p0 = p[0], p1 = p[1], r0 = p[2], r1 = p[3];
      pkw[0] = p0.x; pkw[1] = p0.y; pkw[2] = p0.z; pkw[3] = p0.w;
      pkw[4] = p1.x; pkw[5] = p1.y; pkw[6] = p1.z; pkw[7] = p1.w;
      rw[0] = r0.x; rw[1] = r0.y; rw[2] = r0.z; rw[3] = r0.w;
      rw[4] = r1.x; rw[5] = r1.y; rw[6] = r1.z; rw[7] = r1.w;
    }
    const uint32_t meta = rec[18ull * n + li];
    const bool own = valid && !(meta & kPrepFallback);
    const uint32_t f = verify_one_prepped<WA, CB>(pkw, rw, rec + li, n, meta, comb_b, vt);
    bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
    if (own) store_verdict(flags_out, strict_bits, li, f);
  }
  report_faults(fault, bad);
}

}  // namespace hsv

extern "C" hipError_t hsv_launch_tx_records(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size,
                                            uint32_t n, uint8_t *records, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = (n + hsv::kTxBlock - 1) / hsv::kTxBlock;
  hipLaunchKernelGGL((hsv::hsv_tx_record_kernel<false>), dim3(grid), dim3(hsv::kTxBlock), 0, stream, txs, offsets,
                     tx_size, n, reinterpret_cast<uint4 *>(records), nullptr, nullptr, nullptr, 0);
  return hipGetLastError();
}

extern "C" hipError_t hsv_launch_tx_prep(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                                         uint8_t *records, uint32_t *prep, uint32_t *fb_count, uint32_t *fb_list,
                                         int lat_bits, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t grid = (n + hsv::kTxBlock - 1) / hsv::kTxBlock;
  hipLaunchKernelGGL((hsv::hsv_tx_record_kernel<true>), dim3(grid), dim3(hsv::kTxBlock), 0, stream, txs, offsets,
                     tx_size, n, reinterpret_cast<uint4 *>(records), prep, fb_count, fb_list, lat_bits);
  return hipGetLastError();
}

extern "C" hipError_t hsv_launch_tx_mask(const uint64_t *offsets, uint32_t n, uint8_t *flags,
                                         uint32_t *strict_bits, hipStream_t stream) {
  if (n == 0 || !offsets) return hipSuccess;
  const uint32_t grid = (n + hsv::kTxBlock - 1) / hsv::kTxBlock;
  hipLaunchKernelGGL(hsv::hsv_tx_mask_kernel<false>, dim3(grid), dim3(hsv::kTxBlock), 0, stream, offsets, n, flags,
                     strict_bits);
  return hipGetLastError();
}

// The two launches above for a span table (hsv_internal.h): transaction i is
// txs[spans[2i], spans[2i+1]).
extern "C" hipError_t hsv_launch_tx_records_spans(const uint8_t *txs, const uint64_t *spans, uint32_t n,
                                                  uint8_t *records, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!spans) return hipErrorInvalidValue;
  const uint32_t grid = (n + hsv::kTxBlock - 1) / hsv::kTxBlock;
  hipLaunchKernelGGL((hsv::hsv_tx_record_kernel<false, true>), dim3(grid), dim3(hsv::kTxBlock), 0, stream, txs, spans,
                     (uint64_t)0, n, reinterpret_cast<uint4 *>(records), nullptr, nullptr, nullptr, 0);
  return hipGetLastError();
}

extern "C" hipError_t hsv_launch_tx_mask_spans(const uint64_t *spans, uint32_t n, uint8_t *flags,
                                               uint32_t *strict_bits, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!spans) return hipErrorInvalidValue;
  const uint32_t grid = (n + hsv::kTxBlock - 1) / hsv::kTxBlock;
  hipLaunchKernelGGL(hsv::hsv_tx_mask_kernel<true>, dim3(grid), dim3(hsv::kTxBlock), 0, stream, spans, n, flags,
                     strict_bits);
  return hipGetLastError();
}

// Blocks per CU of the fused transaction kernel (its persistent grid must fit
// the device at once, as hsv_verify_hp_kernel's), cached per device.
extern "C" int hsv_tx_fused_blocks_per_cu(int device) {
  static std::mutex mu;
  static std::unordered_map<int, int> bpc;
  std::lock_guard<std::mutex> lk(mu);
  auto it = bpc.find(device);
  if (it == bpc.end()) {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &b, reinterpret_cast<const void *>(hsv::hsv_verify_tx_fused_kernel<4, HSV_HP_WAVES, 16>), hsv::kBlock,
            0) != hipSuccess)
      return -1;
    it = bpc.emplace(device, b).first;
  }
  return it->second;
}

extern "C" hipError_t hsv_launch_tx_fused(uint32_t grid, const uint8_t *txs, const uint64_t *offsets,
                                          uint64_t tx_size, uint32_t n, uint8_t *records, uint32_t *rec,
                                          void *ctr, uint32_t *fb_list, uint32_t *ready, int lat_bits,
                                          uint8_t *flags_out, uint32_t *strict_bits, void *vt_ws,
                                          const uint32_t *comb_b, uint32_t *canary, uint32_t nonce, uint32_t inject,
                                          uint32_t *fault, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if ((uint64_t)n * 128u > 0xffffffffull || grid == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL((hsv::hsv_verify_tx_fused_kernel<4, HSV_HP_WAVES, 16>), dim3(grid), dim3(hsv::kBlock), 0, stream,
                     txs, offsets, tx_size, n, records, rec, static_cast<hsv::HcCounters *>(ctr), fb_list, ready,
                     lat_bits, flags_out, strict_bits, static_cast<uint4 *>(vt_ws), comb_b, canary, nonce, inject,
                     fault);
  return hipGetLastError();
}

// ---- one round of hsv_committee_verify_transactions* -------------------------------
// n <= 2^22 transactions: the round of hsv_routed.hpp (RoutedRound: grids,
// memsets, the comb pass by table width).  Workspace from the library pool:
// per-lane tables | counters | canaries | records | hit list | miss list |
// fallback list | prepass words.  SPANS: offsets is tx_span's span table.
namespace {
template <bool SPANS>
hipError_t launch_committee_tx(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                               const uint32_t *keytab, uint32_t keymask, uint64_t seed, const uint8_t *pks,
                               const uint8_t *key_flags, uint32_t nkeys, const uint32_t *const *key_tables,
                               int digit_bits, const uint32_t *btable, const uint32_t *comb16, uint8_t *flags_out,
                               uint32_t *strict_bits, uint32_t *fault, uint64_t *totals, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > (1u << 22) || (digit_bits != 8 && digit_bits != 4) || !btable || !comb16 || !fault || (nkeys && (!keytab || !pks || !key_flags || !key_tables)))
    return hipErrorInvalidValue;
  hsv::RoutedRound r;
  hipError_t e = r.size(n, digit_bits, reinterpret_cast<const void *>(hsv::hsv_ctx_comb_kernel),
                        reinterpret_cast<const void *>(hsv::hsv_ctx_comb4_kernel),
                        reinterpret_cast<const void *>(hsv::hsv_ctx_generic_kernel<4, HSV_HP_WAVES, 16>));
  if (e != hipSuccess) return e;
  const size_t rec_bytes = (size_t)n * 128, hit_bytes = hsv::up256((size_t)n * sizeof(uint2));
  const size_t list_bytes = hsv::up256((size_t)n * sizeof(uint32_t));
  const size_t prep_bytes = (size_t)n * hsv::kPrepWords * sizeof(uint32_t);
  hsv::Workspace ws(nullptr, 0, r.head_bytes() + rec_bytes + hit_bytes + 2 * list_bytes + prep_bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *p = ws.get();
  uint4 *vt_ws = reinterpret_cast<uint4 *>(p);
  hsv::RoutedCounters *ctr = reinterpret_cast<hsv::RoutedCounters *>(p += r.vt_bytes);
  uint32_t *canary = reinterpret_cast<uint32_t *>(p += 256);
  uint8_t *records = (p += r.canary_bytes);
  uint2 *hit_list = reinterpret_cast<uint2 *>(p += rec_bytes);
  uint32_t *miss_list = reinterpret_cast<uint32_t *>(p += hit_bytes);
  uint32_t *fb_list = reinterpret_cast<uint32_t *>(p += list_bytes);
  uint32_t *prep = reinterpret_cast<uint32_t *>(p += list_bytes);
  const uint32_t inject = (uint32_t)hsvi_inject_mode();
  e = hsv::RoutedRound::zero(ctr, strict_bits, n, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hsv::hsv_ctx_route_kernel<SPANS>, dim3(r.blocks_needed), dim3(hsv::kTxBlock), 0, stream, txs, offsets,
                       tx_size, n, reinterpret_cast<uint4 *>(records), keytab, keymask, seed, pks, nkeys, ctr, hit_list,
                       miss_list, prep, fb_list, hsvi_lattice_bits(), flags_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(r.pick(hsv::hsv_ctx_comb_kernel, hsv::hsv_ctx_comb4_kernel), dim3(r.grid_c), dim3(256), 0,
                       stream, records, n, ctr, hit_list, pks, key_flags, nkeys, key_tables, r.pick(btable, comb16),
                       flags_out, strict_bits, inject, fault);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL((hsv::hsv_ctx_generic_kernel<4, HSV_HP_WAVES, 16>), dim3(r.grid_g), dim3(hsv::kBlock), 0, stream,
                       records, n, flags_out, strict_bits, vt_ws, comb16, prep, ctr, miss_list, fb_list, canary,
                       hsvi_next_nonce(), inject, fault, totals);
    e = hipGetLastError();
  }
  return ws.done(e);
}
}  // namespace

extern "C" hipError_t hsv_launch_committee_tx(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                                              const uint32_t *keytab, uint32_t keymask, uint64_t seed,
                                              const uint8_t *pks, const uint8_t *key_flags, uint32_t nkeys,
                                              const uint32_t *const *key_tables, int digit_bits,
                                              const uint32_t *btable, const uint32_t *comb16, uint8_t *flags_out,
                                              uint32_t *strict_bits, uint32_t *fault, uint64_t *totals,
                                              hipStream_t stream) {
  return launch_committee_tx<false>(txs, offsets, tx_size, n, keytab, keymask, seed, pks, key_flags, nkeys, key_tables,
                                    digit_bits, btable, comb16, flags_out, strict_bits, fault, totals, stream);
}

extern "C" hipError_t hsv_launch_committee_tx_spans(const uint8_t *txs, const uint64_t *spans, uint32_t n,
                                                    const uint32_t *keytab, uint32_t keymask, uint64_t seed,
                                                    const uint8_t *pks, const uint8_t *key_flags, uint32_t nkeys,
                                                    const uint32_t *const *key_tables, int digit_bits,
                                                    const uint32_t *btable, const uint32_t *comb16,
                                                    uint8_t *flags_out, uint32_t *strict_bits, uint32_t *fault,
                                                    uint64_t *totals, hipStream_t stream) {
  if (n && !spans) return hipErrorInvalidValue;
  return launch_committee_tx<true>(txs, spans, 0, n, keytab, keymask, seed, pks, key_flags, nkeys, key_tables,
                                   digit_bits, btable, comb16, flags_out, strict_bits, fault, totals, stream);
}
