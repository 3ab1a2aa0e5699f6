// Whole messages of known signers (hsv_committee_verify_msgs*, include/hsv.h).
//
// RFC 8032 5.1.7 PureEdDSA as hsv_verify_msgs* (hsv_msgs.hip), with the signer
// looked up on the device as hsv_committee_verify_transactions* does
// (hsv_mempool.hip, hsv_keytab.hpp): an item whose 32 pk bytes equal a committee
// member's is verified from the member's comb table (verify_one_comb_k: 64
// mixed additions and one decompression), any other by the generic point pass.
// A round of at most 2^22 items is three launches on the caller's stream:
//   1. hsv_cmsg_route_kernel    one lane per item: SHA-512(R || A || M) block by
//      block (msg_hash_lane, hsv_msgwave.hpp), then the lookup; members to the
//      hit list as (i, member index) with k mod l in the k record, the others
//      to the miss list as i -- those lanes also run the point pass's prepass;
//      an item with decreasing offsets goes on no list and gets flags 0 here;
//   2. hsv_cmsg_comb_kernel     persistent, 64 hit-list entries per batch;
//   3. hsv_cmsg_generic_kernel  persistent, the fallback list and then the miss
//      list, as hsv_verify_hp_kernel's KREC form.
// Both passes read pk, R and s in place from the caller's arrays and the
// challenge from the route kernel's records; neither reads a message byte, so
// one long message keeps one wave of the route kernel busy and no wave of a
// persistent grid.  Every hand-off is a kernel boundary: no ready words, no
// polling, nothing a pass could wait for.  Flags are those of hsv_verify_msgs*
// bit for bit: both routes return verify_one's byte for the same (pk, sig, k),
// and a hit means the 32 pk bytes equal the member's.
//
// Whole messages by member index (hsv_committee_verify_msgs_indexed*): the
// caller names each item's member, so there is no lookup and no miss side.
//   * at most kCombQuadMax items, 8-bit tables: ONE launch of
//     hsv_cmsg_quad_kernel, the latency form of hsv_committee.hip (4 votes per
//     block: a comb wave, two R waves, a hash wave) with a hash wave that runs
//     msg_hash_wave<64> over head = R || member key;
//   * otherwise a round of at most 2^22 items is a memset of the counters and
//     two launches: hsv_cmsg_index_kernel (one lane per item: the hash, (i,
//     member) to the hit list, k mod l to the k record) and the comb pass above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <unordered_map>

#define HSV_SHA_BITOP3 1  // v_bitop3_b32 in the message hash, as hsv_msgs.hip
#include "hsv_internal.h"
#include "hsv_keytab.hpp"
#include "hsv_msgwave.hpp"
#include "hsv_verify_hc.hpp"
#include "hsv_pointpass.hpp"
#include "hsv_quad.hpp"
#include "hsv_routed.hpp"

namespace hsv {

// One lane per item; the list compaction's rules: hsv_routed.hpp.  Every store
// and atomic sits after the hash loop (msg_hash_lane), so no loop surrounds
// them; a lane past n redoes item n - 1 in that loop and stores nothing.
// krec: k mod l of the members' items, eight words, row stride n.
__global__ void __launch_bounds__(kMsgBlock)
hsv_cmsg_route_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                      uint64_t sig_stride, const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ offsets,
                      uint64_t msg_len, uint64_t msg_stride, uint32_t n, const uint32_t *__restrict__ keytab,
                      uint32_t keymask, uint64_t seed, const uint8_t *__restrict__ pks, uint32_t nkeys,
                      RoutedCounters *__restrict__ ctr, uint2 *__restrict__ hit_list, uint32_t *__restrict__ miss_list,
                      uint32_t *__restrict__ krec, uint32_t *__restrict__ prep, uint32_t *__restrict__ fb_list,
                      int lat_bits, uint8_t *__restrict__ flags_out) {
  __shared__ uint4 stage_all[kMsgWaves][64 * kMsgQ];
  __builtin_amdgcn_s_setprio(3);  // as hsv_msg_prep_kernel: ahead of an earlier call's running passes
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kMsgBlock + wv * 64u >= n) return;  // whole wave past the end
  const uint32_t i_in = blockIdx.x * kMsgBlock + threadIdx.x;
  const uint32_t i = i_in < n ? i_in : n - 1u;
  const uint8_t *pki = pk + (uint64_t)i * pk_stride, *sigi = sig + (uint64_t)i * sig_stride;
  uint32_t hw[16];
  const bool ok = msg_hash_lane(pk, pk_stride, sig, sig_stride, msgs, offsets, msg_len, msg_stride, i, lane,
                                stage_all[wv], hw);
  const bool live = i_in < n && ok;
  if (i_in < n && !ok && flags_out) flags_out[i] = 0;  // void: on no list (its strict bit: zeroed by the host)
  uint32_t pkw[8];
  load_words8(pki, pkw);
  uint32_t kidx = kKeytabMiss;
  if (live && nkeys) kidx = keytab_find(keytab, keymask, seed, pks, pkw);
  const bool hit = live && kidx < nkeys, miss = live && !hit;
  const uint64_t hm = __ballot(hit), mm = __ballot(miss);
  // lane 0 reserves the wave's hit entries, lane 1 its miss entries
  uint32_t base = 0;
  const uint32_t cnt = (uint32_t)__popcll(lane ? mm : hm);
  if (lane < 2u && cnt) base = atomicAdd(lane ? &ctr->misses : &ctr->hits, cnt);
  const uint32_t hb = (uint32_t)__shfl((int)base, 0), mb = (uint32_t)__shfl((int)base, 1);
  if (hit) {  // the comb route takes k mod l as it is: no lattice reduction
    hit_list[hb + mask_rank(hm, lane)] = make_uint2(i, kidx);
    const sc k = sc_reduce512(hw);
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) krec[(uint64_t)j * n + i] = k.v[j];
  }
  bool fb = false;
  if (miss) {
    miss_list[mb + mask_rank(mm, lane)] = i;
    uint32_t s[8];
    load_words8(sigi + 32, s);
    fb = prep_from_hash<4, PutPlain, true>(hw, s, prep + i, n, lat_bits);
  }
  const uint64_t fm = __ballot(fb);
  if (fm) {
    uint32_t fbase = 0;
    if (lane == 0u) fbase = atomicAdd(&ctr->fb_count, (uint32_t)__popcll(fm));
    fbase = (uint32_t)__shfl((int)fbase, 0);
    if (fb) fb_list[fbase + mask_rank(fm, lane)] = i;
  }
}

// The comb pass over the hit list (patterned on hsv_ctx_comb_kernel), for
// either table width (DIGITS 8: tb the 8-bit table of B; 4: the wide comb of
// B): R || s in place from the caller's sig array, k from the k record, the
// member's tables by its index.  The work loop's rules: hsv_routed.hpp.
template <int DIGITS>
__device__ __forceinline__ void cmsg_comb_pass(const uint8_t *sig, uint64_t sig_stride, uint32_t n, RoutedCounters *ctr,
                                               const uint2 *hit_list, const uint32_t *krec, const uint8_t *key_flags,
                                               uint32_t nkeys, const uint32_t *const *key_tables, const uint32_t *tb,
                                               uint8_t *flags_out, uint32_t *strict_bits, uint32_t inject,
                                               uint32_t *fault) {
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
    uint32_t sigw[16];
    load_words8(sig + (uint64_t)i * sig_stride, sigw);
    load_words8(sig + (uint64_t)i * sig_stride + 32, sigw + 8);
    sc k;
    HSV_UNROLL
    for (int w = 0; w < 8; ++w) k.v[w] = krec[(uint64_t)w * n + i];
    const uint32_t f = verify_comb_k<DIGITS>(key_flags[kk], sigw, k, key_tables[kk], tb, inject);
    bad |= (f & kFault) ? 1u : 0u;
    store_verdict(flags_out, strict_bits, i, f);
  }
  report_faults(fault, bad);
}

__global__ void __launch_bounds__(256, 2)
hsv_cmsg_comb_kernel(const uint8_t *__restrict__ sig, uint64_t sig_stride, uint32_t n, RoutedCounters *__restrict__ ctr,
                     const uint2 *__restrict__ hit_list, const uint32_t *__restrict__ krec,
                     const uint8_t *__restrict__ key_flags, uint32_t nkeys,
                     const uint32_t *const *__restrict__ key_tables, const uint32_t *__restrict__ btable,
                     uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits, uint32_t inject,
                     uint32_t *__restrict__ fault) {
  cmsg_comb_pass<8>(sig, sig_stride, n, ctr, hit_list, krec, key_flags, nkeys, key_tables, btable, flags_out,
                    strict_bits, inject, fault);
}

// hsv_cmsg_comb_kernel for a committee with compact (4-bit digit) tables
// (verify_one_comb4_k: 80 mixed additions and one decompression; comb16: the
// wide comb of B, where hsv_cmsg_comb_kernel reads the narrow one).
__global__ void __launch_bounds__(256, 2)
hsv_cmsg_comb4_kernel(const uint8_t *__restrict__ sig, uint64_t sig_stride, uint32_t n, RoutedCounters *__restrict__ ctr,
                      const uint2 *__restrict__ hit_list, const uint32_t *__restrict__ krec,
                      const uint8_t *__restrict__ key_flags, uint32_t nkeys,
                      const uint32_t *const *__restrict__ key_tables, const uint32_t *__restrict__ comb16,
                      uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits, uint32_t inject,
                      uint32_t *__restrict__ fault) {
  cmsg_comb_pass<4>(sig, sig_stride, n, ctr, hit_list, krec, key_flags, nkeys, key_tables, comb16, flags_out,
                    strict_bits, inject, fault);
}

// hsv_ctx_generic_kernel (hsv_mempool.hip) with pk, R and s read in place from
// the caller's arrays at their strides instead of 128-byte records, and the
// fallback items' k mod l read from the b words of their prepass record, as
// hsv_verify_hp_kernel's KREC form: the fallback list first (the full-length
// path), then 64 miss-list entries per batch through verify_one_prepped.
// totals (diagnostics, hsv_test_committee_msgs_counts): one lane adds the
// round's list lengths {hits, misses, fallback items}.
template <int WA, int WAVES, int CB>
__global__ void __launch_bounds__(kBlock, WAVES)
hsv_cmsg_generic_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                        uint64_t sig_stride, uint32_t n, uint8_t *__restrict__ flags_out,
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
  if (fb_end + nm == 0u) return;  // every item was a member's (or void)
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
      uint32_t pkw[8], sigw[16];
      load_words8(pk + (uint64_t)idx * pk_stride, pkw);
      load_words8(sig + (uint64_t)idx * sig_stride, sigw);
      load_words8(sig + (uint64_t)idx * sig_stride + 32, sigw + 8);
      sc k;
      HSV_UNROLL
      for (int w = 0; w < 8; ++w) k.v[w] = rec[(10ull + (uint64_t)w) * n + idx];
      const uint32_t f = verify_one_full_comb<WA, false, CB>(pkw, sigw, k, comb_b, vt);
      bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
      if (valid) store_verdict(flags_out, strict_bits, idx, f);
      continue;
    }
    const uint32_t b0 = base - fb_end;
    const bool valid = b0 + lane < nm;
    const uint32_t li = min(miss_list[valid ? b0 + lane : b0], n - 1u);
    uint32_t pkw[8], rw[8];
    load_words8(pk + (uint64_t)li * pk_stride, pkw);
    load_words8(sig + (uint64_t)li * sig_stride, rw);
    const uint32_t meta = rec[18ull * n + li];
    const bool own = valid && !(meta & kPrepFallback);
    const uint32_t f = verify_one_prepped<WA, CB>(pkw, rw, rec + li, n, meta, comb_b, vt);
    bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
    if (own) store_verdict(flags_out, strict_bits, li, f);
  }
  report_faults(fault, bad);
}

// ---- by member index ---------------------------------------------------------------
// Item i of an index-addressed batch: its message range by hsv_verify_msgs*'
// addressing and the head of its hash, R (sig + i * sig_stride) || the key of
// member kk (pks + 32 kk).  Returns false for a decreasing pair of offsets.
__device__ __forceinline__ bool cmsg_item(const uint8_t *__restrict__ sig, uint64_t sig_stride,
                                          const uint64_t *__restrict__ offsets, uint64_t msg_len, uint64_t msg_stride,
                                          const uint8_t *__restrict__ pks, uint32_t i, uint32_t kk, uint32_t head[16],
                                          uint64_t &lo, uint64_t &mlen) {
  uint64_t hi;
  if (offsets) {
    lo = offsets[i];
    hi = offsets[i + 1];
  } else {
    lo = (uint64_t)i * msg_stride;
    hi = lo + msg_len;
  }
  mlen = hi - lo;
  load_words8(sig + (uint64_t)i * sig_stride, head);
  load_words8(pks + (uint64_t)kk * 32, head + 8);
  return hi >= lo;
}

// this TU's launches by member index (hsv_test_cmsg_indexed_counts): the items
// that hsv_cmsg_index_kernel put on a hit list, summed over the process
__device__ unsigned long long g_cmsg_index_live;

// The first launch of the bulk route: hsv_cmsg_route_kernel without the lookup
// and without the miss side.  One lane per item; a live item (index < nkeys,
// offsets not decreasing) goes to the hit list as (i, kidx) with k mod l in the
// k record, any other lane of the batch stores flags 0 and hashes the empty
// message.  Every store and atomic sits after the hash loop (msg_hash_wave).
__global__ void __launch_bounds__(kMsgBlock)
hsv_cmsg_index_kernel(const uint32_t *__restrict__ key_idx, const uint8_t *__restrict__ sig, uint64_t sig_stride,
                      const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ offsets, uint64_t msg_len,
                      uint64_t msg_stride, uint32_t n, const uint8_t *__restrict__ pks, uint32_t nkeys,
                      RoutedCounters *__restrict__ ctr, uint2 *__restrict__ hit_list, uint32_t *__restrict__ krec,
                      uint8_t *__restrict__ flags_out) {
  __shared__ uint4 stage_all[kMsgWaves][64 * kMsgQ];
  __builtin_amdgcn_s_setprio(3);  // as hsv_cmsg_route_kernel
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (blockIdx.x * kMsgBlock + wv * 64u >= n) return;  // whole wave past the end
  const uint32_t i_in = blockIdx.x * kMsgBlock + threadIdx.x;
  const uint32_t i = i_in < n ? i_in : n - 1u;
  const uint32_t kidx = key_idx[i];
  uint32_t head[16], hw[16];
  uint64_t lo, mlen;
  const bool ok = cmsg_item(sig, sig_stride, offsets, msg_len, msg_stride, pks, i, kidx < nkeys ? kidx : 0u, head, lo, mlen);
  const bool live = i_in < n && ok && kidx < nkeys;
  msg_hash_wave<64>(head, msgs, live ? lo : 0, live ? mlen : 0, lane, stage_all[wv], hw);
  if (i_in < n && !live) flags_out[i] = 0;  // void: on no list
  const uint64_t hm = __ballot(live);
  uint32_t base = 0;
  if (lane == 0u && hm) {  // lane 0 reserves the wave's entries
    base = atomicAdd(&ctr->hits, (uint32_t)__popcll(hm));
    atomicAdd(&g_cmsg_index_live, (unsigned long long)__popcll(hm));
  }
  const uint32_t hb = (uint32_t)__shfl((int)base, 0);
  if (live) {
    hit_list[hb + mask_rank(hm, lane)] = make_uint2(i, kidx);
    const sc k = sc_reduce512(hw);
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) krec[(uint64_t)j * n + i] = k.v[j];
  }
}

// The one-launch latency form: comb_quad_block's twin (hsv_committee.hip; the
// geometry: hsv_quad.hpp) for whole messages.  Only the hash wave differs: all
// 64 lanes call msg_hash_wave<64>, lanes 0..3 with the block's votes, the
// others (and the last block's spare slots, and a void vote) with an empty
// message, so the wave's trip count is the longest of the block's at most 4
// messages.  A vote whose offsets decrease is void: its bit goes to the comb
// wave beside k_rec, and lane g == 0 writes its flags as 0, as for a key index
// out of range.  The comb wave, the R waves, the swap rounds, the checks, the
// flag byte and the fault word are comb_quad_block's; the k_ready wait inside
// the block is the kernel's only wait.  No completion markers, no wave clocks.
// (A twin and not a parameter of comb_quad_block: the digest kernels are the
// most timing-sensitive code of the tree and keep their text to themselves.)
__device__ __forceinline__ void cmsg_quad_block(const uint32_t *__restrict__ key_idx, const uint8_t *__restrict__ sig,
                                                uint64_t sig_stride, const uint8_t *__restrict__ msgs,
                                                const uint64_t *__restrict__ offsets, uint64_t msg_len,
                                                uint64_t msg_stride, uint32_t m, const uint8_t *__restrict__ pks,
                                                const uint8_t *__restrict__ key_flags, uint32_t nkeys,
                                                const uint32_t *const *__restrict__ key_tables,
                                                const uint32_t *__restrict__ btable, uint8_t *__restrict__ flags_out,
                                                uint32_t inject, uint32_t *__restrict__ fault, uint32_t blk) {
  __shared__ uint32_t r_x[kFusedVotes][kFeLimbs], r_y[kFusedVotes][kFeLimbs], r_fl[kFusedVotes];
  __shared__ uint32_t k_rec[kFusedVotes][9], k_void[kFusedVotes], k_ready;
  __shared__ uint4 stage[64 * kMsgQ];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t base = blk * kFusedVotes;
  // vote v of the block reads vote min(base + v, m - 1): the last block's
  // spare slots repeat the batch's last vote and write no flag
  auto vote_of = [&](uint32_t v) { return base + v < m ? base + v : m - 1u; };
  if (threadIdx.x == 0) k_ready = 0u;  // LDS keeps the last block's flag: cleared before any wave can look
  __syncthreads();
  auto vote_sig = [&](uint32_t v) { return reinterpret_cast<const uint4 *>(sig + (uint64_t)vote_of(v) * sig_stride); };
  if (wave == kHashWaveIdx) {
    const uint32_t vl = lane % (uint32_t)kFusedVotes;  // a lane without a vote reads its row's (in range) and hashes nothing
    const bool own = lane < (uint32_t)kFusedVotes && base + lane < m;
    const uint32_t i = vote_of(vl), kidx = key_idx[i];
    uint32_t head[16], h[16];
    uint64_t lo, mlen;
    const bool ok = cmsg_item(sig, sig_stride, offsets, msg_len, msg_stride, pks, i, kidx < nkeys ? kidx : 0u, head, lo, mlen);
    const bool live = own && ok && kidx < nkeys;
    msg_hash_wave<64>(head, msgs, live ? lo : 0, live ? mlen : 0, lane, stage, h);
    if (lane < (uint32_t)kFusedVotes) {
      uint32_t kr[9];
      const sc k = sc_reduce512(h);
      recode_add<9, 8, kCombPos>(k.v, 8, kr);
      HSV_UNROLL
      for (int w = 0; w < 9; ++w) k_rec[lane][w] = kr[w];
      k_void[lane] = ok ? 0u : 1u;
    }
    __hip_atomic_store(&k_ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    return;
  }
  if (wave >= 1) {
    const RLane L;
    const uint32_t row = lane >> 4;
    const uint32_t vr = (wave - 1u) * kRVotesPerWave + row / kRRows;  // this row's vote in the block
    if (vr < (uint32_t)kFusedVotes) {
      const uint4 *sp = vote_sig(vr);
      const uint4 s0 = sp[0], s1 = sp[1];
      const uint32_t rw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      fe rx, ry;
      uint32_t small, nc = 0;
      const uint32_t r_ok = ge_decompress_row(rw, rx, ry, small, nc, L);
      const uint32_t small_r = r_ok & small;
      if (L.k == 0u && row % kRRows == 0u) {
        HSV_UNROLL
        for (int l = 0; l < kFeLimbs; ++l) {
          r_x[vr][l] = rx.v[l];
          r_y[vr][l] = ry.v[l];
        }
        r_fl[vr] = r_ok | (small_r << 1) | (nc << 2);  // bit 2: self-check (fl_to_fe)
      }
    }
    __syncthreads();
    return;
  }
  const uint32_t vl = lane / kCombLanes, g = lane % kCombLanes;
  const uint32_t i0 = base + vl;
  const bool valid = i0 < m;
  const uint32_t kidx = key_idx[vote_of(vl)];
  const bool kin = kidx < nkeys;
  const uint32_t kk = kin ? kidx : 0u;
  uint32_t sigw[16];
  {
    const uint4 *sp = vote_sig(vl);
    const uint4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
    sigw[0] = s0.x; sigw[1] = s0.y; sigw[2] = s0.z; sigw[3] = s0.w;
    sigw[4] = s1.x; sigw[5] = s1.y; sigw[6] = s1.z; sigw[7] = s1.w;
    sigw[8] = s2.x; sigw[9] = s2.y; sigw[10] = s2.z; sigw[11] = s2.w;
    sigw[12] = s3.x; sigw[13] = s3.y; sigw[14] = s3.z; sigw[15] = s3.w;
  }
  const uint32_t s_ok = sc_is_canonical(sigw + 8);
  const uint32_t kf = key_flags[kk];  // now, not after the final barrier (comb_quad_block)
  const uint32_t *ta = key_tables[kk];
  ge_ext q = ge_identity();
  uint32_t sr[9];
  recode_add<9, 8, kCombPos>(sigw + 8, 8, sr);
  uint64_t sd = lane_digits(sr, g), kd;
  // the s half first, while the hash wave works on k
  HSV_NOUNROLL
  for (int jj = 0; jj < kCombPosPerLane; ++jj) {
    const uint32_t j = g * kCombPosPerLane + (uint32_t)jj;
    const CombPosTab tpb{btable + (uint64_t)j * kCombEnt * kCombEntryWords};
    q = ge_add_niels<true>(q, select_niels<8>(tpb, (uint32_t)sd & 0xffu));
    sd >>= 8;
  }
  while (__hip_atomic_load(&k_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u)
    __builtin_amdgcn_s_sleep(1);
  uint32_t kvoid;
  {
    uint32_t kr[9];
    HSV_UNROLL
    for (int w = 0; w < 9; ++w) kr[w] = k_rec[vl][w];
    kd = lane_digits(kr, g);
    kvoid = k_void[vl];
  }
  const bool kvalid = kin && kvoid == 0u;
  HSV_NOUNROLL
  for (int jj = 0; jj < kCombPosPerLane; ++jj) {
    const uint32_t j = g * kCombPosPerLane + (uint32_t)jj;
    const CombPosTab tpa{ta + (uint64_t)j * kCombEnt * kCombEntryWords};
    ge_niels na = select_niels<8>(tpa, (uint32_t)kd & 0xffu);
    kd >>= 8;
    if (inject != kInjectNone && jj == 0) na = niels_injected(na, inject);
    q = ge_add_niels<true>(q, na);
  }
  HSV_UNROLL
  for (int mask = 1; mask < kCombLanes; mask <<= 1)
    q = ge_add_cached_rt(q, ge_to_cached(ge_swap_xor(q, mask)), mask < kCombLanes / 2);
  // the self-check of Q needs nothing from the R waves: before the barrier
  uint32_t z_nonzero = 0;
  const uint32_t sane = ge_is_sane_row(q, z_nonzero);
  __syncthreads();
  fe rx, ry;
  HSV_UNROLL
  for (int l = 0; l < kFeLimbs; ++l) {
    rx.v[l] = r_x[vl][l];
    ry.v[l] = r_y[vl][l];
  }
  const uint32_t rf = r_fl[vl];
  const uint32_t r_ok = rf & 1u, small_r = (rf >> 1) & 1u;
  const uint32_t same = ge_eq_affine_row(q, rx, ry, z_nonzero);
  const uint32_t a_ok = (kf & kKeyAOk) ? 1u : 0u;
  const uint32_t small_a = a_ok & ((kf & kKeySmallA) ? 1u : 0u);
  const uint32_t parse_ok = s_ok & a_ok & r_ok;
  const uint32_t eq_ok = parse_ok & same;
  const uint32_t strict_ok = eq_ok & (small_a ^ 1u) & (small_r ^ 1u);
  const uint32_t f = (strict_ok ? kStrictOk : 0u) | (eq_ok ? kEqOk : 0u) | (parse_ok ? kParseOk : 0u) |
                     (small_a ? kSmallA : 0u) | (small_r ? kSmallR : 0u) | (s_ok ? kSOk : 0u) |
                     (a_ok ? kAOk : 0u) | (r_ok ? kROk : 0u);
  const uint32_t fb = a_ok & r_ok & (sane ^ 1u);
  if (fb | ((rf >> 2) & 1u)) fault[0] = 1u;  // device self-check (hsv_pointpass.hpp report_faults)
  if (valid && g == 0u) flags_out[i0] = kvalid ? (uint8_t)f : (uint8_t)0;
}

__global__ void __launch_bounds__(kFusedThreads)
hsv_cmsg_quad_kernel(const uint32_t *__restrict__ key_idx, const uint8_t *__restrict__ sig, uint64_t sig_stride,
                     const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ offsets, uint64_t msg_len,
                     uint64_t msg_stride, uint32_t m, const uint8_t *__restrict__ pks,
                     const uint8_t *__restrict__ key_flags, uint32_t nkeys,
                     const uint32_t *const *__restrict__ key_tables, const uint32_t *__restrict__ btable,
                     uint8_t *__restrict__ flags_out, uint32_t inject, uint32_t *__restrict__ fault) {
  cmsg_quad_block(key_idx, sig, sig_stride, msgs, offsets, msg_len, msg_stride, m, pks, key_flags, nkeys, key_tables,
                  btable, flags_out, inject, fault, blockIdx.x);
}

}  // namespace hsv

// ---- one round of hsv_committee_verify_msgs* -----------------------------------
// n <= 2^22 items: the round of hsv_routed.hpp (RoutedRound: grids, memsets,
// the comb pass by table width).  Workspace from the library pool: per-lane
// tables | counters | canaries | k record | hit list | miss list | fallback
// list | prepass words.  No 128-byte records: the passes read pk and sig in
// place.
extern "C" hipError_t hsv_launch_committee_msgs(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                                uint64_t sig_stride, const uint8_t *msgs, const uint64_t *offsets,
                                                uint64_t msg_len, uint64_t msg_stride, uint32_t n,
                                                const uint32_t *keytab, uint32_t keymask, uint64_t seed,
                                                const uint8_t *pks, const uint8_t *key_flags, uint32_t nkeys,
                                                const uint32_t *const *key_tables, int digit_bits,
                                                const uint32_t *btable, const uint32_t *comb16, uint8_t *flags_out,
                                                uint32_t *strict_bits, uint32_t *fault, uint64_t *totals,
                                                hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > (1u << 22) || (digit_bits != 8 && digit_bits != 4) || !pk || !sig || !btable || !comb16 || !fault ||
      (nkeys && (!keytab || !pks || !key_flags || !key_tables)))
    return hipErrorInvalidValue;
  hsv::RoutedRound r;
  hipError_t e = r.size(n, digit_bits, reinterpret_cast<const void *>(hsv::hsv_cmsg_comb_kernel),
                        reinterpret_cast<const void *>(hsv::hsv_cmsg_comb4_kernel),
                        reinterpret_cast<const void *>(hsv::hsv_cmsg_generic_kernel<4, HSV_HP_WAVES, 16>));
  if (e != hipSuccess) return e;
  const size_t krec_bytes = hsv::up256((size_t)n * 32), hit_bytes = hsv::up256((size_t)n * sizeof(uint2));
  const size_t list_bytes = hsv::up256((size_t)n * sizeof(uint32_t));
  const size_t prep_bytes = (size_t)n * hsv::kPrepWords * sizeof(uint32_t);
  hsv::Workspace ws(nullptr, 0, r.head_bytes() + krec_bytes + hit_bytes + 2 * list_bytes + prep_bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *p = ws.get();
  uint4 *vt_ws = reinterpret_cast<uint4 *>(p);
  hsv::RoutedCounters *ctr = reinterpret_cast<hsv::RoutedCounters *>(p += r.vt_bytes);
  uint32_t *canary = reinterpret_cast<uint32_t *>(p += 256);
  uint32_t *krec = reinterpret_cast<uint32_t *>(p += r.canary_bytes);
  uint2 *hit_list = reinterpret_cast<uint2 *>(p += krec_bytes);
  uint32_t *miss_list = reinterpret_cast<uint32_t *>(p += hit_bytes);
  uint32_t *fb_list = reinterpret_cast<uint32_t *>(p += list_bytes);
  uint32_t *prep = reinterpret_cast<uint32_t *>(p += list_bytes);
  const uint32_t inject = (uint32_t)hsvi_inject_mode();
  e = hsv::RoutedRound::zero(ctr, strict_bits, n, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hsv::hsv_cmsg_route_kernel, dim3((n + hsv::kMsgBlock - 1) / hsv::kMsgBlock),
                       dim3(hsv::kMsgBlock), 0, stream, pk, pk_stride, sig, sig_stride, msgs, offsets, msg_len,
                       msg_stride, n, keytab, keymask, seed, pks, nkeys, ctr, hit_list, miss_list, krec, prep, fb_list,
                       hsvi_lattice_bits(), flags_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(r.pick(hsv::hsv_cmsg_comb_kernel, hsv::hsv_cmsg_comb4_kernel), dim3(r.grid_c), dim3(256), 0,
                       stream, sig, sig_stride, n, ctr, hit_list, krec, key_flags, nkeys, key_tables,
                       r.pick(btable, comb16), flags_out, strict_bits, inject, fault);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL((hsv::hsv_cmsg_generic_kernel<4, HSV_HP_WAVES, 16>), dim3(r.grid_g), dim3(hsv::kBlock), 0, stream,
                       pk, pk_stride, sig, sig_stride, n, flags_out, strict_bits, vt_ws, comb16, prep, ctr, miss_list,
                       fb_list, canary, hsvi_next_nonce(), inject, fault, totals);
    e = hipGetLastError();
  }
  return ws.done(e);
}

// ---- one round of hsv_committee_verify_msgs_indexed* ----------------------------
namespace {
// How hsv_launch_committee_msgs_indexed routes a round: -1 by n and the table
// width (the product's rule), 0 the bulk route, 1 the quad form at every n.  A
// measurement switch that only libhsv_test.so can move (hsv_test_cmsg_indexed_form),
// as g_msgs_small in hsv_kernels.hip.
std::atomic<int> g_cmsg_indexed_form{-1};
std::atomic<uint64_t> g_cmsg_indexed_quads, g_cmsg_indexed_rounds;  // quad launches, bulk rounds so far
}  // namespace

extern "C" int hsvi_set_cmsg_indexed_form(int mode) {
  if (mode < -1 || mode > 1) return -2;
  return g_cmsg_indexed_form.exchange(mode);
}
extern "C" int hsvi_cmsg_indexed_form(void) { return g_cmsg_indexed_form.load(); }

// {quad launches, bulk rounds, items live in the bulk hit lists}: the first two
// of the process, the third of the current device; 0 or a hipError_t
extern "C" int hsvi_cmsg_indexed_counts(uint64_t out[3]) {
  unsigned long long live = 0;
  out[0] = g_cmsg_indexed_quads.load();
  out[1] = g_cmsg_indexed_rounds.load();
  out[2] = 0;
  if (out[1] == 0) return 0;  // no bulk round yet: nothing on a device to read
  const hipError_t e = hipMemcpyFromSymbol(&live, HIP_SYMBOL(hsv::g_cmsg_index_live), sizeof(live));
  out[2] = live;
  return (int)e;
}

// n <= 2^22 items by member index.  The quad form: one launch, no workspace, no
// memset.  The bulk route: the counters zeroed, hsv_cmsg_index_kernel, then the
// comb pass of the table width with no strict words; workspace from the
// library pool: counters | k record | hit list.
extern "C" hipError_t hsv_launch_committee_msgs_indexed(const uint32_t *key_idx, const uint8_t *sig,
                                                        uint64_t sig_stride, const uint8_t *msgs,
                                                        const uint64_t *offsets, uint64_t msg_len,
                                                        uint64_t msg_stride, uint32_t n, const uint8_t *pks,
                                                        const uint8_t *key_flags, uint32_t nkeys,
                                                        const uint32_t *const *key_tables, int digit_bits,
                                                        const uint32_t *btable, const uint32_t *comb16,
                                                        uint8_t *flags_out, uint32_t *fault, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const int mode = g_cmsg_indexed_form.load();
  if (n > (1u << 22) || (digit_bits != 8 && digit_bits != 4) || (mode == 1 && digit_bits != 8) || !key_idx || !sig ||
      !flags_out || !btable || !comb16 || !fault || (nkeys && (!pks || !key_flags || !key_tables)))
    return hipErrorInvalidValue;
  if (nkeys == 0) return hipMemsetAsync(flags_out, 0, n, stream);  // no member: every index is out of range
  const uint32_t inject = (uint32_t)hsvi_inject_mode();
  if (digit_bits == 8 && (mode == 1 || (mode < 0 && n <= hsv::kCombQuadMax))) {
    g_cmsg_indexed_quads.fetch_add(1);
    hipLaunchKernelGGL(hsv::hsv_cmsg_quad_kernel, dim3((n + hsv::kFusedVotes - 1) / hsv::kFusedVotes),
                       dim3(hsv::kFusedThreads), 0, stream, key_idx, sig, sig_stride, msgs, offsets, msg_len,
                       msg_stride, n, pks, key_flags, nkeys, key_tables, btable, flags_out, inject, fault);
    return hipGetLastError();
  }
  g_cmsg_indexed_rounds.fetch_add(1);
  hsv::RoutedRound r;
  hipError_t e = r.size(n, digit_bits, reinterpret_cast<const void *>(hsv::hsv_cmsg_comb_kernel),
                        reinterpret_cast<const void *>(hsv::hsv_cmsg_comb4_kernel),
                        reinterpret_cast<const void *>(hsv::hsv_cmsg_generic_kernel<4, HSV_HP_WAVES, 16>));
  if (e != hipSuccess) return e;
  r.comb_only();
  const size_t krec_bytes = hsv::up256((size_t)n * 32), hit_bytes = hsv::up256((size_t)n * sizeof(uint2));
  hsv::Workspace ws(nullptr, 0, r.head_bytes() + krec_bytes + hit_bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *p = ws.get();
  hsv::RoutedCounters *ctr = reinterpret_cast<hsv::RoutedCounters *>(p);
  uint32_t *krec = reinterpret_cast<uint32_t *>(p += r.head_bytes());
  uint2 *hit_list = reinterpret_cast<uint2 *>(p += krec_bytes);
  e = hsv::RoutedRound::zero(ctr, nullptr, n, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hsv::hsv_cmsg_index_kernel, dim3((n + hsv::kMsgBlock - 1) / hsv::kMsgBlock),
                       dim3(hsv::kMsgBlock), 0, stream, key_idx, sig, sig_stride, msgs, offsets, msg_len, msg_stride, n,
                       pks, nkeys, ctr, hit_list, krec, flags_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(r.pick(hsv::hsv_cmsg_comb_kernel, hsv::hsv_cmsg_comb4_kernel), dim3(r.grid_c), dim3(256), 0,
                       stream, sig, sig_stride, n, ctr, hit_list, krec, key_flags, nkeys, key_tables,
                       r.pick(btable, comb16), flags_out, (uint32_t *)nullptr, inject, fault);
    e = hipGetLastError();
  }
  return ws.done(e);
}
