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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

#define HSV_SHA_BITOP3 1  // v_bitop3_b32 in the message hash, as hsv_msgs.hip
#include "hsv_internal.h"
#include "hsv_keytab.hpp"
#include "hsv_msgwave.hpp"
#include "hsv_verify_hc.hpp"
#include "hsv_pointpass.hpp"
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
