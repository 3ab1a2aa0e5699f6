// The one-launch latency forms of the generic verifier: what a batch of at
// most kPairMax items runs instead of the two-pass kernels of hsv_kernels.hip
// (DESIGN.md 4a, 4e, 4l).
//
//  hsv_verify_quad_kernel        <= kQuadMax items: one item per block, R and A a wave each
//  hsv_verify_joint_kernel       <= kJointMax: one item per wave, kJointItems per block
//  hsv_verify_row_kernel         <= row_max(): two 16-lane rows per item, kRowItems per block
//  hsv_verify_pair_fused_kernel  <= kPairMax: two lanes per item, kFusedItems per block
//
// All four have one signature, and each is compiled twice: for 32-byte digests
// (hsv_launch_small) and for whole messages (MSG, hsv_launch_small_msgs).  In
// every form one wave of the block runs the items' scalar prepass into an LDS
// record while the other waves decompress R and A and build their tables; the
// steps the forms have in common stand once, above the kernels, where hipcc
// compiled them to the same code.  SmallForm picks the form by n,
// launch_small launches it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hsv_internal.h"
#include "hsv_verify_core.hpp"
#include "hsv_verify_hc.hpp"
#include "hsv_rowpoint.hpp"
#include "hsv_pointpass.hpp"
#include "hsv_msgwave.hpp"

namespace hsv {

// ---- two lanes per item: the even lane of a pair owns R, the odd lane A ----
// A lone wave issues one VALU instruction per 4 clocks whatever its lane
// count, so a QC of 67 or 667 votes costs one verification's instruction
// count end to end.  Each lane of a pair decompresses its own point, builds
// its own table, runs a one-scalar Straus loop (c1 for R, |c0| for A: 34
// windows, 4 doublings + 1 addition) and half of the wide B comb (digits 0-7 /
// 8-15); the two partial sums meet through a lane swap and one addition.  Per
// lane that is one root chain instead of two and half the additions, with the
// same 136 doublings.

// q += sum of comb digits [8h, 8h + 8) of s (CB = 16) or [16h, 16h + 16) (CB = 8)
template <int CB>
__device__ __forceinline__ ge_ext comb_add_b_half(ge_ext q, const uint32_t s[8], const uint32_t *tb, uint32_t h) {
  constexpr int NP = 256 / CB, HALF = NP / 2;
  constexpr int ENT = 1 << (CB - 1);
  uint32_t sr[9];
  recode_add<9, CB, NP>(s, 8, sr);
  HSV_UNROLL
  for (int i = 0; i < 4; ++i) sr[i] = h ? sr[i + 4] : sr[i];  // the upper 128 bits for h = 1
  HSV_NOUNROLL
  for (int j = 0; j < HALF; ++j) {
    const uint32_t cb = sr[0] & ((1u << CB) - 1u);
    HSV_UNROLL
    for (int i = 0; i < 3; ++i) sr[i] = (sr[i] >> CB) | (sr[i + 1] << (32 - CB));
    sr[3] >>= CB;
    const CombPosTab tpb{tb + (uint64_t)(j + (int)h * HALF) * ENT * kCombEntryWords};
    q = ge_add_niels<true>(q, select_niels<CB>(tpb, cb));
  }
  return q;
}

__device__ __forceinline__ fe fe_swap_pair(const fe &a) {
  fe r;
  HSV_UNROLL
  for (int i = 0; i < kFeLimbs; ++i) r.v[i] = (uint32_t)__shfl_xor((int)a.v[i], 1, 64);
  return r;
}

// Pair-lane point pass of a prepped (non-fallback) item, in two phases; both
// lanes of the pair return the item's flag byte.  p = lane parity: 0 owns R,
// 1 owns A.  Phase 1 needs only the point: decompression and its table.
template <int WA, class VT>
__device__ __forceinline__ void pair_point_phase(uint32_t p, const uint32_t pk[8], const uint32_t rb[8], VT &vt,
                                                 uint32_t &ok, uint32_t &small) {
  constexpr int TS = 1 << (WA - 1);
  uint32_t pt[8];
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) pt[i] = p ? pk[i] : rb[i];
  fe x, y;
  ok = ge_decompress(pt, x, y);
  small = ok & y_is_small_order(y);
  vt_build<TS>(vt, 0, fe_carry(fe_neg(x)), y);
}

// Phase 2: the scalars from the prepass record (word j of the item at
// rec[j * stride]), one-scalar Straus, half of the B comb, the lane swap.
template <int WA, int CB, class VT>
__device__ __forceinline__ uint32_t pair_scalar_phase(uint32_t p, uint32_t ok, uint32_t small, const uint32_t *rec,
                                                      uint64_t stride, uint32_t meta, const uint32_t *tb, VT &vt) {
  using G = HalfCombWindows<WA>;
  uint32_t d[1][5];
  HSV_UNROLL
  for (int i = 0; i < 5; ++i) d[0][i] = rec[(uint64_t)(i + 5 * (int)p) * stride];
  ge_ext q = straus_vt<WA, G::NW, 5, 1, false>(d, vt, (p && (meta & kPrepC0Neg)) ? 1u : 0u);
  uint32_t b[8];
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) b[i] = rec[(10 + i) * stride];
  q = comb_add_b_half<CB>(q, b, tb, p);
  ge_ext o;
  o.X = fe_swap_pair(q.X);
  o.Y = fe_swap_pair(q.Y);
  o.Z = fe_swap_pair(q.Z);
  o.T = fe_swap_pair(q.T);
  q = ge_add_cached_rt(q, ge_to_cached(o), false);
  // (tried: this exchange as one helper with the row form's; 126 lines differ, one v_cmp and four v_cndmask re-encoded)
  const uint32_t ok_o = (uint32_t)__shfl_xor((int)ok, 1, 64), small_o = (uint32_t)__shfl_xor((int)small, 1, 64);
  const uint32_t r_ok = p ? ok_o : ok, small_r = p ? small_o : small;
  const uint32_t a_ok = p ? ok : ok_o, small_a = p ? small : small_o;
  const uint32_t same = ge_is_neutral(q);
  return flags_byte(meta & kPrepSOk, a_ok, r_ok, small_a, small_r, same) | fault_bit(a_ok, r_ok, q);
}

// ---- what the four kernels share ---------------------------------------------
// MSG = false (the 32-byte-digest path): the prepass role hashes R || A || the
// 32 bytes at msg + i * msg_stride.  MSG = true (messages of any length): the
// kernel takes a MsgRange in place of msg, its prepass role hashes each item's
// whole message and the point roles never read a message byte: a fallback
// item's k mod l comes from the b words of its LDS record (verify_fallback_item),
// and an item the prepass marked kPrepVoid (a decreasing pair of offsets) gets
// flags 0, no strict bit, and no share of the helper waves' work.  Everything
// else -- canaries, injection, self-checks, stores -- is one code for both.
struct MsgRange {
  const uint8_t *msgs;
  const uint64_t *offsets;  // n + 1 of them, or null: msg_len bytes at msgs + i * msg_stride
  uint64_t msg_len;
};
template <bool MSG>
using SmallMsgArg = std::conditional_t<MSG, MsgRange, const uint8_t *__restrict__>;
// metas whose item takes no part in the half-size scalar phase
template <bool MSG>
constexpr uint32_t kPrepNoScalars = MSG ? (kPrepFallback | kPrepVoid) : kPrepFallback;

// The prepass role: ITEMS items from `base` on, item base + l on lane l, records
// to srec (SoA, row stride ITEMS).  Digests: the lanes that own an item work
// alone.  Messages: ALL 64 LANES of the wave must call this, because
// msg_hash_lane shuffles, votes and stages the wave's loads cooperatively.  A
// lane that owns no item hashes one of its own block again (base + lane % ITEMS,
// clamped to n - 1) and stores nothing, so the wave-uniform fast paths are
// decided by the block's real items, the trip count is the block's longest
// message, and no lane reads outside a message of the block.
template <int WA, uint32_t ITEMS, bool MSG>
__device__ __forceinline__ void small_prepass(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                              uint64_t sig_stride, const SmallMsgArg<MSG> &msg, uint64_t msg_stride,
                                              uint32_t base, uint32_t n, uint32_t lane, uint32_t *srec, int lat_bits) {
  static_assert(ITEMS >= 1 && ITEMS <= 64, "one lane per item of the block");
  if constexpr (MSG) {
    __shared__ uint4 stage[64 * kMsgQ];
    const uint32_t own = base + lane % ITEMS;
    const uint32_t li = own < n ? own : n - 1u;
    uint32_t hw[16], s[8];
    const bool ok = msg_hash_lane(pk, pk_stride, sig, sig_stride, msg.msgs, msg.offsets, msg.msg_len, msg_stride, li,
                                  lane, stage, hw);
    load_words8(sig + (uint64_t)li * sig_stride + 32, s);
    if (lane < ITEMS) (void)prep_from_hash<WA, PutPlain, true>(hw, s, srec + lane, ITEMS, lat_bits, !ok);
  } else if (lane < ITEMS) {
    const uint32_t li = base + lane < n ? base + lane : n - 1u;
    uint32_t pkw[8], sigw[16], msgw[8];
    load_triple(pk, pk_stride, sig, sig_stride, msg, msg_stride, li, pkw, sigw, msgw);
    (void)prep_scalars<WA>(pkw, sigw, msgw, srec + lane, ITEMS, lat_bits);
  }
}

// The canary protocol of a workspace slot (hsv_pointpass.hpp, report_faults):
// the slot's owner stores the launch's nonce when it starts -- the inverse
// under kInjectCanary, which the closing compare must then report -- and ends
// with its self-check bits (1: a final point or a carry chain) and the compare.
__device__ __forceinline__ uint32_t canary_start(uint32_t nonce, uint32_t inject) {
  return inject == kInjectCanary ? ~nonce : nonce;
}
__device__ __forceinline__ void report_slot_faults(uint32_t *fault, uint32_t bad, const uint32_t *canary,
                                                   uint32_t slot, uint32_t nonce) {
  report_faults(fault, bad | (canary[slot] != nonce ? 2u : 0u));
}

// ---- pair form ------------------------------------------------------------------
// A block of three waves takes 64 items.  Waves 0 and 1 run the pair lanes'
// point phase (decompress R or A, build its table) while wave 2 runs the scalar
// prepass of the same 64 items (SHA-512, k mod l, lattice reduction, recoding)
// into an LDS record.  The waves run on different SIMDs, so the prepass's
// latency hides behind the root chains; after the barrier the pair waves read
// their scalars from LDS.  Fallback items run the full-length path on both
// lanes of their pair.  (Round 1 ran the prepass and the pair lanes as two
// launches, hsv_verify_pair_kernel; it is in git history at d5207a5.)
constexpr int kFusedItems = 64;
template <int WA, int CB, bool MSG = false>
__global__ void __launch_bounds__(3 * 64)
hsv_verify_pair_fused_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                             uint64_t sig_stride, SmallMsgArg<MSG> msg, uint64_t msg_stride, uint32_t n,
                             uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits,
                             uint4 *__restrict__ vt_ws, const uint32_t *__restrict__ comb_b, int lat_bits,
                             uint32_t *__restrict__ canary, uint32_t nonce, uint32_t inject,
                             uint32_t *__restrict__ fault) {
  constexpr int kEnt = (1 << (WA - 1)) + 1;
  __shared__ uint32_t srec[kPrepWords * kFusedItems];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t base = blockIdx.x * kFusedItems;
  const uint32_t t = threadIdx.x;  // pair lanes: t < 128
  const uint32_t p = t & 1u, item = base + (t >> 1);
  const uint32_t slot = blockIdx.x * 2u * kFusedItems + (t & 127u);
  GlobalVarTab<kEnt> vt{vt_ws + (uint64_t)slot * vt_lane_uint4<WA>(), inject};
  if (wave < 2) canary[slot] = canary_start(nonce, inject);
  uint32_t ok = 0, small = 0;
  if (wave == 2) {
    small_prepass<WA, kFusedItems, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, base, n, lane, srec,
                                        lat_bits);
  } else {
    const uint32_t li = item < n ? item : n - 1u;
    uint32_t pkw[8], rw[8];
    load_words8(pk + (uint64_t)li * pk_stride, pkw);
    load_words8(sig + (uint64_t)li * sig_stride, rw);
    pair_point_phase<WA>(p, pkw, rw, vt, ok, small);
  }
  __syncthreads();
  if (wave == 2) return;
  const uint32_t il = t >> 1;
  const uint32_t meta = srec[(kPrepWords - 1) * kFusedItems + il];
  uint32_t f;
  const uint32_t li = item < n ? item : n - 1u;
  if (meta & kPrepFallback) {
    f = verify_fallback_item<WA, CB, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, li, srec + il,
                                          kFusedItems, comb_b, vt);
  } else {
    // (a void item's record holds the scalars of the empty message: computed and discarded)
    f = pair_scalar_phase<WA, CB>(p, ok, small, srec + il, kFusedItems, meta, comb_b, vt);
  }
  report_slot_faults(fault, (f & kFault) ? 1u : 0u, canary, slot, nonce);
  if constexpr (MSG) f = (meta & kPrepVoid) ? 0u : f;
  if (item < n && p == 0u) store_verdict(flags_out, strict_bits, item, f);
}

// ---- row form -------------------------------------------------------------------
// Every field product of a verification spread over a 16-lane DPP row
// (hsv_rowpoint.hpp), two rows per item as the pair form's two lanes.  A block
// of four waves takes kRowItems items: waves 0-2 hold 12 rows (row 2i
// decompresses R of item i and builds [0..8](-R), row 2i + 1 the same for A,
// tables in LDS) while wave 3 runs the scalar prepass of the block's items into
// an LDS record.  After the barrier each row runs its one-scalar Straus (c1 for
// R, |c0| for A) and half of the B comb; the two rows of an item swap their
// sums (lane ^ 16) and add them.  Fallback items run the full-length one-lane
// path on lane 0 of their R row.  Same flags, self-checks and canaries as the
// pair form.
// (Round 3 also spread every element over a pair of rows here, RowLane2, three
// items per block: its range went to the joint form in round 5, 0.178-0.182
// against 0.130-0.134 ms up to 768 items, profiles/r05l_cutover.txt; the
// kernel's RR parameter is in git history at d5207a5.)
constexpr int kRowRows = 12;
constexpr int kRowItems = kRowRows / 2;
template <int WA, int CB, bool MSG = false>
__global__ void __launch_bounds__(4 * 64)
hsv_verify_row_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                      uint64_t sig_stride, SmallMsgArg<MSG> msg, uint64_t msg_stride, uint32_t n,
                      uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits,
                      uint4 *__restrict__ vt_ws, const uint32_t *__restrict__ comb_b, int lat_bits,
                      uint32_t *__restrict__ canary, uint32_t nonce, uint32_t inject, uint32_t *__restrict__ fault) {
  using G = HalfCombWindows<WA>;
  constexpr int TS = 1 << (WA - 1);
  constexpr int kEnt = TS + 1;
  __shared__ uint32_t srec[kPrepWords * kRowItems];
  __shared__ uint32_t stab[kRowRows * kEnt * 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t base = blockIdx.x * kRowItems;
  if (wave == 3) {
    small_prepass<WA, (uint32_t)kRowItems, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, base, n, lane, srec,
                                                lat_bits);
    __syncthreads();
    return;
  }
  const RowLane L;
  const uint32_t rb = wave * 4u + (lane >> 4);  // row of the block
  const uint32_t il = rb >> 1, role = rb & 1u;  // role 0: R, 1: A
  const uint32_t item = base + il;
  const uint32_t li = item < n ? item : n - 1u;
  const uint32_t slot = blockIdx.x * (uint32_t)kRowRows + rb;
  canary[slot] = canary_start(nonce, inject);
  uint32_t ok, small, nc = 0;
  uint32_t *tab = stab + rb * (uint32_t)(kEnt * 64);
  {
    uint32_t enc[8];
    load_words8(role ? pk + (uint64_t)li * pk_stride : sig + (uint64_t)li * sig_stride, enc);
    fe x, y;
    ok = ge_decompress_row(enc, x, y, small, nc, L);
    small &= ok;
    row_table_build<TS>(tab, x, y, L, inject, role == 0u);
  }
  __syncthreads();
  const uint32_t meta = srec[(kPrepWords - 1) * kRowItems + il];
  uint32_t f = 0, bad = 0;
  if (meta & kPrepFallback) {
    if (role == 0u && L.k == 0u) {
      GlobalVarTab<kEnt> vt{vt_ws + (uint64_t)slot * vt_lane_uint4<WA>(), inject};
      f = verify_fallback_item<WA, CB, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, li, srec + il,
                                            kRowItems, comb_b, vt);
      bad = (f & kFault) ? 1u : 0u;
    }
  } else {
    // (a void item's record holds the scalars of the empty message: computed and discarded)
    uint32_t d[5];
    HSV_UNROLL
    for (int i = 0; i < 5; ++i) d[i] = srec[(i + 5 * (int)role) * kRowItems + il];
    rp_ext q = row_straus<WA, G::NW>(d, tab, (role && (meta & kPrepC0Neg)) ? 1u : 0u, L);
    uint32_t b[8];
    HSV_UNROLL
    for (int i = 0; i < 8; ++i) b[i] = srec[(10 + i) * kRowItems + il];
    q = row_comb_half<CB>(q, b, comb_b, role, L);
    // both rows of the item end with the whole sum Q
    q = rp_add_cached(q, rp_to_cached(rp_swap_rows(q, 16), fl_from_fe(fe_d2(), L), L), false, L);
    // (tried: this exchange as one helper with the pair form's, 38,861 / 38,082 instructions against 38,858 / 38,081;
    // the ending below as one helper with the quad and joint forms', 38,865 / 38,087)
    const uint32_t ok_o = (uint32_t)__shfl_xor((int)ok, 16, 64);
    const uint32_t small_o = (uint32_t)__shfl_xor((int)small, 16, 64);
    const uint32_t r_ok = role ? ok_o : ok, small_r = role ? small_o : small;
    const uint32_t a_ok = role ? ok : ok_o, small_a = role ? small : small_o;
    ge_ext qe;
    qe.X = fl_to_fe(q.X, L, nc);
    qe.Y = fl_to_fe(q.Y, L, nc);
    qe.Z = fl_to_fe(q.Z, L, nc);
    qe.T = qe.Z;
    uint32_t z_nonzero;
    const uint32_t sane = ge_is_sane_row(qe, z_nonzero);
    const uint32_t same = fe_is_zero(qe.X) & fe_eq(qe.Y, qe.Z) & z_nonzero;  // ge_is_neutral
    f = flags_byte(meta & kPrepSOk, a_ok, r_ok, small_a, small_r, same);
    bad = (a_ok & r_ok & (sane ^ 1u)) ? 1u : 0u;
  }
  report_slot_faults(fault, bad | nc, canary, slot, nonce);
  if constexpr (MSG) f = (meta & kPrepVoid) ? 0u : f;
  if (item < n && role == 0u && L.k == 0u) store_verdict(flags_out, strict_bits, item, f);
}

// ---- quad form (round 5) ------------------------------------------------------------
// One item per block of four waves, one per SIMD.  Waves 0 and 1 hold R and
// A, each as one point per WAVE whose four rows compute the four independent
// products of every formula round at once (hsv_rowpoint.hpp q_*), so a
// doubling costs two row products instead of eight.  Each decompresses its
// point (the two-row chain, run by both row pairs) and builds [0..8](-P) in
// LDS while wave 2 runs the scalar prepass; then each runs its one-scalar
// Straus (c1 for R, |c0| for A) adding only the windows above the low
// kQuadLo.  The helper waves add those low windows over the same tables
// (wave 2 for c1, then the whole wide B comb; wave 3 for |c0|), and the R
// wave adds the three handed-over sums and checks.  Fallback items (no short
// lattice pair) run the full-length one-lane path on lane 0 of the R wave.
// Same flags, self-checks and canaries as the row form.  Kernel 84.4 us at one
// item (95.6 us without the helpers, profiles/r05y_kernel_trace/); phases in
// profiles/r05y_quadclk.txt.  The cut-over: one block per CU at <= 256 items;
// from 257 on some SIMDs would hold two of these lone-issue waves (0.169-0.173
// ms, profiles/r05k_cutover.txt), so larger batches take the joint form below
// (0.129-0.132 ms up to 768 items, profiles/r05x_cutover.txt).
#ifndef HSV_QUAD_MAX  // measurement builds may move the cut-over (tools/row_cutover_probe.py)
#define HSV_QUAD_MAX 256
#endif
constexpr uint32_t kQuadMax = HSV_QUAD_MAX;
// windows of each half-size scalar run by the helper waves (the low 80 bits):
// the point waves keep their 128 doublings but add only the high windows
constexpr int kQuadLo = 20;
#ifdef HSV_QUAD_CLOCKS
// Measurement builds only (tools/build_ab_libs.sh quadclk "-DHSV_QUAD_CLOCKS"):
// lane 0 of each wave of block 0 stamps the 100 MHz clock at fixed points
// (0 entry, 1 decompressed / prepass done, 2 table built, 3 past barrier 1,
// 4 Straus done, 5 wave 2's B comb done, 6 past barrier 2, 7 exit).
__device__ uint64_t g_quad_clk[4][9];  // slot 8: the wave's HW_ID (SIMD_ID in bits 5:4)
#define HSV_QUAD_CLK(w, slot)                                                  \
  do {                                                                         \
    if (blockIdx.x == 0u && (threadIdx.x & 63u) == 0u) {                       \
      g_quad_clk[w][slot] = wall_clock64();                                    \
      if (slot == 0) g_quad_clk[w][8] = __builtin_amdgcn_s_getreg((31 << 11) | 4); \
    }                                                                          \
  } while (0)
#else
#define HSV_QUAD_CLK(w, slot) \
  do {                        \
  } while (0)
#endif
template <int WA, int CB, bool MSG = false>
__global__ void __launch_bounds__(4 * 64)
hsv_verify_quad_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                       uint64_t sig_stride, SmallMsgArg<MSG> msg, uint64_t msg_stride, uint32_t n,
                       uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits,
                       uint4 *__restrict__ vt_ws, const uint32_t *__restrict__ comb_b, int lat_bits,
                       uint32_t *__restrict__ canary, uint32_t nonce, uint32_t inject, uint32_t *__restrict__ fault) {
  using G = HalfCombWindows<WA>;
  constexpr int TS = 1 << (WA - 1);
  constexpr int kEnt = TS + 1;
  __shared__ uint32_t srec[kPrepWords];
  __shared__ uint32_t stab[2][kEnt * 64];
  __shared__ uint32_t sq_a[4 * 16];     // the A wave's sum, cached form (component r on row r)
  __shared__ uint32_t sq_h[2][4 * 16];  // the helpers' sums: [c1_lo](-R) + [b]B, [c0_lo](-A)
  __shared__ uint32_t s_a[2];           // the A wave's ok, small
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t item = blockIdx.x;
  const uint32_t li = item < n ? item : n - 1u;
  HSV_QUAD_CLK(wave, 0);
  if (wave >= 2) {
    // helpers: wave 2 runs the scalar prepass (a digest on lane 0 alone; every
    // lane hashes the block's one message); after the tables are built, each
    // helper adds the low kQuadLo windows of one scalar over its table (wave
    // 2: c1 over -R, then the whole wide B comb over b; wave 3: |c0| over -A)
    // while the point waves run the high windows
    if (wave == 2u)
      small_prepass<WA, 1u, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, item, n, lane, srec, lat_bits);
    HSV_QUAD_CLK(wave, 1);
    __syncthreads();
    HSV_QUAD_CLK(wave, 3);
    const uint32_t meta = srec[kPrepWords - 1];
    if (!(meta & kPrepNoScalars<MSG>)) {
      const QuadLane L;
      const uint32_t h = wave - 2u;  // 0: R, 1: A
      uint32_t d[5];
      HSV_UNROLL
      for (int i = 0; i < 5; ++i) d[i] = srec[i + 5 * (int)h];
      qp_ext q = quad_straus_low<WA, G::NW, kQuadLo>(d, stab[h], (h && (meta & kPrepC0Neg)) ? 1u : 0u, L);
      HSV_QUAD_CLK(wave, 4);
      if (h == 0u) {
        uint32_t b[8];
        HSV_UNROLL
        for (int i = 0; i < 8; ++i) b[i] = srec[10 + i];
        HSV_NOUNROLL
        for (uint32_t half = 0; half < 2u; ++half) q = quad_comb_half<CB>(q, b, comb_b, half, L);
      }
      sq_h[h][L.r * 16u + L.k] = q_cached_component(q, fl_from_fe(fe_d2(), L), L);
    }
    HSV_QUAD_CLK(wave, 5);
    __syncthreads();
    HSV_QUAD_CLK(wave, 6);
    return;
  }
  const uint32_t role = wave;  // 0: R, 1: A
  const uint32_t slot = blockIdx.x * 2u + role;
  if (lane == 0u) canary[slot] = canary_start(nonce, inject);
  uint32_t ok, small, nc = 0;
  uint32_t *tab = stab[role];
  {
    const RowLane2 L2;
    uint32_t enc[8];
    load_words8(role ? pk + (uint64_t)li * pk_stride : sig + (uint64_t)li * sig_stride, enc);
    fe x, y;
    ok = ge_decompress_row(enc, x, y, small, nc, L2);  // both row pairs, the same chain
    small &= ok;
    HSV_QUAD_CLK(role, 1);
    const QuadLane L;
    quad_table_build<TS>(tab, x, y, L, inject, role == 0u);
    HSV_QUAD_CLK(role, 2);
  }
  __syncthreads();
  HSV_QUAD_CLK(role, 3);
  const QuadLane L;
  const uint32_t meta = srec[kPrepWords - 1];
  uint32_t f = 0, bad = 0;
  qp_ext q{};
  if (!(meta & kPrepNoScalars<MSG>)) {
    uint32_t d[5];
    HSV_UNROLL
    for (int i = 0; i < 5; ++i) d[i] = srec[i + 5 * (int)role];
    q = quad_straus<WA, G::NW, kQuadLo>(d, tab, (role && (meta & kPrepC0Neg)) ? 1u : 0u, L);
    HSV_QUAD_CLK(role, 4);
    if (role == 1u) {
      sq_a[L.r * 16u + L.k] = q_cached_component(q, fl_from_fe(fe_d2(), L), L);
      if (lane == 0u) {
        s_a[0] = ok;
        s_a[1] = small;
      }
    }
  }
  __syncthreads();
  HSV_QUAD_CLK(role, 6);
  if (role == 1u) {
    report_slot_faults(fault, nc, canary, slot, nonce);
    return;
  }
  if (meta & kPrepFallback) {
    if (lane == 0u) {
      GlobalVarTab<kEnt> vt{vt_ws + (uint64_t)slot * vt_lane_uint4<WA>(), inject};
      if constexpr (MSG) {
        f = verify_fallback_item<WA, CB, true>(pk, pk_stride, sig, sig_stride, msg, msg_stride, li, srec, 1, comb_b,
                                               vt);
      } else {  // (tried: verify_fallback_item here too; the digest twin came out 39,630 instructions against 39,629)
        uint32_t pkw[8], sigw[16], msgw[8];
        load_triple(pk, pk_stride, sig, sig_stride, msg, msg_stride, li, pkw, sigw, msgw);
        f = verify_one_full_comb<WA, false, CB>(pkw, sigw, msgw, comb_b, vt);
      }
      bad = (f & kFault) ? 1u : 0u;
    }
  } else if (MSG && (meta & kPrepVoid)) {
    // a void item: no wave ran its scalar phase, nothing was handed over; f = 0
  } else {
    // Q = the R wave's sum + the A wave's + the helpers' (cached forms from LDS)
    q = q_add_op(q, q_op_of_cached(sq_a, L), L);
    q = q_add_op(q, q_op_of_cached(sq_h[0], L), L);
    q = q_add_op(q, q_op_of_cached(sq_h[1], L), L);
    const uint32_t a_ok = s_a[0], small_a = s_a[1];
    // (tried: this ending as one helper with the row and joint forms', 39,626 / 38,880 instructions against
    // 39,629 / 38,883)
    ge_ext qe;
    qe.X = fl_to_fe(q.X, L, nc);
    qe.Y = fl_to_fe(q.Y, L, nc);
    qe.Z = fl_to_fe(q.Z, L, nc);
    qe.T = qe.Z;
    uint32_t z_nonzero;
    const uint32_t sane = ge_is_sane_row(qe, z_nonzero);
    const uint32_t same = fe_is_zero(qe.X) & fe_eq(qe.Y, qe.Z) & z_nonzero;  // ge_is_neutral
    f = flags_byte(meta & kPrepSOk, a_ok, ok, small_a, small, same);
    bad = (a_ok & ok & (sane ^ 1u)) ? 1u : 0u;
  }
  report_slot_faults(fault, bad | nc, canary, slot, nonce);
  if (item < n && lane == 0u) store_verdict(flags_out, strict_bits, item, f);
  HSV_QUAD_CLK(0, 7);
}

// ---- joint quad form --------------------------------------------------------------
// One item per WAVE, kJointItems point waves and one prepass wave per block, so
// 768 items still hold one block per CU and one wave per SIMD.  The point
// wave decompresses R on rows 0-1 and A on rows 2-3 at once (the two-row
// chain, each pair its own element), builds both tables [0..8](-R),
// [0..8](-A) in LDS with the quad formulas, then runs one two-scalar Straus
// (shared doublings, quad_straus2) over all but the low kJointLo windows; the
// prepass wave adds each item's low windows and its wide B comb meanwhile and
// hands the sum over in LDS.  Same flags, fallback, self-checks
// and canaries as the quad form.
constexpr uint32_t kJointItems = 3;
// windows of both scalars the prepass wave adds for each item after its
// prepasses (the low 28 bits): it finishes its three items' shares about when
// the point waves finish the rest
constexpr int kJointLo = 7;
#ifndef HSV_JOINT_MAX  // measurement builds may move the cut-over (tools/row_cutover_probe.py)
#define HSV_JOINT_MAX 768
#endif
constexpr uint32_t kJointMax = HSV_JOINT_MAX;
template <int WA, int CB, bool MSG = false>
__global__ void __launch_bounds__((kJointItems + 1) * 64)
hsv_verify_joint_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                        uint64_t sig_stride, SmallMsgArg<MSG> msg, uint64_t msg_stride, uint32_t n,
                        uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits,
                        uint4 *__restrict__ vt_ws, const uint32_t *__restrict__ comb_b, int lat_bits,
                        uint32_t *__restrict__ canary, uint32_t nonce, uint32_t inject, uint32_t *__restrict__ fault) {
  using G = HalfCombWindows<WA>;
  constexpr int TS = 1 << (WA - 1);
  constexpr int kEnt = TS + 1;
  constexpr uint32_t K = kJointItems;
  __shared__ uint32_t srec[kPrepWords * K];
  __shared__ uint32_t stab[K][2][kEnt * 64];
  __shared__ uint32_t sq_b[K][4 * 16];  // each item's low windows + [b]B, cached form (component r on row r)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t base = blockIdx.x * K;
  if (wave == K) {
    // the items' scalar prepasses on lanes 0..K-1, then each item's whole
    // wide B comb (16 additions) while the point waves run their Straus loops
    small_prepass<WA, K, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, base, n, lane, srec, lat_bits);
    __syncthreads();
    const QuadLane L;
    const uint32_t d2 = fl_from_fe(fe_d2(), L);
    HSV_NOUNROLL
    for (uint32_t t = 0; t < K; ++t) {
      const uint32_t meta_t = srec[(kPrepWords - 1) * K + t];
      if (meta_t & kPrepNoScalars<MSG>) continue;
      // the low kJointLo windows of the item's two scalars over its tables,
      // then its whole wide B comb onto that sum
      uint32_t d1[5], d0[5], b[8];
      HSV_UNROLL
      for (int i = 0; i < 5; ++i) {
        d1[i] = srec[i * K + t];
        d0[i] = srec[(5 + i) * K + t];
      }
      HSV_UNROLL
      for (int i = 0; i < 8; ++i) b[i] = srec[(10 + i) * K + t];
      qp_ext qb = quad_straus2_low<WA, G::NW, kJointLo>(d1, d0, stab[t][0], stab[t][1],
                                                         (meta_t & kPrepC0Neg) ? 1u : 0u, L);
      HSV_NOUNROLL
      for (uint32_t h = 0; h < 2u; ++h) qb = quad_comb_half<CB>(qb, b, comb_b, h, L);
      sq_b[t][L.r * 16u + L.k] = q_cached_component(qb, d2, L);
    }
    __syncthreads();
    return;
  }
  const uint32_t item = base + wave;
  const uint32_t li = item < n ? item : n - 1u;
  const uint32_t slot = blockIdx.x * K + wave;
  if (lane == 0u) canary[slot] = canary_start(nonce, inject);
  uint32_t ok, small, nc = 0;  // rows 0-1: R's, rows 2-3: A's
  uint32_t *tab_r = stab[wave][0], *tab_a = stab[wave][1];
  {
    const RowLane2 L2;
    const uint32_t role = lane >> 5;  // 0: R, 1: A
    uint32_t enc[8];
    load_words8(role ? pk + (uint64_t)li * pk_stride : sig + (uint64_t)li * sig_stride, enc);
    fe x, y;
    ok = ge_decompress_row(enc, x, y, small, nc, L2);  // each row pair its own element
    small &= ok;
    const QuadLane L;
    HSV_NOUNROLL
    for (uint32_t t = 0; t < 2u; ++t) {
      // element t (rows 2t, 2t + 1) on every row: v_permlane32_swap puts the
      // lower half's value in result 0 and the upper half's in result 1
      fe xt, yt;
      HSV_UNROLL
      for (int l = 0; l < kFeLimbs; ++l) {
        const auto px = __builtin_amdgcn_permlane32_swap(x.v[l], x.v[l], false, false);
        const auto py = __builtin_amdgcn_permlane32_swap(y.v[l], y.v[l], false, false);
        xt.v[l] = t ? px[1] : px[0];
        yt.v[l] = t ? py[1] : py[0];
      }
      quad_table_build<TS>(t ? tab_a : tab_r, xt, yt, L, inject, t == 0u);
    }
  }
  __syncthreads();
  const QuadLane L;
  const uint32_t meta = srec[(kPrepWords - 1) * K + wave];
  const uint32_t r_ok = __builtin_amdgcn_readlane(ok, 0), small_r = __builtin_amdgcn_readlane(small, 0);
  const uint32_t a_ok = __builtin_amdgcn_readlane(ok, 32), small_a = __builtin_amdgcn_readlane(small, 32);
  uint32_t f = 0, bad = 0;
  qp_ext q{};
  if (!(meta & kPrepNoScalars<MSG>)) {
    uint32_t d1[5], d0[5];
    HSV_UNROLL
    for (int i = 0; i < 5; ++i) {
      d1[i] = srec[i * K + wave];
      d0[i] = srec[(5 + i) * K + wave];
    }
    q = quad_straus2<WA, G::NW, kJointLo>(d1, d0, tab_r, tab_a, (meta & kPrepC0Neg) ? 1u : 0u, L);
  }
  __syncthreads();  // the prepass wave's [b]B
  if (meta & kPrepFallback) {
    if (lane == 0u) {
      GlobalVarTab<kEnt> vt{vt_ws + (uint64_t)slot * vt_lane_uint4<WA>(), inject};
      f = verify_fallback_item<WA, CB, MSG>(pk, pk_stride, sig, sig_stride, msg, msg_stride, li, srec + wave, K,
                                            comb_b, vt);
      bad = (f & kFault) ? 1u : 0u;
    }
  } else if (MSG && (meta & kPrepVoid)) {
    // a void item: neither wave ran its scalar phase, nothing was handed over; f = 0
  } else {
    q = q_add_op(q, q_op_of_cached(sq_b[wave], L), L);
    // (tried: this ending as one helper with the row and quad forms', 39,527 / 38,763 instructions against
    // 39,530 / 38,766)
    ge_ext qe;
    qe.X = fl_to_fe(q.X, L, nc);
    qe.Y = fl_to_fe(q.Y, L, nc);
    qe.Z = fl_to_fe(q.Z, L, nc);
    qe.T = qe.Z;
    uint32_t z_nonzero;
    const uint32_t sane = ge_is_sane_row(qe, z_nonzero);
    const uint32_t same = fe_is_zero(qe.X) & fe_eq(qe.Y, qe.Z) & z_nonzero;  // ge_is_neutral
    f = flags_byte(meta & kPrepSOk, a_ok, r_ok, small_a, small_r, same);
    bad = (a_ok & r_ok & (sane ^ 1u)) ? 1u : 0u;
  }
  report_slot_faults(fault, bad | nc, canary, slot, nonce);
  if (item < n && lane == 0u) store_verdict(flags_out, strict_bits, item, f);
}

}  // namespace hsv

namespace {

// The row form at or below this many items.  p50 of a generic call, row /
// pair form (tools/row_cutover_probe.py, profiles/r03zp_row_cutover.txt):
// 0.216 / 0.450 ms at 64 items, 0.226 / 0.466 at 1024, 0.230 / 0.467 at 1536
// (256 blocks of four waves: one block per CU), 0.422 / 0.470 at 2048, 0.427 /
// 0.477 at 3072, 0.626 / 0.487 at 4096.
constexpr uint32_t kRowMaxDefault = 3072;
constexpr uint32_t row_max() { return kRowMaxDefault; }

// The small form n <= kPairMax items take (hsv_internal.h; at 2^12 items the
// pair form is 27 % faster end to end than the two-pass point pass, at 2^15
// 7 % slower, profiles/r01o_qc_latency.json): its kernel, grid, block size and
// workspace slots -- one full-length table and one canary per slot.
//   quad  (<= kQuadMax): one item per block, a slot per point wave;
//   joint (<= kJointMax): kJointItems items per block, a slot per point wave;
//   row   (<= row_max()): kRowItems items per block, a slot per row (the
//         fallback path's tables; the row tables live in LDS);
//   pair  (<= kPairMax): kFusedItems items per block, a slot per pair lane.
// MSG: the message instantiations, the same grids, blocks and slots.  Their
// cut-overs are constants of their own beside the digest path's, set from
// profiles/msgs_small_latency.json: at every measured size and
// length the form chosen here has a p50 no higher than the two-launch form's
// in the same run, so none of them moved.  p50 of a device call + synchronise,
// this form / two launches, 32-byte and ragged 0..1024-byte messages: quad
// 0.117 / 0.693 and 0.192 / 0.767 ms at 256 items; joint 0.127 / 0.694 and
// 0.215 / 0.768 at 257, 0.132 / 0.698 and 0.212 / 0.773 at 768; row 0.212 /
// 0.699 and 0.295 / 0.774 at 769, 0.349 / 0.713 and 0.401 / 0.803 at 3072; pair
// 0.457 / 0.714 and 0.505 / 0.803 at 3073, 0.469 / 0.733 and 0.523 / 0.829 at
// 8192.  The choice depends on n alone: in the device form the lengths live in
// device memory, and a long message costs its one lane the same serial hash in
// either route.  `force` (1 quad, 2 joint, 3 row, 4 pair; 0 = by n) is the test
// library's hsv_test_msgs_small.
constexpr uint32_t kMsgQuadMax = hsv::kQuadMax;
constexpr uint32_t kMsgJointMax = hsv::kJointMax;
constexpr uint32_t kMsgRowMax = kRowMaxDefault;
enum SmallFormId : int { kFormQuad = 1, kFormJoint = 2, kFormRow = 3, kFormPair = 4 };

template <int WA, int CB, bool MSG = false>
struct SmallForm {
  decltype(&hsv::hsv_verify_quad_kernel<WA, CB, MSG>) kern;
  uint32_t grid, block;
  size_t slots;
  int id;
  explicit SmallForm(uint32_t n, int force = 0) {
    id = force                                        ? force
         : n <= (MSG ? kMsgQuadMax : hsv::kQuadMax)   ? kFormQuad
         : n <= (MSG ? kMsgJointMax : hsv::kJointMax) ? kFormJoint
         : n <= (MSG ? kMsgRowMax : row_max())        ? kFormRow
                                                      : kFormPair;
    if (id == kFormQuad) {
      kern = hsv::hsv_verify_quad_kernel<WA, CB, MSG>;
      grid = n, block = 4 * 64, slots = (size_t)grid * 2u;
    } else if (id == kFormJoint) {
      kern = hsv::hsv_verify_joint_kernel<WA, CB, MSG>;
      grid = (n + hsv::kJointItems - 1) / hsv::kJointItems, block = (hsv::kJointItems + 1) * 64;
      slots = (size_t)grid * hsv::kJointItems;
    } else if (id == kFormRow) {
      kern = hsv::hsv_verify_row_kernel<WA, CB, MSG>;
      grid = (n + hsv::kRowItems - 1) / hsv::kRowItems, block = 4 * 64;
      slots = (size_t)grid * hsv::kRowRows;
    } else {
      kern = hsv::hsv_verify_pair_fused_kernel<WA, CB, MSG>;
      grid = (n + hsv::kFusedItems - 1) / hsv::kFusedItems, block = 3 * 64;
      slots = (size_t)grid * 2u * hsv::kFusedItems;
    }
  }
};

// One launch of the form.  Workspace: the slots' tables, then their canaries.
template <int WA, int CB, bool MSG = false>
hipError_t launch_small(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                        hsv::SmallMsgArg<MSG> msg, uint64_t msg_stride, uint32_t n, uint8_t *flags_out,
                        uint32_t *strict_bits, const uint32_t *comb_b, uint32_t *fault, hipStream_t stream,
                        void *ws_in = nullptr, size_t ws_cap = 0, size_t *ws_need = nullptr, int force = 0,
                        int *form_id = nullptr) {
  const SmallForm<WA, CB, MSG> f(n, force);
  if (form_id) *form_id = f.id;
  const size_t ws_bytes = f.slots * hsv::vt_lane_uint4<WA>() * sizeof(uint4);
  const size_t need = ws_bytes + f.slots * sizeof(uint32_t);
  if (ws_need) {  // size query only
    *ws_need = need;
    return hipSuccess;
  }
  hsv::Workspace ws(ws_in, ws_cap, need, stream);
  hipError_t e = ws.status();
  if (e != hipSuccess) return e;
  if (strict_bits) e = hipMemsetAsync(strict_bits, 0, (size_t)((n + 31u) / 32u) * 4u, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(f.kern, dim3(f.grid), dim3(f.block), 0, stream, pk, pk_stride, sig, sig_stride, msg,
                       msg_stride, n, flags_out, strict_bits, reinterpret_cast<uint4 *>(ws.get()), comb_b,
                       hsvi_lattice_bits(), reinterpret_cast<uint32_t *>(ws.get() + ws_bytes), hsvi_next_nonce(),
                       (uint32_t)hsvi_inject_mode(), fault);
    e = hipGetLastError();
  }
  return ws.done(e);
}

}  // namespace

extern "C" hipError_t hsv_launch_small(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                                       const uint8_t *msg, uint64_t msg_stride, uint32_t n, uint8_t *flags_out,
                                       uint32_t *strict_bits, const uint32_t *comb16, uint32_t *fault, void *ws,
                                       size_t ws_cap, hipStream_t stream) {
  return launch_small<4, 16>(pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits, comb16, fault,
                             stream, ws, ws_cap);
}

extern "C" size_t hsv_small_ws_bytes(uint32_t n) {
  size_t need = 0;
  (void)launch_small<4, 16>(nullptr, 0, nullptr, 0, nullptr, 0, n, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, 0, &need);
  return need;
}

extern "C" hipError_t hsv_launch_small_msgs(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                            uint64_t sig_stride, const uint8_t *msgs, const uint64_t *offsets,
                                            uint64_t msg_len, uint64_t msg_stride, uint32_t n, uint8_t *flags_out,
                                            uint32_t *strict_bits, const uint32_t *comb16, uint32_t *fault, int force,
                                            int *form_id, hipStream_t stream) {
  return launch_small<4, 16, true>(pk, pk_stride, sig, sig_stride, hsv::MsgRange{msgs, offsets, msg_len}, msg_stride,
                                   n, flags_out, strict_bits, comb16, fault, stream, nullptr, 0, nullptr, force,
                                   form_id);
}

#ifdef HSV_QUAD_CLOCKS
// Measurement builds only: block 0's stamps of the last quad-form launch (4
// waves x 9 u64, 100 MHz); 0 or -1 on a HIP error.
extern "C" __attribute__((visibility("default"))) int hsv_quad_clocks(uint64_t *out) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(hsv::g_quad_clk), sizeof(hsv::g_quad_clk)) == hipSuccess ? 0 : -1;
}
#endif
