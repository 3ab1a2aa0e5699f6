// Half-size scalars + fixed-base comb for B (the default generic kernel).
//
// Same verification equation as verify_one_half (hsv_verify_core.hpp):
//   EQ_OK  <=>  [c1](-R) + [|c0|](-sign(c0) A) + [b]B == O,
//   (c0, c1) = lattice_reduce(k),  b = (c1 s) mod l,
// evaluated in two phases so the hot loop stays small:
//   1. Straus over the two ~128-bit scalars c1, |c0| (< 2^138): NW windows of WA bits,
//      WA doublings + 2 cached additions per window, entries of the per-lane
//      tables [0..2^(WA-1)](-R), [0..2^(WA-1)](-sign(c0) A) read from memory
//      (VT, one 128-byte line per entry) a window ahead of their use;
//   2. [b]B from the comb table T_B[j][m] = [m 2^(8j)]B (hsv_comb.hpp, built
//      once per device, L2-resident): 32 mixed additions, no doublings.
// Each phase has one copy of its point formula (runtime with_t flag), so the
// window loop is ~3k instructions instead of ~10k and stays in the shared
// instruction cache.  A lane whose lattice reduction fails (~2^-22.6) takes
// verify_one_full_comb: the same two phases with the full-length k.
//
// The throughput point pass (hsv_verify_hp_kernel, the fused transaction
// launch) runs phase 1 over ONE joint table instead (jt_build, straus_joint,
// the JOINT form of verify_one_prepped): the 12 lines i(-R) + j(-A) of the
// sign-folded pairs of signed radix-4 digits in {-1 .. 2}, 70 columns of 2 bits
// with two doublings and one cached addition each -- the same doublings and additions
// per bit, four table lines fewer to build, pack, store and read back.  Its
// prepasses write the record's digits as 2-bit columns (prep_from_hash, DW = 2).
// The latency forms and the committee kernels keep the two 4-bit tables.
#pragma once
#include "hsv_comb.hpp"
#include "hsv_lattice.hpp"
#include "hsv_verify_core.hpp"

namespace hsv {

// q += [s]B for a scalar s < 2^256 (8 words) via a comb table of B: CB = 8,
// the 384 KiB table (32 signed radix-2^8 digits), or CB = 16, the 48 MiB
// wide table (16 signed radix-2^16 digits); digits consumed from the bottom.
// (s >= 2^256 - C is only reached for non-canonical s, whose flags do not
// depend on the equation.)
template <int CB>
HSV_INL ge_ext comb_add_b(ge_ext q, const uint32_t s[8], const uint32_t *tb) {
  static_assert(CB == 8 || CB == 16, "comb digit width");
#ifdef HSV_TIMING_STUB_COMB  // tools/phase_probe.py only
  return q;
#endif
  constexpr int NP = 256 / CB;
  constexpr int ENT = 1 << (CB - 1);
  uint32_t sr[9];
  recode_add<9, CB, NP>(s, 8, sr);
  HSV_NOUNROLL
  for (int j = 0; j < NP; ++j) {
    const uint32_t cb = sr[0] & ((1u << CB) - 1u);
    HSV_UNROLL
    for (int i = 0; i < 8; ++i) sr[i] = (sr[i] >> CB) | (sr[i + 1] << (32 - CB));
    sr[8] >>= CB;
    const CombPosTab tpb{tb + (uint64_t)j * ENT * kCombEntryWords};
    q = ge_add_niels<true>(q, select_niels<CB>(tpb, cb));
  }
  return q;
}

HSV_INL uint32_t flags_byte(uint32_t s_ok, uint32_t a_ok, uint32_t r_ok, uint32_t small_a, uint32_t small_r,
                            uint32_t same) {
  const uint32_t parse_ok = s_ok & a_ok & r_ok;
  const uint32_t eq_ok = parse_ok & same;
  const uint32_t strict_ok = eq_ok & (small_a ^ 1u) & (small_r ^ 1u);
  return (strict_ok ? kStrictOk : 0u) | (eq_ok ? kEqOk : 0u) | (parse_ok ? kParseOk : 0u) |
         (small_a ? kSmallA : 0u) | (small_r ? kSmallR : 0u) | (s_ok ? kSOk : 0u) |
         (a_ok ? kAOk : 0u) | (r_ok ? kROk : 0u);
}

// Straus over NV (1 or 2) variable bases from VT tables 0..NV-1, scalars given
// as recoded digit registers d[v] (L limbs, top window at the top bit).
// Returns the accumulator with T valid (the comb phase follows).
// flip_last: negate every digit of the last scalar (its table holds the
// negated base).
// Leading windows whose digits are zero in every lane of the wave only add
// the identity to the identity and are skipped (wave-uniform: the window
// count is the wave's largest scalar).  The lattice outputs of a 64-lane
// wave fit 131 bits in ~88% of waves, which drops the top window and its
// four doublings (tools/lattice_bits.py).
template <class T>
HSV_INL bool wave_any(T c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(c != 0) != 0;
#else
  return c != 0;
#endif
}

template <int WA, int NW, int L, int NV, bool PREFETCH, class VT>
HSV_INL ge_ext straus_vt(uint32_t d[NV][L], VT &vt, uint32_t flip_last = 0) {
  constexpr int TS = 1 << (WA - 1);
  ge_ext q = ge_identity();
#ifdef HSV_TIMING_STUB_STRAUS  // tools/phase_probe.py only: wrong results, timing share of the window loop
  return q;
#endif
  int top = NW - 1;
  HSV_NOUNROLL
  while (top > 0) {
    uint32_t nz = 0;
    HSV_UNROLL
    for (int v = 0; v < NV; ++v) nz |= (d[v][L - 1] >> (32 - WA)) ^ (uint32_t)TS;
    if (wave_any(nz)) break;
    HSV_UNROLL
    for (int v = 0; v < NV; ++v) limbs_shl<L>(d[v], WA);
    --top;
  }
  HSV_NOUNROLL
  for (int i = top; i >= 0; --i) {
    uint32_t m[NV], neg[NV];
    HSV_UNROLL
    for (int v = 0; v < NV; ++v) {
      m[v] = digit_mag<TS>(d[v][L - 1] >> (32 - WA), neg[v]);
      if (v == NV - 1) neg[v] ^= flip_last;
      limbs_shl<L>(d[v], WA);
    }
    if constexpr (PREFETCH) {
      // both entries in flight during the doublings (2 x 32 registers)
      uint32_t w[NV][32];
      HSV_UNROLL
      for (int v = 0; v < NV; ++v) vt.get(v, m[v], w[v]);
      if (i != top) {
        HSV_NOUNROLL
        for (int j = 0; j < WA; ++j) q = ge_dbl_rt(q, j == WA - 1);
      }
      uint32_t cur[32], cneg = neg[0];
      HSV_UNROLL
      for (int x = 0; x < 32; ++x) cur[x] = w[0][x];
      HSV_NOUNROLL
      for (int v = 0; v < NV; ++v) {
        q = ge_add_cached_rt(q, ge_cached_cneg(cached_unpack(cur), cneg), v + 1 < NV || i == 0);
        if (NV > 1) {
          HSV_UNROLL
          for (int x = 0; x < 32; ++x) cur[x] = w[NV - 1][x];
          cneg = neg[NV - 1];
        }
      }
    } else {
      // entries loaded right before their addition (fewer live registers;
      // latency left to the other waves of the SIMD)
      if (i != top) {
        HSV_NOUNROLL
        for (int j = 0; j < WA; ++j) q = ge_dbl_rt(q, j == WA - 1);
      }
      uint32_t mv = m[0], cneg = neg[0];
      HSV_NOUNROLL
      for (int v = 0; v < NV; ++v) {
        uint32_t cur[32];
        vt.get(v, mv, cur);
        q = ge_add_cached_rt(q, ge_cached_cneg(cached_unpack(cur), cneg), v + 1 < NV || i == 0);
        mv = m[NV - 1];
        cneg = neg[NV - 1];
      }
    }
  }
  return q;
}

// Full-length path (fallback): [k](-A) by Straus with table 0, [s]B by comb,
// compared with R as points (dalek's check, verify_one's flags).  This form
// takes the challenge k = SHA-512(R || A || M) mod l already reduced (the
// any-length message path reads it from the prepass record, hsv_msgs.hip).
template <int WA, bool PREFETCH = true, int CB = 8, class VT>
HSV_INL uint32_t verify_one_full_comb(const uint32_t pk[8], const uint32_t sig[16], const sc &k,
                                      const uint32_t *tb, VT &vt) {
  using G = Windows<WA, WA>;
  const uint32_t s_ok = sc_is_canonical(sig + 8);
  fe ax, ay;
  const uint32_t a_ok = ge_decompress(pk, ax, ay);
  const uint32_t small_a = a_ok & y_is_small_order(ay);
  vt_build<G::TS>(vt, 0, fe_carry(fe_neg(ax)), ay);
  uint32_t d[1][8];
  recode_add<8, WA, G::NA>(k.v, 8, d[0]);
  limbs_shl_const<8, 256 - G::KBITS>(d[0]);
  ge_ext q = straus_vt<WA, G::NA, 8, 1, PREFETCH>(d, vt);
  q = comb_add_b<CB>(q, sig + 8, tb);
  fe rx, ry;
  const uint32_t r_ok = ge_decompress(sig, rx, ry);
  const uint32_t small_r = r_ok & y_is_small_order(ry);
  return flags_byte(s_ok, a_ok, r_ok, small_a, small_r, ge_eq_affine(q, rx, ry)) | fault_bit(a_ok, r_ok, q);
}

// The same for a 32-byte message, hashed here.
template <int WA, bool PREFETCH = true, int CB = 8, class VT>
HSV_INL uint32_t verify_one_full_comb(const uint32_t pk[8], const uint32_t sig[16], const uint32_t msg[8],
                                      const uint32_t *tb, VT &vt) {
  uint32_t h[16];
  sha512_96(sig, pk, msg, h);
  const sc k = sc_reduce512(h);
  return verify_one_full_comb<WA, PREFETCH, CB>(pk, sig, k, tb, vt);
}

template <int WA>
struct HalfCombWindows {
  static constexpr int NW = (kLatCombBits + 1 + WA) / WA;  // c + C_WA < 2^(NW*WA) for c < 2^138
  static constexpr int BITS = NW * WA;
  static_assert(BITS <= 160 && BITS >= kLatCombBits + 2, "scalar bound vs loop length");
};

template <int WA, bool PREFETCH = true, int CB = 8, class VT>
HSV_INL uint32_t verify_one_half_comb(const uint32_t pk[8], const uint32_t sig[16], const uint32_t msg[8],
                                      const uint32_t *tb, VT &vt, bool &fallback, int lat_bits = kLatCombBits) {
  using G = HalfCombWindows<WA>;
  constexpr int TS = 1 << (WA - 1);
  const uint32_t s_ok = sc_is_canonical(sig + 8);
  uint32_t h[16];
  sha512_96(sig, pk, msg, h);
  const sc k = sc_reduce512(h);

  // tables first (R and A are dead afterwards), the lattice reduction after
  // them, so its outputs are not live across the two root chains
  uint32_t a_ok, small_a, r_ok, small_r;
  {
    fe x, y;
    r_ok = ge_decompress(sig, x, y);
    small_r = r_ok & y_is_small_order(y);
    vt_build<TS>(vt, 0, fe_carry(fe_neg(x)), y);
  }
  {
    fe x, y;
    a_ok = ge_decompress(pk, x, y);
    small_a = a_ok & y_is_small_order(y);
    vt_build<TS>(vt, 1, fe_carry(fe_neg(x)), y);  // -A; the sign of c0 flips the digits
  }
  const LatOut lat = lattice_reduce(k, lat_bits);
  fallback = !lat.ok;
  uint32_t d[2][5];
  recode_top5<WA, G::NW>(lat.c1, d[0]);
  recode_top5<WA, G::NW>(lat.c0, d[1]);
  ge_ext q = straus_vt<WA, G::NW, 5, 2, PREFETCH>(d, vt, lat.c0_neg);
  const sc b = sc_mul_small(lat.c1, sig + 8);
  q = comb_add_b<CB>(q, b.v, tb);
  const uint32_t same = ge_is_neutral(q);  // Q == O
  return flags_byte(s_ok, a_ok, r_ok, small_a, small_r, same) | fault_bit(a_ok, r_ok, q);
}

// ---- two-pass form: scalar prepass + point pass ---------------------------
// The prepass (one lane per item) does everything that depends only on the
// scalars: s < l, SHA-512, k mod l, the lattice reduction, the recoded
// digits of c1 and |c0| and b = (c1 s) mod l, and writes them to a
// structure-of-arrays record (word j of item i at rec[j * stride + i]).
// Items without a short pair are flagged there and listed, so the point pass
// can deal them out first: their full-length work then overlaps the bulk of
// the batch instead of trailing it.
constexpr int kPrepWords = 19;  // d(c1)[5] | d(|c0|)[5] | b[8] | meta
enum : uint32_t { kPrepSOk = 1u, kPrepC0Neg = 2u, kPrepFallback = 4u };

// How prep_scalars stores its record words: plain stores here; the fused
// transaction launch (hsv_mempool.hip) passes write-through stores, because
// other workgroups of the same launch read the records.
struct PutPlain {
  static HSV_MEMBER void u32(uint32_t *p, uint32_t v) { *p = v; }
};

// The prepass after the hash: h = the 64 bytes of SHA-512(R || A || M) as 16
// little-endian words, s = the signature's scalar.  k mod l, the lattice
// reduction, the recoding and the record stores.
// lat_bits: the lattice bound (kLatCombBits; lower values only to exercise the
// full-length path in tests, hsvi_set_lattice_bits).
// KREC (the any-length message path, hsv_msgs.hip): the point pass cannot hash
// the message again, so a fallback item's eight b words -- meaningless for it
// -- carry k mod l instead; and an item marked `skip` (its message range is
// malformed) gets the meta word kPrepVoid alone: the point pass answers flags 0.
// DW: the digit width of the record's ten digit words.  DW = WA is the format
// of straus_vt (NW windows of WA bits); DW = 2 the joint point pass's: 70
// columns of signed radix-4 digits chunk - 1 in {-1, 0, 1, 2}, top-aligned in
// the same five words (recode_cols, straus_joint).  Nothing else in the record
// depends on it.
// need (DW = 2 only): where given, the item's column class (col_class), by
// which hsv_verify_hp_kernel deals its batches.
constexpr uint32_t kPrepVoid = 8u;

// ---- 2-bit columns, digits in {-1 .. 2} ---------------------------------------
// The scalars are magnitudes (|c0| >= 0, c1 > 0), so the digit set leans to
// the positive side: m columns of digits in {-1 .. 2} reach 2 (4^m - 1) / 3,
// one bit more than the symmetric {-2 .. 1} of recode_top5<2>, and the
// wave-uniform skip of leading zero columns (straus_joint) drops about half a
// column more per wave (tools/lattice_bits.py).  Adding C = (4^NW - 1) / 3,
// chunks 0b01 .. 01, makes chunk t of the sum the digit plus kColOffset.
constexpr int kColOffset = 1;
HSV_INL constexpr uint32_t col_const_limb(int nw, int j) {
  uint32_t r = 0;
  for (int b = 0; b < 32; b += 2)
    if (32 * j + b < 2 * nw) r |= 1u << b;
  return r;
}
// c < 2^138 gives c + C < 2^138 + 4^70 / 3 < 4^70
static_assert(kLatCombBits + 2 <= HalfCombWindows<2>::BITS && HalfCombWindows<2>::NW == 70,
              "2-bit columns: c < 2^138 plus the recoding constant (4^70 - 1) / 3 must stay below 4^70");
// x (5 limbs) + C over NW columns, the top column at the top bit of 5 limbs
template <int NW>
HSV_INL void recode_cols(const uint32_t x[5], uint32_t out[5]) {
  uint64_t t = 0;
  HSV_UNROLL
  for (int j = 0; j < 5; ++j) {
    t += (uint64_t)x[j] + col_const_limb(NW, j);
    out[j] = (uint32_t)t;
    t >>= 32;
  }
  limbs_shl_const<5, 160 - 2 * NW>(out);
}

// Columns a scalar needs: cols(c) = the smallest m with c <= 2 (4^m - 1) / 3,
// that is 3c < 2 4^m + 1; the recoding's 70 - cols(c) leading digits are zero.
// An item's class is max(cols(|c0|), cols(c1)) clamped to kColNeedMin ..
// kColNeedMax, numbered from the longest: class 0 needs >= 67 columns, class
// kColClasses - 1 at most 62 (64: 52%, 65: 41% of random challenges).
constexpr int kColNeedMin = 62, kColNeedMax = 67, kColClasses = kColNeedMax - kColNeedMin + 1;
// limb j of 2 (4^m - 1) / 3, chunks 0b10
HSV_INL constexpr uint32_t col_reach_limb(int m, int j) { return col_const_limb(m, j) << 1; }
HSV_INL uint32_t col_class(const uint32_t c0[5], const uint32_t c1[5]) {
  uint32_t over = 0;  // thresholds below max(c0, c1)
  HSV_UNROLL
  for (int m = kColNeedMin; m < kColNeedMax; ++m) {
    const uint32_t t[5] = {col_reach_limb(m, 0), col_reach_limb(m, 1), col_reach_limb(m, 2), col_reach_limb(m, 3),
                           col_reach_limb(m, 4)};
    over += (mp_lt<5>(t, c0) || mp_lt<5>(t, c1)) ? 1u : 0u;
  }
  return (uint32_t)(kColClasses - 1) - over;
}

template <int WA, class Put = PutPlain, bool KREC = false, int DW = WA>
HSV_INL bool prep_from_hash(const uint32_t h[16], const uint32_t s[8], uint32_t *rec, uint64_t stride,
                            int lat_bits = kLatCombBits, bool skip = false, uint32_t *need = nullptr) {
  using G = HalfCombWindows<DW>;
  static_assert(DW != 2 || WA != 2, "DW = 2 is the column format; straus_vt's 2-bit windows are not built");
  const uint32_t s_ok = sc_is_canonical(s);
  const sc k = sc_reduce512(h);
  const LatOut lat = lattice_reduce(k, lat_bits);
  if constexpr (DW == 2) {
    if (need) *need = col_class(lat.c0, lat.c1);
  }
  uint32_t d[5];
  if constexpr (DW == 2) recode_cols<G::NW>(lat.c1, d);
  else recode_top5<DW, G::NW>(lat.c1, d);
  HSV_UNROLL
  for (int i = 0; i < 5; ++i) Put::u32(rec + i * stride, d[i]);
  if constexpr (DW == 2) recode_cols<G::NW>(lat.c0, d);
  else recode_top5<DW, G::NW>(lat.c0, d);
  HSV_UNROLL
  for (int i = 0; i < 5; ++i) Put::u32(rec + (5 + i) * stride, d[i]);
  const sc b = sc_mul_small(lat.c1, s);
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) Put::u32(rec + (10 + i) * stride, KREC && !lat.ok ? k.v[i] : b.v[i]);
  const uint32_t meta = (s_ok ? kPrepSOk : 0u) | (lat.c0_neg ? kPrepC0Neg : 0u) | (lat.ok ? 0u : kPrepFallback);
  Put::u32(rec + 18 * stride, KREC && skip ? kPrepVoid : meta);
  return !lat.ok && !(KREC && skip);
}

template <int WA, class Put = PutPlain, int DW = WA>
HSV_INL bool prep_scalars(const uint32_t pk[8], const uint32_t sig[16], const uint32_t msg[8], uint32_t *rec,
                          uint64_t stride, int lat_bits = kLatCombBits, uint32_t *need = nullptr) {
  uint32_t h[16];
  sha512_96(sig, pk, msg, h);
  return prep_from_hash<WA, Put, false, DW>(h, sig + 8, rec, stride, lat_bits, false, need);
}

// Point pass of a prepped item: the half-size equation of
// verify_one_half_comb with the scalars read back from the record.
// `rb` is R (the first 32 bytes of the signature).
// HSV_PHASE_CLOCKS (tools/phase_clock_probe.py only): wall-clock stamps at the
// phase boundaries of the point pass, clk[1..3] after decompression, tables
// and the window loop.
#ifdef HSV_PHASE_CLOCKS
#define HSV_CLK(j)                       \
  do {                                   \
    if (clk) clk[j] = wall_clock64();    \
  } while (0)
#else
#define HSV_CLK(j) \
  do {             \
  } while (0)
#endif

// ---- joint table over 2-bit columns ------------------------------------------
// With P = -R and Q = -A, a column of the two scalars' signed radix-4 digits
// (i, j), j already flipped by the sign of c0, adds iP + jQ: one addition per
// 2 bits from ONE table, where straus_vt spends two per 4 bits from two.  The
// doublings and additions per bit are the same; the table is 12 lines instead
// of 16 and costs 2 doublings + 8 additions to build instead of 2 + 12.
// The record's digits are i in {-1 .. 2} and, after the flip, j in {-2 .. 2}.
// Folded by sign, i in {0, 1, 2} and j in {-2 .. 2} (i = 0: j >= 0): with
// s = 5i + j the line is |s| and the fold is s < 0, since |j| <= 2 < 5 --
//   0 the identity (the shared line), 1, 2 = Q, 2Q, 5i + j the lines with P
//   (3 .. 7 = P - 2Q .. P + 2Q, 8 .. 12 = 2P - 2Q .. 2P + 2Q).
//   VT::put_line(l, const uint32_t w[32])   store line l (1 .. kJointLines)
//   VT::get_line(l, uint32_t w[32])         load it back (0: the identity)
constexpr int kJointLines = 12;
constexpr uint32_t kJointFirstLineOfR = 3;  // lines below hold multiples of Q alone

HSV_INL uint32_t joint_line(int i, int j, uint32_t &neg) {
  const int s = 5 * i + j;
  neg = s < 0;
  return (uint32_t)(s < 0 ? -s : s);
}

// a column's line and fold from the two scalars' 2-bit chunks (digit =
// chunk - OFF); flip: c0 < 0, the digit of |c0| changes sign.  OFF =
// kColOffset is the record's format: i = -1 folds to the lines 3 .. 7
// (s = -5 + j < 0) and i = -2 does not occur.  OFF = 2 is the symmetric set of
// recode_top5<2>; the table serves both.
template <int OFF = 2>
HSV_INL uint32_t joint_column(uint32_t ci, uint32_t cj, uint32_t flip, uint32_t &neg) {
  static_assert(OFF == 1 || OFF == 2, "digits in {-1 .. 2} or {-2 .. 1}");
  const int j = (int)cj - OFF;
  return joint_line((int)ci - OFF, flip ? -j : j, neg);
}

template <class VT>
HSV_INL void jt_put(VT &vt, uint32_t line, const ge_ext &p) {
  uint32_t w[32];
  cached_pack(ge_to_cached(p), w);
  vt.put_line(line, w);
}

// Lines ls <- P + Q and ld <- P - Q for a cached Q.  The sum's and the
// difference's cross products differ; C = T1 2dT2 and D = Z1 2Z2 are shared,
// with F and G swapped for the difference.  Operand classes as
// ge_add_cached_rt.  All six products come first and the sum is stored before
// the difference is finished, so that neither Q nor the sum stays live.
template <class VT>
HSV_INL void jt_pair(VT &vt, const ge_ext &p, const ge_cached &q, uint32_t ls, uint32_t ld) {
  const fe a = fe_sub(p.Y, p.X), b = fe_add(p.Y, p.X);
  fe A, B, A2, B2, C, D;
  fe_mul2(p.T, q.T2d, p.Z, q.Z2, C, D);
  fe_mul2(a, q.YmX, b, q.YpX, A, B);
  fe_mul2(a, q.YpX, b, q.YmX, A2, B2);
  const fe F = fe_sub(D, C), G = fe_add(D, C);
  jt_put(vt, ls, ge_finish_rt(fe_sub(B, A), F, G, fe_add(B, A), true));
  jt_put(vt, ld, ge_finish_rt(fe_sub(B2, A2), G, F, fe_add(B2, A2), true));
}

// The 12 lines for the affine points P = (xp, yp), Q = (xq, yq).  Q and 2Q
// first; then for P and 2P the line itself and its sums and differences with
// Q and 2Q, which are read back from the table: one pair body in a loop.
template <class VT>
HSV_INL void jt_build(VT &vt, const fe &xp, const fe &yp, const fe &xq, const fe &yq) {
#ifdef HSV_TIMING_STUB_TABLES  // tools/phase_probe.py only: tables left unwritten
  return;
#endif
  ge_ext p, q;
  p.X = xp;
  p.Y = yp;
  p.Z = fe_small(1);
  q.X = xq;
  q.Y = yq;
  q.Z = fe_small(1);
  fe_mul2(xp, yp, xq, yq, p.T, q.T);
  uint32_t neg;
  jt_put(vt, joint_line(0, 1, neg), q);
  jt_put(vt, joint_line(0, 2, neg), ge_dbl_rt(q, true));
  HSV_NOUNROLL
  for (int i = 1; i <= 2; ++i) {
    if (i == 2) p = ge_dbl_rt(p, true);
    jt_put(vt, joint_line(i, 0, neg), p);
    HSV_NOUNROLL
    for (int j = 1; j <= 2; ++j) {
      uint32_t w[32];
      vt.get_line(joint_line(0, j, neg), w);
      jt_pair(vt, p, cached_unpack(w), joint_line(i, j, neg), joint_line(i, -j, neg));
    }
  }
}

// Straus over the joint table: d[0] the digits of c1, d[1] those of |c0| (five
// words each, NW 2-bit columns of recode_cols, the top column at the top bit);
// flip: c0 < 0.
// Per column two doublings and one cached addition of +-line; T only where
// the addition follows, and after the last column (the comb phase follows).
// Leading columns that are zero in every lane of the wave are skipped, as in
// straus_vt.  The line is loaded right before its addition.
template <int NW, class VT>
HSV_INL ge_ext straus_joint(uint32_t d[2][5], VT &vt, uint32_t flip) {
  ge_ext q = ge_identity();
#ifdef HSV_TIMING_STUB_STRAUS  // tools/phase_probe.py only
  return q;
#endif
  int top = NW - 1;
  HSV_NOUNROLL
  while (top > 0) {
    const uint32_t nz = ((d[0][4] >> 30) ^ (uint32_t)kColOffset) | ((d[1][4] >> 30) ^ (uint32_t)kColOffset);
    if (wave_any(nz)) break;
    limbs_shl<5>(d[0], 2);
    limbs_shl<5>(d[1], 2);
    --top;
  }
  HSV_NOUNROLL
  for (int c = top; c >= 0; --c) {
    uint32_t neg;
    const uint32_t line = joint_column<kColOffset>(d[0][4] >> 30, d[1][4] >> 30, flip, neg);
    limbs_shl<5>(d[0], 2);
    limbs_shl<5>(d[1], 2);
    if (c != top) {
      HSV_NOUNROLL
      for (int j = 0; j < 2; ++j) q = ge_dbl_rt(q, j == 1);
    }
    uint32_t cur[32];
    vt.get_line(line, cur);
    q = ge_add_cached_rt(q, ge_cached_cneg(cached_unpack(cur), neg), c == 0);
  }
  return q;
}

// Which point pass hsv_verify_hp_kernel and the fused transaction launch run,
// and so which digit format their prepasses write (hsv_prep_kernel, the
// transaction record kernels, hsv_msg_prep_kernel): the joint table over
// 2-bit columns, or (0, A/B builds only) the two 4-bit tables.
#ifndef HSV_JOINT_POINTPASS
#define HSV_JOINT_POINTPASS 1
#endif
template <int WA>
constexpr bool joint_pointpass() { return HSV_JOINT_POINTPASS && WA == 4; }
template <int WA>
constexpr int pointpass_digit_bits() { return joint_pointpass<WA>() ? 2 : WA; }

// JOINT: the record holds 2-bit columns (prep_from_hash with DW = 2) and the
// point pass runs over the joint table; otherwise two WA-bit tables.
template <int WA, int CB, bool JOINT = false, class VT>
HSV_INL uint32_t verify_one_prepped(const uint32_t pk[8], const uint32_t rb[8], const uint32_t *rec,
                                    uint64_t stride, const uint32_t meta, const uint32_t *tb, VT &vt,
                                    uint64_t *clk = nullptr) {
  using G = HalfCombWindows<JOINT ? 2 : WA>;
  constexpr int TS = 1 << (WA - 1);
  uint32_t a_ok, small_a, r_ok, small_r;
  {
    fe xr, yr, xa, ya;
    ge_decompress2(rb, pk, xr, yr, xa, ya, r_ok, a_ok);  // both root chains at once
    small_r = r_ok & y_is_small_order(yr);
    small_a = a_ok & y_is_small_order(ya);
    HSV_CLK(1);
    if constexpr (JOINT) {
      jt_build(vt, fe_carry(fe_neg(xr)), yr, fe_carry(fe_neg(xa)), ya);
    } else {
      vt_build<TS>(vt, 0, fe_carry(fe_neg(xr)), yr);
      vt_build<TS>(vt, 1, fe_carry(fe_neg(xa)), ya);
    }
    HSV_CLK(2);
  }
  uint32_t d[2][5];
  HSV_UNROLL
  for (int i = 0; i < 5; ++i) {
    d[0][i] = rec[i * stride];
    d[1][i] = rec[(5 + i) * stride];
  }
  const uint32_t c0_neg = (meta & kPrepC0Neg) ? 1u : 0u;
  ge_ext q;
  if constexpr (JOINT) q = straus_joint<G::NW>(d, vt, c0_neg);
  else q = straus_vt<WA, G::NW, 5, 2, false>(d, vt, c0_neg);
  HSV_CLK(3);
  uint32_t b[8];
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) b[i] = rec[(10 + i) * stride];
  q = comb_add_b<CB>(q, b, tb);
  const uint32_t same = ge_is_neutral(q);
  return flags_byte(meta & kPrepSOk, a_ok, r_ok, small_a, small_r, same) | fault_bit(a_ok, r_ok, q);
}

}  // namespace hsv
