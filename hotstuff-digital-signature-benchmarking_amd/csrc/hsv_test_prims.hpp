// Test dispatch of the one-lane primitives: an op code and raw operands in, raw
// results out.  The device kernels of hsv_test_prims.hip (libhsv_test.so only)
// and the host program tests/native/prims_host.cpp run this same text, so what
// differs between the two answers is what the compiler made of the headers:
// on the device the inline-asm branches of hsv_fe26x10.hpp, the hardware
// reciprocal of lat_floor_div and the wave votes of hsv_lattice.hpp.
//
// Field record, kPrimFieldIn = 24 words in:  op, aux, f[10], g[10], 2 unused.
//   Limbs are taken as given: no masking, no fe_from_words_masked.  The caller
//   keeps every operand inside the class its op documents (hsv_fe26x10.hpp).
//   kPrimFieldOut = 24 words out: status, then the result words listed at the
//   op codes; words an op does not list are not written (both callers hand
//   in a zeroed record).
// Scalar record, kPrimScalarIn = 32 words in:  op, aux, 30 operand words.
//   kPrimScalarOut = 16 words out: status, then the result words.
// status: kPrimDone, or kPrimBadOp for an unknown op code (nothing else is
// written).  No index is derived from input data: `item` is the record's
// position, and aux only bounds a loop (fe_sqn) or is a bit count (lattice).
#pragma once
#include "hsv_lattice.hpp"

namespace hsv {

constexpr int kPrimFieldIn = 24, kPrimFieldOut = 24;
constexpr int kPrimScalarIn = 32, kPrimScalarOut = 16;
constexpr uint32_t kPrimDone = 0x600du, kPrimBadOp = 0xbad0u;
constexpr uint32_t kPrimMaxSqn = 16;

enum PrimFieldOp : uint32_t {
  kPfMul = 1,        // fe_mul(f, g)                       -> 10 limbs
  kPfMul2 = 2,       // fe_mul2(f, g, g, f)                -> 10 + 10 limbs
  kPfMulP = 3,       // fe_mul_p(prep_f(f), prep_g(g))     -> 10 limbs
  kPfMul2P = 4,      // fe_mul2_p, operands as kPfMul2     -> 10 + 10 limbs
  kPfSq = 5,         // fe_sq(f)                           -> 10 limbs
  kPfSq2 = 6,        // fe_sq2(f, g)                       -> 10 + 10 limbs
  kPfAdd = 7,        // fe_add(f, g)                       -> 10 limbs
  kPfSub = 8,        // fe_sub(f, g)                       -> 10 limbs
  kPfNeg = 9,        // fe_neg(f)                          -> 10 limbs
  kPfCarry = 10,     // fe_carry(f)                        -> 10 limbs
  kPfCanon = 11,     // fe_canon(f)                        -> 10 limbs
  kPfPack = 12,      // fe_pack(f)                         -> 8 words
  kPfPackLoose = 13, // fe_pack_loose(f), fe_unpack_loose  -> 8 words + 10 limbs
  kPfIsZero = 14,    // fe_is_zero(f)                      -> 1 word
  kPfEq = 15,        // fe_eq(f, g)                        -> 1 word
  kPfLowBit = 16,    // fe_canon_low_bit(f)                -> 1 word
  kPfSelect = 17,    // fe_select(f, g, item & 1)          -> 10 limbs
  kPfInvert = 18,    // fe_invert(f)                       -> 10 limbs
  kPfPow22523 = 19,  // fe_pow22523(f)                     -> 10 limbs
  kPfPow22523x2 = 20,// fe_pow22523_2(f, g)                -> 10 + 10 limbs
  kPfSqn = 21,       // fe_sqn(f, aux), aux <= kPrimMaxSqn -> 10 limbs
};

enum PrimScalarOp : uint32_t {
  kPsReduce512 = 1,   // x[16]                  -> 8 words
  kPsIsCanonical = 2, // s[8]                   -> 1 word
  kPsMulAdd = 3,      // a[8], b[8], c[8]       -> 8 words  (a b + c mod l)
  kPsMulSmall = 4,    // c1[5], 3 unused, s[8]  -> 8 words  (c1 s mod l)
  kPsLattice = 5,     // k[8], aux = max_bits   -> ok, c0_neg, c0[5], c1[5]
};

HSV_INL void prim_put_fe(uint32_t *out, const fe &r) {
  HSV_UNROLL
  for (int i = 0; i < 10; ++i) out[i] = r.v[i];
}

// in: kPrimFieldIn words; out: kPrimFieldOut words; item: the record's index
HSV_INL void prim_field_op(const uint32_t *in, uint32_t item, uint32_t *out) {
  const uint32_t op = in[0], aux = in[1];
  fe f, g;
  HSV_UNROLL
  for (int i = 0; i < 10; ++i) {
    f.v[i] = in[2 + i];
    g.v[i] = in[12 + i];
  }
  uint32_t *res = out + 1;
  fe r, s;
  switch (op) {
    case kPfMul:
      prim_put_fe(res, fe_mul(f, g));
      break;
    case kPfMul2:
      fe_mul2(f, g, g, f, r, s);
      prim_put_fe(res, r);
      prim_put_fe(res + 10, s);
      break;
    case kPfMulP:
      prim_put_fe(res, fe_mul_p(fe_prep_f(f), fe_prep_g(g)));
      break;
    case kPfMul2P:
      fe_mul2_p(fe_prep_f(f), fe_prep_g(g), fe_prep_f(g), fe_prep_g(f), r, s);
      prim_put_fe(res, r);
      prim_put_fe(res + 10, s);
      break;
    case kPfSq:
      prim_put_fe(res, fe_sq(f));
      break;
    case kPfSq2:
      fe_sq2(f, g, r, s);
      prim_put_fe(res, r);
      prim_put_fe(res + 10, s);
      break;
    case kPfAdd:
      prim_put_fe(res, fe_add(f, g));
      break;
    case kPfSub:
      prim_put_fe(res, fe_sub(f, g));
      break;
    case kPfNeg:
      prim_put_fe(res, fe_neg(f));
      break;
    case kPfCarry:
      prim_put_fe(res, fe_carry(f));
      break;
    case kPfCanon:
      prim_put_fe(res, fe_canon(f));
      break;
    case kPfPack:
      fe_pack(f, res);
      break;
    case kPfPackLoose:
      fe_pack_loose(f, res);
      prim_put_fe(res + 8, fe_unpack_loose(res));
      break;
    case kPfIsZero:
      res[0] = fe_is_zero(f);
      break;
    case kPfEq:
      res[0] = fe_eq(f, g);
      break;
    case kPfLowBit:
      res[0] = fe_canon_low_bit(f);
      break;
    case kPfSelect:
      prim_put_fe(res, fe_select(f, g, item & 1u));
      break;
    case kPfInvert:
      prim_put_fe(res, fe_invert(f));
      break;
    case kPfPow22523:
      prim_put_fe(res, fe_pow22523(f));
      break;
    case kPfPow22523x2:
      fe_pow22523_2(f, g, r, s);
      prim_put_fe(res, r);
      prim_put_fe(res + 10, s);
      break;
    case kPfSqn:
      if (aux > kPrimMaxSqn) {
        out[0] = kPrimBadOp;
        return;
      }
      prim_put_fe(res, fe_sqn(f, (int)aux));
      break;
    default:
      out[0] = kPrimBadOp;
      return;
  }
  out[0] = kPrimDone;
}

// in: kPrimScalarIn words; out: kPrimScalarOut words
HSV_INL void prim_scalar_op(const uint32_t *in, uint32_t *out) {
  const uint32_t op = in[0], aux = in[1];
  const uint32_t *x = in + 2;
  uint32_t *res = out + 1;
  sc a, b, c, r;
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) {
    a.v[i] = x[i];
    b.v[i] = x[8 + i];
    c.v[i] = x[16 + i];
  }
  switch (op) {
    case kPsReduce512:
      r = sc_reduce512(x);
      break;
    case kPsIsCanonical:
      res[0] = sc_is_canonical(x);
      out[0] = kPrimDone;
      return;
    case kPsMulAdd:
      r = sc_muladd(a, b, c);
      break;
    case kPsMulSmall:
      r = sc_mul_small(a.v, b.v);
      break;
    case kPsLattice: {
      if (aux < 1u || aux > 159u) {
        out[0] = kPrimBadOp;
        return;
      }
      const LatOut o = lattice_reduce(a, (int)aux);
      res[0] = o.ok;
      res[1] = o.c0_neg;
      HSV_UNROLL
      for (int i = 0; i < 5; ++i) {
        res[2 + i] = o.c0[i];
        res[7 + i] = o.c1[i];
      }
      out[0] = kPrimDone;
      return;
    }
    default:
      out[0] = kPrimBadOp;
      return;
  }
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) res[i] = r.v[i];
  out[0] = kPrimDone;
}

}  // namespace hsv
