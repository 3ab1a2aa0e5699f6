// Ed25519 key expansion and signing, one lane per group of items (RFC 8032;
// reference crypto/src/lib.rs:167-175 generate_keypair, 185-191 Signature::new).
//
// Per item:
//   r = SHA-512(prefix || M) mod l,  R = [r]B,
//   k = SHA-512(enc(R) || pk || M) mod l,  s = r + k a mod l,  sig = enc(R) || s
// with (a, prefix, pk) the 96-byte expanded key record of the item's key.
//
// [r]B comes from the comb of B every device context holds (hsv_comb.hpp):
// 16 mixed additions with the wide table (about 16 x 7 field products).  The
// encoding of R needs 1/Z, and fe_invert is a chain of about 265 products --
// more than twice the point work.  The verifier never inverts (it compares
// projectively), so that cost is new here, and it is amortised the way the
// table builders do it (comb_build_run): a lane carries G items, keeps their
// (X, Y, Z), multiplies the Z's up, inverts the product once and walks back
// (3 products per item for the inverse, 2 for x and y).  Per item that is
// about 112 + 7 (self-check) + 6 + 265 / G field products and two SHA-512.
//
// Between the two phases an item's state (X, Y, Z, the prefix product before
// it, r and a status word) lives in a Store the caller provides: the kernels
// use a launch workspace laid out word by word across the wave's lanes
// (coalesced), the host test a plain array.
//
// Self-check, as everywhere in the library: before an item's Z enters the
// product its point passes ge_is_sane.  The addition law is complete, so a
// valid table never fails it; an item that does (corrupted table memory)
// contributes 1 instead of Z -- it cannot poison its group -- gets 64 zero
// bytes and is reported to the caller (fault[0]).
//
// Table lookups are indexed by digits of the secret scalars r and a: this is
// not a constant-time signer.  It is meant for load generation and for
// synthesising inputs, not for custody of a validator key.
#pragma once
#include "hsv_comb.hpp"

namespace hsv {

constexpr int kSignKeyBytes = 96;  // a (32, reduced mod l) | prefix (32) | pk (32)
constexpr int kSignGroup = 8;      // G of the product launches

// [x]B for any x < 2^256 (8 little-endian words) from the comb of B with
// WB-bit signed digits (WB = 16: the wide table, 16 additions; WB = 8: the
// narrow one, 32), in extended coordinates.  The recoding adds
// C = sum 2^(WB-1) 2^(WB j); for x >= 2^256 - C the sum carries out of the top
// digit and [2^256]B = 2 [2^(WB-1) 2^(256-WB)]B, twice the last entry of the
// top position, is added (never taken for a reduced scalar).
// inject: fault injection (tests), applied to the entry of position 0.
template <int WB>
HSV_INL ge_ext fixed_base_comb(const uint32_t x[8], const uint32_t *table, uint32_t inject = kInjectNone) {
  static_assert(WB == 8 || WB == 16, "comb digit width");
  constexpr int NP = 256 / WB;
  constexpr int ENT = 1 << (WB - 1);
  uint32_t sr[9];
  recode_add<9, WB, NP>(x, 8, sr);
  ge_ext q = ge_identity();
  HSV_NOUNROLL
  for (int j = 0; j < NP; ++j) {
    const uint32_t c = sr[0] & ((1u << WB) - 1u);
    HSV_UNROLL
    for (int i = 0; i < 8; ++i) sr[i] = (sr[i] >> WB) | (sr[i + 1] << (32 - WB));
    sr[8] >>= WB;
    const CombPosTab tp{table + (uint64_t)j * ENT * kCombEntryWords};
    ge_niels n = select_niels<WB>(tp, c);
    if (inject != kInjectNone && j == 0) n = niels_injected(n, inject);
    q = ge_add_niels<true>(q, n);
  }
  if (sr[0] & 1u) {
    const CombPosTab tp{table + (uint64_t)(NP - 1) * ENT * kCombEntryWords};
    const ge_niels top = tp.load(ENT - 1);
    q = ge_add_niels<true>(ge_add_niels<true>(q, top), top);
  }
  return q;
}

// ---- loads and stores of little-endian words --------------------------------
// p 16-byte aligned, N a multiple of 4
template <int N>
HSV_INL void sign_load16(const uint8_t *p, uint32_t w[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  HSV_UNROLL
  for (int i = 0; i < N / 4; ++i) {
    const uint4 v = q[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
#else
  for (int i = 0; i < N; ++i)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
           ((uint32_t)p[4 * i + 3] << 24);
#endif
}

template <int N>
HSV_INL void sign_store16(uint8_t *p, const uint32_t w[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4 *q = reinterpret_cast<uint4 *>(p);
  HSV_UNROLL
  for (int i = 0; i < N / 4; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
#else
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < 4; ++k) p[4 * i + k] = (uint8_t)(w[i] >> (8 * k));
#endif
}

// a 32-byte message at any alignment: word loads when p is 4-byte aligned
HSV_INL void sign_load_msg32(const uint8_t *p, uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    HSV_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = q[i];
    return;
  }
#endif
  HSV_UNROLL
  for (int i = 0; i < 8; ++i)
    w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
           ((uint32_t)p[4 * i + 3] << 24);
}

// ---- SHA-512 shapes of signing ----------------------------------------------
HSV_SHA_INL void sha512_digest_words(const uint64_t h[8], uint32_t out[16]) {
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) {
    out[2 * i] = bswap32((uint32_t)(h[i] >> 32));
    out[2 * i + 1] = bswap32((uint32_t)h[i]);
  }
}

// One block: NW little-endian words (NW = 8: a seed; NW = 16: prefix || Digest).
// The 96-byte shape is sha512_96.
template <int NW>
HSV_SHA_INL void sha512_words(const uint32_t *in, uint32_t out[16]) {
  static_assert(NW % 2 == 0 && NW <= 26, "one padded block");
  uint64_t w[16];
  HSV_UNROLL
  for (int i = 0; i < 16; ++i) w[i] = 0;
  HSV_UNROLL
  for (int i = 0; i < NW / 2; ++i) w[i] = be64_from_le32(in[2 * i], in[2 * i + 1]);
  w[NW / 2] = 0x8000000000000000ull;
  w[15] = (uint64_t)NW * 32u;
  uint64_t h[8];
  sha512_init(h);
  sha512_compress(h, w);
  sha512_digest_words(h, out);
}

// bytes [off, off + 8) of msg || 0x80 || 0 0 ... as one big-endian word
HSV_SHA_INL uint64_t sha512_msg_word(const uint8_t *msg, uint64_t len, uint64_t off) {
  uint64_t x = 0;
  if (off + 8 <= len) {
    HSV_UNROLL
    for (int i = 0; i < 8; ++i) x = (x << 8) | msg[off + i];
    return x;
  }
  HSV_UNROLL
  for (int i = 0; i < 8; ++i) {
    const uint64_t pos = off + (uint64_t)i;
    uint64_t b = 0;
    if (pos < len) b = msg[pos];
    else if (pos == len) b = 0x80;
    x = (x << 8) | b;
  }
  return x;
}

// SHA-512(head || msg): head = HW little-endian words (8: the prefix, 16:
// enc(R) || pk), msg = len bytes at any alignment, any length.
template <int HW>
HSV_SHA_INL void sha512_head_msg(const uint32_t *head, const uint8_t *msg, uint64_t len, uint32_t out[16]) {
  static_assert(HW % 2 == 0 && HW <= 32, "head within the first block");
  constexpr int HQ = HW / 2;
  const uint64_t total = (uint64_t)HW * 4u + len;
  const uint64_t nblocks = (total + 1 + 16 + 127) / 128;
  uint64_t h[8];
  sha512_init(h);
  HSV_NOUNROLL
  for (uint64_t b = 0; b < nblocks; ++b) {
    uint64_t w[16];
    HSV_UNROLL
    for (int j = HQ; j < 16; ++j) w[j] = sha512_msg_word(msg, len, b * 128u + (uint64_t)j * 8u - (uint64_t)HW * 4u);
    HSV_UNROLL
    for (int j = 0; j < HQ; ++j)
      w[j] = b == 0 ? be64_from_le32(head[2 * j], head[2 * j + 1])
                    : sha512_msg_word(msg, len, b * 128u + (uint64_t)j * 8u - (uint64_t)HW * 4u);
    if (b + 1 == nblocks) w[15] = total * 8u;  // w[14] is zero: len < 2^61
    sha512_compress(h, w);
  }
  sha512_digest_words(h, out);
}

// ---- the state of an item between the two phases -----------------------------
constexpr int kWsX = 0, kWsY = kFeLimbs, kWsZ = 2 * kFeLimbs, kWsP = 3 * kFeLimbs;  // P: prefix product BEFORE the item
constexpr int kWsR = 4 * kFeLimbs, kWsStatus = kWsR + 8;
constexpr int kSignWsWords = kWsStatus + 1;
// status of a slot
enum : uint32_t {
  kSlotDead = 0,   // no item (past the end of the batch): nothing is written
  kSlotOk = 1,
  kSlotFault = 2,  // the point failed the self-check: zero output, fault
  kSlotZero = 3,   // key index out of range: zero output, no fault
};

template <class Store>
HSV_INL void ws_put_fe(Store &st, int g, int at, const fe &a) {
  HSV_UNROLL
  for (int i = 0; i < kFeLimbs; ++i) st.put(g, at + i, a.v[i]);
}
template <class Store>
HSV_INL fe ws_get_fe(const Store &st, int g, int at) {
  fe a;
  HSV_UNROLL
  for (int i = 0; i < kFeLimbs; ++i) a.v[i] = st.get(g, at + i);
  return a;
}

// Phase 1 of one item: the point p enters the lane's running product pp.
// Returns 1 when p passed the self-check.
template <class Store>
HSV_INL uint32_t group_push(const ge_ext &p, fe &pp, Store &st, int g) {
  const uint32_t ok = ge_is_sane(p);
  const fe zc = fe_select(fe_small(1), p.Z, ok);
  ws_put_fe(st, g, kWsX, p.X);
  ws_put_fe(st, g, kWsY, p.Y);
  ws_put_fe(st, g, kWsZ, zc);
  ws_put_fe(st, g, kWsP, pp);
  pp = fe_mul(pp, zc);
  return ok;
}

// Phase 2 of one item (slots are walked from the last to the first): inv is
// 1 / (product of the Z's of slots 0..g) on entry and of slots 0..g-1 on
// return; enc receives the 32-byte encoding of the slot's point.
template <class Store>
HSV_INL void group_pop(fe &inv, const Store &st, int g, uint32_t enc[8]) {
  const fe zinv = fe_mul(inv, ws_get_fe(st, g, kWsP));
  inv = fe_mul(inv, ws_get_fe(st, g, kWsZ));
  fe x, y;
  fe_mul2(ws_get_fe(st, g, kWsX), zinv, ws_get_fe(st, g, kWsY), zinv, x, y);
  fe_pack(y, enc);
  enc[7] |= fe_is_negative(x) << 31;
}

// ---- key expansion -----------------------------------------------------------
struct KeygenArgs {
  const uint8_t *seeds;   // n * 32 B, 16-byte aligned
  uint64_t n;
  uint8_t *keys;          // n * 96 B, 16-byte aligned
  const uint32_t *table;  // comb of B (WB-bit digits)
  uint32_t inject, inject_item;  // tests (host build): corrupt the table entry item inject_item reads
};

// Items first, first + step, ..., G of them, through `st`.  Returns 1 when an
// item failed the self-check.
template <int WB, int G, class Store>
HSV_INL uint32_t keygen_lane(const KeygenArgs &a, uint64_t first, uint32_t step, Store &st) {
  fe pp = fe_small(1);
  uint32_t bad = 0;
  HSV_NOUNROLL
  for (int g = 0; g < G; ++g) {
    const uint64_t i = first + (uint64_t)g * step;
    uint32_t status = kSlotDead;
    if (i < a.n) {
      uint32_t seed[8], h[16];
      sign_load16<8>(a.seeds + i * 32u, seed);
      sha512_words<8>(seed, h);
      h[0] &= ~7u;  // clamp: bits 0-2 cleared, bit 255 cleared, bit 254 set
      h[7] = (h[7] & 0x7fffffffu) | 0x40000000u;
      uint32_t wide[16];
      HSV_UNROLL
      for (int j = 0; j < 16; ++j) wide[j] = j < 8 ? h[j] : 0u;
      const sc s = sc_reduce512(wide);
      uint32_t rec[16];
      HSV_UNROLL
      for (int j = 0; j < 16; ++j) rec[j] = j < 8 ? s.v[j] : h[j];
      sign_store16<16>(a.keys + i * (uint64_t)kSignKeyBytes, rec);
      const uint32_t inj = (a.inject != kInjectNone && i == a.inject_item) ? a.inject : (uint32_t)kInjectNone;
      const uint32_t ok = group_push(fixed_base_comb<WB>(s.v, a.table, inj), pp, st, g);
      status = ok ? kSlotOk : kSlotFault;
      bad |= ok ^ 1u;
    }
    st.put(g, kWsStatus, status);
  }
  fe inv = fe_invert(pp);
  HSV_NOUNROLL
  for (int g = G - 1; g >= 0; --g) {
    const uint32_t status = st.get(g, kWsStatus);
    if (status == kSlotDead) continue;
    const uint64_t i = first + (uint64_t)g * step;
    uint32_t enc[8];
    group_pop(inv, st, g, enc);
    if (status != kSlotOk) {
      HSV_UNROLL
      for (int j = 0; j < 8; ++j) enc[j] = 0u;
    }
    sign_store16<8>(a.keys + i * (uint64_t)kSignKeyBytes + 64, enc);
  }
  return bad;
}

// ---- signing -----------------------------------------------------------------
struct SignArgs {
  const uint8_t *keys;      // nkeys expanded records of 96 B, 16-byte aligned
  uint32_t nkeys;
  const uint32_t *key_idx;  // m indices, or NULL: item i uses key i
  const uint8_t *msg;       // item i's message at msg + i * msg_stride (0: one shared message), any alignment
  uint64_t msg_len, msg_stride;
  uint64_t m;
  uint8_t *sig;             // item i's R || s at sig + i * sig_stride, 16-byte aligned (SignSlotIo; unused by
  uint64_t sig_stride;      // the transaction signer, whose TxSignIo knows where the tails are)
  const uint32_t *table;    // comb of B (WB-bit digits)
  uint32_t inject, inject_item;  // tests (host build): corrupt the table entry item inject_item reads
};

// Where sign_lane takes an item's slot status from and where the item's
// output goes.  This one is hsv_signer_sign*'s: every item of the batch is
// live, and R || s goes to the item's aligned 64-byte slot.  The transaction
// signer's is TxSignIo (hsv_txsign.hpp).
struct SignSlotIo {
  static constexpr bool kPointOnly = false;  // sign_lane hashes: true only for MsgSignIo (hsv_msgsign.hpp)
  // kSlotOk (sign), kSlotZero (zero output) or kSlotDead (the item is skipped: nothing is written)
  HSV_MEMBER uint32_t slot(const SignArgs &a, uint64_t, uint32_t ki) const { return ki < a.nkeys ? kSlotOk : kSlotZero; }
  // status: kSlotOk (sigw = R || s), kSlotZero or kSlotFault (sigw = 0)
  HSV_MEMBER void store(const SignArgs &a, uint64_t i, uint32_t, const uint32_t sigw[16]) const {
    sign_store16<16>(a.sig + i * a.sig_stride, sigw);
  }
};

// FAST: msg_len == 32 (the Digest): both hashes are one block each.
// Io::kPointOnly (the point launch of hsv_signer_sign_msgs*, hsv_msgsign.hpp):
// neither hash is taken here -- r comes from io.nonce_words(), and store()
// receives enc(R) in sigw[0..8) and nothing else.
template <int WB, int G, bool FAST, class Store, class Io = SignSlotIo>
HSV_INL uint32_t sign_lane(const SignArgs &a, uint64_t first, uint32_t step, Store &st, const Io &io = Io()) {
  fe pp = fe_small(1);
  uint32_t bad = 0;
  HSV_NOUNROLL
  for (int g = 0; g < G; ++g) {
    const uint64_t i = first + (uint64_t)g * step;
    uint32_t status = kSlotDead;
    if (i < a.m) {
      const uint32_t ki = a.key_idx ? a.key_idx[i] : (uint32_t)i;
      status = io.slot(a, i, ki);
      if (status == kSlotOk) {
        sc r;
        if constexpr (Io::kPointOnly) {
          io.nonce_words(i, r.v);
        } else {
          const uint8_t *mp = a.msg + i * a.msg_stride;
          uint32_t in[16], h[16];
          sign_load16<8>(a.keys + (uint64_t)ki * kSignKeyBytes + 32, in);  // prefix
          if (FAST) {
            sign_load_msg32(mp, in + 8);
            sha512_words<16>(in, h);
          } else {
            sha512_head_msg<8>(in, mp, a.msg_len, h);
          }
          r = sc_reduce512(h);
        }
        const uint32_t inj = (a.inject != kInjectNone && i == a.inject_item) ? a.inject : (uint32_t)kInjectNone;
        const uint32_t ok = group_push(fixed_base_comb<WB>(r.v, a.table, inj), pp, st, g);
        if constexpr (!Io::kPointOnly) {
          HSV_UNROLL
          for (int j = 0; j < 8; ++j) st.put(g, kWsR + j, r.v[j]);
        }
        status = ok ? kSlotOk : kSlotFault;
        bad |= ok ^ 1u;
      }
    }
    st.put(g, kWsStatus, status);
  }
  fe inv = fe_invert(pp);
  HSV_NOUNROLL
  for (int g = G - 1; g >= 0; --g) {
    const uint32_t status = st.get(g, kWsStatus);
    if (status == kSlotDead) continue;
    const uint64_t i = first + (uint64_t)g * step;
    uint32_t sigw[16];
    HSV_UNROLL
    for (int j = 0; j < 16; ++j) sigw[j] = 0u;
    if (status != kSlotZero) {
      uint32_t enc[8];
      group_pop(inv, st, g, enc);
      if constexpr (Io::kPointOnly) {
        if (status == kSlotOk) {
          HSV_UNROLL
          for (int j = 0; j < 8; ++j) sigw[j] = enc[j];
        }
      } else if (status == kSlotOk) {
        const uint32_t ki = a.key_idx ? a.key_idx[i] : (uint32_t)i;
        const uint8_t *key = a.keys + (uint64_t)ki * kSignKeyBytes;
        const uint8_t *mp = a.msg + i * a.msg_stride;
        uint32_t head[16], h[16];
        HSV_UNROLL
        for (int j = 0; j < 8; ++j) head[j] = enc[j];
        sign_load16<8>(key + 64, head + 8);  // pk
        if (FAST) {
          uint32_t mw[8];
          sign_load_msg32(mp, mw);
          sha512_96(head, head + 8, mw, h);
        } else {
          sha512_head_msg<16>(head, mp, a.msg_len, h);
        }
        const sc k = sc_reduce512(h);
        sc sa, r;
        sign_load16<8>(key, sa.v);
        HSV_UNROLL
        for (int j = 0; j < 8; ++j) r.v[j] = st.get(g, kWsR + j);
        const sc s = sc_muladd(k, sa, r);
        HSV_UNROLL
        for (int j = 0; j < 8; ++j) {
          sigw[j] = enc[j];
          sigw[8 + j] = s.v[j];
        }
      }
    }
    io.store(a, i, status, sigw);
  }
  return bad;
}

}  // namespace hsv
