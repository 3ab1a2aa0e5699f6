// The point pass's shared pieces (hsv_kernels.hip: hsv_verify_hp_kernel;
// hsv_small.hip: the latency forms; hsv_mempool.hip: the fused transaction
// launch; hsv_routed.hpp: the routed rounds): the per-lane table store, record
// loads, the verdict store, a fallback item's full-length path, work counters
// and the device self-check words.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hsv_verify_core.hpp"
#include "hsv_verify_hc.hpp"

#ifndef HSV_HP_WAVES
#define HSV_HP_WAVES 3  // waves per SIMD of the point pass (launch bounds: 168 VGPRs)
#endif

namespace hsv {

constexpr int kBlock = 256;


// Per-lane variable-base tables in global memory (hsv_verify_core.hpp, VT):
// lane region = 2 tables x (ENT - 1) entries x 128 B, entry = 8 x uint4.
// Entry 0 of every table is the identity: it is not stored per lane; a zero
// digit reads this one shared line (L2-resident) instead.  Loose encoding of
// (Y+X, Y-X, 2Z, 2dT) = (1, 1, 2, 0).
__device__ const uint4 kVtIdentity[8] = {{1u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {1u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u},
                                         {2u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};

// Fault injection (hsv_test_inject_fault, tests only; uniform kernel argument,
// kInject* in hsv_verify_core.hpp): the table stores of every lane are
// replaced, between the table build and the window loop, by what a corrupted
// workspace would hold.
template <int ENT>
struct GlobalVarTab {
  static constexpr int kStored = ENT - 1;  // entries 1 .. ENT-1 per table
  uint4 *base;
  uint32_t inject = kInjectNone;
  __device__ __forceinline__ void put(int t, int m, const uint32_t w[32]) const {
    if (m == 0) return;
    uint4 *e = base + (t * kStored + m - 1) * 8;
    if (__builtin_expect(inject == kInjectZeroTables || (inject == kInjectFlipTables && t == 0), 0)) {
      HSV_UNROLL
      for (int q = 0; q < 8; ++q)
        e[q] = inject == kInjectZeroTables ? make_uint4(0u, 0u, 0u, 0u)
                                           : make_uint4(w[4 * q] ^ (q == 0 ? 1u : 0u), w[4 * q + 1], w[4 * q + 2],
                                                        w[4 * q + 3]);
      return;
    }
    HSV_UNROLL
    for (int q = 0; q < 8; ++q) {
#ifdef HSV_TIMING_STUB_TABLE_STORES  // timing probe only: entries computed, never stored
      asm volatile("" ::"v"(w[4 * q]), "v"(w[4 * q + 1]), "v"(w[4 * q + 2]), "v"(w[4 * q + 3]));
#else
      e[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
#endif
    }
  }
  __device__ __forceinline__ void get(int t, uint32_t m, uint32_t w[32]) const {
    const uint4 *e = m ? base + (t * kStored + (int)m - 1) * 8 : kVtIdentity;
    HSV_UNROLL
    for (int q = 0; q < 8; ++q) {
      const uint4 v = e[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
};

template <int WA>
constexpr int vt_lane_uint4() { return 2 * (1 << (WA - 1)) * 8; }

// The joint table of the throughput point pass (hsv_verify_hc.hpp, jt_build /
// straus_joint): kJointLines lines of 128 B per lane, line l at
// base + (l - 1) * 8; line 0, the identity, is the shared one.  The
// full-length path of a fallback item keeps its 8-line table of -A in the
// same slot (put / get, table 0 of GlobalVarTab<9>: lines 1 .. 8).
// Fault injection as GlobalVarTab: zeros in every line, or one bit flipped in
// the lines that involve R (and in the fallback path's table 0).
struct GlobalJointTab {
  uint4 *base;
  uint32_t inject = kInjectNone;
  __device__ __forceinline__ void put(int t, int m, const uint32_t w[32]) const {
    GlobalVarTab<9>{base, inject}.put(t, m, w);
  }
  __device__ __forceinline__ void get(int t, uint32_t m, uint32_t w[32]) const {
    GlobalVarTab<9>{base, inject}.get(t, m, w);
  }
  __device__ __forceinline__ void put_line(uint32_t l, const uint32_t w[32]) const {
    uint4 *e = base + (l - 1u) * 8u;
    if (__builtin_expect(inject == kInjectZeroTables || (inject == kInjectFlipTables && l >= kJointFirstLineOfR), 0)) {
      HSV_UNROLL
      for (int q = 0; q < 8; ++q)
        e[q] = inject == kInjectZeroTables ? make_uint4(0u, 0u, 0u, 0u)
                                           : make_uint4(w[4 * q] ^ (q == 0 ? 1u : 0u), w[4 * q + 1], w[4 * q + 2],
                                                        w[4 * q + 3]);
      return;
    }
    HSV_UNROLL
    for (int q = 0; q < 8; ++q) {
#ifdef HSV_TIMING_STUB_TABLE_STORES  // timing probe only: lines computed, never stored
      asm volatile("" ::"v"(w[4 * q]), "v"(w[4 * q + 1]), "v"(w[4 * q + 2]), "v"(w[4 * q + 3]));
#else
      e[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
#endif
    }
  }
  __device__ __forceinline__ void get_line(uint32_t l, uint32_t w[32]) const {
    const uint4 *e = l ? base + (l - 1u) * 8u : kVtIdentity;
    HSV_UNROLL
    for (int q = 0; q < 8; ++q) {
      const uint4 v = e[q];
      w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
  }
};
constexpr int kJointLaneUint4 = kJointLines * 8;  // 96 uint4 = 1.5 KiB per lane
static_assert(kJointLines >= 8, "the fallback path's 8-line table shares the slot");

// the throughput point pass's table type and slot size (joint_pointpass, hsv_verify_hc.hpp)
template <int WA>
using PointPassTab = std::conditional_t<joint_pointpass<WA>(), GlobalJointTab, GlobalVarTab<(1 << (WA - 1)) + 1>>;
template <int WA>
constexpr int pointpass_lane_uint4() { return joint_pointpass<WA>() ? kJointLaneUint4 : vt_lane_uint4<WA>(); }


// one (pk, sig, msg) record into words
__device__ __forceinline__ void load_triple(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                            uint64_t sig_stride, const uint8_t *msg, uint64_t msg_stride,
                                            uint64_t i, uint32_t pkw[8], uint32_t sigw[16], uint32_t msgw[8]) {
  const uint4 *p = reinterpret_cast<const uint4 *>(pk + i * pk_stride);
  const uint4 *s = reinterpret_cast<const uint4 *>(sig + i * sig_stride);
  const uint4 *m = reinterpret_cast<const uint4 *>(msg + i * msg_stride);
  const uint4 p0 = p[0], p1 = p[1];
  const uint4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
  const uint4 m0 = m[0], m1 = m[1];
  pkw[0] = p0.x; pkw[1] = p0.y; pkw[2] = p0.z; pkw[3] = p0.w;
  pkw[4] = p1.x; pkw[5] = p1.y; pkw[6] = p1.z; pkw[7] = p1.w;
  sigw[0] = s0.x; sigw[1] = s0.y; sigw[2] = s0.z; sigw[3] = s0.w;
  sigw[4] = s1.x; sigw[5] = s1.y; sigw[6] = s1.z; sigw[7] = s1.w;
  sigw[8] = s2.x; sigw[9] = s2.y; sigw[10] = s2.z; sigw[11] = s2.w;
  sigw[12] = s3.x; sigw[13] = s3.y; sigw[14] = s3.z; sigw[15] = s3.w;
  msgw[0] = m0.x; msgw[1] = m0.y; msgw[2] = m0.z; msgw[3] = m0.w;
  msgw[4] = m1.x; msgw[5] = m1.y; msgw[6] = m1.z; msgw[7] = m1.w;
}

// 32 bytes (16-byte aligned) into eight words
__device__ __forceinline__ void load_words8(const uint8_t *p, uint32_t w[8]) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// item i's verdict through either output: the flag byte, the STRICT_OK bit
__device__ __forceinline__ void store_verdict(uint8_t *flags_out, uint32_t *strict_bits, uint32_t i, uint32_t f) {
  if (flags_out) flags_out[i] = (uint8_t)f;
  if (strict_bits && (f & kStrictOk)) atomicOr(&strict_bits[i >> 5], 1u << (i & 31u));
}

// The full-length path of item i, a fallback item (no short lattice pair).
// KREC = false: k is hashed here from R || A || the 32 bytes at msg + i *
// msg_stride.  KREC = true (whole messages: the prepass hashed them, and msg,
// of whatever type, is never touched): k mod l is words 10..17 of the item's
// prepass record (rec = the item's column, row stride `stride`).
template <int WA, int CB, bool KREC, class M, class VT>
__device__ __forceinline__ uint32_t verify_fallback_item(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                                         uint64_t sig_stride, M msg, uint64_t msg_stride,
                                                         uint32_t i, const uint32_t *rec, uint64_t stride,
                                                         const uint32_t *tb, VT &vt) {
  uint32_t pkw[8], sigw[16];
  if constexpr (KREC) {
    load_words8(pk + (uint64_t)i * pk_stride, pkw);
    load_words8(sig + (uint64_t)i * sig_stride, sigw);
    load_words8(sig + (uint64_t)i * sig_stride + 32, sigw + 8);
    sc k;
    HSV_UNROLL
    for (int j = 0; j < 8; ++j) k.v[j] = rec[(uint64_t)(10 + j) * stride];
    return verify_one_full_comb<WA, false, CB>(pkw, sigw, k, tb, vt);
  } else {
    uint32_t msgw[8];
    load_triple(pk, pk_stride, sig, sig_stride, msg, msg_stride, i, pkw, sigw, msgw);
    return verify_one_full_comb<WA, false, CB>(pkw, sigw, msgw, tb, vt);
  }
}

// Work counters of the comb kernels, zeroed before the launch (kCtrBytes
// reserved).  The class counters sit on 128-byte lines of their own: every
// block of a prepass adds to them while the launch runs.
struct HcCounters {
  uint32_t next;      // main pass: next item handed out
  uint32_t fb_count;  // deferred full-length items appended to fb_list
  uint32_t fb_next;   // fallback pass: next fb_list entry handed out
  uint32_t pad;
  uint32_t rnext;     // fused transaction launch: next 64-transaction record batch handed out
  uint32_t rdone;     // fused transaction launch: record batches published
  uint32_t pad2[26];
  struct Line {
    uint32_t count;
    uint32_t pad[31];
  } cls[kColClasses];  // dealt point pass: items on each column class's list (deal_append)
};
constexpr size_t kCtrBytes = 1024;
static_assert(sizeof(HcCounters) == 128 * (1 + kColClasses) && sizeof(HcCounters) <= kCtrBytes, "counter block");

// Dealing by column count (hsv_prep_kernel, hsv_msg_prep_kernel ->
// hsv_verify_hp_kernel).  The prepass appends every item that is not a
// fallback item to the list of its class (col_class, hsv_verify_hc.hpp): list
// k is cls_list + k * n, its length ctr->cls[k].count.  A wave finds its items
// of a class with one ballot and reserves their places in the block's count
// (LDS); the block then adds each class's count to the global counter once:
// one global atomic per class and block, not per lane or wave.
// The point pass then walks [fallback items | list 0 | list 1 | ...], longest
// need first: a 64-item batch holds items of one column count (two where it
// straddles a class boundary), so the wave-uniform column loop of
// straus_joint runs what its items need and not the count of the one long
// scalar in 60 that index order puts into most waves.
// Every thread of the block calls (two barriers inside); on: this lane has an
// item to append.
__device__ __forceinline__ void deal_append(HcCounters *ctr, uint32_t *cls_list, uint32_t n, bool on, uint32_t cls,
                                            uint32_t idx) {
  __shared__ uint32_t s_count[kColClasses], s_base[kColClasses];
  const uint32_t lane = threadIdx.x & 63u;
  if (threadIdx.x < (uint32_t)kColClasses) s_count[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t at = 0;  // this lane's place among the block's items of its class
  HSV_UNROLL
  for (uint32_t k = 0; k < (uint32_t)kColClasses; ++k) {
    const uint64_t m = __ballot(on && cls == k);
    if (m == 0) continue;
    const uint32_t lead = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(&s_count[k], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)lead);
    if (on && cls == k) at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)kColClasses) {
    const uint32_t c = s_count[threadIdx.x];
    s_base[threadIdx.x] = c ? atomicAdd(&ctr->cls[threadIdx.x].count, c) : 0u;
  }
  __syncthreads();
  if (on) cls_list[(uint64_t)cls * n + s_base[cls] + at] = idx;
}

// The dealt range's item at position p (< the lists' total length): prefix
// offsets from the counters, wave-uniform; the class is found per lane.
struct DealOffsets {
  uint32_t end[kColClasses];  // end[k] = cls[0] + .. + cls[k]
  __device__ __forceinline__ explicit DealOffsets(const HcCounters *ctr) {
    uint32_t s = 0;
    HSV_UNROLL
    for (int k = 0; k < kColClasses; ++k) {
      s += __builtin_amdgcn_readfirstlane(ctr->cls[k].count);
      end[k] = s;
    }
  }
  __device__ __forceinline__ uint32_t total() const { return end[kColClasses - 1]; }
  __device__ __forceinline__ uint32_t item(const uint32_t *cls_list, uint32_t n, uint32_t p) const {
    uint32_t k = 0, lo = 0;
    HSV_UNROLL
    for (int c = 0; c + 1 < kColClasses; ++c) {
      const bool past = p >= end[c];
      k = past ? (uint32_t)c + 1u : k;
      lo = past ? end[c] : lo;
    }
    return cls_list[(uint64_t)k * n + (p - lo)];
  }
};

// Device self-checks of the product kernels (a device failure must
// never become a silent reject).  Each launch gets
//   fault[2]  two words the host zeroed: fault[0] <- 1 when an item's final
//             point fails ge_is_sane (kFault), fault[1] <- 1 when a lane's
//             canary changed; written with plain stores once the work loop
//             is done (no atomics, so the words may live in pinned host memory);
//   canary    one word per lane slot of the workspace, set to the launch's
//             nonce when the lane starts and compared after every batch.
// The host turns a non-zero word into HSV_ERR_DEVICE_FAULT.
__device__ __forceinline__ void report_faults(uint32_t *fault, uint32_t bad) {
  if (bad & 1u) fault[0] = 1u;
  if (bad & 2u) fault[1] = 1u;
}

}  // namespace hsv
