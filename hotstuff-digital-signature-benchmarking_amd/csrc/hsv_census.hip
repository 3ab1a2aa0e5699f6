// The signer census kernels (hsv_census_keys*, hsv_census_transactions*):
// which 32-byte signer keys occur in a batch, and how often.  Nothing is
// decompressed or verified; the census says who signs, not whether they sign
// well.
//
// Two launches per call on the caller's stream, after one memset of the
// workspace (totals | slot words | counts, 8 bytes per slot):
//   1. hsv_census_count_kernel<MODE>  one lane per item loads its key words
//      (MODE: a key array, offset-addressed or fixed-size transactions), looks
//      them up in the `skip` committee (keytab_find).  The wave then folds its
//      equal keys in registers -- the key of the first open lane is
//      broadcast, a ballot counts the lanes that hold it, that lane leads the
//      group -- and the leaders insert side by side (census_insert,
//      hsv_census.hpp), each carrying its group's population count: one
//      compare-and-swap or add per distinct key per wave, so a batch of four
//      keys, each 2^18 times, is not 2^20 atomics on four words.
//      Members, malformed items, overflowed items, claimed slots and counted
//      items are wave totals, one atomic add each.
//   2. hsv_census_gather_kernel<MODE>  one lane per slot, after the first
//      launch has ended: a ballot of the occupied slots, one reservation per
//      wave, the claimer's 32 key bytes copied from the input and the count
//      beside them; entries from `distinct` on are zeroed, and one lane
//      writes the summary.
// Every hand-off is the kernel boundary between the two: no ready words and no
// polling.  What the workgroups of the first launch share, and why plain
// staleness cannot hurt it, is argued in hsv_census.hpp's head comment.
//
// The loops of the count kernel that touch the table are wave-uniform: the
// fold is steered by a ballot and the probe walk goes on while any lane is
// open, its body masked (tests/test_kernel_isa.py has the reason: a divergent
// loop around an atomic).  The lookup in `skip` is keytab_find as the
// route kernel of hsv_mempool.hip runs it, per lane, with no store inside.
// Stores are plain vector stores of 4 bytes or wider.
#include <hip/hip_runtime.h>

#include "hsv.h"
#include "hsv_census.hpp"
#include "hsv_internal.h"
#include "hsv_keytab.hpp"
#include "hsv_routed.hpp"  // mask_rank
#include "hsv_txhash.hpp"  // tx_load_words

namespace hsv {

constexpr int kCensusBlock = 256;
constexpr int kCensusKeys = 0, kCensusOffsets = 1, kCensusFixed = 2;  // MODE

// the call's totals, at the start of the workspace; zeroed with it
struct CensusTotals {
  uint32_t members, malformed, overflow, distinct, counted;  // written by the count kernel, in this order
  uint32_t next;                                             // the gather kernel's reservations
  uint32_t pad[2];
};
constexpr size_t kCensusHeadBytes = 256;
static_assert(sizeof(CensusTotals) <= kCensusHeadBytes, "the totals fit the workspace's head");

// Where item i's 32 key bytes lie.  kCensusKeys: base + i * stride, 16-byte
// aligned.  Transactions: bytes [len - 96, len - 64) of transaction i, which
// spans [offsets[i], offsets[i + 1]) (kCensusOffsets) or [i * stride, (i + 1) *
// stride) (kCensusFixed) of base, as tx_span of hsv_mempool.hip addresses it;
// malformed (load returns false, nothing loaded) when it is shorter than 96
// bytes or its offsets decrease.  A transaction's key is read in three aligned
// 16-byte chunks clamped to the last chunk that holds a byte of the
// transaction; each holds at least one byte of it, so every load is in bounds
// at any alignment of base.
template <int MODE>
struct CensusInput {
  const uint8_t *base;
  const uint64_t *offsets;
  uint64_t stride;
  __device__ __forceinline__ bool load(uint32_t i, uint32_t w[8]) const {
    if constexpr (MODE == kCensusKeys) {
      const uint4 *p = reinterpret_cast<const uint4 *>(base + (uint64_t)i * stride);
      const uint4 a = p[0], b = p[1];
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
      w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
      return true;
    } else {
      uint64_t lo, hi;
      if constexpr (MODE == kCensusOffsets) {
        lo = offsets[i];
        hi = offsets[(uint64_t)i + 1];
      } else {
        lo = (uint64_t)i * stride;
        hi = lo + stride;
      }
      if (!(hi >= lo && hi - lo >= 96)) return false;
      const uintptr_t b = reinterpret_cast<uintptr_t>(base);
      const uint4 *q = reinterpret_cast<const uint4 *>(b & ~uintptr_t(15));
      const uint64_t start = (uint64_t)(b & 15u) + lo;
      const uint64_t key = start + (hi - lo) - 96;
      auto ld = [q](uint64_t k, uint32_t c[4]) {
        const uint4 v = q[k];
        c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
      };
      tx_load_words<8>(ld, key >> 4, (uint32_t)(key & 15u), (start + (hi - lo) - 1) >> 4, w);
      return true;
    }
  }
};

template <int MODE>
__global__ void __launch_bounds__(kCensusBlock)
hsv_census_count_kernel(CensusInput<MODE> in, uint32_t n, uint32_t *__restrict__ tab, uint32_t *__restrict__ counts,
                        uint32_t mask, uint64_t seed, const uint32_t *__restrict__ keytab, uint32_t keymask,
                        uint64_t keyseed, const uint8_t *__restrict__ pks, uint32_t nkeys,
                        CensusTotals *__restrict__ totals) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t i64 = (uint64_t)blockIdx.x * kCensusBlock + threadIdx.x;
  if (i64 - lane >= n) return;  // whole wave past the end
  const uint32_t i = i64 < n ? (uint32_t)i64 : n - 1u;
  uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const bool ok = i64 < n && in.load(i, w);
  const bool malformed = i64 < n && !ok;
  bool member = false;
  if (ok && nkeys) member = keytab_find(keytab, keymask, keyseed, pks, w) < nkeys;
  const uint64_t mm = __ballot(member), bm = __ballot(malformed);
  // fold the wave's equal keys: the first lane that holds a key leads it and
  // carries the group's population count (registers only, no memory)
  const uint64_t pending = __ballot(ok && !member);
  uint64_t todo = pending;
  bool leads = false;
  uint32_t c = 0;
  while (todo) {
    const int first = __ffsll((unsigned long long)todo) - 1;
    uint32_t kw[8];
    HSV_UNROLL
    for (int k = 0; k < 8; ++k) kw[k] = (uint32_t)__builtin_amdgcn_readlane((int)w[k], first);
    const uint64_t group = __ballot(census_key_eq(w, kw)) & todo;  // the first lane's own bit is among them
    const bool me = lane == (uint32_t)first;
    leads = me ? true : leads;
    c = me ? (uint32_t)__popcll(group) : c;
    todo &= ~group;
  }
  // the leaders insert side by side; the walk is the wave's (census_insert)
  const uint32_t r = census_insert(tab, counts, mask, seed, in, i, w, c, leads);
  const uint32_t claimed = (uint32_t)__popcll(__ballot(r == kCensusClaimed));
  uint32_t overflow = 0;
  for (uint64_t om = __ballot(r == kCensusOverflow); om; om &= om - 1ull)  // rare: a full neighbourhood
    overflow += (uint32_t)__builtin_amdgcn_readlane((int)c, __ffsll((unsigned long long)om) - 1);
  const uint32_t counted = (uint32_t)__popcll(pending) - overflow;
  // lanes 0..4 add the wave's totals, one atomic each, one region
  const uint32_t v = lane == 0u   ? (uint32_t)__popcll(mm)
                     : lane == 1u ? (uint32_t)__popcll(bm)
                     : lane == 2u ? overflow
                     : lane == 3u ? claimed
                                  : counted;
  if (lane < 5u && v) HSV_CENSUS_ADD(&totals->members + lane, v);
}

template <int MODE>
__global__ void __launch_bounds__(kCensusBlock)
hsv_census_gather_kernel(CensusInput<MODE> in, uint64_t n, const uint32_t *__restrict__ tab,
                         const uint32_t *__restrict__ counts, uint32_t slots, CensusTotals *__restrict__ totals,
                         uint4 *__restrict__ keys_out, uint32_t *__restrict__ counts_out,
                         unsigned long long *__restrict__ summary) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * kCensusBlock + threadIdx.x;  // slots <= 2^22
  // the first launch's totals: it has ended
  const uint32_t distinct = min(totals->distinct, slots);
  const uint32_t e = s < slots ? tab[s] : 0u;
  const uint64_t occupied = __ballot(e != 0u);
  uint32_t base = 0;
  if (lane == 0u && occupied) base = atomicAdd(&totals->next, (uint32_t)__popcll(occupied));
  base = (uint32_t)__shfl((int)base, 0);
  const uint32_t pos = base + mask_rank(occupied, lane);
  if (e != 0u && pos < distinct) {  // (pos < distinct always: one reservation per claimed slot)
    uint32_t w[8];
    (void)in.load(min(e - 1u, (uint32_t)(n - 1u)), w);  // the claimer: well-formed, below n
    keys_out[2ull * pos] = make_uint4(w[0], w[1], w[2], w[3]);
    keys_out[2ull * pos + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    counts_out[pos] = counts[s];
  }
  if (s < slots && s >= distinct) {  // the tail: entries no reservation reaches
    keys_out[2ull * s] = make_uint4(0u, 0u, 0u, 0u);
    keys_out[2ull * s + 1] = make_uint4(0u, 0u, 0u, 0u);
    counts_out[s] = 0u;
  }
  if (s == 0u) {  // hsv_census_summary, six 8-byte words
    summary[0] = n;
    summary[1] = totals->counted;
    summary[2] = totals->members;
    summary[3] = totals->malformed;
    summary[4] = totals->overflow;
    summary[5] = distinct;  // distinct, reserved = 0
  }
}

namespace {

template <int MODE>
hipError_t launch_census(const uint8_t *in, const uint64_t *offsets, uint64_t stride, uint32_t n, uint32_t slots,
                         uint64_t seed, const uint32_t *keytab, uint32_t keymask, uint64_t keyseed, const uint8_t *pks,
                         uint32_t nkeys, uint8_t *keys_out, uint32_t *counts_out, void *summary, hipStream_t stream) {
  const size_t bytes = kCensusHeadBytes + 8 * (size_t)slots;
  Workspace ws(nullptr, 0, bytes, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *p = ws.get();
  CensusTotals *totals = reinterpret_cast<CensusTotals *>(p);
  uint32_t *tab = reinterpret_cast<uint32_t *>(p + kCensusHeadBytes);
  uint32_t *counts = tab + slots;
  const CensusInput<MODE> input{in, offsets, stride};
  hipError_t e = hipMemsetAsync(p, 0, bytes, stream);
  if (e == hipSuccess && n) {
    const uint32_t grid = (uint32_t)(((uint64_t)n + kCensusBlock - 1) / kCensusBlock);
    hipLaunchKernelGGL(hsv_census_count_kernel<MODE>, dim3(grid), dim3(kCensusBlock), 0, stream, input, n, tab, counts,
                       slots - 1u, seed, keytab, keymask, keyseed, pks, nkeys, totals);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hsv_census_gather_kernel<MODE>, dim3((slots + kCensusBlock - 1) / kCensusBlock),
                       dim3(kCensusBlock), 0, stream, input, (uint64_t)n, tab, counts, slots, totals,
                       reinterpret_cast<uint4 *>(keys_out), counts_out, static_cast<unsigned long long *>(summary));
    e = hipGetLastError();
  }
  return ws.done(e);
}

}  // namespace
}  // namespace hsv

static_assert(sizeof(hsv_census_summary) == 48, "six 8-byte words, as the gather kernel writes them");

// One census of n items on `stream` (hsv_internal.h): mode 0 a key array (in
// and stride multiples of 16), 1 transactions addressed by offsets, 2
// fixed-size transactions of `stride` bytes.
extern "C" hipError_t hsv_launch_census(int mode, const uint8_t *in, const uint64_t *offsets, uint64_t stride,
                                        uint32_t n, uint32_t slots, uint64_t seed, const uint32_t *keytab,
                                        uint32_t keymask, uint64_t keyseed, const uint8_t *pks, uint32_t nkeys,
                                        uint8_t *keys_out, uint32_t *counts_out, void *summary, hipStream_t stream) {
  if (!hsv::census_slots_ok(slots) || !keys_out || !counts_out || !summary || (n && !in) ||
      (nkeys && (!keytab || !pks)) || (mode == hsv::kCensusOffsets && n && !offsets))
    return hipErrorInvalidValue;
  switch (mode) {
    case hsv::kCensusKeys:
      return hsv::launch_census<hsv::kCensusKeys>(in, nullptr, stride, n, slots, seed, keytab, keymask, keyseed, pks,
                                                  nkeys, keys_out, counts_out, summary, stream);
    case hsv::kCensusOffsets:
      return hsv::launch_census<hsv::kCensusOffsets>(in, offsets, 0, n, slots, seed, keytab, keymask, keyseed, pks,
                                                     nkeys, keys_out, counts_out, summary, stream);
    case hsv::kCensusFixed:
      return hsv::launch_census<hsv::kCensusFixed>(in, nullptr, stride, n, slots, seed, keytab, keymask, keyseed, pks,
                                                   nkeys, keys_out, counts_out, summary, stream);
  }
  return hipErrorInvalidValue;
}
