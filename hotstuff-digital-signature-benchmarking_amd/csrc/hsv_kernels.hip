// The generic verifier's throughput kernels and its launch dispatch.
//
//  hsv_prep_kernel       pass 1: one lane per item, the scalar work, into a
//                        prepass record (hsv_verify_hc.hpp)
//  hsv_verify_hp_kernel  pass 2: the persistent point pass over those records;
//                        its KREC instantiation serves whole messages behind
//                        hsv_msgs.hip's prepass
//  hsv_mad_peak_kernel   issue-rate probe of v_mad_u64_u32 for the roofline
//                        denominator (bench.py reports against it)
//
// Host side: the workspace pool (hsv_ws_malloc), launch_hp, and the
// hsv_launch_* entry points, which send at most kPairMax items to the
// one-launch latency forms of hsv_small.hip; the test hooks' state (lattice
// bound, injection mode, canary nonce, the message route switch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <unordered_map>

#include "hsv_internal.h"
#include "hsv_verify_core.hpp"
#include "hsv_verify_hc.hpp"
#include "hsv_pointpass.hpp"

namespace hsv {

#ifdef HSV_PHASE_CLOCKS  // tools/phase_clock_probe.py only: 8 words per 64-item batch of the point pass
constexpr uint32_t kPhaseCap = 1u << 16;
__device__ uint64_t g_phase_clk[kPhaseCap * 8];
#endif

// Two-pass form (hsv_verify_hc.hpp, prep_scalars / verify_one_prepped).
// Pass 1: one lane per item, scalar work only; records to `rec` (SoA, row
// stride n), fallback items appended to fb_list, every other item to the list
// of its column class (deal_append, hsv_pointpass.hpp; cls_list null: no lists,
// the point pass runs in index order).
template <int WA>
__global__ void __launch_bounds__(kBlock)
hsv_prep_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                uint64_t sig_stride, const uint8_t *__restrict__ msg, uint64_t msg_stride, uint32_t n,
                uint32_t *__restrict__ rec, HcCounters *__restrict__ ctr, uint32_t *__restrict__ fb_list,
                uint32_t *__restrict__ cls_list, int lat_bits) {
  // The prepass usually runs beside the previous batch's point pass (another
  // stream, or the previous chunk of a host pipeline), whose waves keep every
  // SIMD's VALU busy; this batch's point pass cannot start before the prepass
  // ends.  Highest wave priority: the SIMD issues the prepass's waves first.
  __builtin_amdgcn_s_setprio(3);
  const uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
  bool listed = false;
  uint32_t cls = 0;
  if (idx < n) {
    uint32_t pkw[8], sigw[16], msgw[8];
    load_triple(pk, pk_stride, sig, sig_stride, msg, msg_stride, idx, pkw, sigw, msgw);
    const bool fb =
        prep_scalars<WA, PutPlain, pointpass_digit_bits<WA>()>(pkw, sigw, msgw, rec + idx, n, lat_bits, &cls);
    if (fb) fb_list[atomicAdd(&ctr->fb_count, 1u)] = idx;
    listed = !fb;
  }
  if (cls_list) deal_append(ctr, cls_list, n, listed, cls, idx);  // the whole block: barriers inside
}

// Pass 2: persistent grid, 64-item batches from ctr->next over a virtual
// range [fallback items | all items].  Fallback batches come first and run
// the full-length path; in the regular range a fallback item's lane computes
// nothing it stores.  strict_bits is zeroed before the launch and every
// batch ORs its bits in (a word can receive bits from both ranges).
// Dealt (cls_list not null, the default): the regular range is the prepass's
// class lists end to end, longest column need first, without the fallback
// items; a batch is 64 consecutive positions of it, the lane's item comes
// from the list, and a lane past the end redoes the batch's first item and
// stores nothing.  A batch's items then share no strict_bits words: one
// atomicOr per accepted item, as the fallback range.
// KREC (messages of any length, hsv_launch_verify_msgs): the prepass
// (hsv_msg_prep_kernel, hsv_msgs.hip) has hashed the whole message, and this
// pass never touches message bytes (msg is unused): a fallback item's k mod l
// comes from the b words of its record, and an item the prepass marked
// kPrepVoid (malformed message range) gets flags 0.
template <int WA, int WAVES, int CB, bool KREC = false>
__global__ void __launch_bounds__(kBlock, WAVES)
hsv_verify_hp_kernel(const uint8_t *__restrict__ pk, uint64_t pk_stride, const uint8_t *__restrict__ sig,
                     uint64_t sig_stride, const uint8_t *__restrict__ msg, uint64_t msg_stride, uint32_t n,
                     uint8_t *__restrict__ flags_out, uint32_t *__restrict__ strict_bits,
                     uint4 *__restrict__ vt_ws, const uint32_t *__restrict__ comb_b,
                     const uint32_t *__restrict__ rec, HcCounters *__restrict__ ctr,
                     const uint32_t *__restrict__ fb_list, const uint32_t *__restrict__ cls_list,
                     uint32_t *__restrict__ canary, uint32_t nonce, uint32_t inject, uint32_t *__restrict__ fault) {
  constexpr bool JOINT = joint_pointpass<WA>();
  const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
  PointPassTab<WA> vt{vt_ws + (uint64_t)slot * pointpass_lane_uint4<WA>(), inject};
  const uint32_t lane = threadIdx.x & 63u;
  canary[slot] = nonce;
  uint32_t bad = 0;
  const uint32_t nfb = __builtin_amdgcn_readfirstlane(ctr->fb_count);
  const uint32_t fb_end = (nfb + 63u) & ~63u;
  const uint32_t words = (n + 31u) / 32u;
  const bool deal = cls_list != nullptr;
  const DealOffsets off(ctr);
  const uint32_t nreg = deal ? off.total() : n;  // length of the regular range
#ifdef HSV_PHASE_CLOCKS
  uint32_t nbw = 0;  // batches this wave has taken
#endif
  for (;;) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr->next, 64u);
    base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
    if (base >= fb_end + nreg) break;
    if (inject == kInjectCanary) canary[slot] = ~nonce;
    if (base < fb_end) {
      const uint32_t j = base + lane;
      const bool valid = j < nfb;
      const uint32_t idx = fb_list[valid ? j : base];
      const uint32_t f = verify_fallback_item<WA, CB, KREC>(pk, pk_stride, sig, sig_stride, msg, msg_stride, idx,
                                                            rec + idx, n, comb_b, vt);
      bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
      if (valid) {  // (tried: store_verdict; 51,326 / 48,780 instructions against 51,319 / 48,777)
        if (flags_out) flags_out[idx] = (uint8_t)f;
        if (strict_bits && (f & kStrictOk)) atomicOr(&strict_bits[idx >> 5], 1u << (idx & 31u));
      }
      continue;
    }
    const uint32_t b0 = base - fb_end;
    const bool valid = b0 + lane < nreg;
    const uint32_t pos = valid ? b0 + lane : b0;
    const uint32_t li = deal ? min(off.item(cls_list, n, pos), n - 1u) : pos;
    uint32_t pkw[8], rw[8];
    load_words8(pk + (uint64_t)li * pk_stride, pkw);
    load_words8(sig + (uint64_t)li * sig_stride, rw);
    const uint32_t meta = rec[18ull * n + li];
    const bool own = valid && !(meta & kPrepFallback);
#ifdef HSV_PHASE_CLOCKS
    uint64_t clk[5];
    ++nbw;
    const uint64_t cyc0 = clock64();
    clk[0] = wall_clock64();
    const uint32_t f = verify_one_prepped<WA, CB, JOINT>(pkw, rw, rec + li, n, meta, comb_b, vt, clk);
    clk[4] = wall_clock64();
    {  // lanes 0..7 store one word each (one store region keeps the work loop uniform)
      uint64_t v = 1;
      HSV_UNROLL
      for (int j = 0; j < 5; ++j) v = lane == (uint32_t)j ? clk[j] : v;
      v = lane == 5u ? (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) : v;  // HW_ID
      v = lane == 6u ? ((uint64_t)blockIdx.x << 8 | nbw) : v;
      v = lane == 7u ? (0x100u | (uint64_t)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) |  // XCC_ID
                        ((clock64() - cyc0) << 16))  // shader clocks over the batch
                     : v;
      if (lane < 8u && b0 / 64u < kPhaseCap) g_phase_clk[(uint64_t)(b0 / 64u) * 8u + lane] = v;
    }
#else
    const uint32_t f = verify_one_prepped<WA, CB, JOINT>(pkw, rw, rec + li, n, meta, comb_b, vt);
#endif
    bad |= ((f & kFault) ? 1u : 0u) | (canary[slot] != nonce ? 2u : 0u);
    const uint32_t fo = KREC && (meta & kPrepVoid) ? 0u : f;
    if (own && flags_out) flags_out[li] = (uint8_t)fo;
    if (deal) {
      if (own && strict_bits && (fo & kStrictOk)) atomicOr(&strict_bits[li >> 5], 1u << (li & 31u));
    } else if (strict_bits) {
      const uint64_t mask = __ballot(own && (fo & kStrictOk));
      const uint32_t w = b0 / 32u + lane;
      const uint32_t part = lane ? (uint32_t)(mask >> 32) : (uint32_t)mask;
      if (lane < 2u && w < words && part) atomicOr(&strict_bits[w], part);
    }
  }
  report_faults(fault, bad);
}

// ---- streamed host batches (round 4) ---------------------------------------
// (Round 4 also had a streamed host form here: one persistent launch reading
// the records through the pinned staging's device mapping while the host was
// still packing them.  It measured slower than the chunked copy pipeline,
// 11.7 against 9.9 ms per 2^20 (profiles/r04d_host_api_ab.txt), and was
// removed from the library in round 5; it is in git history at 394d4d2.)

// ---- v_mad_u64_u32 issue-rate probe -------------------------------------
// 8 independent accumulation chains, 16 mads per asm statement (the compiler
// puts an s_nop after every asm statement that writes an SGPR, so one mad per
// statement would measure mad + s_nop).
constexpr int kPeakIters = 2048;

#define HSV_PEAK_MAD(c) "v_mad_u64_u32 %" #c ", s[40:41], %8, %9, %" #c "\n\t"
__global__ void __launch_bounds__(256) hsv_mad_peak_kernel(uint32_t *sink, uint32_t seed) {
  const uint32_t t = threadIdx.x + blockIdx.x * blockDim.x + seed;
  uint64_t x0 = t, x1 = t + 1, x2 = t + 2, x3 = t + 3, x4 = t + 4, x5 = t + 5, x6 = t + 6, x7 = t + 7;
  const uint32_t a = t | 1u, b = t * 3u + 7u;
  for (int it = 0; it < kPeakIters; ++it)
    asm volatile(HSV_PEAK_MAD(0) HSV_PEAK_MAD(1) HSV_PEAK_MAD(2) HSV_PEAK_MAD(3) HSV_PEAK_MAD(4) HSV_PEAK_MAD(5)
                 HSV_PEAK_MAD(6) HSV_PEAK_MAD(7) HSV_PEAK_MAD(0) HSV_PEAK_MAD(1) HSV_PEAK_MAD(2) HSV_PEAK_MAD(3)
                 HSV_PEAK_MAD(4) HSV_PEAK_MAD(5) HSV_PEAK_MAD(6) HSV_PEAK_MAD(7)
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7)
                 : "v"(a), "v"(b)
                 : "s40", "s41");
  const uint64_t r = x0 ^ x1 ^ x2 ^ x3 ^ x4 ^ x5 ^ x6 ^ x7;
  if ((uint32_t)(r ^ (r >> 32)) == 0x9e3779b9u) sink[0] = 1u;
}
#undef HSV_PEAK_MAD

}  // namespace hsv

// Kernel variant ids (hsv_set_variant, test library).  The library builds two
// (kVariantIds below):
//  19: two passes -- scalar prepass (hsv_prep_kernel), then the persistent
//      point pass with the fallback items dealt out first (WA 4, 3 waves/SIMD,
//      wide comb of B)
//  21: the default: 19's kernels above 2^13 items; at or below, the latency
//      forms (quad / joint / row / pair)
// Ids 0-18, 20 and 22 were rounds 1-4's measured alternatives; they left the
// source in round 5 (git history before that cleanup).  The id space stays
// [0, 22) so old measurement records keep their meaning.
extern "C" int hsvi_num_variants(void) { return 22; }

namespace {
struct WsPools {
  std::mutex mu;
  std::unordered_map<int, hipMemPool_t> pools;  // device -> the library's workspace pool
};
WsPools &ws_pools() {
  static WsPools p;
  return p;
}
}  // namespace

// hsv_shutdown: return the pools' free blocks to the driver (blocks still in
// use by enqueued work stay)
extern "C" void hsv_ws_trim(void) {
  WsPools &wp = ws_pools();
  std::lock_guard<std::mutex> lk(wp.mu);
  for (auto &kv : wp.pools) (void)hipMemPoolTrimTo(kv.second, 0);
}

// Free memory the pool keeps between calls (HSV_WS_POOL_KEEP_MB, default 4096
// MiB; 0 returns every block at each synchronisation): a freed block is reused
// only by later launches on the same stream, so an application that spreads
// batches over many streams would otherwise keep one workspace per stream
// (about 0.5 GB for a 2^20-item batch) out of its own allocator's reach.  Above
// the threshold the pool hands idle blocks back to the driver whenever a
// stream or event synchronisation observes their frees.
static uint64_t ws_pool_keep_bytes() {
  static const uint64_t b = [] {
    long long mb = 4096;
    if (const char *v = std::getenv("HSV_WS_POOL_KEEP_MB")) mb = std::atoll(v);
    if (mb < 0) mb = 0;
    return (uint64_t)mb << 20;
  }();
  return b;
}

extern "C" hipError_t hsv_ws_malloc(void **p, size_t bytes, hipStream_t stream) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  WsPools &wp = ws_pools();
  hipMemPool_t pool = nullptr;
  {
    std::lock_guard<std::mutex> lk(wp.mu);
    auto &pools = wp.pools;
    auto it = pools.find(dev);
    if (it == pools.end()) {
      hipMemPoolProps props = {};
      props.allocType = hipMemAllocationTypePinned;
      props.handleTypes = hipMemHandleTypeNone;
      props.location.type = hipMemLocationTypeDevice;
      props.location.id = dev;
      e = hipMemPoolCreate(&pool, &props);
      if (e != hipSuccess) return e;
      uint64_t keep = ws_pool_keep_bytes();
      e = hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
      if (e != hipSuccess) return e;
      // A block is reused only on the stream that freed it (stream order
      // alone makes that safe).  No cross-stream reuse of any kind:
      // - internal dependencies would make a new launch wait for another
      //   stream, and launches on different streams (consecutive batches,
      //   pipelined chunks) must be free to overlap;
      // - with event-dependency and opportunistic reuse, a launch on a
      //   stream that had waited (through a third stream) on an event of the
      //   freeing stream got a block still in use by a running launch there:
      //   two point passes shared one work counter and prepass records and
      //   returned wrong flags (round 5, tools/mempool_split_probe.py,
      //   tests/test_device_model.py::test_batches_behind_cross_stream_event_chains).
      int no = 0;
      for (hipMemPoolAttr a : {hipMemPoolReuseAllowInternalDependencies, hipMemPoolReuseFollowEventDependencies,
                               hipMemPoolReuseAllowOpportunistic}) {
        e = hipMemPoolSetAttribute(pool, a, &no);
        if (e != hipSuccess) return e;
      }
#ifdef HSV_WS_POOL_PROBE
      // Measurement builds only (tools/build_ab_libs.sh): one
      // cross-stream reuse policy back on -- 1 event dependencies, 2
      // opportunistic -- to pin which one handed a running launch's block on.
      {
        int yes = 1;
        e = hipMemPoolSetAttribute(pool, HSV_WS_POOL_PROBE == 1 ? hipMemPoolReuseFollowEventDependencies
                                                                : hipMemPoolReuseAllowOpportunistic, &yes);
        if (e != hipSuccess) return e;
      }
#endif
      it = pools.emplace(dev, pool).first;
    }
    pool = it->second;
  }
  e = hipMallocFromPoolAsync(p, bytes, pool, stream);
  if (e == hipErrorOutOfMemory) {
    // Blocks freed on other streams are never reused here.  When the device
    // runs out: wait for the calling stream (its own frees complete), hand
    // every idle block of the pool back to the driver -- blocks freed on
    // idle or destroyed streams among them -- and try once more; otherwise
    // the caller gets the out-of-memory error.  No device-wide wait: that
    // would stall every stream of the application, and blocks still held by
    // launches running on other streams stay theirs.
    (void)hipGetLastError();
    hsvi_resident_pause(1);
    if (hipStreamSynchronize(stream) == hipSuccess && hipMemPoolTrimTo(pool, 0) == hipSuccess)
      e = hipMallocFromPoolAsync(p, bytes, pool, stream);
    hsvi_resident_pause(0);
    if (e == hipSuccess) (void)hipGetLastError();
  }
  return e;
}

namespace {

// Lattice bound of the comb-path prepass (hsvi_set_lattice_bits; tests lower
// it to 133 so the lattice-fallback fixtures take the full-length path).
std::atomic<int> g_lat_bits{hsv::kLatCombBits};

// Fault injection mode of the launches the calling thread issues
// (hsvi_set_inject; only libhsv_test.so exports a setter).  Thread-scoped: a
// test that injects on one thread leaves every other thread's calls alone.
thread_local uint32_t t_inject = hsv::kInjectNone;

// Dealing by column count in the calling thread's two-launch point passes
// (hsvi_set_deal; only libhsv_test.so exports a setter): bit 0 on (the
// default), off = index order, for parity tests and A/B runs; bit 1: each such
// launch waits for its stream and keeps its class counts (hsvi_deal_counts).
#ifndef HSV_DEAL_DEFAULT  // 0: A/B builds in index order (tools/build_ab_libs.sh)
#define HSV_DEAL_DEFAULT 1
#endif
thread_local int t_deal = HSV_DEAL_DEFAULT;
thread_local uint32_t t_deal_counts[hsv::kColClasses] = {};

// HSV_TX_FUSED=0: transactions as the record kernel + point pass pair (the
// round-5 form), for A/B runs; read once per process.
bool tx_fused_enabled() {
  static const bool on = [] {
    const char *v = std::getenv("HSV_TX_FUSED");
    return !(v && v[0] == '0');
  }();
  return on;
}

// Per-launch canary nonce: odd, so never 0 (zeroed memory) or all-ones.
uint32_t next_nonce() {
  static std::atomic<uint32_t> ctr{0x9e3779b9u};
  return (ctr.fetch_add(0x61c88646u) * 2654435761u) | 1u;
}


// Two-pass launch (variants 19/20): prepass over all items, then the
// persistent point pass.  Workspace: per-lane tables | counters (kCtrBytes) |
// fallback list (4 B per item) | prep records (kPrepWords x 4 B per item).
// Transactions whose records the prepass writes itself (hsv_launch_tx_prep):
// the point pass then reads pk / R (and, for fallback items, s and the
// digest) from `records` at stride 128.
struct TxPrep {
  const uint8_t *txs;
  const uint64_t *offsets;
  uint64_t tx_size;
  uint8_t *records;
};
// Messages of any length (hsv_launch_verify_msgs): the prepass is
// hsv_launch_msg_prep, which hashes each whole message, and the point pass is
// the KREC instantiation, which never reads a message.
struct MsgPrep {
  const uint8_t *msgs;
  const uint64_t *offsets;
  uint64_t msg_len, msg_stride;
};

template <int WA, int WAVES, int CB>
hipError_t launch_hp(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                     const uint8_t *msg, uint64_t msg_stride, uint32_t n, uint8_t *flags_out,
                     uint32_t *strict_bits, const uint32_t *comb_b, uint32_t *fault, hipStream_t stream,
                     const TxPrep *tx = nullptr, void *ws_in = nullptr, size_t ws_cap = 0,
                     size_t *ws_need = nullptr, const MsgPrep *mp = nullptr) {
  const void *kern = mp ? reinterpret_cast<const void *>(hsv::hsv_verify_hp_kernel<WA, WAVES, CB, true>)
                        : reinterpret_cast<const void *>(hsv::hsv_verify_hp_kernel<WA, WAVES, CB>);
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  static std::mutex mu;
  static std::unordered_map<int, std::pair<int, int>> slots_per_dev;  // device, form -> (blocks per CU, CUs)
  int bpc = 1, cus = 1;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = slots_per_dev.find(2 * dev + (mp ? 1 : 0));
    if (it == slots_per_dev.end()) {
      int b = 0, c = 0;
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kern, hsv::kBlock, 0);
      if (e != hipSuccess) return e;
      e = hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
      if (e != hipSuccess) return e;
      it = slots_per_dev.emplace(2 * dev + (mp ? 1 : 0), std::make_pair(std::max(1, b), std::max(1, c))).first;
    }
    bpc = it->second.first;
    cus = it->second.second;
  }
  // A persistent grid must fit the device at once: its blocks leave when the
  // work counter runs out, and a block still waiting for a place would hold
  // the launch open.  Once the resident latency service has run in this
  // process its block may sit on one CU (and a request from another thread
  // may relaunch it while this grid is dispatched), so the grid then leaves
  // one CU's worth of blocks out (1/256 of the slots).
  // Transactions of the product form run as ONE fused launch (records,
  // prepass and point pass; hsv_mempool.hip) unless HSV_TX_FUSED=0 selects
  // the record kernel + point pass pair; its grid follows its own occupancy.
  const bool fused = tx && WA == 4 && WAVES == HSV_HP_WAVES && CB == 16 && tx_fused_enabled() &&
                     (uint64_t)n * 128u <= 0xffffffffull && hsv_tx_fused_blocks_per_cu(dev) > 0;
  if (fused) bpc = std::min(bpc, hsv_tx_fused_blocks_per_cu(dev));
  const int resident = bpc * (hsvi_resident_started() && cus > 1 ? cus - 1 : cus);
  const uint32_t blocks_needed = (n + hsv::kBlock - 1) / hsv::kBlock;
  const uint32_t grid = std::min<uint32_t>(blocks_needed, (uint32_t)resident);
  const size_t ws_bytes = (size_t)grid * hsv::kBlock * hsv::pointpass_lane_uint4<WA>() * sizeof(uint4);
  const size_t canary_bytes = ((size_t)grid * hsv::kBlock * sizeof(uint32_t) + 255) & ~(size_t)255;
  const size_t fb_bytes = (size_t)n * sizeof(uint32_t);
  const size_t rec_bytes = (size_t)n * hsv::kPrepWords * sizeof(uint32_t);
  const size_t ready_bytes = fused ? (((size_t)(n + 63u) / 64u) * sizeof(uint32_t) + 255) & ~(size_t)255 : 0;
  // class lists of the dealt point pass (one of n entries per class: an item
  // sits on one of them).  The transaction forms keep index order: the fused
  // launch ties point batches to record batches, and the pair's record kernel
  // keeps no lists.  The size does not depend on the test switch.
  const bool lists = !tx && hsv::joint_pointpass<WA>();
  const size_t cls_bytes = lists ? (size_t)n * hsv::kColClasses * sizeof(uint32_t) : 0;
  const size_t need = ws_bytes + hsv::kCtrBytes + canary_bytes + fb_bytes + rec_bytes + ready_bytes + cls_bytes;
  if (ws_need) {  // size query only
    *ws_need = need;
    return hipSuccess;
  }
  hsv::Workspace ws(ws_in, ws_cap, need, stream);
  if (ws.status() != hipSuccess) return ws.status();
  uint8_t *ws8 = ws.get();
  uint4 *vt_ws = reinterpret_cast<uint4 *>(ws8);
  hsv::HcCounters *ctr = reinterpret_cast<hsv::HcCounters *>(ws8 + ws_bytes);
  uint8_t *p = ws8 + ws_bytes + hsv::kCtrBytes;
  uint32_t *canary = reinterpret_cast<uint32_t *>(p);
  uint32_t *fb_list = reinterpret_cast<uint32_t *>(p += canary_bytes);
  uint32_t *rec = reinterpret_cast<uint32_t *>(p += fb_bytes);
  uint32_t *ready = reinterpret_cast<uint32_t *>(p += rec_bytes);
  uint32_t *cls_list = reinterpret_cast<uint32_t *>(p += ready_bytes);
  if (!lists || !(t_deal & 1)) cls_list = nullptr;  // index order
  e = hipMemsetAsync(ctr, 0, sizeof(hsv::HcCounters), stream);
  if (e == hipSuccess && strict_bits) e = hipMemsetAsync(strict_bits, 0, (size_t)((n + 31u) / 32u) * 4u, stream);
  if (e == hipSuccess && fused) {
    e = hipMemsetAsync(ready, 0, ready_bytes, stream);
    if (e == hipSuccess)
      e = hsv_launch_tx_fused(grid, tx->txs, tx->offsets, tx->tx_size, n, tx->records, rec, ctr, fb_list, ready,
                              g_lat_bits.load(), flags_out, strict_bits, vt_ws, comb_b, canary, next_nonce(), t_inject,
                              fault, stream);
    return ws.done(e);
  }
  if (e == hipSuccess && tx) {
    static_assert(WA == 4, "hsv_launch_tx_prep writes the WA = 4 point pass's prepass record");
    e = hsv_launch_tx_prep(tx->txs, tx->offsets, tx->tx_size, n, tx->records, rec, &ctr->fb_count, fb_list,
                           g_lat_bits.load(), stream);
    pk = tx->records;
    sig = tx->records + 32;
    msg = tx->records + 96;
    pk_stride = sig_stride = msg_stride = 128;
  } else if (e == hipSuccess && mp) {
    static_assert(WA == 4, "hsv_launch_msg_prep writes the WA = 4 point pass's prepass record");
    e = hsv_launch_msg_prep(pk, pk_stride, sig, sig_stride, mp->msgs, mp->offsets, mp->msg_len, mp->msg_stride, n,
                            rec, ctr, fb_list, cls_list, g_lat_bits.load(), stream);
  } else if (e == hipSuccess) {
    hipLaunchKernelGGL((hsv::hsv_prep_kernel<WA>), dim3(blocks_needed), dim3(hsv::kBlock), 0, stream, pk, pk_stride,
                       sig, sig_stride, msg, msg_stride, n, rec, ctr, fb_list, cls_list, g_lat_bits.load());
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    if (mp) {
      hipLaunchKernelGGL((hsv::hsv_verify_hp_kernel<WA, WAVES, CB, true>), dim3(grid), dim3(hsv::kBlock), 0, stream,
                         pk, pk_stride, sig, sig_stride, nullptr, 0, n, flags_out, strict_bits, vt_ws, comb_b, rec,
                         ctr, fb_list, cls_list, canary, next_nonce(), t_inject, fault);
    } else {
      hipLaunchKernelGGL((hsv::hsv_verify_hp_kernel<WA, WAVES, CB>), dim3(grid), dim3(hsv::kBlock), 0, stream, pk,
                         pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits, vt_ws, comb_b, rec,
                         ctr, fb_list, cls_list, canary, next_nonce(), t_inject, fault);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess && (t_deal & 2)) {  // test hook: this launch's class counts, read back before the block is freed
    hsv::HcCounters h;
    e = hipMemcpyAsync(&h, ctr, sizeof(h), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    for (int k = 0; e == hipSuccess && k < hsv::kColClasses; ++k) t_deal_counts[k] = h.cls[k].count;
  }
  return ws.done(e);
}

}  // namespace

extern "C" hipError_t hsv_launch_verify_ws(int variant, const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                           uint64_t sig_stride, const uint8_t *msg, uint64_t msg_stride, uint32_t n,
                                           uint8_t *flags_out, uint32_t *strict_bits, const uint32_t *comb_b,
                                           uint32_t *fault, void *ws, size_t ws_cap, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (variant != 19 && variant != 21)
    return hsv_launch_verify(variant, pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits,
                             comb_b, fault, stream);
  if (!comb_b || !fault) return hipErrorInvalidValue;
  if (variant == 21 && n <= hsv::kPairMax)
    return hsv_launch_small(pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits, comb_b, fault,
                            ws, ws_cap, stream);
  return launch_hp<4, HSV_HP_WAVES, 16>(pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits,
                                        comb_b, fault, stream, nullptr, ws, ws_cap);
}

extern "C" size_t hsv_launch_ws_bytes(int variant, uint32_t n) {
  size_t need = 0;
  if (variant == 21 && n <= hsv::kPairMax)
    need = hsv_small_ws_bytes(n);
  else if (variant == 19 || variant == 21)
    (void)launch_hp<4, HSV_HP_WAVES, 16>(nullptr, 0, nullptr, 0, nullptr, 0, n, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, 0, &need);
  return need;
}

extern "C" hipError_t hsv_launch_verify(int variant, const uint8_t *pk, uint64_t pk_stride,
                                        const uint8_t *sig, uint64_t sig_stride,
                                        const uint8_t *msg, uint64_t msg_stride, uint32_t n,
                                        uint8_t *flags_out, uint32_t *strict_bits,
                                        const uint32_t *comb_b, uint32_t *fault, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (hsv_variant_needs_comb(variant) && !comb_b) return hipErrorInvalidValue;
  if (!fault && variant >= 19) return hipErrorInvalidValue;
  switch (variant) {
    case 19:
      return launch_hp<4, 3, 16>(pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits, comb_b,
                                 fault, stream);
    case 21:
      if (n <= hsv::kPairMax)
        return hsv_launch_small(pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits, comb_b,
                                fault, nullptr, 0, stream);
      return launch_hp<4, HSV_HP_WAVES, 16>(pk, pk_stride, sig, sig_stride, msg, msg_stride, n, flags_out, strict_bits,
                                            comb_b, fault, stream);
    default: return hipErrorInvalidValue;
  }
}

extern "C" hipError_t hsv_launch_verify_tx(int variant, const uint8_t *txs, const uint64_t *offsets,
                                           uint64_t tx_size, uint32_t n, uint8_t *records, uint8_t *flags_out,
                                           uint32_t *strict_bits, const uint32_t *comb_b, uint32_t *fault,
                                           hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if ((variant == 19 || variant == 21) && n > hsv::kPairMax) {
    if (!comb_b || !fault) return hipErrorInvalidValue;
    const TxPrep tx{txs, offsets, tx_size, records};
    return launch_hp<4, HSV_HP_WAVES, 16>(nullptr, 0, nullptr, 0, nullptr, 0, n, flags_out, strict_bits, comb_b,
                                          fault, stream, &tx);
  }
  hipError_t e = hsv_launch_tx_records(txs, offsets, tx_size, n, records, stream);
  if (e != hipSuccess) return e;
  return hsv_launch_verify(variant, records, 128, records + 32, 128, records + 96, 128, n, flags_out, strict_bits,
                           comb_b, fault, stream);
}

namespace {
// How hsv_launch_verify_msgs routes n <= kPairMax items: -1 the small form
// hsv_small.hip picks by n (the default), 0 the two launches of larger batches
// (the parent's behaviour, for A/B runs), 1..4 one small form at every such n.
// A measurement switch, so only libhsv_test.so can move it (hsvi_set_msgs_small
// behind hsv_test_msgs_small): the product library reads no environment
// variable for it (tests/test_capi.py keeps that list closed).
std::atomic<int> g_msgs_small{-1};
// launches so far by form: two-launch, quad, joint, row, pair
std::atomic<uint64_t> g_msgs_forms[1 + hsv::kSmallForms];
}  // namespace

extern "C" int hsvi_set_msgs_small(int mode) {
  if (mode < -1 || mode > hsv::kSmallForms) return -2;
  return g_msgs_small.exchange(mode);
}

extern "C" int hsvi_msgs_form_counts(uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = g_msgs_forms[i].load();
  return 0;
}

// Messages of any length.  At <= kPairMax items one launch of a small form's
// message instantiation, whose prepass wave hashes the whole messages beside
// the point waves; above, the message prepass, then the point
// pass that reads k from the record for fallback items.
extern "C" hipError_t hsv_launch_verify_msgs(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                             uint64_t sig_stride, const uint8_t *msgs, const uint64_t *offsets,
                                             uint64_t msg_len, uint64_t msg_stride, uint32_t n, uint8_t *flags_out,
                                             uint32_t *strict_bits, const uint32_t *comb16, uint32_t *fault,
                                             hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!comb16 || !fault) return hipErrorInvalidValue;
  const int mode = g_msgs_small.load();
  if (mode != 0 && n <= hsv::kPairMax) {
    int id = 0;
    const hipError_t e = hsv_launch_small_msgs(pk, pk_stride, sig, sig_stride, msgs, offsets, msg_len, msg_stride, n,
                                               flags_out, strict_bits, comb16, fault, mode > 0 ? mode : 0, &id, stream);
    g_msgs_forms[id].fetch_add(1);
    return e;
  }
  g_msgs_forms[0].fetch_add(1);
  const MsgPrep mp{msgs, offsets, msg_len, msg_stride};
  return launch_hp<4, HSV_HP_WAVES, 16>(pk, pk_stride, sig, sig_stride, nullptr, 0, n, flags_out, strict_bits, comb16,
                                        fault, stream, nullptr, nullptr, 0, nullptr, &mp);
}

// Variant ids compiled into this library.  The product build carries the
// default (21: variant 19's two-pass kernels above 2^13 items, the pair-lane
// latency form at or below) and 19 itself.  The other ids of earlier rounds
// are measurement history (git history before round 5's cleanup).
static const int kVariantIds[] = {19, 21};

extern "C" int hsvi_variant_list(int *out, int cap) {
  const int n = (int)(sizeof(kVariantIds) / sizeof(kVariantIds[0]));
  for (int i = 0; out && i < n && i < cap; ++i) out[i] = kVariantIds[i];
  return n;
}

extern "C" int hsvi_variant_available(int variant) {
  for (int v : kVariantIds)
    if (v == variant) return 1;
  return 0;
}

extern "C" double hsv_launch_mad_peak(int device_cus) {
  // device-wide waits and a free below: the resident service is paused
  struct Pause {
    Pause() { hsvi_resident_pause(1); }
    ~Pause() { hsvi_resident_pause(0); }
  } pause;
  uint32_t *sink = nullptr;
  if (hipMalloc(&sink, 64) != hipSuccess) return -1.0;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  const int grid = device_cus * 8;
  hipLaunchKernelGGL(hsv::hsv_mad_peak_kernel, dim3(grid), dim3(256), 0, 0, sink, 1u);
  (void)hipDeviceSynchronize();
  (void)hipEventRecord(e0, 0);
  const int reps = 5;
  for (int r = 0; r < reps; ++r)
    hipLaunchKernelGGL(hsv::hsv_mad_peak_kernel, dim3(grid), dim3(256), 0, 0, sink, (uint32_t)r);
  (void)hipEventRecord(e1, 0);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(sink);
  const double macs = (double)reps * grid * 256.0 * hsv::kPeakIters * 16.0;
  return ms > 0.f ? macs / (ms * 1e-3) : -1.0;
}

// The lattice bound of the comb-path prepass (tests): 0 restores the default
// (kLatCombBits); otherwise 128..kLatCombBits.  Returns the previous bound, or
// -1 for an out-of-range value.
extern "C" int hsvi_set_lattice_bits(int bits) {
  if (bits == 0) bits = hsv::kLatCombBits;
  if (bits < 128 || bits > hsv::kLatCombBits) return -1;
  return g_lat_bits.exchange(bits);
}

// Fault injection mode of the calling thread's following launches (kInject*:
// 1 zeroed tables, 2 overwritten canary, 3 flipped table bits, 4 a record
// batch of the fused transaction launch never published; 0 = off).
// Returns the previous mode, or -1 for an unknown one.
extern "C" int hsvi_set_inject(int mode) {
  if (mode < 0 || mode > (int)hsv::kInjectNoPublish) return -1;
  const int prev = (int)t_inject;
  t_inject = (uint32_t)mode;
  return prev;
}
extern "C" int hsvi_inject_mode(void) { return (int)t_inject; }

// Dealing mode of the calling thread's following two-launch point passes: bit 0
// deal by column count (off: index order), bit 1 keep each launch's class
// counts for hsvi_deal_counts (the launch then waits for its stream).  The
// default is 1.  Returns the previous mode, or -1 for an unknown one.
extern "C" int hsvi_set_deal(int mode) {
  if (mode < 0 || mode > 3) return -1;
  const int prev = t_deal;
  t_deal = mode;
  return prev;
}
// Items per column class (hsv_verify_hc.hpp col_class: out[0] needs >= 67
// columns .. out[5] at most 62) of the calling thread's last launch under mode
// bit 1; all zero when that launch ran in index order.
extern "C" int hsvi_deal_counts(uint32_t out[6]) {
  static_assert(hsv::kColClasses == 6, "hook signature");
  for (int i = 0; i < hsv::kColClasses; ++i) out[i] = t_deal_counts[i];
  return 0;
}
// for the launchers of other translation units (hsv_small.hip, hsv_mempool.hip)
extern "C" int hsvi_lattice_bits(void) { return g_lat_bits.load(); }
extern "C" uint32_t hsvi_next_nonce(void) { return next_nonce(); }

namespace {
__global__ void hsv_fault_exchange_kernel(uint32_t *words, uint32_t *out) {
  if (threadIdx.x < 2) out[threadIdx.x] = atomicExch(&words[threadIdx.x], 0u);
}
}  // namespace

extern "C" hipError_t hsv_launch_fault_exchange(uint32_t *words, uint32_t *out, hipStream_t stream) {
  hipLaunchKernelGGL(hsv_fault_exchange_kernel, dim3(1), dim3(64), 0, stream, words, out);
  return hipGetLastError();
}

extern "C" int hsv_variant_needs_comb(int variant) {
  if (variant >= 10 && variant <= 14) return 8;
  if (variant >= 15 && variant <= 22) return 16;
  return 0;
}

#ifdef HSV_PHASE_CLOCKS
extern "C" __attribute__((visibility("default"))) int hsv_phase_clocks_read(uint64_t *dst, size_t words, int clear) {
  const size_t nw = std::min<size_t>(words, (size_t)hsv::kPhaseCap * 8);
  if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(hsv::g_phase_clk), nw * sizeof(uint64_t)) != hipSuccess) return -1;
  if (clear) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(hsv::g_phase_clk)) != hipSuccess) return -1;
    if (hipMemset(p, 0, (size_t)hsv::kPhaseCap * 8 * sizeof(uint64_t)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
