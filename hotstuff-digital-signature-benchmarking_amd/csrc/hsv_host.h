// Host-side state shared by the C-ABI translation units (hsv_capi.cpp,
// hsv_committee_api.cpp, hsv_resident.cpp, hsv_auto_committee.cpp, hsv_tx.cpp,
// hsv_msgs_api.cpp, hsv_signer_api.cpp, hsv_numa.cpp) and hsv_test_hooks.cpp.
// Not part of the public ABI.  What only the three committee units share is in
// hsv_committee_host.h.
//
// The call layer every entry-point family is built from:
//   * BatchSpan (hsv_batch.hpp): the chunk walk of a ragged or fixed-size host
//     batch, a chunk's geometry and the length check;
//   * StagedBlock: one pool block with aligned regions and the self-check
//     words, drained by finish() -- the staged host forms of the message
//     calls, which are one walk (staged_msgs_host), as those of the
//     transaction calls are (staged_tx_host);
//   * DeviceCall: device, guard, B table and fault words of a stream-ordered
//     device-form call.
//
// Device model (include/hsv.h, hsv_init):
//   * one DevCtx per visible GPU, created lazily;
//   * each DevCtx owns a small pool of Slots (stream + pinned staging +
//     device buffer + mutex), so concurrent host-buffer calls -- several
//     tokio workers verifying QCs and votes at once -- run side by side
//     instead of queueing on one staging buffer;
//   * the fixed-base B tables (narrow comb for the committee kernels, wide
//     comb for the generic kernels) are per device and shared by its slots.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "hsv.h"
#include "hsv_batch.hpp"
#include "hsv_internal.h"

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

namespace hsvh {

// ---- errors ----------------------------------------------------------------
int fail(int code, const std::string &msg);
int hip_fail(const char *where, hipError_t e);
const std::string &last_error();

// ---- host timeline of a call (hsv_host_call_marks) ---------------------------
// Every public entry point that verifies opens a CallScope; the path below it
// stamps the HSV_MARK_* points it passes (ms from the entry), or, in a
// pipelined call, four marks per chunk.
class CallScope {
 public:
  CallScope();
  ~CallScope();
  CallScope(const CallScope &) = delete;
  CallScope &operator=(const CallScope &) = delete;
};
void call_mark(int which);
void call_chunk_mark();

// ---- sizes -------------------------------------------------------------------
constexpr size_t kAlign = 256;
constexpr size_t kChunk = size_t(1) << 22;        // items per verification launch
constexpr size_t kShardMin = size_t(1) << 16;     // shard host batches across devices at or above this
constexpr size_t kZeroCopyMax = size_t(1) << 12;  // small batches read straight from pinned memory
inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// Bytes of transactions or messages a host form stages per launch (one larger
// item: alone).  Tests lower it through hsv_test_stage_bytes (libhsv_test.so).
constexpr size_t kStageBytes = size_t(1) << 29;
inline std::atomic<size_t> g_stage_bytes{kStageBytes};

// The two copies into pinned staging.
//   * stage_stream: streaming stores, so the bytes sit in DRAM and not in the
//     writing core's cache: the GPU's reads of a zero-copy launch then need no
//     snoop of a remote core's cache, whose cost grows with the distance from
//     that core to the PCIe root (after a host load had moved the calling
//     thread, the C3 QC read 0.0634 against 0.0543 ms, profiles/r05q_idle.txt).
//     dst 16-byte aligned; the tail of n that is not a multiple of 16 is a
//     plain copy.  stage_fence() orders the streaming stores before the launch
//     that reads them.
//   * stage_copy (hsv_capi.cpp, declared below): a cached memcpy below 64 KiB,
//     non-temporal stores from there on, split over the pack pool above 1 MiB.
// Only committee_run's key_idx copy is a stage_stream.  Its signature and
// message copies, run_on_device's pack and the transaction walk are
// stage_copy: until the two had names of their own they were overloads of one,
// told apart by the source pointer's type, and those sites' const uint8_t *
// sources always took this one.
inline void stage_stream(uint8_t *dst, const void *src, size_t n) {
  const uint8_t *s = static_cast<const uint8_t *>(src);
#if defined(__SSE2__)
  size_t i = 0;
  for (; i + 16 <= n; i += 16)
    _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i), _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i)));
  if (i < n) std::memcpy(dst + i, s + i, n - i);
#else
  std::memcpy(dst, s, n);
#endif
}
inline void stage_fence() {
#if defined(__SSE2__)
  _mm_sfence();
#endif
}

// ---- device contexts ---------------------------------------------------------
struct Slot {
  std::mutex mu;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // second compute stream of large host batches
  hipStream_t copy = nullptr;     // host-to-device stream of large host batches
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // staged[2], unused, joined[2] (run_pipelined)
  uint8_t *d_ws[3] = {nullptr, nullptr, nullptr};  // launch workspaces of the compute streams (run_pipelined)
  size_t ws_cap = 0;
  uint8_t *d_buf = nullptr;
  size_t d_cap = 0;
  uint8_t *h_buf = nullptr;
  uint8_t *h_buf_dev = nullptr;  // h_buf's device address (zero-copy launches), looked up once
  size_t h_cap = 0;
  // flag bytes, self-check words and completion markers of the committee
  // latency form (committee_run), in COHERENT pinned memory: the host reads
  // them while the kernel may still be running (marker sync), so they must not
  // sit in the GPU's L2 -- correctness does not rest on the release fence's
  // write-back of non-coherent lines (round-4 advice)
  uint8_t *h_sync = nullptr;
  uint8_t *h_sync_dev = nullptr;
  size_t h_sync_cap = 0;
  size_t pipe_warm_n = 0;  // items of the last completed pipelined call (HSV_PIPE_NOCOPY)
};

struct DevCtx {
  int device = 0;
  int cus = 0;
  std::mutex table_mu;             // guards the two B tables and d_fault below
  uint32_t *d_btable = nullptr;    // narrow comb of B (committee kernels)
  uint32_t *d_btable16 = nullptr;  // wide comb of B (generic kernels)
  uint32_t *d_fault = nullptr;     // self-check words of the device-resident calls (hsv_device_faults);
                                   // words kFaultOutWord.. receive the read-and-clear exchange
  std::mutex fault_mu;             // one read-and-clear of d_fault at a time
  std::vector<std::unique_ptr<Slot>> slots;
  std::atomic<unsigned> rr{0};
  std::mutex side_mu;                    // guards the side-stream pool
  std::vector<hipStream_t> side_free;    // idle second streams of multi-chunk device-API batches
  std::vector<hipStream_t> side_all;     // every side stream created (hsv_shutdown)
  std::atomic<unsigned> tx_count_rr{0};  // next list-length slot of d_fault (committee_tx_counts)
  std::atomic<unsigned> msg_count_rr{0};  // the same of the message calls (committee_msgs_counts)
};

// Makes `device` current for the calling thread and restores the previous
// current device on destruction (the library never leaves the caller's
// thread on another device).
class DeviceGuard {
 public:
  explicit DeviceGuard(int device);
  ~DeviceGuard();
  hipError_t status() const { return status_; }

 private:
  int prev_ = -1;
  hipError_t status_ = hipSuccess;
};

int ensure_init();  // HSV_OK or HSV_ERR_NO_DEVICE
int device_count_inited();
DevCtx &ctx(int device);
int variant();

// Device a host-buffer call of n items that is not sharded runs on: the
// bound device (hsv_init(d) / HSV_DEVICE), else the calling thread's
// current HIP device.
int home_device();
// Number of shards a host batch of n items is split into (1 = no sharding)
// and the device shard s runs on.
int shard_count(size_t n);
int shard_device(int shard, int nshards);

// Lock a free slot of `c` (try every slot, then wait on one).
class SlotLease {
 public:
  explicit SlotLease(DevCtx &c);
  Slot &slot() { return *s_; }

 private:
  Slot *s_;
  std::unique_lock<std::mutex> lk_;
};

// Stream and buffers of a slot (current device must be c.device).
int slot_prepare(Slot &s, size_t dev_bytes, size_t host_bytes);
int slot_stream2(Slot &s);
int slot_pipeline(Slot &s);  // stream2, the copy stream, the events of run_pipelined
// the slot's coherent sync region (Slot::h_sync) of at least `bytes`
int slot_sync_region(Slot &s, size_t bytes);

// Device self-check words (hsv_pointpass.hpp report_faults): two words per
// launch, zeroed before it; non-zero after it -> HSV_ERR_DEVICE_FAULT.
constexpr size_t kFaultBytes = 8;
int check_faults(const uint8_t *words, const char *where);
// The per-device words of the stream-ordered device API (current device
// must be c.device); allocated and zeroed on first use.
int device_fault_words(DevCtx &c, uint32_t **out);
constexpr size_t kFaultOutWord = 4;  // d_fault[4..5]: output of hsv_launch_fault_exchange
// d_fault bytes [64, 256): kTxCountSlots slots of four 64-bit words, the list
// lengths of the committee transaction calls (committee_tx_counts); a call
// takes the next slot in turn
constexpr size_t kTxCountSlots = 6, kTxCountOff = 64, kTxCountBytes = 32;
// d_fault bytes [256, 448): the same for the committee message calls
// (committee_msgs_counts), slots of their own
constexpr size_t kMsgCountOff = 256;
constexpr size_t kDeviceFaultBytes = 512;  // the whole block
// The words a device-API call reports into: the caller's d_fault (zeroed on
// `stream` here), or the per-device words when d_fault is NULL.
int call_fault_words(DevCtx &c, uint32_t *d_fault, hipStream_t stream, uint32_t **out);

// One stream-ordered block from the library pool for one launch of a staged
// host form: the self-check words, then the regions add() lays out at kAlign
// (and kAlign of slack after the last).  A step after a failed one is skipped;
// finish() reports the first failure, and always frees the block and drains
// the stream, so nothing of the call stays in flight.
class StagedBlock {
 public:
  explicit StagedBlock(hipStream_t stream) : st_(stream) {}
  size_t add(size_t bytes) {  // offset of a new region
    const size_t off = size_;
    size_ += round_up(bytes, kAlign);
    return off;
  }
  // Allocates the block; zeroes the self-check words and the first `zeroed`
  // bytes of the first region.  HSV_OK, or the error `what` names.
  int alloc(const char *what, size_t zeroed = 0);
  uint8_t *at(size_t off) const { return d_ + off; }
  uint32_t *fault() const { return reinterpret_cast<uint32_t *>(d_); }
  bool ok() const { return e_ == hipSuccess; }
  void step(hipError_t e) {
    if (ok()) e_ = e;
  }
  void in(size_t off, const void *src, size_t bytes) {
    if (ok() && bytes) e_ = hipMemcpyAsync(d_ + off, src, bytes, hipMemcpyHostToDevice, st_);
  }
  void out(void *dst, size_t off, size_t bytes) {
    if (ok() && bytes) e_ = hipMemcpyAsync(dst, d_ + off, bytes, hipMemcpyDeviceToHost, st_);
  }
  // Self-check words out, free, drain: HSV_OK, the first failed step's error,
  // or HSV_ERR_DEVICE_FAULT (check_faults).
  int finish(const char *where);

 private:
  hipStream_t st_;
  uint8_t *d_ = nullptr;
  size_t size_ = kAlign;  // the self-check words' region
  hipError_t e_ = hipSuccess;
};

// A side stream of device c for one call (current device must be c.device),
// returned to the pool when the lease ends: concurrent device-API calls never
// share one, so a call's join event only waits for its own chunks.
class SideStreamLease {
 public:
  explicit SideStreamLease(DevCtx &c);
  ~SideStreamLease();
  hipStream_t stream() const { return s_; }

 private:
  DevCtx &c_;
  hipStream_t s_ = nullptr;
};

// B tables of device c (current device must be c.device).
int ensure_btable(DevCtx &c);
int ensure_btable16(DevCtx &c);
int comb_table_for(DevCtx &c, int variant, const uint32_t **out);

// memcpy into pinned staging (cached below 64 KiB, see stage_stream above);
// large copies split over the pack pool of the current device (its helpers run
// on the GPU's NUMA node)
void stage_copy(uint8_t *dst, const uint8_t *src, size_t bytes);

// ---- host placement (hsv_numa.cpp) -------------------------------------------
struct HostPlace {
  int node = -1;          // NUMA node of the GPU's PCIe function (-1: unknown / single node)
  std::vector<int> cpus;  // that node's CPUs the process may use (empty: threads stay unpinned)
  int pack_threads = 0;   // helpers of the device's pack pool
};
bool parse_cpulist(const std::string &text, std::vector<int> &out);
std::vector<int> current_affinity();
bool pin_current_thread(const std::vector<int> &cpus);
int default_pack_threads();
// For PCI functions `bdfs` under the sysfs tree `root`: each one's node, the
// node's CPUs within `allowed` (sorted), and the pack-pool size (the node's
// CPUs split among its GPUs, at most pack_default)
std::vector<HostPlace> plan_host_places(const std::string &root, const std::vector<std::string> &bdfs,
                                        const std::vector<int> &allowed, int pack_default);
// The placement of a visible device (sysfs under /sys, the process affinity
// at first use); a device without NUMA information gets an unpinned place.
const HostPlace &device_place(int device);

// Run fn(shard, device) for shards [0, k) of a host batch, each on the
// persistent shard worker of its index, pinned to the NUMA node of its
// device; returns HSV_OK or the first shard's error.  The caller's fault
// injection mode (tests) reaches the workers.
int run_sharded(int k, const std::function<int(int shard, int device)> &fn);

// Device owning a device pointer (hipPointerGetAttributes); -1 if unknown.
int pointer_device(const void *p);

// What every stream-ordered device-form call does once its arguments have
// passed their checks: ensure_init, the device it runs on, the stream's
// device checked against it, that device made current for the object's
// lifetime, the B table asked for, and the fault words (call_fault_words).
// Pointer mode (owner == NULL): the device of d_ptr, else the current one.
// Handle mode: owner_device, which d_ptr must not contradict (`owner` names
// the handle in the error text).
class DeviceCall {
 public:
  // ensure_btable, ensure_btable16, comb_table_for(variant()); kBoth: the
  // narrow table in `comb` and the wide one in `comb16`; kNone: no table (the
  // signer census does no curve arithmetic)
  enum Table { kNarrow, kWide, kVariant, kBoth, kNone };
  int begin(const void *d_ptr, void *stream, uint32_t *d_fault, Table table, const char *owner = nullptr,
            int owner_device = -1);
  DevCtx *c = nullptr;
  hipStream_t stream = nullptr;
  int v = 0;                       // variant() (kVariant only)
  const uint32_t *comb = nullptr;  // the table asked for
  const uint32_t *comb16 = nullptr;  // kBoth: the wide table
  uint32_t *fault = nullptr;

 private:
  std::optional<DeviceGuard> guard_;
};

// ---- hooks shared with hsv_test_hooks.cpp (exported by libhsv_test.so only) ----
int auto_committee_corrupt_tables();  // zero the cached tables of the automatic committee

// ---- the automatic committee cache (hsv_auto_committee.cpp) -------------------
// Strict verification of small batches whose keys are all cached: HSV_OK
// when done, 1 when the caller should take the generic path, < 0 on error.
int auto_committee_try(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg, size_t msg_stride, size_t n,
                       uint8_t *flags_out);
void auto_committee_shutdown();
// resident latency service (on by default, hsv_resident.cpp)
// A scope in which its kernel does not run: stopped at construction, and no
// request or relaunch until destruction (small calls launch meanwhile).  Held
// around every hipFree / hipHostFree of the library -- they wait for every
// grid on the device -- and around device-wide waits.
class ResidentPause {
 public:
  ResidentPause();
  ~ResidentPause();
  ResidentPause(const ResidentPause &) = delete;
  ResidentPause &operator=(const ResidentPause &) = delete;
};
void resident_quiesce();  // stop its kernel now (the next request relaunches it)
void resident_counts(uint64_t *posted, uint64_t *answered);
int resident_post_bad(uint32_t m);  // test hook: a request the kernel must refuse
int resident_set_mode(int on);      // hsv_set_resident_service
// test hook (hsv_test_committee_tx_counts): hits, misses and fallback items of
// the calling thread's last hsv_committee_verify_transactions* call
int committee_tx_counts(uint64_t out[3]);
// the same of its last hsv_committee_verify_msgs* call (hsv_test_committee_msgs_counts)
int committee_msgs_counts(uint64_t out[3]);

// The generic host-buffer path (hsv_capi.cpp): records at the given strides.
int run_host(const uint8_t *pk, size_t pk_stride, const uint8_t *sig, size_t sig_stride, const uint8_t *msg,
             size_t msg_stride, size_t n, uint8_t *flags_out);
int batch_verdict(const uint8_t *flags, size_t n);
// The length check of the transaction host forms (hsv_tx.cpp): HSV_OK, or
// HSV_ERR_INVALID_ARG naming the first transaction shorter than 96 bytes.
int tx_lengths_ok(const uint64_t *offsets, size_t tx_size, size_t n);

// measurement hook (hsv_test_batch_stages, hsv_batch_api.cpp): the stages of
// the generic serialized-batch device form between device events
int batch_stage_times(const uint8_t *d_bufs, const uint64_t *d_offsets, size_t n_batches, size_t tx_cap,
                      hsv_batch_result *d_results, float ms_out[4]);

// measurement hook (hsv_test_seal_stages, hsv_seal_api.cpp): the stages of
// hsv_seal_transactions_device between device events
int seal_stage_times(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n, const uint8_t *d_flags,
                     uint64_t batch_size, int flush, uint8_t *d_out, size_t out_cap, uint64_t *d_batch_offsets,
                     size_t batches_cap, uint8_t *d_digests, hsv_seal_summary *d_summary, float ms_out[4]);

// ---- the staged host forms and the argument checks of the generic calls and
// ---- their committee twins (hsv_tx.cpp, hsv_msgs_api.cpp) ----------------------
// A step run once on the slot's stream after slot_prepare (the committee's
// counts_begin), or none.
using StagedBegin = std::function<int(hipStream_t)>;

// Transactions [lo, hi) of the caller's arrays through a slot of device c
// (current, its tables ensured by the caller), chunk by chunk: at most kChunk
// items and g_stage_bytes bytes per launch.  Per chunk one H2D copy, the
// memset of flags and self-check words, `launch` on the chunk in HBM (d_rec:
// rec_bytes per item, 128 for the generic kernels' records, 0 = no region),
// the D2H, the drain, check_faults under `where`, the copy out.
using TxLaunch = std::function<int(const uint8_t *d_txs, const uint64_t *d_offsets, size_t m, uint8_t *d_rec,
                                   uint8_t *d_flags, uint32_t *d_fault, hipStream_t stream)>;
int staged_tx_host(DevCtx &c, const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t lo, size_t hi,
                   uint8_t *flags_out, size_t rec_bytes, const StagedBegin &begin, const TxLaunch &launch,
                   const char *where);
// "no output", and the length check of a fixed size, of the two
// *_verify_transactions_device calls
int tx_device_args_ok(const uint64_t *d_offsets, size_t tx_size, const uint8_t *d_flags,
                      const uint32_t *d_strict_bits);

// n whole messages through a slot of device c and one StagedBlock per launch
// (flags | column | sig | offsets rebased to the chunk | message bytes): at
// most kChunk items and g_stage_bytes message bytes per launch.  The column
// says who signed each item: the 32 pk bytes of the pk-addressed calls, or the
// 4-byte member index of hsv_committee_verify_msgs_indexed; `launch` gets its
// device copy as d_col.  `tables` ensures the B tables `launch` reads (current
// device c.device); alloc_what and finish_where are the caller's texts for
// hsv_last_error.
struct StagedColumn {
  const uint8_t *src;
  size_t item_bytes;  // 32 (pk) or 4 (member index)
};
using MsgsLaunch = std::function<hipError_t(const uint8_t *d_col, const uint8_t *d_sig, const uint8_t *d_msgs,
                                            const uint64_t *d_offsets, size_t m, uint8_t *d_flags, uint32_t *d_fault,
                                            hipStream_t stream)>;
int staged_msgs_host(DevCtx &c, const std::function<int()> &tables, const StagedBegin &begin,
                     const MsgsLaunch &launch, const char *alloc_what, const char *finish_where,
                     const StagedColumn &col, const uint8_t *sig, const uint8_t *msgs, const uint64_t *offsets,
                     size_t msg_len, size_t msg_stride, size_t n, uint8_t *flags_out);
// the checks of the two *_verify_msgs host calls after their null test ...
int msgs_host_args_ok(const uint8_t *msgs, const uint64_t *offsets, size_t msg_len, size_t msg_stride, size_t n);
// ... and of the two device calls from "null d_msgs" on
int msgs_device_args_ok(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig, size_t sig_stride,
                        const uint8_t *d_msgs, const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                        const uint8_t *d_flags, const uint32_t *d_strict_bits);

}  // namespace hsvh
