// ---- automatic committee cache behind the drop-in verify_batch ---------------------
// Consensus keys are fixed per epoch (consensus/src/config.rs:39-43), so the
// keys of every QC repeat round after round.  A key missing from the cache
// is counted once per batch it appears in; from its second batch on it is
// queued, and a background thread builds the queued keys' tables on a stream
// of its own, appends them to the cache and publishes a new immutable view.
// A verify call never waits for a build: it takes the committee kernels when
// every key of its batch is in the published view and the generic kernels
// otherwise, with identical flags either way (tests/test_committee.py).
// Capacity kAutoMaxKeys keys; batches larger than that are never counted.
// When the cache is full and batches keep missing it (a new epoch), it is
// dropped and relearnt.  A failed build is a cache miss, never an error.
// HSV_AUTO_COMMITTEE=0 or hsv_set_auto_committee(0) turns it off.
//
// The cache hands the committee kernels (hsv_committee.hip) a device array of
// per-key table pointers, as the explicit committee does
// (hsv_committee_api.cpp), so it grows by appending 64-key table blocks:
// existing tables never move, a build for new keys never copies the old ones,
// and peak table memory is one copy of the cache.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "hsv_committee_host.h"
#include "hsv_keyindex.hpp"

namespace hsvh {
namespace {

constexpr uint32_t kAutoMaxKeys = 8192;      // 3 GiB of tables at most
constexpr uint32_t kBlockKeys = 64;          // tables allocated 64 keys (24 MiB) at a time
constexpr size_t kCommitteeTryMax = 4096;    // hsv_verify / verify_strict batches that try the cache
constexpr size_t kLearnStrictMax = 16;       // ... and that teach it their keys (votes, single verifies)
constexpr uint32_t kResetAfterMisses = 256;  // missing batches against a full cache before a relearn
constexpr int kMaxBuildFailures = 3;         // then the cache stays off until hsv_set_auto_committee(1)

struct AutoStore {  // append-only device storage, freed with the last view using it
  int device = 0;
  uint8_t *d_pks = nullptr;
  uint8_t *d_kflags = nullptr;
  uint32_t **d_tabptr = nullptr;
  uint32_t *d_tmp = nullptr;
  hipStream_t stream = nullptr;  // builds only
  std::vector<uint32_t *> blocks;
  // host copy of the encodings (kAutoMaxKeys * 32 B, allocated once: a view's
  // pointer into it stays valid as later builds append)
  std::unique_ptr<uint8_t[]> h_pks{new uint8_t[(size_t)kAutoMaxKeys * 32]};
  ~AutoStore() {
    ResidentPause pause;  // hipFree waits for every grid on the device
    DeviceGuard guard(device);
    if (stream) (void)hipStreamDestroy(stream);
    for (uint32_t *b : blocks) (void)hipFree(b);
    if (d_pks) (void)hipFree(d_pks);
    if (d_kflags) (void)hipFree(d_kflags);
    if (d_tabptr) (void)hipFree(d_tabptr);
    if (d_tmp) (void)hipFree(d_tmp);
  }
};

struct AutoView {  // immutable snapshot: keys [0, n) of `store` are built
  std::shared_ptr<AutoStore> store;
  CommitteeDev dev;
  KeyIndex index;
};

struct AutoCommittee {
  std::mutex mu;  // everything below; `view` is also read lock-free (atomic_load)
  std::shared_ptr<const AutoView> view;
  std::unordered_map<Key32, uint32_t, KeyHash> seen;  // uncached key -> batches it appeared in
  std::vector<Key32> pending;
  std::unordered_set<Key32, KeyHash> pending_set;
  bool building = false;
  uint64_t generation = 0;  // bumped by a reset; a build of an older generation is discarded
  // batches that missed a full cache in a row; written under mu on a miss,
  // reset without the lock on a hit (the QC hot path takes no lock)
  std::atomic<uint32_t> miss_streak{0};
  int failures = 0;
  std::thread worker;
  std::condition_variable idle;
  std::atomic<int> enabled{-1};  // -1: read HSV_AUTO_COMMITTEE on first use
  std::atomic<uint64_t> builds{0};
  std::atomic<uint64_t> faults{0};  // cached-path launches whose self-check failed
  ~AutoCommittee() {
    std::unique_lock<std::mutex> lk(mu);
    idle.wait(lk, [&] { return !building; });
    lk.unlock();
    if (worker.joinable()) worker.join();
  }
};

AutoCommittee &AC() {
  static AutoCommittee a;
  return a;
}

bool auto_enabled() {
  AutoCommittee &a = AC();
  int e = a.enabled.load();
  if (e < 0) {
    const char *v = std::getenv("HSV_AUTO_COMMITTEE");
    e = (v && v[0] == '0') ? 0 : 1;
    a.enabled.store(e);
  }
  return e == 1;
}

std::shared_ptr<const AutoView> current_view() { return std::atomic_load(&AC().view); }

// Build tables for `keys` on top of `base` (nullptr: a fresh store on
// `device`).  Runs without the cache lock.
int build_view(const std::shared_ptr<const AutoView> &base, int device, const std::vector<Key32> &keys,
               std::shared_ptr<const AutoView> &out) {
  DeviceGuard guard(device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  std::shared_ptr<AutoStore> store = base ? base->store : std::make_shared<AutoStore>();
  const uint32_t n0 = base ? base->dev.n : 0;
  const uint32_t m = std::min<uint32_t>((uint32_t)keys.size(), kAutoMaxKeys - n0);
  hipError_t e = hipSuccess;
  if (!base) {
    store->device = device;
    e = hipMalloc(&store->d_pks, (size_t)kAutoMaxKeys * 32);
    if (e == hipSuccess) e = hipMalloc(&store->d_kflags, kAutoMaxKeys);
    if (e == hipSuccess) e = hipMalloc(&store->d_tabptr, (size_t)kAutoMaxKeys * sizeof(uint32_t *));
    if (e == hipSuccess) e = hipMalloc(&store->d_tmp, hsv_comb_tmp_bytes(kBlockKeys));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&store->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail("allocating the committee cache", e);
  }
  const uint64_t words = hsv_comb_table_bytes() / 4;
  while ((uint64_t)store->blocks.size() * kBlockKeys < (uint64_t)n0 + m) {
    uint32_t *blk = nullptr;
    e = hipMalloc(&blk, (size_t)kBlockKeys * hsv_comb_table_bytes());
    if (e != hipSuccess) return hip_fail("allocating committee tables", e);
    store->blocks.push_back(blk);
  }
  std::vector<uint8_t> encs((size_t)m * 32);
  std::vector<uint32_t *> ptrs(m);
  for (uint32_t i = 0; i < m; ++i) {
    std::memcpy(encs.data() + (size_t)i * 32, keys[i].data(), 32);
    const uint32_t slot = n0 + i;
    ptrs[i] = store->blocks[slot / kBlockKeys] + (uint64_t)(slot % kBlockKeys) * words;
  }
  std::memcpy(store->h_pks.get() + (size_t)n0 * 32, encs.data(), encs.size());  // slots no published view reads yet
  e = hipMemcpyAsync(store->d_pks + (size_t)n0 * 32, encs.data(), encs.size(), hipMemcpyHostToDevice, store->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(store->d_tabptr + n0, ptrs.data(), m * sizeof(uint32_t *), hipMemcpyHostToDevice, store->stream);
  if (e == hipSuccess)
    e = build_tables(store->d_pks + (size_t)n0 * 32, m, ptrs.data(), store->d_kflags + n0, store->d_tmp, kBlockKeys,
                     store->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(store->stream);
  if (e != hipSuccess) return hip_fail("building committee tables", e);
  auto v = std::make_shared<AutoView>();
  v->store = store;
  v->dev.device = store->device;
  v->dev.n = n0 + m;
  v->dev.h_pks = store->h_pks.get();
  v->dev.d_pks = store->d_pks;
  v->dev.d_kflags = store->d_kflags;
  v->dev.d_tabptr = store->d_tabptr;
  if (base) v->index = base->index;
  for (uint32_t i = 0; i < m; ++i) v->index.emplace(keys[i], n0 + i);
  out = v;
  return HSV_OK;
}

void worker_main() {
  AutoCommittee &a = AC();
  std::unique_lock<std::mutex> lk(a.mu);
  for (;;) {
    if (a.pending.empty() || a.enabled.load() != 1) {
      a.pending.clear();
      a.pending_set.clear();
      a.building = false;
      a.idle.notify_all();
      return;
    }
    std::vector<Key32> keys;
    keys.swap(a.pending);
    const uint64_t gen = a.generation;
    std::shared_ptr<const AutoView> base = a.view;
    const int device = base ? base->dev.device : home_device();
    lk.unlock();
    std::shared_ptr<const AutoView> built;
    const int rc = build_view(base, device, keys, built);
    lk.lock();
    for (const Key32 &k : keys) {
      a.pending_set.erase(k);
      a.seen.erase(k);
    }
    if (rc == HSV_OK && gen == a.generation) {
      std::atomic_store(&a.view, built);
      a.builds.fetch_add(1);
    } else if (rc != HSV_OK && ++a.failures >= kMaxBuildFailures) {
      a.enabled.store(0);  // verification goes on through the generic kernels
    }
  }
}

// Drop the published view and everything learnt so far (a.mu held): the next
// batches relearn from scratch, and a build in flight is discarded when it
// ends (its generation is older).
void drop_view_locked(AutoCommittee &a) {
  std::atomic_store(&a.view, std::shared_ptr<const AutoView>());
  a.seen.clear();
  a.pending.clear();
  a.pending_set.clear();
  a.miss_streak = 0;
  ++a.generation;
}

// The view to verify this batch with (every key in it; idx receives the
// member indices), or nullptr: the generic path.  Records misses.
std::shared_ptr<const AutoView> auto_lookup(const uint8_t *pk, size_t pk_stride, size_t n, uint32_t *idx,
                                            bool count_misses) {
  std::shared_ptr<const AutoView> v = current_view();
  std::vector<Key32> missing;
  for (size_t i = 0; i < n; ++i) {
    if (v) {
      const int64_t m = v->index.find(pk + i * pk_stride);
      if (m >= 0) {
        idx[i] = (uint32_t)m;
        continue;
      }
    }
    if (!count_misses) return nullptr;
    missing.push_back(key_of(pk + i * pk_stride));
  }
  AutoCommittee &a = AC();
  if (missing.empty()) {
    if (v && v->dev.device != home_device()) return nullptr;  // cache lives on another device
    if (a.miss_streak.load(std::memory_order_relaxed)) a.miss_streak.store(0, std::memory_order_relaxed);
    return v;
  }
  if (n > kAutoMaxKeys) return nullptr;  // not a committee-sized batch
  std::sort(missing.begin(), missing.end());
  missing.erase(std::unique(missing.begin(), missing.end()), missing.end());  // once per batch
  std::unique_lock<std::mutex> lk(a.mu);
  const uint32_t cached = v ? v->dev.n : 0;
  if (cached + a.pending_set.size() >= kAutoMaxKeys && a.miss_streak.fetch_add(1) + 1 >= kResetAfterMisses) {
    // a full cache that keeps missing: a new epoch, relearn from scratch
    drop_view_locked(a);
    return nullptr;
  }
  for (const Key32 &k : missing) {
    if (a.pending_set.count(k)) continue;
    if (++a.seen[k] >= 2 && cached + a.pending_set.size() < kAutoMaxKeys) {
      a.pending.push_back(k);
      a.pending_set.insert(k);
    }
  }
  if (a.seen.size() > 4 * (size_t)kAutoMaxKeys) a.seen.clear();
  if (!a.pending.empty() && !a.building && a.enabled.load() == 1) {
    a.building = true;
    if (a.worker.joinable()) a.worker.join();  // the previous build thread has finished
    a.worker = std::thread(worker_main);
  }
  return nullptr;
}

// The cached path's self-check failed: its tables (or the memory under them)
// are no longer trusted.  Drop the view the failing call used -- unless a
// newer one was published meanwhile -- and relearn from scratch; the call
// itself is answered by the generic kernels.  Counted (hsv_auto_committee_faults).
void auto_invalidate(const std::shared_ptr<const AutoView> &bad) {
  AutoCommittee &a = AC();
  a.faults.fetch_add(1);
  std::lock_guard<std::mutex> lk(a.mu);
  if (std::atomic_load(&a.view) != bad) return;
  drop_view_locked(a);
}

// Run a batch on the cached tables.  HSV_OK, 1 (take the generic path:
// the self-check failed, the view is dropped), or another error.
int auto_run(const std::shared_ptr<const AutoView> &v, const uint32_t *idx, const uint8_t *sig, size_t sig_stride,
             const uint8_t *msg, size_t msg_stride, size_t n, uint8_t *flags_out) {
  const int rc = committee_run(v->dev, idx, sig, sig_stride, msg, msg_stride, n, flags_out);
  if (rc == HSV_ERR_DEVICE_FAULT) {
    auto_invalidate(v);
    return 1;
  }
  return rc;
}

void auto_reset(bool enable) {
  AutoCommittee &a = AC();
  std::unique_lock<std::mutex> lk(a.mu);
  a.enabled.store(enable ? 1 : 0);
  if (!enable) {
    a.pending.clear();
    a.idle.wait(lk, [&] { return !a.building; });
    drop_view_locked(a);
  }
  a.failures = 0;
}

}  // namespace

int auto_committee_try(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg, size_t msg_stride, size_t n,
                       uint8_t *flags_out) {
  // only the latency range (a vote, a TC); large batches of fresh keys would
  // pay a hash lookup per item for nothing.  Calls of a few signatures --
  // Vote::verify on every incoming vote (consensus/src/core.rs:240), the
  // proposer's Block::verify -- count their keys as sightings too, so a
  // committee whose votes arrive before its first QCs is learnt from them;
  // larger strict batches only read the cache (their keys need not recur).
  if (n > kCommitteeTryMax || !auto_enabled()) return 1;
  thread_local std::vector<uint32_t> idx;  // per-call scratch kept by the thread
  idx.resize(n);
  std::shared_ptr<const AutoView> v = auto_lookup(pk, 32, n, idx.data(), n <= kLearnStrictMax);
  call_mark(HSV_MARK_LOOKUP);
  if (!v || v->dev.device != home_device()) return 1;
  return auto_run(v, idx.data(), sig, 64, msg, msg_stride, n, flags_out);
}

int auto_committee_corrupt_tables() {
  std::shared_ptr<const AutoView> v = current_view();
  if (!v || v->store->blocks.empty()) return 0;
  DeviceGuard guard(v->dev.device);
  for (uint32_t *b : v->store->blocks) {
    const hipError_t e = hipMemset(b, 0, (size_t)kBlockKeys * hsv_comb_table_bytes());
    if (e != hipSuccess) return hip_fail("hipMemset", e);
  }
  return (int)v->dev.n;
}

void auto_committee_shutdown() {
  resident_stop();
  auto_reset(false);
  AutoCommittee &a = AC();
  std::lock_guard<std::mutex> lk(a.mu);
  a.enabled.store(-1);  // re-read the environment on next use
}

}  // namespace hsvh

using namespace hsvh;

extern "C" {

int hsv_verify_batch_packed(const uint8_t digest[32], const uint8_t *votes, size_t n) {
  CallScope call;
  if (n == 0) return 1;
  if (!digest || !votes) return fail(HSV_ERR_INVALID_ARG, "null argument");
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  thread_local std::vector<uint8_t> flags;  // per-call scratch kept by the thread
  thread_local std::vector<uint32_t> idx;
  flags.resize(n);
  if (n >= 2 && auto_enabled()) {
    idx.resize(n);
    std::shared_ptr<const AutoView> v = auto_lookup(votes, 96, n, idx.data(), true);
    call_mark(HSV_MARK_LOOKUP);
    if (v) {
      rc = auto_run(v, idx.data(), votes + 32, 96, digest, 0, n, flags.data());
      if (rc == HSV_OK) return batch_verdict(flags.data(), n);
      // the self-check failed (the cache is dropped) or another infrastructure
      // error on the cached path: the generic path answers
    }
  }
  rc = run_host(votes, 96, votes + 32, 96, digest, 0, n, flags.data());
  return rc != HSV_OK ? rc : batch_verdict(flags.data(), n);
}

int hsv_set_auto_committee(int enable) {
  auto_reset(enable != 0);
  return HSV_OK;
}

size_t hsv_auto_committee_size(void) {
  std::shared_ptr<const AutoView> v = current_view();
  return v ? v->dev.n : 0;
}

uint64_t hsv_auto_committee_faults(void) { return AC().faults.load(); }

int hsv_auto_committee_wait(int timeout_ms) {
  AutoCommittee &a = AC();
  std::unique_lock<std::mutex> lk(a.mu);
  const bool done = a.idle.wait_for(lk, std::chrono::milliseconds(timeout_ms < 0 ? 0 : timeout_ms),
                                    [&] { return !a.building; });
  return done ? 1 : 0;
}

}  // extern "C"
