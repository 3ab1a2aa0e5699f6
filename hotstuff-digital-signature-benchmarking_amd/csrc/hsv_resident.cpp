// ---- resident latency service (on by default; HSV_QC_RESIDENT=0 turns it off) ------
// One block of hsv_comb_resident_kernel stays on a CU of the home device and
// answers requests of at most hsv_comb_resident_votes() votes posted in
// coherent pinned memory (QcResidentReq): 2.2 us round trip for a block of its
// shape against 5.8 us for a launch with marker sync
// (profiles/r05a_aql_latency.txt), so one verify_strict of a cached key costs
// 0.034 ms instead of 0.039 ms launched (0.037 ms for the dalek port on one
// host core).  It holds that one CU while it runs.  The kernel leaves on the
// stop word -- hsv_shutdown, hsv_set_resident_service(0), an atexit handler,
// and every ResidentPause: the library pauses the service around each of its
// own hipFree / hipHostFree (on ROCm they wait for every grid on the device)
// and around its device-wide waits -- or after the idle time
// (HSV_QC_RESIDENT_IDLE_MS, default 50 ms) without a request; the next request
// relaunches it.  No launch pauses the service: once its block has run
// (hsvi_resident_started), the persistent point pass sizes its grid to leave
// one CU out, so each of its blocks finds a place beside the resident one.
// A request unanswered within kResidentWait, or a relaunch that does not
// start, takes the call to the launch path and keeps the service off for a
// backoff, so the service can cost latency but never a verdict.  An
// application that synchronises the whole device (hipDeviceSynchronize,
// torch.cuda.synchronize) waits at most the idle time after the last request
// (INTEGRATION.md).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "hsv_committee_host.h"

namespace hsvh {
namespace {

constexpr auto kResidentWait = std::chrono::milliseconds(50);
constexpr int kResidentMaxFailures = 4;  // then the service stays off for the process

struct ResidentQc {
  std::mutex mu;
  int device = -1;
  QcResidentReq *h = nullptr;  // coherent pinned
  QcResidentReq *d = nullptr;  // its device address
  hipStream_t stream = nullptr;
  uint32_t seq = 0;
  int failures = 0;                                   // relaunch / answer failures so far
  std::chrono::steady_clock::time_point retry_after;  // backoff after a failure
  int paused = 0;   // live ResidentPause scopes: no request, no relaunch
  // 1 on, 0 off (hsv_set_resident_service); -1: HSV_QC_RESIDENT on first use.
  // Read without the lock: a call that finds it on and the lock busy launches.
  std::atomic<int> mode{-1};
  bool atexit_registered = false;
  std::atomic<bool> started{false};   // its block has run in this process (hsvi_resident_started)
  uint64_t posted = 0, answered = 0;  // requests posted / answered (hsvi_resident_counts)
};

ResidentQc &RQ() {
  static ResidentQc r;
  return r;
}

bool resident_on(ResidentQc &r) {
  int m = r.mode.load(std::memory_order_relaxed);
  if (m < 0) {
    const char *v = std::getenv("HSV_QC_RESIDENT");
    int want = (v && v[0] == '0') ? 0 : 1;
    r.mode.compare_exchange_strong(m, want);  // a concurrent hsv_set_resident_service wins
    m = r.mode.load(std::memory_order_relaxed);
  }
  return m == 1;
}

uint64_t resident_idle_ticks() {
  static const uint64_t t = [] {
    long ms = 50;
    if (const char *v = std::getenv("HSV_QC_RESIDENT_IDLE_MS")) ms = std::atol(v);
    ms = std::max(1L, std::min(ms, 10000L));
    return (uint64_t)ms * 100000ull;  // the kernel's 100 MHz clock
  }();
  return t;
}

// stop the kernel and wait for its grid (mu held)
void resident_stop_locked(ResidentQc &r) {
  if (!r.h || !r.stream) return;
  __atomic_store_n(&r.h->stop, 1u, __ATOMIC_RELEASE);
  DeviceGuard guard(r.device);
  (void)hipStreamSynchronize(r.stream);
  __atomic_store_n(&r.h->stop, 0u, __ATOMIC_RELEASE);
}

// a failed relaunch or an unanswered request (mu held): off for a growing
// backoff, for good after kResidentMaxFailures
void resident_failed_locked(ResidentQc &r) {
  ++r.failures;
  r.retry_after = std::chrono::steady_clock::now() + std::chrono::milliseconds(250 << std::min(r.failures, 6));
}

// the kernel running on `device` (mu held): HSV_OK or kResidentUnavailable
int resident_ensure_locked(ResidentQc &r, int device) {
  if (r.paused || !resident_on(r) || r.failures >= kResidentMaxFailures) return kResidentUnavailable;
  if (r.failures && std::chrono::steady_clock::now() < r.retry_after) return kResidentUnavailable;
  if (r.h && r.device != device) return kResidentUnavailable;  // one device per process
  if (!r.h) {
    void *h = nullptr, *d = nullptr;
    // coherent pinned memory: the running kernel reads what the host writes
    // after it started (a non-coherent area let it read a stale request
    // header and fault, profiles/r04res_pytest_sub2.txt)
    if (hipHostMalloc(&h, sizeof(QcResidentReq), hipHostMallocCoherent) != hipSuccess) {
      r.failures = kResidentMaxFailures;
      return kResidentUnavailable;
    }
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d ||
        hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess) {
      (void)hipHostFree(h);  // the kernel never ran: nothing to wait for
      r.failures = kResidentMaxFailures;
      return kResidentUnavailable;
    }
    std::memset(h, 0, sizeof(QcResidentReq));
    r.h = static_cast<QcResidentReq *>(h);
    r.d = static_cast<QcResidentReq *>(d);
    r.device = device;
    r.seq = 0;
  }
  if (__atomic_load_n(&r.h->alive, __ATOMIC_ACQUIRE) == 1u) return HSV_OK;
  // not running (first use, or it left after its idle time): relaunch
  (void)hipStreamSynchronize(r.stream);  // the previous grid has fully ended
  __atomic_store_n(&r.h->stop, 0u, __ATOMIC_RELEASE);
  if (hsv_launch_comb_resident(r.d, resident_idle_ticks(), r.stream) != hipSuccess) {
    resident_failed_locked(r);
    return kResidentUnavailable;
  }
  r.started.store(true);
  if (!r.atexit_registered) {  // after HIP's own: runs before the runtime tears down
    std::atexit(resident_stop);
    r.atexit_registered = true;
  }
  // The block announces itself once it holds a CU.  A device busy with other
  // grids may not give it one soon: then this call launches instead, the
  // stop word makes the block leave as soon as it starts, and the service
  // backs off.
  const auto t0 = std::chrono::steady_clock::now();
  while (__atomic_load_n(&r.h->alive, __ATOMIC_ACQUIRE) != 1u)
    if (std::chrono::steady_clock::now() - t0 > kResidentWait) {
      resident_stop_locked(r);
      resident_failed_locked(r);
      return kResidentUnavailable;
    }
  return HSV_OK;
}

// ResidentPause and hsvi_resident_pause(1): the kernel stopped (when it runs)
// and, until the matching leave, no request and no relaunch
void resident_pause_enter() {
  ResidentQc &r = RQ();
  std::lock_guard<std::mutex> lk(r.mu);
  ++r.paused;
  if (r.h && __atomic_load_n(&r.h->alive, __ATOMIC_ACQUIRE) == 1u) resident_stop_locked(r);
}

// a leave without its enter (hsvi_resident_pause(0) alone) changes nothing
void resident_pause_leave() {
  ResidentQc &r = RQ();
  std::lock_guard<std::mutex> lk(r.mu);
  if (r.paused > 0) --r.paused;
}

}  // namespace

int resident_run(const CommitteeDev &cd, const uint32_t *key_idx, const uint8_t *sig, size_t sig_stride,
                 const uint8_t *msg, size_t msg_stride, size_t m, uint8_t *flags_out, const uint32_t *btable) {
  ResidentQc &r = RQ();
  // one request at a time: a concurrent caller launches instead of queueing
  // behind this one (the launch path takes 0.039 ms, a queue could take more)
  std::unique_lock<std::mutex> lk(r.mu, std::try_to_lock);
  if (!lk.owns_lock()) return kResidentUnavailable;
  if (resident_ensure_locked(r, cd.device) != HSV_OK) return kResidentUnavailable;
  QcResidentReq &q = *r.h;
  QcResidentBody b{};  // the payload, chunked into the request area at each post
  b.m = (uint32_t)m;
  b.nkeys = cd.n;
  b.inject = (uint32_t)hsvi_inject_mode();
  b.msg_per_vote = msg_stride ? 1u : 0u;
  b.pks = cd.d_pks;
  b.key_flags = cd.d_kflags;
  b.key_tables = cd.d_tabptr;
  b.btable = btable;
  const size_t mm = std::min<size_t>(m, kResidentVotes);  // m > kResidentVotes is the kernel's to refuse
  for (size_t i = 0; i < mm; ++i) {
    b.key_idx[i] = key_idx[i];
    if (key_idx[i] < cd.n) std::memcpy(b.pk[i], cd.h_pks + (size_t)key_idx[i] * 32, 32);  // else flag 0
    std::memcpy(b.sig[i], sig + i * sig_stride, 64);
    if (msg_stride) std::memcpy(b.msg[i], msg + i * msg_stride, 32);
  }
  if (!msg_stride) std::memcpy(b.msg[0], msg, 32);
  uint32_t words[kResidentChunks * 3];
  std::memcpy(words, &b, sizeof(b));
  call_mark(HSV_MARK_STAGED);
  // Each chunk {seq, three payload words} in ONE aligned 16-byte store, the
  // width of the kernel's read of it: a read can then never pair a new seq
  // with an older payload word (16-byte aligned SSE stores are single
  // accesses on x86-64 processors with AVX).  The compiler fence keeps the
  // chunks' stores in program order; x86 makes them visible in that order.
  auto post = [&](uint32_t sq) {
    std::atomic_signal_fence(std::memory_order_release);
    for (int c = 0; c < kResidentChunks; ++c) {
      QcResidentChunk *ch = &q.chunk[c];
#if defined(__SSE2__)
      _mm_store_si128(reinterpret_cast<__m128i *>(ch),
                      _mm_set_epi32((int)words[3 * c + 2], (int)words[3 * c + 1], (int)words[3 * c], (int)sq));
#else
      ch->w[0] = words[3 * c];
      ch->w[1] = words[3 * c + 1];
      ch->w[2] = words[3 * c + 2];
      __atomic_store_n(&ch->seq, sq, __ATOMIC_RELEASE);
#endif
    }
    std::atomic_signal_fence(std::memory_order_release);
  };
  // One retry: the kernel may leave on its idle timer just as a request is
  // posted (it read the doorbell before the store); then it is relaunched
  // and the same request posted again under a new number.
  uint64_t a0 = 0, a1 = 0;
  for (int attempt = 0;; ++attempt) {
    const uint32_t sq = ++r.seq == 0 ? ++r.seq : r.seq;  // never 0
    post(sq);
    ++r.posted;
    call_mark(HSV_MARK_LAUNCH);
    const auto t0 = std::chrono::steady_clock::now();
    bool answered = false;
    for (;;) {  // both 8-byte answer words carry this request's seq
      a0 = __atomic_load_n(&q.answer[0], __ATOMIC_ACQUIRE);
      a1 = __atomic_load_n(&q.answer[1], __ATOMIC_ACQUIRE);
      if ((uint32_t)a0 == sq && (uint32_t)a1 == sq) {
        answered = true;
        break;
      }
      if (std::chrono::steady_clock::now() - t0 > kResidentWait) break;
    }
    if (answered) break;
    if (attempt == 0 && __atomic_load_n(&q.alive, __ATOMIC_ACQUIRE) == 0u &&
        resident_ensure_locked(r, cd.device) == HSV_OK)
      continue;
    // no answer from a running kernel: stop it and back off, the launch
    // path answers
    resident_stop_locked(r);
    resident_failed_locked(r);
    return kResidentUnavailable;
  }
  ++r.answered;
  call_mark(HSV_MARK_SYNC);
  const uint32_t fb = (uint32_t)(a1 >> 32), fl = (uint32_t)(a0 >> 32);
  if (fb & kResidentBadRequest)
    return fail(HSV_ERR_DEVICE_FAULT, "committee verify (resident): the kernel refused the request header");
  const uint32_t fw[2] = {fb & kResidentFaultCurve, fb & kResidentFaultCanary};
  const int rc = check_faults(reinterpret_cast<const uint8_t *>(fw), "committee verify (resident)");
  if (rc != HSV_OK) return rc;
  for (size_t i = 0; i < m; ++i) flags_out[i] = (uint8_t)(fl >> (8 * i));
  call_mark(HSV_MARK_DONE);
  return HSV_OK;
}

bool resident_enabled() { return resident_on(RQ()); }

void resident_stop() {
  ResidentQc &r = RQ();
  std::lock_guard<std::mutex> lk(r.mu);
  resident_stop_locked(r);
}

// A scope in which the resident kernel does not run: the constructor stops it
// (when it runs) and, until the destructor, no request is posted and no
// relaunch happens -- a concurrent small call takes the launch path.  Around
// every hipFree / hipHostFree of the library (they wait for every grid on the
// device, and would otherwise wait for the service's idle exit, or forever
// under steady requests) and around its device-wide waits.
ResidentPause::ResidentPause() { resident_pause_enter(); }

ResidentPause::~ResidentPause() { resident_pause_leave(); }

// Stop the resident kernel now, without keeping it paused (the next request
// relaunches it).  A no-op when it does not run.
void resident_quiesce() { ResidentPause p; }

void resident_counts(uint64_t *posted, uint64_t *answered) {
  ResidentQc &r = RQ();
  std::lock_guard<std::mutex> lk(r.mu);
  if (posted) *posted = r.posted;
  if (answered) *answered = r.answered;
}

// hsv_set_resident_service: 1 on, 0 off (the kernel stops now); the previous mode
int resident_set_mode(int on) {
  ResidentQc &r = RQ();
  std::lock_guard<std::mutex> lk(r.mu);
  const int prev = resident_on(r) ? 1 : 0;
  r.mode.store(on ? 1 : 0);
  if (!on) resident_stop_locked(r);
  if (on) r.failures = 0;  // an explicit re-enable clears the backoff
  return prev;
}

// Test hook: one resident request whose header claims m votes (0 or above
// the limit: the kernel must refuse it with HSV_ERR_DEVICE_FAULT, never read
// through it); needs the automatic cache's committee (nkeys, tables).
int resident_post_bad(uint32_t m) {
  if (!resident_enabled()) return fail(HSV_ERR_INVALID_ARG, "the resident service is off");
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(home_device());
  DeviceGuard guard(c.device);
  rc = ensure_btable(c);
  if (rc != HSV_OK) return rc;
  // resident_run copies min(m, kResidentVotes) votes: arrays of that size
  const uint32_t idx[kResidentVotes] = {};
  uint8_t sig[kResidentVotes * 64] = {}, msg[32] = {}, flags[16];
  CommitteeDev cd;
  cd.device = c.device;
  cd.n = 1;
  static const uint8_t zero_key[32] = {0};
  cd.h_pks = zero_key;
  cd.d_pks = reinterpret_cast<const uint8_t *>(c.d_btable);  // valid device memory, never read: m is refused
  cd.d_kflags = cd.d_pks;
  cd.d_tabptr = reinterpret_cast<const uint32_t *const *>(c.d_btable);
  rc = resident_run(cd, idx, sig, 64, msg, 0, m, flags, c.d_btable);
  return rc == kResidentUnavailable ? fail(HSV_ERR_HIP, "resident service unavailable") : rc;
}

}  // namespace hsvh

extern "C" void hsvi_resident_pause(int on) { on ? hsvh::resident_pause_enter() : hsvh::resident_pause_leave(); }

extern "C" int hsvi_resident_started(void) {
  hsvh::ResidentQc &r = hsvh::RQ();
  return r.started.load() && hsvh::resident_on(r) ? 1 : 0;
}

extern "C" int hsv_set_resident_service(int mode) { return hsvh::resident_set_mode(mode != 0); }
