// The signer census behind the C ABI (hsv_census_keys*, hsv_census_transactions*):
// the distinct signer keys of a batch and how often each occurs, counted on
// the device (hsv_census.hip), so that a caller can build the hsv_committee
// that hsv_committee_verify_transactions* wants from the keys it actually sees.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "hsv.h"
#include "hsv_census.hpp"
#include "hsv_committee_host.h"
#include "hsv_internal.h"
#include "hsv_keyindex.hpp"

namespace hsvh {
namespace {

constexpr int kModeKeys = 0, kModeOffsets = 1, kModeFixed = 2;  // hsv_launch_census
constexpr size_t kCensusHostMax = size_t(1) << 22;               // items of a host form

thread_local uint64_t t_census_seed = 0;  // hsv_test_census_seed; 0: the per-process seed
uint64_t census_seed() { return t_census_seed ? t_census_seed : KeyHash::seed(); }

int slots_ok(uint32_t slots) {
  return hsv::census_slots_ok(slots) ? HSV_OK
                                     : fail(HSV_ERR_INVALID_ARG, "slots must be a power of two in [16, 2^22]");
}

// the launch, for a committee to leave out or none
int census_enqueue(const hsv_committee *skip, int mode, const uint8_t *d_in, const uint64_t *d_offsets, size_t stride,
                   size_t n, uint32_t slots, uint8_t *d_keys_out, uint32_t *d_counts_out, hsv_census_summary *d_summary,
                   hipStream_t s) {
  CommitteeKeys k;
  if (skip) k = committee_keys_of(skip);
  const hipError_t e = hsv_launch_census(mode, d_in, d_offsets, stride, (uint32_t)n, slots, census_seed(), k.d_keytab,
                                         k.keymask, KeyHash::seed(), k.d_pks, k.n, d_keys_out, d_counts_out, d_summary, s);
  return e == hipSuccess ? HSV_OK : hip_fail("census launch", e);
}

// the checks the two device forms share, after their input's own
int device_args_ok(size_t n, uint32_t slots, const uint8_t *d_keys_out, const uint32_t *d_counts_out,
                   const hsv_census_summary *d_summary) {
  const int rc = slots_ok(slots);
  if (rc != HSV_OK) return rc;
  if (!d_keys_out || !d_counts_out || !d_summary) return fail(HSV_ERR_INVALID_ARG, "null output");
  if (n > 0xffffffffull) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if ((reinterpret_cast<uintptr_t>(d_keys_out) & 15u) != 0)
    return fail(HSV_ERR_ALIGN, "d_keys_out must be 16-byte aligned");
  if (((reinterpret_cast<uintptr_t>(d_counts_out) | reinterpret_cast<uintptr_t>(d_summary)) & 7u) != 0)
    return fail(HSV_ERR_ALIGN, "d_counts_out and d_summary must be 8-byte aligned");
  return HSV_OK;
}

int device_census(const hsv_committee *skip, int mode, const uint8_t *d_in, const uint64_t *d_offsets, size_t stride,
                  size_t n, uint32_t slots, uint8_t *d_keys_out, uint32_t *d_counts_out, hsv_census_summary *d_summary,
                  void *stream) {
  DeviceCall call;
  const void *where = d_in ? static_cast<const void *>(d_in) : d_keys_out;  // n == 0: the inputs may be NULL
  int rc = ensure_init();  // before the handle is read: without a device there is no committee
  if (rc != HSV_OK) return rc;
  rc = skip ? call.begin(where, stream, nullptr, DeviceCall::kNone, "committee", committee_device_of(skip))
            : call.begin(where, stream, nullptr, DeviceCall::kNone);
  if (rc != HSV_OK) return rc;
  return census_enqueue(skip, mode, d_in, d_offsets, stride, n, slots, d_keys_out, d_counts_out, d_summary,
                        call.stream);
}

// The host forms' one body: key(i) is item i's 32 key bytes in the caller's
// memory, or NULL for a malformed transaction, which is counted here and never
// staged.  The keys are gathered into a slot's pinned staging piece by piece
// (BatchSpan over 32-byte items: at most kChunk items and g_stage_bytes bytes
// per copy), the key kernel runs once over all of them in a StagedBlock, and
// the `distinct` entries come back to be sorted.
template <class KeyOf>
int host_census(hsv_committee *skip, const KeyOf &key, size_t n, uint32_t slots, uint8_t *keys_out,
                uint32_t *counts_out, size_t keys_cap, hsv_census_summary *summary, const char *where) {
  int rc = ensure_init();
  if (rc != HSV_OK) return rc;
  DevCtx &c = ctx(skip ? committee_device_of(skip) : home_device());
  DeviceGuard guard(c.device);
  if (guard.status() != hipSuccess) return hip_fail("hipSetDevice", guard.status());
  std::vector<uint32_t> good;  // the well-formed items
  good.reserve(n);
  for (size_t i = 0; i < n; ++i)
    if (key(i)) good.push_back((uint32_t)i);
  const size_t m = good.size();
  const BatchSpan span{nullptr, 32, 32};
  const size_t piece = m ? span.chunk_end(0, m, kChunk, g_stage_bytes.load()) : 0;
  SlotLease lease(c);
  Slot &s = lease.slot();
  rc = slot_prepare(s, 0, std::max<size_t>(piece * 32, kAlign));
  if (rc != HSV_OK) return rc;
  StagedBlock blk(s.stream);
  const size_t off_keys = blk.add(m * 32), off_kout = blk.add((size_t)slots * 32);
  const size_t off_cout = blk.add((size_t)slots * 4), off_sum = blk.add(sizeof(hsv_census_summary));
  rc = blk.alloc("allocating the census buffers");
  if (rc != HSV_OK) return rc;
  for (size_t a = 0; a < m && blk.ok(); a += piece) {
    const size_t b = std::min(m, a + piece);
    for (size_t j = a; j < b; ++j) std::memcpy(s.h_buf + (j - a) * 32, key(good[j]), 32);
    blk.in(off_keys + a * 32, s.h_buf, (b - a) * 32);
    if (blk.ok()) blk.step(hipStreamSynchronize(s.stream));  // the staging is written again
  }
  if (blk.ok())
    rc = census_enqueue(skip, kModeKeys, blk.at(off_keys), nullptr, 32, m, slots, blk.at(off_kout),
                        reinterpret_cast<uint32_t *>(blk.at(off_cout)),
                        reinterpret_cast<hsv_census_summary *>(blk.at(off_sum)), s.stream);
  hsv_census_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  std::vector<uint8_t> keys;
  std::vector<uint32_t> counts;
  if (rc == HSV_OK && blk.ok()) {
    blk.out(&sum, off_sum, sizeof(sum));
    if (blk.ok()) blk.step(hipStreamSynchronize(s.stream));
    if (blk.ok() && sum.distinct <= slots) {
      keys.resize((size_t)sum.distinct * 32);
      counts.resize(sum.distinct);
      blk.out(keys.data(), off_kout, keys.size());
      blk.out(counts.data(), off_cout, counts.size() * 4);
    }
  }
  const int frc = blk.finish(where);  // frees the block and drains the stream
  if (rc != HSV_OK) return rc;
  if (frc != HSV_OK) return frc;
  if (sum.distinct > slots) return fail(HSV_ERR_HIP, "census summary out of range");
  // count descending, then key bytes ascending
  std::vector<uint32_t> order(sum.distinct);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    if (counts[x] != counts[y]) return counts[x] > counts[y];
    return std::memcmp(&keys[(size_t)x * 32], &keys[(size_t)y * 32], 32) < 0;
  });
  const size_t w = std::min<size_t>(sum.distinct, keys_cap);
  for (size_t j = 0; j < w; ++j) {
    std::memcpy(keys_out + j * 32, &keys[(size_t)order[j] * 32], 32);
    counts_out[j] = counts[order[j]];
  }
  sum.items = n;
  sum.malformed = n - m;
  *summary = sum;
  return HSV_OK;
}

// the checks the two host forms share, after their input's own
int host_args_ok(size_t n, uint32_t slots, const uint8_t *keys_out, const uint32_t *counts_out, size_t keys_cap,
                 const hsv_census_summary *summary) {
  const int rc = slots_ok(slots);
  if (rc != HSV_OK) return rc;
  if (!summary || (keys_cap && (!keys_out || !counts_out))) return fail(HSV_ERR_INVALID_ARG, "null output");
  if (n > kCensusHostMax) return fail(HSV_ERR_INVALID_ARG, "more than 2^22 items (census a sample, or use the device form)");
  return HSV_OK;
}

}  // namespace
}  // namespace hsvh

using namespace hsvh;

extern "C" {

void hsvi_set_census_seed(uint64_t seed) { t_census_seed = seed; }

int hsv_census_keys_device(const hsv_committee *skip, const uint8_t *d_pk, size_t pk_stride, size_t n, uint32_t slots,
                           uint8_t *d_keys_out, uint32_t *d_counts_out, hsv_census_summary *d_summary, void *stream) {
  int rc = device_args_ok(n, slots, d_keys_out, d_counts_out, d_summary);
  if (rc != HSV_OK) return rc;
  if (n && !d_pk) return fail(HSV_ERR_INVALID_ARG, "null d_pk");
  if (((reinterpret_cast<uintptr_t>(d_pk) | pk_stride) & 15u) != 0)
    return fail(HSV_ERR_ALIGN, "d_pk and pk_stride must be multiples of 16");
  if (n && pk_stride < 32) return fail(HSV_ERR_INVALID_ARG, "key records overlap");
  return device_census(skip, kModeKeys, d_pk, nullptr, pk_stride, n, slots, d_keys_out, d_counts_out, d_summary,
                       stream);
}

int hsv_census_transactions_device(const hsv_committee *skip, const uint8_t *d_txs, const uint64_t *d_offsets,
                                   size_t tx_size, size_t n, uint32_t slots, uint8_t *d_keys_out,
                                   uint32_t *d_counts_out, hsv_census_summary *d_summary, void *stream) {
  int rc = device_args_ok(n, slots, d_keys_out, d_counts_out, d_summary);
  if (rc != HSV_OK) return rc;
  if (n && !d_txs) return fail(HSV_ERR_INVALID_ARG, "null d_txs");
  if (n && !d_offsets && tx_size < 96) return fail(HSV_ERR_INVALID_ARG, "transactions are shorter than 96 bytes");
  if (reinterpret_cast<uintptr_t>(d_offsets) & 7u) return fail(HSV_ERR_ALIGN, "d_offsets must be 8-byte aligned");
  return device_census(skip, d_offsets ? kModeOffsets : kModeFixed, d_txs, d_offsets, d_offsets ? 0 : tx_size, n, slots,
                       d_keys_out, d_counts_out, d_summary, stream);
}

int hsv_census_keys(hsv_committee *skip, const uint8_t *pk, size_t pk_stride, size_t n, uint32_t slots,
                    uint8_t *keys_out, uint32_t *counts_out, size_t keys_cap, hsv_census_summary *summary) {
  CallScope call;
  int rc = host_args_ok(n, slots, keys_out, counts_out, keys_cap, summary);
  if (rc != HSV_OK) return rc;
  if (n && !pk) return fail(HSV_ERR_INVALID_ARG, "null pk");
  if (n && pk_stride < 32) return fail(HSV_ERR_INVALID_ARG, "key records overlap");
  return host_census(skip, [&](size_t i) { return pk + i * pk_stride; }, n, slots, keys_out, counts_out, keys_cap,
                     summary, "hsv_census_keys");
}

int hsv_census_transactions(hsv_committee *skip, const uint8_t *txs, const uint64_t *offsets, size_t tx_size, size_t n,
                            uint32_t slots, uint8_t *keys_out, uint32_t *counts_out, size_t keys_cap,
                            hsv_census_summary *summary) {
  CallScope call;
  int rc = host_args_ok(n, slots, keys_out, counts_out, keys_cap, summary);
  if (rc != HSV_OK) return rc;
  if (n && !txs) return fail(HSV_ERR_INVALID_ARG, "null txs");
  if (n && !offsets && tx_size < 96) return fail(HSV_ERR_INVALID_ARG, "transactions are shorter than 96 bytes");
  return host_census(
      skip,
      [&](size_t i) -> const uint8_t * {
        const uint64_t lo = offsets ? offsets[i] : (uint64_t)i * tx_size;
        const uint64_t hi = offsets ? offsets[i + 1] : lo + tx_size;
        return hi >= lo && hi - lo >= 96 ? txs + hi - 96 : nullptr;
      },
      n, slots, keys_out, counts_out, keys_cap, summary, "hsv_census_transactions");
}

}  // extern "C"
