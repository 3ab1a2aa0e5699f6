// The benchmark's sample transactions behind the C ABI (include/hsv.h):
// hsv_batch_samples_bincode* -- what the `benchmark` block of BatchMaker::seal
// logs about a batch (mempool/src/batch_maker.rs:118-125, 133-153), from its
// stored bincode bytes -- and hsv_client_bursts*, the transactions the
// benchmark client sends (node/src/client.rs:106-148).  The device forms run in
// hsv_samples.hip; the host forms need no GPU.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <string>
#include <vector>

#include "hsv.h"
#include "hsv_host.h"
#include "hsv_internal.h"
#include "hsv_samples.hpp"
#include "hsv_wire_parse.h"

using namespace hsvh;

namespace {

int bursts_args_ok(const uint8_t *txs, size_t tx_size, size_t trailer, uint64_t burst, size_t n) {
  if (burst == 0) return fail(HSV_ERR_INVALID_ARG, "burst is 0");
  if (trailer > tx_size || tx_size - trailer < hsv::kClientPreamble)
    return fail(HSV_ERR_INVALID_ARG, "tx_size is below 9 + trailer");
  if (n && !txs) return fail(HSV_ERR_INVALID_ARG, "null txs");
  if (n > 0xffffffffull) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if (n && tx_size > ~size_t(0) / n) return fail(HSV_ERR_INVALID_ARG, "n * tx_size does not fit");
  return HSV_OK;
}

}  // namespace

extern "C" {

int hsv_batch_samples_bincode(const uint8_t *buf, size_t len, hsv_batch_samples *res, uint64_t *ids_out,
                              size_t ids_cap) {
  if (!buf && len) return fail(HSV_ERR_INVALID_ARG, "null buffer");
  std::vector<uint64_t> spans;
  std::string err;
  size_t n = 0;
  if (!hsvw::parse_batch(buf, len, 0, &spans, n, err)) return fail(HSV_ERR_PARSE, "bincode: " + err);
  hsv_batch_samples r{HSV_BATCH_OK, 0, n, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    const uint64_t lo = spans[2 * i], tx_len = spans[2 * i + 1] - lo;
    r.size += tx_len;
    if (!tx_len || !hsv::is_sample(tx_len, buf[lo])) continue;
    if (ids_out && r.n_samples < ids_cap) {
      uint64_t id = 0;
      for (int k = 1; k <= 8; ++k) id = (id << 8) | buf[lo + k];
      ids_out[r.n_samples] = id;
    }
    ++r.n_samples;
  }
  if (res) *res = r;
  if (ids_out && ids_cap < r.n_samples) return fail(HSV_ERR_INVALID_ARG, "ids_cap is below the sample count");
  return 1;
}

int hsv_batches_samples_bincode_device(const uint8_t *d_bufs, const uint64_t *d_offsets, size_t n_batches,
                                       size_t tx_cap, hsv_batch_samples *d_index, uint64_t *d_ids, size_t ids_cap,
                                       void *stream) {
  if (n_batches == 0) return HSV_OK;
  if (!d_bufs || !d_offsets || !d_index || (ids_cap && !d_ids)) return fail(HSV_ERR_INVALID_ARG, "null argument");
  if (n_batches > 0xffffffffu || tx_cap > 0xffffffffu) return fail(HSV_ERR_INVALID_ARG, "batch too large");
  if ((reinterpret_cast<uintptr_t>(d_offsets) | reinterpret_cast<uintptr_t>(d_index) |
       reinterpret_cast<uintptr_t>(d_ids)) & 7u)
    return fail(HSV_ERR_ALIGN, "d_offsets, d_index and d_ids must be 8-byte aligned");
  DeviceCall call;
  const int rc = call.begin(d_bufs, stream, nullptr, DeviceCall::kNone);
  if (rc != HSV_OK) return rc;
  const hipError_t e =
      hsv_launch_batch_samples(d_bufs, d_offsets, (uint32_t)n_batches, tx_cap, d_index, d_ids, ids_cap, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("sample index launch", e);
}

int hsv_client_bursts(uint8_t *txs, size_t tx_size, size_t trailer, uint64_t counter0, uint64_t burst, uint64_t r0,
                      size_t n, uint64_t *r_out) {
  const int rc = bursts_args_ok(txs, tx_size, trailer, burst, n);
  if (rc != HSV_OK) return rc;
  const size_t body = tx_size - trailer;
  for (size_t i = 0; i < n; ++i) {
    const hsv::ClientPreamble p = hsv::client_preamble(i, burst, counter0, r0);
    uint8_t *a = txs + i * tx_size;
    for (size_t k = 0; k < hsv::kClientPreamble; ++k) a[k] = p.byte(k);
    std::memset(a + hsv::kClientPreamble, 0, body - hsv::kClientPreamble);
  }
  if (r_out) *r_out = r0 + hsv::client_standard_before(n, burst, counter0);
  return HSV_OK;
}

int hsv_client_bursts_device(uint8_t *d_txs, size_t tx_size, size_t trailer, uint64_t counter0, uint64_t burst,
                             uint64_t r0, size_t n, uint64_t *r_out, void *stream) {
  int rc = bursts_args_ok(d_txs, tx_size, trailer, burst, n);
  if (rc != HSV_OK) return rc;
  if (r_out) *r_out = r0 + hsv::client_standard_before(n, burst, counter0);  // host arithmetic: nothing is read back
  if (n == 0) return HSV_OK;
  DeviceCall call;
  rc = call.begin(d_txs, stream, nullptr, DeviceCall::kNone);
  if (rc != HSV_OK) return rc;
  const hipError_t e = hsv_launch_client_bursts(d_txs, tx_size, trailer, counter0, burst, r0, n, call.stream);
  return e == hipSuccess ? HSV_OK : hip_fail("client burst launch", e);
}

}  // extern "C"
