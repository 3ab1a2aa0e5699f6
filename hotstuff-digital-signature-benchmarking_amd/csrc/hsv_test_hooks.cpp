// The exported test and measurement hooks of libhsv_test.so (declared in
// csrc/hsv_test_hooks.h).  Each forwards to an internal, hidden function of
// the shared objects; libhsv.so is linked without this file.
#include "hsv_test_hooks.h"

#include <string>
#include <thread>
#include <vector>

#include "hsv_host.h"
#include "hsv_internal.h"

extern "C" {

int hsv_test_inject_fault(int mode) { return hsvi_set_inject(mode); }
int hsv_test_inject_mode(void) { return hsvi_inject_mode(); }
int hsv_test_corrupt_auto_committee(void) { return hsvh::auto_committee_corrupt_tables(); }
int hsv_test_lanesplit_check(const uint32_t *in, uint32_t rows, uint32_t *out) {
  return hsvi_lanesplit_check(in, rows, out);
}
int hsv_test_field_ops(const uint32_t *in, uint32_t n, uint32_t *out) { return hsvi_test_field_ops(in, n, out); }
int hsv_test_scalar_ops(const uint32_t *in, uint32_t n, uint32_t *out) { return hsvi_test_scalar_ops(in, n, out); }
int hsv_set_lattice_bits(int bits) { return hsvi_set_lattice_bits(bits); }
int hsv_test_deal(int mode) { return hsvi_set_deal(mode); }
int hsv_test_deal_counts(uint32_t out[6]) { return out ? hsvi_deal_counts(out) : HSV_ERR_INVALID_ARG; }
int hsv_set_variant(int variant) { return hsvi_set_variant(variant); }
int hsv_variant_list(int *out, int cap) { return hsvi_variant_list(out, cap); }
int hsv_variant_available(int variant) { return hsvi_variant_available(variant); }
int hsv_num_variants(void) { return hsvi_num_variants(); }
int hsv_set_virtual_shards(int k) { return hsvi_set_virtual_shards(k); }
int hsv_test_pipe_nocopy(int on) { return hsvi_set_pipe_nocopy(on); }
int hsv_test_pipe_schedule(const uint64_t *sizes, int count) { return hsvi_set_pipe_schedule(sizes, count); }

int hsv_test_numa_plan(const char *sysfs_root, const char *bdfs_csv, const char *allowed_cpulist, int pack_default,
                       int *node_out, int *ncpus_out, int *pack_out, int cap) {
  if (!sysfs_root || !bdfs_csv || !allowed_cpulist) return HSV_ERR_INVALID_ARG;
  std::vector<std::string> bdfs;
  std::string cur;
  for (const char *p = bdfs_csv;; ++p) {
    if (*p == ',' || *p == '\0') {
      bdfs.push_back(cur);
      cur.clear();
      if (*p == '\0') break;
    } else {
      cur += *p;
    }
  }
  std::vector<int> allowed;
  if (!hsvh::parse_cpulist(allowed_cpulist, allowed)) return HSV_ERR_INVALID_ARG;
  const std::vector<hsvh::HostPlace> pl = hsvh::plan_host_places(sysfs_root, bdfs, allowed, pack_default);
  for (int i = 0; i < (int)pl.size() && i < cap; ++i) {
    if (node_out) node_out[i] = pl[i].node;
    if (ncpus_out) ncpus_out[i] = (int)pl[i].cpus.size();
    if (pack_out) pack_out[i] = pl[i].pack_threads;
  }
  return (int)pl.size();
}

int hsv_test_pinned_thread_cpus(const char *cpulist, int *cpus_out, int cap) {
  std::vector<int> want;
  if (!cpulist || !hsvh::parse_cpulist(cpulist, want)) return HSV_ERR_INVALID_ARG;
  std::vector<int> got;
  bool ok = false;
  std::thread t([&] {
    ok = hsvh::pin_current_thread(want);
    got = hsvh::current_affinity();
  });
  t.join();
  if (!ok) return HSV_ERR_INVALID_ARG;
  for (int i = 0; i < (int)got.size() && i < cap; ++i) cpus_out[i] = got[i];
  return (int)got.size();
}
void hsv_test_resident_counts(uint64_t *posted, uint64_t *answered) { hsvh::resident_counts(posted, answered); }
int hsv_test_resident_post_bad(uint32_t m) { return hsvh::resident_post_bad(m); }
int hsv_test_tx_records(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                        uint8_t *d_records, void *stream) {
  if (n > UINT32_MAX) return HSV_ERR_INVALID_ARG;
  const hipError_t e = hsv_launch_tx_records(d_txs, d_offsets, tx_size, (uint32_t)n, d_records,
                                             reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? HSV_OK : HSV_ERR_HIP;
}
int hsv_test_signer_group(int g) { return hsvi_set_signer_group(g); }
size_t hsv_test_tx_sign_chunk(size_t items) { return hsvi_set_tx_sign_chunk(items); }
size_t hsv_test_msg_sign_chunk(size_t items) { return hsvi_set_msg_sign_chunk(items); }
int hsv_test_committee_tx_counts(uint64_t out[3]) { return hsvh::committee_tx_counts(out); }
int hsv_test_committee_msgs_counts(uint64_t out[3]) { return hsvh::committee_msgs_counts(out); }
int hsv_test_msgs_small(int mode) { return hsvi_set_msgs_small(mode); }
int hsv_test_msgs_form_counts(uint64_t out[5]) { return hsvi_msgs_form_counts(out); }
int hsv_test_cmsg_indexed_form(int mode) { return hsvi_set_cmsg_indexed_form(mode); }
int hsv_test_cmsg_indexed_counts(uint64_t out[3]) {
  if (!out) return HSV_ERR_INVALID_ARG;
  return hsvi_cmsg_indexed_counts(out) == 0 ? HSV_OK : HSV_ERR_HIP;
}
int hsv_test_batch_stages(const uint8_t *d_bufs, const uint64_t *d_offsets, size_t n_batches, size_t tx_cap,
                          void *d_results, float ms_out[4]) {
  return hsvh::batch_stage_times(d_bufs, d_offsets, n_batches, tx_cap, static_cast<hsv_batch_result *>(d_results),
                                 ms_out);
}
int hsv_test_census_seed(uint64_t seed) {
  hsvi_set_census_seed(seed);
  return HSV_OK;
}
int hsv_test_seal_stages(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                         const uint8_t *d_flags, uint64_t batch_size, int flush, uint8_t *d_out, size_t out_cap,
                         uint64_t *d_batch_offsets, size_t batches_cap, uint8_t *d_digests, void *d_summary,
                         float ms_out[4]) {
  return hsvh::seal_stage_times(d_txs, d_offsets, tx_size, n, d_flags, batch_size, flush, d_out, out_cap,
                                d_batch_offsets, batches_cap, d_digests, static_cast<hsv_seal_summary *>(d_summary),
                                ms_out);
}
size_t hsv_test_stage_bytes(size_t bytes) { return hsvh::g_stage_bytes.exchange(bytes ? bytes : hsvh::kStageBytes); }

}  // extern "C"
