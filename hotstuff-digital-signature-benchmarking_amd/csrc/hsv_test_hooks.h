/*
 * hsv_test_hooks.h -- test and measurement hooks of libhsv_test.so.
 *
 * libhsv_test.so is libhsv.so's object files plus csrc/hsv_test_hooks.cpp and
 * the test kernels of csrc/hsv_test_prims.hip: the same product kernels and
 * host code, and in addition the hooks below.  The
 * product library exports none of them (tests/test_capi.py checks its
 * dynamic symbols against include/hsv.h), so no stray call can change the
 * behaviour of a deployed process.  tests/ and tools/ load libhsv_test.so
 * for the cases that need a hook (hsverify/_testing.py).
 */
#ifndef HSV_TEST_HOOKS_H_
#define HSV_TEST_HOOKS_H_

#include "hsv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fault injection for the launches the CALLING THREAD issues from now on
 * (csrc/hsv_verify_core.hpp kInject*: 1 zeroed tables, 2 overwritten
 * workspace canary, 3 one flipped table bit; 0 = off).  Other threads' calls
 * are unaffected.  Returns the previous mode, or -1 for an unknown one. */
HSV_API int hsv_test_inject_fault(int mode);
HSV_API int hsv_test_inject_mode(void);
/* Zero the tables of the automatic committee cache in HBM (a real
 * corruption, for the cached path's self-check); returns the number of
 * cached keys, 0 when there is no cache, < 0 on error. */
HSV_API int hsv_test_corrupt_auto_committee(void);
/* Row-form field arithmetic against the one-lane form (tests/test_lanesplit.py). */
HSV_API int hsv_test_lanesplit_check(const uint32_t *in, uint32_t rows, uint32_t *out);
/* The device's one-lane field arithmetic (hsv_fe26x10.hpp, its inline-asm
 * branch) and its mod-l and lattice routines on raw operands, one item per
 * lane (csrc/hsv_test_prims.hpp has the op codes and the record layout; the
 * same text runs on the host in tests/native/prims_host.cpp).  in: n records
 * of 24 (field) or 32 (scalar) words; out: n records of 24 or 16 words, all
 * host memory.  0, or a hipError_t (tests/test_prims_gpu.py). */
HSV_API int hsv_test_field_ops(const uint32_t *in, uint32_t n, uint32_t *out);
HSV_API int hsv_test_scalar_ops(const uint32_t *in, uint32_t n, uint32_t *out);
/* Lattice bound of the comb-path prepass (0 = default 138; 133 sends the
 * lattice-fallback fixtures down the full-length path); previous bound or -1. */
HSV_API int hsv_set_lattice_bits(int bits);
/* Tests and A/B runs: how the CALLING THREAD's following two-launch point
 * passes (above 2^13 items: hsv_verify_device, hsv_verify_msgs*) take their
 * batches.  Bit 0: dealt by column count (the default, 1); clear: index
 * order, the same flags.  Bit 1: each such launch waits for its stream and
 * keeps the lengths of its class lists for hsv_test_deal_counts.  Returns the
 * previous mode, or -1 for an unknown one. */
HSV_API int hsv_test_deal(int mode);
/* Items per column class of the calling thread's last launch under bit 1:
 * out[0] those that need >= 67 columns, out[1] 66, ... out[5] at most 62
 * (fallback items are on no list; all zero after an index-order launch).
 * HSV_OK. */
HSV_API int hsv_test_deal_counts(uint32_t out[6]);
/* Kernel variant of the following calls (the ids hsv_variant_list reports). */
HSV_API int hsv_set_variant(int variant);
HSV_API int hsv_variant_list(int *out, int cap);
HSV_API int hsv_variant_available(int variant);
HSV_API int hsv_num_variants(void);
/* Split host batches of >= 2^16 items into k shards on the bound device
 * (the multi-device gather path on a one-GPU box); 0 restores the default. */
HSV_API int hsv_set_virtual_shards(int k);
/* Measurement only (tools/host_api_ab.py): a pipelined host call of the same
 * size as the slot's previous one skips the pack and the copies and verifies
 * what that call left in HBM -- the chunk schedule's GPU time alone.  Its
 * flags are the previous inputs' flags, so it never belongs in a product
 * library.  Returns the previous setting. */
HSV_API int hsv_test_pipe_nocopy(int on);
/* Measurement only (tools/host_sched_ab.py): the launch-chunk sizes of the
 * pipelined host call (items; the last size repeats; count 0 restores the
 * default schedule).  Returns HSV_OK or HSV_ERR_INVALID_ARG. */
HSV_API int hsv_test_pipe_schedule(const uint64_t *sizes, int count);
/* Host placement plan (csrc/hsv_numa.cpp) for the PCI functions in bdfs_csv
 * ("0000:0d:00.0,...") under a sysfs tree at sysfs_root, within the CPUs of
 * allowed_cpulist ("0-7"): per function its NUMA node (-1 unknown), the
 * number of that node's allowed CPUs its threads are pinned to, and its
 * pack-pool size.  Returns the number of functions or HSV_ERR_INVALID_ARG. */
HSV_API int hsv_test_numa_plan(const char *sysfs_root, const char *bdfs_csv, const char *allowed_cpulist,
                               int pack_default, int *node_out, int *ncpus_out, int *pack_out, int cap);
/* A thread pinned the way the library pins its shard workers and pack
 * helpers, to the CPUs of `cpulist`: the affinity it then reports (count, CPUs
 * written to cpus_out), or HSV_ERR_INVALID_ARG. */
HSV_API int hsv_test_pinned_thread_cpus(const char *cpulist, int *cpus_out, int cap);
/* The resident latency service (HSV_QC_RESIDENT=1): requests posted to it and
 * answered by it in this process so far (either pointer may be NULL). */
HSV_API void hsv_test_resident_counts(uint64_t *posted, uint64_t *answered);
/* Post one resident request whose header claims m votes (0, or above the
 * service's limit): the kernel must refuse it, so the call returns
 * HSV_ERR_DEVICE_FAULT without reading through the header. */
HSV_API int hsv_test_resident_post_bad(uint32_t m);
/* Measurement only (tools/mempool_split_probe.py): the 128-byte records
 * pk || R || s || SHA-512(message)[..32] of n transactions, enqueued on
 * `stream` (the record kernel of hsv_verify_transactions_device's small-batch
 * form, without the verification). */
HSV_API int hsv_test_tx_records(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                                uint8_t *d_records, void *stream);
/* Measurement (tools/sign_bench.py) and tests: items per lane (G) of the
 * signer's following launches -- the batch over which one field inversion is
 * shared (csrc/hsv_sign_core.hpp).  Built: 1 (unbatched), 2, 4, 8, 16; 0
 * restores the product's.  Returns the previous value, or -1 for a value that
 * is not built. */
HSV_API int hsv_test_signer_group(int g);
/* Tests: items per launch of hsv_signer_sign_transactions* (the product's is
 * 2^22), so that a batch of a few hundred transactions crosses a launch
 * boundary.  0 restores the product's.  Returns the previous value. */
HSV_API size_t hsv_test_tx_sign_chunk(size_t items);
/* Tests: items per round of hsv_signer_sign_msgs* (the product's is 2^22), so
 * that a batch of a few hundred messages crosses a round boundary.  0 restores
 * the product's.  Returns the previous value. */
HSV_API size_t hsv_test_msg_sign_chunk(size_t items);
/* Tests: bytes of transactions or messages the host forms hsv_verify_transactions*,
 * hsv_verify_msgs, hsv_signer_sign_transactions and hsv_signer_sign_msgs stage per launch (the
 * product's is 2^29; one larger item goes alone), so that a small batch takes
 * several launches and its offsets are rebased.  0 restores the product's.
 * Returns the previous value. */
HSV_API size_t hsv_test_stage_bytes(size_t bytes);
/* Tests: how the calling thread's last hsv_committee_verify_transactions* call
 * split its batch, summed over its rounds: out[0] transactions verified from
 * a member's comb table (hits), out[1] by the generic kernels (misses),
 * out[2] those of the misses that took the full-length fallback path.  The
 * lengths live on the device: after the device form they are valid once the
 * caller has synchronised its stream.  HSV_OK, or HSV_ERR_INVALID_ARG when the
 * thread has made no such call. */
HSV_API int hsv_test_committee_tx_counts(uint64_t out[3]);
/* Tests: the same for the calling thread's last hsv_committee_verify_msgs*
 * call (items instead of transactions).  The two hooks keep slots of their
 * own: a call of one kind leaves the other hook's answer as it was. */
HSV_API int hsv_test_committee_msgs_counts(uint64_t out[3]);
/* Tests and measurement (tools/msgs_small_bench.py): how hsv_verify_msgs*
 * verifies a launch of at most 2^13 items.  -1 = the small form of that size
 * (the default); 0 = the message prepass and the point pass, two launches, as
 * larger batches; 1, 2, 3, 4 = the quad, joint, row, pair form at every such
 * size.  Process-wide; the product library has no such switch.  Returns the
 * previous mode, or -2 for an unknown one.  Needs no device. */
HSV_API int hsv_test_msgs_small(int mode);
/* Launches of hsv_verify_msgs* in this process so far, by form: out[0]
 * two-launch, out[1] quad, out[2] joint, out[3] row, out[4] pair.  HSV_OK. */
HSV_API int hsv_test_msgs_form_counts(uint64_t out[5]);
/* Tests and measurement (tools/committee_msgs_indexed_bench.py): how
 * hsv_committee_verify_msgs_indexed* verifies a round.  -1 = by its size and the
 * committee's table width, the product's rule (the default); 0 = the two
 * launches of the bulk route at every size; 1 = the one-launch latency form at
 * every size -- a call on a compact committee then answers
 * HSV_ERR_INVALID_ARG.  Process-wide; the product library has no such switch.
 * Returns the previous mode, or -2 for an unknown one.  Needs no device. */
HSV_API int hsv_test_cmsg_indexed_form(int mode);
/* What those calls launched in this process so far: out[0] latency-form
 * launches, out[1] rounds of the bulk route, out[2] the items those rounds put
 * on their hit lists (counted on the current device: valid once the caller has
 * synchronised its streams).  HSV_OK, or HSV_ERR_HIP. */
HSV_API int hsv_test_cmsg_indexed_counts(uint64_t out[3]);
/* Measurement only (tools/batch_wire_probe.py): the stages of the generic
 * route of hsv_batches_verify_bincode_device, one after the other on the null
 * stream of the buffers' device, each between two device events: ms_out[0] the
 * parse (count, index and span kernels), [1] the span-mode record kernel, [2]
 * the verification launch over the records and the mask, [3] the verdict
 * kernel.  n_batches >= 1, 1 <= tx_cap <= 2^22; d_results as that call's.
 * Synchronises.  HSV_OK or an error. */
HSV_API int hsv_test_batch_stages(const uint8_t *d_bufs, const uint64_t *d_offsets, size_t n_batches, size_t tx_cap,
                                  void *d_results, float ms_out[4]);
/* Tests: the seed of the census table's slot hash (hsv_census_*) for the
 * calling thread's calls, in the place of the per-process random one, so that
 * a test can choose keys that share a home slot (the hash is keytab_hash of
 * csrc/hsv_keytab.hpp).  The lookup in a `skip` committee keeps the process
 * seed, which its table was built under.  0 restores the process seed.
 * HSV_OK.  Needs no device. */
HSV_API int hsv_test_census_seed(uint64_t seed);
/* Measurement only (tools/seal_bench.py): hsv_seal_transactions_device with
 * its arguments, on the null stream of the buffers' device, with a device event
 * between its stages: ms_out[0] the scan (three launches), [1] the cut wave,
 * [2] the two copy launches, [3] the digest launch (0 when d_digests is NULL).
 * Synchronises.  HSV_OK or that call's error. */
HSV_API int hsv_test_seal_stages(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                                 const uint8_t *d_flags, uint64_t batch_size, int flush, uint8_t *d_out, size_t out_cap,
                                 uint64_t *d_batch_offsets, size_t batches_cap, uint8_t *d_digests, void *d_summary,
                                 float ms_out[4]);

#ifdef __cplusplus
}
#endif

#endif /* HSV_TEST_HOOKS_H_ */
