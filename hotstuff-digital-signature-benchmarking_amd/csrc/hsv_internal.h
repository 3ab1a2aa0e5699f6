// Internal interfaces between the C-ABI layer (hsv_capi.cpp) and the kernels.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// Stream-ordered workspace for a launch on `stream` (current device), freed
// with hipFreeAsync on the same stream.  It comes from a memory pool the
// library owns per device, which keeps its freed blocks (release threshold
// max).  With hipMallocAsync on the default pool (release threshold 0), the
// QC latency kernel of one thread, run while another thread made the
// process's first committee-cache allocations, accepted a forged vote in 8 of
// 16 runs of tests/native/crypto_tests.cpp; with this pool, 0 of 16
// (tools/forgery_debug.sh).  The
// default-pool switch of the measurement build (HSV_WS_POOL=default) left
// the source with that build in round 5; the library always uses its own pool.
hipError_t hsv_ws_malloc(void **p, size_t bytes, hipStream_t stream);
void hsv_ws_trim(void);  // hsv_shutdown: release the pools' free blocks

// The resident latency service (hsv_resident.cpp) from the kernel
// launchers: pause (on = 1) / resume (on = 0) it around a device-wide wait,
// as hsvh::ResidentPause; hsvi_resident_started() is 1 once its block has run
// in this process with the service on -- the persistent point pass then
// leaves one CU's worth of blocks out of its grid, so every block of that
// grid finds a place while the resident block holds its CU.
void hsvi_resident_pause(int on);
int hsvi_resident_started(void);

// Everything declared here is internal: the library is built with
// -fvisibility=hidden, so none of it is exported from libhsv.so (only the
// HSV_API functions of include/hsv.h are).  The test and measurement hooks of
// csrc/hsv_test_hooks.h are exported by libhsv_test.so only; they call the
// hsvi_* functions below.

// Enqueue one verification launch on `stream` (no synchronisation).
int hsvi_num_variants(void);            // id space
int hsvi_variant_list(int *out, int cap);  // ids built into this library; returns their count
int hsvi_variant_available(int variant);
// fault: two device-visible words the caller zeroed before the launch; the
// kernels set fault[0] (an item's final point failed the self-check) and
// fault[1] (a workspace canary changed) -- see hsv_pointpass.hpp report_faults.
// Required (non-null) for the product variants.
hipError_t hsv_launch_verify(int variant, const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                             uint64_t sig_stride, const uint8_t *msg, uint64_t msg_stride,
                             uint32_t n, uint8_t *flags_out, uint32_t *strict_bits,
                             const uint32_t *comb_b, uint32_t *fault, hipStream_t stream);
// The same launch with a caller-provided workspace (ws, ws_cap bytes; the
// library pool is used when it is NULL or too small): a pipeline keeps one per
// stream instead of allocating per launch.  hsv_launch_ws_bytes(variant, n):
// the workspace a launch of n items needs (0 for variants without one).
hipError_t hsv_launch_verify_ws(int variant, const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig,
                                uint64_t sig_stride, const uint8_t *msg, uint64_t msg_stride, uint32_t n,
                                uint8_t *flags_out, uint32_t *strict_bits, const uint32_t *comb_b, uint32_t *fault,
                                void *ws, size_t ws_cap, hipStream_t stream);
size_t hsv_launch_ws_bytes(int variant, uint32_t n);
// Fault injection (tests only; hsv_kernels.hip): the mode of the launches the
// calling thread issues (thread-scoped, so one test's injection never reaches
// another thread's calls); hsvi_set_inject returns the previous mode, or -1.
int hsvi_inject_mode(void);
int hsvi_set_inject(int mode);
// Lattice bound of the comb-path prepass (tests; 0 = default); returns the
// previous bound or -1.
int hsvi_set_lattice_bits(int bits);
// Dealing by column count in the two-launch point pass (tests and A/B runs;
// hsv_kernels.hip), for the calling thread's launches: bit 0 on (the default),
// off = index order; bit 1: keep each launch's class counts, which
// hsvi_deal_counts reports (out[0] >= 67 columns .. out[5] <= 62).
// hsvi_set_deal returns the previous mode, or -1.
int hsvi_set_deal(int mode);
int hsvi_deal_counts(uint32_t out[6]);
// The bound in force, and a fresh canary nonce (odd, never 0): what launch_hp
// hands its kernels, for the launchers of hsv_small.hip and hsv_mempool.hip.
int hsvi_lattice_bits(void);
uint32_t hsvi_next_nonce(void);
// The one-launch latency forms (hsv_small.hip), which hsv_launch_verify* and
// hsv_launch_verify_msgs take at n <= hsv::kPairMax items: quad, joint, row or
// pair by n.  Arguments as the entry point's; comb16: the wide comb of B.
// hsv_small_ws_bytes(n): the workspace the digest launch needs.  force: 0 the
// form by n, 1..kSmallForms that form at any n; *form_id: the form launched.
hipError_t hsv_launch_small(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                            const uint8_t *msg, uint64_t msg_stride, uint32_t n, uint8_t *flags_out,
                            uint32_t *strict_bits, const uint32_t *comb16, uint32_t *fault, void *ws, size_t ws_cap,
                            hipStream_t stream);
size_t hsv_small_ws_bytes(uint32_t n);
hipError_t hsv_launch_small_msgs(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                                 const uint8_t *msgs, const uint64_t *offsets, uint64_t msg_len, uint64_t msg_stride,
                                 uint32_t n, uint8_t *flags_out, uint32_t *strict_bits, const uint32_t *comb16,
                                 uint32_t *fault, int force, int *form_id, hipStream_t stream);
// Row-form field arithmetic against the one-lane form (hsv_committee.hip).
int hsvi_lanesplit_check(const uint32_t *in, uint32_t rows, uint32_t *out);
// The one-lane field, scalar and lattice primitives on raw operands
// (hsv_test_prims.hip, linked into libhsv_test.so only): n records of
// hsv::kPrimFieldIn / kPrimScalarIn words in, kPrimFieldOut / kPrimScalarOut
// words out (hsv_test_prims.hpp), host buffers; 0 or a hipError_t.
int hsvi_test_field_ops(const uint32_t *in, uint32_t n, uint32_t *out);
int hsvi_test_scalar_ops(const uint32_t *in, uint32_t n, uint32_t *out);
// Read-and-clear of two device fault words in one atomic exchange each, on
// `stream`: out (device memory, 2 words) receives the old values.
hipError_t hsv_launch_fault_exchange(uint32_t *words, uint32_t *out, hipStream_t stream);
// digit width of the B comb table a variant reads: 8 (hsv_comb_table_bytes),
// 16 (the wide table, hsv_comb16_table_bytes) or 0 (none); comb_b must be
// that table for such variants
int hsv_variant_needs_comb(int variant);

// Time the v_mad_u64_u32 probe on the current device; MAC/s.
double hsv_launch_mad_peak(int device_cus);

#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
namespace hsv {
// The latency forms at or below this many items, the two-pass kernels above;
// the forms' ids are 1..kSmallForms (quad, joint, row, pair).
constexpr uint32_t kPairMax = 1u << 13;
constexpr int kSmallForms = 4;

// A launcher's workspace: the caller's when it holds `need` bytes (a pipeline
// that keeps one per stream), else a block from the library pool, which
// done() frees on the stream.
class Workspace {
 public:
  Workspace(void *ws_in, size_t ws_cap, size_t need, hipStream_t stream) : stream_(stream) {
    if (ws_in && ws_cap >= need)
      p_ = ws_in;
    else
      e_ = hsv_ws_malloc(&own_, need, stream);
  }
  hipError_t status() const { return e_; }
  uint8_t *get() const { return static_cast<uint8_t *>(own_ ? own_ : p_); }
  // the launcher's result: e, or the free's status when e is hipSuccess
  hipError_t done(hipError_t e) {
    const hipError_t ef = own_ ? hipFreeAsync(own_, stream_) : hipSuccess;
    own_ = nullptr;
    return e != hipSuccess ? e : ef;
  }

 private:
  hipStream_t stream_;
  void *p_ = nullptr, *own_ = nullptr;
  hipError_t e_ = hipSuccess;
};
}  // namespace hsv
#endif

// ---- committee key cache (hsv_committee.hip) -----------------------------
// Request block of the resident committee service (hsv_comb_resident_kernel,
// csrc/hsv_committee.hip), in coherent pinned host memory.  The request's
// payload (QcResidentBody, 144 words) travels in 48 chunks of 16 bytes, each
// {seq, three payload words}: the host writes a chunk's payload words, then
// its seq with a release store (x86 keeps stores in order), so a 16-byte
// read that finds the new seq in a chunk finds that chunk's new payload.  The
// kernel polls all 48 chunks with ONE vector load (one 16-byte read per lane)
// and takes the request once every chunk carries the same new seq -- the
// doorbell and the body in one PCIe round trip, no acquire fence.  It answers
// with two 8-byte stores {seq, flags} and {seq, fault bits}, each a single
// transaction, so the host needs no fence on its side either.
constexpr int kResidentVotes = 4;
struct QcResidentBody {                  // 144 words, offsets fixed (the kernel reads them raw)
  uint32_t m, nkeys, inject, msg_per_vote;  // votes (1..kResidentVotes), members, fault injection, 0/1
  const uint8_t *pks;                    // the committee view's device arrays
  const uint8_t *key_flags;
  const uint32_t *const *key_tables;
  const uint32_t *btable;
  uint32_t key_idx[kResidentVotes];      // word 12
  uint32_t sig[kResidentVotes][16];      // word 16: R || s per vote
  uint32_t msg[kResidentVotes][8];       // word 80: one digest per vote, or the shared digest in msg[0]
  uint32_t pk[kResidentVotes][8];        // word 112: each vote's key encoding (the member's, byte for byte)
};
constexpr int kResidentChunks = 48;      // 3 payload words each
static_assert(sizeof(QcResidentBody) == kResidentChunks * 3 * 4, "48 chunks of three words");
struct alignas(16) QcResidentChunk {
  uint32_t seq, w[3];
};
// answer bits besides the flags: bit 0 / 1 the self-check words of the
// launched form (curve check, canary), bit 2 the request header was refused
constexpr uint32_t kResidentFaultCurve = 1u, kResidentFaultCanary = 2u, kResidentBadRequest = 4u;
struct QcResidentReq {
  uint32_t stop, alive, pad0[14];        // host: stop word; kernel: set while it runs
  QcResidentChunk chunk[64];             // [0, kResidentChunks): the request
  uint64_t answer[2];                    // kernel: seq | flags << 32, seq | fault bits << 32
  uint32_t pad1[12];
};

#ifdef __cplusplus
extern "C" {
#endif
hipError_t hsv_launch_comb_resident(QcResidentReq *d_req, uint64_t idle_ticks, hipStream_t stream);
uint32_t hsv_comb_resident_votes(void);  // votes one request may hold (0: no service in this build)
hipError_t hsv_launch_comb_build(const uint8_t *encs, uint32_t nkeys, uint32_t negate, uint32_t *tables,
                                 uint32_t *tmp, uint8_t *key_flags, hipStream_t stream);
// key_tables[i]: device pointer to key i's comb table; digit_bits: 8
// (hsv_comb_table_bytes each; btable: the narrow comb of B) or 4 (compact,
// hsv_comb4_table_bytes each: the one-lane kernel at every m, done must be
// NULL, and btable is the WIDE comb of B, hsv_comb16_table_bytes)
hipError_t hsv_launch_comb_verify(const uint32_t *key_idx, const uint8_t *sig, uint64_t sig_stride,
                                  const uint8_t *msg, uint64_t msg_stride, uint32_t m, const uint8_t *pks,
                                  const uint8_t *key_flags, uint32_t nkeys, const uint32_t *const *key_tables,
                                  int digit_bits, const uint32_t *btable, uint8_t *flags_out, uint32_t *fault,
                                  uint32_t *done, hipStream_t stream);
// Completion markers of the latency form (done != NULL above, m votes): one
// word per block, set to 1 by the block once its flags are released to the
// system; 0 when m is above the latency form's range (no markers).
uint32_t hsv_comb_marker_blocks(uint32_t m);
uint64_t hsv_comb_table_bytes(void);
uint64_t hsv_comb_tmp_bytes(uint32_t nkeys);
// compact (4-bit digit) key tables, hsv_comb.hpp: nkeys tables contiguous at `tables`
hipError_t hsv_launch_comb4_build(const uint8_t *encs, uint32_t nkeys, uint32_t negate, uint32_t *tables,
                                  uint32_t *tmp, uint8_t *key_flags, hipStream_t stream);
uint64_t hsv_comb4_table_bytes(void);
uint64_t hsv_comb4_tmp_bytes(uint32_t nkeys);
// wide (16-bit digit) comb table of B, hsv_comb.hpp
hipError_t hsv_launch_comb16_build(uint32_t *table, uint32_t *tmp, hipStream_t stream);
uint64_t hsv_comb16_table_bytes(void);
uint64_t hsv_comb16_tmp_bytes(void);
#ifdef __cplusplus
}
#endif

// ---- mempool transactions (hsv_mempool.hip) -------------------------------
#ifdef __cplusplus
extern "C" {
#endif
// 128-byte records pk || R || s || SHA-512(message)[..32] for n transactions
// (offsets[i]..offsets[i+1] of txs, or fixed tx_size when offsets is NULL).
hipError_t hsv_launch_tx_records(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                                 uint8_t *records, hipStream_t stream);
// The same records plus the point pass's scalar prepass on them (one read of
// each transaction): prep = the SoA prepass records (kPrepWords words per
// item, row stride n), items without a short lattice pair appended to fb_list
// through *fb_count.  Used by hsv_launch_verify_tx.
hipError_t hsv_launch_tx_prep(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                              uint8_t *records, uint32_t *prep, uint32_t *fb_count, uint32_t *fb_list,
                              int lat_bits, hipStream_t stream);
// Records, prepass and point pass in ONE persistent launch (hsv_mempool.hip,
// hsv_verify_tx_fused_kernel): grid = the point pass's persistent grid
// (hsv_tx_fused_blocks_per_cu blocks per CU), ctr = the zeroed HcCounters,
// ready = nbatch = ceil(n / 64) zeroed words, vt_ws / canary as
// hsv_verify_hp_kernel's.  n * 128 must stay below 2^32.
int hsv_tx_fused_blocks_per_cu(int device);
hipError_t hsv_launch_tx_fused(uint32_t grid, const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size,
                               uint32_t n, uint8_t *records, uint32_t *rec, void *ctr, uint32_t *fb_list,
                               uint32_t *ready, int lat_bits, uint8_t *flags_out, uint32_t *strict_bits, void *vt_ws,
                               const uint32_t *comb_b, uint32_t *canary, uint32_t nonce, uint32_t inject,
                               uint32_t *fault, hipStream_t stream);
// Transactions end to end: records (128 B per item, caller's buffer) and
// verification, fused as above for large batches of the product variants;
// otherwise hsv_launch_tx_records + hsv_launch_verify.
hipError_t hsv_launch_verify_tx(int variant, const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size,
                                uint32_t n, uint8_t *records, uint8_t *flags_out, uint32_t *strict_bits,
                                const uint32_t *comb_b, uint32_t *fault, hipStream_t stream);
// One round (n <= 2^22) of hsv_committee_verify_transactions*: the route
// kernel (records, key lookup in keytab / keymask / seed over the committee's
// pks, hit and miss lists, the misses' prepass), the comb pass over the hit
// list (key_flags, key_tables, btable: the narrow comb of B) and the generic
// pass over the miss list (comb16: the wide comb); digit_bits (8 or 4): the
// width of key_tables, which picks the comb pass (the compact one reads comb16
// for [s]B, not btable).  Every flag byte and strict
// word of the round is written; fault as hsv_launch_verify.  totals (may be
// NULL): three 64-bit device words that receive += {hits, misses, fallback
// items}.  nkeys == 0: every transaction is a miss, the committee arrays may
// be NULL.
hipError_t hsv_launch_committee_tx(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                                   const uint32_t *keytab, uint32_t keymask, uint64_t seed, const uint8_t *pks,
                                   const uint8_t *key_flags, uint32_t nkeys, const uint32_t *const *key_tables,
                                   int digit_bits, const uint32_t *btable, const uint32_t *comb16, uint8_t *flags_out,
                                   uint32_t *strict_bits, uint32_t *fault, uint64_t *totals, hipStream_t stream);
// One signer census (hsv_census_*; hsv_census.hip) on `stream`: the count
// kernel and the gather kernel over a zeroed workspace of 8 bytes per slot
// from the library pool.  mode 0: n keys at in + i * stride (both multiples of
// 16); 1: transactions in[offsets[i], offsets[i + 1]); 2: transactions of
// `stride` bytes; in at any alignment for 1 and 2.  slots: a power of two in
// [16, 2^22]; seed: the slot hash's.  keytab / keymask / keyseed / pks / nkeys:
// the committee whose members are left out (nkeys == 0: none, the arrays may
// be NULL).  Every entry of keys_out (32 * slots bytes, 16-byte aligned) and
// counts_out (slots words) and the 48-byte summary are written.
hipError_t hsv_launch_census(int mode, const uint8_t *in, const uint64_t *offsets, uint64_t stride, uint32_t n,
                             uint32_t slots, uint64_t seed, const uint32_t *keytab, uint32_t keymask,
                             uint64_t keyseed, const uint8_t *pks, uint32_t nkeys, uint8_t *keys_out,
                             uint32_t *counts_out, void *summary, hipStream_t stream);
// The slot-hash seed of the calling thread's census calls (hsv_test_census_seed,
// hsv_census_api.cpp): 0 restores the per-process seed.
void hsvi_set_census_seed(uint64_t seed);
// One seal (hsv_seal_transactions*; hsv_seal.hip) on `stream`: n transactions
// addressed as above (offsets, or fixed tx_size when it is NULL; any
// alignment), kept when flags[i] has HSV_STRICT_OK (flags == NULL: all), cut by
// the greedy rule at batch_size and laid down as MempoolMessage::Batch messages
// in out[0, out_cap).  batch_offsets: batches_cap + 1 entries, all written;
// digests (optional): 32 bytes per batch; summary: a hsv_seal_summary, 8-byte
// aligned.  Workspace: 20 bytes per transaction and 4 per batch of
// min(batches_cap, n), a block of its own from the library pool.  marks
// (optional, measurements): five events recorded before the scan, the cut, the
// copy and the digest launches and after the last.
hipError_t hsv_launch_seal(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size, uint32_t n,
                           const uint8_t *flags, uint64_t batch_size, int flush, uint8_t *out, uint64_t out_cap,
                           uint64_t *batch_offsets, uint64_t batches_cap, uint8_t *digests, void *summary,
                           hipEvent_t *marks, hipStream_t stream);
// Ed25519 over messages of any length (hsv_verify_msgs*): k = SHA-512(R || A
// || M) over the whole message.  Message i is msgs[offsets[i], offsets[i+1])
// (offsets != NULL; a decreasing pair gives flags 0) or msg_len bytes at
// msgs + i * msg_stride; msgs at any alignment, pk / sig and their strides
// multiples of 16.  At <= 2^13 items one launch on `stream`: the message
// instantiation of the small form of that size (quad, joint, row or pair, as
// hsv_launch_verify), whose prepass wave hashes the block's messages.  Above,
// two launches: hsv_launch_msg_prep
// (hsv_msgs.hip: one lane per item hashes its message and writes the SoA
// prepass record, with k mod l in the b words of a fallback item), then the
// point pass, which never reads a message.  comb16: the wide comb of B;
// workspace, fault words and canaries as hsv_launch_verify.
hipError_t hsv_launch_verify_msgs(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                                  const uint8_t *msgs, const uint64_t *offsets, uint64_t msg_len,
                                  uint64_t msg_stride, uint32_t n, uint8_t *flags_out, uint32_t *strict_bits,
                                  const uint32_t *comb16, uint32_t *fault, hipStream_t stream);
// The route of hsv_launch_verify_msgs at <= 2^13 items (hsv_test_msgs_small):
// -1 a small form chosen by n (default), 0 two launches as above 2^13 items,
// 1..4 quad, joint, row, pair at every such n.  Returns the
// previous mode, or -2 for an unknown one.  hsvi_msgs_form_counts: launches so
// far by form -- two-launch, quad, joint, row, pair.  Neither needs a device.
int hsvi_set_msgs_small(int mode);
int hsvi_msgs_form_counts(uint64_t out[5]);
hipError_t hsv_launch_msg_prep(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                               const uint8_t *msgs, const uint64_t *offsets, uint64_t msg_len, uint64_t msg_stride,
                               uint32_t n, uint32_t *prep, void *ctr, uint32_t *fb_list, uint32_t *cls_list,
                               int lat_bits, hipStream_t stream);
// One round (n <= 2^22) of hsv_committee_verify_msgs* (hsv_committee_msgs.hip):
// the messages of hsv_launch_verify_msgs with the committee arguments of
// hsv_launch_committee_tx.  Three launches on `stream`: the route kernel (the
// message hash, the key lookup, hit and miss lists, k mod l for the hits, the
// misses' prepass), the comb pass over the hit list and the generic pass over
// the miss list; both read pk / sig in place and never a message byte.  Every
// flag byte and strict word of the round is written (a decreasing pair of
// offsets: flags 0); fault, totals and nkeys == 0 as hsv_launch_committee_tx.
hipError_t hsv_launch_committee_msgs(const uint8_t *pk, uint64_t pk_stride, const uint8_t *sig, uint64_t sig_stride,
                                     const uint8_t *msgs, const uint64_t *offsets, uint64_t msg_len,
                                     uint64_t msg_stride, uint32_t n, const uint32_t *keytab, uint32_t keymask,
                                     uint64_t seed, const uint8_t *pks, const uint8_t *key_flags, uint32_t nkeys,
                                     const uint32_t *const *key_tables, int digit_bits, const uint32_t *btable,
                                     const uint32_t *comb16, uint8_t *flags_out, uint32_t *strict_bits,
                                     uint32_t *fault, uint64_t *totals, hipStream_t stream);
// One round (n <= 2^22) of hsv_committee_verify_msgs_indexed* (hsv_committee_msgs.hip):
// the messages of hsv_launch_verify_msgs, item i signed by member key_idx[i] (an
// index >= nkeys: flags 0, as a decreasing pair of offsets).  At n <= 2^12 with
// 8-bit tables one launch of the latency form (hsv_cmsg_quad_kernel), else a
// memset of the counters and two launches (hsv_cmsg_index_kernel and the comb
// pass of hsv_launch_committee_msgs).  Every flag byte is written; no strict
// words; fault as hsv_launch_comb_verify; btable / comb16: the narrow and the
// wide comb of B.
hipError_t hsv_launch_committee_msgs_indexed(const uint32_t *key_idx, const uint8_t *sig, uint64_t sig_stride,
                                             const uint8_t *msgs, const uint64_t *offsets, uint64_t msg_len,
                                             uint64_t msg_stride, uint32_t n, const uint8_t *pks,
                                             const uint8_t *key_flags, uint32_t nkeys,
                                             const uint32_t *const *key_tables, int digit_bits, const uint32_t *btable,
                                             const uint32_t *comb16, uint8_t *flags_out, uint32_t *fault,
                                             hipStream_t stream);
// Its route (hsv_test_cmsg_indexed_form): -1 by n and the table width
// (default), 0 the two launches at every n, 1 the latency form at every n (8-bit
// tables only).  Returns the previous mode, or -2 for an unknown one.
// hsvi_cmsg_indexed_counts: {latency-form launches, two-launch rounds} of the
// process so far and the items those rounds put on their hit lists on the
// current device (valid once the caller's streams are synchronised).
int hsvi_set_cmsg_indexed_form(int mode);
int hsvi_cmsg_indexed_form(void);
int hsvi_cmsg_indexed_counts(uint64_t out[3]);
// flags 0 (and STRICT_OK bit cleared) for transactions shorter than 96 bytes
hipError_t hsv_launch_tx_mask(const uint64_t *offsets, uint32_t n, uint8_t *flags, uint32_t *strict_bits,
                              hipStream_t stream);
// Span-table addressing (the serialized batches of hsv_batches_verify_bincode*):
// transaction i is txs[spans[2i], spans[2i+1]), pairs of any order and distance;
// a pair shorter than 96 bytes or decreasing is a malformed transaction, as
// above.  hsv_launch_tx_records, hsv_launch_tx_mask and hsv_launch_committee_tx
// over such a table: the span instantiations of the same kernels.
hipError_t hsv_launch_tx_records_spans(const uint8_t *txs, const uint64_t *spans, uint32_t n, uint8_t *records,
                                       hipStream_t stream);
hipError_t hsv_launch_tx_mask_spans(const uint64_t *spans, uint32_t n, uint8_t *flags, uint32_t *strict_bits,
                                    hipStream_t stream);
hipError_t hsv_launch_committee_tx_spans(const uint8_t *txs, const uint64_t *spans, uint32_t n,
                                         const uint32_t *keytab, uint32_t keymask, uint64_t seed, const uint8_t *pks,
                                         const uint8_t *key_flags, uint32_t nkeys, const uint32_t *const *key_tables,
                                         int digit_bits, const uint32_t *btable, const uint32_t *comb16,
                                         uint8_t *flags_out, uint32_t *strict_bits, uint32_t *fault, uint64_t *totals,
                                         hipStream_t stream);

// ---- serialized mempool batches (hsv_batchwire.hip) -------------------------
// The device-side parse of n_batches bincode MempoolMessage::Batch messages,
// batch b = bufs[offsets[b], offsets[b+1]) at any alignment (hsv_batchscan.hpp).
// Four launches on `stream`, all sized by n_batches:
//   count   one wave per batch: status[b] (kBatchOk / kBatchParse) and count[b]
//           (0 for a malformed batch);
//   index   first[b] = the counts before b, first[n_batches] = their sum; a batch
//           with first[b] + count[b] > tx_cap becomes kBatchOverflow;
//   spans   one wave per kBatchOk batch writes its transactions' span pairs,
//           relative to bufs, at spans[2 * first[b] ..] (the caller zeroed
//           spans[0 .. 2 * tx_cap), so every other entry reads as an empty span).
// hsv_launch_batch_reduce (after the verification): results[b] = {status, index,
// n_tx, first} from status / count / first and the flags of its transactions
// (kBatchTx and the lowest index whose flags lack HSV_STRICT_OK).  results is a
// hsv_batch_result array (include/hsv.h).
hipError_t hsv_launch_batch_scan(const uint8_t *bufs, const uint64_t *offsets, uint32_t n_batches, uint64_t tx_cap,
                                 uint32_t *status, uint64_t *count, uint64_t *first, uint64_t *spans,
                                 hipStream_t stream);
hipError_t hsv_launch_batch_reduce(const uint32_t *status, const uint64_t *count, const uint64_t *first,
                                   const uint8_t *flags, uint32_t n_batches, void *results, hipStream_t stream);

// ---- the benchmark's sample transactions (hsv_samples.hip) -------------------
// The sample index of the same batches (hsv_batches_samples_bincode_device): a
// memset of the span table, hsv_launch_batch_scan and four launches on `stream`.
// index: n_batches hsv_batch_samples, 8-byte aligned; ids: ids_cap 8-byte words,
// of which only those below the call's sample count are written.  Workspace:
// 20 bytes per transaction of tx_cap (<= 2^32 - 1) and 20 per batch, a block of
// its own from the library pool.
hipError_t hsv_launch_batch_samples(const uint8_t *bufs, const uint64_t *offsets, uint32_t n_batches, uint64_t tx_cap,
                                    void *index, uint64_t *ids, uint64_t ids_cap, hipStream_t stream);
// The client's transactions (hsv_client_bursts_device): one launch, bytes
// [0, tx_size - trailer) of n <= 2^32 - 1 transactions at txs + i * tx_size, any
// alignment; burst > 0 and tx_size - trailer >= 9.
hipError_t hsv_launch_client_bursts(uint8_t *txs, uint64_t tx_size, uint64_t trailer, uint64_t counter0,
                                    uint64_t burst, uint64_t r0, uint64_t n, hipStream_t stream);
#ifdef __cplusplus
}
#endif

// ---- batch signer (hsv_signer.hip) -----------------------------------------
#ifdef __cplusplus
extern "C" {
#endif
// One launch each, at most 2^22 items, enqueued on `stream` (no
// synchronisation); comb16: the wide comb of B; fault: as hsv_launch_verify
// (fault[0] only).  seeds (n * 32 B), keys (96-byte records a | prefix | pk)
// and sig / sig_stride are 16-byte aligned; msg may have any alignment.
hipError_t hsv_launch_keygen(const uint8_t *seeds, uint32_t n, uint8_t *keys, const uint32_t *comb16,
                             uint32_t *fault, hipStream_t stream);
// item i: key key_idx[i] (NULL: key i; an index >= nkeys writes a zero
// signature), message msg + i * msg_stride of msg_len bytes
hipError_t hsv_launch_sign(const uint8_t *keys, uint32_t nkeys, const uint32_t *key_idx, const uint8_t *msg,
                           uint64_t msg_len, uint64_t msg_stride, uint32_t m, uint8_t *sig, uint64_t sig_stride,
                           const uint32_t *comb16, uint32_t *fault, hipStream_t stream);
// Mempool transactions signed in place (hsv_txsign.hpp): pk || R || s into the
// last 96 bytes of transaction i (offsets[i]..offsets[i+1] of txs, or fixed
// tx_size when offsets is NULL; any alignment), over SHA-512(message)[..32].
// Two launches: hsv_launch_tx_digest (hsv_txsign.hip; dig: m * 32 B, 16-byte
// aligned, status: m words) and the signing launch.  A transaction shorter
// than 96 bytes or with decreasing offsets is left untouched.
hipError_t hsv_launch_tx_sign(const uint8_t *keys, uint32_t nkeys, const uint32_t *key_idx, uint8_t *txs,
                              const uint64_t *offsets, uint64_t tx_size, uint32_t m, const uint32_t *comb16,
                              uint32_t *fault, hipStream_t stream);
hipError_t hsv_launch_tx_digest(const uint8_t *txs, const uint64_t *offsets, uint64_t tx_size,
                                const uint32_t *key_idx, uint32_t nkeys, uint32_t n, uint8_t *dig, uint32_t *status,
                                hipStream_t stream);
// Items per launch of hsv_signer_sign_transactions* (tests; 0 = the default
// 2^22); previous value.
size_t hsvi_set_tx_sign_chunk(size_t items);
// Items per lane (G) of the following signer launches: one of the built
// values (1, 2, 4, 8, 16), 0 = the product's; previous value or -1.
int hsvi_set_signer_group(int g);
int hsvi_signer_group(void);  // the G in force
// Whole messages of any lengths signed into 64-byte slots (hsv_msgsign.hpp):
// message i = msgs[offsets[i], offsets[i+1]) or msg_len bytes at msgs + i *
// msg_stride, any alignment; R || s to sig + i * sig_stride (multiples of 16).
// Three launches on `stream` (hsv_msgsign.hip): nonce, point, response.  A key
// index out of range or a decreasing pair of offsets gives 64 zero bytes.
hipError_t hsv_launch_msg_sign(const uint8_t *keys, uint32_t nkeys, const uint32_t *key_idx, const uint8_t *msgs,
                               const uint64_t *offsets, uint64_t msg_len, uint64_t msg_stride, uint32_t m,
                               uint8_t *sig, uint64_t sig_stride, const uint32_t *comb16, uint32_t *fault,
                               hipStream_t stream);
// Items per round of hsv_signer_sign_msgs* (tests; 0 = the default 2^22);
// previous value.
size_t hsvi_set_msg_sign_chunk(size_t items);
#ifdef __cplusplus
}
#endif

// ---- error reporting shared by the C-ABI translation units -----------------
#ifdef __cplusplus
extern "C" {
#endif
// sets hsv_last_error() on the calling thread; returns code
int hsvi_set_error(int code, const char *msg);
// test hooks of hsv_capi.cpp (exported as hsv_set_* by libhsv_test.so only)
int hsvi_set_virtual_shards(int k);
int hsvi_set_pipe_nocopy(int on);  // hsv_test_pipe_nocopy (libhsv_test.so only)
int hsvi_set_pipe_schedule(const uint64_t *sizes, int count);  // hsv_test_pipe_schedule
int hsvi_set_variant(int v);
#ifdef __cplusplus
}
#endif
