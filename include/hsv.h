/*
 * hsv.h -- C ABI of the MI355X Ed25519 batch verifier (libhsv.so).
 *
 * Drop-in boundary for the reference's hot path, the `crypto` crate of
 * mwaurawakati/hotstuff-digital-signature-benchmarking:
 *
 *   crypto::Signature::verify        crypto/src/lib.rs:204-208  -> hsv_verify_strict
 *   crypto::Signature::verify_batch  crypto/src/lib.rs:210-223  -> hsv_verify_batch
 *                                                                   hsv_verify_batch_packed
 *   (batched strict API)                     -> hsv_verify
 *   (the same over whole messages of any length, RFC 8032 5.1.7) -> hsv_verify_msgs,
 *                                                                   hsv_verify_msgs_device,
 *                                                                   hsv_committee_verify_msgs*,
 *                                                                   hsv_committee_verify_msgs_indexed*
 *   crypto::Signature::new           crypto/src/lib.rs:185-191  -> hsv_sign, hsv_signer_sign*
 *   crypto::generate_keypair         crypto/src/lib.rs:167-175  -> hsv_public_key, hsv_signer_create
 *   mempool transaction check  mempool/src/batch_maker.rs:79-85 -> hsv_verify_transactions*,
 *                                                                   hsv_committee_verify_transactions*
 *   QC / TC signature checks from wire bytes
 *                        consensus/src/messages.rs:180-198, 290-315 -> hsv_qc_verify_bincode,
 *                                                                   hsv_tc_verify_bincode
 *   Block / Timeout / Vote signature checks, one call each
 *                        consensus/src/messages.rs:55-76, 250-265, 136-146 -> hsv_proposal_verify,
 *                                                                   hsv_block_verify_bincode,
 *                                                                   hsv_blocks_verify_bincode,
 *                                                                   hsv_timeout_verify_bincode,
 *                                                                   hsv_vote_verify_bincode
 *   Core::make_vote's payload check from the stored batch bytes
 *                        consensus/src/core.rs:113-142          -> hsv_batch_verify_bincode,
 *                                                                   hsv_batches_verify_bincode*
 *   BatchMaker::run / seal and Processor's store key
 *                        mempool/src/batch_maker.rs:78-131, processor.rs:30 -> hsv_seal_transactions*
 *
 * Plain pointers and sizes only.  All inputs are borrowed for the duration of
 * the call; the library never retains a caller pointer.  Every entry point is
 * thread-safe (the reference calls verify from tokio worker threads,
 * node/src/main.rs:16).  A return value < 0 is an infrastructure error (no
 * GPU, HIP failure, bad argument) and NEVER encodes a signature rejection;
 * there is no CPU fallback for verification -- callers decide what to do.
 *
 * Byte layouts are the reference's: PublicKey = 32 bytes (crypto/src/lib.rs:66),
 * Signature = part1 (R, 32 B) || part2 (s, 32 B) as produced by flatten()
 * (lib.rs:197-202), Digest = 32 bytes (lib.rs:22).
 */
#ifndef HSV_H_
#define HSV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every function below is exported from libhsv.so; nothing else is (the
 * library is built with -fvisibility=hidden and a version script, and
 * tests/test_capi.py checks that its dynamic symbols are exactly these). */
#if defined(__GNUC__) || defined(__clang__)
#define HSV_API __attribute__((visibility("default")))
#else
#define HSV_API
#endif

/* ---- per-signature flag byte (hsv_verify / hsv_verify_device) ---------- */
#define HSV_STRICT_OK 0x01u /* == ed25519-dalek PublicKey::verify_strict Ok   */
#define HSV_EQ_OK 0x02u     /* PARSE_OK and [s]B == R + [k]A (cofactorless)    */
#define HSV_PARSE_OK 0x04u  /* S_OK and A_OK and R_OK                          */
#define HSV_SMALL_A 0x08u   /* A decodes and [8]A == O                         */
#define HSV_SMALL_R 0x10u   /* R decodes and [8]R == O                         */
#define HSV_S_OK 0x20u      /* s < l (canonical)                               */
#define HSV_A_OK 0x40u      /* A decompresses                                  */
#define HSV_R_OK 0x80u      /* R decompresses                                  */
/* verify_batch item accepted  <=>  (flags & (HSV_PARSE_OK|HSV_EQ_OK)) == both  */

/* ---- return codes ------------------------------------------------------- */
#define HSV_OK 0
#define HSV_ERR_NO_DEVICE (-1)
#define HSV_ERR_HIP (-2)
#define HSV_ERR_INVALID_ARG (-3)
#define HSV_ERR_ALLOC (-4)
#define HSV_ERR_ALIGN (-5)
#define HSV_ERR_PARSE (-6) /* malformed wire bytes (hsv_*_bincode) */
/* The device self-checks failed: an item's final point was not a curve point
 * (corrupted table memory, workspace or HBM) or a workspace canary changed.
 * The launch's flags are not a verdict; callers treat it like any other
 * infrastructure error (a GPU failure is never a silent reject). */
#define HSV_ERR_DEVICE_FAULT (-7)

/* ---- lifecycle and device binding -------------------------------------- */
/* Optional: contexts are created lazily on first use.
 *   device >= 0  binds the process to that GPU: every host-buffer call
 *                (hsv_verify*, hsv_verify_batch*, transactions, certificates,
 *                committee creation) runs on it.  This is the one-process-
 *                per-GPU deployment (the reference runs one node per process,
 *                node/src/main.rs:16); returns 1.
 *   device == -1 every visible GPU: host batches of >= 2^16 items are
 *                sharded across them by contiguous range (one host thread
 *                each, flags gathered into the caller's buffer); smaller
 *                batches run on the calling thread's current HIP device.
 *                Returns the number of devices.
 * Without a call, the environment variable HSV_DEVICE (same values) applies,
 * else -1.  Each device keeps a pool of HSV_SLOTS (default 4) staging slots,
 * so concurrent calls (several tokio workers) do not queue behind one buffer.
 * A slot's streams (and the device API's side streams) are created at the
 * greatest stream priority, so they draw on hardware queues of their own
 * instead of sharing the application's.
 * Device-resident calls (hsv_*_device*) always run on the device that owns
 * their input pointers; a stream of another device is an error.
 * Returns < 0 for a device index out of range. */
HSV_API int hsv_init(int device);
/* The binding in effect: a device index, or -1 for "every device". */
HSV_API int hsv_bound_device(void);
/* Release all device buffers, streams and pinned staging memory. */
HSV_API void hsv_shutdown(void);
/* Number of visible HIP devices (0 when none). */
HSV_API int hsv_device_count(void);
/* Human-readable description of the last error on the calling thread. */
HSV_API const char *hsv_last_error(void);
/* Library version string, "hsv MAJOR.MINOR.PATCH (gfx950)".  0.3.0: the
 * three device-API calls (hsv_verify_device_bits, hsv_committee_verify_device,
 * hsv_verify_transactions_device) take the optional d_fault argument before
 * `stream`; a caller built against 0.2.x headers must be rebuilt (check
 * HSV_ABI_VERSION against hsv_abi_version() at startup).  Entry points added
 * since (the last: the benchmark's sample transactions,
 * hsv_batch_samples_bincode* and hsv_client_bursts*) change no
 * existing signature
 * and leave both the version and HSV_ABI_VERSION as they are. */
#define HSV_ABI_VERSION 3
HSV_API const char *hsv_version(void);
/* The ABI generation this library implements (HSV_ABI_VERSION of its header). */
HSV_API int hsv_abi_version(void);

/* ---- verification, host buffers (synchronous) --------------------------- */
/* Verify n independent triples.  pk: n*32 B, sig: n*64 B (R||s),
 * msg: n*32 B when msg_stride == 32, or one shared 32-B digest when
 * msg_stride == 0 (the QC case).  flags_out: n bytes (HSV_* bits above).
 * n == 0 is valid and does nothing. */
HSV_API int hsv_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg, size_t msg_stride,
               size_t n, uint8_t *flags_out);

/* crypto::Signature::verify (crypto/src/lib.rs:204-208):
 * returns 1 = Ok, 0 = Err(CryptoError), < 0 = infrastructure error. */
HSV_API int hsv_verify_strict(const uint8_t digest[32], const uint8_t pk[32], const uint8_t sig[64]);

/* crypto::Signature::verify_batch (crypto/src/lib.rs:210-223), votes as
 * parallel arrays pk[n*32], sig[n*64] over one shared digest:
 * returns 1 = Ok, 0 = Err, < 0 = infrastructure error.  n == 0 -> 1 (Ok). */
HSV_API int hsv_verify_batch(const uint8_t digest[32], const uint8_t *pk, const uint8_t *sig, size_t n);

/* Same, votes packed as n 96-byte records pk(32)||R(32)||s(32). */
HSV_API int hsv_verify_batch_packed(const uint8_t digest[32], const uint8_t *votes, size_t n);

/* Automatic committee cache behind hsv_verify_batch[_packed] (on by default;
 * env HSV_AUTO_COMMITTEE=0 turns it off).  Consensus keys repeat every round
 * (consensus/src/config.rs Committee): a key seen in two batches is queued,
 * and a background thread builds its comb table on a stream of its own and
 * appends it to the cache (at most 8192 keys, 384 KiB each; batches of more
 * than 8192 votes are never cached).  A verify call never waits for a build:
 * batches whose keys are all cached take the committee kernels, all others
 * the generic kernels, with identical flags either way.  A failed build is a
 * cache miss, never an error; when a full cache keeps missing (a new epoch)
 * it is dropped and relearnt.  Strict batches of <= 4096 cached keys
 * (hsv_verify, hsv_verify_strict) use it too.  enable = 0 also drops it. */
HSV_API int hsv_set_auto_committee(int enable);
/* Number of keys in the automatic cache (0 when none). */
HSV_API size_t hsv_auto_committee_size(void);
/* Wait up to timeout_ms for a pending cache build to be published:
 * 1 = no build in flight, 0 = timed out.  (Warm-up and tests.) */
HSV_API int hsv_auto_committee_wait(int timeout_ms);
/* Number of cached-path launches whose device self-check failed since the
 * process started.  Such a call is answered by the generic kernels instead,
 * and the cache is dropped and relearnt (its tables are no longer trusted). */
HSV_API uint64_t hsv_auto_committee_faults(void);

/* Resident latency service (on by default; env HSV_QC_RESIDENT=0 turns it
 * off).  Calls of 1-4 votes whose keys are all in a committee cache
 * (hsv_verify_strict, small hsv_verify / hsv_verify_batch*, the explicit
 * committee) are posted to one block of the latency kernel that stays on a CU
 * of the home device, instead of a launch each: one verify_strict costs
 * about 0.034 ms instead of 0.039 ms.  The block leaves after
 * HSV_QC_RESIDENT_IDLE_MS (default 50) without a request and is relaunched by
 * the next one; while it runs it holds one CU, so a device-wide
 * synchronisation of the application (hipDeviceSynchronize) waits at most
 * that idle time.  The library pauses it around its own frees, and its
 * persistent large-batch grids leave one CU free once it has run.  Verdicts
 * never depend on it: a request it does not answer goes to the launch path.
 * mode 1 = on, 0 = off (the block stops before the call returns).  Returns
 * the previous mode. */
HSV_API int hsv_set_resident_service(int mode);

/* ---- verification, device-resident buffers (stream-ordered, async) ------ */
/* Inputs already in HBM (of any device: the call runs on the device owning
 * d_pk, and `stream` must belong to it).  Record i reads
 * pk + i*pk_stride (32 B), sig + i*sig_stride (64 B), msg + i*msg_stride
 * (32 B; msg_stride may be 0).  Pointers and strides must be multiples of 16.
 * Writes n flag bytes to d_flags.  stream: a hipStream_t (NULL = default).
 * Does not synchronise.  Batches above 2^22 items run as 2^22-item launches
 * alternating over `stream` and a library stream forked from and joined back
 * into `stream` by events: the call stays ordered on `stream` as one unit. */
HSV_API int hsv_verify_device(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig,
                      size_t sig_stride, const uint8_t *d_msg, size_t msg_stride, size_t n,
                      uint8_t *d_flags, void *stream);

/* As hsv_verify_device, additionally packing STRICT_OK bits into
 * d_strict_bits[(n+31)/32] (bit i of word i/32 = item i).  Either output
 * pointer may be NULL.
 * d_fault (optional): two device words owned by the caller.  The library
 * zeroes them on `stream` before the call's launches and the kernels set
 * d_fault[0] (a final point failed the curve self-check) and d_fault[1] (a
 * workspace canary changed, i.e. memory the launch wrote was overwritten).
 * Read them after synchronising `stream`: both zero means the flags are a
 * verdict, anything else is an infrastructure error (HSV_ERR_DEVICE_FAULT on
 * the host-buffer calls).  The words belong to this call alone, so concurrent
 * callers on other streams never see or clear each other's faults.  With
 * d_fault NULL the launches report into the per-device word read by
 * hsv_device_faults. */
HSV_API int hsv_verify_device_bits(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig,
                           size_t sig_stride, const uint8_t *d_msg, size_t msg_stride, size_t n,
                           uint8_t *d_flags, uint32_t *d_strict_bits, uint32_t *d_fault, void *stream);

/* ---- verification over messages of any length ----------------------------- */
/* Ed25519 over messages of any length: flags as hsv_verify, with
 * k = SHA-512(R || A || M) over the whole message M (RFC 8032 5.1.7, dalek
 * verify_strict's rules for everything else).  This is the verifying half of
 * hsv_signer_sign* and hsv_sign_many; a mempool transaction
 * (hsv_verify_transactions*) is a different scheme, signed over
 * SHA-512(message)[..32].
 * offsets != NULL: message i is msgs[offsets[i] .. offsets[i+1]) (n+1 entries).
 * offsets == NULL: message i is msg_len bytes at msgs + i*msg_stride
 *                  (msg_stride 0: one shared message).
 * A message may be empty.  msgs may have any alignment.
 * Host form: synchronous, on the bound or current device; n == 0 does
 * nothing.  Decreasing offsets, or a NULL msgs when any message is non-empty,
 * return HSV_ERR_INVALID_ARG; a failed device self-check returns
 * HSV_ERR_DEVICE_FAULT.  There is no CPU fallback (HSV_ERR_NO_DEVICE without a
 * GPU).  Plain staged copies on one device: this call is neither pipelined
 * nor sharded across GPUs. */
HSV_API int hsv_verify_msgs(const uint8_t *pk, const uint8_t *sig, const uint8_t *msgs,
                            const uint64_t *offsets, size_t msg_len, size_t msg_stride,
                            size_t n, uint8_t *flags_out);
/* Device-resident, stream-ordered form; never synchronises.  d_pk, d_sig and
 * their strides must be multiples of 16 (HSV_ERR_ALIGN), as in
 * hsv_verify_device; d_msgs, msg_stride and the offsets (relative to d_msgs)
 * may have any alignment.  d_flags, d_strict_bits and d_fault as
 * hsv_verify_device_bits (either output may be NULL, not both).  An item whose
 * offsets decrease gets flags 0; its neighbours are unaffected.  Batches above
 * 2^22 items run as 2^22-item launches, in order on `stream`.  A launch of at
 * most 2^13 items (a vote, a certificate; the tail of a larger batch) is one
 * kernel of the latency forms of hsv_verify_device, whose prepass wave hashes
 * the whole messages: 0.11 - 0.15 ms up to 768 items of up to 416 bytes on an
 * MI355X.  Larger launches are two kernels (message prepass, point pass).
 * The host form takes the same routes. */
HSV_API int hsv_verify_msgs_device(const uint8_t *d_pk, size_t pk_stride, const uint8_t *d_sig,
                                   size_t sig_stride, const uint8_t *d_msgs, const uint64_t *d_offsets,
                                   size_t msg_len, size_t msg_stride, size_t n, uint8_t *d_flags,
                                   uint32_t *d_strict_bits, uint32_t *d_fault, void *stream);

/* Self-check results of the device-resident calls on `device` (-1: every
 * device) that ran without a d_fault of their own, since the last clear.
 * Read after synchronising the streams those calls ran on.  Returns 0 (no
 * fault), the fault bits (1: curve check, 2: canary), or < 0 on error.
 * clear != 0 reads and resets the word in one atomic exchange on the device,
 * so a fault recorded by a launch still running on another stream is either
 * returned now or kept for the next read, never lost.  Host-buffer calls
 * report their own launches' faults as HSV_ERR_DEVICE_FAULT instead. */
HSV_API int hsv_device_faults(int device, int clear);

/* ---- committee key cache --------------------------- */
/* Consensus keys are fixed per epoch (consensus/src/config.rs Committee).  A
 * committee holds, in HBM of the device bound at creation (hsv_init), a 384 KiB
 * fixed-base comb table of -A per key; verifying a vote by a member then costs
 * 64 mixed additions and no doublings.  Flags are identical to hsv_verify's
 * (undecodable or small-order keys are accepted as members and reported
 * through HSV_A_OK / HSV_SMALL_A exactly as the generic path does). */
typedef struct hsv_committee hsv_committee;
/* Build tables for n public keys (n*32 B). */
HSV_API int hsv_committee_create(const uint8_t *pks, size_t n, hsv_committee **out);
/* The same with the table width chosen: digit_bits 8 (hsv_committee_create's
 * tables: 32 positions x 128 entries, 384 KiB per key) or 4 (compact: 64
 * positions x 8 entries, 48 KiB per key, so 2^20 keys take 48 GiB instead of
 * 384 GiB and 100 000 keys 4.6 GiB instead of 36.6 GiB); any other value is
 * HSV_ERR_INVALID_ARG.  A compact committee is accepted by every call that
 * takes an hsv_committee, with the flags, strict bits, fault words, chunking,
 * alignment rules and error codes of a full one over the same keys; it pays
 * 80 mixed additions per signature instead of 64.  It has no latency form:
 * every batch size runs one item per lane -- no zero-copy form, no
 * 16-lanes-per-vote kernel, no resident service -- so small batches (a QC)
 * belong to a full committee.  Both kinds may exist side by side, over the
 * same keys or different ones.
 * When to use it (profiles/committee_compact_bench_2p20.json: 2^20
 * device-resident items, a uniformly random member per item, every ratio
 * within one run): with every signer a member a compact committee runs at
 * 2.22 - 2.31 x the rate of the generic call (hsv_verify_msgs_device on
 * 32-byte messages, hsv_verify_transactions_device on 512-byte transactions)
 * at K = 1000, 1.98 - 2.02 x at 2^14 and 1.65 - 1.71 x at 2^17 keys (6 GiB of
 * tables, far beyond the Infinity Cache: 0.71 - 0.74 of its own rate at K =
 * 1000), and at 0.89 - 0.91 x the rate of a full committee at K = 1000; with
 * half of the signers members it takes 0.75 - 0.82 of the generic call's
 * time.  Use it where the full tables do not fit; where they do, the full
 * committee is faster and has the latency forms.  2^17 keys build in 0.18 -
 * 0.36 s. */
#define HSV_COMMITTEE_DIGITS_FULL 8    /* 384 KiB per key */
#define HSV_COMMITTEE_DIGITS_COMPACT 4 /* 48 KiB per key */
HSV_API int hsv_committee_create_ex(const uint8_t *pks, size_t n, int digit_bits, hsv_committee **out);
/* 8 or 4; 0 for NULL. */
HSV_API int hsv_committee_digit_bits(const hsv_committee *c);
/* Table memory the committee holds on its device: n * 393216 or n * 49152. */
HSV_API uint64_t hsv_committee_table_bytes(const hsv_committee *c);
HSV_API void hsv_committee_destroy(hsv_committee *c);
HSV_API size_t hsv_committee_size(const hsv_committee *c);
/* Index of pk in the committee, or -1. */
HSV_API int64_t hsv_committee_index(const hsv_committee *c, const uint8_t pk[32]);
/* Votes by member index: key_idx[m], sig m*64 B, msg m*32 B (msg_stride 32)
 * or one shared digest (msg_stride 0); flags_out m bytes.  An index >= n
 * yields flags 0. */
HSV_API int hsv_committee_verify(hsv_committee *c, const uint32_t *key_idx, const uint8_t *sig,
                         const uint8_t *msg, size_t msg_stride, size_t m, uint8_t *flags_out);
/* crypto::Signature::verify_batch over votes packed pk||R||s: members use the
 * cached tables, any other key the generic kernel.  1 = Ok, 0 = Err, < 0 error. */
HSV_API int hsv_committee_verify_batch_packed(hsv_committee *c, const uint8_t digest[32], const uint8_t *votes,
                                      size_t m);
/* Device-resident, stream-ordered form (device = the committee's: buffers or
 * a stream of another device are HSV_ERR_INVALID_ARG, and nothing is
 * enqueued); d_fault (optional) as hsv_verify_device_bits. */
HSV_API int hsv_committee_verify_device(const hsv_committee *c, const uint32_t *d_key_idx, const uint8_t *d_sig,
                                size_t sig_stride, const uint8_t *d_msg, size_t msg_stride, size_t m,
                                uint8_t *d_flags, uint32_t *d_fault, void *stream);
/* Mempool transactions (layout and scheme of hsv_verify_transactions* below)
 * whose signers are mostly members of c.  Flags are bit for bit those of
 * hsv_verify_transactions* for the same bytes: a transaction whose pk bytes
 * equal a member's takes that member's comb table, any other the generic
 * kernels; which it is, is decided on the device, per transaction.  An empty
 * committee is valid (everything takes the generic kernels).
 * offsets != NULL: a ragged batch, n + 1 entries relative to txs; offsets ==
 * NULL: fixed tx_size.  txs at any alignment.
 * Host form: synchronous, on the committee's device, one staged copy per
 * launch (neither pipelined nor sharded across devices: the tables live on
 * one).  A transaction shorter than 96 bytes, or decreasing offsets, is
 * HSV_ERR_INVALID_ARG before any device work; a failed device self-check is
 * HSV_ERR_DEVICE_FAULT.
 * Device form: stream-ordered, never synchronises; device = the committee's
 * (as hsv_committee_verify_device).  d_flags / d_strict_bits: either may be
 * NULL, not both; every flag byte and strict word of the n transactions is
 * written.  A transaction shorter than 96 bytes, or whose offsets decrease,
 * gets flags 0 and strict bit 0 (its neighbours are unaffected); tx_size < 96
 * with d_offsets == NULL is HSV_ERR_INVALID_ARG.  d_fault (optional) as
 * hsv_verify_device_bits: word 0 from the curve self-check of either route,
 * word 1 from the generic route's canaries.  Batches above 2^22 run as rounds
 * of 2^22 in order on `stream`, three launches each.
 * When to use it (profiles/committee_tx_bench_2p20.json: 2^20 device-resident
 * transactions of 512 B, K = 4, 100 and 1000 keys, against
 * hsv_verify_transactions_device on the same bytes in the same run): with
 * every signer a member the call takes 0.40 of that call's time at each K
 * (2.49 - 2.52 x the rate); with half of the transactions members', 0.72 -
 * 0.73; with no member at all, 1.00 (0.995 - 1.004): the lookup costs
 * nothing measurable, and a caller who knows few of its signers loses
 * nothing but the committee's table memory (384 KiB per key). */
HSV_API int hsv_committee_verify_transactions(hsv_committee *c, const uint8_t *txs, const uint64_t *offsets,
                                              size_t tx_size, size_t n, uint8_t *flags_out);
HSV_API int hsv_committee_verify_transactions_device(const hsv_committee *c, const uint8_t *d_txs,
                                                     const uint64_t *d_offsets, size_t tx_size, size_t n,
                                                     uint8_t *d_flags, uint32_t *d_strict_bits,
                                                     uint32_t *d_fault, void *stream);
/* Whole messages of any length (RFC 8032 5.1.7 PureEdDSA; addressing and
 * scheme of hsv_verify_msgs* above) whose signers are mostly members of c.
 * Flags are bit for bit those of hsv_verify_msgs* for the same bytes: an item
 * whose 32 pk bytes equal a member's takes that member's comb table, any other
 * the generic kernels; which it is, is decided on the device, per item.  An
 * empty committee is valid; of a key listed twice the first index is used;
 * an undecodable or small-order member key shows in HSV_A_OK / HSV_SMALL_A as
 * everywhere else.
 * offsets != NULL: n + 1 entries relative to msgs; offsets == NULL: msg_len
 * bytes per item at msg_stride (0 = one shared message).  Empty messages are
 * allowed, msgs may sit at any alignment; pk / sig pointers and strides of the
 * device form are multiples of 16 (HSV_ERR_ALIGN).
 * Host form: synchronous, on the committee's device, plain staged copies
 * chunked as hsv_verify_msgs (at most 2^22 items and 2^29 message bytes per
 * round), neither pipelined nor sharded across devices.  Decreasing offsets
 * are HSV_ERR_INVALID_ARG before any device work; a failed device self-check
 * is HSV_ERR_DEVICE_FAULT; without a GPU, HSV_ERR_NO_DEVICE.
 * Device form: stream-ordered, never synchronises; device = the committee's
 * (as hsv_committee_verify_device).  d_flags / d_strict_bits: either may be
 * NULL, not both; every flag byte and strict word of the n items is written.
 * An item whose offsets decrease gets flags 0 and strict bit 0 (its neighbours
 * are unaffected).  d_fault (optional) as hsv_verify_device_bits: word 0 from
 * the curve self-check of either route, word 1 from the generic route's
 * canaries.  Batches above 2^22 run as rounds of 2^22 in order on `stream`,
 * three launches each; no pass after the first reads a message byte.
 * When to use it (profiles/committee_msgs_bench_2p20.json: 2^20 device-resident
 * items, K = 4, 100 and 1000 keys, against hsv_verify_msgs_device on the same
 * bytes in the same run): with every signer a member the call runs at 2.59 -
 * 2.72 x that call's rate on 32-byte messages, 2.52 - 2.57 x on 416-byte ones
 * and 2.32 - 2.34 x on ragged lengths 0 .. 1024; with half of the keys members
 * it takes 0.73 - 0.77 of that call's time; with no member at all, 1.00 - 1.03:
 * a caller who knows few of its signers loses a few percent and the
 * committee's table memory (384 KiB per key). */
HSV_API int hsv_committee_verify_msgs(hsv_committee *c, const uint8_t *pk, const uint8_t *sig,
                                      const uint8_t *msgs, const uint64_t *offsets, size_t msg_len,
                                      size_t msg_stride, size_t n, uint8_t *flags_out);
HSV_API int hsv_committee_verify_msgs_device(const hsv_committee *c, const uint8_t *d_pk, size_t pk_stride,
                                             const uint8_t *d_sig, size_t sig_stride, const uint8_t *d_msgs,
                                             const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                                             size_t n, uint8_t *d_flags, uint32_t *d_strict_bits,
                                             uint32_t *d_fault, void *stream);
/* The same whole messages with each signer named by its member index, as
 * hsv_committee_verify* names it (hsv_committee_index per vote, on the host):
 * a QC or TC whose votes sign whole messages.  Flags are bit for bit those of
 * hsv_verify_msgs* for (member key_idx[i]'s 32 key bytes, sig i, message i);
 * an index >= hsv_committee_size gives flags 0, as hsv_committee_verify does;
 * of a key listed twice either index gives the same flags.  Message
 * addressing as hsv_committee_verify_msgs* above (offsets / msg_len and
 * msg_stride, empty messages, msgs at any alignment).
 * Host form: synchronous, on the committee's device, staged and chunked as
 * hsv_committee_verify_msgs with the indices in the place of pk; decreasing
 * offsets are HSV_ERR_INVALID_ARG before any device work; a failed device
 * self-check is HSV_ERR_DEVICE_FAULT; without a GPU, HSV_ERR_NO_DEVICE.  It
 * uses neither the resident service nor the zero-copy markers nor the
 * automatic cache.
 * Device form: stream-ordered, never synchronises; device = the committee's
 * (as hsv_committee_verify_device).  d_sig and sig_stride are multiples of 16
 * (HSV_ERR_ALIGN), d_offsets 8-byte and d_key_idx 4-byte aligned.  d_flags is
 * required and every one of its m bytes is written; there are no strict bits
 * (hsv_committee_verify_device has none either).  An item whose offsets
 * decrease gets flags 0 and leaves its neighbours alone.  d_fault as
 * hsv_committee_verify_device.  At m <= 2^12 on a committee with 8-bit tables
 * the call is ONE launch without a memset (the 16-lanes-per-vote latency form
 * of hsv_committee_verify_device with a hash wave that reads whole messages);
 * above, and at every m on a compact committee, a memset and two launches
 * per round of 2^22 items.
 * When to use it: when the caller knows the member index of every signer --
 * there is no route for strangers here; mixed batches belong to
 * hsv_committee_verify_msgs*.  Measured (profiles/committee_msgs_indexed_bench.json,
 * K = 1000 keys, device-resident items, p50 of the call plus a
 * stream synchronise, against hsv_committee_verify_msgs_device and
 * hsv_verify_msgs_device on the same bytes in the same run): 0.052 ms at 67
 * votes of 32 bytes (0.273 and 0.116 ms), 0.078 ms at 416 bytes (0.291 and
 * 0.146), 0.069 - 0.120 ms at 667 votes (0.289 - 0.371 and 0.131 - 0.214),
 * 0.130 - 0.262 ms at 4096 (0.300 - 0.394 and 0.485 - 0.539); on 32-byte
 * messages 0.90 - 1.01 x hsv_committee_verify_device on the same votes as
 * digests.  From about 100 bytes on, the hash of the block's longest message
 * decides a small call's time.  At 2^20 items 0.98 - 1.00 x the pk-addressed
 * call's time. */
HSV_API int hsv_committee_verify_msgs_indexed(hsv_committee *c, const uint32_t *key_idx, const uint8_t *sig,
                                              const uint8_t *msgs, const uint64_t *offsets, size_t msg_len,
                                              size_t msg_stride, size_t m, uint8_t *flags_out);
HSV_API int hsv_committee_verify_msgs_indexed_device(const hsv_committee *c, const uint32_t *d_key_idx,
                                                     const uint8_t *d_sig, size_t sig_stride, const uint8_t *d_msgs,
                                                     const uint64_t *d_offsets, size_t msg_len, size_t msg_stride,
                                                     size_t m, uint8_t *d_flags, uint32_t *d_fault, void *stream);

/* ---- mempool transactions -------------------------- */
/* A client transaction is  message || pk (32 B) || sig (64 B, R||s)  and its
 * signature is checked over Digest(SHA-512(message)[..32]) with
 * Signature::verify, as in the reference's transaction check
 * (mempool/src/batch_maker.rs:79-85, consensus/src/core.rs:121-127).  The
 * per-transaction flags are hsv_verify's flags for that (pk, sig, digest);
 * HSV_STRICT_OK is the reference's `signature.verify(..).is_ok()`.
 * Transactions shorter than 96 bytes (the reference's slice would panic) are
 * rejected with HSV_ERR_INVALID_ARG by the host-buffer calls.  The signing
 * mirror, for load generation, is hsv_signer_sign_transactions* below. */

/* Ragged batch: transaction i is txs[offsets[i] .. offsets[i+1]) (n+1
 * offsets).  flags_out: n bytes. */
HSV_API int hsv_verify_transactions(const uint8_t *txs, const uint64_t *offsets, size_t n, uint8_t *flags_out);

/* Fixed-size batch (the benchmark client's transactions all have the same
 * size, node/src/client.rs): transaction i is txs[i*tx_size .. (i+1)*tx_size). */
HSV_API int hsv_verify_transactions_fixed(const uint8_t *txs, size_t tx_size, size_t n, uint8_t *flags_out);

/* Device-resident, stream-ordered form.  d_offsets (n+1 entries, relative to
 * d_txs) or NULL for fixed-size transactions of tx_size bytes.  Any alignment
 * of d_txs.  Transactions shorter than 96 bytes get flags 0.  Outputs and
 * d_fault as hsv_verify_device_bits (d_flags / d_strict_bits: either may be
 * NULL, not both). */
HSV_API int hsv_verify_transactions_device(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                                   uint8_t *d_flags, uint32_t *d_strict_bits, uint32_t *d_fault, void *stream);

/* ---- signer census: who signs a batch, and how often --------------------- */
/* hsv_committee_verify_transactions* needs the known clients' keys in an
 * hsv_committee; a mempool sees only the 32 pk bytes inside each transaction.
 * The census returns the distinct signer keys of a batch and how often each
 * occurs, counted on the GPU; the caller builds a committee from the frequent
 * ones (hsv_committee_create) and passes it to the calls above.  No existing
 * call changes: the census is explicit and opt-in.
 * Key: the 32 raw pk bytes.  Of a transaction these are bytes [len - 96,
 * len - 64), addressed by d_offsets / tx_size exactly as
 * hsv_verify_transactions_device addresses them, at any byte alignment.
 * Nothing is decompressed or verified: the census says who signs, not whether
 * they sign well.  A transaction shorter than 96 bytes, or whose offsets
 * decrease, is counted in `malformed` and nowhere else.
 * slots: the size of the census table, a power of two, 16 <= slots <= 2^22
 * (else HSV_ERR_INVALID_ARG).  Open addressing, linear probing, the slot hash
 * keyed with the per-process seed (keys are attacker-chosen bytes).  A probe
 * walk is bounded by min(slots, 256) slots: an item whose key finds neither
 * itself nor an empty slot within the bound is added to `overflow`, so a flood
 * of distinct keys cannot turn the call into an n x slots walk.  Slots never
 * empty: a key is either recorded with its exact count or not recorded at all.
 * At load <= 1/4 a run of 256 occupied slots does not occur in practice:
 * size slots >= 4 x the distinct keys you expect.
 * skip (optional): a key that is a member of `skip` is added to `members` and
 * not recorded -- "who are the frequent strangers?", for a caller who already
 * holds a committee.  Full and compact committees alike. */
typedef struct hsv_census_summary {
  uint64_t items;     /* n */
  uint64_t counted;   /* sum of the counts written */
  uint64_t members;   /* signer is a member of `skip` (0 without one) */
  uint64_t malformed; /* transaction forms: shorter than 96 bytes or decreasing offsets */
  uint64_t overflow;  /* the key found no slot (above) */
  uint32_t distinct;  /* entries written to keys_out / counts_out */
  uint32_t reserved;  /* 0 */
} hsv_census_summary; /* items == counted + members + malformed + overflow, always */

/* Device forms: stream-ordered, they never synchronise.  Device and stream as
 * hsv_verify_transactions_device (the device that owns the inputs; a stream
 * of another device is HSV_ERR_INVALID_ARG); with skip != NULL the inputs must
 * lie on its device.  Key form: d_pk and pk_stride are multiples of 16, as in
 * hsv_verify_device, pk_stride >= 32.  Transaction form: d_offsets (n + 1
 * entries relative to d_txs) or NULL for fixed tx_size (below 96:
 * HSV_ERR_INVALID_ARG).  d_keys_out (32 * slots bytes) is 16-byte,
 * d_counts_out (slots words) and d_summary 8-byte aligned (HSV_ERR_ALIGN).
 * Every entry of d_keys_out and d_counts_out is written: the first `distinct`
 * are the census, in no particular order, the rest are 0.  n <= 2^32 - 1;
 * n == 0 is valid (the inputs may be NULL) and gives an all-zero summary.
 * Two launches and one memset; the workspace, 8 bytes per slot, is a block of
 * its own per call from the library's stream-ordered pool.  All argument
 * errors are reported before any device work. */
HSV_API int hsv_census_keys_device(const hsv_committee *skip, const uint8_t *d_pk, size_t pk_stride, size_t n,
                                   uint32_t slots, uint8_t *d_keys_out, uint32_t *d_counts_out,
                                   hsv_census_summary *d_summary, void *stream);
HSV_API int hsv_census_transactions_device(const hsv_committee *skip, const uint8_t *d_txs, const uint64_t *d_offsets,
                                           size_t tx_size, size_t n, uint32_t slots, uint8_t *d_keys_out,
                                           uint32_t *d_counts_out, hsv_census_summary *d_summary, void *stream);
/* Host forms: synchronous, on skip's device or else the device a host-buffer
 * call runs on.  Only the 32 key bytes of each item are staged (a 512-byte
 * transaction costs 32 bytes of host-to-device copy), at any alignment and
 * pk_stride >= 32.  The result is sorted by count descending, then key bytes
 * ascending, so it is deterministic; the first min(distinct, keys_cap) entries
 * are written to keys_out (32 bytes each) and counts_out, which may be NULL
 * when keys_cap is 0; summary->distinct is the full number.  n <= 2^22 (above:
 * HSV_ERR_INVALID_ARG before any device work).  Without a GPU,
 * HSV_ERR_NO_DEVICE. */
HSV_API int hsv_census_keys(hsv_committee *skip, const uint8_t *pk, size_t pk_stride, size_t n, uint32_t slots,
                            uint8_t *keys_out, uint32_t *counts_out, size_t keys_cap, hsv_census_summary *summary);
HSV_API int hsv_census_transactions(hsv_committee *skip, const uint8_t *txs, const uint64_t *offsets, size_t tx_size,
                                    size_t n, uint32_t slots, uint8_t *keys_out, uint32_t *counts_out, size_t keys_cap,
                                    hsv_census_summary *summary);

/* ---- wire formats ---------------------------------- */
/* Certificates verified straight from their bincode bytes (bincode 1.3
 * defaults: little-endian, u64 lengths; PublicKey is its base64 string,
 * crypto/src/lib.rs:94-101).  Only the signature part of the reference's
 * verify is done here; the quorum/stake checks stay with the caller, who can
 * get the decoded keys back.  Returns 1 = Ok, 0 = Err (a signature fails),
 * HSV_ERR_PARSE for malformed bytes, other < 0 for infrastructure errors. */

/* consensus::QC (consensus/src/messages.rs:162-167): hash (32) | round (u64)
 * | votes Vec<(PublicKey, Signature)>.  Checks
 * Signature::verify_batch(&qc.digest(), &qc.votes) (messages.rs:196-197),
 * qc.digest() = SHA-512(hash || round_le)[..32] (messages.rs:201-207).
 * n_votes_out (optional): number of votes; pks_out (optional, 32 B per vote):
 * the decoded keys, in order. */
HSV_API int hsv_qc_verify_bincode(const uint8_t *buf, size_t len, size_t *n_votes_out, uint8_t *pks_out);

/* consensus::TC (messages.rs:281-285): round (u64) | votes
 * Vec<(PublicKey, Signature, Round)>.  Checks every vote with
 * Signature::verify over SHA-512(round_le || high_qc_round_le)[..32]
 * (messages.rs:306-313); 1 iff all pass.  flags_out (optional, one byte per
 * vote): the per-vote HSV_* flags. */
HSV_API int hsv_tc_verify_bincode(const uint8_t *buf, size_t len, size_t *n_votes_out, uint8_t *flags_out);

/* ---- proposals, votes and timeouts in one call each ----------------------- */
/* The signature half of Block::verify, Timeout::verify and Vote::verify
 * (consensus/src/messages.rs:55-76, 250-265, 136-146): every signature of
 * the object -- the author's, the embedded QC's votes, the embedded TC's
 * votes -- goes down in ONE verification call, each over its own digest, and
 * the flags are read back under each stage's own acceptance rule.  The stake,
 * quorum and authority-reuse checks of the reference (committee.stake,
 * quorum_threshold, the `used` sets of QC::verify / TC::verify) are NOT done
 * here: they stay with the caller, as for hsv_qc_verify_bincode and
 * hsv_tc_verify_bincode, and run before this call as they do in the
 * reference.
 *
 * A proposal as plain data, as a shim fills it from a deserialized Block.
 * Pointers are borrowed for the call; one whose count is 0 may be NULL. */
typedef struct hsv_proposal {
  uint8_t author[32];
  uint8_t signature[64]; /* R || s */
  uint64_t round;
  const uint8_t *payload; /* n_payload * 32 B: the payload digests */
  size_t n_payload;
  uint8_t qc_hash[32];
  uint64_t qc_round;
  const uint8_t *qc_votes; /* n_qc records of 96 B: pk || R || s */
  size_t n_qc;
  int has_tc; /* 0: tc == None */
  uint64_t tc_round;
  const uint8_t *tc_votes; /* n_tc records of 104 B: pk || R || s || high_qc_round (u64 LE) */
  size_t n_tc;
} hsv_proposal;

/* The verdict in the reference's order: `stage` is the first stage that
 * fails (author signature, then QC, then TC), `index` the lowest failing vote
 * of that stage (0 for the author).  For a QC the index is informational:
 * dalek's verify_batch names no vote. */
#define HSV_STAGE_OK 0u
#define HSV_STAGE_AUTHOR 1u
#define HSV_STAGE_QC 2u
#define HSV_STAGE_TC 3u
#define HSV_STAGE_PARSE 4u /* hsv_blocks_verify_bincode only: the block's bytes are malformed */
typedef struct hsv_proposal_result {
  uint32_t stage;
  uint32_t index;
} hsv_proposal_result;

/* Rules (exactly the reference's):
 *   author  HSV_STRICT_OK over SHA-512(author || round_le || payload... ||
 *           qc.hash)[..32] (messages.rs:80-89);
 *   QC      only if qc != QC::genesis(), and PartialEq compares hash and round
 *           alone (messages.rs:216-220): a QC with a zero hash and round 0 is
 *           skipped whatever votes it carries.  Otherwise every vote must have
 *           (flags & (HSV_PARSE_OK|HSV_EQ_OK)) == both over
 *           SHA-512(hash || round_le)[..32]; an empty vote list passes;
 *   TC      if present, every vote HSV_STRICT_OK over
 *           SHA-512(tc.round_le || high_qc_round_le)[..32].
 * Returns 1 = Ok (res->stage == HSV_STAGE_OK), 0 = Err (res says where), < 0
 * an infrastructure error, never a rejection.  res (optional) is written on
 * 0 and 1 only.
 * flags_out (optional, 1 + n_qc + n_tc bytes): the items' raw HSV_* flags in
 * the order author, QC votes, TC votes; the votes of a skipped (genesis) QC
 * are not verified and read 0.
 * c == NULL: the items go through hsv_verify with per-item digests -- the
 * automatic committee cache, the latency forms, the resident service for at
 * most 4 items.  c != NULL: through hsv_committee_verify by member index; a
 * key that is not a member of c gets an index >= hsv_committee_size and so
 * flags 0, a rejection at its stage and index, as the reference rejects a
 * non-member (UnknownAuthority). */
HSV_API int hsv_proposal_verify(hsv_committee *c, const hsv_proposal *p, hsv_proposal_result *res,
                                uint8_t *flags_out);

/* consensus::Block from its bincode bytes (messages.rs:16-24): qc | tc:
 * Option<TC> (u8 tag 0 / 1) | author: PublicKey str | round: u64 | payload:
 * Vec<Digest> | signature (64); then hsv_proposal_verify.  Malformed bytes
 * (truncation, trailing bytes, a count beyond the buffer, bad base64, an
 * Option tag other than 0 or 1) are HSV_ERR_PARSE, reported before any device
 * is looked for.  n_qc_out / n_tc_out (optional): the vote counts (n_tc 0
 * without a TC); pks_out (optional, 32 B each): the decoded keys in the order
 * author, QC voters, TC voters, for the caller's stake and quorum checks. */
HSV_API int hsv_block_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len, hsv_proposal_result *res,
                                     size_t *n_qc_out, size_t *n_tc_out, uint8_t *pks_out);

/* consensus::Timeout (messages.rs:222-228): high_qc | round | author |
 * signature.  The author is checked strict over
 * SHA-512(round_le || high_qc.round_le)[..32] (messages.rs:268-275), high_qc
 * under the QC rule unless it is genesis; one verification call.  The TC stage
 * is never reported.  pks_out: author, then the QC voters. */
HSV_API int hsv_timeout_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len, hsv_proposal_result *res,
                                       size_t *n_qc_out, uint8_t *pks_out);

/* consensus::Vote (messages.rs:112-118): hash | round | author | signature,
 * checked strict over SHA-512(hash || round_le)[..32] (messages.rs:149-156).
 * c == NULL: routed exactly as hsv_verify_strict; c != NULL: one item by
 * member index.  1 = Ok, 0 = Err, HSV_ERR_PARSE, other < 0. */
HSV_API int hsv_vote_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len);

/* A chain of blocks (a node catching up through the synchronizer): block i is
 * bufs[offsets[i] .. offsets[i+1]) (n_blocks + 1 non-decreasing offsets, else
 * HSV_ERR_INVALID_ARG).  All items of all blocks go down in ONE verification
 * call -- so a long chain takes the pipelined or sharded host path, or the
 * committee's comb pass when c is given -- and the flags are reduced per block
 * on the host.  results (optional, n_blocks entries): each block's verdict; a
 * block whose bytes do not parse gets HSV_STAGE_PARSE and leaves its
 * neighbours alone.  Returns the number of blocks with HSV_STAGE_OK (0 for
 * n_blocks == 0), or < 0 for an infrastructure error. */
HSV_API int hsv_blocks_verify_bincode(hsv_committee *c, const uint8_t *bufs, const uint64_t *offsets,
                                      size_t n_blocks, hsv_proposal_result *results);

/* ---- serialized mempool batches -------------------------------------------
 * Core::make_vote's payload check (consensus/src/core.rs:113-142) from the
 * stored bytes: a mempool::MempoolMessage::Batch(Vec<Vec<u8>>) as
 * BatchMaker::seal serializes it (mempool/src/batch_maker.rs:127-131; bincode
 * 1.3 defaults): u32 LE variant tag (0 = Batch) | u64 LE count | count x (u64 LE
 * length, bytes).  The transactions are verified where they lie: nothing is
 * deserialized, re-packed or copied on the device; the transaction kernels
 * address them through a table of span pairs.
 * Rule, per transaction: the flags of hsv_verify_transactions* for the same
 * bytes, bit for bit (Signature::verify over SHA-512(message)[..32], the last
 * 96 bytes pk || R || s).  A transaction shorter than 96 bytes gets flags 0
 * and is a rejection at its index (the reference's slice would panic; batches
 * are untrusted network bytes).  A batch passes iff every transaction has
 * HSV_STRICT_OK; an empty batch passes.
 * Malformed (HSV_BATCH_PARSE; HSV_ERR_PARSE from the single-batch calls): a tag
 * other than 0 (a BatchRequest, which make_vote rejects, is tag 1), truncation
 * anywhere, a count above the remaining bytes / 8, a length that runs past the
 * batch's own end (whatever bytes follow it), trailing bytes after the last
 * transaction.  (bincode::deserialize itself would accept trailing bytes; this
 * library's parsers reject them in every object.)  A malformed batch leaves
 * its neighbours alone.
 * The stake and quorum checks stay with the caller, and so does the batch's own
 * digest (its store key) on this read side; the write side,
 * hsv_seal_transactions* below, can deliver it with the batch it builds. */
#define HSV_BATCH_OK 0u
#define HSV_BATCH_TX 1u       /* transaction `index` is the lowest that fails */
#define HSV_BATCH_PARSE 2u    /* not a well-formed MempoolMessage::Batch */
#define HSV_BATCH_OVERFLOW 3u /* device form: its transactions do not fit tx_cap */
typedef struct hsv_batch_result {
  uint32_t status, index;
  uint64_t n_tx;  /* the batch's transactions; 0 for a malformed batch */
  uint64_t first; /* the index of its first transaction in the flags array */
} hsv_batch_result;

/* The parse alone, on the host; needs no GPU.  1 = well-formed (n_tx_out,
 * optional: the count), HSV_ERR_PARSE otherwise.  spans_out (optional,
 * spans_cap entries): transaction i is buf[spans_out[2i], spans_out[2i+1]);
 * spans_cap < 2 * count is HSV_ERR_INVALID_ARG. */
HSV_API int hsv_batch_parse_bincode(const uint8_t *buf, size_t len, size_t *n_tx_out, uint64_t *spans_out,
                                    size_t spans_cap);

/* Host form: batch b is bufs[offsets[b] .. offsets[b+1]) (n_batches + 1
 * non-decreasing offsets, else HSV_ERR_INVALID_ARG), at any alignment.
 * Synchronous, on the home device (c == NULL: the generic kernels) or the
 * committee's (c != NULL: the routes of hsv_committee_verify_transactions*; a
 * compact committee is accepted like a full one).  The host parses -- a
 * malformed batch costs no device work -- and stages whole batches in rounds
 * within the item and byte limits of hsv_verify_transactions (2^22
 * transactions, 2^29 bytes); a single batch above the byte limit is
 * HSV_ERR_INVALID_ARG (the reference's frames are far smaller).  Not sharded
 * across devices.  Transactions are numbered in batch order over the
 * well-formed batches; results (optional, n_batches entries) and flags_out
 * (optional; flags_cap below the total is HSV_ERR_INVALID_ARG before any device
 * work) as above.  Returns the number of batches with HSV_BATCH_OK, or < 0:
 * HSV_ERR_NO_DEVICE without a GPU, HSV_ERR_DEVICE_FAULT for a failed
 * self-check. */
HSV_API int hsv_batches_verify_bincode(hsv_committee *c, const uint8_t *bufs, const uint64_t *offsets,
                                       size_t n_batches, hsv_batch_result *results, uint8_t *flags_out,
                                       size_t flags_cap);
/* One batch: 1 = every transaction verifies, 0 = one does not (res says which),
 * HSV_ERR_PARSE, other < 0.  res (optional) is written on 0 and 1 only. */
HSV_API int hsv_batch_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len, hsv_batch_result *res);

/* Device form: the batches already in HBM, parsed there (one wave per batch
 * streams it through LDS; csrc/hsv_batchwire.hip).  Stream-ordered, never
 * synchronises; d_fault (optional), device ownership and the stream checks as
 * hsv_verify_transactions_device (c == NULL) / hsv_committee_verify_device.
 * d_offsets: n_batches + 1 entries, 8-byte aligned; a batch whose offsets
 * decrease is HSV_BATCH_PARSE.  d_results: n_batches entries, 8-byte aligned.
 * d_flags (optional): every byte of d_flags[0 .. tx_cap) is written, bytes past
 * the total are 0.  A batch whose transactions do not all lie below tx_cap gets
 * HSV_BATCH_OVERFLOW and is not verified (n_tx and first still say what it
 * needs); earlier batches are unaffected.  The transaction count is known on
 * the device only, so every launch and the workspace (16 + 128 bytes per
 * transaction, from the library's stream-ordered pool) are sized by tx_cap: the
 * caller takes the exact count from hsv_batch_parse_bincode while the bytes
 * pass through the host, or accepts the padding's cost -- a padded slot is
 * verified like a malformed transaction.  tx_cap above 2^32 - 1 and n_batches
 * above 2^32 - 1 are HSV_ERR_INVALID_ARG.
 * When to use it (profiles/batch_wire_bench.json: 512-byte transactions, batches
 * of 500,000 B = 977 transactions, p50, both sides in one run): for batches
 * that already lie in HBM.  1024 batches take 10.23 ms against 9.47 ms of
 * hsv_verify_transactions_device on the same transactions packed with
 * precomputed offsets (1.08 x): the excess is the parse, 0.70 ms, which is one
 * wave's serial walk per batch and so costs the same 0.63 - 0.70 ms for 1, 64 or
 * 1024 batches.  It therefore dominates few batches: 64 take 1.50 against
 * 0.98 ms (1.53 x), one takes 0.90 against 0.26 ms (3.4 x).  A caller whose
 * bytes pass through the host takes the host form, where the parse costs
 * nothing measurable: one batch of 500,000 B in 0.314 ms against 0.307 ms of
 * hsv_verify_transactions on transactions already packed (15,000 B: 0.165
 * against 0.163 ms), and the repacking that call needs (0.38 ms and 0.02 ms
 * as a parse plus one copy per transaction) is saved. */
HSV_API int hsv_batches_verify_bincode_device(const hsv_committee *c, const uint8_t *d_bufs,
                                              const uint64_t *d_offsets, size_t n_batches, size_t tx_cap,
                                              hsv_batch_result *d_results, uint8_t *d_flags, uint32_t *d_fault,
                                              void *stream);

/* ---- sealing verified transactions into mempool batches -------------------
 * BatchMaker::run / seal (mempool/src/batch_maker.rs:78-131) on the device: the
 * mirror of the serialized-batch calls above.  Of n transactions, addressed as
 * hsv_verify_transactions_device addresses them (d_offsets, or fixed tx_size;
 * any byte alignment), those with flags[i] & HSV_STRICT_OK are kept -- the
 * flags of any verify call: generic, committee or the batch-wire form.  With
 * d_flags == NULL every transaction is kept, whatever its length: a pure
 * serializer, for load generation.  A transaction whose offsets decrease is
 * malformed: dropped and counted.
 * The kept transactions are walked in index order; each is appended and its
 * length (the whole transaction, trailer included) added to a running size;
 * when the size is >= batch_size the batch is closed and the size reset
 * (batch_maker.rs:87-92).  flush != 0 closes a last batch that holds at least
 * one transaction (the timer branch, lines 100-105); flush == 0 leaves those
 * transactions held, and held_first says from which index the caller submits
 * again.  Each batch is  u32 LE 0 | u64 LE count | count x (u64 LE length,
 * bytes), the bincode of MempoolMessage::Batch; the batches lie end to end in
 * the output, so (d_out, d_batch_offsets) is a valid (d_bufs, d_offsets) of
 * hsv_batches_verify_bincode_device.  d_digests (optional): per batch,
 * SHA-512(batch bytes)[..32], the store key Processor computes
 * (mempool/src/processor.rs:30). */
#define HSV_SEAL_OK 0u
#define HSV_SEAL_OVERFLOW 1u /* out_cap or batches_cap too small; bytes / n_batches say what is needed */
typedef struct hsv_seal_summary {
  uint64_t items, sealed, rejected, malformed, held;
  uint64_t held_first; /* lowest index of a held transaction; n if none */
  uint64_t bytes;      /* length of all batches together */
  uint32_t n_batches, status;
} hsv_seal_summary; /* 64 bytes; items == sealed + rejected + malformed + held, always */

/* Host arithmetic, no GPU: an out_cap and a batches_cap that are never below
 * the need of n transactions of total_tx_bytes bytes together, whichever are
 * kept.  batch_size == 0, or sums beyond 64 bits: HSV_ERR_INVALID_ARG. */
HSV_API int hsv_seal_bound(uint64_t total_tx_bytes, uint64_t n, uint64_t batch_size, uint64_t *bytes_out,
                           uint64_t *batches_out);
/* Device form: stream-ordered, never synchronises; device ownership and stream
 * checks as hsv_verify_transactions_device.  d_out at any alignment;
 * d_batch_offsets (batches_cap + 1 entries, all written: entries past n_batches
 * repeat the end offset) and d_summary 8-byte aligned, as d_offsets, else
 * HSV_ERR_ALIGN.  d_digests: 32 bytes x batches_cap, any alignment; entries
 * past n_batches are not written.  On HSV_SEAL_OVERFLOW the contents of d_out,
 * the offsets and the digests are unspecified, nothing is written at or beyond
 * d_out + out_cap nor beyond the arrays' caps, and the summary is exact.
 * HSV_ERR_INVALID_ARG, before any device work: batch_size == 0, n > 2^32 - 1,
 * fixed tx_size == 0 with n > 0, a NULL d_batch_offsets or d_summary, a NULL
 * d_txs with n > 0 or d_out with out_cap > 0, and a [d_out, d_out + out_cap)
 * that overlaps a fixed-size input.  n == 0 is valid and gives zero batches.
 * Six launches (seven with digests) and no wait of one workgroup for another;
 * the workspace, 20 bytes per transaction, is a block of its own per call from
 * the library's stream-ordered pool.
 * When to use it: for transactions and flags already in HBM
 * (profiles/seal_bench.json, one MI355X: 2^20 transactions of 512 B, 5 % rejected,
 * batch_size 500,000): the call takes 3.29 ms (scan 0.05, cut 2.84, copy 0.37),
 * 0.32 x hsv_verify_transactions_device on the same bytes (10.39 ms); the copy
 * launches take 1.98 x a device-to-device hipMemcpyAsync of the output.  d_digests adds
 * 34.2 ms, against 34.8 ms of hashlib over the same batches on 16 host threads: no
 * faster than the host, but a device-resident pipeline has no other source for the
 * store key. */
HSV_API int hsv_seal_transactions_device(const uint8_t *d_txs, const uint64_t *d_offsets, size_t tx_size, size_t n,
                                         const uint8_t *d_flags, uint64_t batch_size, int flush, uint8_t *d_out,
                                         size_t out_cap, uint64_t *d_batch_offsets, size_t batches_cap,
                                         uint8_t *d_digests, hsv_seal_summary *d_summary, void *stream);
/* Host form: the transactions are staged once, verified there
 * (hsv_verify_transactions_device for c == NULL, else
 * hsv_committee_verify_transactions_device; a transaction shorter than 96
 * bytes gets flags 0 and is rejected, as in those calls) and sealed on the same
 * stream; one device-to-host copy of [0, bytes) brings the batches back, the
 * offsets (batches_cap + 1 entries), digests_out (optional, 32 bytes x
 * batches_cap) and flags_out (optional, n bytes) beside it.  Synchronous, on
 * the committee's device or the home device; at most 2^22 transactions and
 * 2^29 bytes (HSV_ERR_INVALID_ARG above), not sharded.  With out_cap or
 * batches_cap too small the summary says HSV_SEAL_OVERFLOW with the exact
 * needs, flags_out is written and nothing else is.  Without a GPU,
 * HSV_ERR_NO_DEVICE. */
HSV_API int hsv_seal_transactions(hsv_committee *c, const uint8_t *txs, const uint64_t *offsets, size_t tx_size,
                                  size_t n, uint64_t batch_size, int flush, uint8_t *out, size_t out_cap,
                                  uint64_t *batch_offsets_out, size_t batches_cap, uint8_t *digests_out,
                                  uint8_t *flags_out, hsv_seal_summary *summary);

/* ---- the benchmark's sample transactions -----------------------------------
 * The reference measures itself through sample transactions.  Its client
 * (node/src/client.rs:106-148) puts exactly one into every burst: byte 0, then
 * the burst counter as a big-endian u64; every other transaction is byte 1, then
 * a running r; both zero-padded to the transaction size.  BatchMaker::seal
 * (mempool/src/batch_maker.rs:118-125, 133-153, feature `benchmark`) picks the
 * samples out of each batch -- tx[0] == 0 && tx.len() > 8, the id bytes 1..9
 * big-endian -- and logs "Batch {digest:?} contains sample tx {id}" for each and
 * "Batch {digest:?} contains {size} B" for the batch, size being the sum of the
 * transactions' lengths (current_batch_size); benchmark/benchmark/logs.py
 * computes TPS and latency from those lines and the client's "Sending sample
 * transaction {counter}".  The two calls below are those two ends for a
 * device-resident pipeline: client bursts -> hsv_signer_sign_transactions_device
 * -> a verify call -> hsv_seal_transactions_device -> the sample index, with no
 * batch copied to the host to be walked there.
 *
 * Sample index.  A transaction is a sample iff its length is > 8 and its first
 * byte is 0.  An empty transaction is not a sample (the reference's tx[0] would
 * panic on one; a batch from the store is untrusted bytes).  Ids are the bytes
 * 1..9 read big-endian at any byte alignment, in batch order and in transaction
 * order inside a batch. */
typedef struct hsv_batch_samples {
  uint32_t status, pad;  /* HSV_BATCH_OK / HSV_BATCH_PARSE / HSV_BATCH_OVERFLOW; pad = 0 */
  uint64_t n_tx;         /* as hsv_batch_result */
  uint64_t size;         /* sum of the transactions' lengths: what seal() logs as "contains {} B" */
  uint64_t n_samples;    /* transactions with len > 8 and byte 0 == 0 */
  uint64_t first_sample; /* index of this batch's first id in the ids array */
} hsv_batch_samples;     /* 40 bytes */

/* Host form, one batch; needs no GPU (like hsv_batch_parse_bincode).  1 = the
 * batch is well-formed and res (optional) is written, HSV_ERR_PARSE otherwise.
 * ids_out == NULL only counts; a non-NULL ids_out with ids_cap < n_samples is
 * HSV_ERR_INVALID_ARG with res still written (and the first ids_cap ids).
 * first_sample is 0. */
HSV_API int hsv_batch_samples_bincode(const uint8_t *buf, size_t len, hsv_batch_samples *res, uint64_t *ids_out,
                                      size_t ids_cap);
/* Device form: stream-ordered, never synchronises.  Batch b is
 * d_bufs[d_offsets[b] .. d_offsets[b+1]), parsed exactly as
 * hsv_batches_verify_bincode_device parses it: the same malformed rules, the same
 * meaning of tx_cap, the same HSV_BATCH_OVERFLOW; arguments, device ownership
 * and stream checks as there (n_batches or tx_cap above 2^32 - 1:
 * HSV_ERR_INVALID_ARG).  d_offsets, d_index (n_batches entries) and d_ids
 * (ids_cap entries; may be NULL when ids_cap == 0) are 8-byte aligned, else
 * HSV_ERR_ALIGN.  n_batches == 0 is valid and writes nothing.
 * first_sample and n_samples are exact whatever ids_cap is: an id whose position
 * is >= ids_cap is not written, nothing is written at or beyond d_ids + ids_cap,
 * and positions between the call's sample count and ids_cap are left untouched.
 * ids_cap = tx_cap always suffices.  A malformed batch gets HSV_BATCH_PARSE and
 * zeros elsewhere.  A batch whose transactions do not all lie below tx_cap gets
 * HSV_BATCH_OVERFLOW: n_tx and size are still exact (size = length - 12 -
 * 8 n_tx, which the parse knows), n_samples is 0, it contributes no ids, and
 * first_sample is where they would have begun; earlier batches are complete.
 * (d_out, d_batch_offsets) of hsv_seal_transactions_device can be passed whole,
 * with n_batches = batches_cap and tx_cap = the seal's n: the repeated end
 * offsets past the real count are zero-length batches, which come out as
 * HSV_BATCH_PARSE with no ids -- a device pipeline calls this without reading
 * the seal's n_batches back.  The seal's digests are the {digest} of the log
 * lines, entry for entry.
 * The parse (hsv_launch_batch_scan, as in the verify call), then four launches
 * (csrc/hsv_samples.hip): one lane per transaction reads its span and first
 * byte, an ordered compaction over the whole call (a workgroup scan, a scan of
 * the workgroup sums, an apply pass that writes the ids), and one lane per batch.
 * No workgroup waits for another.  The workspace, 20 bytes per transaction of
 * tx_cap and 20 per batch, is a block of its own per call from the library's
 * stream-ordered pool.
 * What it costs (profiles/samples_bench.json, one MI355X: 2^20 transactions of
 * 512 B from hsv_client_bursts_device with burst 1000, sealed at batch_size
 * 500,000 into 1074 batches; medians, one run): 0.87 ms for the seal's whole
 * output, 0.26 x the seal (3.34 ms) and 0.077 x hsv_batches_verify_bincode_device
 * on the same batches (11.40 ms); most of it is the device parse that call pays
 * as well.  The bursts themselves take 0.134 ms per 2^20, 1.49 x a hipMemsetAsync
 * of the bytes they write and 0.07 x signing them (1.82 ms). */
HSV_API int hsv_batches_samples_bincode_device(const uint8_t *d_bufs, const uint64_t *d_offsets, size_t n_batches,
                                               size_t tx_cap, hsv_batch_samples *d_index, uint64_t *d_ids,
                                               size_t ids_cap, void *stream);

/* The client's bursts (client.rs:106-148).  Transaction i lies at txs + i *
 * tx_size, at any alignment.  It belongs to burst j = i / burst with counter
 * c = counter0 + j (mod 2^64), at position x = i % burst, and is that burst's
 * sample iff x == c % burst.  A sample is 00 || BE64(c); any other transaction is
 * 01 || BE64(r) with r = r0 + (the number of non-sample transactions among
 * 0..i inclusive), mod 2^64 -- the reference's `r += 1` before the write.  Bytes
 * [9, tx_size - trailer) are zero; the last `trailer` bytes are never written:
 * trailer = 96 leaves room for hsv_signer_sign_transactions*, trailer = 0 is the
 * reference's unsigned filler.  n need not be a multiple of burst.  *r_out
 * (optional) is the r to continue with (the counter to continue with is
 * counter0 + n / burst, when n is a multiple of burst); it is computed on the
 * host in closed form in both forms.  burst == 0 or tx_size < 9 + trailer is HSV_ERR_INVALID_ARG (the
 * reference's size >= 9 check), as are n > 2^32 - 1 and a NULL txs with n > 0;
 * n == 0 does nothing.  The host form needs no GPU.  The device form is one
 * stream-ordered launch (sixteen lanes per transaction, 16-byte stores where the
 * destination allows), never synchronises, and checks device ownership and the
 * stream as hsv_verify_transactions_device. */
HSV_API int hsv_client_bursts(uint8_t *txs, size_t tx_size, size_t trailer, uint64_t counter0, uint64_t burst,
                              uint64_t r0, size_t n, uint64_t *r_out);
HSV_API int hsv_client_bursts_device(uint8_t *d_txs, size_t tx_size, size_t trailer, uint64_t counter0,
                                     uint64_t burst, uint64_t r0, size_t n, uint64_t *r_out, void *stream);

/* ---- signing (host CPU; not on the hot path) ---------------------------- */
/* Public key for a 32-byte secret seed (dalek Keypair from SecretKey). */
HSV_API int hsv_public_key(const uint8_t seed[32], uint8_t pk_out[32]);
/* RFC 8032 deterministic signature (Signature::new). */
HSV_API int hsv_sign(const uint8_t seed[32], const uint8_t *msg, size_t msg_len, uint8_t sig_out[64]);
/* Bulk: n seeds (n*32 B), n messages of msg_len bytes each; writes n public
 * keys and n signatures.  nthreads <= 0 picks min(hardware concurrency, 16). */
HSV_API int hsv_sign_many(const uint8_t *seeds, const uint8_t *msgs, size_t msg_len, size_t n,
                  uint8_t *pk_out, uint8_t *sig_out, int nthreads);

/* ---- signing and key derivation on the GPU (batch) ----------------------- */
/* The GPU form of generate_keypair and Signature::new for load generators and
 * input synthesis: a signer expands its seeds once into 96-byte records
 * a | prefix | pk in HBM of the device bound at creation (hsv_init, as a
 * committee) and then signs batches from them, bit-exact with hsv_sign /
 * hsv_sign_many (RFC 8032, deterministic).
 * NOT constant time: [r]B and [a]B are sums of entries of the B comb table,
 * and those lookups are indexed by digits of the secret scalars.  This path is
 * for load generation and synthesising inputs, never for custody of a
 * validator key.  There is no CPU fallback: without a GPU every call below
 * returns HSV_ERR_NO_DEVICE (hsv_sign_many is the host signer). */
typedef struct hsv_signer hsv_signer;
/* Expand nkeys seeds (nkeys*32 B) on the GPU.  nkeys == 0 gives an empty signer. */
HSV_API int hsv_signer_create(const uint8_t *seeds, size_t nkeys, hsv_signer **out);
HSV_API void hsv_signer_destroy(hsv_signer *s);
HSV_API size_t hsv_signer_size(const hsv_signer *s);
/* The public keys, in seed order: nkeys*32 B. */
HSV_API int hsv_signer_public_keys(const hsv_signer *s, uint8_t *pk_out);
/* Sign m messages of msg_len bytes each (any length): item i signs
 * msgs + i*msg_stride with key key_idx[i].  key_idx == NULL: item i uses key
 * i (m <= nkeys).  msg_stride == 0: one shared message (a committee signing
 * one QC digest).  An index >= nkeys writes 64 zero bytes and raises no fault
 * (as hsv_committee_verify answers flags 0).  sig_out: m*64 B, R || s.  Host
 * buffers, synchronous; m == 0 does nothing.  A failed device self-check (an
 * [r]B that is not a curve point: corrupted table memory) zeroes that item's
 * signature and returns HSV_ERR_DEVICE_FAULT. */
HSV_API int hsv_signer_sign(hsv_signer *s, const uint32_t *key_idx, const uint8_t *msgs, size_t msg_len,
                            size_t msg_stride, size_t m, uint8_t *sig_out);
/* Device-resident, stream-ordered form (device = the signer's: buffers or a
 * stream of another device are HSV_ERR_INVALID_ARG, and nothing is enqueued;
 * no synchronisation): item i's signature goes to d_sig + i*sig_stride, so
 * sig_stride 96 with d_sig = records + 32 fills packed pk||R||s vote records.
 * d_sig and sig_stride must be multiples of 16 (HSV_ERR_ALIGN); d_msg may have
 * any alignment.  d_fault (optional) as hsv_verify_device_bits (only
 * d_fault[0] is ever set).  Batches above 2^22 items run as 2^22-item
 * launches, in order on `stream`. */
HSV_API int hsv_signer_sign_device(const hsv_signer *s, const uint32_t *d_key_idx, const uint8_t *d_msg, size_t msg_len,
                                   size_t msg_stride, size_t m, uint8_t *d_sig, size_t sig_stride, uint32_t *d_fault,
                                   void *stream);
/* Sign mempool transactions in place: the signing mirror of
 * hsv_verify_transactions*.  Fill in the last 96 bytes of every transaction:
 * pk (32) || R || s (64), the signature over Digest(SHA-512(message)[..32])
 * with message = the bytes before them -- what hsv_verify_transactions*
 * accepts, bit-exact with hsv_public_key plus hsv_sign(seed,
 * SHA-512(message)[..32], 32).  Message bytes are never written; the message
 * may be empty (a 96-byte transaction).
 * offsets != NULL: transaction i is txs[offsets[i] .. offsets[i+1]) (n+1
 *                  entries, relative to txs).
 * offsets == NULL: transaction i is txs[i*tx_size .. (i+1)*tx_size).
 * txs, the offsets and tx_size may have any alignment.  key_idx == NULL: item
 * i uses key i (n <= nkeys); otherwise key key_idx[i], and an index >= nkeys
 * writes 96 zero bytes and raises no fault (as hsv_signer_sign writes a zero
 * signature).  As the rest of the signer this path is NOT constant time: it is
 * for load generation and input synthesis only, never for a key that matters.
 * Host form: synchronous, on the signer's device; n == 0 does nothing.  A
 * transaction shorter than 96 bytes, or decreasing offsets, return
 * HSV_ERR_INVALID_ARG before anything is written (the length check of
 * hsv_verify_transactions); a failed device self-check returns
 * HSV_ERR_DEVICE_FAULT (that item: its pk and a zero signature).  There is no
 * CPU fallback (HSV_ERR_NO_DEVICE without a GPU).  Plain staged copies on one
 * device: this call is neither pipelined nor sharded across GPUs. */
HSV_API int hsv_signer_sign_transactions(hsv_signer *s, const uint32_t *key_idx, uint8_t *txs,
                                         const uint64_t *offsets, size_t tx_size, size_t n);
/* Device-resident, stream-ordered form (device = the signer's: buffers or a
 * stream of another device are HSV_ERR_INVALID_ARG); never synchronises.  A
 * transaction shorter than 96 bytes, or one whose offsets decrease, is left
 * completely untouched, and its neighbours are unaffected (with d_offsets NULL
 * a tx_size below 96 is HSV_ERR_INVALID_ARG, as in
 * hsv_verify_transactions_device).  d_fault (optional) as
 * hsv_signer_sign_device: only d_fault[0] is ever set, by an item whose [r]B
 * fails the self-check; that item gets its pk and a zero signature.  Batches
 * above 2^22 items run as 2^22-item launches, in order on `stream`.  Every
 * launch is two kernels: the message digests, then the signatures. */
HSV_API int hsv_signer_sign_transactions_device(const hsv_signer *s, const uint32_t *d_key_idx, uint8_t *d_txs,
                                                const uint64_t *d_offsets, size_t tx_size, size_t n,
                                                uint32_t *d_fault, void *stream);
/* Sign whole messages whose lengths differ: the signing mirror of
 * hsv_verify_msgs*, which is the verifying half of this call.  Addressing is
 * hsv_verify_msgs*'s, keys and outputs are hsv_signer_sign*'s:
 * offsets != NULL: message i is msgs[offsets[i] .. offsets[i+1]) (m+1 entries,
 *                  relative to msgs).
 * offsets == NULL: message i is msg_len bytes at msgs + i*msg_stride
 *                  (msg_stride 0: one shared message; a non-zero stride below
 *                  msg_len is HSV_ERR_INVALID_ARG).
 * A message may be empty.  msgs may have any alignment, and may be NULL when
 * every message is empty.  key_idx == NULL: item i uses key i (m <= nkeys,
 * else HSV_ERR_INVALID_ARG); otherwise key key_idx[i], and an index >= nkeys
 * writes 64 zero bytes and raises no fault.  sig_out: m*64 B, R || s, bit-exact
 * with hsv_sign(seed, M, len).  As the rest of the signer this path is
 * NOT constant time: it is for load generation and input synthesis only, never
 * for a key that matters.
 * Host form: synchronous, on the signer's device; m == 0 does nothing.
 * Decreasing offsets return HSV_ERR_INVALID_ARG (hsv_last_error names the
 * item) before any device work and before a byte of sig_out is written; a
 * failed device self-check returns HSV_ERR_DEVICE_FAULT (that item: 64 zero
 * bytes).  There is no CPU fallback (HSV_ERR_NO_DEVICE without a GPU).  Plain
 * staged copies on one device, at most 2^22 items and 2^29 message bytes per
 * round: this call is neither pipelined nor sharded across GPUs. */
HSV_API int hsv_signer_sign_msgs(hsv_signer *s, const uint32_t *key_idx, const uint8_t *msgs,
                                 const uint64_t *offsets, size_t msg_len, size_t msg_stride,
                                 size_t m, uint8_t *sig_out);
/* Device-resident, stream-ordered form (device = the signer's: buffers or a
 * stream of another device are HSV_ERR_INVALID_ARG); never synchronises.
 * d_sig and sig_stride must be multiples of 16, d_key_idx 4-byte and d_offsets
 * 8-byte aligned (HSV_ERR_ALIGN, checked before anything else is looked at);
 * sig_stride >= 64.  An item whose offsets decrease gets 64 zero bytes and no
 * fault; its neighbours are unaffected.  d_fault (optional) as
 * hsv_signer_sign_device: only d_fault[0] is ever set, by an item whose [r]B
 * fails the self-check; that item gets 64 zero bytes.  Batches above 2^22
 * items run as 2^22-item rounds, in order on `stream`.  A round is three
 * kernels: the nonces r = SHA-512(prefix || M), the points R = [r]B, the
 * responses s = r + SHA-512(R || pk || M) a. */
HSV_API int hsv_signer_sign_msgs_device(const hsv_signer *s, const uint32_t *d_key_idx,
                                        const uint8_t *d_msgs, const uint64_t *d_offsets,
                                        size_t msg_len, size_t msg_stride, size_t m,
                                        uint8_t *d_sig, size_t sig_stride, uint32_t *d_fault,
                                        void *stream);

/* Synthesis helper for the corrupted-input mixes (SURVEY 8(d) C3/C4 "mixed-
 * order A"; Appendix A.3 rows 7-8): the key A' = [a]B + [2*torsion+1]T8 (a
 * from seed as in hsv_public_key, T8 a point of order 8, torsion in 0..3) and
 * a signature over msg whose challenge k is = 0 (mod 8) when accept != 0
 * (verify_strict accepts: cofactorless equation holds) or != 0 (mod 8) when
 * accept == 0 (rejected; a cofactored verifier would accept). */
HSV_API int hsv_sign_mixed_order(const uint8_t seed[32], const uint8_t *msg, size_t msg_len, int torsion, int accept,
                         uint8_t pk_out[32], uint8_t sig_out[64]);

/* ---- measurement helpers ------------------------------------------------ */
/* Measured issue rate of v_mad_u64_u32 on the current device, in
 * multiply-accumulates per second (the roofline denominator). */
HSV_API double hsv_measure_mad_peak(void);
/* Kernel variant id the library runs (21: the product default). */
HSV_API int hsv_get_variant(void);
/* Host threads of the staging-copy pool, the calling thread excluded. */
HSV_API int hsv_pack_threads(void);
/* The calling thread's last host-buffer verification: host milliseconds spent
 * packing into pinned staging, bytes copied host-to-device, wall milliseconds
 * of the call (any pointer may be NULL). */
HSV_API void hsv_host_call_stats(double *pack_ms, double *h2d_bytes, double *call_ms);
/* Host timeline of the calling thread's last call, milliseconds from its
 * entry.  For a latency call (one launch: a QC, a vote, a small batch) the
 * HSV_MARK_* points below (a point the call did not pass reads -1); for a
 * pipelined call four marks per chunk (staging buffer free, packed, copy
 * enqueued, launch enqueued).  Writes min(count, cap) values to out (may be
 * NULL) and returns the count. */
#define HSV_MARK_LOOKUP 0  /* committee-cache lookup done                 */
#define HSV_MARK_SLOT 1    /* staging slot leased                         */
#define HSV_MARK_STAGED 2  /* inputs packed into pinned staging           */
#define HSV_MARK_LAUNCH 3  /* kernel launch enqueued                      */
#define HSV_MARK_SYNC 4    /* stream synchronisation returned             */
#define HSV_MARK_DONE 5    /* flags copied out, self-check words read     */
#define HSV_MARKS 6
HSV_API int hsv_host_call_marks(double *out, int cap);

#ifdef __cplusplus
}
#endif

#endif /* HSV_H_ */
