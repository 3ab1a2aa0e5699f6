// What the three committee translation units share (hsv_committee_api.cpp:
// the explicit committee and committee_run; hsv_resident.cpp: the resident
// latency service; hsv_auto_committee.cpp: the automatic cache).  Internal,
// like hsv_host.h, which it brings with it (and hsv.h and hsv_internal.h).
#pragma once
#include "hsv_host.h"

namespace hsvh {

// ---- committee tables on one device ----------------------------------------------
struct CommitteeDev {
  int device = 0;
  uint32_t n = 0;
  const uint8_t *h_pks = nullptr;  // host copy of the n key encodings, by member index
  const uint8_t *d_pks = nullptr;
  const uint8_t *d_kflags = nullptr;
  const uint32_t *const *d_tabptr = nullptr;
  int digit_bits = 8;  // width of the tables behind d_tabptr: 8, or 4 (compact, hsv_committee_create_ex)
};

// ---- hsv_committee_api.cpp ---------------------------------------------------------
// Votes by member index on the committee's device, through a slot of that
// device: the kernels read the pinned staging buffer directly for batches of
// at most kZeroCopyMax votes (the latency path), otherwise via copies.
int committee_run(const CommitteeDev &cd, const uint32_t *key_idx, const uint8_t *sig, size_t sig_stride,
                  const uint8_t *msg, size_t msg_stride, size_t m, uint8_t *flags_out);
// Builds comb tables for `nkeys` encodings already in HBM at d_encs into
// tables[i] (device pointers, host array), flags into d_kflags, on stream st.
// Keys are built in runs of contiguous table memory.  digit_bits: 8, or 4 for
// compact tables (d_tmp sized by the matching hsv_comb*_tmp_bytes(tmp_keys)).
hipError_t build_tables(const uint8_t *d_encs, uint32_t nkeys, uint32_t *const *tables, uint8_t *d_kflags,
                        uint32_t *d_tmp, uint32_t tmp_keys, hipStream_t st, int digit_bits = 8);

// The committee routes of the serialized-batch calls (hsv_batch_api.cpp): the
// handle's device, and the rounds of hsv_committee_verify_transactions_device
// over a span table (transaction i = d_bufs[d_spans[2i], d_spans[2i+1]); every
// flag byte of the n transactions is written; device c current, its two B
// tables ensured by the caller).
int committee_device_of(const hsv_committee *cm);
// The handle's key table for the signer census (hsv_census_api.cpp), which
// leaves a committee's members out: keytab_find's arguments (hsv_keytab.hpp;
// the table was built under KeyHash::seed()).  n == 0: an empty committee, the
// pointers are NULL.
struct CommitteeKeys {
  int device = 0;
  uint32_t n = 0;
  const uint32_t *d_keytab = nullptr;
  uint32_t keymask = 0;
  const uint8_t *d_pks = nullptr;
};
CommitteeKeys committee_keys_of(const hsv_committee *cm);
int committee_tx_spans_enqueue(const hsv_committee *cm, DevCtx &c, const uint32_t *btable, const uint32_t *comb16,
                               const uint8_t *d_bufs, const uint64_t *d_spans, size_t n, uint8_t *d_flags,
                               uint32_t *d_fault, hipStream_t s);

// ---- hsv_resident.cpp --------------------------------------------------------------
constexpr int kResidentUnavailable = 1;
// One request of at most hsv_comb_resident_votes() votes: HSV_OK, an error
// (HSV_ERR_DEVICE_FAULT from the self-checks or the kernel's request check),
// or kResidentUnavailable (the caller launches instead).
int resident_run(const CommitteeDev &cd, const uint32_t *key_idx, const uint8_t *sig, size_t sig_stride,
                 const uint8_t *msg, size_t msg_stride, size_t m, uint8_t *flags_out, const uint32_t *btable);
bool resident_enabled();
// Stop the kernel and wait for its grid, whether or not it reports alive
// (hsv_shutdown); resident_quiesce() stops only a block that does.
void resident_stop();

}  // namespace hsvh
