// Block::verify, Timeout::verify and Vote::verify in one verification call
// each (consensus/src/messages.rs:55-76, 250-265, 136-146; the callers are
// handle_proposal, handle_timeout and handle_vote of consensus/src/core.rs).
// Assembled from the three calls a shim would otherwise make -- the author's
// hsv_verify_strict, the QC's hsv_verify_batch_packed, the TC's strict batch
// -- a proposal costs up to three dependent GPU round trips; here all of its
// 1 + n_qc + n_tc signatures go down as one batch with per-item digests.
//
// This file adds no launch path: a batch runs through hsv_verify (the
// automatic committee cache, the latency forms, the resident service; for a
// chain of blocks the pipelined or sharded host path) or, with an explicit
// committee, through hsv_committee_verify by member index.  The batch assembly
// and the reduction of its flags to the reference's verdict are in
// hsv_proposal.hpp, the parsers in hsv_wire_parse.cpp; neither needs a GPU.
// The stake / quorum / authority-reuse checks stay with the caller.
#include <cstring>
#include <string>
#include <vector>

#include "hsv.h"
#include "hsv_host.h"
#include "hsv_internal.h"
#include "hsv_proposal.hpp"
#include "hsv_wire_parse.h"

namespace {

int parse_error(const std::string &what) { return hsvi_set_error(HSV_ERR_PARSE, ("bincode: " + what).c_str()); }

// per-call scratch kept by the thread
struct Scratch {
  hsvp::Items items;
  std::vector<uint8_t> flags, pre;
  std::vector<uint32_t> idx;
  std::vector<hsvp::Layout> layouts;
};
Scratch &scratch() {
  thread_local Scratch s;
  return s;
}

// The batch in ONE verification call; s.flags receives one byte per item.
int run_items(hsv_committee *c, Scratch &s) {
  const hsvp::Items &it = s.items;
  s.flags.assign(it.n, 0);
  if (it.n == 0) return HSV_OK;
  if (!c) return hsv_verify(it.pk.data(), it.sig.data(), it.msg.data(), 32, it.n, s.flags.data());
  // by member index; a stranger gets the first index past the members: flags 0
  const uint32_t none = (uint32_t)hsv_committee_size(c);
  s.idx.resize(it.n);
  for (size_t i = 0; i < it.n; ++i) {
    const int64_t k = hsv_committee_index(c, it.pk.data() + 32 * i);
    s.idx[i] = k < 0 ? none : (uint32_t)k;
  }
  return hsv_committee_verify(c, s.idx.data(), it.sig.data(), it.msg.data(), 32, it.n, s.flags.data());
}

// One object: its items, the call, the verdict.
int verify_object(hsv_committee *c, const hsvp::Object &o, hsv_proposal_result *res, uint8_t *flags_out) {
  Scratch &s = scratch();
  s.items.clear();
  const hsvp::Layout l = hsvp::append(o, s.items);
  const int rc = run_items(c, s);
  if (rc != HSV_OK) return rc;
  const hsv_proposal_result r = hsvp::reduce(l, s.flags.data());
  if (res) *res = r;
  if (flags_out) hsvp::scatter_flags(l, s.flags.data(), flags_out);
  return r.stage == HSV_STAGE_OK ? 1 : 0;
}

bool proposal_args_ok(const hsv_proposal *p) {
  return p && (p->payload || !p->n_payload) && (p->qc_votes || !p->n_qc) &&
         (!p->has_tc || p->tc_votes || !p->n_tc);
}

}  // namespace

extern "C" {

int hsv_proposal_verify(hsv_committee *c, const hsv_proposal *p, hsv_proposal_result *res, uint8_t *flags_out) {
  hsvh::CallScope call;  // the host timeline includes the digests and the assembly
  if (!proposal_args_ok(p)) return hsvi_set_error(HSV_ERR_INVALID_ARG, "null argument");
  return verify_object(c, hsvp::object_of(*p, scratch().pre), res, flags_out);
}

int hsv_block_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len, hsv_proposal_result *res,
                             size_t *n_qc_out, size_t *n_tc_out, uint8_t *pks_out) {
  hsvh::CallScope call;  // the host timeline includes the parse
  if (!buf && len) return hsvi_set_error(HSV_ERR_INVALID_ARG, "null buffer");
  thread_local hsvw::BlockParsed b;  // keeps its vote buffers from call to call
  std::string err;
  if (!hsvw::parse_block(buf, len, b, err)) return parse_error(err);
  const hsv_proposal &p = b.p;
  if (n_qc_out) *n_qc_out = p.n_qc;
  if (n_tc_out) *n_tc_out = p.n_tc;
  if (pks_out) {
    std::memcpy(pks_out, p.author, 32);
    uint8_t *o = pks_out + 32;
    for (size_t i = 0; i < p.n_qc; ++i, o += 32) std::memcpy(o, p.qc_votes + 96 * i, 32);
    for (size_t i = 0; i < p.n_tc; ++i, o += 32) std::memcpy(o, p.tc_votes + 104 * i, 32);
  }
  return verify_object(c, hsvp::object_of(p, scratch().pre), res, nullptr);
}

int hsv_timeout_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len, hsv_proposal_result *res,
                               size_t *n_qc_out, uint8_t *pks_out) {
  hsvh::CallScope call;
  if (!buf && len) return hsvi_set_error(HSV_ERR_INVALID_ARG, "null buffer");
  thread_local hsvw::TimeoutParsed t;
  std::string err;
  if (!hsvw::parse_timeout(buf, len, t, err)) return parse_error(err);
  if (n_qc_out) *n_qc_out = t.n_qc;
  if (pks_out) {
    std::memcpy(pks_out, t.author, 32);
    for (size_t i = 0; i < t.n_qc; ++i) std::memcpy(pks_out + 32 * (i + 1), t.qc_votes.data() + 96 * i, 32);
  }
  hsvp::Object o;
  o.author = t.author;
  o.signature = t.signature;
  hsvp::timeout_digest(t.round, t.qc_round, o.author_digest);
  o.qc_hash = t.qc_hash;
  o.qc_round = t.qc_round;
  o.qc_votes = t.qc_votes.data();
  o.n_qc = t.n_qc;
  return verify_object(c, o, res, nullptr);
}

int hsv_vote_verify_bincode(hsv_committee *c, const uint8_t *buf, size_t len) {
  hsvh::CallScope call;
  if (!buf && len) return hsvi_set_error(HSV_ERR_INVALID_ARG, "null buffer");
  hsvw::VoteParsed v;
  std::string err;
  if (!hsvw::parse_vote(buf, len, v, err)) return parse_error(err);
  if (!c) return hsv_verify_strict(v.digest, v.author, v.signature);
  const int64_t k = hsv_committee_index(c, v.author);
  const uint32_t idx = k < 0 ? (uint32_t)hsv_committee_size(c) : (uint32_t)k;
  uint8_t f = 0;
  const int rc = hsv_committee_verify(c, &idx, v.signature, v.digest, 0, 1, &f);
  if (rc != HSV_OK) return rc;
  return (f & HSV_STRICT_OK) ? 1 : 0;
}

int hsv_blocks_verify_bincode(hsv_committee *c, const uint8_t *bufs, const uint64_t *offsets, size_t n_blocks,
                              hsv_proposal_result *results) {
  hsvh::CallScope call;
  if (n_blocks == 0) return 0;
  if (!offsets) return hsvi_set_error(HSV_ERR_INVALID_ARG, "null offsets");  for (size_t i = 0; i < n_blocks; ++i)
    if (offsets[i + 1] < offsets[i])
      return hsvi_set_error(HSV_ERR_INVALID_ARG, ("block " + std::to_string(i) + ": offsets decrease").c_str());
  if (!bufs && offsets[n_blocks] != offsets[0]) return hsvi_set_error(HSV_ERR_INVALID_ARG, "null buffer");
  Scratch &s = scratch();
  s.items.clear();
  s.layouts.assign(n_blocks, hsvp::Layout());
  std::vector<uint8_t> parsed(n_blocks, 0);
  thread_local hsvw::BlockParsed b;
  std::string err;
  for (size_t i = 0; i < n_blocks; ++i) {
    const size_t len = (size_t)(offsets[i + 1] - offsets[i]);
    if (!hsvw::parse_block(len ? bufs + offsets[i] : nullptr, len, b, err)) continue;
    s.layouts[i] = hsvp::append(hsvp::object_of(b.p, s.pre), s.items);
    parsed[i] = 1;
  }
  const int rc = run_items(c, s);
  if (rc != HSV_OK) return rc;
  int ok = 0;
  for (size_t i = 0; i < n_blocks; ++i) {
    const hsv_proposal_result r =
        parsed[i] ? hsvp::reduce(s.layouts[i], s.flags.data()) : hsv_proposal_result{HSV_STAGE_PARSE, 0};
    if (results) results[i] = r;
    ok += r.stage == HSV_STAGE_OK;
  }
  return ok;
}

}  // extern "C"
