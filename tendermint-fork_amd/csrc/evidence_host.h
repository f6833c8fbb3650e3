// evidence_host.h — DuplicateVoteEvidence on the host: the request checks of
// tmed_verify_duplicate_votes and tmed_evidence_hashes, the staging of an evidence into the records
// evidence_free.h reads, and the host entries tmed_evidence_bytes / tmed_verify_duplicate_votes_host,
// which run the shared source lane by lane with no device (evidence.hip holds the kernels and the
// device batches; tests/native/evidence_host.cpp compiles this header on its own).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tmed25519.h"
#include "evidence_free.h"
#include "votes_host.h"

namespace tmed_evidence_host {

using tmed::EvRec;
using tmed::EvStep;
using tmed::VoteRec;

static_assert(tmed::kEvOk == TMED_DUPVOTE_OK && tmed::kEvNotAValidator == TMED_DUPVOTE_NOT_A_VALIDATOR &&
                  tmed::kEvHrsMismatch == TMED_DUPVOTE_HRS_MISMATCH &&
                  tmed::kEvAddressMismatch == TMED_DUPVOTE_ADDRESS_MISMATCH &&
                  tmed::kEvSameBlockId == TMED_DUPVOTE_SAME_BLOCK_ID &&
                  tmed::kEvAddressNotOfKey == TMED_DUPVOTE_ADDRESS_NOT_OF_KEY &&
                  tmed::kEvValidatorPower == TMED_DUPVOTE_VALIDATOR_POWER &&
                  tmed::kEvTotalPower == TMED_DUPVOTE_TOTAL_POWER && tmed::kEvPanic == TMED_DUPVOTE_PANIC &&
                  tmed::kEvVoteASignature == TMED_DUPVOTE_VOTE_A_SIGNATURE &&
                  tmed::kEvVoteBSignature == TMED_DUPVOTE_VOTE_B_SIGNATURE && tmed::kEvGoPath == TMED_DUPVOTE_GO_PATH,
              "evidence_free.h codes are the header's");

inline bool evidence_arrays_ok(const tmed_dup_evidence &e) {
  if (e.votes.n != 2 * e.n || e.n > 0x3fffffffu) return false;
  if (e.n == 0) return true;
  return tmed_votes_host::votes_arrays_ok(e.votes) && e.total_voting_powers && e.validator_powers && e.ts_seconds &&
         e.ts_nanos;
}

inline int check_request(const tmed_dup_request &r) {
  if (!r.vals || !r.ev || (r.chain_id_len && !r.chain_id)) return TMED_EINVAL;
  if (!evidence_arrays_ok(*r.ev)) return TMED_EINVAL;
  if (r.vals->n > 0x7fffffffu || (r.vals->n && (!r.vals->pubkeys || !r.vals->addresses || !r.vals->powers)))
    return TMED_EINVAL;
  return TMED_OK;
}

// Evidence i of request `req`: its two votes as the kernels' records (va, vb) and its own fields.
inline void fill_evidence(const tmed_dup_evidence &e, size_t i, uint32_t req, VoteRec &va, VoteRec &vb, EvRec &r) {
  const tmed_votes &v = e.votes;
  tmed_votes_host::fill_rec(v, 2 * i, req, 0, va);
  tmed_votes_host::fill_rec(v, 2 * i + 1, req, 0, vb);
  memset(&r, 0, sizeof(r));
  r.total_power = e.total_voting_powers[i];
  r.val_power = e.validator_powers[i];
  r.sec = e.ts_seconds[i];
  r.nanos = e.ts_nanos[i];
  r.req = req;
  for (size_t k = 0; k < 2; k++) {
    r.hash_len[k] = v.block_hash_lens ? v.block_hash_lens[2 * i + k] : 32;
    r.psh_len[k] = v.psh_hash_lens ? v.psh_hash_lens[2 * i + k] : 32;
    r.addr_len[k] = v.address_lens ? v.address_lens[2 * i + k] : 20;
    r.sig_len[k] = v.sig_lens ? v.sig_lens[2 * i + k] : 64;
  }
}

inline bool device_route(const tmed_dup_request &q) { return q.chain_id_len <= tmed::kVoteChainMax; }
inline void fill_step(const tmed_dup_request &q, uint64_t addr_base, EvStep &s) {
  memset(&s, 0, sizeof(s));
  s.total_power = q.vals->total_power;
  s.addr_base = addr_base;
  s.n_vals = (uint32_t)q.vals->n;
  s.cid_len = q.chain_id_len;
  if (device_route(q) && q.chain_id_len) memcpy(s.chain, q.chain_id, q.chain_id_len);
}

// GetByAddress (types/validator_set.go:270-278): the first validator, in index order, whose address
// equals the vote's under bytes.Equal; a vote address of any length but 20 matches none.
inline uint32_t lookup_host(const tmed_valset &vs, const VoteRec &va, const EvRec &r) {
  if (r.addr_len[0] != 20) return tmed::kEvNone;
  for (size_t v = 0; v < vs.n; v++)
    if (memcmp(vs.addresses + 20 * v, va.addr, 20) == 0) return (uint32_t)v;
  return tmed::kEvNone;
}

// One evidence's side of the host results.
struct HostLane {
  uint8_t pre, state[2];
  uint32_t found, len[2];
};

// evidence_lanes (below) as evidence_host.cpp exports it to the HIP units: the device batch's host
// route calls it for requests whose chain ID the slots cannot hold.
void request_lanes_host(const tmed_dup_request &q, HostLane *lanes);

// Everything below runs SHA-256 on the host, so it is compiled as plain C++ only (evidence_host.cpp,
// tests/native/evidence_host.cpp), as the second half of votes_host.h is.
#if !defined(__HIPCC__)
inline void lane_host(const tmed_dup_request &q, const EvStep &s, const VoteRec &va, const VoteRec &vb, const EvRec &r,
                      HostLane &out) {
  const tmed_valset &vs = *q.vals;
  const uint32_t found = lookup_host(vs, va, r);
  out.found = found;
  out.pre = tmed::ev_prechecks(va, vb, r, s, found, found == tmed::kEvNone ? 0 : vs.powers[found],
                               [&](uint32_t w[8]) { tmed_votes_host::key_words(vs.pubkeys + 32 * (size_t)found, w); });
  const VoteRec *vr[2] = {&va, &vb};
  for (int k = 0; k < 2; k++) {
    out.state[k] = tmed::ev_vote_state(*vr[k]);
    out.len[k] = (out.pre || out.state[k]) ? 0 : tmed::vote_free_size(*vr[k], q.chain_id_len);
  }
}

// Every evidence of request q.
inline void request_lanes(const tmed_dup_request &q, HostLane *lanes) {
  EvStep s;
  fill_step(q, 0, s);
  for (size_t i = 0; i < q.ev->n; i++) {
    VoteRec va, vb;
    EvRec r;
    fill_evidence(*q.ev, i, 0, va, vb, r);
    lane_host(q, s, va, vb, r, lanes[i]);
  }
}

inline int verify_duplicate_votes_host(const tmed_dup_request *reqs, size_t n_reqs, uint8_t *pre_codes,
                                       uint8_t *vote_states, int32_t *found, uint32_t *msg_lens, uint8_t *route) {
  if (n_reqs && !reqs) return TMED_EINVAL;
  size_t total = 0;
  for (size_t q = 0; q < n_reqs; q++) {
    if (check_request(reqs[q]) != TMED_OK) return TMED_EINVAL;
    total += reqs[q].ev->n;
  }
  if (total && !pre_codes) return TMED_EINVAL;
  size_t k = 0;
  std::vector<HostLane> lanes;
  for (size_t q = 0; q < n_reqs; q++) {
    if (route) route[q] = device_route(reqs[q]);
    lanes.resize(reqs[q].ev->n);
    request_lanes(reqs[q], lanes.data());
    for (const HostLane &l : lanes) {
      pre_codes[k] = l.pre;
      if (vote_states) vote_states[2 * k] = l.state[0], vote_states[2 * k + 1] = l.state[1];
      if (found) found[k] = l.found == tmed::kEvNone ? -1 : (int32_t)l.found;
      if (msg_lens) msg_lens[2 * k] = l.len[0], msg_lens[2 * k + 1] = l.len[1];
      k++;
    }
  }
  return TMED_OK;
}
#endif  // !__HIPCC__

inline int evidence_bytes(const tmed_dup_evidence *e, uint8_t *out, size_t out_cap, uint32_t *out_off, size_t *out_len,
                          uint8_t *ok) {
  if (!e || !evidence_arrays_ok(*e) || (e->n && !out_off)) return TMED_EINVAL;
  size_t pos = 0;
  for (size_t i = 0; i < e->n; i++) {
    VoteRec va, vb;
    EvRec r;
    fill_evidence(*e, i, 0, va, vb, r);
    out_off[i] = (uint32_t)pos;
    const bool can = tmed::evidence_encodable(va, vb, r);
    if (ok) ok[i] = can;
    if (!can) {
      if (!ok) return TMED_EINVAL;  // Bytes() panics, or the struct does not carry the bytes
      continue;
    }
    const size_t len = tmed::evidence_size(va, vb, r);
    if (out && pos + len <= out_cap)
      tmed::evidence_write(va, vb, r, e->votes.sigs + 64 * (2 * i), e->votes.sigs + 64 * (2 * i + 1), out + pos);
    pos += len;
    if (pos > 0xffffffffu) return TMED_EINVAL;
  }
  if (e->n) out_off[e->n] = (uint32_t)pos;
  if (out_len) *out_len = pos;
  return (out && pos > out_cap) ? TMED_ENOMEM : TMED_OK;
}

}  // namespace tmed_evidence_host
