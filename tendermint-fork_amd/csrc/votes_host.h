// votes_host.h — free-standing votes on the host: the request checks of tmed_verify_votes, the
// staging of a vote into the record vote_free.h reads (its bytes: vote_wire.h), and the host entries tmed_votes_sign_bytes /
// tmed_verify_votes_host, which run the shared source lane by lane with no device (votes.hip holds
// the kernel and the device batch; tests/native/votes_host.cpp compiles this header on its own).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tmed25519.h"
#include "vote_free.h"

namespace tmed_votes_host {

using tmed::VoteRec;
using tmed::VoteStep;

static_assert(tmed::kVoteOk == TMED_VOTE_OK && tmed::kVoteIndexNegative == TMED_VOTE_INDEX_NEGATIVE &&
                  tmed::kVoteAddressEmpty == TMED_VOTE_ADDRESS_EMPTY &&
                  tmed::kVoteUnexpectedStep == TMED_VOTE_UNEXPECTED_STEP &&
                  tmed::kVoteIndexNotInSet == TMED_VOTE_INDEX_NOT_IN_SET &&
                  tmed::kVoteAddressNotInSet == TMED_VOTE_ADDRESS_NOT_IN_SET &&
                  tmed::kVoteAddressNotOfKey == TMED_VOTE_ADDRESS_NOT_OF_KEY && tmed::kVotePanic == TMED_VOTE_PANIC &&
                  tmed::kVoteInvalidSignature == TMED_VOTE_INVALID_SIGNATURE && tmed::kVoteGoPath == TMED_VOTE_GO_PATH &&
                  tmed::kVoteFlagAddVote == TMED_VOTES_ADDVOTE,
              "vote_free.h codes are the header's");

inline bool votes_arrays_ok(const tmed_votes &v) {
  return v.n == 0 || (v.types && v.heights && v.rounds && v.block_hashes && v.psh_totals && v.psh_hashes &&
                      v.ts_seconds && v.ts_nanos && v.addresses && v.validator_indexes && v.sigs);
}
// the arrays VoteSignBytes reads
inline bool votes_sign_arrays_ok(const tmed_votes &v) {
  return v.n == 0 || (v.types && v.heights && v.rounds && v.block_hashes && v.psh_totals && v.psh_hashes &&
                      v.ts_seconds && v.ts_nanos);
}

inline int check_request(const tmed_vote_request &r) {
  if (!r.vals || !r.votes || (r.chain_id_len && !r.chain_id)) return TMED_EINVAL;
  if (!votes_arrays_ok(*r.votes) || r.votes->n > 0x7fffffffu) return TMED_EINVAL;
  if (r.vals->n > 0x7fffffffu || (r.vals->n && !r.vals->pubkeys)) return TMED_EINVAL;
  if ((r.flags & TMED_VOTES_ADDVOTE) && r.vals->n && !r.vals->addresses) return TMED_EINVAL;
  return TMED_OK;
}

inline uint8_t clip_len(uint32_t len) { return (uint8_t)(len > 255 ? 255 : len); }

// The reference's length rule: a signature whose length is not 64 is rejected (crypto/ed25519/ed25519.go:150-152).
inline bool sig_full(const tmed_votes &v, size_t i) { return !v.sig_lens || v.sig_lens[i] == 64; }
// Vote i's signature as the verify kernels read it: 64 bytes, a shorter one padded with zeros.
inline void vote_sig(const tmed_votes &v, size_t i, uint8_t *out) {
  const uint32_t sl = v.sig_lens ? v.sig_lens[i] : 64;
  memcpy(out, v.sigs + 64 * i, sl < 64 ? sl : 64);
  if (sl < 64) memset(out + sl, 0, 64 - sl);
}
// A key's 32 bytes as the eight little-endian words the address check hashes (the device twin:
// slot_rows.h key_words).
inline void key_words(const uint8_t *k, uint32_t w[8]) {
  for (int j = 0; j < 8; j++)
    w[j] = (uint32_t)k[4 * j] | ((uint32_t)k[4 * j + 1] << 8) | ((uint32_t)k[4 * j + 2] << 16) | ((uint32_t)k[4 * j + 3] << 24);
}

// The fields VoteSignBytes reads of vote i.
inline void fill_sign_fields(const tmed_votes &v, size_t i, VoteRec &r) {
  memset(&r, 0, sizeof(r));
  r.type = v.types[i];
  r.height = v.heights[i];
  r.round = v.rounds[i];
  r.sec = v.ts_seconds[i];
  r.nanos = v.ts_nanos[i];
  r.psh_total = v.psh_totals[i];
  const uint32_t hl = v.block_hash_lens ? v.block_hash_lens[i] : 32, pl = v.psh_hash_lens ? v.psh_hash_lens[i] : 32;
  r.hash_len = clip_len(hl);
  r.psh_len = clip_len(pl);
  memcpy(r.hash, v.block_hashes + 32 * i, hl < 32 ? hl : 32);
  memcpy(r.psh, v.psh_hashes + 32 * i, pl < 32 ? pl : 32);
}

// Vote i of request `req` as the kernel's record (key: its validator's index in the key set, keyed route).
inline void fill_rec(const tmed_votes &v, size_t i, uint32_t req, uint32_t key, VoteRec &r) {
  fill_sign_fields(v, i, r);
  const uint32_t al = v.address_lens ? v.address_lens[i] : 20;
  r.addr_len = clip_len(al);
  memcpy(r.addr, v.addresses + 20 * i, al < 20 ? al : 20);
  r.val_index = v.validator_indexes[i];
  r.sig_full = sig_full(v, i);
  r.key = key;
  r.req = req;
}

// The request's side of the checks; the chain ID is copied when it fits the record (the device route).
inline bool device_route(const tmed_vote_request &q) { return q.chain_id_len <= tmed::kVoteChainMax; }
inline void fill_step(const tmed_vote_request &q, uint64_t addr_base, VoteStep &s) {
  memset(&s, 0, sizeof(s));
  s.height = q.height;
  s.round = q.round;
  s.type = q.msg_type;
  s.flags = q.flags;
  s.cid_len = q.chain_id_len;
  s.n_vals = (uint32_t)q.vals->n;
  s.addr_base = addr_base;
  if (device_route(q) && q.chain_id_len) memcpy(s.chain, q.chain_id, q.chain_id_len);
}

// request_prechecks (below) as votes_host.cpp exports it to the HIP units: the device batch's host
// route calls it for requests whose chain ID the slots cannot hold.
void request_prechecks_host(const tmed_vote_request &q, uint8_t *codes);

// Everything below runs SHA-256 on the host, so it is compiled as plain C++ only (votes_host.cpp,
// tests/native/votes_host.cpp): in a HIP unit sha256.h's round constants are a __constant__ device
// table, whose host-side shadow holds no data.
#if !defined(__HIPCC__)
// Checks 1-7 of vote i of request q on the host (the key read from the request's set).
inline uint8_t precheck_host(const tmed_vote_request &q, const VoteStep &s, const VoteRec &r) {
  const tmed_valset &vs = *q.vals;
  return tmed::vote_prechecks(r, s, vs.addresses, [&](uint32_t w[8]) { key_words(vs.pubkeys + 32 * (size_t)r.val_index, w); });
}

// The checks of every vote of request q, codes[i] for vote i.
inline void request_prechecks(const tmed_vote_request &q, uint8_t *codes) {
  VoteStep s;
  fill_step(q, 0, s);
  const tmed_votes &v = *q.votes;
  for (size_t i = 0; i < v.n; i++) {
    VoteRec r;
    fill_rec(v, i, 0, 0, r);
    codes[i] = precheck_host(q, s, r);
  }
}

inline int verify_votes_host(const tmed_vote_request *reqs, size_t n_reqs, uint8_t *codes, uint32_t *msg_lens,
                             uint8_t *route) {
  if (n_reqs && !reqs) return TMED_EINVAL;
  size_t total = 0;
  for (size_t q = 0; q < n_reqs; q++) {
    if (check_request(reqs[q]) != TMED_OK) return TMED_EINVAL;
    total += reqs[q].votes->n;
  }
  if (total && !codes) return TMED_EINVAL;
  size_t k = 0;
  for (size_t q = 0; q < n_reqs; q++) {
    VoteStep s;
    fill_step(reqs[q], 0, s);
    if (route) route[q] = device_route(reqs[q]);
    const tmed_votes &v = *reqs[q].votes;
    for (size_t i = 0; i < v.n; i++, k++) {
      VoteRec r;
      fill_rec(v, i, (uint32_t)q, 0, r);
      codes[k] = precheck_host(reqs[q], s, r);
      if (msg_lens) msg_lens[k] = codes[k] ? 0 : tmed::vote_free_size(r, reqs[q].chain_id_len);
    }
  }
  return TMED_OK;
}

#endif  // !__HIPCC__

inline int votes_sign_bytes(const char *chain_id, uint32_t chain_id_len, const tmed_votes *v, uint8_t *out,
                            size_t out_cap, uint32_t *out_off, size_t *out_len, uint8_t *malformed) {
  if (!v || (chain_id_len && !chain_id) || !votes_sign_arrays_ok(*v) || (v->n && !out_off)) return TMED_EINVAL;
  size_t pos = 0;
  for (size_t i = 0; i < v->n; i++) {
    VoteRec r;
    fill_sign_fields(*v, i, r);
    out_off[i] = (uint32_t)pos;
    const bool bad = tmed::vote_bid_malformed(r);
    if (malformed) malformed[i] = bad;
    if (bad) {
      if (!malformed) return TMED_EINVAL;  // CanonicalizeBlockID panics (types/canonical.go:19-22)
      continue;
    }
    const size_t len = tmed::vote_free_size(r, chain_id_len);
    if (out && pos + len <= out_cap) tmed::vote_free_write(r, (const uint8_t *)chain_id, chain_id_len, out + pos);
    pos += len;
    if (pos > 0xffffffffu) return TMED_EINVAL;
  }
  if (v->n) out_off[v->n] = (uint32_t)pos;
  if (out_len) *out_len = pos;
  return (out && pos > out_cap) ? TMED_ENOMEM : TMED_OK;
}

}  // namespace tmed_votes_host
