// validate_host.h — validateBlock (state/validation.go:15-151) and the Block.ValidateBasic it runs first
// (types/block.go:55-106) replayed on the host over hashes, compare masks, commit outcomes, medians and
// proposer lookups computed elsewhere: the host half of tmed_validate_blocks / tmed_validate_blocks_with
// (include/tmed25519.h has the outcome codes and cites each check's lines).  Host C++ only (no HIP):
// commit.hip and validate.hip include it for the device entry, validate_host.cpp for
// tmed_validate_blocks_with, and tests/native/validate_host.cpp compiles the same code with stub
// hashes and a stub verifier under AddressSanitizer and UndefinedBehaviorSanitizer.
//
// validate_run does, in the reference's order:
//   1. per request, the two basic checks (header_basic_ok, commit_basic_ok);
//   A. `hashes`: for the requests that pass them, Commit.Hash, Data.Hash, EvidenceList.Hash, Header.Hash
//      of the block before every linked request, ValidatorSet.Hash of the known sets, and the mask of
//      the compares that failed (block_check_kernel on the device, host_masks here for the _with entry);
//   2. the checks from LAST_COMMIT_HASH through INITIAL_HAS_SIGS;
//   B. `verify`: VerifyCommit of the requests still undecided, as one batch of tmed_commit_requests;
//      `tail`: MedianTime of those whose commit verified and, where `hashes` has not looked them up already, their proposers;
//   3. LAST_COMMIT through EVIDENCE_OVERFLOW.
#pragma once

#include <string.h>

#include <vector>

#include "../../include/tmed25519.h"
#include "light_host.h"

namespace tmed_validate {

using tmed_light::bytes_equal;
using tmed_light::GoTime;
using tmed_light::time_after;
using tmed_light::time_ok;

// The compares of one block, as bits of its mask (a set bit: the two 32-byte values differ) and of its
// enable word (a set bit: both values are 32 bytes long and the compare is the kernel's to make).
constexpr uint32_t kCmpCommit = 1u, kCmpData = 2u, kCmpEvidence = 4u, kCmpVals = 8u, kCmpNext = 16u, kCmpLink = 32u;
constexpr int kCompares = 6;
constexpr uint32_t kCmpLookup = 1u << 31;  // enable word only: look ProposerAddress up in the set
// tmed_header.hashes[] by name
constexpr int kHLastCommit = 0, kHData = 1, kHVals = 2, kHNext = 3, kHConsensus = 4, kHApp = 5, kHResults = 6,
              kHEvidence = 7, kHProposer = 8;

constexpr uint8_t kEmptyHash[32] = {0xe3, 0xb0, 0xc4, 0x42, 0x98, 0xfc, 0x1c, 0x14, 0x9a, 0xfb, 0xf4, 0xc8, 0x99, 0x6f, 0xb9, 0x24,
                                    0x27, 0xae, 0x41, 0xe4, 0x64, 0x9b, 0x93, 0x4c, 0xa4, 0x95, 0x99, 0x1b, 0x78, 0x52, 0xb8, 0x55};

inline bool linked(const tmed_block_request &r) { return (r.flags & TMED_VB_LINK_PREV) != 0; }
inline bool knows(const tmed_block_request &r, uint32_t bit) { return (r.state->known & bit) != 0; }
inline bool valset_hash_ok(const tmed_valset *v) { return v && (!v->n || (v->pubkeys && v->powers)); }

// What every entry reads of the call: TMED_EINVAL for a NULL struct or array, unknown bits, a link on block 0.
inline int check_call(const tmed_block_batch *b, const tmed_block_result *out) {
  if (!b) return TMED_EINVAL;
  if (b->n == 0) return TMED_OK;
  if (!b->blocks || !out || b->n > 0x7fffffffu) return TMED_EINVAL;
  for (size_t i = 0; i < b->n; i++) {
    const tmed_block_request &r = b->blocks[i];
    if (!r.header || !r.state || (r.flags & ~TMED_VB_LINK_PREV) || (i == 0 && linked(r))) return TMED_EINVAL;
    const tmed_header &h = *r.header;
    const tmed_block_state &s = *r.state;
    for (int k = 0; k < 9; k++)
      if (h.hash_lens[k] && !h.hashes[k]) return TMED_EINVAL;
    if ((h.chain_id_len && !h.chain_id) || (h.last_block_id.hash_len && !h.last_block_id.hash) ||
        (h.last_block_id.psh_hash_len && !h.last_block_id.psh_hash))
      return TMED_EINVAL;
    if ((s.known & ~TMED_VB_KNOW_ALL) || (s.chain_id_len && !s.chain_id)) return TMED_EINVAL;
    if ((s.last_block_id.hash_len && !s.last_block_id.hash) || (s.last_block_id.psh_hash_len && !s.last_block_id.psh_hash))
      return TMED_EINVAL;
    if ((s.app_hash_len && !s.app_hash) || (s.last_results_hash_len && !s.last_results_hash)) return TMED_EINVAL;
    if ((s.known & TMED_VB_KNOW_CONSENSUS_HASH) && !s.consensus_hash) return TMED_EINVAL;
    if ((s.known & TMED_VB_KNOW_VALIDATORS) &&
        (!valset_hash_ok(s.validators) || s.validators->n > 0x7fffffffu || (s.validators->n && !s.validators->addresses)))
      return TMED_EINVAL;
    if ((s.known & TMED_VB_KNOW_NEXT_VALIDATORS) && !valset_hash_ok(s.next_validators)) return TMED_EINVAL;
    if (r.commit_basic_ok) {
      if (!r.last_commit) return TMED_EINVAL;
      const tmed_commit &c = *r.last_commit;
      if (c.n_sigs > 0xffffffffu || (c.n_sigs && (!c.flags || !c.ts_seconds || !c.ts_nanos || !c.addresses || !c.sigs)))
        return TMED_EINVAL;
      const tmed_valset *lv = s.last_validators;
      if (h.height != s.initial_height && (!lv || (lv->n && (!lv->pubkeys || !lv->powers || !lv->addresses))))
        return TMED_EINVAL;
    }
  }
  // the transactions and the evidence lists: the arrays of tmed_txs_hashes / tmed_evidence_hashes
  if (b->block_off) {
    if (!b->tx_off || b->block_off[0] != 0) return TMED_EINVAL;
    for (size_t i = 0; i < b->n; i++)
      if (b->block_off[i + 1] < b->block_off[i]) return TMED_EINVAL;
    const size_t L = b->block_off[b->n];
    for (size_t k = 0; k < L; k++)
      if (b->tx_off[k + 1] < b->tx_off[k] || b->tx_off[k + 1] - b->tx_off[k] > 0xffffffffu - 64) return TMED_EINVAL;
    if (L && b->tx_off[L] > b->tx_off[0] && !b->txs) return TMED_EINVAL;
  }
  if (b->list_off) {
    if (!b->ev || b->list_off[0] != 0) return TMED_EINVAL;
    for (size_t i = 0; i < b->n; i++)
      if (b->list_off[i + 1] < b->list_off[i]) return TMED_EINVAL;
    const size_t K = b->list_off[b->n];
    if (K && !b->items) return TMED_EINVAL;
    size_t n_op = 0;
    for (size_t k = 0; k < K; k++) {
      if (b->items[k] >= 0 && (uint64_t)b->items[k] >= b->ev->n) return TMED_EINVAL;
      if (b->items[k] < 0) {
        const uint64_t j = (uint64_t)(-1 - b->items[k]);
        if (j >= 0x7fffffffu) return TMED_EINVAL;
        if (j + 1 > n_op) n_op = (size_t)j + 1;
      }
    }
    if (n_op) {
      if (!b->opaque_off) return TMED_EINVAL;
      for (size_t j = 0; j < n_op; j++)
        if (b->opaque_off[j + 1] < b->opaque_off[j]) return TMED_EINVAL;
      if (b->opaque_off[n_op] > b->opaque_off[0] && !b->opaque) return TMED_EINVAL;
    }
  }
  return TMED_OK;
}

// Phase A's work list.
struct Plan {
  const tmed_block_batch *b;
  std::vector<size_t> need;      // the requests that pass both basic checks
  std::vector<size_t> need_hdr;  // the requests whose Header.Hash a linked request of `need` reads
};

// Phase A's results, arrays of n entries indexed by request (32 bytes a hash).  ok = 0: Commit.Hash /
// EvidenceList.Hash cannot be reproduced from the structs; Header.Hash is nil.
struct Hashes {
  std::vector<uint8_t> commit, commit_ok, data, evidence, evidence_ok, header, header_ok, vals, next;
  std::vector<uint32_t> enable, mask;  // kCmp* bits
  std::vector<int32_t> proposer;       // where enable has kCmpLookup and have_proposer: the found index or -1
  bool have_proposer = false;
  explicit Hashes(size_t n)
      : commit(32 * n), commit_ok(n), data(32 * n), evidence(32 * n), evidence_ok(n), header(32 * n), header_ok(n),
        vals(32 * n), next(32 * n), enable(n), mask(n), proposer(n, -1) {}
};

// The header's value of compare slot s and its length.
inline const uint8_t *want_of(const tmed_header &h, int s, uint32_t *len) {
  static const int field[5] = {kHLastCommit, kHData, kHEvidence, kHVals, kHNext};
  if (s == 5) {
    *len = h.last_block_id.hash_len;
    return h.last_block_id.hash;
  }
  *len = h.hash_lens[field[s]];
  return h.hashes[field[s]];
}
// The computed value of slot s for request i, or nullptr where there is none.
inline const uint8_t *got_of(const tmed_block_batch &b, const Hashes &H, size_t i, int s) {
  const tmed_block_request &r = b.blocks[i];
  switch (s) {
    case 0: return H.commit_ok[i] ? &H.commit[32 * i] : nullptr;
    case 1: return &H.data[32 * i];
    case 2: return H.evidence_ok[i] ? &H.evidence[32 * i] : nullptr;
    case 3: return knows(r, TMED_VB_KNOW_VALIDATORS) ? &H.vals[32 * i] : nullptr;
    case 4: return knows(r, TMED_VB_KNOW_NEXT_VALIDATORS) ? &H.next[32 * i] : nullptr;
    default: return linked(r) && H.header_ok[i - 1] ? &H.header[32 * (i - 1)] : nullptr;
  }
}

// The enable words of the plan's requests, from the hashes' ok bytes: slot s is the kernel's iff both
// values exist and the header's is 32 bytes long; the lookup iff the set is known and the address is
// 20 bytes long.
inline void fill_enable(const Plan &p, Hashes &H) {
  for (const size_t i : p.need) {
    const tmed_block_request &r = p.b->blocks[i];
    uint32_t en = 0;
    for (int s = 0; s < kCompares; s++) {
      uint32_t len;
      (void)want_of(*r.header, s, &len);
      if (len == 32 && got_of(*p.b, H, i, s)) en |= 1u << s;
    }
    if (knows(r, TMED_VB_KNOW_VALIDATORS) && r.header->hash_lens[kHProposer] == 20) en |= kCmpLookup;
    H.enable[i] = en;
  }
}

// block_check_kernel's compares on the host (the _with entry, the stand-alone program).
inline void host_masks(const Plan &p, Hashes &H) {
  fill_enable(p, H);
  for (const size_t i : p.need) {
    uint32_t m = 0;
    for (int s = 0; s < kCompares; s++) {
      if (!(H.enable[i] >> s & 1)) continue;
      uint32_t len;
      const uint8_t *want = want_of(*p.b->blocks[i].header, s, &len);
      if (memcmp(want, got_of(*p.b, H, i, s), 32) != 0) m |= 1u << s;
    }
    H.mask[i] = m;
  }
}

// HasAddress by the reference's scan (types/validator_set.go:262-268): the first index, or -1.
inline int32_t proposer_scan(const tmed_valset &v, const uint8_t *addr) {
  for (size_t k = 0; k < v.n; k++)
    if (memcmp(v.addresses + 20 * k, addr, 20) == 0) return (int32_t)k;
  return -1;
}

// The state a request is validated against: the struct's, or block i-1's under TMED_VB_LINK_PREV.
struct Eff {
  int64_t last_height;
  GoTime last_time;
};
inline Eff eff_state(const tmed_block_batch &b, size_t i) {
  const tmed_block_request &r = b.blocks[i];
  if (linked(r)) {
    const tmed_header &p = *b.blocks[i - 1].header;
    return Eff{p.height, GoTime{p.time_seconds, p.time_nanos}};
  }
  return Eff{r.state->last_block_height, GoTime{r.state->last_block_time_seconds, r.state->last_block_time_nanos}};
}

// One hash compare of the replay.  Returns 0: equal; 1: a mismatch (o.hash holds the computed value).
inline int hash_compare(const tmed_block_batch &b, const Hashes &H, size_t i, int s, tmed_block_result &o) {
  uint32_t len;
  const uint8_t *want = want_of(*b.blocks[i].header, s, &len);
  (void)want;
  const uint8_t *got = got_of(b, H, i, s);
  bool differ;
  if (!got) differ = len != 0;  // only the link's nil Header.Hash comes here: it compares as empty bytes
  else if (len != 32) differ = true;
  else differ = (H.mask[i] >> s & 1) != 0;
  if (!differ) return 0;
  o.hash_len = got ? 32 : 0;
  if (got) memcpy(o.hash, got, 32);
  return 1;
}

// Step 2 for a request that passed the basic checks.  Returns its outcome, or -1: phase B decides.
inline int checks_before_commit(const tmed_block_batch &b, const Hashes &H, size_t i, tmed_block_result &o) {
  const tmed_block_request &r = b.blocks[i];
  const tmed_header &h = *r.header;
  const tmed_block_state &s = *r.state;
  const Eff e = eff_state(b, i);
  if (!H.commit_ok[i]) return TMED_VB_GO_PATH;
  if (hash_compare(b, H, i, 0, o)) return TMED_VB_LAST_COMMIT_HASH;
  if (hash_compare(b, H, i, 1, o)) return TMED_VB_DATA_HASH;
  if (r.evidence_basic_bad >= 0) {
    o.idx = r.evidence_basic_bad;
    return TMED_VB_EVIDENCE_BASIC;
  }
  if (!H.evidence_ok[i]) return TMED_VB_GO_PATH;
  if (hash_compare(b, H, i, 2, o)) return TMED_VB_EVIDENCE_HASH;
  if (h.version_app != s.version_app || h.version_block != s.version_block) return TMED_VB_VERSION;
  if (!bytes_equal((const uint8_t *)h.chain_id, h.chain_id_len, (const uint8_t *)s.chain_id, s.chain_id_len))
    return TMED_VB_CHAIN_ID;
  if (e.last_height == 0 && h.height != s.initial_height) return TMED_VB_HEIGHT_INITIAL;
  if (e.last_height > 0 && h.height != (int64_t)((uint64_t)e.last_height + 1)) return TMED_VB_HEIGHT;
  // BlockID.Equals (types/block.go:1170-1173): the PartSetHeader, then the hash
  const tmed_block_id &a = h.last_block_id, &w = s.last_block_id;
  bool same = a.psh_total == w.psh_total && bytes_equal(a.psh_hash, a.psh_hash_len, w.psh_hash, w.psh_hash_len);
  if (linked(r)) {
    if (hash_compare(b, H, i, 5, o)) return TMED_VB_LAST_BLOCK_ID;
    if (!same) {
      o.hash_len = H.header_ok[i - 1] ? 32 : 0;
      if (o.hash_len) memcpy(o.hash, &H.header[32 * (i - 1)], 32);
    }
  } else {
    same = same && bytes_equal(a.hash, a.hash_len, w.hash, w.hash_len);
  }
  if (!same) return TMED_VB_LAST_BLOCK_ID;
  if (!knows(r, TMED_VB_KNOW_APP_HASH)) o.skipped |= TMED_VB_KNOW_APP_HASH;
  else if (!bytes_equal(h.hashes[kHApp], h.hash_lens[kHApp], s.app_hash, s.app_hash_len)) return TMED_VB_APP_HASH;
  if (!knows(r, TMED_VB_KNOW_CONSENSUS_HASH)) o.skipped |= TMED_VB_KNOW_CONSENSUS_HASH;
  else if (!bytes_equal(h.hashes[kHConsensus], h.hash_lens[kHConsensus], s.consensus_hash, 32)) return TMED_VB_CONSENSUS_HASH;
  if (!knows(r, TMED_VB_KNOW_LAST_RESULTS_HASH)) o.skipped |= TMED_VB_KNOW_LAST_RESULTS_HASH;
  else if (!bytes_equal(h.hashes[kHResults], h.hash_lens[kHResults], s.last_results_hash, s.last_results_hash_len))
    return TMED_VB_LAST_RESULTS_HASH;
  if (!knows(r, TMED_VB_KNOW_VALIDATORS)) o.skipped |= TMED_VB_KNOW_VALIDATORS;
  else if (hash_compare(b, H, i, 3, o)) return TMED_VB_VALIDATORS_HASH;
  if (!knows(r, TMED_VB_KNOW_NEXT_VALIDATORS)) o.skipped |= TMED_VB_KNOW_NEXT_VALIDATORS;
  else if (hash_compare(b, H, i, 4, o)) return TMED_VB_NEXT_VALIDATORS_HASH;
  if (h.height == s.initial_height && r.last_commit->n_sigs != 0) return TMED_VB_INITIAL_HAS_SIGS;
  return -1;
}

// Step 3 for a request phase B ran: cr its VerifyCommit (nullptr at the initial height), med its
// MedianTime (nullptr unless height > initial height), proposer its lookup.
inline int checks_after_commit(const tmed_block_batch &b, size_t i, const tmed_commit_result *cr,
                               const tmed_median_result *med, int32_t proposer, tmed_block_result &o) {
  const tmed_block_request &r = b.blocks[i];
  const tmed_header &h = *r.header;
  const tmed_block_state &s = *r.state;
  const Eff e = eff_state(b, i);
  if (cr) {
    o.verified = cr->verified;
    if (cr->code != TMED_COMMIT_OK) {
      o.commit = *cr;
      return TMED_VB_LAST_COMMIT;
    }
  }
  if (h.hash_lens[kHProposer] != 20) return TMED_VB_PROPOSER_SIZE;
  if (knows(r, TMED_VB_KNOW_VALIDATORS)) {  // else skipped with the hash check, whose bit says so
    o.proposer_idx = proposer;
    if (proposer < 0) return TMED_VB_PROPOSER_UNKNOWN;
  }
  const GoTime t{h.time_seconds, h.time_nanos};
  if (h.height > s.initial_height) {
    if (!time_ok(t) || !time_ok(e.last_time)) return TMED_VB_GO_PATH;
    if (!time_after(t, e.last_time)) return TMED_VB_TIME_NOT_AFTER;
    if (med->code == TMED_MEDIAN_GO_PATH) return TMED_VB_GO_PATH;
    if (t.sec != med->seconds || t.nsec != med->nanos) {
      o.median_seconds = med->seconds;
      o.median_nanos = med->nanos;
      return TMED_VB_TIME_NOT_MEDIAN;
    }
  } else if (h.height == s.initial_height) {
    if (!time_ok(t) || !time_ok(e.last_time)) return TMED_VB_GO_PATH;
    if (t.sec != e.last_time.sec || t.nsec != e.last_time.nsec) return TMED_VB_TIME_NOT_GENESIS;
  } else {
    return TMED_VB_HEIGHT_BELOW_INITIAL;
  }
  if (r.evidence_byte_size > s.evidence_max_bytes) return TMED_VB_EVIDENCE_OVERFLOW;
  return TMED_VB_OK;
}

// hashes(plan, H): fill H for the plan's requests (the ok bytes, enable, mask; optionally the proposers).
// verify(creqs, m, cres): tmed_verify_commits over m requests.
// tail(mreqs, m_of, mres, need_prop, proposer): MedianTime of the pairs mreqs (pair j is request m_of[j]'s)
//   into mres, and the proposer of every request of need_prop into proposer[i] (first index or -1).
// Each returns TMED_OK or an error.
template <class HashesFn, class TailFn, class VerifyFn>
int validate_run(const tmed_block_batch *batch, tmed_block_result *out, HashesFn &&hashes, TailFn &&tail,
                 VerifyFn &&verify) {
  int rc = check_call(batch, out);
  if (rc != TMED_OK || batch->n == 0) return rc;
  const tmed_block_batch &b = *batch;
  const size_t n = b.n;
  std::vector<int> code(n, -1);
  Plan plan{batch, {}, {}};
  for (size_t i = 0; i < n; i++) {
    memset(&out[i], 0, sizeof(out[i]));
    out[i].proposer_idx = -1;
    if (!b.blocks[i].header_basic_ok) code[i] = TMED_VB_HEADER_BASIC;
    else if (!b.blocks[i].commit_basic_ok) code[i] = TMED_VB_COMMIT_BASIC;
    else {
      plan.need.push_back(i);
      if (linked(b.blocks[i]) && (plan.need_hdr.empty() || plan.need_hdr.back() != i - 1)) plan.need_hdr.push_back(i - 1);
    }
  }
  Hashes H(n);
  if (!plan.need.empty()) {
    rc = hashes(plan, H);
    if (rc != TMED_OK) return rc;
  }
  // phase B's work: VerifyCommit against (state.ChainID, state.LastBlockID, Height - 1), MedianTime
  std::vector<size_t> live, need_prop;
  std::vector<tmed_block_id> bids(n);
  std::vector<tmed_commit_request> creqs;
  std::vector<size_t> c_at(n, (size_t)-1), m_at(n, (size_t)-1), m_of;
  for (const size_t i : plan.need) {
    code[i] = checks_before_commit(b, H, i, out[i]);
    if (code[i] >= 0) continue;
    live.push_back(i);
    const tmed_block_request &r = b.blocks[i];
    const tmed_block_state &s = *r.state;
    if (r.header->height != s.initial_height) {
      bids[i] = s.last_block_id;
      if (linked(r)) {
        bids[i].hash = &H.header[32 * (i - 1)];
        bids[i].hash_len = H.header_ok[i - 1] ? 32 : 0;
      }
      c_at[i] = creqs.size();
      creqs.push_back(tmed_commit_request{TMED_MODE_COMMIT, s.chain_id, s.chain_id_len, s.last_validators, &bids[i],
                                          (int64_t)((uint64_t)r.header->height - 1), r.last_commit, 0, 0});
    }
    if (!H.have_proposer && (H.enable[i] & kCmpLookup)) need_prop.push_back(i);
  }
  std::vector<tmed_commit_result> cres(creqs.size());
  if (!creqs.empty()) {
    rc = verify(creqs.data(), creqs.size(), cres.data());
    if (rc != TMED_OK) return rc;
  }
  // MedianTime only of the blocks whose commit verified: a failed VerifyCommit is the outcome already
  std::vector<tmed_median_request> mreqs;
  for (const size_t i : live) {
    const tmed_block_request &r = b.blocks[i];
    if (r.header->height > r.state->initial_height && cres[c_at[i]].code == TMED_COMMIT_OK) {
      m_at[i] = mreqs.size();
      mreqs.push_back(tmed_median_request{r.last_commit, r.state->last_validators});
      m_of.push_back(i);
    }
  }
  std::vector<tmed_median_result> mres(mreqs.size());
  if (!mreqs.empty() || !need_prop.empty()) {
    rc = tail(mreqs.data(), m_of, mres.data(), need_prop, H.proposer.data());
    if (rc != TMED_OK) return rc;
  }
  for (const size_t i : live)
    code[i] = checks_after_commit(b, i, c_at[i] != (size_t)-1 ? &cres[c_at[i]] : nullptr,
                                  m_at[i] != (size_t)-1 ? &mres[m_at[i]] : nullptr,
                                  (H.enable[i] & kCmpLookup) ? H.proposer[i] : -1, out[i]);
  for (size_t i = 0; i < n; i++) out[i].code = code[i];
  return TMED_OK;
}

}  // namespace tmed_validate
