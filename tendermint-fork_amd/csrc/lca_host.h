// lca_host.h — LightClientAttackEvidence on the host: VerifyLightClientAttack (evidence/verify.go:
// 113-154) and validateABCIEvidence (:226-271) replayed over hashes, commit outcomes and byzantine
// lists computed elsewhere, and GetByzantineValidators lane by lane with no device (lca_free.h is the
// rule).  Host C++ only (no HIP): commit.hip and lca.hip include it for the device entries,
// lca_host.cpp for tmed_byzantine_validators_host and tmed_verify_light_client_attacks_with, and
// tests/native/lca_host.cpp compiles the same code with a stub commit verifier under AddressSanitizer
// and UndefinedBehaviorSanitizer.
//
// lca_run does, in the reference's order:
//   1. per request, what the host decides alone: GO_PATH (a header time outside the Timestamp range),
//      the attack kind, and NOT_DERIVED (:124-127: the same heights and an invalid conflicting header);
//   2. `hashes`: Header.Hash of both headers of the requests still undecided;
//   3. `commits`: VerifyCommitLightTrusting (heights differ, :117-121) and VerifyCommitLight (:130-133)
//      on the one conflicting commit, side by side in one batch of tmed_commit_requests;
//   4. TRUSTING, COMMIT, TOTAL_POWER (:136-139), TIME_NOT_VIOLATED (:142-145), SAME_HASH (:148-151);
//   5. `tail`: the byzantine lists of the requests that passed all of that, and Hash() of every request
//      of step 2;
//   6. validateABCIEvidence's compare of the computed list with the claimed one.
#pragma once

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/tmed25519.h"
#include "lca_free.h"
#include "light_host.h"

namespace tmed_lca {

using tmed_light::GoTime;

inline bool valset_lookup_ok(const tmed_valset *vs) { return vs && vs->n <= 0x7fffffffu && (!vs->n || (vs->addresses && vs->powers)); }

// What every entry reads of a request: TMED_EINVAL for a NULL struct or array.
inline int check_lca_request(const tmed_lca_request &r) {
  if (!r.conflicting_header || !r.conflicting_commit || !r.trusted_header || !r.trusted_commit) return TMED_EINVAL;
  if (!valset_lookup_ok(r.conflicting_vals) || !valset_lookup_ok(r.common_vals)) return TMED_EINVAL;
  const tmed_commit &c = *r.conflicting_commit, &t = *r.trusted_commit;
  if (c.n_sigs > 0x7fffffffu || (c.n_sigs && (!c.flags || !c.addresses)) || (t.n_sigs && !t.flags)) return TMED_EINVAL;
  for (const tmed_header *h : {r.conflicting_header, r.trusted_header})
    for (int k = 2; k <= 6; k++)
      if (h->hash_lens[k] && !h->hashes[k]) return TMED_EINVAL;
  if (r.n_byz > 0x7fffffffu || (r.n_byz && (r.byz_is_nil || !r.byz_addresses || !r.byz_powers))) return TMED_EINVAL;
  return TMED_OK;
}

// The call's requests and its output ranges.
inline int check_lca_call(const tmed_lca_request *reqs, size_t n, const int32_t *byz, const uint64_t *byz_off,
                          const void *out) {
  if (n == 0) return TMED_OK;
  if (!reqs || !byz_off || !out || n > 0x7fffffffu) return TMED_EINVAL;
  for (size_t i = 0; i < n; i++) {
    if (check_lca_request(reqs[i]) != TMED_OK) return TMED_EINVAL;
    if (byz_off[i + 1] < byz_off[i] || byz_off[i + 1] - byz_off[i] < reqs[i].conflicting_commit->n_sigs) return TMED_EINVAL;
  }
  if (byz_off[n] > byz_off[0] && !byz) return TMED_EINVAL;
  return TMED_OK;
}

// The candidates of one request (lca_free.h): their commit positions into pos, the set they are looked
// up in; false where the reference panics on an index out of range.
inline const tmed_valset *lookup_set(const tmed_lca_request &r, int kind) {
  return kind == TMED_LCA_LUNATIC ? r.common_vals : r.conflicting_vals;
}
inline bool plan_candidates(const tmed_lca_request &r, int kind, std::vector<uint32_t> &pos) {
  pos.clear();
  const tmed_commit &c = *r.conflicting_commit, &t = *r.trusted_commit;
  if (kind == TMED_LCA_LUNATIC) {
    for (size_t i = 0; i < c.n_sigs; i++)
      if (c.flags[i] == tmed::kFlagCommit) pos.push_back((uint32_t)i);
  } else if (kind == TMED_LCA_EQUIVOCATION) {
    for (size_t i = 0; i < c.n_sigs; i++) {
      if (c.flags[i] == tmed::kFlagAbsent) continue;
      if (i >= t.n_sigs) return false;  // trusted.Commit.Signatures[i]: index out of range
      if (t.flags[i] != tmed::kFlagAbsent) pos.push_back((uint32_t)i);
    }
  }
  return true;
}
inline bool cand_len_ok(const tmed_commit &c, uint32_t i) { return !c.address_lens || c.address_lens[i] == 20; }

// A request's result from its candidates' lookups in ranked order (the found ones first, -1 behind
// them): the entries into list, kind and count into o.
inline void finish_list(int kind, const int32_t *ranked, size_t n_cand, int32_t *list, tmed_byz_result &o) {
  size_t found = 0;
  while (found < n_cand && ranked[found] >= 0) found++;
  o.kind = kind;
  o.state = TMED_BYZ_OK;
  o.count = 0;
  if (kind == TMED_LCA_EQUIVOCATION && found < n_cand) {  // a nil *Validator in the list
    if (n_cand >= 2) {
      o.state = TMED_BYZ_PANIC;  // Less dereferences it
    } else {
      list[0] = -1;
      o.count = 1;
    }
    return;
  }
  for (size_t k = 0; k < found; k++) list[k] = ranked[k];
  o.count = (uint32_t)found;
}

// GetByzantineValidators of one request on one thread: the linear GetByAddress per candidate and a
// sort by lca_before.
inline void byzantine_validators_one(const tmed_lca_request &r, int kind, int32_t *list, tmed_byz_result &o) {
  std::vector<uint32_t> pos;
  if (!plan_candidates(r, kind, pos)) {
    o.kind = kind;
    o.state = TMED_BYZ_PANIC;
    o.count = 0;
    return;
  }
  const tmed_valset &vs = *lookup_set(r, kind);
  const tmed_commit &c = *r.conflicting_commit;
  struct Cand {
    uint32_t key[tmed::kLcaKeyDw], pos;
    int32_t found;
  };
  std::vector<Cand> cs(pos.size());
  for (size_t k = 0; k < pos.size(); k++) {
    Cand &cd = cs[k];
    cd.pos = pos[k];
    cd.found = -1;
    if (cand_len_ok(c, pos[k]))
      for (size_t v = 0; v < vs.n; v++)
        if (memcmp(vs.addresses + 20 * v, c.addresses + 20 * (size_t)pos[k], 20) == 0) {
          cd.found = (int32_t)v;
          break;
        }
    uint32_t addr[5] = {0, 0, 0, 0, 0};
    if (cd.found >= 0) memcpy(addr, vs.addresses + 20 * (size_t)cd.found, 20);
    tmed::lca_key(cd.found >= 0, cd.found >= 0 ? vs.powers[cd.found] : 0, addr, cd.key);
  }
  std::sort(cs.begin(), cs.end(), [](const Cand &a, const Cand &b) { return tmed::lca_before(a.key, a.pos, b.key, b.pos); });
  std::vector<int32_t> ranked(cs.size());
  for (size_t k = 0; k < cs.size(); k++) ranked[k] = cs[k].found;
  finish_list(kind, ranked.data(), ranked.size(), list, o);
}

inline int byzantine_validators_host(const tmed_lca_request *reqs, size_t n, int32_t *byz, const uint64_t *byz_off,
                                     tmed_byz_result *out) {
  const int rc = check_lca_call(reqs, n, byz, byz_off, out);
  if (rc != TMED_OK) return rc;
  for (size_t i = 0; i < n; i++) byzantine_validators_one(reqs[i], tmed::lca_kind(reqs[i]), byz + byz_off[i], out[i]);
  return TMED_OK;
}

// Step 6 for a request whose list (b, list) is computed.
inline int validate_abci(const tmed_lca_request &r, const tmed_byz_result &b, const int32_t *list, tmed_lca_result &o) {
  if (b.state == TMED_BYZ_PANIC) return TMED_LCA_PANIC;
  o.n_byz_expected = b.count;
  if (b.count == 0 && !r.byz_is_nil) {  // validators == nil && ev.ByzantineValidators != nil
    o.actual = (int64_t)r.n_byz;
    return TMED_LCA_AMNESIA_HAS_VALIDATORS;
  }
  if (b.count != r.n_byz) {
    o.expected = b.count;
    o.actual = (int64_t)r.n_byz;
    return TMED_LCA_BYZ_COUNT;
  }
  const tmed_valset &vs = *lookup_set(r, b.kind);
  for (uint32_t idx = 0; idx < b.count; idx++) {
    const int32_t v = list[idx];
    if (v < 0) return TMED_LCA_PANIC;  // val.Address of a nil *Validator
    o.idx = (int32_t)idx;
    o.val_idx = v;
    const uint32_t alen = r.byz_address_lens ? r.byz_address_lens[idx] : 20;
    if (alen != 20 || memcmp(r.byz_addresses + 20 * (size_t)idx, vs.addresses + 20 * (size_t)v, 20) != 0)
      return TMED_LCA_BYZ_ADDRESS;
    if (r.byz_powers[idx] != vs.powers[v]) {
      o.expected = vs.powers[v];
      o.actual = r.byz_powers[idx];
      return TMED_LCA_BYZ_POWER;
    }
  }
  o.idx = o.val_idx = 0;
  return TMED_LCA_OK;
}

// hashes(live, ch, cok, th, tok): Header.Hash of the conflicting (ch / cok) and the trusted (th / tok)
//   header of every request of live, into arrays of n entries indexed by request (ok = 0: nil).
// commits(creqs, m, cres): tmed_verify_commits over m requests.
// tail(live, ch, cok, need, kinds, bres, ev_hash): the list of every request of need into its byz range
//   with bres[i] (kinds[i]: its attack kind), and Hash() of every request of live into ev_hash[32 i ..).
// Each returns TMED_OK or an error.
template <class Hashes, class Commits, class Tail>
int lca_run(const tmed_lca_request *reqs, size_t n, uint32_t flags, int32_t *byz, const uint64_t *byz_off,
            tmed_lca_result *out, Hashes &&hashes, Commits &&commits, Tail &&tail) {
  if (flags) return TMED_EINVAL;
  int rc = check_lca_call(reqs, n, byz, byz_off, out);
  if (rc != TMED_OK) return rc;
  for (size_t i = 0; i < n; i++)
    for (const tmed_header *h : {reqs[i].conflicting_header, reqs[i].trusted_header})
      if (h->chain_id_len && !h->chain_id) return TMED_EINVAL;
  std::vector<int> code(n, -1), kinds(n);
  std::vector<size_t> live;
  for (size_t i = 0; i < n; i++) {
    const tmed_lca_request &r = reqs[i];
    memset(&out[i], 0, sizeof(out[i]));
    out[i].kind = kinds[i] = tmed::lca_kind(r);
    const GoTime ct{r.conflicting_header->time_seconds, r.conflicting_header->time_nanos};
    const GoTime tt{r.trusted_header->time_seconds, r.trusted_header->time_nanos};
    if (!tmed_light::time_ok(ct) || !tmed_light::time_ok(tt)) code[i] = TMED_LCA_GO_PATH;
    else if (r.common_header_height == r.conflicting_header->height && kinds[i] == TMED_LCA_LUNATIC)
      code[i] = TMED_LCA_NOT_DERIVED;
    else live.push_back(i);
  }
  std::vector<uint8_t> ch(32 * n), cok(n), th(32 * n), tok(n), ev_hash(32 * n);
  if (!live.empty()) {
    rc = hashes(live, ch.data(), cok.data(), th.data(), tok.data());
    if (rc != TMED_OK) return rc;
  }
  // Trusting then Light on the one Commit, side by side (seam_host.h pair_request sends a signature
  // both loops reach once)
  std::vector<tmed_commit_request> creqs;
  std::vector<size_t> t_at(n, (size_t)-1), l_at(n, (size_t)-1);
  for (const size_t i : live) {
    const tmed_lca_request &r = reqs[i];
    const tmed_header &t = *r.trusted_header;
    if (r.common_header_height != r.conflicting_header->height) {
      t_at[i] = creqs.size();
      creqs.push_back(tmed_commit_request{TMED_MODE_LIGHT_TRUSTING, t.chain_id, t.chain_id_len, r.common_vals, nullptr, 0,
                                          r.conflicting_commit, 1, 3});  // light.DefaultTrustLevel
    }
    l_at[i] = creqs.size();
    creqs.push_back(tmed_commit_request{TMED_MODE_LIGHT, t.chain_id, t.chain_id_len, r.conflicting_vals,
                                        &r.conflicting_commit->block_id, r.conflicting_header->height, r.conflicting_commit,
                                        0, 0});
  }
  std::vector<tmed_commit_result> cres(creqs.size());
  if (!creqs.empty()) {
    rc = commits(creqs.data(), creqs.size(), cres.data());
    if (rc != TMED_OK) return rc;
  }
  std::vector<size_t> need;
  for (const size_t i : live) {
    const tmed_lca_request &r = reqs[i];
    tmed_lca_result &o = out[i];
    const tmed_commit_result *t = t_at[i] != (size_t)-1 ? &cres[t_at[i]] : nullptr, *l = &cres[l_at[i]];
    o.verified_trusting = t ? t->verified : 0;
    o.verified_light = l->verified;
    const GoTime ct{r.conflicting_header->time_seconds, r.conflicting_header->time_nanos};
    const GoTime tt{r.trusted_header->time_seconds, r.trusted_header->time_nanos};
    if (t && t->code != TMED_COMMIT_OK) {
      code[i] = t->code == TMED_COMMIT_PANIC ? TMED_LCA_PANIC : TMED_LCA_TRUSTING;
      o.commit = *t;
    } else if (l->code != TMED_COMMIT_OK) {
      code[i] = l->code == TMED_COMMIT_PANIC ? TMED_LCA_PANIC : TMED_LCA_COMMIT;
      o.commit = *l;
    } else if (r.total_voting_power != r.common_vals->total_power) {
      code[i] = TMED_LCA_TOTAL_POWER;
      o.expected = r.total_voting_power;
      o.actual = r.common_vals->total_power;
    } else if (r.conflicting_header->height > r.trusted_header->height && tmed_light::time_after(ct, tt)) {
      code[i] = TMED_LCA_TIME_NOT_VIOLATED;
    } else if (tmed_light::bytes_equal(th.data() + 32 * i, tok[i] ? 32 : 0, ch.data() + 32 * i, cok[i] ? 32 : 0)) {
      code[i] = TMED_LCA_SAME_HASH;
    } else {
      need.push_back(i);
    }
  }
  std::vector<tmed_byz_result> bres(n);
  if (!live.empty()) {
    rc = tail(live, ch.data(), cok.data(), need, kinds.data(), bres.data(), ev_hash.data());
    if (rc != TMED_OK) return rc;
  }
  for (const size_t i : live) memcpy(out[i].hash, ev_hash.data() + 32 * i, 32);
  for (const size_t i : need) code[i] = validate_abci(reqs[i], bres[i], byz + byz_off[i], out[i]);
  for (size_t i = 0; i < n; i++) out[i].code = code[i];
  return TMED_OK;
}

// Everything below runs SHA-256 on the host, so it is compiled as plain C++ only (lca_host.cpp,
// tests/native/lca_host.cpp), as the second half of evidence_host.h is.
#if !defined(__HIPCC__)
inline void evidence_hash_host(const uint8_t *hdr_hash, bool ok, int64_t common_height, uint8_t out[32]) {
  uint32_t hdr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st[8];
  if (ok) memcpy(hdr, hdr_hash, 32);
  tmed::lca_evidence_hash(hdr, ok, common_height, st);
  for (int k = 0; k < 8; k++) {
    const uint32_t be = tmed::lca_bswap(st[k]);
    memcpy(out + 4 * k, &be, 4);
  }
}

// The tail of lca_run with no device.
inline int tail_host(const tmed_lca_request *reqs, const std::vector<size_t> &live, const uint8_t *ch, const uint8_t *cok,
                     const std::vector<size_t> &need, const int *kinds, int32_t *byz, const uint64_t *byz_off,
                     tmed_byz_result *bres, uint8_t *ev_hash) {
  for (const size_t i : live) evidence_hash_host(ch + 32 * i, cok[i] != 0, reqs[i].common_height, ev_hash + 32 * i);
  for (const size_t i : need) byzantine_validators_one(reqs[i], kinds[i], byz + byz_off[i], bres[i]);
  return TMED_OK;
}
#endif  // !__HIPCC__

}  // namespace tmed_lca
