// light_host.h — light.Verify (light/verifier.go:135-151) replayed on the host over hashes and commit
// outcomes computed elsewhere: the host half of tmed_light_verify / tmed_light_verify_with
// (include/tmed25519.h has the outcome codes and cites each check's lines).  Host C++ only (no HIP):
// seam_host.h includes it, and tests/native/light_host.cpp compiles the same code with a stub commit
// verifier under AddressSanitizer and UndefinedBehaviorSanitizer.
//
// light_run does, in the reference's order:
//   1. per request, the checks the host decides alone: the trusted header's expiry (:46/:105), then
//      SignedHeader.ValidateBasic's (types/light.go:137-151) basic_ok, chain ID and commit height;
//   2. `hashes`: Header.Hash of the requests still undecided, ValidatorSet.Hash of those that also
//      pass the height and time checks (:164-181), which come after the header-hash compare;
//   3. the hash compares (light.go:152-154, verifier.go:183-189, :117-123);
//   4. `commits`: VerifyCommitLightTrusting (non-adjacent, :58) and VerifyCommitLight (:73/:126) of
//      the requests that passed everything before, as one batch of tmed_commit_requests, or two with
//      TMED_LIGHT_ORDERED;
//   5. the outcome: the Trusting failure before the Light failure.
#pragma once

#include <string.h>

#include <vector>

#include "../../include/tmed25519.h"
#include "vote_wire.h"

namespace tmed_light {

// gogoproto StdTime's range (vote_wire.h timestamp_encodable): the range in which Time.Add of an
// int64-nanosecond duration cannot overflow and outside which the reference's own marshalling fails.
using tmed::kMaxSeconds;
using tmed::kMinSeconds;
constexpr int64_t kNanos = 1000000000ll;

// Go's time.Time as (Unix seconds, nanoseconds in [0, 1e9)): wall-clock comparisons only.
struct GoTime {
  int64_t sec;
  int32_t nsec;
};
inline bool time_ok(GoTime t) { return tmed::timestamp_encodable(t.sec, t.nsec); }
// Time.Add (time/time.go): d / 1e9 and d % 1e9 truncate toward zero in Go as in C++.
inline GoTime time_add(GoTime t, int64_t d) {
  int64_t sec = t.sec + d / kNanos;
  int64_t ns = (int64_t)t.nsec + d % kNanos;
  if (ns >= kNanos) {
    sec++;
    ns -= kNanos;
  } else if (ns < 0) {
    sec--;
    ns += kNanos;
  }
  return GoTime{sec, (int32_t)ns};
}
inline bool time_after(GoTime a, GoTime b) { return a.sec > b.sec || (a.sec == b.sec && a.nsec > b.nsec); }
inline bool time_before(GoTime a, GoTime b) { return time_after(b, a); }

inline bool bytes_equal(const uint8_t *a, size_t na, const uint8_t *b, size_t nb) {  // bytes.Equal
  return na == nb && (na == 0 || memcmp(a, b, na) == 0);
}

inline int check_light_request(const tmed_light_request &r) {
  if (!r.header || !r.commit || !r.vals) return TMED_EINVAL;
  if ((r.chain_id_len && !r.chain_id) || (r.header->chain_id_len && !r.header->chain_id)) return TMED_EINVAL;
  if (r.header->hash_lens[2] && !r.header->hashes[2]) return TMED_EINVAL;
  if (r.commit->block_id.hash_len && !r.commit->block_id.hash) return TMED_EINVAL;
  if (r.trusted_next_vals_hash_len && !r.trusted_next_vals_hash) return TMED_EINVAL;
  return TMED_OK;
}

// Untrusted height == trusted height + 1 (Go's int64 addition wraps).
inline bool light_adjacent(const tmed_light_request &r) {
  return r.header->height == (int64_t)((uint64_t)r.trusted_height + 1);
}

// Step 1.  Returns the request's outcome, or -1: undecided, its header hash is needed.  *later: the
// first failing check among HEIGHT_NOT_GREATER, TIME_NOT_AFTER, TIME_FROM_FUTURE (0: none), which
// wins only if the header-hash compare passes.
inline int light_host_checks(const tmed_light_request &r, tmed_light_result &o, int *later) {
  const tmed_header &h = *r.header;
  const GoTime trusted{r.trusted_time_seconds, r.trusted_time_nanos}, now{r.now_seconds, r.now_nanos};
  const GoTime untrusted{h.time_seconds, h.time_nanos};
  *later = 0;
  if (!time_ok(trusted) || !time_ok(now) || !time_ok(untrusted)) return TMED_LIGHT_GO_PATH;
  const GoTime expires = time_add(trusted, r.trusting_period_ns);  // HeaderExpired, :207-210
  if (!time_after(expires, now)) {
    o.expired_seconds = expires.sec;
    o.expired_nanos = expires.nsec;
    return TMED_LIGHT_OLD_HEADER_EXPIRED;
  }
  if (!r.basic_ok) return TMED_LIGHT_HEADER_BASIC;
  if (!bytes_equal((const uint8_t *)h.chain_id, h.chain_id_len, (const uint8_t *)r.chain_id, r.chain_id_len))
    return TMED_LIGHT_WRONG_CHAIN;
  if (r.commit->height != h.height) return TMED_LIGHT_COMMIT_HEIGHT;
  if (h.height <= r.trusted_height) *later = TMED_LIGHT_HEIGHT_NOT_GREATER;
  else if (!time_after(untrusted, trusted)) *later = TMED_LIGHT_TIME_NOT_AFTER;
  else if (!time_before(untrusted, time_add(now, r.max_clock_drift_ns))) *later = TMED_LIGHT_TIME_FROM_FUTURE;
  return -1;
}

// Step 3 for a request step 1 left undecided.  hash / ok: its Header.Hash (ok = 0: nil); vals_hash:
// its untrusted set's hash (read only when later == 0).  Returns the outcome, or -1: the commit
// checks decide.
inline int light_hash_checks(const tmed_light_request &r, tmed_light_result &o, int later, const uint8_t *hash,
                             uint8_t ok, const uint8_t *vals_hash) {
  const tmed_header &h = *r.header;
  if (!bytes_equal(hash, ok ? 32 : 0, r.commit->block_id.hash, r.commit->block_id.hash_len)) {
    o.hash_len = ok ? 32 : 0;
    if (ok) memcpy(o.hash, hash, 32);
    return TMED_LIGHT_COMMIT_HEADER_HASH;
  }
  if (later) return later;
  if (!bytes_equal(h.hashes[2], h.hash_lens[2], vals_hash, 32)) {
    o.hash_len = 32;
    memcpy(o.hash, vals_hash, 32);
    return TMED_LIGHT_VALS_HASH;
  }
  if (o.adjacent &&
      !bytes_equal(h.hashes[2], h.hash_lens[2], r.trusted_next_vals_hash, r.trusted_next_vals_hash_len))
    return TMED_LIGHT_NEXT_VALS_HASH;
  return -1;
}

// hashes(need_hdr, need_vals, hdr_hash, hdr_ok, vals_hash): fill hdr_hash[32 i ..) / hdr_ok[i] for
// every request i of need_hdr and vals_hash[32 i ..) for every i of need_vals (arrays of n entries).
// commits(creqs, m, cres): tmed_verify_commits over m requests.  Both return TMED_OK or an error.
template <class Hashes, class Commits>
int light_run(const tmed_light_request *reqs, size_t n, uint32_t flags, tmed_light_result *out, Hashes &&hashes,
              Commits &&commits) {
  if ((flags & ~TMED_LIGHT_ORDERED) || (n && (!reqs || !out))) return TMED_EINVAL;
  for (size_t i = 0; i < n; i++) {
    const int rc = check_light_request(reqs[i]);
    if (rc != TMED_OK) return rc;
    if (!light_adjacent(reqs[i]) && !reqs[i].trusted_vals) return TMED_EINVAL;
  }
  std::vector<int> code(n), later(n, 0);
  std::vector<size_t> need_hdr, need_vals;
  for (size_t i = 0; i < n; i++) {
    memset(&out[i], 0, sizeof(out[i]));
    out[i].adjacent = light_adjacent(reqs[i]) ? 1 : 0;
    code[i] = light_host_checks(reqs[i], out[i], &later[i]);
    if (code[i] < 0) {
      need_hdr.push_back(i);
      if (!later[i]) need_vals.push_back(i);
    }
  }
  std::vector<uint8_t> hdr_hash(32 * n), hdr_ok(n), vals_hash(32 * n);
  if (!need_hdr.empty()) {
    const int rc = hashes(need_hdr, need_vals, hdr_hash.data(), hdr_ok.data(), vals_hash.data());
    if (rc != TMED_OK) return rc;
  }
  // the commit requests of the pairs every earlier check passed: Trusting then Light, side by side
  // (the seam then sends a signature both loops reach once: seam_host.h pair_request)
  std::vector<size_t> live;
  for (const size_t i : need_hdr) {
    code[i] = light_hash_checks(reqs[i], out[i], later[i], hdr_hash.data() + 32 * i, hdr_ok[i], vals_hash.data() + 32 * i);
    if (code[i] < 0) live.push_back(i);
  }
  const bool ordered = (flags & TMED_LIGHT_ORDERED) != 0;
  std::vector<tmed_commit_request> creqs;
  std::vector<size_t> t_at(n, (size_t)-1), l_at(n, (size_t)-1);
  auto trusting = [&](size_t i) {
    const tmed_light_request &r = reqs[i];
    t_at[i] = creqs.size();
    creqs.push_back(tmed_commit_request{TMED_MODE_LIGHT_TRUSTING, r.chain_id, r.chain_id_len, r.trusted_vals, nullptr, 0,
                                        r.commit, r.trust_num, r.trust_den});
  };
  auto light = [&](size_t i) {
    const tmed_light_request &r = reqs[i];
    l_at[i] = creqs.size();
    creqs.push_back(tmed_commit_request{TMED_MODE_LIGHT, r.chain_id, r.chain_id_len, r.vals, &r.commit->block_id,
                                        r.header->height, r.commit, 0, 0});
  };
  for (const size_t i : live) {
    if (!out[i].adjacent) trusting(i);
    if (out[i].adjacent || !ordered) light(i);
  }
  std::vector<tmed_commit_result> cres(creqs.size());
  if (!creqs.empty()) {
    const int rc = commits(creqs.data(), creqs.size(), cres.data());
    if (rc != TMED_OK) return rc;
  }
  if (ordered) {  // the Light requests of the pairs whose Trusting check passed, as a second batch
    const size_t first = creqs.size();
    for (const size_t i : live)
      if (!out[i].adjacent && cres[t_at[i]].code == TMED_COMMIT_OK) light(i);
    cres.resize(creqs.size());
    if (creqs.size() > first) {
      const int rc = commits(creqs.data() + first, creqs.size() - first, cres.data() + first);
      if (rc != TMED_OK) return rc;
    }
  }
  for (const size_t i : live) {
    tmed_light_result &o = out[i];
    const tmed_commit_result *t = t_at[i] != (size_t)-1 ? &cres[t_at[i]] : nullptr;
    const tmed_commit_result *l = l_at[i] != (size_t)-1 ? &cres[l_at[i]] : nullptr;
    o.verified_trusting = t ? t->verified : 0;
    o.verified_light = l ? l->verified : 0;
    if (t && t->code != TMED_COMMIT_OK) {
      code[i] = TMED_LIGHT_TRUSTING;
      o.commit = *t;
    } else if (l->code != TMED_COMMIT_OK) {
      code[i] = TMED_LIGHT_COMMIT;
      o.commit = *l;
    } else {
      code[i] = TMED_LIGHT_OK;
    }
  }
  for (size_t i = 0; i < n; i++) out[i].code = code[i];
  return TMED_OK;
}

}  // namespace tmed_light
