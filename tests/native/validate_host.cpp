// validate_host.cpp — TEST-ONLY stand-alone host program: the replay of validateBlock
// (csrc/validate_host.h: the call check, the plan, the enable words, the host compares, the two halves of
// the replay, the link to the previous block) driven with stub hashes, stub medians and a stub commit
// verifier.  tests/test_validate_host.py builds it through tests/native/validate_host.mk with
// -fsanitize=address,undefined and runs it as a plain executable.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "validate_host.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "validate_host.cpp:%d: %s\n", __LINE__, #c);   \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

namespace V = tmed_validate;

// The stub hash of (kind, block): 32 bytes.
void stub_hash(int kind, size_t i, uint8_t out[32]) {
  for (int k = 0; k < 32; k++) out[k] = (uint8_t)(kind * 37 + i * 11 + k);
}

// A chain of n valid blocks over one set of nv validators, block i at height first + i.
struct Chain {
  size_t n, nv;
  std::vector<uint8_t> addr, pub, field;  // field: n x 6 x 32 header values
  std::vector<int64_t> pow;
  tmed_valset vs;
  std::vector<uint8_t> flags, sigs;
  std::vector<int64_t> sec;
  std::vector<int32_t> nan;
  std::vector<tmed_commit> commits;
  std::vector<tmed_header> headers;
  std::vector<tmed_block_state> states;
  std::vector<tmed_block_request> reqs;
  tmed_block_batch batch;
  uint8_t cons[32], psh[32];
  Chain(size_t n_, size_t nv_, int64_t first, bool link)
      : n(n_), nv(nv_), addr(20 * nv_), pub(32 * nv_), field(n_ * 6 * 32), pow(nv_, 10), flags(nv_, 2), sigs(64 * nv_), sec(nv_, 100),
        nan(nv_, 7), commits(n_), headers(n_), states(n_), reqs(n_) {
    for (size_t v = 0; v < nv; v++) addr[20 * v] = (uint8_t)(v + 1);
    memset(&vs, 0, sizeof(vs));
    vs.n = nv, vs.pubkeys = pub.data(), vs.powers = pow.data(), vs.addresses = addr.data(), vs.total_power = 10 * (int64_t)nv;
    stub_hash(9, 0, cons);
    stub_hash(8, 0, psh);
    for (size_t i = 0; i < n; i++) {
      tmed_commit &c = commits[i];
      memset(&c, 0, sizeof(c));
      c.height = first + (int64_t)i - 1;
      c.n_sigs = nv, c.flags = flags.data(), c.addresses = addr.data(), c.ts_seconds = sec.data(), c.ts_nanos = nan.data(), c.sigs = sigs.data();
      tmed_header &h = headers[i];
      memset(&h, 0, sizeof(h));
      h.version_block = 11, h.chain_id = "stub", h.chain_id_len = 4, h.height = first + (int64_t)i;
      h.time_seconds = 100 + (int64_t)i, h.time_nanos = 7;  // the stub median of block i
      uint8_t *f = &field[i * 6 * 32];
      stub_hash(0, i, f), stub_hash(1, i, f + 32), stub_hash(2, i, f + 64), stub_hash(3, 0, f + 96), stub_hash(3, 0, f + 128);
      if (i) stub_hash(5, i - 1, f + 160);
      const int at[5] = {V::kHLastCommit, V::kHData, V::kHEvidence, V::kHVals, V::kHNext};
      for (int s = 0; s < 5; s++) h.hashes[at[s]] = f + 32 * s, h.hash_lens[at[s]] = 32;
      h.hashes[V::kHConsensus] = cons, h.hash_lens[V::kHConsensus] = 32;
      h.hashes[V::kHProposer] = addr.data() + 20 * (i % nv), h.hash_lens[V::kHProposer] = 20;
      h.last_block_id.hash = f + 160, h.last_block_id.hash_len = i ? 32 : 0;
      h.last_block_id.psh_total = 1, h.last_block_id.psh_hash = psh, h.last_block_id.psh_hash_len = 32;
      tmed_block_state &s = states[i];
      memset(&s, 0, sizeof(s));
      s.version_block = 11, s.chain_id = "stub", s.chain_id_len = 4, s.initial_height = 1;
      s.last_block_height = link && i ? -5 : first + (int64_t)i - 1;
      s.last_block_id = h.last_block_id;
      if (link && i) s.last_block_id.hash = nullptr, s.last_block_id.hash_len = 0;
      s.last_block_time_seconds = link && i ? 0 : 50;
      s.consensus_hash = cons;
      s.validators = s.next_validators = s.last_validators = &vs;
      s.evidence_max_bytes = 1000, s.known = TMED_VB_KNOW_ALL;
      tmed_block_request &r = reqs[i];
      memset(&r, 0, sizeof(r));
      r.header = &h, r.last_commit = &c, r.state = &s, r.header_basic_ok = r.commit_basic_ok = 1, r.evidence_basic_bad = -1;
      r.flags = link && i ? TMED_VB_LINK_PREV : 0;
    }
    memset(&batch, 0, sizeof(batch));
    batch.n = n, batch.blocks = reqs.data();
  }
};

// validate_run with the stub hashes (every block's six values), the host compares, a verifier that
// accepts a commit iff its first flag is 2, the stub median (100 + i, 7) and the linear proposer scan.
int run(const Chain &c, std::vector<tmed_block_result> &out, size_t *verified = nullptr) {
  out.assign(c.n + 1, tmed_block_result());
  return V::validate_run(
      &c.batch, out.data(),
      [&](const V::Plan &p, V::Hashes &H) {
        for (const size_t i : p.need) {
          stub_hash(0, i, &H.commit[32 * i]), stub_hash(1, i, &H.data[32 * i]), stub_hash(2, i, &H.evidence[32 * i]);
          stub_hash(3, 0, &H.vals[32 * i]), stub_hash(3, 0, &H.next[32 * i]);
          H.commit_ok[i] = H.evidence_ok[i] = 1;
        }
        for (const size_t i : p.need_hdr) stub_hash(5, i, &H.header[32 * i]), H.header_ok[i] = 1;
        V::host_masks(p, H);
        return (int)TMED_OK;
      },
      [&](const tmed_median_request *, const std::vector<size_t> &m_of, tmed_median_result *mres,
          const std::vector<size_t> &need_prop, int32_t *proposer) {
        for (size_t j = 0; j < m_of.size(); j++) mres[j] = tmed_median_result{TMED_MEDIAN_OK, 100 + (int64_t)m_of[j], 7, 1, 0};
        for (const size_t i : need_prop)
          proposer[i] = V::proposer_scan(*c.reqs[i].state->validators, c.reqs[i].header->hashes[V::kHProposer]);
        return (int)TMED_OK;
      },
      [&](const tmed_commit_request *rq, size_t m, tmed_commit_result *res) {
        if (verified) *verified += m;
        for (size_t j = 0; j < m; j++) {
          memset(&res[j], 0, sizeof(res[j]));
          res[j].verified = (uint32_t)rq[j].commit->n_sigs;
          if (rq[j].commit->flags[0] != 2) res[j].code = TMED_COMMIT_WRONG_SIGNATURE;
          if (rq[j].height != rq[j].commit->height) res[j].code = TMED_COMMIT_WRONG_HEIGHT;
          if (rq[j].block_id->hash_len != rq[j].commit->block_id.hash_len) res[j].code = TMED_COMMIT_WRONG_BLOCK_ID;
        }
        return (int)TMED_OK;
      });
}

int good_chains() {
  for (const bool link : {false, true})
    for (const size_t n : {(size_t)1, (size_t)3, (size_t)65}) {
      Chain c(n, 5, 2, link);
      for (size_t i = 0; i < n; i++) {  // the commits name the block before theirs
        c.commits[i].block_id = c.headers[i].last_block_id;
      }
      std::vector<tmed_block_result> out;
      size_t verified = 0;
      CHECK(run(c, out, &verified) == TMED_OK);
      CHECK(verified == n);
      for (size_t i = 0; i < n; i++) {
        CHECK(out[i].code == TMED_VB_OK);
        CHECK(out[i].proposer_idx == (int32_t)(i % 5) && out[i].verified == 5 && out[i].skipped == 0);
      }
    }
  return 0;
}

int failures() {
  Chain c(8, 3, 2, true);
  for (size_t i = 0; i < c.n; i++) c.commits[i].block_id = c.headers[i].last_block_id;
  c.reqs[1].header_basic_ok = 0;                                   // HEADER_BASIC, sends nothing
  c.field[2 * 192 + 32] ^= 1;                                      // block 2: DataHash
  c.field[3 * 192 + 160 + 31] ^= 0x80;                             // block 3: the link's hash
  c.headers[4].hash_lens[V::kHVals] = 20;                          // block 4: ValidatorsHash of another length
  uint8_t stranger[20] = {0xee};
  c.headers[5].hashes[V::kHProposer] = stranger;                   // block 5: an unknown proposer
  c.headers[6].time_nanos = 8;                                     // block 6: not the median
  c.reqs[7].evidence_byte_size = 1001;                             // block 7: overflow
  std::vector<tmed_block_result> out;
  size_t verified = 0;
  CHECK(run(c, out, &verified) == TMED_OK);
  const int want[8] = {TMED_VB_OK, TMED_VB_HEADER_BASIC, TMED_VB_DATA_HASH, TMED_VB_LAST_BLOCK_ID, TMED_VB_VALIDATORS_HASH,
                       TMED_VB_PROPOSER_UNKNOWN, TMED_VB_TIME_NOT_MEDIAN, TMED_VB_EVIDENCE_OVERFLOW};
  for (size_t i = 0; i < 8; i++) CHECK(out[i].code == want[i]);
  CHECK(verified == 4);  // blocks 0, 5, 6, 7
  uint8_t h[32];
  stub_hash(1, 2, h);
  CHECK(out[2].hash_len == 32 && memcmp(out[2].hash, h, 32) == 0);
  stub_hash(5, 2, h);
  CHECK(out[3].hash_len == 32 && memcmp(out[3].hash, h, 32) == 0);
  CHECK(out[6].median_seconds == 106 && out[6].median_nanos == 7);
  CHECK(out[8].code == 0);  // nothing written past the call's results
  // unknown fields: skipped and reported; NULL sets allowed
  Chain d(2, 3, 2, false);
  for (size_t i = 0; i < d.n; i++) d.commits[i].block_id = d.headers[i].last_block_id;
  d.states[1].known = 0;
  d.states[1].validators = d.states[1].next_validators = nullptr;
  d.field[192 + 96] ^= 1;
  CHECK(run(d, out) == TMED_OK);
  CHECK(out[0].code == TMED_VB_OK && out[1].code == TMED_VB_OK && out[1].skipped == TMED_VB_KNOW_ALL && out[1].proposer_idx == -1);
  // malformed calls
  Chain e(2, 3, 2, false);
  e.reqs[0].flags = TMED_VB_LINK_PREV;
  CHECK(run(e, out) == TMED_EINVAL);
  e.reqs[0].flags = 0;
  e.states[1].known = 32;
  CHECK(run(e, out) == TMED_EINVAL);
  e.states[1].known = TMED_VB_KNOW_ALL;
  e.reqs[1].last_commit = nullptr;
  CHECK(run(e, out) == TMED_EINVAL);
  e.reqs[1].commit_basic_ok = 0;  // a nil LastCommit is an outcome
  CHECK(run(e, out) == TMED_OK && out[1].code == TMED_VB_COMMIT_BASIC);
  return 0;
}

}  // namespace

int main() {
  if (good_chains() || failures()) return 1;
  printf("validate-ok\n");
  return 0;
}
