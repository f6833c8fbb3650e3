// seam_race.cpp — TEST-ONLY: the commit seam's host half (csrc/seam_host.h, the code commit.hip
// runs) on a light-client-shaped batch, driven as the pipelined seam drives it (bs_pump / bs_finish:
// seam_plan with a staging group and template rows, the staged bits produced in staging order by a
// stand-in verifier, then finish_batch) or, with KEYSETS > 1, as one seam call on sets of several
// key sets (run_seam / ctx_verify: seam_plan, group_by_keyset, per group the bits and scatter_bits,
// then copy_aliases and seam_replay once); everything but the stand-in verifier is a call into
// seam_host.h.  Built with ThreadSanitizer by
// tests/test_native_sanitizers.py and run with the pool jitter on.  A part of a parallel region that
// reads what another part of the same region writes (round 5's Group::add_run read off[r + 1] of the
// next part) is a data race TSan reports on the first run, whatever the timing.
//
// Prints a digest of every request's outcome; the test compares it with a run on one host thread
// (TMED_HOST_THREADS=1: every region serial), so the parallel merge, aliasing and finish must also
// give exactly the serial plan's results — and, as outcomes depend only on fake_bit(key, signature),
// the same digest whatever KEYSETS is.
//
//
// Also prints `plan`, a digest of everything seam_plan itself hands on, per iteration: its return code,
// every Plan (the vof of an undecided Trusting request by content), the results of the requests it
// decided, Cands, and for a pipelined batch the staging group and the template rows it built.  It reads
// only ps.v, the candidates, the group and the templates, never the planner's per-worker state, so the
// same source measures any planner that keeps those outputs (tests/test_seam_plan_parts.py holds the
// values of the planner before its per-worker state became one record).
//
// usage: seam_race HEADERS VALIDATORS ITERATIONS JITTER_US SEED [KEYSETS [SHAPES]]
// SHAPES: KIND:HEADERS:VALIDATORS[,...] (default pairs:HEADERS:VALIDATORS), planned one after another
// in every iteration on the same Plans / Cands / Group / Templates.  KIND is
//   pairs     per header a Trusting request, then the Light request on the same commit
//   light     per header the Light request alone (no pairing)
//   decided   pairs, the first 160 requests decided before any candidate (Trusting: a zero trust
//             denominator; Light: the wrong height)
// One line of counts per shape (of the last iteration), the two digests at the end of the last.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "seam_host.h"

// no key-set cache in this harness: planning builds its own address indexes
struct KcCall {};
static const AddrIndex *kc_addr_index(const KcCall *, const tmed_valset &) { return nullptr; }

namespace {

// The stand-in verifier: a pseudo-random bit of (key, signature) — the same tuple always gets the
// same bit, so an alias (one verification serving two requests) reads exactly what its own
// verification would have said.
uint8_t fake_bit(const uint8_t *key, const uint8_t *sig) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < 32; i++) h = (h ^ key[i]) * 1099511628211ull;
  for (int i = 0; i < 64; i++) h = (h ^ sig[i]) * 1099511628211ull;
  return (h >> 7) % 53 != 0;  // ~2 % invalid
}

struct SetData {
  std::vector<uint8_t> pubs, addrs;
  std::vector<int64_t> powers;
  std::vector<uint32_t> kix;  // the keys' pool indexes (KEYSETS > 1): one index per distinct key
  tmed_valset vs{};
  // handle: the set's key-set handle (0: generic); next_index: the pool's next free index
  void make(size_t n, std::mt19937_64 &rng, const SetData *from, size_t change, uint64_t handle, uint32_t *next_index) {
    pubs.resize(32 * n);
    addrs.resize(20 * n);
    powers.resize(n);
    if (next_index) {
      kix.resize(n);
      for (size_t v = 0; v < n; v++) kix[v] = !from || v == change ? (*next_index)++ : from->kix[v];
      vs.keyset_index = kix.data();
    }
    vs.keyset = handle;
    for (size_t v = 0; v < n; v++) {
      const bool fresh = !from || v == change;
      for (int b = 0; b < 32; b++) pubs[32 * v + b] = fresh ? (uint8_t)rng() : from->pubs[32 * v + b];
      for (int b = 0; b < 20; b++) addrs[20 * v + b] = fresh ? (uint8_t)rng() : from->addrs[20 * v + b];
      powers[v] = fresh ? 1 + (int64_t)(rng() % 100) : from->powers[v];
    }
    int64_t total = 0;
    for (int64_t p : powers) total += p;
    vs.n = n;
    vs.pubkeys = pubs.data();
    vs.powers = powers.data();
    vs.addresses = addrs.data();
    vs.total_power = total;
  }
};

struct CommitData {
  std::vector<uint8_t> flags, addrs, sigs, hash, psh;
  std::vector<int64_t> sec;
  std::vector<int32_t> nan;
  std::vector<uint32_t> slen;
  tmed_commit c{};
  void make(const SetData &signers, int64_t height, std::mt19937_64 &rng) {
    const size_t n = signers.vs.n;
    flags.resize(n);
    addrs = signers.addrs;
    sigs.resize(64 * n);
    sec.resize(n);
    nan.resize(n);
    slen.resize(n);
    hash.resize(32);
    psh.resize(32);
    for (auto &b : hash) b = (uint8_t)rng();
    for (auto &b : psh) b = (uint8_t)rng();
    for (size_t i = 0; i < n; i++) {
      const unsigned r = rng() % 100;
      flags[i] = r < 80 ? 2 : (r < 95 ? 1 : 3);  // Commit / Absent / Nil
      for (int b = 0; b < 64; b++) sigs[64 * i + b] = (uint8_t)rng();
      sec[i] = 1700000000 + height;
      nan[i] = (int32_t)(rng() % 1000000000);
      slen[i] = rng() % 211 == 0 ? 63 : 64;
    }
    c.height = height;
    c.round = 0;
    c.block_id = tmed_block_id{hash.data(), 32, 1, psh.data(), 32};
    c.n_sigs = n;
    c.flags = flags.data();
    c.addresses = addrs.data();
    c.ts_seconds = sec.data();
    c.ts_nanos = nan.data();
    c.sigs = sigs.data();
    c.sig_lens = slen.data();
    c.address_lens = nullptr;
  }
};

// The device: one bit per staged position of group grp, in staging order (stage_group's layout).
void fake_device(const std::vector<tmed_commit_request> &reqs, const Cands &cands, const Group &grp,
                 std::vector<uint8_t> &bits) {
  const size_t m = grp.size(cands);
  bits.assign(m, 0);
  for_segments(cands, grp, 0, m, [&](size_t j, uint32_t u0, uint32_t u1, size_t p) {
    const Run &run = cands.runs[grp.run(cands, j)];
    const tmed_commit_request &r = reqs[run.req];
    for (uint32_t u = u0; u < u1; u++) {
      const size_t i = (size_t)(run.sig + (int32_t)u), v = (size_t)(run.val + (int32_t)u);
      bits[p + (u - u0)] = fake_bit(r.vals->pubkeys + 32 * v, r.commit->sigs + 64 * i);
    }
  });
}

// One shape's requests and what they point into.
struct Batch {
  std::vector<SetData> sets;
  std::vector<CommitData> commits;
  std::vector<tmed_commit_request> reqs;
  size_t aliases = 0, parts = 0, cands = 0, ngroups = 0, accepted = 0;
  // the light client's sets: set h + 1 is set h with one validator replaced (light/verifier.go).
  // KEYSETS > 1: blocks of 50 sets take the handles 0 (generic), 1 .. KEYSETS - 1 in turn, every key
  // with its index in one pool, so same_key's comparison of indexes tells what the bytes would
  void make(const std::string &kind, size_t headers, size_t nval, size_t keysets, std::mt19937_64 &rng) {
    static const char chain[] = "test_chain_id";
    uint32_t next_index = 0;
    uint32_t *pool = keysets > 1 ? &next_index : nullptr;
    const auto handle = [&](size_t h) { return keysets > 1 ? (uint64_t)((h / 50) % keysets) : 0; };
    sets.resize(headers + 1);
    sets[0].make(nval, rng, nullptr, 0, handle(0), pool);
    for (size_t h = 1; h <= headers; h++)
      sets[h].make(nval, rng, &sets[h - 1], (size_t)(rng() % nval), handle(h), pool);
    commits.resize(headers);
    for (size_t h = 0; h < headers; h++) commits[h].make(sets[h + 1], (int64_t)(h + 2), rng);
    // per header: the Trusting request against the trusted set, then the Light request against the
    // untrusted set on the SAME commit (pair_request aliases their shared verifications)
    for (size_t h = 0; h < headers; h++) {
      tmed_commit_request t{};
      t.mode = TMED_MODE_LIGHT_TRUSTING;
      t.chain_id = chain;
      t.chain_id_len = sizeof(chain) - 1;
      t.vals = &sets[h].vs;
      t.commit = &commits[h].c;
      t.trust_num = 1;
      t.trust_den = kind == "decided" && reqs.size() < 160 ? 0 : 3;
      if (kind != "light") reqs.push_back(t);
      tmed_commit_request l{};
      l.mode = TMED_MODE_LIGHT;
      l.chain_id = chain;
      l.chain_id_len = sizeof(chain) - 1;
      l.vals = &sets[h + 1].vs;
      l.block_id = &commits[h].c.block_id;
      l.height = commits[h].c.height + (kind == "decided" && reqs.size() < 160 ? 1 : 0);
      l.commit = &commits[h].c;
      reqs.push_back(l);
    }
  }
};

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void add(uint64_t x) { h = (h ^ x) * 1099511628211ull; }
  template <class V>
  void all(const V &v) {
    add(v.size());
    for (const auto &x : v) add((uint64_t)x);
  }
  void result(const tmed_commit_result &o) {
    const int64_t f[] = {o.code, o.got, o.needed, o.expected, o.actual, o.idx, o.idx_first, o.val_idx, o.verified};
    for (int64_t x : f) add((uint64_t)x);
  }
};

// What seam_plan hands on (see the head of the file); grp, tp: null for a call without them.
void plan_digest(Fnv &d, int rc, const std::vector<tmed_commit_request> &reqs, const tmed_commit_result *out,
                 const Plans &ps, const Cands &c, const Group *grp, const Templates *tp) {
  d.add((uint64_t)rc);
  for (size_t q = 0; q < reqs.size(); q++) {
    const Plan &pl = ps.v[q];
    const int64_t f[] = {pl.decided, pl.needed, pl.panic_idx, pl.stop, (int64_t)pl.cand_off, pl.ncand,
                         (int64_t)pl.run_lo, (int64_t)pl.run_hi, pl.dv_idx, pl.dv_val, pl.dv_first};
    for (int64_t x : f) d.add((uint64_t)x);
    if (pl.decided) d.result(out[q]);
    else if (reqs[q].mode == TMED_MODE_LIGHT_TRUSTING)
      for (size_t i = 0; i < reqs[q].commit->n_sigs; i++) d.add((uint64_t)pl.vof[i]);
  }
  d.add(c.runs.size());
  for (const Run &r : c.runs)
    for (uint64_t x : {(uint64_t)r.req, (uint64_t)r.sig, (uint64_t)r.val, (uint64_t)r.len}) d.add(x);
  d.all(c.off);
  d.add(c.alias.size());
  for (const auto &a : c.alias) { d.add(a.first); d.add(a.second); }
  d.all(c.tmpl_of);
  d.all(c.preq);
  d.all(c.pal);
  d.all(c.pseg);
  if (grp) { d.all(grp->rix); d.all(grp->ub); d.all(grp->pos); }
  if (!tp) return;
  d.add(tp->ready);
  if (!tp->ready) return;  // (not built by this call: the caller builds them with device_templates)
  d.add(tp->nrows);
  d.add(tp->fits);
  for (size_t b = 0; b < tp->nrows * tmed::kVoteTmplBytes; b++) d.add(tp->rows[b]);
  d.all(tp->row_of);
}

}  // namespace

int main(int argc, char **argv) {
  const int iters = argc > 3 ? atoi(argv[3]) : 3;
  const int jitter = argc > 4 ? atoi(argv[4]) : 0;
  const uint64_t seed = argc > 5 ? (uint64_t)atoll(argv[5]) : 7;
  const size_t keysets = argc > 6 ? (size_t)atol(argv[6]) : 1;
  const std::string spec = argc > 7 ? argv[7]
                                    : std::string("pairs:") + (argc > 1 ? argv[1] : "600") + ":" + (argc > 2 ? argv[2] : "48");
  g_pool_jitter_us.store(jitter);
  std::mt19937_64 rng(seed);
  std::vector<std::unique_ptr<Batch>> shapes;
  for (size_t at = 0; at < spec.size();) {
    const size_t end = std::min(spec.find(',', at), spec.size());
    const size_t c1 = spec.find(':', at), c2 = c1 == std::string::npos ? c1 : spec.find(':', c1 + 1);
    if (c2 == std::string::npos || c2 > end) { printf("bad shape\n"); return 1; }
    shapes.emplace_back(new Batch);
    shapes.back()->make(spec.substr(at, c1 - at), (size_t)atol(spec.c_str() + c1 + 1), (size_t)atol(spec.c_str() + c2 + 1),
                        keysets, rng);
    at = end + 1;
  }
  Fnv digest, plan;
  Plans ps;
  Cands cands;
  Group grp;
  Templates tp;
  std::vector<uint64_t> gkeys;
  std::vector<Group> groups;
  std::vector<uint8_t> bits, valid;
  for (int it = 0; it < iters; it++)
  for (auto &shape : shapes) {
    Batch &b = *shape;
    const std::vector<tmed_commit_request> &reqs = b.reqs;
    const size_t n = reqs.size();
    std::vector<tmed_commit_result> out(n);
    const bool piped = keysets <= 1;  // one key set: a pipelined batch; several: one seam call
    int rc = piped ? seam_plan(reqs.data(), n, out.data(), ps, cands, nullptr, &grp, &tp)
                   : seam_plan(reqs.data(), n, out.data(), ps, cands);
    plan_digest(plan, rc, reqs, out.data(), ps, cands, piped ? &grp : nullptr, piped ? &tp : nullptr);
    if (rc != TMED_OK) { printf("seam_plan rc %d\n", rc); return 1; }
    bool fits = tp.fits;
    if (!piped || (cands.size() && !tp.ready)) rc = device_templates(reqs.data(), n, cands, tp, &fits);
    if (rc != TMED_OK) { printf("device_templates rc %d\n", rc); return 1; }
    if (piped) {  // bs_pump / bs_finish
      fake_device(reqs, cands, grp, bits);
      rc = finish_batch(reqs.data(), n, out.data(), ps, cands, grp, bits.data(), valid, true);
    } else {  // run_seam / ctx_verify: one launch sequence per key set
      valid.assign(cands.size(), 0);
      group_by_keyset(reqs.data(), cands, gkeys, groups);
      b.ngroups = 0;
      for (const Group &g : groups) {
        if (g.size(cands) == 0) continue;
        b.ngroups++;
        fake_device(reqs, cands, g, bits);
        scatter_bits(reqs.data(), cands, g, bits.data(), valid.data());
      }
      copy_aliases(cands, valid.data());
      rc = seam_replay(reqs.data(), n, out.data(), ps, valid.data());
      // a pair at a block boundary has sets with different handles: never one verification for both
      const auto handle_of = [&](uint32_t cand) {
        const size_t r = (size_t)(std::upper_bound(cands.off.begin(), cands.off.end(), (size_t)cand) - cands.off.begin()) - 1;
        return reqs[cands.runs[r].req].vals->keyset;
      };
      for (const auto &a : cands.alias)
        if (handle_of(a.first) != handle_of(a.second)) { printf("alias across key sets\n"); return 1; }
    }
    if (rc != TMED_OK) { printf("finish rc %d\n", rc); return 1; }
    b.aliases = cands.alias.size();
    b.parts = cands.preq.size() ? cands.preq.size() - 1 : 0;
    b.cands = cands.size();
    b.accepted = 0;
    for (size_t q = 0; q < n; q++) {
      digest.result(out[q]);
      b.accepted += out[q].code == TMED_COMMIT_OK;
    }
  }
  for (auto &shape : shapes) {
    const Batch &b = *shape;
    if (&shape != &shapes[0]) printf("\n");
    printf("requests %zu candidates %zu aliases %zu parts %zu accepted %zu ", b.reqs.size(), b.cands, b.aliases, b.parts,
           b.accepted);
    if (keysets > 1) printf("groups %zu ", b.ngroups);
  }
  printf("plan %016llx digest %016llx\n", (unsigned long long)plan.h, (unsigned long long)digest.h);
  return 0;
}
