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
// usage: seam_race HEADERS VALIDATORS ITERATIONS JITTER_US SEED [KEYSETS]
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
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

}  // namespace

int main(int argc, char **argv) {
  const size_t headers = argc > 1 ? (size_t)atol(argv[1]) : 600;
  const size_t nval = argc > 2 ? (size_t)atol(argv[2]) : 48;
  const int iters = argc > 3 ? atoi(argv[3]) : 3;
  const int jitter = argc > 4 ? atoi(argv[4]) : 0;
  const uint64_t seed = argc > 5 ? (uint64_t)atoll(argv[5]) : 7;
  const size_t keysets = argc > 6 ? (size_t)atol(argv[6]) : 1;
  g_pool_jitter_us.store(jitter);
  std::mt19937_64 rng(seed);
  // the light client's sets: set h + 1 is set h with one validator replaced (light/verifier.go).
  // KEYSETS > 1: blocks of 50 sets take the handles 0 (generic), 1 .. KEYSETS - 1 in turn, every key
  // with its index in one pool, so same_key's comparison of indexes tells what the bytes would
  uint32_t next_index = 0;
  uint32_t *pool = keysets > 1 ? &next_index : nullptr;
  const auto handle = [&](size_t h) { return keysets > 1 ? (uint64_t)((h / 50) % keysets) : 0; };
  std::vector<SetData> sets(headers + 1);
  sets[0].make(nval, rng, nullptr, 0, handle(0), pool);
  for (size_t h = 1; h <= headers; h++)
    sets[h].make(nval, rng, &sets[h - 1], (size_t)(rng() % nval), handle(h), pool);
  std::vector<CommitData> commits(headers);
  for (size_t h = 0; h < headers; h++) commits[h].make(sets[h + 1], (int64_t)(h + 2), rng);
  const char chain[] = "test_chain_id";
  // per header: the Trusting request against the trusted set, then the Light request against the
  // untrusted set on the SAME commit (pair_request aliases their shared verifications)
  std::vector<tmed_commit_request> reqs;
  for (size_t h = 0; h < headers; h++) {
    tmed_commit_request t{};
    t.mode = TMED_MODE_LIGHT_TRUSTING;
    t.chain_id = chain;
    t.chain_id_len = sizeof(chain) - 1;
    t.vals = &sets[h].vs;
    t.commit = &commits[h].c;
    t.trust_num = 1;
    t.trust_den = 3;
    reqs.push_back(t);
    tmed_commit_request l{};
    l.mode = TMED_MODE_LIGHT;
    l.chain_id = chain;
    l.chain_id_len = sizeof(chain) - 1;
    l.vals = &sets[h + 1].vs;
    l.block_id = &commits[h].c.block_id;
    l.height = commits[h].c.height;
    l.commit = &commits[h].c;
    reqs.push_back(l);
  }
  const size_t n = reqs.size();
  uint64_t digest = 1469598103934665603ull;
  size_t aliases = 0, parts = 0, cands_total = 0, ngroups = 0;
  Plans ps;
  Cands cands;
  Group grp;
  Templates tp;
  std::vector<uint64_t> gkeys;
  std::vector<Group> groups;
  std::vector<uint8_t> bits, valid;
  for (int it = 0; it < iters; it++) {
    std::vector<tmed_commit_result> out(n);
    const bool piped = keysets <= 1;  // one key set: a pipelined batch; several: one seam call
    int rc = piped ? seam_plan(reqs.data(), n, out.data(), ps, cands, nullptr, &grp, &tp)
                   : seam_plan(reqs.data(), n, out.data(), ps, cands);
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
      ngroups = 0;
      for (const Group &g : groups) {
        if (g.size(cands) == 0) continue;
        ngroups++;
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
    aliases = cands.alias.size();
    parts = cands.preq.size() ? cands.preq.size() - 1 : 0;
    cands_total = cands.size();
    for (size_t q = 0; q < n; q++) {
      const tmed_commit_result &o = out[q];
      const int64_t f[] = {o.code, o.got, o.needed, o.expected, o.actual, o.idx, o.idx_first, o.val_idx, o.verified};
      for (int64_t x : f) digest = (digest ^ (uint64_t)x) * 1099511628211ull;
    }
  }
  printf("requests %zu candidates %zu aliases %zu parts %zu ", n, cands_total, aliases, parts);
  if (keysets > 1) printf("groups %zu ", ngroups);
  printf("digest %016llx\n", (unsigned long long)digest);
  return 0;
  return 0;
}
