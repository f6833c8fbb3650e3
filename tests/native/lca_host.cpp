// lca_host.cpp — TEST-ONLY stand-alone host program: the host code of LightClientAttackEvidence
// (csrc/lca_free.h, csrc/lca_host.h: the attack kind, the candidates, GetByAddress, the ordering key,
// Hash(), and the replay of VerifyLightClientAttack) driven with stub hashes and a stub commit
// verifier.  tests/test_lca_host.py builds it through tests/native/lca_host.mk with
// -fsanitize=address,undefined and runs it as a plain executable.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lca_host.h"

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "lca_host.cpp:%d: %s\n", __LINE__, #c);   \
      return 1;                                                 \
    }                                                           \
  } while (0)

namespace {

// A set of n validators: address v = 20 bytes of `fill` with byte `at` set to order[v].
struct Set {
  std::vector<uint8_t> addr, pub;
  std::vector<int64_t> pow;
  tmed_valset vs;
  Set(size_t n, int at, const uint8_t *order, const int64_t *powers, uint8_t fill = 0x55) : addr(20 * n, fill), pub(32 * n), pow(n) {
    for (size_t v = 0; v < n; v++) {
      addr[20 * v + at] = order[v];
      pow[v] = powers ? powers[v] : 10;
    }
    memset(&vs, 0, sizeof(vs));
    vs.n = n;
    vs.pubkeys = pub.data();
    vs.powers = pow.data();
    vs.addresses = addr.data();
    for (size_t v = 0; v < n; v++) vs.total_power += pow[v];
  }
};

// A commit of n signatures with the addresses of `set` in set order and the given flags.
struct Commit {
  std::vector<uint8_t> flags, addr;
  tmed_commit c;
  Commit(const Set &set, const std::vector<uint8_t> &f, int32_t round) : flags(f), addr(set.addr.begin(), set.addr.begin() + 20 * f.size()) {
    memset(&c, 0, sizeof(c));
    c.round = round;
    c.n_sigs = f.size();
    c.flags = flags.data();
    c.addresses = addr.data();
  }
};

int ordering() {
  using namespace tmed;
  // bytes.Compare is on bytes: addresses that differ only in byte 0, 3, 4 or 19, all powers equal
  const uint8_t order[4] = {0x02, 0x01, 0xff, 0x00};
  for (int at : {0, 3, 4, 19}) {
    Set common(4, at, order, nullptr), other(1, 0, order, nullptr, 0x11);
    Commit cm(common, {2, 2, 2, 2}, 1), tc(common, {2, 2, 2, 2}, 1);
    const uint8_t h1[32] = {1}, h2[32] = {2};
    tmed_header a, b;
    memset(&a, 0, sizeof(a));
    memset(&b, 0, sizeof(b));
    a.hashes[5] = h1, a.hash_lens[5] = 32;  // AppHash differs: lunatic
    b.hashes[5] = h2, b.hash_lens[5] = 32;
    tmed_lca_request r;
    memset(&r, 0, sizeof(r));
    r.conflicting_header = &a, r.trusted_header = &b, r.conflicting_commit = &cm.c, r.trusted_commit = &tc.c;
    r.conflicting_vals = &other.vs, r.common_vals = &common.vs, r.byz_is_nil = 1;
    int32_t list[4] = {-9, -9, -9, -9};
    const uint64_t off[2] = {0, 4};
    tmed_byz_result o;
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK);
    CHECK(o.kind == TMED_LCA_LUNATIC && o.state == TMED_BYZ_OK && o.count == 4);
    CHECK(list[0] == 3 && list[1] == 1 && list[2] == 0 && list[3] == 2);
    // powers: descending as int64, differing only above bit 32, 0 and MaxInt64 / 8
    const int64_t pw[4] = {0, (int64_t)1 << 40, INT64_MAX / 8, ((int64_t)1 << 40) + ((int64_t)1 << 33)};
    Set rich(4, at, order, pw);
    r.common_vals = &rich.vs;
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK && o.count == 4);
    CHECK(list[0] == 2 && list[1] == 3 && list[2] == 1 && list[3] == 0);
    // equivocation: the same hashes and rounds; sig 1 absent in the trusted commit, sig 3 of a 19-byte address
    r.trusted_header = &a;
    r.conflicting_vals = &common.vs;
    Commit t2(common, {2, 1, 3, 2}, 1);
    r.trusted_commit = &t2.c;
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK);
    CHECK(o.kind == TMED_LCA_EQUIVOCATION && o.count == 3 && list[0] == 3 && list[1] == 0 && list[2] == 2);
    const uint32_t lens[4] = {20, 20, 20, 19};
    cm.c.address_lens = lens;
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK && o.state == TMED_BYZ_PANIC && o.count == 0);
    Commit t3(common, {1, 1, 1, 2}, 1);
    r.trusted_commit = &t3.c;  // one candidate, nobody found: one nil entry
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK && o.state == TMED_BYZ_OK && o.count == 1 &&
          list[0] == -1);
    Commit t4(common, {2, 2}, 1);
    r.trusted_commit = &t4.c;  // index out of range at sig 2
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK && o.state == TMED_BYZ_PANIC);
    Commit t5(common, {2, 2, 2, 2}, 0);
    r.trusted_commit = &t5.c;  // another round: amnesia
    CHECK(tmed_lca::byzantine_validators_host(&r, 1, list, off, &o) == TMED_OK && o.kind == TMED_LCA_AMNESIA && o.count == 0);
  }
  return 0;
}

int hashes() {
  // 01 .. 20 and CommonHeight 64: SHA-256(01 .. 1f 00 80 01)
  uint8_t hh[32], out[32];
  for (int k = 0; k < 32; k++) hh[k] = (uint8_t)(k + 1);
  const uint8_t want[32] = {0x16, 0x9e, 0xa0, 0x12, 0x20, 0x04, 0x3b, 0x69, 0xad, 0x12, 0xa0, 0x99, 0x62, 0x27, 0x47, 0x4e,
                            0x2a, 0x96, 0x8d, 0xab, 0x0c, 0x12, 0x23, 0x6e, 0x55, 0x79, 0x98, 0x0a, 0xb8, 0x93, 0x08, 0x7d};
  tmed_lca::evidence_hash_host(hh, true, 64, out);
  CHECK(!memcmp(out, want, 32));
  hh[31] ^= 0xff;  // byte 31 is not copied
  tmed_lca::evidence_hash_host(hh, true, 64, out);
  CHECK(!memcmp(out, want, 32));
  const uint8_t nil1[32] = {0x58, 0xcc, 0x2f, 0x44, 0xd3, 0xa2, 0x78, 0x66, 0x87, 0x47, 0x01, 0xfb, 0xad, 0x57, 0x3d, 0xa9,
                            0xad, 0x1c, 0xfd, 0x88, 0xfa, 0x31, 0x45, 0x53, 0x1c, 0x82, 0x2f, 0x20, 0xa5, 0x8b, 0xee, 0xa1};
  tmed_lca::evidence_hash_host(nullptr, false, 1, out);
  CHECK(!memcmp(out, nil1, 32));
  for (int64_t h : {(int64_t)0, (int64_t)-1, (int64_t)1 << 31, (int64_t)1 << 62, INT64_MAX, INT64_MIN})
    tmed_lca::evidence_hash_host(hh, true, h, out);  // every varint length, under the sanitizers
  return 0;
}

int replay() {
  const uint8_t order[3] = {3, 1, 2};
  Set vals(3, 19, order, nullptr);
  Commit cm(vals, {2, 2, 2}, 1), tc(vals, {2, 2, 2}, 1);
  const uint8_t app1[32] = {1}, app2[32] = {2};
  const char chain[] = "c";
  // request 0: equivocation, fine; 1: lunatic at the same height: NOT_DERIVED; 2: lunatic whose Trusting
  // fails; 3: wrong total power; 4: same hash; 5: a claimed address differs; 6: GO_PATH
  const int kN = 7;
  tmed_header ch[kN], th[kN];
  tmed_lca_request rq[kN];
  const uint8_t claimed[60] = {0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55,
                               0x55, 0x55, 0x55, 0x55, 0x55, 1,    0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55,
                               0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 2,    0x55, 0x55,
                               0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55, 0x55,
                               0x55, 0x55, 0x55, 3};
  uint8_t wrong[60];
  memcpy(wrong, claimed, 60);
  wrong[39] = 9;
  const int64_t cp[3] = {10, 10, 10};
  for (int i = 0; i < kN; i++) {
    memset(&ch[i], 0, sizeof(tmed_header));
    ch[i].chain_id = chain, ch[i].chain_id_len = 1, ch[i].height = 10, ch[i].time_seconds = 100;
    ch[i].hashes[5] = app1, ch[i].hash_lens[5] = 32;
    th[i] = ch[i];
    if (i == 1 || i == 2) th[i].hashes[5] = app2;
    memset(&rq[i], 0, sizeof(rq[i]));
    rq[i].conflicting_header = &ch[i], rq[i].trusted_header = &th[i];
    rq[i].conflicting_commit = &cm.c, rq[i].trusted_commit = &tc.c;
    rq[i].conflicting_vals = rq[i].common_vals = &vals.vs;
    rq[i].common_height = 10, rq[i].common_header_height = i == 2 ? 4 : 10;
    rq[i].total_voting_power = i == 3 ? 31 : 30;
    rq[i].n_byz = 3, rq[i].byz_addresses = i == 5 ? wrong : claimed, rq[i].byz_powers = cp;
  }
  th[6].time_nanos = 1000000000;
  int32_t byz[3 * kN];
  uint64_t off[kN + 1];
  for (int i = 0; i <= kN; i++) off[i] = 3 * (uint64_t)i;
  tmed_lca_result res[kN];
  size_t hashed = 0, sent = 0, lists = 0;
  const int rc = tmed_lca::lca_run(
      rq, kN, 0u, byz, off, res,
      [&](const std::vector<size_t> &live, uint8_t *c, uint8_t *cok, uint8_t *t, uint8_t *tok) {
        hashed = live.size();
        for (const size_t i : live) {
          memset(c + 32 * i, 7, 32);
          memset(t + 32 * i, i == 4 ? 7 : 8, 32);
          cok[i] = tok[i] = 1;
        }
        return (int)TMED_OK;
      },
      [&](const tmed_commit_request *c, size_t m, tmed_commit_result *o) {
        sent = m;
        for (size_t q = 0; q < m; q++) {
          memset(&o[q], 0, sizeof(o[q]));
          o[q].verified = 3;
          if (c[q].mode == TMED_MODE_LIGHT_TRUSTING) o[q].code = TMED_COMMIT_NOT_ENOUGH_POWER;
          if (c[q].chain_id_len != 1 || c[q].height != (c[q].mode == TMED_MODE_LIGHT ? 10 : 0)) return (int)TMED_EINVAL;
        }
        return (int)TMED_OK;
      },
      [&](const std::vector<size_t> &live, const uint8_t *c, const uint8_t *cok, const std::vector<size_t> &need,
          const int *kinds, tmed_byz_result *bres, uint8_t *ev_hash) {
        lists = need.size();
        return tmed_lca::tail_host(rq, live, c, cok, need, kinds, byz, off, bres, ev_hash);
      });
  CHECK(rc == TMED_OK);
  CHECK(hashed == 5 && sent == 6 && lists == 2);
  CHECK(res[0].code == TMED_LCA_OK && res[0].kind == TMED_LCA_EQUIVOCATION && res[0].n_byz_expected == 3 &&
        res[0].verified_light == 3 && res[0].verified_trusting == 0);
  CHECK(byz[0] == 1 && byz[1] == 2 && byz[2] == 0);
  CHECK(res[1].code == TMED_LCA_NOT_DERIVED && res[1].kind == TMED_LCA_LUNATIC);
  CHECK(res[2].code == TMED_LCA_TRUSTING && res[2].commit.code == TMED_COMMIT_NOT_ENOUGH_POWER && res[2].verified_trusting == 3);
  CHECK(res[3].code == TMED_LCA_TOTAL_POWER && res[3].expected == 31 && res[3].actual == 30);
  CHECK(res[4].code == TMED_LCA_SAME_HASH);
  CHECK(res[5].code == TMED_LCA_BYZ_ADDRESS && res[5].idx == 1 && res[5].val_idx == 2);
  CHECK(res[6].code == TMED_LCA_GO_PATH);
  uint8_t zero[32] = {0};
  CHECK(memcmp(res[0].hash, zero, 32) != 0 && !memcmp(res[0].hash, res[4].hash, 32) && !memcmp(res[1].hash, zero, 32));
  // malformed calls
  auto nohash = [](const std::vector<size_t> &, uint8_t *, uint8_t *, uint8_t *, uint8_t *) { return (int)TMED_OK; };
  auto nocommit = [](const tmed_commit_request *, size_t, tmed_commit_result *) { return (int)TMED_OK; };
  auto notail = [](const std::vector<size_t> &, const uint8_t *, const uint8_t *, const std::vector<size_t> &, const int *,
                   tmed_byz_result *, uint8_t *) { return (int)TMED_OK; };
  CHECK(tmed_lca::lca_run(rq, 1, 1u, byz, off, res, nohash, nocommit, notail) == TMED_EINVAL);
  CHECK(tmed_lca::lca_run(nullptr, 1, 0u, byz, off, res, nohash, nocommit, notail) == TMED_EINVAL);
  CHECK(tmed_lca::lca_run(rq, 0, 0u, nullptr, nullptr, nullptr, nohash, nocommit, notail) == TMED_OK);
  tmed_lca_request bad = rq[0];
  bad.common_vals = nullptr;
  CHECK(tmed_lca::lca_run(&bad, 1, 0u, byz, off, res, nohash, nocommit, notail) == TMED_EINVAL);
  bad = rq[0];
  bad.byz_is_nil = 1;  // a nil list of three
  CHECK(tmed_lca::lca_run(&bad, 1, 0u, byz, off, res, nohash, nocommit, notail) == TMED_EINVAL);
  const uint64_t tight[2] = {0, 2};  // a range shorter than the commit
  CHECK(tmed_lca::lca_run(rq, 1, 0u, byz, tight, res, nohash, nocommit, notail) == TMED_EINVAL);
  return 0;
}

}  // namespace

int main() {
  if (ordering() || hashes() || replay()) return 1;
  printf("lca-ok\n");
  return 0;
}
