"""ZIP-215 as a context rule on the device: tmed_set_rule / tmed_rule, the keyed batch calls
tmed_verify_batch_keyset_zip215(_device), and every seam call under the rule (tmed_verify_commits,
tmed_blocksync_*, tmed_light_verify, tmed_verify_votes, tmed_verify_commits_multi) on the fixtures of
tests/zip_rule_cases.py, whose expected outcomes tests/test_zip_rule_seam_host.py pins on the CPU
(oracle.commit over oracle.zip215.verify).  Each context's rule is put back to the default before
the test leaves it."""
import contextlib

import numpy as np
import pytest

import light_cases as LC
import tmed.light as L
import tmed.types as T
import tmed.votes as V
import vote_cases as VC
import zip_rule_cases as ZR
from commit_cases import pbid, same, to_product
from conftest import engine_with_env
from oracle import zip215 as Z
from tmed._native import TmedError

pytestmark = pytest.mark.gpu

GO, ZIP = 0, 1
EINVAL = -1


@contextlib.contextmanager
def rule(eng, r):
    eng.set_rule(r)
    try:
        yield
    finally:
        eng.set_rule(GO)


@pytest.fixture(scope="module")
def cached():
    """A context with the seam's key-set cache on (the shared test context has it off: generic route)."""
    e = engine_with_env(TMED_KEYCACHE=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cached_thr():
    """The same with both latency modes off: a seam call's generic batch takes the throughput pipeline
    and its key-cached batch the throughput kernels (separate assemble_votes launch, message slots)."""
    e = engine_with_env(TMED_KEYCACHE=1, TMED_LAT_MAX=0, TMED_GLAT_MAX=0)
    yield e
    e.close()


def _request(mode, n, kind, at, **kw):
    vs, _, bid, h, cm = ZR.commit(n, kind, at, **kw)
    pv, pc = to_product(vs, cm)
    return (vs, bid, h, cm), (mode, pv, ZR.CHAIN, pbid(bid) if mode != T.MODE_LIGHT_TRUSTING else None, h, pc, 1, 3)


# ---- defaults, the setting itself ---------------------------------------------------------------

def test_rule_setting(engine):
    fresh = engine_with_env()
    try:
        assert fresh.rule() == GO
        fresh.set_rule(ZIP)
        assert fresh.rule() == ZIP
        for bad in (7, -1, 2):
            with pytest.raises(TmedError) as e:
                fresh.set_rule(bad)
            assert e.value.code == EINVAL
        assert fresh.rule() == ZIP
        fresh.set_rule(GO)
        assert fresh.rule() == GO
    finally:
        fresh.close()
    assert engine.rule() == GO


# ---- the keyed batch calls ----------------------------------------------------------------------

def _tiled(reps):
    keys, idx, sigs, lens, msgs, offs, go, zp = ZR.corpus()
    n, mb = len(idx), int(offs[-1])
    body = msgs[:mb]
    offs_t = np.concatenate([offs[:-1] + r * mb for r in range(reps)] + [np.array([reps * mb], np.uint32)]).astype(np.uint32)
    msgs_t = np.concatenate([body] * reps + [np.zeros(16, np.uint8)])
    return (keys, np.tile(idx, reps), np.tile(sigs, (reps, 1)), np.tile(lens, reps), msgs_t, offs_t, np.tile(go, reps),
            np.tile(zp, reps), n)


@pytest.mark.parametrize("route", ["latency", "throughput"])
def test_keyed_batch_corpus(engine, route):
    """Both golden files through tmed_verify_batch_keyset_zip215, host and _device, bit for bit against
    oracle.zip215.verify: at the default lat_max (the latency kernels: R from the R blocks where it is canonical) and
    with TMED_LAT_MAX=0 on the corpus three times over (4,266 signatures: the throughput kernels in
    key-grouped order).  The key set holds the files' keys that do not decode; some signatures are
    short (sig_lens); an index past the set is TMED_EINVAL on the host and a rejected signature on the
    device.  On the same handle tmed_verify_batch_keyset still gives the Go rule's bits, also while the
    context's seam rule is ZIP-215."""
    import torch
    eng = engine if route == "latency" else engine_with_env(TMED_LAT_MAX=0)
    keys, idx, sigs, lens, msgs, offs, go, zp, n1 = _tiled(1 if route == "latency" else 3)
    n = len(idx)
    assert route == "latency" or n >= 4096
    h = eng.keyset_load(keys)
    try:
        out = eng.verify_batch_keyset_zip215(h, idx, sigs, msgs, offs, lens)
        assert (out == zp).all(), np.flatnonzero(out != zp)[:10]
        with rule(eng, ZIP):  # the raw calls keep the rule their name states
            assert (eng.verify_keyset_arrays(h, idx, sigs, msgs, offs, lens) == go).all()
            assert (eng.verify_batch_keyset_zip215(h, idx, sigs, msgs, offs, lens) == zp).all()
        assert (eng.verify_keyset_arrays(h, idx, sigs, msgs, offs, lens) == go).all()
        bad = idx.copy()
        bad[5] = len(keys)
        with pytest.raises(TmedError) as e:
            eng.verify_batch_keyset_zip215(h, bad, sigs, msgs, offs, lens)
        assert e.value.code == EINVAL
        # the device form: no sig_lens, so a short signature is decided as its 64 staged bytes
        exp = zp.copy()
        for i in np.flatnonzero(lens[:n1] != 64):
            k, m = keys[idx[i]].tobytes(), msgs[int(offs[i]):int(offs[i + 1])].tobytes()
            exp[i::n1] = Z.verify(k, m, sigs[i].tobytes())
        past = np.arange(3, n, 211)
        bad = idx.copy()
        bad[past[::2]] = len(keys)
        bad[past[1::2]] = 0xFFFFFFFF
        exp[past] = 0
        dev = torch.device("cuda", 0)
        d_vi = torch.from_numpy(bad.view(np.int32)).to(dev)
        d_sig = torch.from_numpy(sigs).to(dev)
        d_msg = torch.from_numpy(msgs).to(dev)
        d_off = torch.from_numpy(offs.view(np.int32)).to(dev)
        d_out = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        eng.verify_batch_keyset_zip215_device(h, d_vi, d_sig, d_msg, d_off, d_out, n, 0)
        torch.cuda.synchronize(dev)
        got = d_out.cpu().numpy()
        assert (got == exp).all(), np.flatnonzero(got != exp)[:10]
    finally:
        eng.keyset_free(h)
        if eng is not engine:
            eng.close()


# ---- a commit the rules disagree on -------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 175])
@pytest.mark.parametrize("kind", ["torsion", "noncanon"])
def test_rule_switch_on_a_divergent_commit(engine, cached, cached_thr, n, kind):
    """VerifyCommit: WRONG_SIGNATURE at the divergent index under the Go rule, OK after
    tmed_set_rule(ZIP215), WRONG_SIGNATURE again after switching back; generic route (cache off) and
    key-cached route (warmed cache), the latter through the latency and the throughput kernels."""
    at = n // 2
    (vs, bid, h, cm), req = _request(T.MODE_COMMIT, n, kind, at)
    exp_go = ZR.expected(0, vs, bid, h, cm, rule="go")
    assert str(exp_go).startswith("wrong signature (#%d)" % at) and ZR.expected(0, vs, bid, h, cm, rule="zip") is None
    for eng in (engine, cached, cached_thr):
        if eng is not engine:
            eng.keycache_warm(req[1])
        s0 = eng.keycache_stats()
        assert same(T.verify_commits(eng, [req])[0], exp_go)
        with rule(eng, ZIP):
            assert T.verify_commits(eng, [req])[0] is None
        assert eng.rule() == GO
        assert same(T.verify_commits(eng, [req])[0], exp_go)
        s1 = eng.keycache_stats()
        if eng is not engine:  # every call found its set in the cache: the rule change invalidated nothing
            assert s1["keyed_sets"] - s0["keyed_sets"] == 3 and s1["generic_sets"] == s0["generic_sets"]


@pytest.mark.parametrize("kind", ["flip", "splusl", "flip_torsion"])
def test_bad_signatures_fail_under_both_rules(engine, cached, kind):
    for n in (4, 175):
        (vs, bid, h, cm), req = _request(T.MODE_COMMIT, n, kind, n // 2)
        exp = ZR.expected(0, vs, bid, h, cm, rule="go")
        assert str(exp).startswith("wrong signature (#%d)" % (n // 2))
        assert same(exp, ZR.expected(0, vs, bid, h, cm, rule="zip"))
        cached.keycache_warm(req[1])
        for eng in (engine, cached):
            assert same(T.verify_commits(eng, [req])[0], exp)
            with rule(eng, ZIP):
                assert same(T.verify_commits(eng, [req])[0], exp)


# ---- routes agree -------------------------------------------------------------------------------

def _mixed_requests():
    """(oracle tuples, requests): the divergent and the bad commits, the three modes."""
    spec = [(T.MODE_COMMIT, 175, "torsion", 87, {}), (T.MODE_COMMIT, 4, "noncanon", 2, {}),
            (T.MODE_LIGHT, 7, "torsion", 1, {}), (T.MODE_LIGHT_TRUSTING, 7, "torsion", 1, {}),
            (T.MODE_LIGHT, 7, "torsion", 1, {"flags": (3, 2, 3, 3, 3, 3, 3)}),
            (T.MODE_COMMIT, 175, "flip", 87, {}), (T.MODE_COMMIT, 7, None, 0, {})]
    pairs = [_request(m, n, k, at, **kw) for m, n, k, at, kw in spec]
    return [(m,) + p[0] for (m, *_), p in zip(spec, pairs)], [p[1] for p in pairs]


def _run(eng, reqs):
    pb = T.PreparedBatch(reqs)
    pb.run(eng)
    return [(pb.res[q].code, pb.res[q].got, pb.res[q].needed, pb.res[q].idx, pb.res[q].verified) for q in range(pb.n)]


def test_routes_agree(engine):
    """The same requests give identical tmed_commit_results, under each rule, with the key-set cache
    off (the generic single check), on the first call of a cached context (generic) and its second
    after tmed_keycache_wait (keyed), on a warmed cache, and through an explicit handle with a permuted
    keyset_index; and they are what oracle.commit says under that rule's verifier."""
    oracle, reqs = _mixed_requests()
    results = {}
    for r, name in ((GO, "go"), (ZIP, "zip")):
        with rule(engine, r):
            results[r] = _run(engine, reqs)
            errs = T.verify_commits(engine, reqs)
        for (mode, vs, bid, h, cm), got in zip(oracle, errs):
            assert same(got, ZR.expected(mode, vs, bid, h, cm, rule=name)), (mode, got)
    assert results[GO] != results[ZIP]
    # the LIGHT request that runs out of power: `got` differs between the rules by the divergent vote's power
    assert results[ZIP][4][:3] == (5, 10, 46) and results[GO][4][0] == 4 and results[GO][4][3] == 1
    first = engine_with_env(TMED_KEYCACHE=1)
    warm = engine_with_env(TMED_KEYCACHE=1)
    handles = []
    try:
        for r in (GO, ZIP):
            first.keycache_flush()
            with rule(first, r):
                s0 = first.keycache_stats()
                assert _run(first, reqs) == results[r]
                s1 = first.keycache_stats()
                assert s1["generic_sets"] > s0["generic_sets"]
                first.keycache_wait()
                assert _run(first, reqs) == results[r]
                s2 = first.keycache_stats()
                assert s2["keyed_sets"] > s1["keyed_sets"] and s2["generic_sets"] == s1["generic_sets"]
        for rq in reqs:
            warm.keycache_warm(rq[1])
        for r in (ZIP, GO):  # a rule change invalidates nothing
            with rule(warm, r):
                s0 = warm.keycache_stats()
                assert _run(warm, reqs) == results[r]
                s1 = warm.keycache_stats()
                assert s1["generic_sets"] == s0["generic_sets"] and s1["keyed_sets"] > s0["keyed_sets"]
        keyed = []
        for rq in reqs:
            vs = rq[1]
            n = len(vs.validators)
            perm = np.array([(3 * i + 1) % n for i in range(n)]) if n % 3 else np.array([(2 * i + 1) % n for i in range(n)])
            assert sorted(perm) == list(range(n))
            hnd = engine.keyset_load(vs.packed()[0][perm])
            handles.append(hnd)
            inv = np.zeros(n, np.uint32)
            inv[perm] = np.arange(n, dtype=np.uint32)
            keyed.append((rq[0], T.ValidatorSet(vs.validators, keyset=hnd, keyset_index=inv)) + tuple(rq[2:]))
        for r in (GO, ZIP):
            with rule(engine, r):
                assert _run(engine, keyed) == results[r]
    finally:
        for hnd in handles:
            engine.keyset_free(hnd)
        first.close()
        warm.close()


# ---- each seam under the rule -------------------------------------------------------------------

def test_blocksync_under_the_rule(engine, cached):
    """3 blocks x 7 validators, the middle block's commit with a divergent signature: tmed_blocksync_verify
    and tmed_blocksync_submit + tmed_blocksync_wait; a window is decided under the rule it was
    submitted under (tmed_set_rule collects it first)."""
    built = [ZR.commit(7, kind, 1, tag="bs", height=100 + i) for i, kind in enumerate((None, "torsion", "flip"))]
    vs = built[0][0]
    pv = to_product(vs, built[0][4])[0]
    bids = [pbid(b[2]) for b in built]
    heights = [b[3] for b in built]
    commits = [to_product(vs, b[4])[1] for b in built]
    exp = {name: [ZR.expected(1, vs, b[2], b[3], b[4], rule=name) for b in built] for name in ("go", "zip")}
    assert [e is None for e in exp["go"]] == [True, False, False] and [e is None for e in exp["zip"]] == [True, True, False]
    cached.keycache_warm(pv)
    for eng in (engine, cached):
        for r, name in ((GO, "go"), (ZIP, "zip"), (GO, "go")):
            with rule(eng, r):
                w = T.BlocksyncWindow(pv, ZR.CHAIN, bids, heights, commits)
                w.run(eng, 2)
                assert all(same(g, e) for g, e in zip(w.errors(), exp[name])), (name, w.errors())
                w2 = T.BlocksyncWindow(pv, ZR.CHAIN, bids, heights, commits)
                w2.submit(eng, 1)
                T.blocksync_wait(eng)
                assert all(same(g, e) for g, e in zip(w2.errors(), exp[name])), (name, w2.errors())
        # submitted under ZIP-215, collected by the switch back to the default
        eng.set_rule(ZIP)
        w3 = T.BlocksyncWindow(pv, ZR.CHAIN, bids, heights, commits)
        try:
            w3.submit(eng, 1)
        finally:
            eng.set_rule(GO)
        assert all(same(g, e) for g, e in zip(w3.errors(), exp["zip"])), w3.errors()
        T.blocksync_wait(eng)


def test_light_verify_under_the_rule(engine, cached):
    cases = ZR.light_cases()
    for eng in (engine, cached):
        for r, name in ((GO, "go"), (ZIP, "zip")):
            with rule(eng, r):
                sets = {}
                pl = L.PreparedLight([c.pair(sets) for c in cases])
                pl.run(eng)
                for q, c in enumerate(cases):
                    exp = ZR.light_expected(c, name)
                    assert (exp is None) == (name == "zip")
                    assert LC.same_outcome(pl.errors()[q], exp, pl.res[q].code), (c.name, name, pl.errors()[q])


def _zip_vote_expected(req, v):
    e = VC.expected(req, v)
    if e == V.VOTE_INVALID_SIGNATURE and len(v.signature) == 64:
        msg = VC.sign_bytes(req.chain_id, v)
        if ZR.verify_zip(req.vals.validators[v.validator_index].pub_key, msg, bytes(v.signature)):
            return V.VOTE_OK
    return e


@pytest.mark.parametrize("chain", [VC.CHAIN, "c" * 51])
@pytest.mark.parametrize("addvote", [False, True])
def test_votes_under_the_rule(engine, cached, cached_thr, chain, addvote):
    """8 votes, one divergent (VOTE_OK against VOTE_INVALID_SIGNATURE), one flipped (invalid under
    both): the device route and the host route of a long chain ID, with and without the addVote checks,
    generic and key-cached."""
    vals, seeds = VC.valset(8, "zipvotes")
    bid = VC.block_id("zipvotes")
    votes = [VC.signed(chain, vals, seeds, i, 1, 7, 2, bid) for i in range(8)]
    votes[3].signature = ZR.sign_torsion(seeds[3], VC.sign_bytes(chain, votes[3]))
    votes[6].signature = ZR.sign_noncanon(seeds[6], VC.sign_bytes(chain, votes[6]))
    votes[5].signature = VC.flip(votes[5].signature, 40)
    req = V.VoteRequest(chain, vals, votes, addvote, 7, 2, 1)
    exp_go = [VC.expected(req, v) for v in votes]
    exp_zip = [_zip_vote_expected(req, v) for v in votes]
    ok, bad = V.VOTE_OK, V.VOTE_INVALID_SIGNATURE
    assert exp_go == [ok, ok, ok, bad, ok, bad, bad, ok] and exp_zip == [ok, ok, ok, ok, ok, bad, ok, ok]
    for eng in (engine, cached, cached_thr):
        if eng is not engine:
            eng.keycache_warm(vals)
        assert [int(c) for c in V.verify_votes(eng, [req])] == exp_go
        with rule(eng, ZIP):
            assert [int(c) for c in V.verify_votes(eng, [req])] == exp_zip
        assert [int(c) for c in V.verify_votes(eng, [req])] == exp_go


def test_multi_needs_equal_rules(engine, cached):
    oracle, reqs = _mixed_requests()
    for r, name in ((GO, "go"), (ZIP, "zip")):
        with rule(engine, r):
            errs = T.verify_commits([engine, engine], reqs)
        for (mode, vs, bid, h, cm), got in zip(oracle, errs):
            assert same(got, ZR.expected(mode, vs, bid, h, cm, rule=name))
    with rule(cached, ZIP):
        with pytest.raises(TmedError) as e:
            T.verify_commits([engine, cached], reqs)
        assert e.value.code == EINVAL
    T.verify_commits([engine, cached], reqs)


# ---- what stays as it was -----------------------------------------------------------------------

def test_raw_batches_and_the_msm_entry_ignore_the_context_rule(engine):
    keys, idx, sigs, lens, msgs, offs, go, zp = ZR.corpus()
    pubs = keys[idx]
    with rule(engine, ZIP):
        assert (engine.verify_arrays(pubs, sigs, msgs, offs, lens) == go).all()
        assert (engine.verify_zip215_arrays(pubs, sigs, msgs, offs, lens) == zp).all()
        st = engine.zip215_stats()
    assert st["chunks"] == 1 and st["equations"] >= 1
    assert (engine.verify_zip215_arrays(pubs, sigs, msgs, offs, lens) == zp).all()
    assert engine.zip215_stats()["chunks"] == 1
