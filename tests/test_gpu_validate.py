"""validateBlock on the device: tmed_validate_blocks against the restatement (tests/validate_cases.py) and
against the composition of the seven existing calls (tmed_commit_hashes, tmed_txs_hashes,
tmed_evidence_hashes, tmed_header_hashes, tmed_valset_hashes, tmed_median_times and the engine's batch
verifier, replayed by tmed_validate_blocks_with).  Every comparison is exact: result struct against
restatement, fused call against composition."""
import contextlib
import json
import os
from dataclasses import replace

import numpy as np
import pytest

import evidence_cases as EC
import tmed.evidence as E
import tmed.merkle as MK
import tmed.state as S
import tmed.types as T
import validate_cases as VC
import zip_rule_cases as ZR
from conftest import engine_with_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 4, 63, 64, 65, 129)  # the scan's stride is 64 lanes
COUNTS = (1, 3, 4, 5, 65)        # four wavefronts a workgroup: the tail, and more than one workgroup


@pytest.fixture(scope="module")
def world():
    return VC.make_world(4, 67)


@pytest.fixture(scope="module")
def cached_engine():
    e = engine_with_env(TMED_KEYCACHE=1)
    yield e
    e.close()


def result_bytes(pb):
    return [bytes(pb.res[q]) for q in range(pb.n)]


def check(eng, cases, exp=None):
    """One fused call against the restatement; returns the PreparedBlocks."""
    pb = S.PreparedBlocks([c.request() for c in cases])
    pb.run(eng)
    exp = VC.expected(cases) if exp is None else exp
    for q, (c, (code, err, skipped), got) in enumerate(zip(cases, exp, pb.errors())):
        assert pb.res[q].code == code, (c.name, S.VB_CODE_NAMES[pb.res[q].code], S.VB_CODE_NAMES[code])
        assert VC.same(got, err), (c.name, got, err)
        assert pb.res[q].skipped == skipped, (c.name, pb.res[q].skipped, skipped)
    return pb


def composed(eng, cases):
    """The route there was before the call: the seven entry points, the proposer scan on the host, and the
    replay fed with their results."""
    n = len(cases)
    blocks = [c.block for c in cases]
    commits = [b.last_commit if b.last_commit is not None else T.Commit(0, 0, T.BlockID(), []) for b in blocks]
    ch, cok = MK.CommitHashBatch(commits).run(eng)
    dh = np.array([np.frombuffer(h, np.uint8) for h in MK.txs_hashes(eng, [list(b.txs) for b in blocks])])
    dup, lists, eok = [], [], np.ones(n, np.uint8)
    for b in blocks:
        lst = []
        for e in b.evidence:
            if isinstance(e, (bytes, bytearray)):
                lst.append(bytes(e))
            else:
                lst.append(len(dup))
                dup.append(e)
        lists.append(lst)
    _, roots = E.evidence_hashes(eng, dup, lists)
    eh = np.zeros((n, 32), np.uint8)
    for i, r in enumerate(roots):
        if r is None:
            eok[i] = 0
        else:
            eh[i] = np.frombuffer(r, np.uint8)
    hh, hok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    for i, h in enumerate(MK.header_hashes(eng, [b.header for b in blocks])):
        if h is not None:
            hh[i], hok[i] = np.frombuffer(h, np.uint8), 1
    sets = {}
    for c in cases:
        for vs in (c.state.validators, c.state.next_validators):
            if vs is not None:
                sets.setdefault(id(vs), vs)
    hashes = dict(zip(sets.keys(), MK.valset_hashes(eng, list(sets.values()))))
    vh, nh = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    prop, med = np.full(n, -1, np.int32), []
    pairs, at = [], {}
    for i, c in enumerate(cases):
        st, b = c.state, c.block
        if st.validators is not None:
            vh[i] = np.frombuffer(hashes[id(st.validators)], np.uint8)
            if len(b.header["proposer_address"]) == 20:  # state.Validators.HasAddress: the host scan
                prop[i] = VC.MC.get_by_address(st.validators, b.header["proposer_address"])[0]
        if st.next_validators is not None:
            nh[i] = np.frombuffer(hashes[id(st.next_validators)], np.uint8)
        if b.last_commit is not None and st.last_validators is not None:
            at[i] = len(pairs)
            pairs.append((b.last_commit, st.last_validators))
    res = S.median_times(eng, pairs)
    med = [res[at[i]] if i in at else (S.MEDIAN_GO_PATH, (0, 0)) for i in range(n)]

    def verifier(pubs, sigs, lens, msgs, offs):
        out = eng.verify_arrays(pubs, sigs, msgs, offs)
        out[lens != 64] = 0
        return out

    pb = S.PreparedBlocks([c.request() for c in cases])
    pb.run_with(verifier, ch, cok, dh, eh, eok, hh, hok, vh, nh, med, prop)
    return pb


def check_both(eng, cases):
    fused = check(eng, cases)
    assert result_bytes(fused) == result_bytes(composed(eng, cases))
    return fused


def engine_signer(eng):
    """signer(seeds, msgs) for validate_cases.make_world through tmed_sign_batch: one call per commit."""
    def sign(seeds, msgs):
        offs = np.zeros(len(msgs) + 1, np.uint32)
        np.cumsum([len(m) for m in msgs], out=offs[1:])
        sigs, _ = eng.sign_arrays(np.array([np.frombuffer(s, np.uint8) for s in seeds]),
                                  np.frombuffer(b"".join(msgs) + bytes(16), np.uint8).copy(), offs)
        return [bytes(s) for s in sigs]
    return sign


# ----------------------------------------------------------------------------- every code, precedence, skips

def test_every_code_once(engine, world):
    scen = VC.code_cases(world)
    assert {code for _, code in scen} == set(range(27))
    pb = check_both(engine, [c for c, _ in scen])
    for q, (c, code) in enumerate(scen):
        assert pb.res[q].code == code, (c.name, pb.res[q].code)
        if code != S.VB_GO_PATH and 0 < code < S.VB_LAST_COMMIT:
            assert pb.res[q].verified == 0, c.name  # decided before the commit: no signature sent
    by = {c.name: pb.res[q] for q, (c, _) in enumerate(scen)}
    assert bytes(by["LAST_COMMIT_HASH"].hash) == VC.commit_hash(world.blocks[2].last_commit)
    assert bytes(by["DATA_HASH"].hash) == VC.BH.txs_hash(world.blocks[2].txs)
    assert bytes(by["VALIDATORS_HASH"].hash) == VC.valset_hash(world.vals)
    assert (by["TIME_NOT_MEDIAN"].median_seconds, by["TIME_NOT_MEDIAN"].median_nanos) == tuple(world.blocks[2].header["time"])
    assert by["ok"].proposer_idx == 0 and by["ok"].verified == 4


def test_precedence_and_unknown_fields(engine, world):
    scen = VC.pair_cases(world)
    pb = check_both(engine, [c for c, _ in scen])
    for q, (c, code) in enumerate(scen):
        assert pb.res[q].code == code, c.name
    known = VC.known_cases(world)
    pb = check_both(engine, [c for c, _ in known])
    for q, (c, bit) in enumerate(known):
        assert pb.res[q].code == S.VB_OK and pb.res[q].skipped == bit, c.name
    blk, st = world.blocks[2], world.states[2]
    spec = replace(st, validators=None, next_validators=None, known=S.KNOW_ALL & ~(S.KNOW_VALIDATORS | S.KNOW_NEXT_VALIDATORS))
    pb = check(engine, [VC.Case("no sets", VC.with_header(blk, proposer_address=bytes(20)), spec)])
    assert pb.res[0].code == S.VB_OK and pb.res[0].proposer_idx == -1


def test_initial_height(engine, world):
    scen = VC.initial_cases(world)
    pb = check_both(engine, [c for c, _ in scen])
    assert [pb.res[q].code for q in range(3)] == [S.VB_OK, S.VB_INITIAL_HAS_SIGS, S.VB_TIME_NOT_GENESIS]
    assert [pb.res[q].verified for q in range(3)] == [0, 0, 0]


# ----------------------------------------------------------------------------- the lookup's stride

@pytest.mark.parametrize("n", SIZES)
def test_set_sizes_and_proposer_positions(engine, n):
    """The proposer at index 0, 63, 64, at the last index, absent, and at an address the set holds twice
    (the first index is reported)."""
    w = VC.make_world(n, 2, tag="size%d" % n)
    blk, st = w.blocks[1], w.states[1]
    stranger = T.address_of(bytes(31) + b"\x07")
    cases, want = [], []
    for at in sorted({0, 63, 64, n - 1}):
        if at < n:
            cases.append(VC.Case("at %d" % at, VC.with_header(blk, proposer_address=w.vals.validators[at].address), st))
            want.append(at)
    cases.append(VC.Case("absent", VC.with_header(blk, proposer_address=stranger), st))
    want.append(-1)
    pb = check_both(engine, cases)
    assert [pb.res[q].proposer_idx for q in range(len(cases))] == want
    assert pb.res[len(cases) - 1].code == S.VB_PROPOSER_UNKNOWN
    if n >= 4:  # validators n - 3 and n - 1 share an address: GetByAddress finds the first
        first, last = n - 3, n - 1
        d = VC.make_world(n, 2, tag="size%d" % n,
                          address_of=lambda i: w.vals.validators[first if i == last else i].address)
        dup = VC.Case("twice", VC.with_header(d.blocks[1], proposer_address=d.vals.validators[last].address), d.states[1])
        pb = check_both(engine, [dup])
        assert pb.res[0].code == S.VB_OK and pb.res[0].proposer_idx == first


# ----------------------------------------------------------------------------- block counts, linked windows

@pytest.mark.parametrize("count", COUNTS)
def test_block_counts(engine, world, count):
    pb = check_both(engine, VC.window(world, 1, count))
    assert [pb.res[q].code for q in range(count)] == [S.VB_OK] * count
    assert S.validate_stats(engine) == (1, 1, count)


def test_speculative_window_and_broken_links(engine, world):
    pb = check_both(engine, VC.window(world, 1, 5, known=0))
    assert [(pb.res[q].code, pb.res[q].skipped) for q in range(5)] == [(S.VB_OK, S.KNOW_ALL)] * 5
    for name, cases, code in VC.broken_links(world):
        pb = check_both(engine, cases)
        assert pb.res[0].code == S.VB_OK and pb.res[1].code == code, name


def test_linked_window_hashes_each_set_once(cached_engine, world):
    """A linked window of 5 over a constant set: one ValidatorSet.Hash, one staging of its addresses, and
    one resolution of the set by the commit seam's key-set cache."""
    cases = VC.window(world, 1, 5)
    s0 = cached_engine.keycache_stats()
    check(cached_engine, cases)
    s1 = cached_engine.keycache_stats()
    assert S.validate_stats(cached_engine) == (1, 1, 5)
    assert s1["lookups"] - s0["lookups"] == 1
    cached_engine.keycache_wait()
    check(cached_engine, cases)  # the warm route: keyed kernels
    s2 = cached_engine.keycache_stats()
    assert s2["keyed_sets"] - s1["keyed_sets"] == 1 and s2["lookups"] - s1["lookups"] == 1


def test_mixed_call_neighbours_unaffected(engine, world):
    """Hash mismatches, a bad signature and a GO_PATH request in the middle of a 65-block call of
    unlinked requests: the other 60 are OK."""
    cases = [VC.Case("b%d" % k, world.blocks[k], world.states[k]) for k in range(1, 66)]
    muts = VC.code_mutators(world)
    bad = {30: S.VB_DATA_HASH, 31: S.VB_VALIDATORS_HASH, 32: S.VB_LAST_COMMIT_HASH, 33: S.VB_GO_PATH, 34: S.VB_LAST_COMMIT}
    for q, code in bad.items():
        b, s = muts[code](cases[q].block, cases[q].state)
        cases[q] = VC.Case(cases[q].name, b, s)
    pb = check_both(engine, cases)
    assert [pb.res[q].code for q in range(65)] == [bad.get(q, S.VB_OK) for q in range(65)]


def test_stale_scratch(engine, world):
    """A large call, then a small one whose results share none of the first's."""
    check(engine, VC.window(world, 1, 65))
    scen = VC.code_cases(world)[:6]
    pb = check_both(engine, [c for c, _ in scen])
    assert [pb.res[q].code for q in range(6)] == [code for _, code in scen]


# ----------------------------------------------------------------------------- the median kernels' shapes

def test_513_signatures(engine):
    """One block whose LastCommit has 513 signatures made by tmed_sign_batch: the median's block shape
    (the wave shape ends at 512; the sizes above take the wave shape)."""
    w = VC.make_world(513, 2, tag="big", signer=engine_signer(engine), txs_per_block=1)
    pb = check_both(engine, [VC.Case("513", w.blocks[1], w.states[1])])
    assert pb.res[0].code == S.VB_OK and pb.res[0].verified == 513
    late = VC.with_header(w.blocks[1], time=(w.blocks[1].header["time"][0], w.blocks[1].header["time"][1] + 1))
    pb = check(engine, [VC.Case("513 late", late, w.states[1])])
    assert pb.res[0].code == S.VB_TIME_NOT_MEDIAN
    assert (pb.res[0].median_seconds, pb.res[0].median_nanos) == tuple(w.blocks[1].header["time"])


# ----------------------------------------------------------------------------- evidence in the blocks

def test_blocks_with_evidence(engine):
    """Duplicate-vote evidence and an opaque item in the lists: the evidence hash of each block's own list."""
    vals, seeds = EC.valset(4, tag="vbev")
    evs = [EC.dup(EC.CHAIN, vals, seeds, i % 4, k=i) for i in range(3)]
    w = VC.make_world(4, 4, tag="evw", evidence_at=lambda h: {2: evs[:2], 3: [evs[2], b"opaque-lca-evidence"]}.get(h, []))
    cases = VC.window(w, 1, 3)
    pb = check_both(engine, cases)
    assert [pb.res[q].code for q in range(3)] == [S.VB_OK] * 3
    wrong = replace(cases[1], block=replace(cases[1].block, evidence=[evs[0]]))
    pb = check_both(engine, [cases[0], wrong])
    assert pb.res[1].code == S.VB_EVIDENCE_HASH and bytes(pb.res[1].hash) == VC.evidence_hash([evs[0]])


# ----------------------------------------------------------------------------- the context's rule

@contextlib.contextmanager
def rule(eng, r):
    eng.set_rule(r)
    try:
        yield
    finally:
        eng.set_rule(0)


def test_zip215_rule(engine):
    """A golden vector of small order (key and R; S = 0) as validator 3's key and commit signature:
    ZIP-215 accepts it for every message, the Go rule refuses it."""
    with open(os.path.join(ROOT, "tests", "golden", "zip215_vectors.json")) as f:
        vectors = [v for v in json.load(f)["vectors"] if v["class"] == "zip_small_both" and v["valid_zip215"] and not v["valid_go"]]
    blk = st = None
    for v in vectors:
        pub, sig = bytes.fromhex(v["pub"]), bytes.fromhex(v["sig"])
        w = VC.make_world(4, 2, tag="zipw", pub_override={3: pub}, sig_override={3: sig})
        blk, st = w.blocks[1], w.states[1]
        msg = VC.oracle_commit(blk.last_commit).vote_sign_bytes(w.chain_id, 3)
        if ZR.verify_zip(pub, msg, sig) and not ZR.verify_go(pub, msg, sig):
            break
    else:
        pytest.fail("no vector diverges on this vote")
    go = VC.Case("go", replace(blk, verify_fn=ZR.verify_go), st)
    zp = VC.Case("zip", replace(blk, verify_fn=ZR.verify_zip), st)
    pb = check(engine, [go])
    assert pb.res[0].code == S.VB_LAST_COMMIT and pb.res[0].commit.code == 4 and pb.res[0].commit.idx == 3
    with rule(engine, 1):
        pb = check(engine, [zp])
        assert pb.res[0].code == S.VB_OK
    assert check(engine, [go]).res[0].code == S.VB_LAST_COMMIT


def test_python_entry_and_kernel_time(engine, world):
    stats = []
    errs = S.validate_blocks(engine, [c.request() for c in VC.window(world, 1, 3)], stats=stats)
    assert errs == [None, None, None] and stats == [(0, 4, 0)] * 3
    assert S.validate_kernel_ms(engine) > 0.0
    errs = S.validate_blocks(engine, [(VC.with_header(world.blocks[2], chain_id="x"), world.states[2])])
    assert str(errs[0]) == "wrong Block.Header.ChainID. Expected %s, got x" % VC.CHAIN
