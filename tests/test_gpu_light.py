"""light.Verify on the device: header_hash_kernel against oracle.merkle.header_hash at every edge of
the leaf encodings and of the launch shape, and tmed_light_verify (header hashes, set hashes and
signatures on the GPU) against the restatement in light_cases.py over the CPU suite's scenarios, a
small light-client workload, and beside a submitted blocksync window."""
import pytest

import header_cases as HC
import light_cases as LC
import tmed.light as L
import tmed.types as T
from commit_cases import oracle_result, pbid, same, to_product
from conftest import engine_with_env
from oracle import commit as C
from oracle import merkle as M
from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of
from test_merkle_oracle import KAT_HEADER_HASH

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- header_hash_kernel

def test_header_kernel_edges_gpu(engine):
    """The KAT, every zero-omission, chain-id lengths 0 / 1 / 50 / 51, AppHash lengths 0 .. 65, the
    LastBlockID leaf either side of 118 bytes, an empty ValidatorsHash (ok = 0): one call, eligible
    headers through the fused kernel and the others through the host-leaf route."""
    from tmed.merkle import header_hashes
    hs = HC.edge_headers()
    routes = {HC.fused_ok(h) for h in hs}
    assert routes == {True, False}
    got = header_hashes(engine, hs)
    assert got[0].hex().upper() == KAT_HEADER_HASH
    for i, (h, g) in enumerate(zip(hs, got)):
        assert g == M.header_hash(h), (i, HC.fused_ok(h), h)
    assert sum(g is None for g in got) >= 2
    # each of them alone too: group 0 of a launch whose other 15 groups have no header
    for h in hs[:30]:
        assert header_hashes(engine, [h]) == [M.header_hash(h)], h


def test_header_kernel_zeroes_the_hash_of_a_nil_header_gpu(engine):
    import ctypes
    import numpy as np
    from tmed.merkle import HeaderBatch, _bind, _p
    hs = [HC.with_(validators_hash=b""), HC.with_(), HC.with_(validators_hash=b"", app_hash=bytes(65))]
    b = HeaderBatch(hs)
    b.out[:] = 0xAA
    assert _bind().tmed_header_hashes(engine._h, b.hs, 3, _p(b.out), _p(b.ok)) == 0
    assert list(b.ok[:3]) == [0, 1, 0]
    assert not b.out[0].any() and not b.out[2].any() and bytes(b.out[1]) == M.header_hash(hs[1])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_header_kernel_batch_sizes_gpu(engine, n):
    """Group (16 lanes), wave (4 headers) and workgroup (16 headers) edges, eligible and ineligible
    headers mixed in one call."""
    from tmed.merkle import header_hashes
    hs = HC.batch(n)
    got = header_hashes(engine, hs)
    for i, (h, g) in enumerate(zip(hs, got)):
        assert g == M.header_hash(h), (n, i, HC.fused_ok(h))
    if n >= 63:
        assert {HC.fused_ok(h) for h in hs} == {True, False}


def test_header_kernel_only_eligible_batches_gpu(engine):
    """Nothing but eligible headers, at the same sizes: the whole call is one launch."""
    from tmed.merkle import header_hashes
    pool = [h for h in HC.edge_headers() if HC.fused_ok(h)]
    for n in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257):
        hs = [dict(pool[(7 * i + n) % len(pool)], data_hash=bytes([i % 256]) * 32) for i in range(n)]
        got = header_hashes(engine, hs)
        for i, (h, g) in enumerate(zip(hs, got)):
            assert g == M.header_hash(h), (n, i)


# ----------------------------------------------------------------------------- tmed_light_verify

@pytest.fixture(scope="module")
def cached_engine():
    """A context with the seam's key-set cache on (the shared test context has it off)."""
    e = engine_with_env(TMED_KEYCACHE=1)
    yield e
    e.close()


def _check(engine, cases, codes=None, flags=0, stats=None):
    sets = {}
    pl = L.PreparedLight([c.pair(sets) for c in cases])
    pl.run(engine, flags)
    got = pl.errors()
    for q, c in enumerate(cases):
        exp = c.expected()
        code = pl.res[q].code
        if codes is not None:
            assert code == codes[q], (c.name, code, codes[q])
        assert LC.same_outcome(got[q], exp, code), (c.name, got[q], exp)
        if stats is not None:
            stats.append((pl.res[q].verified_trusting, pl.res[q].verified_light))
    return pl


@pytest.mark.parametrize("flags", [0, L.LIGHT_ORDERED])
@pytest.mark.parametrize("cache", ["off", "on"])
def test_light_scenarios_gpu(engine, cached_engine, cache, flags):
    """The CPU suite's cases (the reference's tables, one case per outcome, the precedence pairs, the
    boundary times, headers outside the kernel's limits) through tmed_light_verify: equal to the
    restatement, with the key-set cache off and on (twice there: the second call finds every set
    cached), speculative and ordered."""
    e = engine if cache == "off" else cached_engine
    scen = LC.scenarios()
    cases = [c for c, _ in scen] + [c for c, _ in LC.tables()]
    codes = [code for _, code in scen] + [None] * len(LC.tables())
    for _ in range(2 if cache == "on" else 1):
        if cache == "on":
            e.keycache_wait()
        stats = []
        pl = _check(e, cases, None, flags, stats)
        for q, code in enumerate(codes):
            if code is None:
                continue
            assert pl.res[q].code == code, (cases[q].name, pl.res[q].code, code)
            if code not in (L.OK, L.TRUSTING, L.COMMIT):
                assert stats[q] == (0, 0), cases[q].name  # decided before the commit checks: no signatures
    for (case, pinned), q in zip(LC.tables(), range(len(scen), len(cases))):
        if isinstance(pinned, tuple):
            assert (pl.res[q].commit.got, pl.res[q].commit.needed) == pinned[1:], case.name


def test_light_ordered_sends_no_light_signatures_after_a_failed_trusting_gpu(engine):
    cases = [c for c, code in LC.scenarios() if code == L.TRUSTING]
    assert len(cases) >= 3
    spec, ordered = [], []
    _check(engine, cases, None, 0, spec)
    _check(engine, cases, None, L.LIGHT_ORDERED, ordered)
    assert all(vl == 0 for _, vl in ordered)
    assert [vt for vt, _ in spec] == [vt for vt, _ in ordered]


@pytest.mark.parametrize("cache", ["off", "on"])
def test_light_c3_shape_gpu(engine, cached_engine, cache):
    """12 heights x 25 validators, the set changing by one key per height; all pairs (h, h + k), k = 1
    (adjacent) and 2..4; a header changed after signing, a wrong set, a bad signature before and one
    past the crossing: outcomes and Got / Needed equal the restatement."""
    e = engine if cache == "off" else cached_engine
    cases = LC.c3_shape()
    assert len(cases) == 11 + 10 + 9 + 8
    for flags in (0, L.LIGHT_ORDERED):
        pl = _check(e, cases, None, flags)
    codes = set(pl.codes())
    assert {L.OK, L.COMMIT_HEADER_HASH, L.VALS_HASH} <= codes and (L.COMMIT in codes or L.TRUSTING in codes)
    late = [q for q, c in enumerate(cases) if c.untrusted.header["height"] == 11]
    assert late and all(pl.res[q].code == L.OK for q in late)  # the bad signature past the crossing is never reached


def test_light_beside_a_submitted_blocksync_window_gpu(engine):
    """A blocksync window is submitted, then tmed_light_verify runs (it collects the window first),
    then blocksync_wait: the results of both equal the oracle's."""
    chain = "light-bs"
    vs, seeds = make_valset([seed_of("lbs", i) for i in range(8)], [10] * 8)
    bids, heights, ocommits, pcommits = [], [], [], []
    for b in range(3):
        bid = make_block_id("lbs%d" % b)
        cm = make_commit(vs, seeds, chain, 10 + b, 0, bid)
        if b == 1:
            s = bytearray(cm.signatures[0].signature)
            s[7] ^= 4
            cm.signatures[0].signature = bytes(s)
        pv, pc = to_product(vs, cm)
        bids.append(bid)
        heights.append(10 + b)
        ocommits.append(cm)
        pcommits.append(pc)
    w = T.BlocksyncWindow(pv, chain, [pbid(b) for b in bids], heights, pcommits)
    cases = [c for c, _ in LC.scenarios()]
    w.submit(engine, 1)
    _check(engine, cases, [code for _, code in LC.scenarios()])
    T.blocksync_wait(engine)
    for b in range(3):
        assert same(w.errors()[b], oracle_result(1, vs, chain, bids[b], heights[b], ocommits[b], 0, 0)), b
    assert list(w.codes()) == [0, 4, 0]


def test_light_python_mirror_gpu(engine):
    """tmed.light.verify: the public Python entry point, reference-shaped errors."""
    cases = [c for c, _ in LC.tables()]
    got = L.verify(engine, [c.pair() for c in cases])
    for c, g in zip(cases, got):
        assert LC.same(g, c.expected()), (c.name, g)
    assert any(isinstance(g, L.ErrNewValSetCantBeTrusted) for g in got)
    assert any(isinstance(g, L.ErrOldHeaderExpired) for g in got)
    assert any(isinstance(g, L.ErrInvalidHeader) and isinstance(g.reason, T.ErrNotEnoughVotingPowerSigned) for g in got)
