"""The half-size kernels on the device at a chosen k (tmed_test_verify_k, tests/hs_k_cases.py).

k = H(R || A || M) mod L is a hash, so real signatures reach the kernels that consume sc_halfsize's
result only where random k lead: tight window counts 30..34, never the (k, 1) fallback (W = 64), a
wave of W = 29, a top digit 16 on both scalars, a chosen e = d S mod L.  The test-only entry runs a
context's ordinary generic route — the latency kernels or verify_prep / prep_r / main_hs<26|16> (or
variant 5's verify_main_kernel), the same chunk loop — with signature i's k taken from the caller, so:

* identity: with k = hram(R, A, b"") it returns byte for byte what verify_arrays returns, on every
  context (this pins the hook and both hand-off layouts);
* the whole shuffled corpus, cofactorless and (throughput contexts) ZIP-215, equals the Python bits;
* a wave holding one W = 64 lane at n = 1, 63, 64, 65, 257 (the other lanes run up to 35 windows
  above their own top window): decisions equal the Python bits, and tmed_window_stats shows one lane
  and one wave at 64;
* a wave of 64 lanes all of tight W = 29 runs 29 windows, and the same lanes beside a W = 34 lane
  decide the same;
* the latency kernels on groups of eight with one fallback signature each.

The largest tight W the builder reaches is 36 (family b's even-cofactor pairs); all comparisons are
exact bits.  The expected bits come from hs_k_cases.expect_go / expect_zip215 alone."""
import hashlib

import numpy as np
import pytest

import hs_k_cases as HK
from conftest import engine_with_env
from oracle import ed25519_go as E
from tmed._native import TMED_EINVAL, TmedError
from tmed.workload import c5_mix

pytestmark = pytest.mark.gpu

L = E.L
CONTEXTS = ("latency", "throughput", "b16", "v5", "chunks")
THROUGHPUT = ("throughput", "b16", "v5", "chunks")
HS_STATS = ("throughput", "b16")  # one chunk a call and a half-size hand-off: tmed_window_stats sees the whole batch
CHUNK = 256


@pytest.fixture(scope="module")
def ctxs(generic_engines):
    """The two contexts of generic_engines, and the throughput kernels on the radix-2^16 B windows,
    as main variant 5 (full-length recoding of the same k) and with a slab of 256 slots, so that
    the corpus spans several chunks and the override is read at base + slot."""
    own = {"b16": engine_with_env(TMED_GLAT_MAX=0, TMED_B26=0),
           "v5": engine_with_env(TMED_GLAT_MAX=0, TMED_MAIN_WAVES=5),
           "chunks": engine_with_env(TMED_GLAT_MAX=0, TMED_SLAB_SLOTS=CHUNK)}
    assert own["b16"].b_window_bits() == 16 and generic_engines["throughput"].b_window_bits() == 26
    yield dict(generic_engines, **own)
    for e in own.values():
        e.close()


@pytest.fixture(scope="module")
def corpus(hostsim):
    """The corpus, shuffled once: (cases, pubs, sigs, ks, go, zip)."""
    cases = HK.corpus(hostsim)["cases"]
    order = np.random.default_rng(0x45C).permutation(len(cases))
    cases = [cases[i] for i in order]
    assert len(cases) > 4 * CHUNK
    return (cases,) + HK.arrays(cases)


def _same(out, exp, cases, what):
    bad = np.nonzero(out != exp)[0]
    assert bad.size == 0, (what, [cases[i]["tag"] for i in bad[:12]])


# ------------------------------------------------------------------ identity
@pytest.fixture(scope="module")
def real_pool(generic_engines, golden):
    """(pubs, sigs, ks) over the empty message: 600 signatures signed over it with c5_mix at 1 % (one
    tuple of every C5 class), then the golden vectors' keys and signatures (valid only where their
    message is empty); k = hram(R, A, b"")."""
    eng = generic_engines["throughput"]
    n = 600
    seeds = np.random.default_rng(0x1D).integers(0, 256, (n, 32), dtype=np.uint8)
    sigs, pubs = eng.sign_arrays(seeds, np.zeros(16, np.uint8), np.zeros(n + 1, np.uint32))
    assert len(c5_mix(pubs, sigs, frac=0.01)) == 6
    gv = [v for v in golden if len(v["sig"]) == 128 and len(v["pub"]) == 64]
    pubs = np.concatenate([pubs, np.frombuffer(b"".join(bytes.fromhex(v["pub"]) for v in gv), np.uint8).reshape(-1, 32)])
    sigs = np.concatenate([sigs, np.frombuffer(b"".join(bytes.fromhex(v["sig"]) for v in gv), np.uint8).reshape(-1, 64)])
    ks = np.zeros((pubs.shape[0], 32), np.uint8)
    for i in range(pubs.shape[0]):
        h = hashlib.sha512(sigs[i, :32].tobytes() + pubs[i].tobytes()).digest()
        ks[i] = np.frombuffer((int.from_bytes(h, "little") % L).to_bytes(32, "little"), np.uint8)
    return pubs, sigs, ks


@pytest.mark.parametrize("ctx", CONTEXTS)
def test_the_hash_as_chosen_k_equals_verify_arrays(ctxs, real_pool, ctx):
    eng = ctxs[ctx]
    pubs, sigs, ks = real_pool
    n = pubs.shape[0]
    assert n > 4 * CHUNK
    ref = eng.verify_arrays(pubs, sigs, np.zeros(16, np.uint8), np.zeros(n + 1, np.uint32))
    assert 590 <= int(ref[:600].sum()) <= 595 and 0 < int(ref.sum()) < n
    got = eng.test_verify_k(pubs, sigs, ks)
    assert got.tobytes() == ref.tobytes(), np.nonzero(got != ref)[0][:10].tolist()
    for m in (1, 7, 65):  # a lone signature, a partial group of the latency kernels, a partial second wave
        assert eng.test_verify_k(pubs[:m], sigs[:m], ks[:m]).tobytes() == ref[:m].tobytes(), m


def test_a_k_not_below_L_is_refused(ctxs, real_pool):
    pubs, sigs, ks = real_pool
    for eng in (ctxs["latency"], ctxs["throughput"]):
        for bad in (L, L + 1, 2**256 - 1):
            k3 = ks[:3].copy()
            k3[1] = np.frombuffer(bad.to_bytes(32, "little"), np.uint8)
            with pytest.raises(TmedError) as ei:
                eng.test_verify_k(pubs[:3], sigs[:3], k3)
            assert ei.value.code == TMED_EINVAL
        k3[1] = np.frombuffer((L - 1).to_bytes(32, "little"), np.uint8)
        eng.test_verify_k(pubs[:3], sigs[:3], k3)


# ------------------------------------------------------------------ the corpus
@pytest.mark.parametrize("ctx", CONTEXTS)
def test_corpus_cofactorless(ctxs, corpus, ctx):
    """Every case in one call (main variant 5 among the contexts: the same k on the full-length
    recoding agrees with the others)."""
    cases, pubs, sigs, ks, go, zp = corpus
    _same(ctxs[ctx].test_verify_k(pubs, sigs, ks), go, cases, ctx)


@pytest.mark.parametrize("ctx", THROUGHPUT)
def test_corpus_zip215(ctxs, corpus, ctx):
    cases, pubs, sigs, ks, go, zp = corpus
    _same(ctxs[ctx].test_verify_k(pubs, sigs, ks, zip215=True), zp, cases, ctx)


# ------------------------------------------------------------------ waves
def _certain_fallbacks(corpus):
    """Family a's cases whose k (above 2^128) has a first quotient floor(8L / k) >= 2^33 - 1: far above the 2^32 - 2
    limit, the (k, 1) fallback whatever an fp64 estimate rounds to.  Valid and defective ones."""
    cases = corpus[0]
    fb = [c for c in cases if c["family"] == "a" and c["k"] >> 128 and HK.N8 // c["k"] >= 2**33 - 1]
    assert len(fb) >= 8 and {c["go"] for c in fb} == {True, False}
    assert all(HK.model_halfsize(c["k"])[3] for c in fb)
    return fb


def _short_lanes(corpus):
    """Family b and c cases of tight W <= 33: valid and defective, none near the fallback."""
    cases = corpus[0]
    out = [c for c in cases if c["family"] in "bc" and HK.model_halfsize(c["k"])[2] <= 33]
    assert len(out) > 600 and {c["go"] for c in out} == {True, False}
    assert {HK.model_halfsize(c["k"])[2] for c in out[:256]} >= {30, 31, 32}
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("ctx", THROUGHPUT)
def test_a_fallback_lane_in_the_wave(ctxs, corpus, ctx, n):
    """One (k, 1) lane among n - 1 lanes of W <= 33, at lane 0, at the last lane and at the start of
    the (partial) last wave: every decision equals the Python bits, and the hand-off holds exactly one
    lane and one wave of 64 windows."""
    eng = ctxs[ctx]
    fb, lanes = _certain_fallbacks(corpus), _short_lanes(corpus)
    for j, at in enumerate(sorted({0, n - 1, (n - 1) // 64 * 64})):
        cs = lanes[17 * j:17 * j + n - 1]
        cs.insert(at, fb[(j + n) % len(fb)])
        pubs, sigs, ks, go, zp = HK.arrays(cs)
        _same(eng.test_verify_k(pubs, sigs, ks), go, cs, (ctx, n, at))
        if ctx in HS_STATS:
            lh, wh = eng.window_stats()
            assert int(lh.sum()) == n and int(wh.sum()) == (n + 63) // 64
            assert int(lh[64]) == 1 and int(wh[64]) == 1, (n, at, lh.tolist(), wh.tolist())
        _same(eng.test_verify_k(pubs, sigs, ks, zip215=True), zp, cs, (ctx, n, at, "zip215"))


@pytest.mark.parametrize("ctx", THROUGHPUT)
def test_a_wave_of_the_shortest_window_count(ctxs, corpus, hostsim, ctx):
    """64 lanes all of tight W = 29: the wave runs 29 windows; with a W = 34 lane added its lanes run
    five windows above their own and decide the same."""
    eng = ctxs[ctx]
    cs = HK.signatures_at_w(hostsim, 29, 64)
    assert {c["go"] for c in cs} == {True, False}
    pubs, sigs, ks, go, zp = HK.arrays(cs)
    out = eng.test_verify_k(pubs, sigs, ks)
    _same(out, go, cs, ctx)
    if ctx in HS_STATS:
        lh, wh = eng.window_stats()
        assert int(lh[29]) == 64 and int(wh[29]) == 1 and int(wh.sum()) == 1, (lh.tolist(), wh.tolist())
    w34 = next(c for c in corpus[0] if c["tag"].startswith("b:W_34/") and c["tag"].count("/") == 1)
    assert HK.model_halfsize(w34["k"])[2] == 34
    cs2 = cs + [w34]
    pubs, sigs, ks, go2, zp2 = HK.arrays(cs2)
    out2 = eng.test_verify_k(pubs, sigs, ks)
    _same(out2, go2, cs2, ctx)
    assert out2[:64].tobytes() == out.tobytes()
    if ctx in HS_STATS:
        lh, wh = eng.window_stats()
        assert int(lh[34]) == 1 and int(lh[29]) == 64 and int(wh[34]) == 1, (lh.tolist(), wh.tolist())


@pytest.mark.parametrize("n", [1, 7, 8, 9, 16, 65])
def test_latency_groups_with_one_fallback_each(ctxs, corpus, n):
    """verify_glat_main_kernel runs a wave's eight signatures over the wave's largest W: every group
    of eight holds one (k, 1) signature (at place g mod 8 of group g) and seven of W <= 33."""
    fb, lanes = _certain_fallbacks(corpus), _short_lanes(corpus)
    cs = [fb[(i // 8) % len(fb)] if i % 8 == (i // 8) % 8 else lanes[3 * n + i] for i in range(n)]
    pubs, sigs, ks, go, zp = HK.arrays(cs)
    _same(ctxs["latency"].test_verify_k(pubs, sigs, ks), go, cs, n)
