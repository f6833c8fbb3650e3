"""CPU: the chosen-k cases (tests/hs_k_cases.py) through the host build of the half-size path
(hostsim_verify_hs_k, the host twin of tmed_test_verify_k): the case builder, its coverage and its
expected bits are checked here before anything reaches a device (tests/test_gpu_hs_k.py).

The largest tight window count the builder reaches is 36 (hs_k_cases.LARGEST_W, from the
even-cofactor adjustment); the (k, 1) fallback gives 64.  Unreachable and listed by name in the
builder: a regular digit of +8 (digits are nibble - 8 <= 7), the eight window-0 low pairs with an
even part of d (d is odd), and of e's radix-2^26 digits window 4 of either half (24 bits) and
"max" / "wrap" at window 0 (no bit below)."""
import ctypes

import numpy as np
import pytest

import hs_k_cases as HK
import prim_cases as PC
import scalar_edge_cases as SC
from oracle import ed25519_go as E

L = E.L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_host(hostsim, pubs, sigs, ks, b16, cofactor8, wmin=None):
    n = pubs.shape[0]
    out, wins = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    wm = None if wmin is None else np.full(n, wmin, np.int32)
    hostsim.hostsim_verify_hs_k(_p(pubs), _p(sigs), _p(ks), ctypes.c_size_t(n), _p(out), _p(wins),
                                None if wm is None else _p(wm), int(b16), int(cofactor8))
    return out, wins


@pytest.fixture(scope="module")
def corpus(hostsim):
    return HK.corpus(hostsim)


def test_the_model_of_the_lattice_step_equals_the_host_build(hostsim):
    """(c, d, tight W) of the header comment's model on every k of the chosen-k families and 500
    random ones; the fallback set is not empty and not everything."""
    ks = list(PC.halfsize_quotient_ks()) + list(PC.halfsize_long_euclid_ks()) + list(PC.halfsize_lattice_ks()[0][:514])
    for k in ks:
        c, d, w, fb = HK.model_halfsize(k)
        assert (c, d, w) == HK.host_halfsize(hostsim, k), k
        assert fb == (w == 64)
        if not fb:
            assert (c - d * k) % HK.N8 == 0 and d % 2 == 1
    assert 0 < len(HK.fallback_ks()) < len(PC.halfsize_quotient_ks())


def test_corpus_shape_and_coverage(corpus):
    """The builder's own assertions hold (corpus() raised otherwise); the corpus has every family,
    every kind of reject, both expected bits under both rules, and stays near 1,500 tuples."""
    cases = corpus["cases"]
    assert 1000 <= len(cases) <= 1600, len(cases)
    assert {c["family"] for c in cases} == {"a", "b", "c"}
    for kind in ("/R+T2", "/R+T4", "/R+T8", "/S+1", "/Rflip", "/k+1", "/k-1"):
        assert sum(kind in c["tag"] for c in cases) >= 30, kind
    for key in ("/A0", "/A0+T2", "/A0+T4", "/A0+T8", "/Aid"):
        assert sum(key in c["tag"] for c in cases) >= 100, key
    assert all(c["k"] < L for c in cases)
    go = np.array([c["go"] for c in cases])
    zp = np.array([c["zip"] for c in cases])
    assert (zp | ~go).all()  # ZIP-215 accepts whatever the cofactorless rule does
    assert go.sum() > 300 and (zp & ~go).sum() > 300 and (~zp).sum() > 100
    want, unreachable = HK.named_targets()
    assert len(want) == 6 + 3 + 16 + 4 + 4 + (25 + 16) * 2 + 25 + 8 and len(unreachable) == 2 + 8
    e_want, e_unreachable = HK.e_targets()
    assert len(e_want) == 2 * (4 * 3 - 2) and len(e_unreachable) == 2 * (3 + 2)
    assert max(w for *_, w in corpus["pairs"]) == HK.LARGEST_W == 36
    assert {w for *_, w in corpus["pairs"]} >= set(range(29, 37))
    # a small-order defect on an even-cofactor-adjusted d (W > 32 comes from the adjustment alone)
    assert any(t[0] == "W" and w > 32 for t, *_, w in corpus["pairs"])
    assert sum("b:W_3" in c["tag"] and "/R+T" in c["tag"] and not c["go"] for c in cases) >= 4


def test_expected_bits_restate_the_oracle_on_real_signatures(golden):
    """expect_go / expect_zip215 at k = hram(R, A, M) equal oracle.ed25519_go.verify and
    oracle.zip215.verify on golden vectors of every verdict."""
    from oracle import zip215
    gv = [v for v in golden if len(v["sig"]) == 128 and len(v["pub"]) == 64][::9]
    assert len(gv) > 50 and {v["valid"] for v in gv} == {True, False}
    for v in gv:
        pub, sig, msg = bytes.fromhex(v["pub"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])
        k = E.hram(sig[:32], pub, msg)
        assert HK.expect_go(pub, sig, k) == E.verify(pub, msg, sig) == v["valid"]
        assert HK.expect_zip215(pub, sig, k) == zip215.verify(pub, msg, sig)


@pytest.mark.parametrize("cofactor8", [0, 1])
@pytest.mark.parametrize("b16", [0, 1])
def test_corpus_through_the_host_build(hostsim, corpus, b16, cofactor8):
    """Every case, radix 26 and radix 16, cofactorless and cofactored: each lane over its own W and
    over 64 windows (the wave of a fallback lane) decides as the Python bits; the window count is 64
    exactly on the k the model sends to (k, 1)."""
    cases = corpus["cases"]
    pubs, sigs, ks, go, zp = HK.arrays(cases)
    exp = zp if cofactor8 else go
    fb = np.array([HK.model_halfsize(c["k"])[3] for c in cases])
    assert 20 < fb.sum() < len(cases) // 4
    for wmin in (None, 64):
        out, wins = run_host(hostsim, pubs, sigs, ks, b16, cofactor8, wmin)
        bad = np.nonzero(out != exp)[0]
        assert bad.size == 0, (wmin, [cases[i]["tag"] for i in bad[:10]])
        assert ((wins == 64) == fb).all(), [cases[i]["tag"] for i in np.nonzero((wins == 64) != fb)[0][:10]]
        assert wins.min() == 29 and sorted(set(wins[~fb].tolist()))[-1] == HK.LARGEST_W


def test_family_c_reaches_the_chosen_e(hostsim, corpus):
    """e = d S mod L of family c is the chosen e (recomputed from the host build's d), and its
    radix-2^26 digits from the host build equal the model's."""
    by_tag = {c["tag"].split("/")[0]: c for c in corpus["cases"] if c["family"] == "c" and c["go"]}
    seen = 0
    for tag, e, k in corpus["e"]:
        for sgn in "+-":
            c = by_tag.get("c:%s_d%s" % (tag, sgn))
            if c is None or c["k"] != k:
                continue
            _, d, _ = HK.host_halfsize(hostsim, k)
            assert (d < 0) == (sgn == "-")
            s = int.from_bytes(c["sig"][32:], "little")
            assert d * s % L == e, tag
            dl, dh = np.zeros(5, np.int32), np.zeros(5, np.int32)
            hostsim.hostsim_b26_digits(e.to_bytes(32, "little"), _p(dl), _p(dh))
            assert (dl.tolist(), dh.tolist()) == SC.digits_e26(e), tag
            seen += 1
    assert seen == len(corpus["e"])
