"""CPU: the scalar-digit edge cases (tests/scalar_edge_cases.py) against their own models, the
oracle and the host build of the kernel code.

The models reconstruct their scalars; every (radix, window, edge digit) a scalar below L can reach is
hit by some case (the unreachable ones derived here from L, not taken from the case builder); the
expected bits agree with the oracle's C port under both rules; the host build of every verify path
decides each case as the oracle does; hs_b26_digit, whose input e = d S mod L no signature chooses,
is driven at chosen e (as a digit function here; through the B additions of the half-size sum, with
k chosen beside the signature, in tests/test_hs_k_host.py and tests/test_gpu_hs_k.py)."""
import ctypes

import numpy as np
import pytest

import scalar_edge_cases as SC
from oracle import ed25519_go as E
from oracle import port

L = E.L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _s_of(c):
    return int.from_bytes(c["sig"][32:], "little")


def _k_of(c):
    return E.hram(c["sig"][:32], c["pub"], c["msg"])


def test_digit_models_reconstruct_their_scalars():
    for c in SC.cases():
        s, k = _s_of(c), _k_of(c)
        for r in (8, 16):
            ds = SC.digits_biased(s, r)
            assert all(-(1 << (r - 1)) <= d < 1 << (r - 1) for d in ds)
            assert sum(d << (r * m) for m, d in enumerate(ds)) == s, (c["tag"], r)
        ds = SC.digits_s24(s)
        assert len(ds) == 11 and all(abs(d) <= 1 << 23 for d in ds)
        assert sum(d << (24 * m) for m, d in enumerate(ds)) == s, c["tag"]
        if s < L:
            assert 0 <= ds[10] <= 4097  # inside what b24_fill_kernel fills of window 10
        ds = SC.digits_k12(k)
        assert len(ds) == 21 and all(abs(d) <= 2048 for d in ds[:-1]) and 0 <= ds[-1] <= 4097
        assert sum(d << (12 * m) for m, d in enumerate(ds)) == k, c["tag"]
    for tag, e in SC.e26_scalars():
        lo, hi = SC.digits_e26(e)
        assert all(abs(d) <= 1 << 25 for d in lo + hi)
        assert sum(d << (26 * m) for m, d in enumerate(lo)) + (sum(d << (26 * m) for m, d in enumerate(hi)) << 128) == e, tag


def _least_scalar(radix, m, target, biased):
    """The least scalar whose window m sits at the target, or None when the target needs a carry or
    a below bit at window 0.  Every other bit may be 0, so the target is reachable below a bound
    exactly when this scalar is below it."""
    half, mask = 1 << (radix - 1), (1 << radix) - 1
    if target == "min":  # field 2^(r-1), nothing coming in
        return half << (radix * m)
    if target == "max" and biased:  # field 2^(r-1) - 1, nothing coming in
        return (half - 1) << (radix * m)
    if m == 0:
        return None
    # a carry out of window m - 1 needs at least its top bit, the below bit is that bit
    field = mask if target == "wrap" else half - 1
    return (field << (radix * m)) | 1 << (radix * m - 1)


def _reachable(radix, windows, biased, bound):
    out = set()
    for m in range(windows):
        for t in SC.TARGETS:
            x = _least_scalar(radix, m, t, biased)
            if x is not None and x < bound:
                out.add((m, t))
    return out


def test_coverage_matrix_has_no_gap():
    """Every (radix, window, edge digit) some scalar below L reaches is hit: S in radix 2^8 and 2^16
    (biased) and 2^24 (carry-free), k in radix 2^12 (windows 0..19), e's halves in radix 2^26."""
    valid = [c for c in SC.cases() if c["valid"]]
    for r, windows, biased in ((8, 32, True), (16, 16, True), (24, 11, False)):
        want = _reachable(r, windows, biased, L)
        hit = set()
        for c in valid:
            hit |= SC.targets_hit(_s_of(c), r)
        assert want <= hit, (r, sorted(want - hit))
        assert hit <= want, (r, sorted(hit - want))  # the derivation and the models agree
        # what is left out is the top window alone, and a carry / below bit into window 0
        top = {(windows - 1, t) for t in SC.TARGETS}
        none_in = {(0, "wrap")} | (set() if biased else {(0, "max")})
        assert {(m, t) for m in range(windows) for t in SC.TARGETS} - want == top | none_in, r
    want = _reachable(12, 20, False, L)
    assert len(want) == 20 * 3 - 2
    pubs = sorted({c["pub"] for c in valid if c["tag"].startswith("k12_")})
    assert len(pubs) == 3
    for pub in pubs:
        hit = set()
        for c in valid:
            if c["pub"] == pub:
                hit |= SC.targets_hit(_k_of(c), 12)
        assert want <= hit, sorted(want - hit)
    want = {(h, m, t) for h in range(2) for (m, t) in _reachable(26, 5, False, 1 << 128)}
    assert len(want) == 2 * (4 * 3 - 2)  # window 4 holds bits 104..127 of a half: below every edge
    hit = set()
    for _, e in SC.e26_scalars():
        hit |= SC.targets_hit_e26(e)
    assert want == hit, sorted(want ^ hit)


def test_case_list_shape():
    cs = SC.cases()
    tags = [c["tag"] for c in cs]
    assert len(set(tags)) == len(tags)
    s_tags = [t for t, _ in SC.s_scalars()]
    for order in (1, 2, 4, 8):
        assert all("%s_ord%d" % (t, order) in tags for t in s_tags)
    assert [E.decode(pub) is not None and o for o, _, pub in SC.torsion_keys()] == [1, 2, 4, 8]
    for kind in ("Rflip", "S+1", "S+L"):
        rej = [c for c in cs if c["tag"].endswith(kind)]
        assert len(rej) > 50 and not any(c["valid"] for c in rej)
    pos = [c for c in cs if not c["tag"].endswith(("Rflip", "S+1", "S+L"))]
    assert all(c["valid"] for c in pos), [c["tag"] for c in pos if not c["valid"]][:5]


def test_expected_bits_equal_the_port_under_both_rules():
    pubs, sigs, msgs, offs, exp = SC.arrays()
    go = port.verify_batch(pubs, sigs, msgs, offs.astype(np.uint64), 8)
    assert (go == exp).all(), [SC.cases()[i]["tag"] for i in np.nonzero(go != exp)[0]][:10]
    # none of the rejects is one the cofactored rule forgives: the same bits
    zip215 = port.verify_batch(pubs, sigs, msgs, offs.astype(np.uint64), 8, zip215=True)
    assert (zip215 == exp).all(), [SC.cases()[i]["tag"] for i in np.nonzero(zip215 != exp)[0]][:10]


@pytest.mark.parametrize("path", [16, "b16", "hs", "hs16", "hostsim_verify_comb_batch",
                                  "hostsim_verify_comb_batch16", "hostsim_verify_comb_lat"])
def test_edge_cases_through_the_host_build(hostsim, path):
    """Every verify path of the host build: the generic radix-256 / radix-2^16 B windows, the half-size
    path on radix-2^26 and radix-2^16 tables, the key-cached combs (throughput and latency order)."""
    pubs, sigs, msgs, offs, exp = SC.arrays()
    n = len(exp)
    out = np.zeros(n, np.uint8)
    if isinstance(path, str) and path.startswith("hostsim_"):
        karr, idx = SC.keyed(pubs)
        getattr(hostsim, path)(_p(karr), ctypes.c_size_t(len(karr)), _p(idx), _p(sigs), _p(msgs), _p(offs),
                               ctypes.c_size_t(n), _p(out))
    elif path == "hs":
        hostsim.hostsim_verify_batch_hs(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out), None)
    elif path == "hs16":
        hostsim.hostsim_verify_batch_hs16(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out), None)
    elif path == "b16":
        hostsim.hostsim_verify_batch_b16(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out))
    else:
        hostsim.hostsim_verify_batch_g(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out),
                                       ctypes.c_int(path))
    assert (out == exp).all(), [SC.cases()[i]["tag"] for i in np.nonzero(out != exp)[0]][:10]


def test_b26_digits_at_chosen_e(hostsim):
    """hs_b26_digit (verify_hs.h) against the radix-2^26 model at every window's edges."""
    for tag, e in SC.e26_scalars():
        dl, dh = np.zeros(5, np.int32), np.zeros(5, np.int32)
        hostsim.hostsim_b26_digits(e.to_bytes(32, "little"), _p(dl), _p(dh))
        lo, hi = SC.digits_e26(e)
        assert (dl.tolist(), dh.tolist()) == (lo, hi), tag
