"""The checkers of tests/key_order_cases.py and tests/finish_cases.py on outputs made here: they pass
on a correct output (numpy's stable argsort of the bins; the expectation itself) and fail on each
doctored one.  This is what shows that tests/test_gpu_keyed_stages.py can fail; no defect is ever
seeded into a kernel."""
import numpy as np
import pytest

import finish_cases as FC
import key_order_cases as KO


def _order(n=12289, nkeys=10000, base=4096, seed=5):
    v = KO.uniform(n, nkeys, seed)
    v[::97] = nkeys  # some past the set
    perm, cursor = KO.reference_order(v, nkeys, base)
    return v, n, nkeys, base, perm, cursor


def test_bin_rule_on_the_grid():
    got = {(KO.nbins_of(k), KO.shift_of(k)) for k in KO.GRID_NKEYS}
    assert KO.GRID_NBINS <= {b for b, _ in got} and KO.GRID_SHIFTS == {s for _, s in got}
    assert (KO.nbins_of(4095), KO.shift_of(4095)) == (4096, 0) and (KO.nbins_of(8190), KO.shift_of(8190)) == (4096, 1)
    assert (KO.nbins_of(4096), KO.shift_of(4096)) == (2049, 1) and (KO.nbins_of(1 << 24), KO.shift_of(1 << 24)) == (2049, 13)
    assert (KO.nbins_of(1), KO.nbins_of(2)) == (2, 3)
    assert max(KO.nbins_of(k) for k in range(1, 70000)) == KO.BINS
    b = KO.bins_of(np.array([0, 3, 4, 9999, 10000, 0xFFFFFFFF], np.uint32), 10000)
    assert b.tolist() == [0, 0, 1, 2499, 2500, 2500]


@pytest.mark.parametrize("nkeys", [1, 2, 1024, 4095, 4096, 8190, 10000, 1 << 24])
def test_key_order_checker_passes_on_a_stable_sort(nkeys):
    for n in (1, 257, 4097, 12289):
        for base in KO.GRID_BASES:
            v = KO.uniform(n, nkeys, n + base)
            perm, cursor = KO.reference_order(v, nkeys, base)
            KO.check(v, n, nkeys, base, perm, cursor, KO.nbins_of(nkeys), KO.shift_of(nkeys))
    k = nkeys if nkeys > 2 else 4095
    for name, v in KO.distributions(k):
        perm, cursor = KO.reference_order(v, k, 7)
        KO.check(v, len(v), k, 7, perm, cursor, KO.nbins_of(k), KO.shift_of(k))


def test_key_order_checker_fails_on_doctored_outputs():
    v, n, nkeys, base, perm, cursor = _order()
    nb, sh = KO.nbins_of(nkeys), KO.shift_of(nkeys)
    KO.check(v, n, nkeys, base, perm, cursor, nb, sh)
    bins = KO.bins_of(v, nkeys)[perm.astype(np.int64) - base]
    edge = int(np.flatnonzero(np.diff(bins) > 0)[len(bins) // 3000])  # j, j + 1 lie either side of a bin edge

    def doctored(name):
        p, c, b, s = perm.copy(), cursor.copy(), nb, sh
        if name == "duplicate":
            p[100] = p[101]
        elif name == "sentinel":
            p[n - 1] = KO.SENTINEL
        elif name == "below base":
            p[0] = base - 1
        elif name == "swap across a bin edge":
            p[edge], p[edge + 1] = p[edge + 1], p[edge]
        elif name == "cursor off by one":
            c[nb // 2] += 1
        elif name == "last cursor short":
            c[nb - 1] -= 1
        elif name == "wrong shift":
            s += 1
        elif name == "wrong bin count":
            b -= 1
            c = c[:-1]
        return p, c, b, s

    for name in ("duplicate", "sentinel", "below base", "swap across a bin edge", "cursor off by one",
                 "last cursor short", "wrong shift", "wrong bin count"):
        with pytest.raises(AssertionError):
            KO.check(v, n, nkeys, base, *doctored(name))
    # a swap inside one bin is no defect: the order inside a bin is free
    inside = int(np.flatnonzero(np.diff(bins) == 0)[0])
    p = perm.copy()
    p[inside], p[inside + 1] = p[inside + 1], p[inside]
    KO.check(v, n, nkeys, base, p, cursor, nb, sh)


def test_finish_groups_rule():
    exp = {1: (1, 1), 255: (1, 255), 256: (1, 256), 257: (1, 257), 65535: (1, 65535), 65536: (1, 65536),
           65537: (2, 32769), 131072: (2, 65536), 131073: (3, 43691), (1 << 20) - 15: (16, 65536), 1 << 20: (16, 65536)}
    for m, gl in exp.items():
        assert FC.groups(m) == gl, m


def test_finish_checker_fails_on_a_flipped_bit():
    m, base = 4099, 64
    c = FC.case(m, 4099)
    assert len(c["planted"]) >= len(FC.KINDS) + len(FC.GUARDS) and 0 < c["exp"].sum() < m
    for perm in (None, FC.shuffled_perm(m, base, 3)):
        out = np.full(base + m, FC.UNTOUCHED, np.uint8)
        idx = np.arange(m) + base if perm is None else perm[base:base + m].astype(np.int64)
        out[idx] = c["exp"]
        FC.check(c, out, base, perm)
        for pos in list(c["planted"])[::3] + [1, m - 1]:
            bad = out.copy()
            bad[idx[pos]] ^= 1
            with pytest.raises(AssertionError):
                FC.check(c, bad, base, perm)
        stray = out.copy()
        stray[np.setdiff1d(np.arange(base + m), idx)[0]] = 1  # a decision written where no position lands
        with pytest.raises(AssertionError):
            FC.check(c, stray, base, perm)


def test_finish_guard_checker_fails_on_a_poisoned_neighbour():
    m = 4099
    c = FC.case(m, 4099)
    out = c["exp"].copy()
    FC.check_guards(c, out)
    name, lane, zero, near = c["guards"][0]
    bad = out.copy()
    bad[zero[0]] = 1
    with pytest.raises(AssertionError):
        FC.check_guards(c, bad)
    # at G = 1 a lane holds one slot; the host cases at G > 1 and the device's supply the neighbours
    c2 = dict(c, guards=[("first slot", 0, [0], [1])], exp=np.ones(m, np.uint8))
    FC.check_guards(c2, np.array([0, 1] + [1] * (m - 2), np.uint8))
    with pytest.raises(AssertionError):
        FC.check_guards(c2, np.array([0, 0] + [1] * (m - 2), np.uint8))
