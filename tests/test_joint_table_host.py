"""The joint radix-4 table of the half-size throughput path on the host (CPU) build of the kernel
source (tests/native/joint_host.cpp, test-only): the digit split (verify_hs.h hs_split4), the row
index (verify_core.h joint_index), the twelve rows of build_table_joint against the two-table
form's point code and against oracle.ed25519_go, and the joint Straus sum (hs_straus_joint)
against the two-table sum it replaced in the kernels (build_table_affine + hs_straus), compared
as encodings."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import ed25519_go as E

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
ROWS = 12
PAIRS = [(i, j) for i in range(-2, 3) for j in range(-2, 3)]


@pytest.fixture(scope="module")
def jh():
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "joint_host.mk"])
    return ctypes.CDLL(os.path.join(NATIVE, "libjointhost.so"))


def _split(jh, D):
    h, l = ctypes.c_int(0), ctypes.c_int(0)
    jh.jointhost_split4(D, ctypes.byref(h), ctypes.byref(l))
    return h.value, l.value


def test_digit_split(jh):
    """D = 4h + l with l in [-2, 1]: h in [-2, 2] for a regular window's digit, in [0, 4] for the
    top window's, which is then two rows (min(h, 2) and the rest, each at most 2)."""
    for D in range(-8, 9):
        h, l = _split(jh, D)
        assert 4 * h + l == D and -2 <= l <= 1 and -2 <= h <= 2, (D, h, l)
    for D in range(0, 17):
        h, l = _split(jh, D)
        assert 4 * h + l == D and -2 <= l <= 1 and 0 <= h <= 4, (D, h, l)
        h1 = min(h, 2)
        assert 0 <= h - h1 <= 2


def test_row_index(jh):
    """The 24 non-zero pairs map onto exactly 12 rows, (i, j) and (-i, -j) onto the same row with
    opposite signs; the stored (positive) pair has i > 0, or i = 0 and j > 0; (0, 0) is row 0."""
    assert jh.jointhost_index(0, 0) == 0
    rows = {}
    for i, j in PAIRS:
        if (i, j) == (0, 0):
            continue
        idx = jh.jointhost_index(i, j)
        assert 1 <= abs(idx) <= ROWS, (i, j, idx)
        assert (idx < 0) == (i < 0 or (i == 0 and j < 0)), (i, j, idx)
        assert jh.jointhost_index(-i, -j) == -idx
        rows.setdefault(abs(idx), set()).add((i, j) if idx > 0 else (-i, -j))
    assert sorted(rows) == list(range(1, ROWS + 1))
    assert all(len(v) == 1 for v in rows.values())
    order = [next(iter(rows[r])) for r in range(1, ROWS + 1)]
    assert order == [(0, 1), (0, 2), (1, -2), (1, -1), (1, 0), (1, 1), (1, 2), (2, -2), (2, -1), (2, 0), (2, 1), (2, 2)]


def _rand_point(rng):
    return E.pt_mul(rng.randrange(1, E.L), E.BASE)


def _order8():
    for p in E.small_order_points():
        if not E.pt_equal(E.pt_mul(4, p), E.IDENTITY):
            return p
    raise AssertionError("no point of order 8")


def _table_cases():
    rng = random.Random(0x7ab1e)
    t8 = _order8()
    a, r = _rand_point(rng), _rand_point(rng)
    cases = [("random", _rand_point(rng), _rand_point(rng)) for _ in range(6)]
    cases += [
        ("A = R", a, a),
        ("A = -R", a, E.pt_neg(a)),
        ("A of order 8", t8, r),
        ("A with a torsion part", E.pt_add(a, t8), r),
        ("R the identity", a, E.IDENTITY),
        ("R of order 8", a, t8),
        ("A = R of order 8", t8, t8),
        ("both the identity", E.IDENTITY, E.IDENTITY),
    ]
    return cases


def test_table_rows(jh):
    """Every row equals i (-A) + j (-+R): by the two-table form's point code, and by the oracle's."""
    for name, A, R in _table_cases():
        for dneg in (0, 1):
            got = ctypes.create_string_buffer(32 * (ROWS + 1))
            exp = ctypes.create_string_buffer(32 * (ROWS + 1))
            jh.jointhost_rows_enc(E.encode(A), E.encode(R), dneg, got, exp)
            assert got.raw == exp.raw, (name, dneg)
            Pn = E.pt_neg(A)
            Q = R if dneg else E.pt_neg(R)
            mul = lambda k, p: E.pt_mul(k, p) if k >= 0 else E.pt_neg(E.pt_mul(-k, p))
            for i in range(0, 3):
                for j in range(-2, 3):
                    idx = jh.jointhost_index(i, j)
                    if idx < 0:
                        continue
                    want = E.encode(E.pt_add(mul(i, Pn), mul(j, Q)))
                    assert got.raw[32 * idx:32 * idx + 32] == want, (name, dneg, i, j)


def _digits_value(digs):
    """sum digs[n] 16^n."""
    return sum(d << (4 * n) for n, d in enumerate(digs))


def _straus(jh, c, d, e, W, A, R, dneg, b16=0):
    ej, et = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    jh.jointhost_straus(c.to_bytes(32, "little"), d.to_bytes(32, "little"), e.to_bytes(32, "little"), W,
                        E.encode(A), E.encode(R), dneg, b16, ej, et)
    return ej.raw, et.raw


def _oracle_sum(c, d, e, A, R, dneg):
    Q = R if dneg else E.pt_neg(R)
    return E.encode(E.pt_add(E.pt_mul(e, E.BASE), E.pt_add(E.pt_mul(c, E.pt_neg(A)), E.pt_mul(d, Q))))


def test_joint_straus_random(jh):
    """Random (c, d, e) at W in {29, 32, 33, 64}, both B radices and both signs of d: the joint sum
    equals the two-table sum; a share of the cases also against the oracle's scalar products."""
    rng = random.Random(0x57a05)
    n = 0
    for W in (29, 32, 33, 64):
        for k in range(60):
            A, R = (_rand_point(rng), _rand_point(rng)) if k % 10 == 0 or n == 0 else (A, R)
            bits = 4 * W if W < 64 else 252
            # c and |d| below 2^(4W): the top digit reaches 16 when the top nibble is 15 with a carry
            c = rng.randrange(1 << bits)
            d = rng.randrange(1 << min(bits, 150)) | 1
            if k % 7 == 0:
                c |= 0xF8 << (4 * W - 8) if W < 64 else 0
            e = rng.randrange(E.L)
            dneg, b16 = k & 1, (k >> 1) & 1
            ej, et = _straus(jh, c, d, e, W, A, R, dneg, b16)
            assert ej == et, (W, k, hex(c), hex(d), hex(e))
            if k % 6 == 0:
                assert ej == _oracle_sum(c, d, e, A, R, dneg), (W, k)
            n += 1


def test_joint_straus_every_regular_digit_pair(jh):
    """Every pair of recoded digits (-8..7 each: a nibble minus 8) in one regular window, at window
    6 — where a radix-2^26 B step falls between the two sub-steps — and at window 20."""
    rng = random.Random(0xd161)
    A, R = _rand_point(rng), _rand_point(rng)
    W = 32
    for n0 in (6, 20):
        base_c = [rng.randrange(-8, 8) for _ in range(W - 1)] + [rng.randrange(1, 8)]
        base_d = [rng.randrange(-8, 8) for _ in range(W - 1)] + [rng.randrange(1, 8)]
        e = rng.randrange(E.L)
        for dc in range(-8, 8):
            for dd in range(-8, 8):
                cd, ddg = list(base_c), list(base_d)
                cd[n0], ddg[n0] = dc, dd
                c, d = _digits_value(cd), _digits_value(ddg)
                ej, et = _straus(jh, c, d, e, W, A, R, (dc + dd) & 1, 1 if n0 == 20 and dc == 0 else 0)
                assert ej == et, (n0, dc, dd)
                if dc == dd:
                    assert ej == _oracle_sum(c, d, e, A, R, (dc + dd) & 1), (n0, dc, dd)


def test_joint_straus_every_top_digit_pair(jh):
    """Every pair of top digits in [0, 16]^2 (16: the top nibble 15 with the carry of a negative
    digit below it), at W = 32 and W = 33 (the top window the first / the last of its word)."""
    rng = random.Random(0x70b)
    A, R = _rand_point(rng), _rand_point(rng)
    for W in (32, 33):
        e = rng.randrange(E.L)
        low_c = [rng.randrange(-8, 8) for _ in range(W - 2)]
        low_d = [rng.randrange(-8, 8) for _ in range(W - 2)]
        for tc in range(0, 17):
            for td in range(0, 17):
                # a top digit of 16 needs the digit below it negative (the scalar stays below 16^W),
                # one of 0 a positive one (the scalar stays positive); any other takes either sign
                nc = rng.randrange(-8, 0) if tc == 16 else rng.randrange(1, 8) if tc == 0 else rng.randrange(-8, 8)
                nd = rng.randrange(-8, 0) if td == 16 else rng.randrange(1, 8) if td == 0 else rng.randrange(-8, 8)
                c = _digits_value(low_c + [nc, tc])
                d = _digits_value(low_d + [nd, td])
                assert 0 < c < 1 << (4 * W) and 0 < d < 1 << (4 * W)
                ej, et = _straus(jh, c, d, e, W, A, R, td & 1)
                assert ej == et, (W, tc, td)
                if tc == td or tc == 16 or td == 16:
                    assert ej == _oracle_sum(c, d, e, A, R, td & 1), (W, tc, td)


def test_joint_straus_degenerate_points(jh):
    """The sums over the table cases' points (A = +-R, small orders, the identity)."""
    rng = random.Random(0xde9)
    for name, A, R in _table_cases()[5:]:
        for W in (29, 33):
            c, d, e = rng.randrange(1 << (4 * W)), rng.randrange(1 << (4 * W)) | 1, rng.randrange(E.L)
            ej, et = _straus(jh, c, d, e, W, A, R, W & 1)
            assert ej == et == _oracle_sum(c, d, e, A, R, W & 1), (name, W)
