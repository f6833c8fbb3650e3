"""Cases and expectations for the ZIP-215 finish of the key-cached routes (csrc/zip_finish.h
zip_finish_one, csrc/zip_finish.hip keyset_finish_zip_kernel / launch_finish_zip): from a fin slot's
projective P = (X : Y : Z), the 32 bytes of R and the bit already in `out`,

    bit && Z != 0 (mod p) && R decodes permissively && [8](P - R) == identity.

Shared by the host build's test (tests/test_zip_finish_host.py, tests/native/zip_finish_host.cpp) and
the device's (tests/test_gpu_zip_finish.py, tmed_test_finish_zip215).  No GPU here; deterministic,
cached, and callers must not modify what they get.

Every expectation comes from Python integers and oracle.ed25519_go (direct_expected): P = (X/Z, Y/Z)
is a curve point in every row but the Z = 0 ones, which the rule rejects before any arithmetic.  The
limb vectors are what the main kernels may leave (fe25519.h "carried"; tests/prim_cases.py CARRIED_LO /
CARRIED_HI, tests/group_cases.py fe_rep): X, Y, Z are representatives x Z + k p of the coordinates, and
the rows named "limbs at the ends" put Z and one of X, Y on the all-low / all-high vectors and solve
the curve equation for the other coordinate."""
import functools
import json
import os
import random

import numpy as np

import finish_cases as FC
import group_cases as GC
import prim_cases as PC
from oracle import ed25519_go as E

P, L, D = E.P, E.L, E.D
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNTOUCHED = 0xAA
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)  # the device test's m: around one wave and one block, then 17 blocks


def point_order(pt):
    """Order of a point whose order divides 8."""
    for k in (1, 2, 4, 8):
        if E.pt_equal(E.pt_mul(k, pt), E.IDENTITY):
            return k
    raise AssertionError("not a small-order point")


def affine(pt):
    x, y, z, _ = pt
    zi = pow(z, P - 2, P)
    return x * zi % P, y * zi % P


def direct_expected(xl, yl, zl, r, bit):
    """One row's expected bit from its limbs and bytes alone."""
    z = PC.limb_val(zl) % P
    if not bit or z == 0:
        return 0
    rp = E.decode(bytes(r))
    if rp is None:
        return 0
    zi = pow(z, P - 2, P)
    x, y = PC.limb_val(xl) * zi % P, PC.limb_val(yl) * zi % P
    p = (x, y, 1, x * y % P)
    assert E.pt_is_on_curve(p), "a row's P must be a curve point: the oracle's addition is only then the group law"
    return int(E.pt_equal(E.pt_mul(8, E.pt_add(p, E.pt_neg(rp))), E.IDENTITY))


def _proj(pt, zl, rng):
    """Limbs (X, Y, Z) of the affine point pt scaled by the value of the limb vector zl."""
    x, y = affine(pt)
    z = PC.limb_val(zl) % P
    return GC.fe_rep(x * z, rng), GC.fe_rep(y * z, rng), tuple(int(v) for v in zl)


def _zs(rng):
    """A Z limb vector: both all-extreme vectors now and then, otherwise a carried draw (30 % at the ends)."""
    while True:
        z = rng.choice([PC.CARRIED_LO, PC.CARRIED_HI, PC.draw_carried(rng), PC.draw_carried(rng)])
        if PC.limb_val(z) % P:
            return tuple(int(v) for v in z)


def _noncanonical(y, sign):
    """The encoding y + p with the sign bit as given (y < 19, so it fits 255 bits)."""
    assert y < 19
    return ((y + P) | (sign << 255)).to_bytes(32, "little")


def _solve_other(v, for_x):
    """The curve's other coordinate for x = v (for_x) or y = v, or None: -x^2 + y^2 = 1 + d x^2 y^2."""
    if for_x:
        num, den = (1 + v * v) % P, (1 - D * v * v) % P  # y^2
    else:
        num, den = (v * v - 1) % P, (D * v * v + 1) % P  # x^2
    w, ok = E._sqrt_ratio(num, den)
    return w if ok else None


def _extreme_rows(rng):
    """Curve points with Z and one of X, Y on the all-low / all-high limb vectors."""
    rows = []
    for zl in (PC.CARRIED_LO, PC.CARRIED_HI):
        for cl in (PC.CARRIED_LO, PC.CARRIED_HI):
            for for_x in (True, False):
                z = PC.limb_val(zl) % P
                v = PC.limb_val(cl) * pow(z, P - 2, P) % P
                w = _solve_other(v, for_x)
                if w is None:
                    continue
                wl = GC.fe_rep(w * z, rng)
                xl, yl = (cl, wl) if for_x else (wl, cl)
                x, y = (v, w) if for_x else (w, v)
                rows.append((tuple(xl), tuple(yl), tuple(zl), (x, y, 1, x * y % P)))
    assert len(rows) >= 2
    return rows


@functools.lru_cache(maxsize=None)
def golden_rows():
    """Every tuple of tests/golden/zip215_vectors.json (all have 32-byte keys) as a finish row: the bit
    is what the shared prep decides (A decodes, 64 bytes, S < L), P = [S]B + [k](-A) by the oracle, r
    the signature's first half.  The expected bit must equal the file's valid_zip215."""
    with open(os.path.join(ROOT, "tests", "golden", "zip215_vectors.json")) as f:
        vs = json.load(f)["vectors"]
    rng = random.Random(215)
    rows = []
    for v in vs:
        pub, msg, sig = bytes.fromhex(v["pub"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
        assert len(pub) == 32
        a = E.decode(pub)
        s = E.sc_canonical(sig[32:]) if len(sig) == 64 else None
        if a is None or s is None:
            pt, bit, r = E.BASE, 0, (sig + bytes(32))[:32]
        else:
            k = E.hram(sig[:32], pub, msg)
            pt, bit, r = E.pt_add(E.pt_mul(s, E.BASE), E.pt_mul(k, E.pt_neg(a))), 1, sig[:32]
        xl, yl, zl = _proj(pt, _zs(rng), rng)
        rows.append(("golden " + v["class"], xl, yl, zl, r, bit, int(v["valid_zip215"])))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def planted():
    """(name, X limbs, Y limbs, Z limbs, r, bit, expected): every planted row, expectation asserted
    against direct_expected."""
    rng = random.Random(8215)
    small = E.small_order_points()
    orders = [point_order(t) for t in small]
    assert sorted(orders) == [1, 2, 4, 4, 8, 8, 8, 8]
    rows = []

    def add(name, pt, r, want, bit=1, zl=None):
        xl, yl, zl = _proj(pt, zl or _zs(rng), rng)
        rows.append((name, xl, yl, zl, bytes(r), bit, want))

    base = [E.pt_mul(rng.randrange(1, L), E.BASE) for _ in range(6)]
    big = E.pt_mul(rng.randrange(1, L), E.BASE)
    for R in base[:3]:
        add("P = R, canonical encoding", R, E.encode(R), 1)
    # a finish that doubles fewer than three times rejects the orders 8 (and 4)
    for t, o in zip(small, orders):
        add("P = R + T, T of order %d" % o, E.pt_add(base[3], t), E.encode(base[3]), 1)
    for q in (big, E.pt_add(big, small[4]), E.pt_mul(2, E.BASE)):
        add("P = R + Q, Q of large order", E.pt_add(base[4], q), E.encode(base[4]), 0)
    add("P = -R", E.pt_neg(base[4]), E.encode(base[4]), 0)
    # non-canonical encodings that decode: y >= p, both sign bits
    n_noncanon = 0
    for y in range(19):
        for sign in (0, 1):
            r = _noncanonical(y, sign)
            R = E.decode(r)
            if R is None:
                continue
            n_noncanon += 1
            add("R with y >= p (y = %d, sign %d), P = R" % (y, sign), R, r, 1)
            add("R with y >= p (y = %d, sign %d), P = R + T8" % (y, sign), E.pt_add(R, small[5]), r, 1)
            add("R with y >= p (y = %d, sign %d), P = R + Q" % (y, sign), E.pt_add(R, big), r, 0)
    assert n_noncanon >= 4  # y = 0 (order 4) and y = 1 (the identity) at least, both signs
    # x = 0 with the sign bit set: y = 1 and y = -1
    for y, name in ((1, "1"), (P - 1, "-1")):
        r = (y | 1 << 255).to_bytes(32, "little")
        R = E.decode(r)
        assert R is not None and R[0] == 0
        add("R with x = 0, sign bit set, y = %s, P = R" % name, R, r, 1)
        add("R with x = 0, sign bit set, y = %s, P = R + T" % name, E.pt_add(R, small[6]), r, 1)
        add("R with x = 0, sign bit set, y = %s, P = R + Q" % name, E.pt_add(R, big), r, 0)
    # R off the curve
    off = []
    y = 2
    while len(off) < 3:
        if E.decode(y.to_bytes(32, "little")) is None:
            off.append(y.to_bytes(32, "little"))
        y += 1
    off.append((int.from_bytes(off[0], "little") | 1 << 255).to_bytes(32, "little"))
    for r in off:
        add("R off the curve", base[5], r, 0)
        add("R off the curve, P the identity", E.IDENTITY, r, 0)
    # R the identity against P of small order
    for t, o in zip(small, orders):
        add("R the identity, P of order %d" % o, t, E.encode(E.IDENTITY), 1)
    add("R the identity, P of large order", big, E.encode(E.IDENTITY), 0)
    # bits_in = 0 on a matching row
    add("bits_in = 0, P = R", base[0], E.encode(base[0]), 0, bit=0)
    add("bits_in = 0, P = R + T", E.pt_add(base[0], small[1]), E.encode(base[0]), 0, bit=0)
    # Z = 0 planted with X = 0: r the identity, so that a finish without the guard sees
    # X = 0 and Y = Z (all zero) and accepts
    # (0, p and -p as limbs: tests/finish_cases.py _zero_limbs; p's digits are floored, past the carried range)
    zero_forms = [FC._zero_limbs(t) for t in range(3)]
    assert all(PC.limb_val(z) % P == 0 for z in zero_forms) and len(set(zero_forms)) == 3
    for zf in zero_forms:
        for xf in zero_forms:
            for yv in (0, 1, rng.randrange(P)):
                rows.append(("Z = 0 planted with X = 0", xf, GC.fe_rep(yv, rng), zf, E.encode(E.IDENTITY), 1, 0))
    # limbs at the ends of the carried range
    for xl, yl, zl, pt in _extreme_rows(rng):
        rows.append(("limbs at the ends, P = R", xl, yl, zl, E.encode(pt), 1, 1))
        rows.append(("limbs at the ends, P = R + T8", xl, yl, zl, E.encode(E.pt_add(pt, E.pt_neg(small[7]))), 1, 1))
        rows.append(("limbs at the ends, P = R + Q", xl, yl, zl, E.encode(E.pt_add(pt, big)), 1, 0))
    for zl in (PC.CARRIED_LO, PC.CARRIED_HI):
        add("Z at the end of the range, P = R", base[1], E.encode(base[1]), 1, zl=zl)
        add("Z at the end of the range, P = R + T4", E.pt_add(base[1], small[2]), E.encode(base[1]), 1, zl=zl)
        add("Z at the end of the range, P = R + Q", E.pt_add(base[1], big), E.encode(base[1]), 0, zl=zl)
    rows += list(golden_rows())
    for name, xl, yl, zl, r, bit, want in rows:
        assert name.startswith("Z = 0") or all(PC.is_carried(c) for c in (xl, yl, zl)), name
        assert direct_expected(xl, yl, zl, r, bit) == want, name
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _bulk_pool():
    """64 (R, P) pairs for the bulk rows: P = R + T_j (accept) or R + T_j + Q (reject)."""
    rng = random.Random(64215)
    small = E.small_order_points()
    q = E.pt_mul(rng.randrange(1, L), E.BASE)
    pool = []
    for i in range(64):
        R = E.pt_mul(rng.randrange(1, L), E.BASE)
        pt = E.pt_add(R, small[i % 8])
        want = 1
        if i % 4 == 3:
            pt, want = E.pt_add(pt, q), 0
        pool.append((pt, E.encode(R), want))
    return tuple(pool)


@functools.lru_cache(maxsize=None)
def case(m):
    """m rows: the planted ones first (as many as fit, cycling so that m = 1 .. 65 still rotate
    through them by m), bulk rows from the pool after them.
    -> dict(m, xyz (m, 30) int32, r (m, 32) uint8, bits_in, exp, names)."""
    pl = planted()
    pool = _bulk_pool()
    rng = random.Random(1000 + m)
    xyz = np.zeros((m, 30), np.int64)
    r = np.zeros((m, 32), np.uint8)
    bits = np.zeros(m, np.uint8)
    exp = np.zeros(m, np.uint8)
    names = []
    start = (7 * m) % len(pl) if m < len(pl) else 0
    for p in range(m):
        if p < len(pl):
            name, xl, yl, zl, rb, bit, want = pl[(start + p) % len(pl)]
        else:
            pt, rb, want = pool[(p * 37) % len(pool)]
            xl, yl, zl = _proj(pt, _zs(rng), rng)
            bit = 0 if p % 11 == 5 else 1
            want = want if bit else 0
            name = "bulk"
        xyz[p] = np.array(tuple(xl) + tuple(yl) + tuple(zl), np.int64)
        r[p] = np.frombuffer(rb, np.uint8)
        bits[p], exp[p] = bit, want
        names.append(name)
    assert np.abs(xyz).max() < 2**27
    out = dict(m=m, xyz=xyz.astype(np.int32), r=r, bits_in=bits, exp=exp, names=tuple(names))
    for k in ("xyz", "r", "bits_in", "exp"):
        out[k].setflags(write=False)
    return out


def shuffled_perm(m, fin_base, seed):
    """fin_base + m entries, a permutation of [0, fin_base + m)."""
    return np.random.default_rng(seed).permutation(fin_base + m).astype(np.uint32)


def check(c, out, fin_base=0, perm=None):
    """out: the fin_base + m bytes after the finish.  Every position's byte equals the expectation
    (named), every other byte is untouched."""
    m = c["m"]
    assert out.shape == (fin_base + m,)
    idx = (np.arange(m) + fin_base) if perm is None else perm[fin_base:fin_base + m].astype(np.int64)
    got = out[idx]
    bad = np.flatnonzero(got != c["exp"])
    assert bad.size == 0, "%d rows differ, first: %s" % (
        bad.size, [(int(p), c["names"][p], int(got[p]), int(c["exp"][p])) for p in bad[:6]])
    rest = np.ones(fin_base + m, bool)
    rest[idx] = False
    assert (out[rest] == UNTOUCHED).all(), "a byte no position owns was written: %s" % np.flatnonzero(rest & (out != UNTOUCHED))[:8]
