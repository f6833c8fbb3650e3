"""Input cases and expected values for the ZIP-215 batch mode's multi-scalar multiplication
(csrc/zip215.hip zip_msm, run on given rows by tmed_test_zip_msm): tests/test_gpu_zip_msm.py.
Deterministic (fixed seeds), built once per process, and not to be modified by callers.

Every point is a known multiple of the base point plus a known small-order component,
P_i = m_i B + j_i T8 (T8 a generator of the 8-torsion), so a window's expected value
sum_i d_i (-P_i) is ONE scalar multiplication of -(sum d_i m_i mod L) plus -(sum d_i j_i mod 8) T8,
all in oracle.ed25519_go integers.  The prime-order rows are a walk of single additions from four
fixed steps; the encodings come from one batched inversion.  The rows hold -P (the product's
niels_row_store), so every expected value carries that sign.

A case is a dict: n, idx (2n pool indices: the A rows, then the R rows), dig ((16, 2n) int16),
c (n integers), lo, cnt.  Every generator asserts its own coverage."""
import functools
import random

import numpy as np

import prim_cases as PC
from oracle import ed25519_go as E

P, L = E.P, E.L
WIN, ZWIN = 16, 8
POOL_WALK = 16400  # >= 2 * 8193 distinct prime-order points
TOP_MAX = 4097


def glog(w):
    """zip_glog: log2 of the buckets an accumulation lane of window w owns."""
    return 1 if w < 8 else (2 if w < 15 else 0)


# ---- the point pool -------------------------------------------------------------------------------
def _find_t8():
    y = 2
    while True:
        pt = E.decode(y.to_bytes(32, "little"))
        y += 1
        if pt is None:
            continue
        t = E.pt_mul(L, pt)
        if not E.pt_equal(E.pt_mul(4, t), E.IDENTITY):
            return t


def _batch_encode(pts):
    """E.encode of every point, with one inversion for all."""
    pre, acc = [], 1
    for p in pts:
        pre.append(acc)
        acc = acc * p[2] % P
    inv = pow(acc, P - 2, P)
    out = [None] * len(pts)
    for i in range(len(pts) - 1, -1, -1):
        zi = inv * pre[i] % P
        inv = inv * pts[i][2] % P
        x, y = pts[i][0] * zi % P, pts[i][1] * zi % P
        out[i] = (y | ((x & 1) << 255)).to_bytes(32, "little")
    return out


class Pool:
    """pts[i] = m[i] B + j[i] T8 (extended coordinates), enc[i] its encoding.  Indices 0 .. POOL_WALK - 1
    are distinct prime-order points; the named indices follow."""

    def __init__(self):
        rng = random.Random(0x215)
        self.t8 = _find_t8()
        steps = [rng.randrange(1, L) for _ in range(4)]
        step_pts = [E.pt_mul(s, E.BASE) for s in steps]
        m = rng.randrange(1, L)
        pt = E.pt_mul(m, E.BASE)
        self.m, self.j, self.pts = [], [], []
        for _ in range(POOL_WALK):
            self.m.append(m)
            self.j.append(0)
            self.pts.append(pt)
            k = rng.randrange(4)
            m = (m + steps[k]) % L
            pt = E.pt_add(pt, step_pts[k])
        assert len(set(self.m)) == POOL_WALK
        tors = [E.pt_mul(k, self.t8) for k in range(8)]
        self.named = {}

        def add(name, mm, jj):
            self.named[name] = len(self.m)
            self.m.append(mm % L)
            self.j.append(jj % 8)
            self.pts.append(E.pt_add(E.pt_mul(mm % L, E.BASE), tors[jj % 8]))

        add("identity", 0, 0)
        add("order2", 0, 4)
        add("order4", 0, 2)
        add("order4b", 0, 6)
        add("order8", 0, 1)
        add("order8b", 0, 3)
        add("mixed", self.m[7], 1)     # walk point 7 plus an order-8 component
        add("mixed4", self.m[9], 6)
        add("B", 1, 0)
        for k in (3, 11):              # -P of two walk points
            add("neg%d" % k, -self.m[k], 0)
        self.enc = _batch_encode(self.pts)
        self.enc_arr = np.frombuffer(b"".join(self.enc), np.uint8).reshape(-1, 32)
        # the encodings decode to the points they were made from
        for i in [0, 1, POOL_WALK - 1] + list(self.named.values()):
            assert E.pt_equal(E.decode(self.enc[i]), self.pts[i]), i
        assert self.enc[self.named["identity"]] == (1).to_bytes(32, "little")
        assert self.enc[self.named["B"]] == E.encode(E.BASE)
        assert E.pt_equal(E.pt_add(self.pts[3], self.pts[self.named["neg3"]]), E.IDENTITY)

    def __getitem__(self, name):
        return self.named[name]


@functools.lru_cache(maxsize=None)
def pool():
    return Pool()


# ---- expected values ------------------------------------------------------------------------------
def group_rows(case):
    """(rows of the group among the A rows, among the R rows)."""
    n, lo, cnt = case["n"], case["lo"], case["cnt"]
    return range(lo, lo + cnt), range(n + lo, n + lo + cnt)


def window_scalars(case):
    """Per window (s, t): the window's value is -(s B + t T8), s mod L and t mod 8, over the rows of
    the group only; R rows count in windows 0..7 only."""
    pl = pool()
    ra, rr = group_rows(case)
    idx, dig = case["idx"], case["dig"]
    out = []
    for w in range(WIN):
        rows = list(ra) + (list(rr) if w < ZWIN else [])
        d = dig[w]
        s = sum(int(d[r]) * pl.m[idx[r]] for r in rows) % L
        t = sum(int(d[r]) * pl.j[idx[r]] for r in rows) % 8
        out.append((s, t))
    return out


def expected_windows(case):
    pl = pool()
    out = []
    for s, t in window_scalars(case):
        q = E.pt_mul((-s) % L, E.BASE) if s else E.IDENTITY
        if t:
            q = E.pt_add(q, E.pt_mul((-t) % 8, pl.t8))
        out.append(q)
    return out


def expected_windows_per_row(case):
    """The same values by plain per-row scalar multiplication and sum (small cases only)."""
    pl = pool()
    ra, rr = group_rows(case)
    assert len(ra) + len(rr) <= 64
    out = []
    for w in range(WIN):
        acc = E.IDENTITY
        for r in list(ra) + (list(rr) if w < ZWIN else []):
            d = int(case["dig"][w][r])
            q = E.pt_neg(pl.pts[case["idx"][r]])
            acc = E.pt_add(acc, E.pt_mul(abs(d), E.pt_neg(q) if d < 0 else q))
        out.append(acc)
    return out


def expected_ctot(case):
    return sum(case["c"][case["lo"]:case["lo"] + case["cnt"]]) % L


def expected_flag(case):
    """[8](sum_w 2^(16 w) W_w + [ctot] B) = O: the [8] removes the torsion part, so the flag is 1
    exactly when the scalar of B vanishes mod L."""
    tot = expected_ctot(case)
    for w, (s, _) in enumerate(window_scalars(case)):
        tot -= s << (16 * w)
    return 1 if tot % L == 0 else 0


def device_point(limbs4):
    """(X, Y, Z, T) mod p of one window's (4, 10) limbs."""
    return tuple(PC.limb_val([int(v) for v in f]) % P for f in limbs4)


def same_point(dev, want):
    """The device's extended point equals `want` as an affine point and its T is X Y / Z."""
    x, y, z, t = dev
    return z != 0 and E.pt_equal(dev, want) and (x * y - t * z) % P == 0


def case_arrays(case):
    pl = pool()
    n = case["n"]
    pts = pl.enc_arr[np.asarray(case["idx"], np.int64)]
    c = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in case["c"]), np.uint8).reshape(n, 32)
    return pts, case["dig"], c


def _case(n, idx, dig, c=None, lo=0, cnt=None):
    assert len(idx) == 2 * n and dig.shape == (WIN, 2 * n) and dig.dtype == np.int16
    assert dig[15, :n].min() >= 0 and dig[15, :n].max() <= TOP_MAX
    return {"n": n, "idx": list(idx), "dig": dig, "c": list(c) if c is not None else [0] * n, "lo": lo,
            "cnt": n if cnt is None else cnt}


# ---- one-hot digits -------------------------------------------------------------------------------
def onehot_magnitudes(w):
    """|digit| values of window w at which the owner of a bucket changes: the ends of a lane's bucket
    group, the wave boundary at item 63/64, the sort's byte boundary, the 256-thread block boundary
    of zip_accum_kernel (lane 255/256), the level-1 boundary at item 4095/4096, the last items."""
    g = 1 << glog(w)
    if w == 15:  # one bucket per group, two lanes per group
        return [1, 2, 3, 63, 64, 127, 128, 129, 255, 256, 257, 0x0101, 0x0201, 4095, 4096, 4097]
    ends = [1, 2, 3] if g == 2 else [3, 4, 7, 8]
    return ends + [64 * g - 1, 64 * g, 255, 256, 257, 0x0101, 0x0201, 256 * g - 1, 256 * g, 4096 * g - 1,
                   4096 * g, 32767, 32768]


@functools.lru_cache(maxsize=None)
def onehot_cases(rows_kind, flip):
    """cnt = 2 rows; per window ONE non-zero digit, on the A rows (rows_kind "A": row w % 2, all 16
    windows) or on the R rows (rows_kind "R": windows 0..7, with A digits in windows 8..15 only).
    Case k takes magnitude k of every window's list; the sign alternates with k + w, `flip` swaps
    it (32768 only as -32768; the top window only non-negative)."""
    n = 2
    cases = []
    lists = [onehot_magnitudes(w) for w in range(WIN)]
    for k in range(max(len(l) for l in lists)):
        dig = np.zeros((WIN, 2 * n), np.int16)
        for w in range(WIN):
            v = lists[w][k % len(lists[w])]
            neg = ((k + w) % 2 == 1) != bool(flip)
            if v == 32768:
                neg = True
            if w == 15:
                neg = False
            if v == 32767 and flip:  # keep both ends in both passes
                v, neg = 32768, True
            row = (w + k) % 2 + (n if rows_kind == "R" and w < ZWIN else 0)
            dig[w, row] = -v if neg else v
        cases.append(_case(n, [k % 50, 60 + k, 100 + 2 * k, 200 + k], dig, c=[5 + k, 1 << 200]))
    for w in range(WIN):  # every magnitude of every window was used
        used = {int(np.abs(c["dig"][w].astype(np.int32)).max()) for c in cases}
        want = set(lists[w]) if not flip else {32768 if v == 32767 else v for v in lists[w]}
        assert used == want, (w, sorted(want - used))
    return tuple(cases)


PAIRS = ((0x0101, 0x0201), (0x0201, 0x0101), (0x0101, 0x0102), (255, 256), (256, 257), (257, 255), (1, 2), (3, 2),
         (127, 128), (0x0100, 0x0200), (0x01ff, 0x0200), (4095, 4096), (4097, 4096))


@functools.lru_cache(maxsize=None)
def pair_cases():
    """cnt = 2: two digits per window that share a low byte (one bin of the sort's first pass, two of
    its second), share a high byte, or sit on either side of a boundary, in both row orders and
    with mixed signs; the A rows take pair k + w, the R rows (windows 0..7) pair k + w + 5."""
    n = 2
    cases = []
    for k in range(len(PAIRS)):
        dig = np.zeros((WIN, 2 * n), np.int16)
        for w in range(WIN):
            a, b = PAIRS[(k + w) % len(PAIRS)]
            sa, sb = (1, -1) if (w % 2 and w != 15) else (1, 1)
            dig[w, 0], dig[w, 1] = sa * a, sb * b
            if w < ZWIN:
                a, b = PAIRS[(k + w + 5) % len(PAIRS)]
                dig[w, n], dig[w, n + 1] = -a, b
        cases.append(_case(n, [500 + k, 600 + k, 700 + k, 800 + k], dig, c=[k, L - 1 - k]))
    return tuple(cases)


# ---- weighted sums --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weighted_case(lane0):
    """24 signatures; in every window the g buckets of lanes lane0 - 1, lane0, lane0 + 1 all filled
    with distinct points, both signs (A rows, and R rows in windows 0..7); the top window's buckets
    lane0 .. lane0 + 3 hold runs of 1, 2, 3 and 5 entries (halved by its two lanes)."""
    n = 24
    dig = np.zeros((WIN, 2 * n), np.int16)
    for w in range(15):
        g = 1 << glog(w)
        base, span = g * (lane0 - 1), 3 * g
        for i in range(n):
            dig[w, i] = (base + (i * 5 + w) % span) * (-1 if (i + w) % 3 == 0 else 1)
            if w < ZWIN:
                dig[w, n + i] = (base + (i * 7 + 3) % span) * (-1 if i % 2 else 1)
        vals = set(np.abs(dig[w, :n].astype(np.int32)).tolist())
        assert vals == set(range(base, base + span)), w
    runs = [lane0] * 1 + [lane0 + 1] * 2 + [lane0 + 2] * 3 + [lane0 + 3] * 5
    for i, v in enumerate(runs):
        dig[15, (i * 7) % n] = v  # spread over the rows
    assert sorted(dig[15, :n].tolist())[-11:] == sorted(runs)
    return _case(n, list(range(300, 300 + 2 * n)), dig, c=[(i + 1) << (10 * i) for i in range(n)])


# ---- runs -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run_case():
    """130 rows sharing ONE digit per window (the lanes beside the bucket are empty): the run starts
    with P, -P (the sum passes through the identity), then the same point twice, the identity, the
    order-2, -4 and -8 points and two mixed-order points, then distinct points."""
    pl = pool()
    n = 130
    a_idx = [3, pl["neg3"], 5, 5, pl["identity"], pl["order2"], pl["order4"], pl["order8"], pl["mixed"],
             pl["mixed4"], pl["order4b"], pl["order8b"]]
    a_idx += list(range(1000, 1000 + n - len(a_idx)))
    r_idx = [11, pl["neg11"], pl["order8"], pl["order8"]] + list(range(2000, 2000 + n - 4))
    dig = np.zeros((WIN, 2 * n), np.int16)
    for w in range(WIN):
        g = 1 << glog(w)
        v = 4097 if w == 15 else [g * 9 + 1, 128 * g - 1, 64 * g, 32767, 5, 256, 0x0201, 32768][w % 8]
        dig[w, :n] = -v if (w % 2 == 1 and w != 15) or v == 32768 else v
        if w < ZWIN:
            v2 = (v ^ 0x0100) if v < 32768 else 0x7f00  # another bucket, same low byte
            dig[w, n:] = -v2 if w % 3 == 0 else v2
    return _case(n, a_idx + r_idx, dig, c=[L - 1 - i for i in range(n)])


# ---- sort boundaries ------------------------------------------------------------------------------
SORT_CNTS = (2048, 2049, 4096, 4097, 8193)
# <= 40 |digit| values: equal keys span tiles; groups sharing a low byte and groups sharing a high byte
SORT_VALUES = (0, 1, 2, 3, 0x00ff, 0x0100, 0x0101, 0x0201, 0x0301, 0x7f01, 0x0102, 0x0103, 0x01ff, 0x02ff,
               0x7fff, 0x8000, 0x7f00, 0x7ffe, 0x1234, 0x1235, 0x1334, 0x3412, 0x0f0f, 0x0ff0, 0xf00 + 0x0f,
               0x4000, 0x4001, 0x3fff, 0x2000, 0x1fff, 0x00fe, 0x01fe, 0x5555, 0x2aaa, 0x0800, 0x07ff,
               0x7e7e, 0x7e7f, 0x0010, 0x1000)


@functools.lru_cache(maxsize=None)
def sort_case(cnt):
    assert len(set(SORT_VALUES)) <= 40
    rng = np.random.default_rng(cnt)
    n = cnt
    vals = np.array(sorted(set(SORT_VALUES)), np.int32)
    mag = vals[rng.integers(0, len(vals), (WIN, 2 * n))]
    sign = np.where(rng.integers(0, 2, (WIN, 2 * n)) == 1, -1, 1)
    sign[mag == 0x8000] = -1
    dig = (mag * sign).astype(np.int32)
    top = vals[vals <= TOP_MAX]  # the top window: the values of the set it can hold
    assert len(top) >= 20
    dig[15, :n] = top[rng.integers(0, len(top), n)]
    dig = dig.astype(np.int16)
    idx = rng.permutation(POOL_WALK)[:2 * n].tolist()
    return _case(n, idx, dig, c=[int(x) for x in rng.integers(1, 1 << 62, n)])


# ---- sub-ranges -----------------------------------------------------------------------------------
SUB_RANGES = ((0, 300), (0, 1), (299, 1), (1, 298), (150, 150), (149, 2))


@functools.lru_cache(maxsize=None)
def _random_rows(n, seed):
    """Every row with non-zero digits in every window it has, and a non-zero c."""
    rng = np.random.default_rng(seed)
    dig = rng.integers(-32768, 32768, (WIN, 2 * n)).astype(np.int32)
    dig[dig == 0] = 1
    dig[15, :n] = rng.integers(1, TOP_MAX + 1, n)
    pr = random.Random(seed)
    c = [pr.randrange(1, L) for _ in range(n)]
    idx = rng.permutation(POOL_WALK)[:2 * n].tolist()
    return idx, dig.astype(np.int16), c


def subrange_case(lo, cnt, n=300, seed=300):
    idx, dig, c = _random_rows(n, seed)
    assert (dig[:, :n] != 0).all() and (dig[:ZWIN] != 0).all() and all(c)
    return _case(n, idx, dig, c=c, lo=lo, cnt=cnt)


# ---- ctot -----------------------------------------------------------------------------------------
def ctot_cases():
    """cnt in {1, 255, 256, 257} at lo = 37 and lo = 0 of n = 600, with every c = L - 1, every c = 0,
    and random c < L; all digits zero (every window the identity)."""
    n = 600
    pr = random.Random(77)
    kinds = {"max": [L - 1] * n, "zero": [0] * n, "random": [pr.randrange(L) for _ in range(n)]}
    dig = np.zeros((WIN, 2 * n), np.int16)
    idx = list(range(2 * n))
    out = []
    for kind, c in kinds.items():
        for lo in (37, 0, 300):
            for cnt in (1, 255, 256, 257):
                out.append(("%s lo=%d cnt=%d" % (kind, lo, cnt), _case(n, idx, dig, c=c, lo=lo, cnt=cnt)))
    return out


# ---- flag -----------------------------------------------------------------------------------------
def flag_cases():
    """(name, case, flag): an A row equal to B with digit d in window w and c = d 2^(16 w) (the row
    holds -B: the total is the identity) -> 1; c one more -> 0; a total equal to an order-8 point
    -> 1; all digits zero with c = 0 (the all-invalid group) -> 1, with c = 1 -> 0."""
    pl = pool()
    out = []
    for w, d in ((0, 12345), (0, -32768), (3, 777), (15, 4097)):
        for extra, flag in ((0, 1), (1, 0)):
            dig = np.zeros((WIN, 2), np.int16)
            dig[w, 0] = d
            c = ((d << (16 * w)) + extra) % L
            out.append(("B w=%d d=%d c+%d" % (w, d, extra), _case(1, [pl["B"], 0], dig, c=[c]), flag))
    dig = np.zeros((WIN, 2), np.int16)
    dig[0, 0] = 1
    out.append(("order-8 total", _case(1, [pl["order8"], 0], dig, c=[0]), 1))
    dig = np.zeros((WIN, 4), np.int16)
    dig[2, 0], dig[2, 3] = 5, 3  # 5 (-(P + T8)) + 3 (-T4) with c = 5 m 2^32: an order-8 total again
    c = (5 * pl.m[pl["mixed"]] << 32) % L
    out.append(("mixed-order total", _case(2, [pl["mixed"], 1, 2, pl["order4"]], dig, c=[c, 0]), 1))
    zero = np.zeros((WIN, 6), np.int16)
    out.append(("all zero", _case(3, [0, 1, 2, 3, 4, 5], zero, c=[0, 0, 0]), 1))
    out.append(("all zero, c = 1", _case(3, [0, 1, 2, 3, 4, 5], zero, c=[0, 1, 0]), 0))
    for name, case, flag in out:
        assert expected_flag(case) == flag, name
    return out
