"""Cases and expectations for the batched finish (csrc/kernels.hip launch_finish /
verify_finish_kernel / FinDev, csrc/verify_core.h finish_group): Montgomery's simultaneous inversion
over the G <= 16 slots a lane owns, then enc(X/Z, Y/Z) == R.  Shared by the host twin's test
(tests/test_kernel_host.py, hostsim_finish_raw) and the device's (tests/test_gpu_keyed_stages.py,
tmed_test_finish).  No GPU here; deterministic, cached, and callers must not modify what they get.

Expected bit of a row = bits_in && Z != 0 (mod p) && enc(X/Z, Y/Z) == r, in Python integers
(direct_expected).  The finish needs no curve points, so the bulk rows are drawn from pools: position
p takes the pair (x, y) number p * SA mod 4,099 and the Z number p * SB mod 257, with X = x Z and
Y = y Z; each pair is encoded once, and a bulk row's expectation follows from how it was built (the
host test checks that shortcut against direct_expected on every row of its cases).  Z comes as the raw
limb vectors of the pool, which hold both ends of the carried range (fe25519.h: what
ge_p1p1_to_p2 hands over); X and Y come in three limb forms of the same integer.  The planted rows
are built one by one and expected by direct_expected alone."""
import functools
import random

import numpy as np

import group_cases as GC
import prim_cases as PC
from oracle import ed25519_go as E

P = E.P
N_PAIRS, N_Z = 4099, 257  # both prime
SA, SB = 1031, 101
LANES, GROUP_MAX, FIN_CAP = 65536, 16, 1 << 20  # launch_finish kLanes, kernels.h kFinGroupMax, kFinCap
UNTOUCHED = 0xAA
_W = tuple(25 if i % 2 else 26 for i in range(10))


def groups(m):
    """(G, L) of launch_finish for m signatures."""
    G = min(GROUP_MAX, max(1, -(-m // LANES)))
    return G, -(-m // G)


def count_of(lane, m, L):
    return -(-(m - lane) // L) if lane < m else 0


def enc(x, y):
    """The 32 bytes the compare builds: canonical y, the parity of canonical x in bit 255."""
    return ((y % P) | ((x % P) & 1) << 255).to_bytes(32, "little")


def direct_expected(xl, yl, zl, r, bit):
    """One row's expected bit from its limbs alone."""
    z = PC.limb_val(zl) % P
    if not bit or z == 0:
        return 0
    zi = pow(z, P - 2, P)
    return int(enc(PC.limb_val(xl) * zi, PC.limb_val(yl) * zi) == bytes(r))


def limbs_of_ints(vals, style):
    """vals: integers in [0, 2^255); style: one of 0, 1, 2 per value -> (n, 10) int64 limbs of exactly
    that integer.  0: every limb floored (the canonical digits); 1: even limbs rounded into
    [-2^25, 2^25), odd floored (a product's output); 2: every limb rounded (fe_carry's output)."""
    n = len(vals)
    raw = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(n, 4)
    w64 = np.concatenate([raw, np.zeros((n, 1), np.uint64)], axis=1)
    h = np.zeros((n, 10), np.int64)
    for i, off in enumerate(PC.OFF):
        q, b = divmod(off, 64)
        v = w64[:, q] >> np.uint64(b)
        if b:
            v = v | (w64[:, q + 1] << np.uint64(64 - b))
        h[:, i] = (v & np.uint64((1 << _W[i]) - 1)).astype(np.int64)
    style = np.asarray(style)
    for i in range(9):
        rounded = (style == 2) | ((style == 1) & (i % 2 == 0))
        c = np.where(rounded, (h[:, i] + (1 << (_W[i] - 1))) >> _W[i], h[:, i] >> _W[i])
        h[:, i] -= c << _W[i]
        h[:, i + 1] += c
    return h


@functools.lru_cache(maxsize=None)
def pools():
    """xs, ys (4,099 field elements each), their encodings (4099, 32), the Z limb vectors (257, 10)
    and their values mod p (all non-zero)."""
    rng = random.Random(91)
    xs = [rng.randrange(P) for _ in range(N_PAIRS)]
    ys = [rng.randrange(P) for _ in range(N_PAIRS)]
    xs[:4], ys[:4] = [1, P - 1, 2, P - 2], [P - 1, 1, P - 20, 19]
    encs = np.frombuffer(b"".join(enc(x, y) for x, y in zip(xs, ys)), np.uint8).reshape(N_PAIRS, 32)
    small = [GC.split_limbs(v, c) for v in (1, -1, 2, P - 1, 1 - P, (P - 1) // 2) for c in (False, True)]
    zl = [PC.CARRIED_LO, PC.CARRIED_HI] + [z for z in small if z is not None]
    assert len(zl) >= 8
    while len(zl) < N_Z:
        z = PC.draw_carried(rng)  # 30 % of the draws at the ends of every limb's range
        if PC.limb_val(z) % P:
            zl.append(z)
    zv = [PC.limb_val(z) % P for z in zl]
    assert all(zv) and all(PC.is_carried(z) for z in zl)
    return xs, ys, encs, np.array(zl, np.int64), zv


def pool_index(p):
    return p * SA % N_PAIRS, p * SB % N_Z


@functools.lru_cache(maxsize=2)
def bulk(m):
    """Positions 0..m-1 -> xyz (m, 30) int32, r (m, 32) uint8, bits_in (m,), exp (m,).  A row
    matches unless p % 7 == 3 (bit p % 255 of r flipped); bits_in is 0 where p % 11 == 5."""
    xs, ys, encs, zl, zv = pools()
    p = np.arange(m, dtype=np.int64)
    a, b = p * SA % N_PAIRS, p * SB % N_Z
    al, bl = a.tolist(), b.tolist()
    style = (p // 5) % 3
    xyz = np.empty((m, 30), np.int64)
    xyz[:, 0:10] = limbs_of_ints([xs[i] * zv[j] % P for i, j in zip(al, bl)], style)
    xyz[:, 10:20] = limbs_of_ints([ys[i] * zv[j] % P for i, j in zip(al, bl)], (style + 1) % 3)
    xyz[:, 20:30] = zl[b]
    assert np.abs(xyz).max() < 2**27
    r = encs[a].copy()
    off = np.flatnonzero(p % 7 == 3)
    k = off % 255
    r[off, k // 8] ^= (1 << (k % 8)).astype(np.uint8)
    bits = (p % 11 != 5).astype(np.uint8)
    exp = (bits.astype(bool) & (p % 7 != 3)).astype(np.uint8)
    out = (xyz.astype(np.int32), r, bits, exp)
    for arr in out:
        arr.setflags(write=False)
    return out


# ---- planted rows ---------------------------------------------------------------------------------
def _flip(rb, bit):
    rb = bytearray(rb)
    rb[bit // 8] ^= 1 << (bit % 8)
    return bytes(rb)


def _row(x, y, zl, rng, r=None, bit=1):
    """Limbs of (x Z, y Z, Z) for the Z limb vector zl, r = enc(x, y) unless given."""
    z = PC.limb_val(zl) % P
    return (GC.fe_rep(x * z, rng), GC.fe_rep(y * z, rng), tuple(zl), enc(x, y) if r is None else r, bit)


def _extreme_row(xl, yl, zl):
    """A matching row whose X, Y, Z limbs are given (the ends of the carried range)."""
    zi = pow(PC.limb_val(zl) % P, P - 2, P)
    return (xl, yl, zl, enc(PC.limb_val(xl) * zi, PC.limb_val(yl) * zi), 1)


# name, expected bit: the compare rule steered from the point's side
KINDS = (("match, limbs at the upper end", 1), ("match, limbs at the lower end", 1), ("match, mixed ends", 1),
         ("r off by one bit in byte 0", 0), ("r off by one bit in byte 31", 0), ("r with the sign bit flipped", 0),
         ("x = 0, sign bit set in r", 0), ("x = 0, sign bit clear", 1), ("y < 19, r = y + p", 0),
         ("y < 19, r = y", 1), ("bits_in = 0 on a matching row", 0))


def _planted(kind, rng):
    xs, ys, _, zl, _ = pools()
    LO, HI = PC.CARRIED_LO, PC.CARRIED_HI
    z = tuple(int(v) for v in zl[rng.randrange(N_Z)])
    i = rng.randrange(4, N_PAIRS)
    x, y = xs[i], ys[i]
    if kind == 0:
        return _extreme_row(HI, HI, HI)
    if kind == 1:
        return _extreme_row(LO, LO, LO)
    if kind == 2:
        return _extreme_row(HI, LO, PC.draw_carried(rng) if rng.random() < 0.5 else LO)
    if kind == 3:
        return _row(x, y, z, rng, _flip(enc(x, y), 0))
    if kind == 4:
        return _row(x, y, z, rng, _flip(enc(x, y), 248 + rng.randrange(7)))
    if kind == 5:
        return _row(x, y, z, rng, _flip(enc(x, y), 255))
    if kind == 6:
        return _row(0, y, z, rng, _flip(enc(0, y), 255))
    if kind == 7:
        return _row(0, y, z, rng)
    ysmall = rng.randrange(19)
    x &= ~1  # sign bit clear, so y + p < 2^255 fits the 255 bits below it
    if kind == 8:
        return _row(x, ysmall, z, rng, (ysmall + P).to_bytes(32, "little"))
    if kind == 9:
        return _row(x, ysmall, z, rng)
    return _row(x, y, z, rng, bit=0)


def _zero_limbs(t):
    """Z = 0 (mod p) three ways: 0, p and -p."""
    p_digits = tuple(int(v) for v in limbs_of_ints([P], [0])[0])
    assert PC.limb_val(p_digits) == P
    return ((0,) * 10, p_digits, tuple(-v for v in p_digits))[t % 3]


# Z = 0 placements inside one lane's group of cnt slots
GUARDS = ("first slot", "middle slot", "last slot", "two slots", "every slot")


def _guard_slots(g, cnt):
    return ({0}, {cnt // 2}, {cnt - 1}, {0, cnt - 1}, set(range(cnt)))[g]


def anchors(m, G):
    """(lane, direction) of the lanes the planted rows start from: lane 0, the last lane that owns G
    slots, the first lane that owns G - 1, the last lane."""
    L = -(-m // G)
    last_full = m - (G - 1) * L - 1
    out = [(0, 1), (last_full, -1)]
    if last_full + 1 < L:
        out.append((last_full + 1, 1))
    out.append((L - 1, -1))
    assert count_of(last_full, m, L) == G and (last_full + 1 >= L or count_of(last_full + 1, m, L) == G - 1)
    return out


@functools.lru_cache(maxsize=4)
def case(m, bulk_m=None, G=None):
    """The case for m signatures: bulk rows (the first m of bulk(bulk_m)) with the planted ones written
    over them, placed for the device's group size, or for G where the host twin is given one.
    -> dict(m, G, L, full (every kind and placement is in), xyz, r, bits_in, exp, planted {position: kind name},
            guards [(placement name, lane, zero positions, neighbour positions)])."""
    G = G or groups(m)[0]
    L = -(-m // G)
    if G > 1:  # two slots of one lane never share a pool entry
        assert L % N_PAIRS and L % N_Z
    xyz, r, bits, exp = (a[:m].copy() for a in bulk(bulk_m or m))
    xs, ys, encs, zl, zv = pools()
    rng = random.Random(7 * m + 1)
    planted, guards, used = {}, [], set()

    def put(pos, row, want):
        xl, yl, z, rb, bit = row
        xyz[pos] = np.array(xl + yl + tuple(z), np.int64).astype(np.int32)
        r[pos] = np.frombuffer(rb, np.uint8)
        bits[pos] = bit
        exp[pos] = direct_expected(xl, yl, z, rb, bit)
        assert exp[pos] == want, (pos, want)

    def next_lane(lane, d):
        while 0 <= lane < L and lane in used:
            lane += d
        if not 0 <= lane < L:
            return None
        used.add(lane)
        return lane

    for start, d in anchors(m, G):
        lane = start
        for k, (name, want) in enumerate(KINDS):
            lane = next_lane(lane, d)
            if lane is None:
                break
            pos = lane + (k % count_of(lane, m, L)) * L
            put(pos, _planted(k, rng), want)
            planted[pos] = name
        for g, name in enumerate(GUARDS):
            lane = None if lane is None else next_lane(lane, d)
            if lane is None:
                break
            cnt = count_of(lane, m, L)
            zero = sorted(lane + j * L for j in _guard_slots(g, cnt))
            near = [lane + j * L for j in range(cnt) if lane + j * L not in zero]
            for t, pos in enumerate(zero):  # X, Y, r as if Z were 1: a guard that forgot to reject would match
                a, _ = pool_index(pos)
                x, y = xs[a], ys[a]
                put(pos, (GC.fe_rep(x, rng), GC.fe_rep(y, rng), _zero_limbs(g + t), enc(x, y), 1), 0)
                planted[pos] = "Z = 0, " + name
            for pos in near:  # matching neighbours: a poisoned inversion would reject them
                a, b = pool_index(pos)
                put(pos, _row(xs[a], ys[a], tuple(int(v) for v in zl[b]), rng), 1)
            guards.append((name, lane, zero, near))
    full = L >= 64  # room for four anchors' lanes: every kind and every placement made it in
    if full:
        assert {n for n, _ in KINDS} <= set(planted.values())
        assert {"Z = 0, " + n for n in GUARDS} <= set(planted.values())
        if G > 1:  # ... each beside matching neighbours (two slots of a group of two leave none)
            assert all(any(n == name and near for n, _, _, near in guards) for name in GUARDS[:3 if G == 2 else 4])
    for arr in (xyz, r, bits, exp):
        arr.setflags(write=False)
    return dict(m=m, G=G, L=L, full=full, xyz=xyz, r=r, bits_in=bits, exp=exp, planted=planted, guards=guards)


def shuffled_perm(m, fin_base, seed):
    """fin_base + m entries, a permutation of [0, fin_base + m)."""
    return np.random.default_rng(seed).permutation(fin_base + m).astype(np.uint32)


def check(c, out, fin_base=0, perm=None):
    """out: the fin_base + m bytes after the finish.  Every position's byte equals the expectation (the
    planted rows named one by one), every other byte is untouched."""
    m = c["m"]
    assert out.shape == (fin_base + m,)
    idx = (np.arange(m) + fin_base) if perm is None else perm[fin_base:fin_base + m].astype(np.int64)
    got = out[idx]
    for pos, name in c["planted"].items():
        assert got[pos] == c["exp"][pos], "%s: position %d (lane %d) gives %d" % (name, pos, pos % c["L"], got[pos])
    bad = np.flatnonzero(got != c["exp"])
    assert bad.size == 0, "%d rows differ, first at positions %s" % (bad.size, bad[:8])
    rest = np.ones(fin_base + m, bool)
    rest[idx] = False
    assert (out[rest] == UNTOUCHED).all(), "a byte no position owns was written: %s" % np.flatnonzero(rest & (out != UNTOUCHED))[:8]


def check_guards(c, out, fin_base=0, perm=None):
    """The Z = 0 rows are rejected and every neighbour in the same lane's group keeps its bit."""
    m = c["m"]
    idx = (np.arange(m) + fin_base) if perm is None else perm[fin_base:fin_base + m].astype(np.int64)
    assert c["guards"] or not c["full"]  # (a case of a few lanes has no room for them)
    for name, lane, zero, near in c["guards"]:
        for pos in zero:
            assert out[idx[pos]] == 0, "Z = 0 (%s) accepted at position %d, lane %d" % (name, pos, lane)
        for pos in near:
            assert c["exp"][pos] == 1
            assert out[idx[pos]] == 1, "Z = 0 (%s) in lane %d poisoned its neighbour at position %d" % (name, lane, pos)
