"""Input cases and expected values for the group layer: the point formulas of ge25519.h and the
group helpers of verify_core.h (hostsim_ge on the host build, devprim_ge on the device) and the
quad-lane formulas of quad.h (devprim_quad, device only).  Shared by tests/test_group_host.py and
tests/test_gpu_group.py; deterministic (fixed seeds), cached, and not to be modified by callers.

Two kinds of cases.  The formulas are polynomial identities in the coordinates, so the "formula"
cases draw every coordinate as an independent limb vector at the width the function's contract
allows (carried, 2-sum, 3-sum), with the all-low and all-high vectors in every slot: limb
extremes no real signature reaches.  The "real" cases are curve points in non-canonical
representations (scaled by a random lambda, shifted by a multiple of p), exceptional pairs
included, compared with oracle.ed25519_go.  Expected values are Python integers mod p.

Every generator asserts its own coverage, so it cannot thin out silently."""
import functools
import itertools
import random

import prim_cases as PC
from oracle import ed25519_go as E

P = E.P
D2 = E.D2
INV_D = pow(E.D, P - 2, P)
LO, HI, MAG = PC.CARRIED_LO, PC.CARRIED_HI, PC.CARRIED_MAG
ZERO = (0,) * 10
I32_MIN, I32_MAX = -(2**31), 2**31 - 1
val = PC.limb_val

# op numbers of tests/native/ge_ops.h (hostsim_ge, devprim_ge)
(GE_P2_DBL, GE_ADD_CACHED, GE_ADD_CACHED_PRE, GE_MADD_NIELS, GE_P1P1_TO_P2, GE_P1P1_TO_P3, GE_P3_TO_CACHED,
 GE_CACHED_TO_P3, GE_P3_ADD, GE_P3_TO_NIELS) = range(10)
GE_NAMES = ("ge_p2_dbl", "ge_add_cached", "ge_add_cached_pre", "ge_madd_niels", "ge_p1p1_to_p2", "ge_p1p1_to_p3",
            "ge_p3_to_cached", "ge_cached_to_p3", "ge_p3_add", "ge_p3_to_niels")
GE_HAS_NEG = (GE_ADD_CACHED, GE_ADD_CACHED_PRE, GE_MADD_NIELS)
# op numbers of devprim_quad
Q_DBL, Q_ADD, Q_TO_CACHED, Q_IDENTITY, Q_IDENTITY_CACHED, Q_COMB_TAKE, Q_CHAIN = range(7)
Q_NAMES = ("quad_dbl", "quad_add", "quad_to_cached", "quad_identity", "quad_identity_cached", "comb_take", "chain")

# Width of every input slot (1 = carried, k = a sum of k carried values), from the functions'
# comments: ge_p2_dbl "X, Y carried" and fe_sq2 of a carried Z; cached Y+X / Y-X are 2-sums
# (ge_p3_to_cached); niels and unpacked cached fields "up to twice a carried limb"; p1p1
# coordinates "<= 3-sums".  ge_p3_to_niels is not a formula on free limbs (it inverts Z).
GE_WIDTHS = {
    GE_P2_DBL: (1, 1, 1),
    GE_ADD_CACHED: (1, 1, 1, 1, 2, 2, 1, 1),
    GE_ADD_CACHED_PRE: (1, 1, 1, 1, 2, 2, 1, 1),
    GE_MADD_NIELS: (1, 1, 1, 1, 2, 2, 2),
    GE_P1P1_TO_P2: (3, 3, 3, 3),
    GE_P1P1_TO_P3: (3, 3, 3, 3),
    GE_P3_TO_CACHED: (1, 1, 1, 1),
    GE_CACHED_TO_P3: (2, 2, 2, 2),
    GE_P3_ADD: (1, 1, 1, 1, 1, 1, 1, 1),
}
# What each output coordinate's limbs must satisfy: "prod" a product output (carried), "carry" an
# fe_carry output, "p1p1" at most a sum or difference of three carried values, limb by limb,
# "exact" limbs known exactly (checked in check_ge_formula), None unused.
GE_OUT_RANGE = {
    GE_P2_DBL: ("p1p1",) * 4,
    GE_ADD_CACHED: ("p1p1",) * 4,
    GE_ADD_CACHED_PRE: ("p1p1",) * 4,
    GE_MADD_NIELS: ("p1p1",) * 4,
    GE_P1P1_TO_P2: ("prod", "prod", "prod", None),
    GE_P1P1_TO_P3: ("prod",) * 4,
    GE_P3_TO_CACHED: ("exact", "exact", "exact", "prod"),
    GE_CACHED_TO_P3: ("carry", "carry", "carry", "prod"),
    GE_P3_ADD: ("prod",) * 4,
    GE_P3_TO_NIELS: ("carry", "carry", "prod", None),
}


def scaled(k, c):
    return tuple(k * v for v in c)


def limb_add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def limb_sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def wrap_neg32(x):
    """-x as the device computes it in int32: INT32_MIN stays."""
    return ((-x + 2**31) % 2**32) - 2**31


def limb_range_ok(kind, i, v):
    if kind == "prod":
        return PC.in_carried_output_range(i, v)
    if kind == "carry":  # fe_carry64's ranges (PC.PACK_*) lie beside the products'
        return PC.in_carried_output_range(i, v) or PC.PACK_LO[i] <= v <= PC.PACK_HI[i]
    if kind == "p1p1":  # a sum or DIFFERENCE of three carried values: three times the larger end, either sign
        return abs(v) <= 3 * MAG[i]
    return True


def _wide(rng, w, twice_ok=False):
    """A w-sum; for the "twice a carried limb" slots 30 % of the draws are exactly 2 x carried."""
    if twice_ok and w == 2 and rng.random() < 0.3:
        return scaled(2, PC.draw_carried(rng))
    return PC.draw_nsum(rng, w, signed=w > 1 and rng.random() < 0.5)


def _extreme_slots(widths):
    """Every assignment of the all-low / all-high vector (at the slot's width) to the slots; then,
    the wide slots being sums or DIFFERENCES of carried values (Y - X, B - A, ...), every assignment
    of -+ w x the larger end to the wide slots, beside all-low and beside all-high narrow ones."""
    for bits in itertools.product((0, 1), repeat=len(widths)):
        yield tuple(scaled(w, HI if b else LO) for w, b in zip(widths, bits))
    wide = [j for j, w in enumerate(widths) if w > 1]
    for bits in itertools.product((0, 1), repeat=len(wide)):
        for narrow in (LO, HI):
            s = [narrow] * len(widths)
            for j, b in zip(wide, bits):
                s[j] = scaled(widths[j] if b else -widths[j], MAG)
            if wide:
                yield tuple(s)


def _pad8(slots):
    return tuple(slots) + (ZERO,) * (8 - len(slots))


# ---- b. formula identities: ge table ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ge_formula_cases(op):
    """(neg, in[8]) cases of one ge op on free limb vectors: every all-low / all-high assignment of
    the slots (with both neg values where the function takes one), then random draws up to about
    900 cases; the count leaves a partial last block of 64 lanes."""
    widths = GE_WIDTHS[op]
    rng = random.Random(1000 + op)
    negs = (0, 1) if op in GE_HAS_NEG else (0,)
    twice = op in (GE_MADD_NIELS, GE_CACHED_TO_P3)
    cases = [(neg, _pad8(s)) for s in _extreme_slots(widths) for neg in negs]
    n_ext = len(cases)
    while len(cases) < max(900, n_ext + 400) or len(cases) % 64 == 0:
        neg = rng.choice(negs)
        cases.append((neg, _pad8(tuple(_wide(rng, w, twice) for w in widths))))
    # coverage: both extremes in every slot, both neg values, a partial last block
    for j, w in enumerate(widths):
        assert any(c[1][j] == scaled(w, LO) for c in cases) and any(c[1][j] == scaled(w, HI) for c in cases), (op, j)
    assert {c[0] for c in cases} == set(negs), op
    assert len(cases) > 64 and len(cases) % 64 != 0, (op, len(cases))
    return tuple(cases)


def _add_formula(p, pq, mq, c_factor, d, neg):
    """(a - b, a + b, d + c, d - c) of the three additions; p = (X1, Y1, Z1, T1) integers."""
    X1, Y1, _, T1 = p
    a, b = (Y1 + X1) * pq, (Y1 - X1) * mq
    c = (-1 if neg else 1) * c_factor * T1
    return [(a - b) % P, (a + b) % P, (d + c) % P, (d - c) % P]


def ge_formula_expected(op, neg, ins):
    """Expected output coordinates mod p (None where the op leaves the slot unused)."""
    v = [val(c) for c in ins]
    if op == GE_P2_DBL:
        X, Y, Z = v[:3]
        return [2 * X * Y % P, (Y * Y + X * X) % P, (Y * Y - X * X) % P, (2 * Z * Z - Y * Y + X * X) % P]
    if op in (GE_ADD_CACHED, GE_ADD_CACHED_PRE):
        ypx, ymx, zq, t2d = v[4:8]
        if op == GE_ADD_CACHED and neg:
            ypx, ymx = ymx, ypx  # _pre gets the operand already exchanged: used as given
        return _add_formula(v[:4], ypx, ymx, t2d, 2 * v[2] * zq, neg)
    if op == GE_MADD_NIELS:
        ypx, ymx, xy2d = v[4:7]
        if neg:
            ypx, ymx = ymx, ypx
        return _add_formula(v[:4], ypx, ymx, xy2d, 2 * v[2], neg)
    if op in (GE_P1P1_TO_P2, GE_P1P1_TO_P3):
        X, Y, Z, T = v[:4]
        return [X * T % P, Y * Z % P, Z * T % P, X * Y % P if op == GE_P1P1_TO_P3 else None]
    if op == GE_P3_TO_CACHED:
        X, Y, Z, T = v[:4]
        return [(Y + X) % P, (Y - X) % P, Z % P, D2 * T % P]
    if op == GE_CACHED_TO_P3:
        p_, m_, Z, t2d = v[:4]
        return [(p_ - m_) % P, (p_ + m_) % P, 2 * Z % P, t2d * INV_D % P]
    if op == GE_P3_ADD:  # ge_p3_to_cached, ge_add_cached, ge_p1p1_to_p3 composed
        X2, Y2, Z2, T2 = v[4:8]
        x, y, z, t = _add_formula(v[:4], Y2 + X2, Y2 - X2, D2 * T2, 2 * v[2] * Z2, False)
        return [x * t % P, y * z % P, z * t % P, x * y % P]
    raise ValueError(op)


def check_ge_formula(op, neg, ins, limbs, encs):
    """The assertions on one formula case: limbs [4][10] raw outputs, encs [4] canonical values."""
    what = (GE_NAMES[op], neg, ins)
    exp = ge_formula_expected(op, neg, ins)
    kinds = GE_OUT_RANGE[op]
    for k in range(4):
        if exp[k] is None:
            continue
        assert encs[k] == exp[k], what + ("coordinate", k)
        assert val(limbs[k]) % P == exp[k], what + ("limbs of coordinate", k)
        for i in range(10):
            assert limb_range_ok(kinds[k], i, limbs[k][i]), what + ("limb", k, i, limbs[k][i])
    if op == GE_P3_TO_CACHED:  # Y + X, Y - X limb by limb, Z copied
        X, Y, Z = ins[0], ins[1], ins[2]
        assert (tuple(limbs[0]), tuple(limbs[1]), tuple(limbs[2])) == (limb_add(Y, X), limb_sub(Y, X), Z), what


# ---- b. formula identities: quad table ----------------------------------------------------------
def _garbage(rng):
    r = rng.random()
    if r < 0.25:
        return (I32_MIN,) * 10
    if r < 0.5:
        return (I32_MAX,) * 10
    return tuple(rng.choice((I32_MIN, I32_MAX, rng.randint(I32_MIN, I32_MAX))) for _ in range(10))


def _quad_lane3(rng):
    """The cached operand's 2Z lane: carried, or twice a carried value (quad_to_cached's output)."""
    c = PC.draw_carried(rng)
    return scaled(2, c) if rng.random() < 0.5 else c


@functools.lru_cache(maxsize=None)
def quad_formula_cases(op):
    """(v[4], q[4]) per quad for quad_dbl (T garbage at the int32 extremes: it must not be read),
    quad_add (v carried, q lanes 0 and 1 2-sums, lane 2 carried, lane 3 carried or twice carried)
    and quad_to_cached: every all-low / all-high assignment, then random draws up to about 900;
    the count leaves a partial last block of 16 quads."""
    rng = random.Random(2000 + op)
    z4 = (ZERO,) * 4
    cases = []
    if op == Q_DBL:
        for s in _extreme_slots((1, 1, 1)):
            for g in ((I32_MIN,) * 10, (I32_MAX,) * 10, _garbage(rng)):
                cases.append((s + (g,), z4))
        draw = lambda: (tuple(PC.draw_carried(rng) for _ in range(3)) + (_garbage(rng),), z4)
        slots = (1, 1, 1)
    elif op == Q_ADD:
        for s in _extreme_slots((1, 1, 1, 1, 2, 2, 1, 1)):
            cases.append((s[:4], s[4:]))
        for s in _extreme_slots((1, 1, 1, 1, 2, 2, 1, 2)):  # 2Z lane at twice the extremes
            if s[0] == s[1] == s[2] == s[3]:
                cases.append((s[:4], s[4:]))
        draw = lambda: (tuple(PC.draw_carried(rng) for _ in range(4)),
                        (PC.draw_nsum(rng, 2), PC.draw_nsum(rng, 2), PC.draw_carried(rng), _quad_lane3(rng)))
        slots = (1, 1, 1, 1, 2, 2, 1, 1)
    elif op == Q_TO_CACHED:
        for s in _extreme_slots((1, 1, 1, 1)):
            cases.append((s, z4))
        draw = lambda: (tuple(PC.draw_carried(rng) for _ in range(4)), z4)
        slots = (1, 1, 1, 1)
    else:
        raise ValueError(op)
    while len(cases) < 900 or len(cases) % 16 == 0:
        cases.append(draw())
    for j, w in enumerate(slots):
        flat = [(c[0] + c[1])[j] for c in cases]
        assert scaled(w, LO) in flat and scaled(w, HI) in flat, (op, j)
    if op == Q_DBL:
        assert any(c[0][3] == (I32_MIN,) * 10 for c in cases) and any(c[0][3] == (I32_MAX,) * 10 for c in cases)
    assert len(cases) % 16 != 0
    return tuple(cases)


def _round2(e, f, g, h):
    return [e * f % P, g * h % P, f * g % P, e * h % P]


def quad_formula_expected(op, v, q):
    """Expected lane values mod p (quad_to_cached: None on the lanes checked limb by limb)."""
    if op == Q_DBL:
        X, Y, Z = val(v[0]), val(v[1]), val(v[2])
        return _round2(2 * X * Y, Y * Y - X * X - 2 * Z * Z, Y * Y - X * X, -X * X - Y * Y)
    if op == Q_ADD:
        X, Y, Z, T = (val(c) for c in v)
        q0, q1, q2, q3 = (val(c) for c in q)
        a, b, c, d = (Y - X) * q0, (Y + X) * q1, T * q2, Z * q3
        return _round2(b - a, d - c, d + c, b + a)
    raise ValueError(op)


def check_quad_formula(op, v, q, out):
    """The assertions on one quad formula case; out is [4][10] raw limbs."""
    what = (Q_NAMES[op], v, q)
    if op == Q_TO_CACHED:
        X, Y, Z, T = v
        assert tuple(out[0]) == limb_sub(Y, X) and tuple(out[1]) == limb_add(Y, X), what
        assert tuple(out[3]) == scaled(2, Z), what
        assert val(out[2]) % P == D2 * val(T) % P, what
        assert all(PC.in_carried_output_range(i, out[2][i]) for i in range(10)), what + (out[2],)
        return
    exp = quad_formula_expected(op, v, q)
    for r in range(4):
        assert val(out[r]) % P == exp[r], what + ("lane", r)
        for i in range(10):
            assert PC.in_carried_output_range(i, out[r][i]), what + ("limb", r, i, out[r][i])


# ---- comb_take ----------------------------------------------------------------------------------
COMB_ROWS = 451


@functools.lru_cache(maxsize=None)
def comb_take_cases():
    """(window, digits): a synthetic window of COMB_ROWS 128-byte rows (32 int32: YpX, YmX, XY2d and
    two unused words) and 901 digits: 0 and +-j for every row j, shuffled.  Row limbs sit at the
    ends of the carried and twice-carried ranges and of int32 (INT32_MIN, whose negation wraps)."""
    rng = random.Random(3001)
    fixed = [LO, HI, (I32_MIN,) * 10, (I32_MAX,) * 10, scaled(2, LO), scaled(2, HI),
             tuple(I32_MIN if i % 2 else I32_MAX for i in range(10)), tuple(I32_MAX if i % 2 else I32_MIN for i in range(10)),
             (I32_MIN + 1,) * 10, (-1,) * 10, ZERO]

    def field():
        r = rng.random()
        if r < 0.3:
            return rng.choice(fixed)
        if r < 0.6:
            return scaled(2, PC.draw_carried(rng)) if rng.random() < 0.5 else PC.draw_carried(rng)
        return tuple(rng.choice((I32_MIN, I32_MAX, rng.randint(I32_MIN, I32_MAX))) for _ in range(10))

    rows = [f + f + f + (I32_MIN, I32_MAX) for f in fixed]  # the same extreme in all three fields
    rows[-1] = fixed[2] + fixed[3] + fixed[2] + (0, 0)
    while len(rows) < COMB_ROWS - 1:
        rows.append(field() + field() + field() + (rng.randint(I32_MIN, I32_MAX), rng.randint(I32_MIN, I32_MAX)))
    rows.append(fixed[3] + fixed[2] + fixed[2] + (I32_MAX, I32_MIN))  # the largest row
    digits = [0] + [s * j for j in range(1, COMB_ROWS) for s in (1, -1)]
    rng.shuffle(digits)
    top = COMB_ROWS - 1
    assert len(rows) == COMB_ROWS and all(len(r) == 32 for r in rows)
    assert {0, top, -top} <= set(digits) and len(digits) % 16 != 0
    assert I32_MIN in rows[top][20:30] and any(I32_MIN in rows[-d][20:30] for d in digits if d < 0)
    return tuple(rows), tuple(digits)


def comb_take_expected(row, dg):
    """Lanes (YmX, YpX, XY2d, 2) of the row, or (YpX, YmX, -XY2d, 2) for a negative digit."""
    ypx, ymx, xy2d = row[0:10], row[10:20], row[20:30]
    two = (2,) + (0,) * 9
    if dg < 0:
        return [ypx, ymx, tuple(wrap_neg32(x) for x in xy2d), two]
    return [ymx, ypx, xy2d, two]


# ---- c. real points -----------------------------------------------------------------------------
def split_limbs(x, centered=False):
    """The integer x (negative allowed) as carried limbs of value exactly x: even limbs rounded into
    [-2^25, 2^25), odd limbs floored into [0, 2^25) or, centered, rounded into [-2^24, 2^24) as
    fe_carry leaves them; limb 9 takes what is left.  None if that does not fit the carried range."""
    out, rest = [], x
    for i in range(9):
        w = 25 if i % 2 else 26
        if i % 2 == 0 or centered:
            limb = ((rest + (1 << (w - 1))) % (1 << w)) - (1 << (w - 1))
        else:
            limb = rest % (1 << w)
        out.append(limb)
        rest = (rest - limb) >> w
    out.append(rest)
    out = tuple(out)
    assert val(out) == x
    return out if PC.is_carried(out) else None


def fe_rep(x, rng):
    """Carried limbs of some integer congruent to x mod p: x, x + p, x + 2p, x - p, whichever fit,
    with floored or centered odd limbs."""
    x %= P
    reps = [r for r in (split_limbs(x + k * P, c) for k in (0, 1, 2, -1) for c in (False, True)) if r is not None]
    assert reps, hex(x)
    return rng.choice(reps)


def point_rep(pt, rng, scale=True):
    """(X, Y, Z, T) of pt as four carried limb vectors, every coordinate scaled by one random
    lambda (so Z != 1) unless scale is False."""
    lam = rng.randrange(1, P) if scale else 1
    return tuple(fe_rep(c * lam, rng) for c in pt)


def cached_of(rep, neg=False):
    """ge_cached fields (Y+X, Y-X, Z, 2dT) of a point given as limbs: the sums limb by limb."""
    X, Y, Z, T = rep
    rng = random.Random(val(T) % 2**32)
    ypx, ymx, t2d = limb_add(Y, X), limb_sub(Y, X), fe_rep(D2 * val(T), rng)
    return (ymx, ypx, Z, scaled(-1, t2d)) if neg else (ypx, ymx, Z, t2d)


def quad_cached_of(rep, neg=False):
    """quad.h's cached lanes (Y-X, Y+X, 2dT, 2Z); for -Q the first two exchanged, 2dT negated."""
    ypx, ymx, Z, t2d = cached_of(rep, neg)
    return (ymx, ypx, t2d, scaled(2, Z))


def affine(pt):
    x, y, z, _ = pt
    zi = pow(z, P - 2, P)
    return x * zi % P, y * zi % P


def niels_of(pt, rng):
    x, y = affine(pt)
    if rng.random() < 0.5:  # the sums limb by limb (2-sums), or carried representatives
        X, Y = fe_rep(x, rng), fe_rep(y, rng)
        return (limb_add(Y, X), limb_sub(Y, X), fe_rep(D2 * x * y, rng))
    return (fe_rep(y + x, rng), fe_rep(y - x, rng), fe_rep(D2 * x * y, rng))


@functools.lru_cache(maxsize=None)
def real_points():
    """(points, number of small-order ones in front): the 8 points of order dividing 8 (the identity
    first), BASE, torsion + prime-order sums, random multiples of BASE and random decoded points."""
    rng = random.Random(4001)
    small = list(E.small_order_points())
    assert len(small) == 8 and E.pt_equal(small[0], E.IDENTITY)
    pts = small + [E.BASE]
    pts += [E.pt_add(E.pt_mul(rng.randrange(1, E.L), E.BASE), t) for t in small[1:]]
    pts += [E.pt_mul(rng.randrange(1, E.L), E.BASE) for _ in range(8)]
    while len(pts) < 32:
        q = E.decode(rng.randbytes(32))
        if q is not None:
            pts.append(q)
    return tuple(pts), len(small)


@functools.lru_cache(maxsize=None)
def point_pairs():
    """(P, Q) pairs: every point with itself (P + P through the addition formula), with its
    negative, with the identity on either side; small-order + large both ways; random pairs."""
    pts, ns = real_points()
    rng = random.Random(4002)
    ident = pts[0]
    pairs = []
    for p in pts:
        pairs += [(p, p), (p, E.pt_neg(p)), (ident, p), (p, ident)]
    for s in pts[1:ns]:
        for big in (pts[ns], pts[ns + 3], pts[-1]):
            pairs += [(s, big), (big, s)]
    pairs += [(rng.choice(pts), rng.choice(pts)) for _ in range(60)]
    eq = E.pt_equal
    assert any(eq(a, b) and not eq(a, ident) for a, b in pairs)
    assert any(eq(a, E.pt_neg(b)) and not eq(a, b) for a, b in pairs)
    assert any(eq(a, ident) and not eq(b, ident) for a, b in pairs) and any(eq(b, ident) and not eq(a, ident) for a, b in pairs)
    small, large = pts[1:ns], pts[ns:]
    assert any(any(eq(a, s) for s in small) and any(eq(b, g) for g in large) for a, b in pairs)
    return tuple(pairs)


def _p1p1_of_sum(p, q):
    """The completed point (E, H, G, F) of add-2008-hwcd-3: x = E/G, y = H/F."""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b, c, d = (y1 - x1) * (y2 - x2), (y1 + x1) * (y2 + x2), t1 * D2 * t2, 2 * z1 * z2
    return ((b - a) % P, (b + a) % P, (d + c) % P, (d - c) % P)


@functools.lru_cache(maxsize=None)
def ge_real_cases(op):
    """(neg, in[8], expected point) for one ge op on curve points in non-canonical limbs."""
    rng = random.Random(5000 + op)
    pts, _ = real_points()
    cases = []
    if op in (GE_P2_DBL, GE_P3_TO_CACHED, GE_CACHED_TO_P3, GE_P3_TO_NIELS):
        for rnd in range(3):
            for p in pts:
                rep = point_rep(p, rng, scale=rnd > 0)
                if op == GE_P2_DBL:
                    cases.append((0, _pad8(rep[:3]), E.pt_add(p, p)))
                elif op == GE_CACHED_TO_P3:
                    cases.append((0, _pad8(cached_of(rep)), p))
                else:
                    cases.append((0, _pad8(rep), p))
    else:
        for i, (p, q) in enumerate(point_pairs()):
            neg = i % 2 if op in GE_HAS_NEG else 0
            exp = E.pt_add(p, E.pt_neg(q) if neg else q)
            rp, rq = point_rep(p, rng, scale=i % 3 > 0), point_rep(q, rng, scale=i % 5 > 0)
            if op == GE_ADD_CACHED:
                ins = rp + cached_of(rq)
            elif op == GE_ADD_CACHED_PRE:  # the caller exchanges Y+X / Y-X when neg
                c = cached_of(rq)
                ins = rp + ((c[1], c[0], c[2], c[3]) if neg else c)
            elif op == GE_MADD_NIELS:
                ins = rp + niels_of(q, rng)
            elif op == GE_P3_ADD:
                ins = rp + rq
            else:  # the completed sum, every coordinate scaled alike
                lam = rng.randrange(1, P)
                ins = tuple(fe_rep(c * lam, rng) for c in _p1p1_of_sum(p, q))
            cases.append((neg, _pad8(ins), exp))
    while len(cases) % 64 == 0 or len(cases) <= 64:
        cases.append(cases[len(cases) // 2])
    if op in GE_HAS_NEG:
        assert {c[0] for c in cases} == {0, 1}
    assert sum(val(c) < 0 for _, ins, _ in cases for c in ins) > len(cases) // 4, op  # non-canonical limbs
    return tuple(cases)


def _nonzero(x, what):
    assert x % P != 0, what


def check_ge_real(op, neg, ins, exp, limbs, encs):
    """The assertions on one real-point case: the output is the expected group element."""
    what = (GE_NAMES[op], neg, ins)
    kinds = GE_OUT_RANGE[op]
    for k in range(4):
        if kinds[k] is None:
            continue
        assert val(limbs[k]) % P == encs[k], what + ("encoding", k)
        for i in range(10):
            assert limb_range_ok(kinds[k], i, limbs[k][i]), what + ("limb", k, i, limbs[k][i])
    X, Y, Z, T = encs
    if op in (GE_P2_DBL, GE_ADD_CACHED, GE_ADD_CACHED_PRE, GE_MADD_NIELS):  # p1p1: x = X/Z, y = Y/T
        _nonzero(Z * T, what)
        assert E.pt_equal((X * T % P, Y * Z % P, Z * T % P, X * Y % P), exp), what
    elif op == GE_P1P1_TO_P2:
        _nonzero(Z, what)
        assert E.pt_equal((X, Y, Z, 0), exp), what
    elif op in (GE_P1P1_TO_P3, GE_CACHED_TO_P3, GE_P3_ADD):
        _nonzero(Z, what)
        assert (T * Z - X * Y) % P == 0, what
        assert E.pt_equal((X, Y, Z, T), exp), what
    elif op == GE_P3_TO_CACHED:
        ypx, ymx, z, t2d = encs
        _nonzero(z, what)
        x2, y2 = (ypx - ymx) % P, (ypx + ymx) % P  # 2X, 2Y
        assert E.pt_equal((x2, y2, 2 * z % P, 0), exp), what
        assert (2 * t2d * 2 * z - D2 * x2 * y2) % P == 0, what
    else:  # niels: exactly the affine (y + x, y - x, 2dxy)
        x, y = affine(exp)
        assert (encs[0], encs[1], encs[2]) == ((y + x) % P, (y - x) % P, D2 * x * y % P), what


@functools.lru_cache(maxsize=None)
def quad_real_cases(op):
    """(v[4], q[4], expected point) per quad for quad_dbl, quad_add (+Q and -Q) and quad_to_cached
    on curve points."""
    rng = random.Random(6000 + op)
    pts, _ = real_points()
    z4 = (ZERO,) * 4
    cases = []
    if op in (Q_DBL, Q_TO_CACHED):
        for rnd in range(3):
            for p in pts:
                rep = point_rep(p, rng, scale=rnd > 0)
                cases.append((rep, z4, E.pt_add(p, p) if op == Q_DBL else p))
    else:
        for i, (p, q) in enumerate(point_pairs()):
            neg = i % 2 == 1
            rp, rq = point_rep(p, rng, scale=i % 3 > 0), point_rep(q, rng, scale=i % 5 > 0)
            cases.append((rp, quad_cached_of(rq, neg), E.pt_add(p, E.pt_neg(q) if neg else q)))
    while len(cases) % 16 == 0:
        cases.append(cases[len(cases) // 2])
    return tuple(cases)


def check_quad_real(op, v, q, exp, out):
    what = (Q_NAMES[op], v, q)
    c = [val(o) % P for o in out]
    if op == Q_TO_CACHED:  # lanes Y - X, Y + X, 2dT, 2Z
        _nonzero(c[3], what)
        x2, y2 = (c[1] - c[0]) % P, (c[1] + c[0]) % P
        assert E.pt_equal((x2, y2, c[3], 0), exp), what
        assert (2 * c[2] * c[3] - D2 * x2 * y2) % P == 0, what
        return
    check_extended(c, out, exp, what)


def check_extended(c, out, exp, what):
    """An extended output: Z != 0, T Z = X Y, the expected point, carried limbs."""
    X, Y, Z, T = c
    _nonzero(Z, what)
    assert (T * Z - X * Y) % P == 0, what
    assert E.pt_equal((X, Y, Z, T), exp), what
    for r in range(4):
        for i in range(10):
            assert PC.in_carried_output_range(i, out[r][i]), what + ("limb", r, i, out[r][i])


# ---- d. quad chains -----------------------------------------------------------------------------
CHAIN_STEPS = 16


def chain_step(ndbl, sel):
    """One step of a chain program: ndbl doublings, then + operand A (sel 1), + B (sel 2) or nothing."""
    assert 0 <= ndbl <= 16 and sel in (0, 1, 2)
    return ndbl | (sel << 8)


def chain_expected(a, b, steps):
    acc = E.IDENTITY
    through_identity = False
    for i, (ndbl, sel) in enumerate(steps):
        for _ in range(ndbl):
            acc = E.pt_add(acc, acc)
        if sel:
            acc = E.pt_add(acc, a if sel == 1 else b)
        if i > 0 and i + 1 < len(steps) and E.pt_equal(acc, E.IDENTITY):
            through_identity = True
    return acc, through_identity


@functools.lru_cache(maxsize=None)
def chain_cases():
    """(A lanes[4], B lanes[4], program[16], expected point): the accumulator starts as
    quad_identity; operand A is Q and B is -Q (exchanged / negated lanes), both cached lanes
    computed here.  Programs of 4 doublings and +-Q over up to 16 steps (the loop of
    verify_glat_main_kernel), of 16 doublings a step (zip_final_kernel), and programs whose
    accumulator passes through the identity: +Q then -Q, an order-8 point doubled three times, an
    order-4 point doubled twice, an order-2 point doubled once."""
    rng = random.Random(7001)
    pts, ns = real_points()
    order = lambda p: next(k for k in (1, 2, 4, 8) if E.pt_equal(E.pt_mul(k, p), E.IDENTITY))
    small = {k: [p for p in pts[:ns] if order(p) == k] for k in (2, 4, 8)}
    assert len(small[2]) == 1 and len(small[4]) == 2 and len(small[8]) == 4
    progs = []  # (point, steps)
    tail = lambda n: [(4, rng.choice((1, 2))) for _ in range(n)]
    for q in pts[ns:]:
        progs.append((q, [(0, 1)] + tail(15)))                # identity + Q first, then 15 windows
        progs.append((q, [(4, rng.choice((0, 1, 2))) for _ in range(rng.randrange(1, 17))]))
        progs.append((q, [(0, 1), (0, 2)] + tail(6)))         # +Q then -Q: through the identity
        progs.append((q, [(0, 2), (4, 0), (0, 1)] + [(16, rng.choice((1, 2))) for _ in range(3)]))
    for q in small[8]:
        progs.append((q, [(0, 1), (3, 0)] + tail(5)))         # order 8, doubled three times
        progs.append((q, [(0, 2), (3, 1), (4, 2)]))
    for q in small[4]:
        progs.append((q, [(0, 1), (2, 0)] + tail(4)))
    for q in small[2]:
        progs.append((q, [(0, 1), (1, 0), (0, 1), (0, 1)] + tail(3)))
    progs.append((pts[0], [(0, 1)] + tail(4)))                 # Q the identity itself
    progs.append((pts[ns], []))                                # the empty program: quad_identity out
    cases, n_through = [], 0
    for i, (q, steps) in enumerate(progs):
        rep = point_rep(q, rng, scale=i % 4 > 0)
        exp, through = chain_expected(q, E.pt_neg(q), steps)
        n_through += through
        prog = tuple(chain_step(*s) for s in steps) + (0,) * (CHAIN_STEPS - len(steps))
        assert len(prog) == CHAIN_STEPS
        cases.append((quad_cached_of(rep), quad_cached_of(rep, neg=True), prog, exp))
    assert n_through >= len(pts[ns:]) + 8, n_through  # +Q -Q per large point, the small-order programs
    assert any(len(s) == CHAIN_STEPS for _, s in progs)
    while len(cases) % 16 == 0:
        cases.append(cases[1])
    return tuple(cases)
