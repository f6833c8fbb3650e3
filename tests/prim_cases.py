"""Input cases for the kernels' building blocks (fe25519.h / fe_cols.h, sc25519.h, sha512.h,
verify_hs.h, ge25519.h), shared by the CPU suite (tests/test_kernel_host.py, the host build of
that source) and the GPU suite (tests/test_gpu_primitives.py, the device build): limb extremes,
values near p and L, boundary scalars.  Every generator is deterministic (fixed seeds) and cached;
callers must not modify what they get.

Expected values are not kept here: both suites compute them with Python integers, hashlib and
oracle.ed25519_go."""
import functools
import random

from oracle import ed25519_go as E

P = E.P
L = E.L
N8 = 8 * L

# bit offset of limb i (radix 2^25.5)
OFF = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)


def limb_val(c):
    return sum(x << o for x, o in zip(c, OFF))


# ---- field: raw limbs -------------------------------------------------------------------------
# The carried limb ranges (fe25519.h): even limbs [-2^25, 2^25), odd [0, 2^25) from the products
# and [-2^24, 2^24] from fe_carry, limb 1 [-2^16, 2^25 + 2^16) widened by fe_carry's range.
CARRIED_LO = tuple(-(2**24) - 2**16 if i == 1 else (-(2**25) if i % 2 == 0 else -(2**24)) for i in range(10))
CARRIED_HI = tuple(2**25 + 2**16 if i == 1 else 2**25 - 1 for i in range(10))
# the larger end, either sign: what one term of a sum or DIFFERENCE of carried values can reach
CARRIED_MAG = tuple(max(-lo, hi) for lo, hi in zip(CARRIED_LO, CARRIED_HI))

# fe_raw operation numbers (hostsim_fe_raw, devprim_fe_raw)
FE_MUL, FE_SQ, FE_SQ2, FE_SQC, FE_MUL_X2, FE_SQ_X2, FE_SQC_X2, FE_SQ2_SQ = range(8)
FE_RAW_NAMES = ("fe_mul", "fe_sq", "fe_sq2", "fe_sqc", "fe_mul_x2", "fe_sq_x2", "fe_sqc_x2", "fe_sq2_sq")


def is_carried(c):
    return all(CARRIED_LO[i] <= c[i] <= CARRIED_HI[i] for i in range(10))


def in_carried_output_range(i, v):
    """The limb-range assertion on every product's output."""
    return CARRIED_LO[i] <= v <= CARRIED_HI[i] or (i % 2 == 1 and 0 <= v < 2**25)


def draw_carried(rng):
    """One carried value; 30 % of the draws sit at the ends of every limb's range."""
    lo, hi = CARRIED_LO, CARRIED_HI
    r = rng.random()
    if r < 0.3:
        return tuple(lo[i] if rng.random() < 0.5 else hi[i] for i in range(10))
    return tuple(rng.randint(lo[i], hi[i]) for i in range(10))


def draw_nsum(rng, n, signed=False):
    """A sum of n carried values, limb by limb; signed: each summand added or subtracted."""
    cs = [draw_carried(rng) for _ in range(n)]
    if signed:
        cs = [c if rng.random() < 0.5 else tuple(-v for v in c) for c in cs]
    return tuple(sum(c[i] for c in cs) for i in range(10))


@functools.lru_cache(maxsize=None)
def _fused():
    lo, hi = CARRIED_LO, CARRIED_HI
    rng = random.Random(23)

    def carried():
        return draw_carried(rng)

    def nsum(n):
        return draw_nsum(rng, n)

    hi3, lo3 = tuple(3 * v for v in hi), tuple(3 * v for v in lo)
    pairs = [(hi3, hi3), (lo3, lo3), (hi3, lo3)]
    pairs += [(nsum(3), nsum(3)) for _ in range(600)] + [(nsum(1), nsum(2)) for _ in range(300)]
    singles = [carried() for _ in range(400)]
    return tuple(pairs), tuple(singles)


def fused_pairs():
    """903 (a, b) operand pairs, each a sum of up to three carried values: the three all-extreme
    pairs, 600 (3-sum, 3-sum), 300 (1-sum, 2-sum); 30 % of the summands sit at the ends of every
    limb's range."""
    return _fused()[0]


def fused_carried():
    """The carried operands (one carried value, not a sum): both all-extreme values, the 400 of the
    original fe_sq2 loop and the 1-sums among fused_pairs()."""
    pairs, singles = _fused()
    return (CARRIED_LO, CARRIED_HI) + singles + tuple(a for a, _ in pairs if is_carried(a))


@functools.lru_cache(maxsize=None)
def fused_4sum_pairs():
    """316 (f, g) pairs for fe_mul with a 4-sum as its FIRST operand (fe25519.h: f takes x2 copies
    only, so it may be a sum of four carried values; quad.h's doubling passes F = B - A - 2C so):
    the all-extreme pairs (4 hi, 3 hi), (4 lo, 3 lo), both crossed, and the same four against a
    2-sum; F is a DIFFERENCE, so also -+4 x the larger end against -+3 x and -+2 x it; then 200
    (4-sum, 3-sum) and 100 (4-sum, 2-sum) draws of draw_nsum, every other one with signed summands."""
    lo, hi, mag = CARRIED_LO, CARRIED_HI, CARRIED_MAG
    rng = random.Random(47)
    mul = lambda k, c: tuple(k * v for v in c)
    pairs = [(mul(4, a), mul(k, b)) for k in (3, 2) for a, b in ((hi, hi), (lo, lo), (hi, lo), (lo, hi))]
    pairs += [(mul(4 * sa, mag), mul(k * sb, mag)) for k in (3, 2) for sa in (1, -1) for sb in (1, -1)]
    pairs += [(draw_nsum(rng, 4, j % 2 == 1), draw_nsum(rng, 3, j % 2 == 1)) for j in range(200)]
    pairs += [(draw_nsum(rng, 4, j % 2 == 1), draw_nsum(rng, 2, j % 2 == 1)) for j in range(100)]
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def fused_pair_sets():
    """(a0, b0, a1, b1) for the two-product schedules, 3-sum operands: every pair of fused_pairs()
    beside the pair 7 places on, one set all-low beside the other all-high (both ways, and crossed),
    and both sets equal (the extremes and every 9th pair)."""
    pairs = fused_pairs()
    n = len(pairs)
    hi3, lo3 = pairs[0][0], pairs[1][0]
    out = [(lo3, lo3, hi3, hi3), (hi3, hi3, lo3, lo3), (hi3, lo3, lo3, hi3), (lo3, hi3, hi3, lo3)]
    out += [(a, b, a, b) for a, b in pairs[:3] + pairs[3::9]]
    out += [pairs[i] + pairs[(i + 7) % n] for i in range(n)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def carried_pair_sets():
    """(a0, a1) carried operands for fe_sqc_x2 and the first operand of fe_sq2_sq: all-low beside
    all-high (both ways), equal sets, and every carried operand beside the one 5 places on."""
    c = fused_carried()
    n = len(c)
    out = [(CARRIED_LO, CARRIED_HI), (CARRIED_HI, CARRIED_LO), (CARRIED_LO, CARRIED_LO), (CARRIED_HI, CARRIED_HI)]
    out += [(a, a) for a in c[2::11]]
    out += [(c[i], c[(i + 5) % n]) for i in range(n)]
    return tuple(out)


# ---- field: 32-byte encodings -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_byte_pairs():
    """(a, b) integers below 2^255 for the ops of hostsim_fe_op / devprim_fe_bytes: 133 values
    (edges near 0, p and 2^255, 120 random) against 7 (6 edges and one random each)."""
    rng = random.Random(11)
    edge = [0, 1, 2, 19, P - 1, P, P + 1, P + 18, 2**255 - 1, 2**255 - 20, 2**254, 2**26 - 1, 2**51]
    vals = edge + [rng.randrange(2**255) for _ in range(120)]
    out = []
    for a in vals:
        for b in edge[:6] + [rng.randrange(2**255)]:
            out.append((a, b))
    return tuple(out)


def field_byte_expected(a, b):
    """op -> expected value for the ten ops of hostsim_fe_op."""
    A, B = a % P, b % P
    return {0: A * B % P, 1: A * A % P, 2: pow(A, P - 2, P), 3: pow(A, (P - 5) // 8, P), 4: (A + B) % P,
            5: (A - B) % P, 6: 2 * A * A % P, 7: (2 * A + B) ** 2 % P, 8: (2 * A + B) ** 2 % P,
            9: pow(A, P - 2, P)}


@functools.lru_cache(maxsize=None)
def bgcd_values():
    """Inputs of fe_invert_bgcd: random values of every bit length, powers of two and their
    neighbours, values near p and 0."""
    rng = random.Random(23)
    vals = [0, 1, 2, 3, P - 1, P - 2, P, P + 1, 2**255 - 1, 2**254, 2**64, 2**64 - 1, 2**30, 2**30 - 1, 2**60 + 1]
    vals += [2**rng.randrange(255) for _ in range(60)] + [(2**rng.randrange(255)) - 1 for _ in range(60)]
    vals += [rng.randrange(2**rng.randrange(1, 256)) for _ in range(400)] + [P - rng.randrange(2**40) for _ in range(40)]
    return tuple(vals)


# ---- fe_pack256 / fe_unpack256 ------------------------------------------------------------------
# carried ranges (fe_carry64): even [-2^25, 2^25), odd [-2^24, 2^24), limbs 1 and 5 one wider
PACK_LO = tuple((-(2**25) if i % 2 == 0 else -(2**24)) - (1 if i in (1, 5) else 0) for i in range(10))
PACK_HI = tuple((2**25 - 1 if i % 2 == 0 else 2**24 - 1) + (1 if i in (1, 5) else 0) for i in range(10))


@functools.lru_cache(maxsize=None)
def pack256_cases():
    """(cases, g): 2-sums of carried values at the ends of their limb ranges (all-low, all-high,
    alternating, one limb at an extreme, 800 random) and the carried multiplier g."""
    lo, hi = PACK_LO, PACK_HI
    rng = random.Random(5)
    cases = [[2 * lo[i] for i in range(10)], [2 * hi[i] for i in range(10)], [0] * 10,
             [2 * lo[i] if i % 2 else 2 * hi[i] for i in range(10)], [2 * hi[i] if i % 2 else 2 * lo[i] for i in range(10)]]
    for i in range(10):
        for v in (2 * lo[i], 2 * hi[i]):
            c = [0] * 10
            c[i] = v
            cases.append(c)
    cases += [[rng.randint(2 * lo[i], 2 * hi[i]) for i in range(10)] for _ in range(800)]
    g = rng.randrange(P)
    return tuple(tuple(c) for c in cases), g


def check_pack256(c, u, prod, g):
    """The assertions on one pack256 case: unpacked limbs u, product with g (integer)."""
    val = limb_val(c)
    for i in range(9):
        assert 0 <= u[i] < (2**25 if i % 2 else 2**26), (c, u)
    assert -2 <= u[9] <= 2**25, (c, u)
    assert limb_val(u) % P == val % P, (c, u)
    assert prod == val * g % P, (c, u)


# ---- SHA-512 and scalars ------------------------------------------------------------------------
SHA512_LENS = (0, 1, 17, 111, 112, 113, 127, 128, 129, 200, 239, 240, 241, 300, 400)


@functools.lru_cache(maxsize=None)
def sha512_messages():
    rng = random.Random(5)
    return tuple(bytes(rng.randrange(256) for _ in range(n)) for n in SHA512_LENS)


@functools.lru_cache(maxsize=None)
def sha512_stream_cases():
    """(p0, p1, buffer, offsets, lengths): messages of every length 0..300 and the lengths of
    SHA512_LENS at each of the four dword misalignments, laid end to end in one buffer (gaps of
    0..3 bytes set the start's misalignment), and two 32-byte prefixes per message."""
    rng = random.Random(41)
    lens = [(n, r) for n in SHA512_LENS for r in range(4)] + [(n, n % 4) for n in range(301)]
    lens += [(n, (n + 1 + n // 4) % 4) for n in range(0, 301, 3)]
    buf, offs, ls = bytearray(), [], []
    for n, r in lens:
        while len(buf) % 4 != r:
            buf.append(rng.randrange(256))
        offs.append(len(buf))
        ls.append(n)
        buf += rng.randbytes(n)
    k = len(lens)
    p0 = tuple(rng.randbytes(32) for _ in range(k))
    p1 = tuple(rng.randbytes(32) for _ in range(k))
    return p0, p1, bytes(buf), tuple(offs), tuple(ls)


SC_REDUCE_EXTREMES = (b"\xff" * 64, bytes(64), L.to_bytes(64, "little"), (L - 1).to_bytes(64, "little"),
                      (2 * L).to_bytes(64, "little"), (L * (2**259 - 1)).to_bytes(64, "little"))


@functools.lru_cache(maxsize=None)
def sc_reduce_values():
    """512-bit integers for sc_reduce512: the digests of sha512_messages() and the extremes; for
    the Barrett step (q at most one below floor(x / L)) m L - 1, m L, m L + 1 for 200 random m and
    for the largest m with m L < 2^512, and 2^512 - 1; random values of every word length."""
    import hashlib
    rng = random.Random(29)
    top = 2**512
    vals = [int.from_bytes(hashlib.sha512(m).digest(), "little") for m in sha512_messages()]
    vals += [int.from_bytes(x, "little") for x in SC_REDUCE_EXTREMES]
    mmax = (top - 1) // L
    ms = []
    while len(ms) < 200:
        m = rng.randrange(1, mmax + 1) >> rng.choice((0, 0, 0, 64, 128, 200, 255))
        if m >= 1 and m * L + 1 < top:
            ms.append(m)
    for m in ms + [mmax]:
        vals += [x for x in (m * L - 1, m * L, m * L + 1) if x < top]
    vals.append(top - 1)
    vals += [rng.randrange(2**(32 * w)) for w in range(1, 17) for _ in range(8)]
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def sc_canonical_values():
    """256-bit values around L and at the word boundaries of the comparison's borrow chain."""
    rng = random.Random(31)
    vals = [0, 1, L - 2, L - 1, L, L + 1, 2 * L, 2**252, 2**252 - 1, 2**253, 2**255, 2**256 - 1, L + 2**128,
            L - 2**128, L ^ 1, L - 2**32, L + 2**32, (L >> 32) << 32, L | 0xffffffff]
    for w in range(8):
        vals += [(L + (1 << (32 * w))) % 2**256, L - (1 << (32 * w)), L & ~(0xffffffff << (32 * w))]
    vals += [rng.randrange(2**256) for _ in range(60)] + [rng.randrange(L) for _ in range(60)]
    vals += [L + rng.randrange(2**rng.randrange(1, 250)) for _ in range(40)]
    vals += [L - rng.randrange(2**rng.randrange(1, 250)) for _ in range(40)]
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def sc_muladd_cases():
    """(a, b, c) below 2^256 (the signer passes a clamped 2^254-range scalar and reduced k, r):
    all-ones words (every carry of the row chains), L and its neighbours, zero, random."""
    rng = random.Random(37)
    M = 2**256 - 1
    edge = [0, 1, L - 1, L, L + 1, M, 2**255, 2**252, 0xffffffff, M ^ 0xffffffff, 2**128 - 1, M ^ (2**128 - 1)]
    out = [(a, b, c) for a in edge for b in edge for c in (0, L - 1, M)]
    out += [(rng.randrange(2**256), rng.randrange(2**256), rng.randrange(2**256)) for _ in range(200)]
    out += [(rng.randrange(L), rng.randrange(L), rng.randrange(L)) for _ in range(211)]
    return tuple(out)


# ---- sc_halfsize ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def halfsize_lattice_ks():
    """(ks, number of leading boundary values): the rest are random k < L."""
    rng = random.Random(3)
    ks = [0, 1, 2, 3, 8, 16, L - 1, L - 2, 2**127, 2**128 - 1, 2**128, 2**200, 2**252 - 1, 5 * 2**128 + 3]
    n_edge = len(ks)
    ks += [rng.randrange(L) for _ in range(4000)]
    return tuple(ks), n_edge


@functools.lru_cache(maxsize=None)
def halfsize_euclid_ks():
    rng = random.Random(11)
    ks = [0, 1, 2, 3, 8, 16, L - 1, L - 2, 2**127, 2**128 - 1, 2**128, 2**128 + 1, 2**160, 2**200,
          2**252 - 1, 5 * 2**128 + 3, N8 // 3, N8 // 5 + 1]
    ks += [rng.randrange(L) for _ in range(6000)]
    ks += [rng.randrange(2**129) for _ in range(300)] + [rng.randrange(2**170) for _ in range(300)]
    return tuple(ks)


def euclid_quotients(k, n=N8):
    """Partial quotients of n / k (the quotients of the Euclid steps sc_halfsize runs from (8L, k))."""
    out = []
    a, b = n, k
    while b:
        out.append(a // b)
        a, b = b, a % b
    return out


@functools.lru_cache(maxsize=None)
def halfsize_quotient_ks():
    """k with a borderline first quotient floor(8L / k): k = floor(8L / q) + {-1, 0, 1} for q around
    the quotient limit of hs_euclid_step (2^32 - 2) and small q, and k = floor((8L - r) / q), whose
    first remainder is tiny (the second quotient is then out of range, or the cofactor even): these
    hit the 4294967294.0 limit, the even-cofactor adjustment and the (k, 1) fallback.  0 < k < L."""
    ks = []
    for q in (8, 9, 10, 2**16, 2**31, 2**32 - 3, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**33):
        ks += [N8 // q + e for e in (-1, 0, 1)]
    for r in (1, 2, 3, 2**20, 2**31):
        for q in (9, 1000):
            ks.append((N8 - r) // q)
    return tuple(k for k in ks if 0 < k < L)


LONG_EUCLID_MIN = 40


@functools.lru_cache(maxsize=None)
def halfsize_long_euclid_ks():
    """300 values of k with long Euclid runs: the continued fraction of 8L / k is
    [a1; a2, ..., a_{m+1}, ...] with m >= 40 partial quotients a2.. in {1, 2} after the first (k < L
    forces a1 = floor(8L / k) >= 8, so the run of small quotients starts at the second step).  Built
    backwards from the chosen quotients: every real between the convergents of [a1; ..., a_{m+1}]
    and [a1; ..., a_{m+1} + 1] has that prefix, so k is drawn between 8L divided by each; the
    prefix is then checked on the integers."""
    rng = random.Random(43)
    ks = []
    while len(ks) < 300:
        i = len(ks)
        m = LONG_EUCLID_MIN + (i % 40)            # up to 79: the interval below stays > 2^14 wide
        if i % 3 == 0:
            small = [1] * m                       # the slowest remainder sequence
        elif i % 3 == 1:
            small = [2] * m
        else:
            small = [rng.choice((1, 2)) for _ in range(m)]
        cf = [rng.choice((8, 9, 10, 11, 16, 100, 2**20))] + small

        def conv(q):
            h0, h1, k0, k1 = 1, q[0], 0, 1
            for a in q[1:]:
                h0, h1, k0, k1 = h1, a * h1 + h0, k1, a * k1 + k0
            return h1, k1

        p1, q1 = conv(cf)
        p2, q2 = conv(cf[:-1] + [cf[-1] + 1])
        lo, hi = sorted((N8 * q1 // p1, N8 * q2 // p2))
        if hi - lo < 4:
            continue
        k = rng.randrange(lo + 1, hi)
        got = euclid_quotients(k)
        if not (0 < k < L and got[:len(cf)] == cf):
            continue
        ks.append(k)
    return tuple(ks)


def halfsize_edge_ks():
    """The boundary families added for the device comparison (also run on the host build)."""
    return halfsize_quotient_ks() + halfsize_long_euclid_ks()


def check_halfsize(k, c, d, W):
    """The invariants of sc_halfsize on one k: c = d k (mod 8L), d odd, 0 < |d| < L, both inside the
    window count's range, and W = 64 only for the (k, 1) fallback."""
    assert (c - d * k) % N8 == 0, k
    assert d % 2 == 1 and 0 < abs(d) < L, k
    assert 29 <= W <= 64 and max(c.bit_length(), abs(d).bit_length()) <= 4 * W - 1, (k, W)
    if W == 64:
        assert (c, d) == (k, 1), k


# ---- point decoding -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_candidates():
    rng = random.Random(9)
    cands = [bytes(32), bytes(31) + b"\x80"] + [rng.randbytes(32) for _ in range(80)]
    cands += [E.encode(q) for q in E.small_order_points()]
    cands += [(y + P).to_bytes(32, "little") for y in range(19)]
    return tuple(cands)
