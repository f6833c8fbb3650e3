"""Signatures for the half-size kernels at a chosen k (tests/test_hs_k_host.py, tests/test_gpu_hs_k.py).

Every generic verification runs through sc_halfsize (csrc/verify_hs.h): k = H(R || A || M) mod L
becomes a short pair (c, d) and a window count W, and the recoded digits, the top digit, the sign of
d, e = d S mod L, the W-sorted placement and the wave's loop length all follow from it.  No signature
chooses k.  tmed_test_verify_k (and its host twin, hostsim_verify_hs_k) takes k beside the signature,
so the cases here choose it: a case is (pub, sig, k) over the empty message.

The expected bit restates oracle.ed25519_go.verify with k given in place of hram — S canonical,
A = decode(pub), encode([S]B - [k]A) == sig[:32] — and oracle.zip215.verify likewise.  Nothing else
decides a case: neither the host build nor the device.

Construction: A (ordinary, A0 + T with T of order 2, 4 or 8, or the identity), S, and
R = [S]B - [k]A, which is valid.  Rejects: R + T' (T' of order 2, 4, 8: the cofactorless rule
rejects, ZIP-215 accepts; the case a d made even, or a congruence that held only mod L, would
accept), S + 1, one flipped bit of R, k +- 1 under the same R and S.

Families:
  a  the k of prim_cases' chosen-k families (quotients at the 2^32 - 2 limit, tiny first remainders,
     the even-cofactor adjustment, the (k, 1) fallback, long runs of quotients 1 and 2, boundaries).
  b  targeted (c, d): digits chosen, k = c / d mod 8L redrawn until k < L and until the host build's
     sc_halfsize returns exactly that pair (coverage is counted on what it returns, at its W).
  c  chosen e: S = +-e / |d| mod L for a k of family b, so the B additions see e's radix-2^26 edges.

Digit models (restated from the header comments of verify_hs.h, as tests/test_gpu_lds_rows.py does):
sc_recode16 adds 8 to every nibble (x + 0x88..88) and reads nibble - 8, so a regular digit lies in
[-8, 7]; the top window (W - 1) takes the carry into nibble W as + 16, so it lies in [0, 16].  A
digit D splits as 4h + l with l in [-2, 1]; the joint row of a sub-step is 5 i + j for the pair
(i, j) of c's and d's parts.
"""
from __future__ import annotations

import ctypes
import functools
import math
import random

import numpy as np

import prim_cases as PC
import scalar_edge_cases as SC
from oracle import ed25519_go as E

L = E.L
N8 = 8 * L
BIAS = int("88" * 32, 16)


# ------------------------------------------------------------------ expected bits
@functools.lru_cache(maxsize=None)
def _sb_minus_ka(pub: bytes, s: int, k: int):
    """[S]B - [k]A, or None when A does not decode."""
    a = E.decode(pub)
    if a is None:
        return None
    return E.pt_add(E.pt_mul(k, E.pt_neg(a)), E.pt_mul(s, E.BASE))


def expect_go(pub: bytes, sig: bytes, k: int) -> bool:
    """oracle.ed25519_go.verify with k in place of hram(R, A, M)."""
    if len(sig) != 64 or sig[63] & 0xE0:
        return False
    s = E.sc_canonical(sig[32:])
    if s is None:
        return False
    r = _sb_minus_ka(pub, s, k)
    return r is not None and E.encode(r) == sig[:32]


def expect_zip215(pub: bytes, sig: bytes, k: int) -> bool:
    """oracle.zip215.verify with k in place of hram(R, A, M)."""
    if len(sig) != 64:
        return False
    r = E.decode(sig[:32])
    s = E.sc_canonical(sig[32:])
    if r is None or s is None:
        return False
    q = _sb_minus_ka(pub, s, k)
    if q is None:
        return False
    return E.pt_equal(E.pt_mul(8, E.pt_add(q, E.pt_neg(r))), E.IDENTITY)


# ------------------------------------------------------------------ the lattice step, modelled
def _to_double(x: int, words: int) -> float:
    """words_to_double: the words from the top, r = r * 2^32 + word, each step rounded."""
    r = 0.0
    for i in range(words - 1, -1, -1):
        r = r * 4294967296.0 + float((x >> (32 * i)) & 0xffffffff)
    return r


def model_halfsize(k: int):
    """(c, d, tight W, fallback) after the header comment of verify_hs.h: Euclid on (8L, k) to the
    first remainder below 2^128 with its cofactor; an even cofactor is replaced by the balanced
    combination with the previous pair; quotients are fp64 estimates corrected to the exact floor,
    and a step whose estimate reaches 2^32 - 2 falls back to (k, 1) with W = 64.  The estimates are
    IEEE doubles here as in the host build, so the fallback set is the host build's exactly."""
    a, b, ta, tb = N8, k, 0, 1
    fa, fb = _to_double(a, 8), _to_double(b, 8)
    sign = 1  # of tb: t_1 = +1, alternating
    while b >> 128:
        qd = float(math.floor(fa / fb))
        if not qd < 4294967294.0:
            return k, 1, 64, True
        q = int(qd)
        r = a - q * b
        if r < 0:
            q, r = q - 1, r + b
        elif r >= b:
            q, r = q + 1, r - b
        if not 0 <= r < b:
            return k, 1, 64, True
        a, b, ta, tb = b, r, tb, ta + q * tb
        fa, fb = fb, _to_double(b, 8)
        sign = -sign
    if tb % 2 == 0:
        fta, ftb = _to_double(ta, 5), _to_double(tb, 5)
        qmax = float(math.floor(fa / fb))
        if not qmax < 4294967294.0:
            return k, 1, 64, True
        j0 = float(math.floor((fa - fta) / (fb + ftb)))
        j0 = min(max(j0, 0.0), qmax)
        j1 = min(j0 + 1.0, qmax)
        m0, m1 = max(fa - j0 * fb, fta + j0 * ftb), max(fa - j1 * fb, fta + j1 * ftb)
        j = int(j1 if m1 < m0 else j0)
        if a - j * b < 0:
            return k, 1, 64, True
        b, tb, sign = a - j * b, ta + j * tb, -sign
    bits = max(b.bit_length(), tb.bit_length())
    return b, sign * tb, max(29, (bits + 3) // 4), False


def host_halfsize(hostsim, k: int):
    """(c, d signed, tight W) of the host build's sc_halfsize."""
    c32, d32 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    dneg, tight = ctypes.c_int(0), ctypes.c_int(0)
    hostsim.hostsim_halfsize_tight(k.to_bytes(32, "little"), c32, d32, ctypes.byref(dneg), ctypes.byref(tight), 1)
    d = int.from_bytes(d32.raw, "little")
    return int.from_bytes(c32.raw, "little"), -d if dneg.value else d, tight.value


# ------------------------------------------------------------------ digits and targets
def digits16(x: int, W: int) -> list[int]:
    """The W signed radix-16 digits hs_straus_joint reads of x: sc_recode16, the top one with the
    carry into nibble W (hs_top_digit; none at W = 64)."""
    r = x + BIAS
    d = [((r >> (4 * i)) & 15) - 8 for i in range(W)]
    if W < 64:
        d[W - 1] += 16 * ((r >> (4 * W)) & 1)
    return d


def split4(D: int) -> tuple[int, int]:
    lo = ((D + 2) & 3) - 2
    return (D - lo) >> 2, lo


def from_digits(ds: list[int]) -> int:
    return sum(d << (4 * i) for i, d in enumerate(ds))


POSITIONS = ("top", "below", "zero")  # windows W - 1, W - 2 and 0
RUN = 8  # a run: eight consecutive regular windows (a whole recoded word's worth) at one digit


def targets_of(c: int, d: int, W: int) -> set:
    """The named targets the pair (c, d) passes through when its sum runs over its own W windows."""
    dc, dd = digits16(c, W), digits16(abs(d), W)
    hit = {("W", W), ("dneg", int(d < 0))}
    tc, td = dc[W - 1], dd[W - 1]
    if W < 64:
        if tc >= 9:
            hit.add(("top_c", tc))
        if td >= 9:
            hit.add(("top_d", td))
        if tc == 16 and td == 16:
            hit.add(("top_both", 16))
        for name, t in (("tophi_c", tc), ("tophi_d", td)):
            if split4(t)[0] >= 3:
                hit.add((name, split4(t)[0]))
    for pos, n in (("top", W - 1), ("below", W - 2), ("zero", 0)):
        (hc, lc), (hd, ld) = split4(dc[n]), split4(dd[n])
        hit.add((pos, "h", hc, hd))
        hit.add((pos, "l", lc, ld))
    for name, ds in (("run_c", dc), ("run_d", dd)):
        for v in (-8, 7):
            if any(all(x == v for x in ds[i:i + RUN]) for i in range(0, W - RUN)):
                hit.add((name, v))
    return hit


W_TARGETS = (29, 30, 31, 32, 33, 34)


def named_targets() -> tuple[set, dict]:
    """(wanted, unreachable): every named target of family b, and those no pair can reach, each with
    the reason, derived here and not taken from the builder.

    * a regular digit is nibble - 8, in [-8, 7]: +8 never occurs, so a run of +8 does not (the
      largest regular digit, 7, stands in: run_c / run_d at 7);
    * d is odd, so its window-0 digit is odd and its low radix-4 part there is -1 or 1: the eight
      window-0 low pairs with l_d in (-2, 0) do not occur;
    * the top window's digits lie in [0, 16], so their high parts lie in [0, 4] (and in [-2, 2]
      everywhere else)."""
    want = {("W", w) for w in W_TARGETS} | {("dneg", 0), ("dneg", 1), ("top_both", 16)}
    want |= {(n, v) for n in ("top_c", "top_d") for v in range(9, 17)}
    want |= {(n, v) for n in ("tophi_c", "tophi_d") for v in (3, 4)}
    want |= {(n, v) for n in ("run_c", "run_d") for v in (-8, 7)}
    unreachable = {}
    for n in ("run_c", "run_d"):
        unreachable[(n, 8)] = "a regular digit is nibble - 8 <= 7"
    for pos in POSITIONS:
        hs = range(0, 5) if pos == "top" else range(-2, 3)
        want |= {(pos, "h", i, j) for i in hs for j in hs}
        for i in range(-2, 2):
            for j in range(-2, 2):
                if pos == "zero" and j % 2 == 0:
                    unreachable[(pos, "l", i, j)] = "d is odd: its window-0 digit is odd"
                else:
                    want.add((pos, "l", i, j))
    return want, unreachable


# ------------------------------------------------------------------ family b: targeted (c, d)
def _pair_for(target, rng: random.Random):
    """A candidate (c, |d|) whose digits at its intended W put `target` where it belongs, random
    elsewhere; the intended W is what the pair's longer scalar needs when nothing goes wrong."""
    kind = target[0]
    W = rng.choice((30, 31, 31, 32)) if kind != "W" else target[1]
    if kind in ("top_both",):
        W = rng.choice((30, 31))  # both scalars just under 2^(4W): |d| <= 2^127 keeps W <= 31
    if kind == "W" and W == 29:
        # lengths <= 116 bits: every such pair is clamped to 29 windows
        c, d = rng.getrandbits(rng.randrange(90, 117)), rng.getrandbits(rng.randrange(60, 117)) | 1
        return c, d
    dc = [rng.randrange(-8, 8) for _ in range(W)]
    dd = [rng.randrange(-8, 8) for _ in range(W)]
    dc[W - 1], dd[W - 1] = rng.randrange(1, 9), rng.randrange(0, 9)
    if rng.random() < 0.5:
        dc[W - 1], dd[W - 1] = dd[W - 1], dc[W - 1]
    if W == 32:
        dd[W - 1] = min(dd[W - 1], 7)  # |d| <= 2^127: the cofactor of the first remainder below 2^128
    if kind in ("top_c", "top_d", "tophi_c", "tophi_d"):
        v = target[1] if kind.startswith("top_") else rng.choice({3: (10, 11, 12, 13), 4: (14, 15, 16)}[target[1]])
        which = dc if kind.endswith("_c") else dd
        if which is dd and W == 32:
            W = 31
            dc, dd = dc[:31], dd[:31]
            dc[30], which = rng.randrange(1, 9), dd
        which[W - 1] = v
        if v == 16:
            which[W - 2] = rng.randrange(-8, 0)  # below 2^(4W)
    elif kind == "top_both":
        dc[W - 1] = dd[W - 1] = 16
        dc[W - 2], dd[W - 2] = rng.randrange(-8, 0), rng.randrange(-8, 0)
    elif kind in POSITIONS:
        _, part, i, j = target
        n = {"top": W - 1, "below": W - 2, "zero": 0}[kind]
        for ds, v in ((dc, i), (dd, j)):
            lim = 16 if kind == "top" else 7
            if part == "h":
                cand = [D for D in range(0 if kind == "top" else -8, lim + 1) if split4(D)[0] == v]
            else:
                cand = [D for D in range(0 if kind == "top" else -8, lim + 1) if split4(D)[1] == v]
            if ds is dd and kind == "top" and W == 32:
                cand = [D for D in cand if D <= 7] or cand
            ds[n] = rng.choice(cand)
        if kind == "top":
            if dd[W - 1] > 7 and W == 32:
                W = 31
                dc, dd = dc[1:], dd[1:]
            for ds in (dc, dd):
                if ds[W - 1] == 16:
                    ds[W - 2] = rng.randrange(-8, 0)
            if dc[W - 1] == 0 and dd[W - 1] == 0:
                # both top digits zero: only a pair short enough to be clamped to 29 windows has them
                W = 29
                dc, dd = dc[:29], dd[:29]
                dc[28] = dd[28] = 0
                dc[27], dd[27] = rng.randrange(1, 8), rng.randrange(1, 8)
    elif kind in ("run_c", "run_d"):
        which = dc if kind == "run_c" else dd
        at = rng.randrange(1, W - RUN - 1)
        for i in range(at, at + RUN):
            which[i] = target[1]
    dd[0] |= 1  # d odd (as a digit: nibble - 8 odd)
    if kind == "zero" and split4(dd[0])[target[1] == "l"] != target[3]:
        dd[0] = rng.choice([D for D in range(-8, 8) if D % 2 and split4(D)[target[1] == "l"] == target[3]])
    return from_digits(dc), from_digits(dd)


def _k_of_pair(c: int, d: int):
    """k = c / d mod 8L when that is below L, else None (d odd and not a multiple of L)."""
    k = c * pow(d, -1, N8) % N8
    return k if k < L else None


def targeted_pairs(hostsim):
    """[(target, k, c, d, W)]: one k per wanted target (also the W = 33, 34 and largest-W ones,
    which come from the even-cofactor adjustment and are searched for, not built from digits),
    with (c, d, W) as the host build returns them; every wanted target is hit by some entry."""
    rng = random.Random(0x45C0DE)
    want, _ = named_targets()
    out = []
    for target in sorted(want, key=repr):
        if target[0] == "W" and target[1] >= 33:
            continue
        for _ in range(20000):
            c, d = _pair_for(target, rng)
            if c < 0 or d <= 0:
                continue
            ds = -d if (rng.random() < 0.5 if target[0] != "dneg" else target[1]) else d
            k = _k_of_pair(c, ds)
            if k is None:
                continue
            hc, hd, hw = host_halfsize(hostsim, k)
            if (hc, hd) != (c, ds) or target not in targets_of(hc, hd, hw):
                continue
            out.append((target, k, hc, hd, hw))
            break
        else:
            raise AssertionError("no k for target %r" % (target,))
    out += _adjusted_pairs(hostsim, rng)
    return out


LARGEST_W = 36


def _adjusted_pairs(hostsim, rng):
    """k whose pair comes out of the even-cofactor adjustment longer than 128 bits: tight W = 33, 34
    and the largest the construction reaches.  The adjusted pair's magnitude is about
    8L / (r_i + |t_i|), and the adjustment's own quotient r_{i-1} / r_i must stay below 2^32 - 2, so
    r_i |t_i| >~ 8L / 2^32: the longest pairs have r_i ~ |t_i| ~ 2^112 and ~2^143, W = 36 (40,000
    draws of this construction gave W = 36 on 169 and never more).  Built from the continued
    fraction: small quotients until the cofactor t has 100..126 bits, then k a small distance from
    8L times the convergent, so that the next quotient is large and the next remainder short; kept
    when the host build reports the wanted W."""
    out = []
    for w in (33, 34, 35, LARGEST_W):
        for _ in range(20000):
            tbits = rng.randrange(100, 127)
            h0, h1, k0, k1 = 1, rng.choice((8, 9, 11, 16)), 0, 1
            while k1.bit_length() < tbits:
                q = rng.choice((1, 1, 2, 3, 5))
                h0, h1, k0, k1 = h1, q * h1 + h0, k1, q * k1 + k0
            delta = rng.getrandbits(rng.randrange(1, max(2, 255 - 2 * tbits) + 1))
            k = N8 * k1 // h1 + (delta if rng.random() < 0.5 else -delta)
            if not 0 < k < L:
                continue
            hc, hd, hw = host_halfsize(hostsim, k)
            if hw == w:
                out.append((("W", w), k, hc, hd, hw))
                break
        else:
            raise AssertionError("no k with tight W = %d" % w)
    return out


# ------------------------------------------------------------------ family c: chosen e
def e_targets():
    """(wanted, unreachable) (half, window, target) triples of e's radix-2^26 digits for e < L,
    derived from L as tests/test_scalar_edges_host.py derives the other recodings': the least e with
    a half's window at the target has only that field (and the bit below it) set."""
    want, unreachable = set(), {}
    for h in range(2):
        for m in range(5):
            for t in SC.TARGETS:
                if t == "min":
                    x = 1 << (26 * m + 25)
                elif m == 0:
                    unreachable[(h, m, t)] = "window 0 has no bit below it"
                    continue
                else:
                    field = (1 << 26) - 1 if t == "wrap" else (1 << 25) - 1
                    x = (field << (26 * m)) | 1 << (26 * m - 1)
                if x >> 128:
                    unreachable[(h, m, t)] = "window 4 holds bits 104..127 of a half: 24 bits, below every edge"
                elif x << (128 * h) >= L:
                    unreachable[(h, m, t)] = "above L"
                else:
                    want.add((h, m, t))
    return want, unreachable


def e_scalars():
    """[(tag, e)], e < L: those of SC.e26_scalars() below L (e = 0 among them), and one e per reachable target
    (the other half random, below 2^124 where it is the high one)."""
    rng = random.Random(0xE26C)
    out = [(tag, e) for tag, e in SC.e26_scalars() if e < L]
    want, _ = e_targets()
    for h, m, t in sorted(want):
        while True:
            x = SC._edge_scalar(26, m, t, rng, limit_bits=128 if h == 0 else 124)
            e = x | (rng.getrandbits(124) << 128) if h == 0 else rng.getrandbits(128) | (x << 128)
            if e < L and (h, m, t) in SC.targets_hit_e26(e):
                break
        out.append(("e26c_h%d_w%d_%s" % (h, m, t), e))
    return out


# ------------------------------------------------------------------ the signatures
@functools.lru_cache(maxsize=None)
def _keys():
    """[(tag, point, encoding)]: an ordinary key, that key plus a point of order 2, 4 and 8, and the
    identity."""
    a0 = E.pt_mul(0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9 % L, E.BASE)
    tors = {n: pt for n, pt, _ in SC.torsion_keys()}
    keys = [("A0", a0)] + [("A0+T%d" % n, E.pt_add(a0, tors[n])) for n in (2, 4, 8)] + [("Aid", E.IDENTITY)]
    return [(tag, pt, E.encode(pt)) for tag, pt in keys], tors


def _tuple(tag, pub, rb, s, k):
    sig = rb + s.to_bytes(32, "little")
    return {"tag": tag, "pub": pub, "sig": sig, "k": k, "go": expect_go(pub, sig, k),
            "zip": expect_zip215(pub, sig, k)}


def _signatures(tag, k, s, key, defects, more):
    """The valid signature of (key, S, k) and its rejects: R + T' for T' in defects, and when `more`
    S + 1, a flipped bit of R, k + 1 and k - 1."""
    keys, tors = _keys()
    ktag, _, pub = keys[key]
    r = _sb_minus_ka(pub, s, k)
    rb = E.encode(r)
    tag = "%s/%s" % (tag, ktag)
    out = [_tuple(tag, pub, rb, s, k)]
    assert out[0]["go"] and out[0]["zip"], tag
    for n in defects:
        out.append(_tuple("%s/R+T%d" % (tag, n), pub, E.encode(E.pt_add(r, tors[n])), s, k))
        assert not out[-1]["go"] and out[-1]["zip"], out[-1]["tag"]
    if more:
        out.append(_tuple(tag + "/S+1", pub, rb, s + 1, k))
        flip = bytearray(rb)
        flip[k % 32] ^= 1 << (s % 8)
        out.append(_tuple(tag + "/Rflip", pub, bytes(flip), s, k))
        for dk in (1, -1):
            if 0 <= k + dk < L:
                out.append(_tuple("%s/k%+d" % (tag, dk), pub, rb, s, k + dk))
        assert not any(t["go"] for t in out[-4:] if t["pub"] != keys[4][2]), tag  # (k +- 1 is the same under the identity key)
    return out


_CORPUS = None


def corpus(hostsim):
    """{"cases": every tuple ({"tag", "pub", "sig", "k", "go", "zip", "family"}), "pairs": family b's
    (target, k, c, d, W), "e": family c's (tag, e, k)}; built once per process.  The coverage
    assertions are here: every named target of family b and every reachable e target is hit."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    rng = random.Random(0xC0FFEE)
    cases = []

    def add(family, ts):
        for t in ts:
            t["family"] = family
        cases.extend(ts)

    # a: the existing chosen-k families, each valid and with every small-order defect
    ks, n_edge = PC.halfsize_lattice_ks()
    fam_a = [("quot%d" % i, k) for i, k in enumerate(PC.halfsize_quotient_ks())]
    fam_a += [("long%d" % i, k) for i, k in enumerate(PC.halfsize_long_euclid_ks()[::10])]
    fam_a += [("edge%d" % i, k) for i, k in enumerate(ks[:n_edge])]
    assert len(PC.halfsize_quotient_ks()) == 41 and n_edge == 14 and len(fam_a) == 85
    for i, (tag, k) in enumerate(fam_a):
        add("a", _signatures("a:" + tag, k, rng.randrange(L), i % 5, (2, 4, 8), False))

    # b: targeted pairs
    pairs = targeted_pairs(hostsim)
    want, unreachable = named_targets()
    hit = set()
    for _, k, c, d, w in pairs:
        assert (c - d * k) % N8 == 0 and d % 2
        hit |= targets_of(c, d, w)
    assert want <= hit, sorted(want - hit, key=repr)
    assert not (set(unreachable) & hit), sorted(set(unreachable) & hit, key=repr)
    assert max(w for *_, w in pairs) == LARGEST_W
    for i, (target, k, c, d, w) in enumerate(pairs):
        tag = "b:" + "_".join(str(x) for x in target)
        add("b", _signatures(tag, k, rng.randrange(L), (i // 3) % 5, ((2, 4, 8)[i % 3],), True))

    # c: chosen e on pairs of both signs of d (e = |d| S mod L, negated when d < 0)
    by_sign = {s: next(p for p in pairs if (p[3] < 0) == s and p[4] == 32) for s in (False, True)}
    e_want, e_unreachable = e_targets()
    e_hit, e_list = set(), []
    for i, (tag, e) in enumerate(e_scalars()):
        for neg, (_, k, c, d, w) in by_sign.items():
            s = (L - e if neg else e) * pow(abs(d), -1, L) % L
            got = abs(d) * s % L
            assert (L - got if neg and got else got) == e
            e_hit |= SC.targets_hit_e26(e)
            e_list.append((tag, e, k))
            add("c", _signatures("c:%s_d%s" % (tag, "-" if neg else "+"), k, s, (i + neg) % 5, ((2, 4, 8)[i % 3],), False))
    assert e_hit == e_want, sorted(e_hit ^ e_want)
    assert not (set(e_unreachable) & e_hit)

    _CORPUS = {"cases": cases, "pairs": pairs, "e": e_list}
    return _CORPUS


def signatures_at_w(hostsim, w: int, n: int, seed: int = 0x29):
    """n valid and defective tuples (alternating, keys cycling) on n distinct k of tight W = w <= 32,
    drawn as family b draws them: the lanes of the short-wave and fallback-wave tests."""
    rng = random.Random(seed + w)
    out = []
    while len(out) < n:
        c, d = _pair_for(("W", w), rng)
        k = _k_of_pair(c, -d if rng.random() < 0.5 else d) if c >= 0 and d > 0 else None
        if k is None or host_halfsize(hostsim, k)[2] != w:
            continue
        i = len(out)
        ts = _signatures("w%d_%d" % (w, i), k, rng.randrange(L), i % 5, ((2, 4, 8)[i % 3],), False)
        out.append(ts[i % 2])
    return out


def arrays(cases):
    """(pubs, sigs, ks (n x 32 little-endian bytes), expected cofactorless, expected ZIP-215) of cases."""
    n = len(cases)
    pubs = np.frombuffer(b"".join(c["pub"] for c in cases), np.uint8).reshape(n, 32).copy()
    sigs = np.frombuffer(b"".join(c["sig"] for c in cases), np.uint8).reshape(n, 64).copy()
    ks = np.frombuffer(b"".join(c["k"].to_bytes(32, "little") for c in cases), np.uint8).reshape(n, 32).copy()
    go = np.array([c["go"] for c in cases], np.uint8)
    zp = np.array([c["zip"] for c in cases], np.uint8)
    return pubs, sigs, ks, go, zp


def fallback_ks():
    """The k of family a that the model sends to the (k, 1) fallback (W = 64)."""
    return [k for k in PC.halfsize_quotient_ks() if model_halfsize(k)[3]]
