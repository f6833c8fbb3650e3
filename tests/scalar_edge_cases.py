"""Scalars at the edges of the kernels' signed-digit recodings, and valid signatures that carry them
(pure Python; tests/test_scalar_edges_host.py and tests/test_gpu_scalar_edges.py).

S comes straight out of the signature, so a signer chooses it: with A the identity, R = enc([S]B)
verifies for every S < L; with A = T of small order, R = enc([S]B - [j]T) verifies once the message
is ground to k = j (mod ord T).  k's digits come from grinding the message under a fixed nonce.

The digit models below restate the definitions in the header comments (verify_core.h sc_recode256 /
sc_recode_b, kernels.h kB24* / kCombA*, verify_hs.h hs_b26_digit), not the C++:

  biased radix 2^r (r = 8, 16):  x' = x + sum_m 2^(rm + r - 1); d_m = field_m(x') - 2^(r-1),
      in [-2^(r-1), 2^(r-1) - 1]; 256 / r windows.
  carry-free radix 2^r:  d_m = bits [rm, rm + r) + bit (rm - 1) - 2^r bit (rm + r - 1),
      in [-2^(r-1), 2^(r-1)].  r = 24: 11 windows of S.  r = 12: 21 windows of k, the top one
      (m = 20) unsigned: every bit from 240 up + bit 239.  r = 26: five windows of each 128-bit
      half of e.

A window's edge digits ("targets"):
  "max"  the largest digit: 2^(r-1) - 1 biased, +2^(r-1) carry-free (field 2^(r-1) - 1 + the bit below)
  "min"  -2^(r-1)
  "wrap" the all-ones field with a carry (biased) or the bit below (carry-free) coming in: the digit
         wraps to 0 and the carry / below bit goes on into the next window
"""
from __future__ import annotations

import functools
import hashlib
import random

import numpy as np

from oracle import ed25519_go as E

L = E.L
TARGETS = ("max", "min", "wrap")
S_RADICES = (8, 16, 24)
K_BITS, K_WINDOWS = 12, 21


# ------------------------------------------------------------------ digit models
def digits_biased(x: int, r: int) -> list[int]:
    nw = 256 // r
    xb = x + sum(1 << (r * m + r - 1) for m in range(nw))
    assert 0 <= x and xb < 1 << 256
    return [((xb >> (r * m)) & ((1 << r) - 1)) - (1 << (r - 1)) for m in range(nw)]


def _bit(x: int, i: int) -> int:
    return (x >> i) & 1 if i >= 0 else 0


def digits_carry_free(x: int, r: int, nw: int, top_unsigned: bool = False) -> list[int]:
    out = []
    for m in range(nw):
        if top_unsigned and m == nw - 1:
            out.append((x >> (r * m)) + _bit(x, r * m - 1))
        else:
            out.append(((x >> (r * m)) & ((1 << r) - 1)) + _bit(x, r * m - 1) - (_bit(x, r * m + r - 1) << r))
    return out


def digits_s24(s: int) -> list[int]:
    return digits_carry_free(s, 24, 11)


def digits_k12(k: int) -> list[int]:
    return digits_carry_free(k, K_BITS, K_WINDOWS, top_unsigned=True)


def digits_e26(e: int) -> tuple[list[int], list[int]]:
    """(low half's five digits, high half's) of e < 2^256."""
    return (digits_carry_free(e & ((1 << 128) - 1), 26, 5), digits_carry_free(e >> 128, 26, 5))


def digits_of(x: int, radix: int) -> list[int]:
    """S's digits in radix 2^8 / 2^16 (biased) / 2^24 (carry-free); k's in radix 2^12."""
    if radix in (8, 16):
        return digits_biased(x, radix)
    return digits_s24(x) if radix == 24 else digits_k12(x)


def targets_hit(x: int, radix: int) -> set[tuple[int, str]]:
    """The (window, target) pairs x's recoding in that radix (8, 16, 24 of S; 12 of k) passes through."""
    biased = radix in (8, 16)
    ds = digits_of(x, radix)
    half, mask = 1 << (radix - 1), (1 << radix) - 1
    hit = set()
    for m, d in enumerate(ds):
        if radix == K_BITS and m == K_WINDOWS - 1:
            continue  # the unsigned top window has no signed edge
        field = (x >> (radix * m)) & mask
        if d == (half - 1 if biased else half):
            hit.add((m, "max"))
        if d == -half:
            hit.add((m, "min"))
        if d == 0 and field == mask:
            hit.add((m, "wrap"))
    return hit


def targets_hit_e26(e: int) -> set[tuple[int, int, str]]:
    """(half, window, target) for the radix-2^26 digits of e's two 128-bit halves."""
    hit = set()
    for h, x in enumerate((e & ((1 << 128) - 1), e >> 128)):
        for m, d in enumerate(digits_carry_free(x, 26, 5)):
            field = (x >> (26 * m)) & ((1 << 26) - 1)
            if d == 1 << 25:
                hit.add((h, m, "max"))
            if d == -(1 << 25):
                hit.add((h, m, "min"))
            if d == 0 and field == (1 << 26) - 1:
                hit.add((h, m, "wrap"))
    return hit


# ------------------------------------------------------------------ scalars at the edges
def _edge_scalar(radix: int, m: int, target: str, rng: random.Random, limit_bits: int = 252):
    """A scalar below 2^limit_bits whose window m sits at `target`, random elsewhere; None when the
    window's field or the bit it needs from below does not fit."""
    biased = radix in (8, 16)
    half, mask = 1 << (radix - 1), (1 << radix) - 1
    lo = radix * m
    need_in = target == "wrap" or (target == "max" and not biased)  # a carry / below bit coming in
    if need_in and m == 0:
        return None
    field = {"max": half - 1, "min": half, "wrap": mask}[target]
    if lo + field.bit_length() > limit_bits:
        return None
    x = rng.getrandbits(limit_bits)
    # the window's field, and the two bits under it: bit lo - 1 is the below bit (and, biased, decides
    # the carry together with bit lo - 2: 1x carries, 00 does not whatever comes from further down)
    clear = mask << lo
    if m:
        clear |= 3 << (lo - 2) if lo >= 2 else 1 << (lo - 1)
    x &= ~clear
    x |= field << lo
    if need_in:
        x |= 1 << (lo - 1)
    return x & ((1 << limit_bits) - 1)


@functools.lru_cache(maxsize=None)
def s_scalars() -> tuple[tuple[str, int], ...]:
    """(tag, S) with S < L: per radix and window the three edge digits, runs of them, and the
    scalars around 0, 2^128, 2^252 and L."""
    rng = random.Random(0x5CA1A2)
    out = []
    for r in S_RADICES:
        nw = 11 if r == 24 else 256 // r
        for m in range(nw):
            for t in TARGETS:
                x = _edge_scalar(r, m, t, rng)
                if x is None:
                    continue
                assert x < L and (m, t) in targets_hit(x, r), (r, m, t)
                out.append(("r%d_w%d_%s" % (r, m, t), x))
        # runs: every window all ones (a carry through every window), every window at its minimum
        # field, and a run of wrapping windows that starts at each third window
        out.append(("r%d_run_ones" % r, (1 << 252) - 1))
        out.append(("r%d_run_min" % r, sum(1 << (r * m + r - 1) for m in range(nw) if r * m + r <= 252)))
        for m0 in range(1, nw - 1, 3):
            hi = min(r * (nw - 1), 252)
            out.append(("r%d_run_wrap_from%d" % (r, m0), ((1 << hi) - 1) ^ ((1 << (r * m0 - 1)) - 1)))
    top = 1 << 252
    for tag, x in [("zero", 0), ("one", 1), ("two", 2), ("L-1", L - 1), ("L-2", L - 2), ("2^252", top),
                   ("2^252+1", top + 1), ("2^252-1", top - 1), ("2^128", 1 << 128), ("2^128+1", (1 << 128) + 1),
                   ("2^128-1", (1 << 128) - 1),
                   # the largest top windows an S < L reaches: bits 240.. = 4096 with everything under L's
                   # low part, and 4095 + the bit below
                   ("top_4096_low_ones", top + (1 << 124) - 1), ("top_4095_below", top - (1 << 239)),
                   ("top_4095_all", top - 1 - (1 << 200))]:
        assert 0 <= x < L
        out.append((tag, x))
    return tuple(out)


def e26_scalars() -> list[tuple[str, int]]:
    """(tag, e) for hs_b26_digit: every window of both halves at +-2^25 and the wrap, where a 128-bit
    half reaches them, the other half random."""
    rng = random.Random(0xE26)
    out = []
    for h in range(2):
        for m in range(5):
            for t in TARGETS:
                x = _edge_scalar(26, m, t, rng, limit_bits=128)
                if x is None:
                    continue
                other = rng.getrandbits(128)
                e = x | (other << 128) if h == 0 else other | (x << 128)
                assert (h, m, t) in targets_hit_e26(e), (h, m, t)
                out.append(("e26_h%d_w%d_%s" % (h, m, t), e))
    ones = (1 << 128) - 1
    out += [("e26_zero", 0), ("e26_ones", (1 << 256) - 1), ("e26_lo_ones", ones), ("e26_hi_ones", ones << 128),
            ("e26_lo_top", 1 << 127), ("e26_hi_one", 1 << 128), ("e26_L-1", L - 1)]
    return out


# ------------------------------------------------------------------ signatures
def _order(pt) -> int:
    n, q = 1, pt
    while not E.pt_equal(q, E.IDENTITY):
        q, n = E.pt_add(q, pt), n + 1
    return n


@functools.lru_cache(maxsize=None)
def torsion_keys():
    """[(order, point, canonical encoding)] for orders 1 (the identity), 2, 4 and 8."""
    keys = {}
    for pt in E.small_order_points():
        n, enc = _order(pt), E.encode(pt)
        if n not in keys and E.decode(enc) is not None:
            keys[n] = (n, pt, enc)
    return [keys[n] for n in (1, 2, 4, 8)]


def _chosen_s_signature(s: int, sB, order: int, T, pub: bytes, tag: str) -> tuple[bytes, bytes]:
    """(message, signature) valid under the small-order key T for the chosen S: R = [S]B - [j]T and a
    message ground to k = j (mod ord T)."""
    j = s % order
    rb = E.encode(E.pt_add(sB, E.pt_neg(E.pt_mul(j, T))))
    for ctr in range(4096):
        msg = ("edge %s ord%d #%d" % (tag, order, ctr)).encode()
        if E.hram(rb, pub, msg) % order == j:
            return msg, rb + s.to_bytes(32, "little")
    raise RuntimeError("no message for " + tag)


def _case(tag, pub, msg, sig):
    return {"tag": tag, "pub": pub, "msg": msg, "sig": sig, "valid": bool(E.verify(pub, msg, sig))}


K_NONCE = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1 % L


def _k_edge_cases():
    """Three ordinary keys, one fixed nonce: messages ground until window m < 20 of k's radix-2^12
    digits sits at each target ("max" and "wrap" need the bit below: not at m = 0)."""
    want = {(m, t) for m in range(K_WINDOWS - 1) for t in TARGETS if m or t == "min"}
    rb = E.encode(E.pt_mul(K_NONCE, E.BASE))
    out = []
    for ki in range(3):
        h = hashlib.sha512(b"scalar-edge-key-%d" % ki).digest()
        a = E._clamp(h[:32]) % L
        pub = E.encode(E.pt_mul(a, E.BASE))
        left, ctr = set(want), 0
        hasher = hashlib.sha512(rb + pub)
        while left:
            msg = b"k-edge %d/%d" % (ki, ctr)
            ctr += 1
            hh = hasher.copy()
            hh.update(msg)
            k = int.from_bytes(hh.digest(), "little") % L
            # a window at an edge shows in the 13 bits from its below bit up: 0fff, 1000 or 1fff
            # (a quick filter; targets_hit below decides)
            if (k & 0xfff) != 0x800 and not any(((k >> (12 * m - 1)) & 0x1fff) in (0x0fff, 0x1000, 0x1fff)
                                                 for m in range(1, K_WINDOWS - 1)):
                continue
            new = targets_hit(k, K_BITS) & left
            if not new:
                continue
            left -= new
            s = (K_NONCE + k * a) % L
            out.append(_case("k12_key%d_%s" % (ki, "+".join("w%d%s" % mt for mt in sorted(new))), pub, msg,
                             rb + s.to_bytes(32, "little")))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple[dict, ...]:
    """Every edge signature, each {"tag", "pub", "msg", "sig", "valid"} with the expected bit from
    oracle.ed25519_go.verify: the S scalars under the identity key and a canonical key of order 2, 4
    and 8, rejects of a fixed subset (a one-bit flip in R, S + 1 and S + L under the same R), and the
    k-digit cases.  Built once per process."""
    out = []
    for i, (tag, s) in enumerate(s_scalars()):
        sB = E.pt_mul(s, E.BASE)
        for order, T, pub in torsion_keys():
            msg, sig = _chosen_s_signature(s, sB, order, T, pub, tag)
            out.append(_case("%s_ord%d" % (tag, order), pub, msg, sig))
            if (i + order) % 5 == 0:  # a fixed subset also as rejects
                flip = bytearray(sig)
                flip[(i * 7) % 32] ^= 1 << (i % 8)
                out.append(_case("%s_ord%d_Rflip" % (tag, order), pub, msg, bytes(flip)))
                out.append(_case("%s_ord%d_S+1" % (tag, order), pub, msg, sig[:32] + (s + 1).to_bytes(32, "little")))
                out.append(_case("%s_ord%d_S+L" % (tag, order), pub, msg, sig[:32] + (s + L).to_bytes(32, "little")))
    out += _k_edge_cases()
    return tuple(out)


def arrays(cs=None, order=None):
    """(pubs, sigs, msgs, offs (u32), expected) of cases cs (default: all) in the given order."""
    cs = list(cases() if cs is None else cs)
    if order is not None:
        cs = [cs[i] for i in order]
    pubs = np.array([np.frombuffer(c["pub"], np.uint8) for c in cs])
    sigs = np.array([np.frombuffer(c["sig"], np.uint8) for c in cs])
    offs = np.zeros(len(cs) + 1, np.uint32)
    offs[1:] = np.cumsum([len(c["msg"]) for c in cs])
    msgs = np.frombuffer(b"".join(c["msg"] for c in cs) + b"\0" * 16, np.uint8)
    exp = np.array([c["valid"] for c in cs], np.uint8)
    return pubs, sigs, msgs, offs, exp


def keyed(pubs: np.ndarray):
    """(key array, key index per signature) of a batch's distinct keys."""
    keys = sorted({p.tobytes() for p in pubs})
    kidx = {k: i for i, k in enumerate(keys)}
    return (np.array([np.frombuffer(k, np.uint8) for k in keys]),
            np.array([kidx[p.tobytes()] for p in pubs], np.uint32))
