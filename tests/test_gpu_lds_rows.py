"""The P and Q rows of the joint table in LDS (verify_main_hs_kernel<26>'s accessor, SlabLdsTabJ):

* every row 0..12, read as stored and with Y+X / Y-X exchanged, through the accessor
  (tmed_test_lds_rows) against the rows the slab-only accessor stores (tmed_test_joint_rows) on the
  same inputs, bit for bit, and rows 1 and 5 of the slab left as they were;
* decisions of the throughput kernels against the oracle's C port on batches holding every C5 class;
* how often a sub-step of the Straus sum looks up P, Q or the identity, over the first 4,096 C2
  scalars, recoded on the host (the lattice step of tests/native/hostsim.cpp, then sc_recode16,
  hs_top_digit, hs_split4 and joint_index redone here)."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import ed25519_go as E
from oracle import port
from tmed._native import lib
from tmed.workload import SMALL_ORDER, c2_messages, c2_seeds, c5_mix

pytestmark = pytest.mark.gpu

ROWS = 12
LANES = [1, 63, 64, 65, 256, 257]  # a partial wave, a wave's end, a block's end, a second block
FILL = 0xA5


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _triples(n):
    """n (A, R, dneg) encodings: random valid points, A or R of small order (the identity and the
    point of order two among them: x = 0), A with x = 0 beside a random R, A = +-R; both signs of d
    in every kind.  The kinds cycle, so every prefix of 8 or more lanes holds each."""
    rng = np.random.default_rng(0x1d5)
    pts = [E.pt_mul(int.from_bytes(rng.bytes(32), "little") % E.L, E.BASE) for _ in range(16)]
    enc = [E.encode(p) for p in pts]
    tr = []
    for k in range(n):
        kind, s = k % 8, (k // 8) & 1
        a, r = enc[k % 16], enc[(7 * k + 3) % 16]
        if kind == 1:
            a = SMALL_ORDER[(k // 8) % 8]
        elif kind == 2:
            r = SMALL_ORDER[(k // 8) % 8]
        elif kind == 3:
            a = SMALL_ORDER[(k // 8) % 2]  # (0, 1) and (0, -1): x = 0
        elif kind == 4:
            r = a
        elif kind == 5:
            r = E.encode(E.pt_neg(pts[k % 16]))
        elif kind == 6:
            a, r = SMALL_ORDER[(k // 8) % 8], SMALL_ORDER[(3 * (k // 8) + 1) % 8]
        tr.append((a, r, s if kind else 1 - s))
    return tr


def _unpack256(row):
    """fe_unpack256 on a packed 32-byte field element (8 little-endian words) -> ten int32 limbs."""
    w = [int(x) for x in np.frombuffer(row, "<u4")]
    m26, m25 = 0x3ffffff, 0x1ffffff
    v9 = w[7] >> 6
    if w[7] & 0x80000000:
        v9 -= 1 << 26  # arithmetic shift of the int32
    return [w[0] & m26, ((w[0] >> 26) | (w[1] << 6)) & m25, ((w[1] >> 19) | (w[2] << 13)) & m26,
            ((w[2] >> 13) | (w[3] << 19)) & m25, w[3] >> 6, w[4] & m25, ((w[4] >> 25) | (w[5] << 7)) & m26,
            ((w[5] >> 19) | (w[6] << 13)) & m25, ((w[6] >> 12) | (w[7] << 20)) & m26, v9]


def _expected(packed):
    """[13][2][40] limbs from a lane's twelve packed rows (Y+X, Y-X, Z, 2dT of 32 bytes each): row 0
    the identity (1, 1, 1, 0); swap exchanges the first two elements."""
    one, zero = [1] + [0] * 9, [0] * 10
    out = np.zeros((ROWS + 1, 2, 40), np.int32)
    out[0, 0] = out[0, 1] = one + one + one + zero
    for j in range(ROWS):
        f = [_unpack256(packed[128 * j + 32 * k:128 * j + 32 * k + 32]) for k in range(4)]
        out[j + 1, 0] = f[0] + f[1] + f[2] + f[3]
        out[j + 1, 1] = f[1] + f[0] + f[2] + f[3]
    return out


@pytest.mark.parametrize("n", LANES)
def test_rows_through_lds_equal_the_slab_rows(generic_engines, n):
    h = generic_engines["throughput"]._h
    tr = _triples(n)
    a = np.frombuffer(b"".join(t[0] for t in tr), np.uint8).copy()
    r = np.frombuffer(b"".join(t[1] for t in tr), np.uint8).copy()
    dn = np.array([t[2] for t in tr], np.uint8)
    assert n < 8 or (dn[::8].min() == 0 and dn[::8].max() == 1)
    ref = np.zeros((n, ROWS * 128), np.uint8)
    assert lib().tmed_test_joint_rows(h, _p(a), _p(r), _p(dn), n, _p(ref)) == 0
    slab = np.full((n, ROWS, 128), FILL, np.uint8)
    got = np.zeros((n, ROWS + 1, 2, 40), np.int32)
    assert lib().tmed_test_lds_rows(h, _p(a), _p(r), _p(dn), n, _p(slab), _p(got)) == 0
    one = np.array([1] + [0] * 9, np.int32)
    for i in range(n):
        exp = _expected(ref[i].tobytes())
        bad = np.argwhere((got[i] != exp).any(axis=2))
        assert bad.size == 0, (i, bad[:4].tolist())
        assert (got[i, [1, 5], :, 20:30] == one).all(), i  # Z of P and Q is exactly fe_1
    # the slab: rows 1 and 5 untouched, every other row what the slab-only accessor stores
    assert (slab[:, [0, 4]] == FILL).all()
    rest = [j for j in range(ROWS) if j not in (0, 4)]
    assert (slab[:, rest] == ref.reshape(n, ROWS, 128)[:, rest]).all()


N_E2E = 1000
FRAC = 0.06  # 60 replaced tuples: ten of each of c5_mix's six classes


@pytest.fixture(scope="module")
def c5_pool(generic_engines):
    """(pubs, sigs, msgs, offs, expected, replaced): 1,000 C2 tuples with c5_mix at 6 %, the port's
    verdicts computed once."""
    eng = generic_engines["throughput"]
    seeds = c2_seeds(0, N_E2E)
    msgs, offs = c2_messages(0, N_E2E)
    msgs = np.concatenate([msgs, np.zeros(16, np.uint8)])
    sigs, pubs = eng.sign_arrays(seeds, msgs, offs)
    idx = c5_mix(pubs, sigs, frac=FRAC)
    exp = port.verify_batch(pubs, sigs, msgs, offs.astype(np.uint64), 8)
    return pubs, sigs, msgs, offs, exp, idx


def test_every_c5_class_occurs(c5_pool):
    """c5_mix gives replaced tuple j class j % 6: each class ten times at n = 1000, and the port
    rejects every replaced tuple but, at most, flipped message bits (class 0 may flip one)."""
    pubs, sigs, msgs, offs, exp, idx = c5_pool
    assert len(idx) == int(N_E2E * FRAC) == 60
    counts = np.bincount(np.arange(len(idx)) % 6, minlength=6)
    assert (counts == 10).all()
    small = {bytes(s) for s in SMALL_ORDER}
    assert sum(pubs[i].tobytes() in small for i in idx) == 10          # class 2
    assert sum(sigs[i, :32].tobytes() in small for i in idx) == 10     # class 3
    assert sum(int.from_bytes(sigs[i, 32:].tobytes(), "little") >= E.L for i in idx) >= 10  # class 1
    assert sum(int.from_bytes(pubs[i].tobytes(), "little") & ((1 << 255) - 1) >= E.P for i in idx) == 10  # class 4
    keep = np.ones(N_E2E, bool)
    keep[idx] = False
    assert exp[keep].all() and exp[idx].sum() <= 10


@pytest.mark.parametrize("n", [1, 64, 65, 257, 1000])
def test_decisions_equal_the_port(generic_engines, c5_pool, n):
    """The first n tuples, and the n tuples ending at the last replaced one (so the short batches
    hold a C5 tuple too)."""
    eng = generic_engines["throughput"]
    pubs, sigs, msgs, offs, exp, idx = c5_pool
    for lo in sorted({0, max(0, int(idx.max()) + 1 - n)}):
        o = (offs[lo:lo + n + 1] - offs[lo]).astype(np.uint32)
        m = msgs[int(offs[lo]):int(offs[lo + n]) + 16]
        out = eng.verify_arrays(pubs[lo:lo + n], sigs[lo:lo + n], m, o)
        bad = np.nonzero(out != exp[lo:lo + n])[0]
        assert bad.size == 0, (lo, n, bad[:10].tolist())


def _digits(x, W):
    """The W signed radix-16 digits of x as hs_straus_joint reads them: sc_recode16 (x + 0x88..88,
    nibble - 8), the top one with the carry into nibble W (hs_top_digit)."""
    r = x + int("88" * 32, 16)
    d = [((r >> (4 * i)) & 15) - 8 for i in range(W)]
    if W < 64:
        d[W - 1] += 16 * ((r >> (4 * W)) & 1)
    return d


def _split4(D):
    lo = ((D + 2) & 3) - 2
    return (D - lo) >> 2, lo


def lookup_rows(c, d, W):
    """The joint-table rows (|5i + j|) of one signature's sum, in order: the top window's two high
    rows, then a low row, then a high and a low row per window.  first_row: the row taken as the
    accumulator itself (ge_cached_to_p3)."""
    dc, dd = _digits(c, W), _digits(d, W)
    hc, lc = _split4(dc[W - 1])
    hd, ld = _split4(dd[W - 1])
    c1, d1 = min(hc, 2), min(hd, 2)
    rows = [abs(5 * c1 + d1), abs(5 * (hc - c1) + (hd - d1)), abs(5 * lc + ld)]
    for n in range(W - 2, -1, -1):
        hc, lc = _split4(dc[n])
        hd, ld = _split4(dd[n])
        rows += [abs(5 * hc + hd), abs(5 * lc + ld)]
    assert len(rows) == 2 * W + 1 and max(rows) <= ROWS
    return rows


def c2_row_counts(hostsim, n):
    """Lookups per row over the first n C2 scalars k = SHA-512(R || A || M) mod L, each over its own
    tight window count, and how many signatures take P or Q as their first row."""
    seeds = c2_seeds(0, n)
    msgs, offs = c2_messages(0, n)
    sigs, pubs = port.sign_batch(seeds, msgs, offs.astype(np.uint64), 8)
    hist = np.zeros(ROWS + 1, np.int64)
    first_pq = 0
    c32, d32 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    dneg, tight = ctypes.c_int(0), ctypes.c_int(0)
    for i in range(n):
        m = msgs[int(offs[i]):int(offs[i + 1])].tobytes()
        k = int.from_bytes(hashlib.sha512(sigs[i, :32].tobytes() + pubs[i].tobytes() + m).digest(), "little") % E.L
        hostsim.hostsim_halfsize_tight(k.to_bytes(32, "little"), c32, d32, ctypes.byref(dneg), ctypes.byref(tight), 1)
        rows = lookup_rows(int.from_bytes(c32.raw, "little"), int.from_bytes(d32.raw, "little"), tight.value)
        hist += np.bincount(rows, minlength=ROWS + 1)
        first_pq += rows[0] in (1, 5)
    return hist, first_pq


def test_share_of_lookups_served_from_lds(hostsim):
    """Over the first 4,096 C2 scalars 66,101 of 267,106 lookups (65.2 per signature) read P or Q
    (24.75 %: 33,263 Q, 32,838 P) and 18,640 the identity (6.98 %), counted on the host before the
    bounds below were fixed; uniform digits give 1/4 and 1/16.  323 of the signatures start from P or
    Q: the top window's first row, which becomes the accumulator through ge_cached_to_p3."""
    hist, first_pq = c2_row_counts(hostsim, 4096)
    total = int(hist.sum())
    print("lookups", total, "Q", int(hist[1]), "P", int(hist[5]), "identity", int(hist[0]), "first row P/Q", first_pq)
    share = (hist[1] + hist[5]) / total
    assert 0.20 <= share <= 0.30, share
    assert first_pq > 0
