"""The exact kernel source (tendermint-fork_amd/csrc/*.h) compiled for the CPU
(tests/native/hostsim.cpp, test-only) against the oracle — catches arithmetic
bugs without a GPU.  The GPU parity proper is tests/test_gpu_verify.py."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import prim_cases as PC
from oracle import ed25519_go as E
from oracle import port

VP = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(VP)


def _fe(l, op, a, b):
    o = ctypes.create_string_buffer(32)
    l.hostsim_fe_op(op, a.to_bytes(32, "little"), b.to_bytes(32, "little"), o)
    return int.from_bytes(o.raw, "little")


def test_field_ops_vs_bigint(hostsim):
    for a, b in PC.field_byte_pairs():
        for op, e in PC.field_byte_expected(a, b).items():
            assert _fe(hostsim, op, a, b) == e, (op, hex(a), hex(b))


def test_binary_gcd_inversion(hostsim):
    """fe25519.h fe_invert_bgcd (the batched finish's inversion): equal to z^(p-2) on random values,
    powers of two and their neighbours, values near p and 0 (0 -> 0, as z^(p-2))."""
    P = E.P
    for a in PC.bgcd_values():
        assert _fe(hostsim, 9, a, 0) == pow(a % P, P - 2, P), hex(a)


def test_pack256_roundtrip_at_the_limb_extremes(hostsim):
    """fe_pack256 / fe_unpack256 (the 128-B per-lane table entries of verify_main_hs_kernel):
    for 2-sums of carried values at the ends of their limb ranges, the unpacked value is congruent
    mod p, its limbs sit in [0, 2^26) / [0, 2^25) (limb 9 in [-2, 2^25]), and it multiplies
    correctly as a fe_mul operand."""
    cases, g = PC.pack256_cases()
    out = (ctypes.c_int32 * 10)()
    prod = ctypes.create_string_buffer(32)
    for c in cases:
        hostsim.hostsim_pack256((ctypes.c_int32 * 10)(*c), g.to_bytes(32, "little"), out, prod)
        PC.check_pack256(c, list(out), int.from_bytes(prod.raw, "little"), g)


def test_sha512_and_reduce(hostsim):
    for m in PC.sha512_messages():
        o = ctypes.create_string_buffer(64)
        hostsim.hostsim_sha512(m, len(m), o)
        assert o.raw == hashlib.sha512(m).digest()
    for x in PC.sc_reduce_values():
        r = ctypes.create_string_buffer(32)
        hostsim.hostsim_sc_reduce(x.to_bytes(64, "little"), r)
        assert int.from_bytes(r.raw, "little") == x % E.L, hex(x)


def test_sha512_stream_prefixes_and_lengths(hostsim):
    """sha512_stream of p0 || p1 || M with 0, 32 and 64 prefix bytes, every message length 0..300
    (the cases of the device comparison)."""
    p0, p1, buf, offs, lens = PC.sha512_stream_cases()
    o = ctypes.create_string_buffer(64)
    for npre in (0, 32, 64):
        for a, b, at, n in zip(p0, p1, offs, lens):
            m = buf[at:at + n]
            hostsim.hostsim_sha512_pre(npre, a, b, m, n, o)
            assert o.raw == hashlib.sha512((a + b)[:npre] + m).digest(), (npre, n)


def test_sc_is_canonical_and_muladd(hostsim):
    """sc_is_canonical (s < L) around L and at every word of its borrow chain; sc_muladd
    (a b + c mod L) with all-ones words, L and its neighbours."""
    for s in PC.sc_canonical_values():
        assert bool(hostsim.hostsim_sc_is_canonical(s.to_bytes(32, "little"))) == (s < E.L), hex(s)
    r = ctypes.create_string_buffer(32)
    for a, b, c in PC.sc_muladd_cases():
        hostsim.hostsim_sc_muladd(a.to_bytes(32, "little"), b.to_bytes(32, "little"), c.to_bytes(32, "little"), r)
        assert int.from_bytes(r.raw, "little") == (a * b + c) % E.L, (hex(a), hex(b), hex(c))


def test_decode_matches_go_rule(hostsim):
    for p in PC.decode_candidates():
        o = ctypes.create_string_buffer(32)
        ok = hostsim.hostsim_decode(p, o)
        pt = E.decode(p)
        assert bool(ok) == (pt is not None), p.hex()
        if pt is not None:
            assert o.raw == E.encode(pt)


def _verify(l, pubs, sigs, msgs, offs, group=16):
    n = len(pubs)
    out = np.zeros(n, np.uint8)
    if group == "hs":  # main variant 6 (default): half-size scalars, verify_hs.h, radix-2^26 B windows
        l.hostsim_verify_batch_hs(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out), None)
        return out
    if group == "hs16":  # the same with the radix-2^16 B windows (no 8.6-GB tables)
        l.hostsim_verify_batch_hs16(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out), None)
        return out
    if group == "b16":  # main-kernel variant 5: radix-2^16 B windows from the 32769-entry table
        l.hostsim_verify_batch_b16(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out))
        return out
    l.hostsim_verify_batch_g(_p(pubs), _p(sigs), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out),
                             ctypes.c_int(group))
    return out


@pytest.mark.parametrize("group", [0, 1, 5, 16, "b16", "hs", "hs16"])
def test_golden_vectors_hostsim(hostsim, golden, group):
    """Every golden tuple, with per-signature encoding (group 0) and through the batched
    finish (Montgomery inversion over groups of 1, 5 and 16 signatures, partial last group);
    "b16": the radix-2^16 B-window variant of the main kernel."""
    vs = [v for v in golden if len(v["sig"]) == 128]
    pubs = np.array([np.frombuffer(bytes.fromhex(v["pub"]), np.uint8) for v in vs])
    sigs = np.array([np.frombuffer(bytes.fromhex(v["sig"]), np.uint8) for v in vs])
    ms = [bytes.fromhex(v["msg"]) for v in vs]
    offs = np.zeros(len(vs) + 1, np.uint32)
    offs[1:] = np.cumsum([len(m) for m in ms])
    msgs = np.frombuffer(b"".join(ms) + b"\0", np.uint8)
    out = _verify(hostsim, pubs, sigs, msgs, offs, group)
    exp = np.array([v["valid"] for v in vs], np.uint8)
    bad = [vs[i]["class"] for i in np.nonzero(out != exp)[0]]
    assert not bad, bad


def test_finish_raw_cases_hostsim(hostsim):
    """The batched finish alone (hostsim_finish_raw: HostFin / host_finish with FinDev's perm indexing)
    on every case of tests/finish_cases.py at m <= 4,099, with G in {1, 2, 3, 16}, with and without a
    shuffled perm: every bit equals the Python-integer expectation, the Z = 0 rows are rejected
    without touching their lane's group, no byte outside the m decisions is written.  Every row's
    expectation is first recomputed from its limbs alone."""
    import finish_cases as FC
    fin_base = 64
    for m in (1, 17, 255, 256, 257, 4095, 4099):
        for G in (1, 2, 3, 16):
            if G > m or (m == 4099 and G == 16):  # L = 257 would repeat a pool's Z inside a group
                continue
            c = FC.case(m, 4099, G)
            if G == 1:  # (the bulk rows are the same for every G; the planted ones are expected this way anyhow)
                direct = [FC.direct_expected(row[:10], row[10:20], row[20:], bytes(rb), bit)
                          for row, rb, bit in zip(c["xyz"].tolist(), c["r"], c["bits_in"])]
                assert (np.array(direct, np.uint8) == c["exp"]).all()
            for base, perm in ((0, None), (fin_base, None), (0, FC.shuffled_perm(m, 0, m + G)),
                               (fin_base, FC.shuffled_perm(m, fin_base, m - G))):
                out = np.zeros(base + m, np.uint8)
                rc = hostsim.hostsim_finish_raw(ctypes.c_uint32(m), _p(c["xyz"]), _p(c["r"]),
                                                None if perm is None else _p(perm), ctypes.c_uint32(base),
                                                _p(c["bits_in"]), _p(out), ctypes.c_uint32(G))
                assert rc == 0
                FC.check(c, out, base, perm)
                FC.check_guards(c, out, base, perm)


def test_sign_matches_oracle(hostsim):
    rng = np.random.default_rng(2)
    n = 96
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = rng.integers(0, 260, n)
    offs = np.zeros(n + 1, np.uint32)
    offs[1:] = np.cumsum(lens)
    msgs = rng.integers(0, 256, int(offs[-1]) + 1, dtype=np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    pub = np.zeros((n, 32), np.uint8)
    hostsim.hostsim_sign_batch(_p(seeds), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(sig), _p(pub))
    for i in range(n):
        m = msgs[offs[i]:offs[i + 1]].tobytes()
        assert sig[i].tobytes() == port.sign(seeds[i].tobytes(), m)
        assert pub[i].tobytes() == port.pubkey_from_seed(seeds[i].tobytes())


@pytest.mark.parametrize("fn", ["hostsim_verify_comb_batch", "hostsim_verify_comb_batch16", "hostsim_verify_comb_lat"])
def test_comb_path_hostsim(hostsim, golden, fn):
    """Key-cached (radix-256 comb) verification, host build of the kernel code, vs the oracle:
    golden tuples grouped by key (incl. small-order, non-canonical and undecodable keys).
    _lat: latency mode (8 partial comb sums + cross-lane tree, strict R decode + projective
    compare instead of the inversion) — covers the non-canonical / off-curve / x=0-sign R
    classes of the golden set."""
    per = {}
    for v in golden:  # up to 5 tuples of every edge class, so each R / A / S class is hit
        if len(v["sig"]) == 128 and len(per.setdefault(v["class"], [])) < 5:
            per[v["class"]].append(v)
    vs = [v for c in sorted(per) for v in per[c]]
    keys = sorted({v["pub"] for v in vs})
    kidx = {k: i for i, k in enumerate(keys)}
    karr = np.array([np.frombuffer(bytes.fromhex(k), np.uint8) for k in keys])
    idx = np.array([kidx[v["pub"]] for v in vs], np.uint32)
    sigs = np.array([np.frombuffer(bytes.fromhex(v["sig"]), np.uint8) for v in vs])
    ms = [bytes.fromhex(v["msg"]) for v in vs]
    offs = np.zeros(len(vs) + 1, np.uint32)
    offs[1:] = np.cumsum([len(m) for m in ms])
    msgs = np.frombuffer(b"".join(ms) + b"\0", np.uint8)
    out = np.zeros(len(vs), np.uint8)
    getattr(hostsim, fn)(_p(karr), ctypes.c_size_t(len(keys)), _p(idx), _p(sigs), _p(msgs), _p(offs),
                         ctypes.c_size_t(len(vs)), _p(out))
    exp = np.array([v["valid"] for v in vs], np.uint8)
    assert (out == exp).all(), [vs[i]["class"] for i in np.nonzero(out != exp)[0]]
    assert exp.sum() > 10 and (exp == 0).sum() > 10


def _halfsize(fn, k):
    c, d = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    neg = ctypes.c_int()
    W = fn(k.to_bytes(32, "little"), c, d, ctypes.byref(neg))
    ci, di = int.from_bytes(c.raw, "little"), int.from_bytes(d.raw, "little")
    return ci, -di if neg.value else di, W


def test_halfsize_lattice(hostsim):
    """verify_hs.h sc_halfsize: c = d k (mod 8L), d odd, both within the window count's range
    (|x| < 2^(4W-1), the top digit taking the recoding's carry); W = 64 only for the (k, 1)
    fallback; typical W is 32..33."""
    ks, n_edge = PC.halfsize_lattice_ks()
    ws = []
    for k in ks:
        ci, di, W = _halfsize(hostsim.hostsim_halfsize, k)
        PC.check_halfsize(k, ci, di, W)
        ws.append(W)
    rand = ws[n_edge:]
    assert max(rand) <= 36 and sum(rand) / len(rand) < 32.8


def test_halfsize_lattice_at_the_quotient_edges(hostsim):
    """The same invariants where the Euclid steps are borderline: first quotients around the
    2^32 - 2 limit of hs_euclid_step, tiny first remainders (an out-of-range second quotient, the
    even-cofactor adjustment, the (k, 1) fallback) and long runs of quotients 1 and 2."""
    assert len(PC.halfsize_quotient_ks()) == 41 and len(PC.halfsize_long_euclid_ks()) == 300
    for k in PC.halfsize_long_euclid_ks():
        q = PC.euclid_quotients(k)
        assert q[0] >= 8 and all(x in (1, 2) for x in q[1:1 + PC.LONG_EUCLID_MIN]), k
    fallbacks = 0
    for k in PC.halfsize_edge_ks():
        ci, di, W = _halfsize(hostsim.hostsim_halfsize, k)
        PC.check_halfsize(k, ci, di, W)
        fallbacks += W == 64
    assert 0 < fallbacks < 41  # the fallback is reached, and only by quotient-edge values


def test_halfsize_torsion_keys(hostsim):
    """The half-size equation multiplies by d modulo the full group order 8L, so keys with a
    torsion component keep the reference's cofactorless decision: A = A0 + T (T of order 2, 4
    or 8) with R = [r]B - [k]T (valid) or R = [r]B (invalid unless [k]T = 0)."""
    rng = random.Random(9)
    small = E.small_order_points()
    pubs, sigs, msgs, exp = [], [], [], []
    for i in range(96):
        a = rng.randrange(1, E.L)
        T = small[i % 8]
        A = E.pt_add(E.pt_mul(a, E.BASE), T)
        pub = E.encode(A)
        m = rng.randbytes(40)
        r = rng.randrange(1, E.L)
        for mode in range(2):
            R0 = E.pt_mul(r, E.BASE)
            # k depends on R's bytes: pick R first, then S = r + k a (mod L)
            R = R0
            if mode == 0:
                # R = [r]B - [k]T requires k: iterate once with the k of the torsion-corrected R
                for _ in range(4):
                    Rb = E.encode(R)
                    k = int.from_bytes(hashlib.sha512(Rb + pub + m).digest(), "little") % E.L
                    R_new = E.pt_add(R0, E.pt_neg(E.pt_mul(k, T)))
                    if E.encode(R_new) == Rb:
                        break
                    R = R_new
            Rb = E.encode(R)
            k = int.from_bytes(hashlib.sha512(Rb + pub + m).digest(), "little") % E.L
            S = (r + k * a) % E.L
            pubs.append(pub)
            sigs.append(Rb + S.to_bytes(32, "little"))
            msgs.append(m)
            exp.append(1 if E.verify(pub, m, sigs[-1]) else 0)
    n = len(pubs)
    P = np.array([np.frombuffer(p, np.uint8) for p in pubs])
    Sg = np.array([np.frombuffer(s, np.uint8) for s in sigs])
    offs = np.zeros(n + 1, np.uint32)
    offs[1:] = np.cumsum([len(m) for m in msgs])
    M = np.frombuffer(b"".join(msgs) + b"\0", np.uint8)
    out = _verify(hostsim, P, Sg, M, offs, "hs")
    assert (out == np.array(exp, np.uint8)).all()
    assert 0 < sum(exp) < n


def test_halfsize_fast_euclid_equals_reference_loop(hostsim):
    """verify_hs.h's two-steps-per-iteration Euclid phase (in-place, roles swapping) must stop at
    exactly the same remainder as the round-1 loop, so (c, d, W, tight W) are equal on every k —
    random k, the boundary values of the lattice test and the quotient-edge / long-run families."""
    for k in PC.halfsize_euclid_ks() + PC.halfsize_edge_ks():
        out = []
        for fast in (1, 0):
            c, d = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
            neg, tight = ctypes.c_int(), ctypes.c_int()
            W = hostsim.hostsim_halfsize_tight(k.to_bytes(32, "little"), c, d, ctypes.byref(neg), ctypes.byref(tight),
                                               fast)
            out.append((W, c.raw, d.raw, neg.value, tight.value))
        assert out[0] == out[1], k
        assert 29 <= out[0][4] <= out[0][0], k


def test_halfsize_top_digit_and_wave_max(hostsim):
    """Random signatures through the half-size path (host build of verify_hs.h): with each lane's
    own tight W (x < 2^(4W): the top digit carries the recoding's overflow, digits up to 16, added
    as two table entries) and with W raised above it, as in a wave whose largest W exceeds the
    lane's; one flipped bit of S or of the message makes each invalid.  Decisions equal the
    oracle's C port; the tight count puts ~88 % of the lanes at 32 windows (the latency kernels'
    count, x < 2^(4W-1), ~40 %)."""
    rng = np.random.default_rng(17)
    n = 1536
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    offs = (np.arange(n + 1) * 110).astype(np.uint32)
    msgs = rng.integers(0, 256, int(offs[-1]) + 1, dtype=np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    pub = np.zeros((n, 32), np.uint8)
    hostsim.hostsim_sign_batch(_p(seeds), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(sig), _p(pub))
    sig[1::5, 40] ^= 4        # S changed
    msgs[offs[3:n:7]] ^= 1    # message changed
    exp = port.verify_batch(pub, sig, msgs, offs.astype(np.uint64), 8)
    assert 0 < exp.sum() < n
    wins = np.zeros(n, np.int32)
    for extra in (None, 1, 3):
        out = np.zeros(n, np.uint8)
        wmin = None if extra is None else _p(wins + extra)
        hostsim.hostsim_verify_batch_hs_w(_p(pub), _p(sig), _p(msgs), _p(offs), ctypes.c_size_t(n), _p(out),
                                          _p(wins) if extra is None else None, wmin)
        assert (out == exp).all(), (extra, np.nonzero(out != exp)[0][:8])
    assert wins.min() >= 29 and (wins == 32).sum() > n * 3 // 4 and wins.max() <= 34, np.bincount(wins)


def _fe_raw(l, op, a0, b0, a1=None, b1=None, alias=0):
    """(limbs, value) of hostsim_fe_raw (the single products), or that pair for both products of
    hostsim_fe_raw_x2 (the two-product schedules)."""
    A = lambda c: (ctypes.c_int32 * 10)(*c)
    o0, o1 = (ctypes.c_int32 * 10)(), (ctypes.c_int32 * 10)()
    e0, e1 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    if op < PC.FE_MUL_X2:
        l.hostsim_fe_raw(op, A(a0), A(b0), o0, e0)
        return list(o0), int.from_bytes(e0.raw, "little")
    l.hostsim_fe_raw_x2(op, alias, A(a0), A(b0), A(a1), A(b1), o0, e0, o1, e1)
    return (list(o0), int.from_bytes(e0.raw, "little")), (list(o1), int.from_bytes(e1.raw, "little"))


def _check_product(got, exp, what):
    limbs, value = got
    assert value == exp % E.P, what
    for i in range(10):
        assert PC.in_carried_output_range(i, limbs[i]), (what, i, limbs[i])


def test_fused_carry_at_the_limb_extremes(hostsim):
    """fe_mul / fe_sq (3-sum inputs), fe_sq2 and fe_sqc (carried input) at the ends of the carried
    limb ranges (fe25519.h: even limbs [-2^25, 2^25), odd [0, 2^25), limb 1 [-2^16, 2^25 + 2^16),
    and fe_carry's odd [-2^24, 2^24]): the result is the product mod p and its limbs are carried."""
    val = PC.limb_val
    for a, b in PC.fused_pairs():
        ops = [(PC.FE_MUL, val(a) * val(b)), (PC.FE_SQ, val(a) ** 2)]
        if PC.is_carried(a):
            ops += [(PC.FE_SQ2, 2 * val(a) ** 2), (PC.FE_SQC, val(a) ** 2)]
        for op, exp in ops:
            got = _fe_raw(hostsim, op, a, b)
            _check_product(got, exp, (op, a, b))
    # fe_sq2 and fe_sqc on carried inputs at the extremes
    for a in PC.fused_carried():
        for op, exp in ((PC.FE_SQ2, 2 * val(a) ** 2), (PC.FE_SQC, val(a) ** 2)):
            got = _fe_raw(hostsim, op, a, a)
            _check_product(got, exp, (op, a))


@pytest.mark.parametrize("alias", [0, 1, 2, 3])
def test_fused_pair_schedules_at_the_limb_extremes(hostsim, alias):
    """The two-product schedules at the same extremes, within the input bounds fe25519.h states:
    fe_mul_x2 and fe_sq_x2 on 3-sums, fe_sqc_x2 on carried values, fe_sq2_sq on a carried and a
    3-sum operand; one operand set all-low beside the other all-high, and both sets equal.  Each
    result is its product mod p with carried limbs, with separate outputs (alias 0) and with the
    outputs written over the inputs (1: own first input, 2: own last input, 3: the other product's
    first input), which fe25519.h promises to work."""
    val = PC.limb_val
    for a0, b0, a1, b1 in PC.fused_pair_sets():
        what = (alias, a0, b0, a1, b1)
        r0, r1 = _fe_raw(hostsim, PC.FE_MUL_X2, a0, b0, a1, b1, alias)
        _check_product(r0, val(a0) * val(b0), ("fe_mul_x2", 0) + what)
        _check_product(r1, val(a1) * val(b1), ("fe_mul_x2", 1) + what)
        r0, r1 = _fe_raw(hostsim, PC.FE_SQ_X2, a0, b0, a1, b1, alias)
        _check_product(r0, val(a0) ** 2, ("fe_sq_x2", 0) + what)
        _check_product(r1, val(a1) ** 2, ("fe_sq_x2", 1) + what)
    carried = PC.carried_pair_sets()
    sums = PC.fused_pair_sets()
    for j, (a0, a1) in enumerate(carried):
        r0, r1 = _fe_raw(hostsim, PC.FE_SQC_X2, a0, a0, a1, a1, alias)
        _check_product(r0, val(a0) ** 2, ("fe_sqc_x2", 0, alias, a0, a1))
        _check_product(r1, val(a1) ** 2, ("fe_sqc_x2", 1, alias, a0, a1))
        s = sums[j % len(sums)][2 * (j % 2)]  # a 3-sum second operand (the extremes come first)
        r0, r1 = _fe_raw(hostsim, PC.FE_SQ2_SQ, a0, a0, s, s, alias)
        _check_product(r0, 2 * val(a0) ** 2, ("fe_sq2_sq", 0, alias, a0, s))
        _check_product(r1, val(s) ** 2, ("fe_sq2_sq", 1, alias, a0, s))


@pytest.mark.parametrize("B", [10, 11, 12])
def test_radix_2_b_key_comb_digits(B):
    """The key-cached throughput kernel's signed radix-2^B digits of k (kernels.hip
    keyset_straus_ab24, kernels.h kCombA*; B = 12 by default), restated: W = floor(253 / B) windows;
    digit m < W - 1 is bits [Bm, Bm + B) + bit (Bm - 1) - 2^B * bit (Bm + B - 1), in
    [-2^(B-1), 2^(B-1)]; the top digit (m = W - 1) is every bit left + the bit below, unsigned, in
    [0, kCombATopMax] (B = 12: bits 240..252, [0, 4097]) — inside the comb's top window.  Sum of
    digit_m * 2^(Bm) = k for every k < L, including k in [2^252, L) where bit 252 is set."""
    L = 2**252 + 27742317777372353535851937790883648493
    W = 253 // B
    top_field = 253 - B * (W - 1)
    top_max = (1 << (top_field - 1)) + 1           # kernels.h kCombATopMax
    top_rows = ((top_max + 127) // 128) * 128 + 1  # kCombATopEntries
    mask = (1 << B) - 1
    rng = random.Random(11 + B)
    ks = [rng.randrange(L) for _ in range(3000)] + [L - 1, L - 2, 2**252, 2**252 + 12345, 0, 1, 2**241,
                                                     2**252 - 1, (2**253 - 1) % L, 2**240 - 1, 2**252 - 2**239]
    for k in ks:
        w = [(k >> (32 * i)) & 0xffffffff for i in range(8)]
        digits = []
        u = w[0] & mask
        digits.append(u - ((u >> (B - 1)) << B))
        for m in range(W - 1):
            below = (w[0] >> (B - 1)) & 1
            w = [((w[i] >> B) | (w[i + 1] << (32 - B))) & 0xffffffff for i in range(7)] + [w[7] >> B]
            last = m + 2 == W
            u = w[0] if last else w[0] & mask
            top = 0 if last else (u >> (B - 1)) << B
            digits.append(u + below - top)
        assert len(digits) == W
        h = 1 << (B - 1)
        assert all(-h <= d <= h for d in digits[:-1]) and 0 <= digits[-1] <= top_max < top_rows, (k, digits)
        assert sum(d << (B * m) for m, d in enumerate(digits)) == k, k
