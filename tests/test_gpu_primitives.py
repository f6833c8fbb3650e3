"""The kernels' building blocks on the device, at their edges: tests/native/devprim.hip (a
TEST-ONLY harness, never part of the product library) runs fe25519.h / fe_cols.h, sc25519.h,
sha512.h, verify_hs.h and ge25519.h on the GPU, one case per lane, on the inputs the host suite
uses (tests/prim_cases.py).  The device compiles other branches of that source than the host
build does — the inline-asm v_mad_i64_i32 schedules and v_add_u32 doubling, the carry-chain
builtins, the v_rcp_f64 quotient estimate, SHA-512's constant table, alignbit / bitop3 forms,
v_perm message reader and slot stream — so every comparison here is against Python integers,
hashlib and oracle.ed25519_go, exact."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import prim_cases as PC
from oracle import ed25519_go as E

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def devprim():
    """libdevprim.so, (re)made when the compiler is there; its absence is a failure, not a skip."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if os.path.exists(hipcc):
        subprocess.check_call(["make", "-s", "-C", NATIVE, "libdevprim.so"])
    path = os.path.join(NATIVE, "libdevprim.so")
    assert os.path.exists(path), "tests/native/libdevprim.so is missing: make -C tests/native"
    return ctypes.CDLL(path)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _lanes(n):
    """Case counts must leave a partial last block (the kernels guard i < n)."""
    assert n > 64 and n % 64 != 0, n
    return n


def _ok(rc, what):
    assert rc == 0, "%s: HIP error %d" % (what, rc)


def _bytes_arr(vals, width):
    return np.frombuffer(b"".join(v.to_bytes(width, "little") for v in vals), np.uint8).reshape(len(vals), width).copy()


def _ints(arr):
    return [int.from_bytes(r.tobytes(), "little") for r in arr]


def _limbs(cases):
    return np.ascontiguousarray(np.array(cases, dtype=np.int64).astype(np.int32))


def _fe_raw(lib, op, a0, b0, a1, b1, alias=0):
    """Per case ((limbs, value), (limbs, value)) of devprim_fe_raw over the operand lists."""
    n = _lanes(len(a0))
    A0, B0, A1, B1 = _limbs(a0), _limbs(b0), _limbs(a1), _limbs(b1)
    o0, o1 = np.zeros((n, 10), np.int32), np.zeros((n, 10), np.int32)
    e0, e1 = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    _ok(lib.devprim_fe_raw(op, alias, SZ(n), _p(A0), _p(B0), _p(A1), _p(B1), _p(o0), _p(e0), _p(o1), _p(e1)),
        PC.FE_RAW_NAMES[op])
    return list(zip(o0.tolist(), _ints(e0))), list(zip(o1.tolist(), _ints(e1)))


def _check_product(got, exp, what):
    limbs, value = got
    assert value == exp % E.P, what
    for i in range(10):
        assert PC.in_carried_output_range(i, limbs[i]), (what, i, limbs[i])


def test_fe_products_at_the_limb_extremes_gpu(devprim):
    """fe_mul / fe_sq on 3-sums, fe_sq2 / fe_sqc on carried values (the asm schedules fe_mul_fused,
    fe_sq1_fused, fe_sq2_fused, fe_sq1c_fused and dbl32): product mod p, carried limbs."""
    val = PC.limb_val
    pairs = PC.fused_pairs()
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    for op, exp in ((PC.FE_MUL, lambda x, y: val(x) * val(y)), (PC.FE_SQ, lambda x, y: val(x) ** 2)):
        r0, _ = _fe_raw(devprim, op, a, b, a, b)
        for x, y, g in zip(a, b, r0):
            _check_product(g, exp(x, y), (PC.FE_RAW_NAMES[op], x, y))
    c = list(PC.fused_carried())
    for op, mult in ((PC.FE_SQ2, 2), (PC.FE_SQC, 1)):
        r0, _ = _fe_raw(devprim, op, c, c, c, c)
        for x, g in zip(c, r0):
            _check_product(g, mult * val(x) ** 2, (PC.FE_RAW_NAMES[op], x))


@pytest.mark.parametrize("alias", [0, 1, 2, 3])
def test_fe_pair_schedules_at_the_limb_extremes_gpu(devprim, alias):
    """fe_mul_x2, fe_sq_x2 (3-sums), fe_sqc_x2 (carried), fe_sq2_sq (carried, 3-sum): the asm
    schedules fe_mul_fused_x2, fe_sq1_fused_x2, fe_sq1c_fused_x2, fe_sq2_sq1_fused, with separate
    outputs and with the outputs written over the inputs (see the host test of the same name)."""
    val = PC.limb_val
    sets = PC.fused_pair_sets()
    a0, b0, a1, b1 = ([s[k] for s in sets] for k in range(4))
    r0, r1 = _fe_raw(devprim, PC.FE_MUL_X2, a0, b0, a1, b1, alias)
    for s, g0, g1 in zip(sets, r0, r1):
        _check_product(g0, val(s[0]) * val(s[1]), ("fe_mul_x2", 0, alias) + s)
        _check_product(g1, val(s[2]) * val(s[3]), ("fe_mul_x2", 1, alias) + s)
    r0, r1 = _fe_raw(devprim, PC.FE_SQ_X2, a0, b0, a1, b1, alias)
    for s, g0, g1 in zip(sets, r0, r1):
        _check_product(g0, val(s[0]) ** 2, ("fe_sq_x2", 0, alias) + s)
        _check_product(g1, val(s[2]) ** 2, ("fe_sq_x2", 1, alias) + s)
    carried = PC.carried_pair_sets()
    c0, c1 = [c[0] for c in carried], [c[1] for c in carried]
    r0, r1 = _fe_raw(devprim, PC.FE_SQC_X2, c0, c0, c1, c1, alias)
    for x, y, g0, g1 in zip(c0, c1, r0, r1):
        _check_product(g0, val(x) ** 2, ("fe_sqc_x2", 0, alias, x, y))
        _check_product(g1, val(y) ** 2, ("fe_sqc_x2", 1, alias, x, y))
    s3 = [sets[j % len(sets)][2 * (j % 2)] for j in range(len(carried))]  # 3-sum second operands
    r0, r1 = _fe_raw(devprim, PC.FE_SQ2_SQ, c0, c0, s3, s3, alias)
    for x, y, g0, g1 in zip(c0, s3, r0, r1):
        _check_product(g0, 2 * val(x) ** 2, ("fe_sq2_sq", 0, alias, x, y))
        _check_product(g1, val(y) ** 2, ("fe_sq2_sq", 1, alias, x, y))


def test_fe_byte_ops_vs_bigint_gpu(devprim):
    """The ten ops of the host's test_field_ops_vs_bigint on the same 931 pairs: products, both
    inversions, the (p-5)/8 power, add / sub with fe_carry, 3-sum inputs."""
    pairs = PC.field_byte_pairs()
    n = _lanes(len(pairs))
    a, b = _bytes_arr([p[0] for p in pairs], 32), _bytes_arr([p[1] for p in pairs], 32)
    exp = [PC.field_byte_expected(x, y) for x, y in pairs]
    for op in range(10):
        out = np.zeros((n, 32), np.uint8)
        _ok(devprim.devprim_fe_bytes(op, SZ(n), _p(a), _p(b), _p(out)), "fe_bytes %d" % op)
        for (x, y), e, g in zip(pairs, exp, _ints(out)):
            assert g == e[op], (op, hex(x), hex(y))


def test_inversions_gpu(devprim):
    """fe_invert_bgcd and fe_invert equal z^(p-2) on the host test's inputs (every bit length,
    powers of two and neighbours, values near p and 0)."""
    vals = PC.bgcd_values()
    n = _lanes(len(vals))
    a = _bytes_arr([v % 2**255 for v in vals], 32)
    for op in (9, 2):
        out = np.zeros((n, 32), np.uint8)
        _ok(devprim.devprim_fe_bytes(op, SZ(n), _p(a), _p(a), _p(out)), "fe_bytes %d" % op)
        for v, g in zip(vals, _ints(out)):
            assert g == pow(v % 2**255 % E.P, E.P - 2, E.P), (op, hex(v))


def test_pack256_roundtrip_at_the_limb_extremes_gpu(devprim):
    cases, g = PC.pack256_cases()
    n = _lanes(len(cases))
    limbs = _limbs(cases)
    gs = _bytes_arr([g] * n, 32)
    out, prod = np.zeros((n, 10), np.int32), np.zeros((n, 32), np.uint8)
    _ok(devprim.devprim_pack256(SZ(n), _p(limbs), _p(gs), _p(out), _p(prod)), "pack256")
    for c, u, pr in zip(cases, out.tolist(), _ints(prod)):
        PC.check_pack256(c, u, pr, g)


def test_sc_reduce512_gpu(devprim):
    """sc_reduce512 (addc32 / subb32 as the carry-chain builtins) on digests, the extremes and the
    multiples of L with their neighbours, where Barrett's quotient is one below."""
    vals = PC.sc_reduce_values()
    n = _lanes(len(vals))
    x = _bytes_arr(vals, 64)
    out = np.zeros((n, 32), np.uint8)
    _ok(devprim.devprim_sc_reduce(SZ(n), _p(x), _p(out)), "sc_reduce")
    for v, g in zip(vals, _ints(out)):
        assert g == v % E.L, hex(v)


def test_sc_is_canonical_and_muladd_gpu(devprim):
    vals = PC.sc_canonical_values()
    n = _lanes(len(vals))
    s = _bytes_arr(vals, 32)
    ok = np.zeros(n, np.uint8)
    _ok(devprim.devprim_sc_is_canonical(SZ(n), _p(s), _p(ok)), "sc_is_canonical")
    for v, g in zip(vals, ok.tolist()):
        assert bool(g) == (v < E.L), hex(v)
    cases = PC.sc_muladd_cases()
    n = _lanes(len(cases))
    a, b, c = (_bytes_arr([t[k] for t in cases], 32) for k in range(3))
    out = np.zeros((n, 32), np.uint8)
    _ok(devprim.devprim_sc_muladd(SZ(n), _p(a), _p(b), _p(c), _p(out)), "sc_muladd")
    for (x, y, z), g in zip(cases, _ints(out)):
        assert g == (x * y + z) % E.L, (hex(x), hex(y), hex(z))


def test_halfsize_equals_the_reference_loop_gpu(devprim, hostsim):
    """sc_halfsize<true> on the device (quotients from v_rcp_f64 and one Newton step) on every k of
    the host's lattice and Euclid tests and the quotient-edge and long-run families: the lattice
    invariants, and (c, d, dneg, W, tight W) equal to the host's reference loop (IEEE division) —
    quot_estimate's claim that the caller corrects the floor exactly, whatever the estimate."""
    ks = PC.halfsize_lattice_ks()[0] + PC.halfsize_euclid_ks() + PC.halfsize_edge_ks()
    n = _lanes(len(ks))
    kb = _bytes_arr(ks, 32)
    c, d = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    neg, W, tight = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _ok(devprim.devprim_halfsize(SZ(n), _p(kb), _p(c), _p(d), _p(neg), _p(W), _p(tight)), "halfsize")
    hc, hd = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    hneg, htight = ctypes.c_int(), ctypes.c_int()
    differ = []
    for i, k in enumerate(ks):
        ci, di = int.from_bytes(c[i].tobytes(), "little"), int.from_bytes(d[i].tobytes(), "little")
        PC.check_halfsize(k, ci, -di if neg[i] else di, int(W[i]))
        hW = hostsim.hostsim_halfsize_tight(k.to_bytes(32, "little"), hc, hd, ctypes.byref(hneg), ctypes.byref(htight), 0)
        got = (c[i].tobytes(), d[i].tobytes(), int(neg[i]), int(W[i]), int(tight[i]))
        if got != (hc.raw, hd.raw, hneg.value, hW, htight.value):
            differ.append(k)
    assert not differ, (len(differ), [hex(k) for k in differ[:8]])


def test_sha512_stream_gpu(devprim):
    """sha512_stream of p0 || p1 || M with 0, 32 and 64 prefix bytes: every length 0..300 and the
    block-boundary lengths at each dword misalignment of M (the v_perm reader), one buffer."""
    p0, p1, buf, offs, lens = PC.sha512_stream_cases()
    n = _lanes(len(lens))
    for r in range(4):  # every misalignment meets short, one-block-boundary and multi-block messages
        ls = {l for o, l in zip(offs, lens) if o % 4 == r}
        assert {0, 1, 111, 112, 113, 239, 240, 241, 400} <= ls, r
    a0, a1 = np.frombuffer(b"".join(p0), np.uint8).copy(), np.frombuffer(b"".join(p1), np.uint8).copy()
    b = np.frombuffer(buf, np.uint8).copy()
    off, ln = np.array(offs, np.uint32), np.array(lens, np.uint32)
    for npre in (0, 32, 64):
        out = np.zeros((n, 64), np.uint8)
        _ok(devprim.devprim_sha512(SZ(n), npre, _p(a0), _p(a1), _p(b), SZ(len(buf)), _p(off), _p(ln), _p(out)), "sha512")
        for i in range(n):
            m = buf[offs[i]:offs[i] + lens[i]]
            assert out[i].tobytes() == hashlib.sha512((p0[i] + p1[i])[:npre] + m).digest(), (npre, offs[i] % 4, lens[i])


def test_sha512_stream_slot_gpu(devprim):
    """sha512_stream_slot (dwordx4 loads of a 256-byte slot; a third block falls back to the
    stream): every message length 0..256, bytes of the slot past the message ignored."""
    p0, p1, buf, _, _ = PC.sha512_stream_cases()
    n = _lanes(257)
    slots = np.frombuffer((buf * (1 + 256 * n // len(buf)))[:256 * n], np.uint8).copy()
    a0, a1 = np.frombuffer(b"".join(p0[:n]), np.uint8).copy(), np.frombuffer(b"".join(p1[:n]), np.uint8).copy()
    ln = np.arange(n, dtype=np.uint32)
    out = np.zeros((n, 64), np.uint8)
    _ok(devprim.devprim_sha512_slot(SZ(n), _p(a0), _p(a1), _p(slots), _p(ln), _p(out)), "sha512_slot")
    for i in range(n):
        m = slots[256 * i:256 * i + i].tobytes()
        assert out[i].tobytes() == hashlib.sha512(p0[i] + p1[i] + m).digest(), i


def test_decode_matches_go_rule_gpu(devprim):
    cands = PC.decode_candidates()
    n = _lanes(len(cands))
    p = np.frombuffer(b"".join(cands), np.uint8).copy()
    ok, enc = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    _ok(devprim.devprim_decode(SZ(n), _p(p), _p(ok), _p(enc)), "decode")
    for i, c in enumerate(cands):
        pt = E.decode(c)
        assert bool(ok[i]) == (pt is not None), c.hex()
        if pt is not None:
            assert enc[i].tobytes() == E.encode(pt), c.hex()
