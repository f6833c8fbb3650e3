"""The group layer on the device: tests/native/devprim.hip (a TEST-ONLY harness, never part of the
product library) runs the point formulas of ge25519.h and the group helpers of verify_core.h one
case per lane (devprim_ge), and quad.h — the DPP quad-lane formulas of the latency kernels' main
loop and of zip_final_kernel's Horner chain, code that exists on the device only — one case per
quad of lanes (devprim_quad), on the cases of tests/group_cases.py: free limb vectors at the ends
of the ranges each function's magnitude contract allows, curve points (exceptional pairs
included) in non-canonical limbs, and chains of doublings and additions that pass through the
identity.  Every comparison is exact, against Python integers and oracle.ed25519_go."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import group_cases as GC
import prim_cases as PC
from oracle import ed25519_go as E

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
SZ = ctypes.c_size_t
HIP_ERROR_INVALID_VALUE = 1


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
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ok(rc, what):
    assert rc == 0, "%s: HIP error %d" % (what, rc)


def _i32(x):
    return np.ascontiguousarray(np.array(x, dtype=np.int64).astype(np.int32))


def _ints(arr):
    return [int.from_bytes(r.tobytes(), "little") for r in arr]


def _ge(lib, op, negs, ins):
    """devprim_ge over the cases (one launch per neg value): per case (limbs[4][10], values[4])."""
    n = len(ins)
    assert n > 64 and n % 64 != 0, n  # a partial last block (the kernel guards i < n)
    res = [None] * n
    for neg in sorted(set(negs)):
        idx = [i for i in range(n) if negs[i] == neg]
        if len(idx) % 64 == 0:
            idx.append(idx[0])
        a = _i32([ins[i] for i in idx])
        assert a.shape == (len(idx), 8, 10)
        out, enc = np.zeros((len(idx), 4, 10), np.int32), np.zeros((len(idx), 4, 32), np.uint8)
        _ok(lib.devprim_ge(op, neg, SZ(len(idx)), _p(a), _p(out), _p(enc)), GC.GE_NAMES[op])
        for j, i in enumerate(idx):
            res[i] = (out[j].tolist(), _ints(enc[j]))
    return res


def _quad(lib, op, v, q, window=None, dg=None, prog=None, lone=False):
    """devprim_quad over the cases: per case out[4][10]."""
    n = len(v)
    assert lone or n % 16 != 0, n  # a partial last block of 16 quads
    a = _i32([list(x) + list(y) for x, y in zip(v, q)])
    assert a.shape == (n, 8, 10)
    out = np.zeros((n, 4, 10), np.int32)
    nrows = 0 if window is None else len(window)
    _ok(lib.devprim_quad(op, SZ(n), _p(a), _p(window), SZ(nrows), _p(dg), _p(prog), _p(out)), GC.Q_NAMES[op])
    return out.tolist()


def _fe_raw(lib, op, a0, b0, a1, b1):
    n = len(a0)
    assert n > 64 and n % 64 != 0, n
    A0, B0, A1, B1 = _i32(a0), _i32(b0), _i32(a1), _i32(b1)
    o0, o1 = np.zeros((n, 10), np.int32), np.zeros((n, 10), np.int32)
    e0, e1 = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    _ok(lib.devprim_fe_raw(op, 0, SZ(n), _p(A0), _p(B0), _p(A1), _p(B1), _p(o0), _p(e0), _p(o1), _p(e1)),
        PC.FE_RAW_NAMES[op])
    return list(zip(o0.tolist(), _ints(e0))), list(zip(o1.tolist(), _ints(e1)))


def _check_product(got, exp, what):
    limbs, value = got
    assert value == exp % E.P, what
    for i in range(10):
        assert PC.in_carried_output_range(i, limbs[i]), (what, i, limbs[i])


def test_fe_mul_takes_a_4sum_first_operand_gpu(devprim):
    """fe_mul and fe_mul_x2 (the asm schedules fe_mul_fused, fe_mul_fused_x2) with a 4-sum in the f
    slot, the operand quad_dbl passes as F = B - A - 2C: product mod p, carried limbs."""
    val = PC.limb_val
    pairs = PC.fused_4sum_pairs()
    n = len(pairs)
    f, g = [p[0] for p in pairs], [p[1] for p in pairs]
    f1, g1 = [f[(j + 7) % n] for j in range(n)], [g[(j + 7) % n] for j in range(n)]
    r0, _ = _fe_raw(devprim, PC.FE_MUL, f, g, f, g)
    for x, y, got in zip(f, g, r0):
        _check_product(got, val(x) * val(y), ("fe_mul", x, y))
    r0, r1 = _fe_raw(devprim, PC.FE_MUL_X2, f, g, f1, g1)
    for j in range(n):
        _check_product(r0[j], val(f[j]) * val(g[j]), ("fe_mul_x2", 0, f[j], g[j], f1[j], g1[j]))
        _check_product(r1[j], val(f1[j]) * val(g1[j]), ("fe_mul_x2", 1, f[j], g[j], f1[j], g1[j]))


@pytest.mark.parametrize("op", sorted(GC.GE_WIDTHS), ids=lambda op: GC.GE_NAMES[op])
def test_ge_formulas_at_the_limb_extremes_gpu(devprim, op):
    """The host test of the same name, on the device build of the formulas."""
    cases = GC.ge_formula_cases(op)
    res = _ge(devprim, op, [c[0] for c in cases], [c[1] for c in cases])
    for (neg, ins), (limbs, encs) in zip(cases, res):
        GC.check_ge_formula(op, neg, ins, limbs, encs)


@pytest.mark.parametrize("op", range(10), ids=lambda op: GC.GE_NAMES[op])
def test_ge_ops_on_curve_points_gpu(devprim, op):
    """The host test of the same name, on the device build."""
    cases = GC.ge_real_cases(op)
    res = _ge(devprim, op, [c[0] for c in cases], [c[1] for c in cases])
    for (neg, ins, exp), (limbs, encs) in zip(cases, res):
        GC.check_ge_real(op, neg, ins, exp, limbs, encs)


@pytest.mark.parametrize("op", [GC.Q_DBL, GC.Q_ADD, GC.Q_TO_CACHED], ids=lambda op: GC.Q_NAMES[op])
def test_quad_formulas_at_the_limb_extremes_gpu(devprim, op):
    """quad_dbl, quad_add and quad_to_cached as polynomial identities on free limb vectors, lane r
    of a quad holding coordinate r: the four products (E F, G H, F G, E H) mod p with carried
    limbs; quad_dbl never reads T (garbage at the int32 extremes); F is the doubling's 4-sum."""
    cases = GC.quad_formula_cases(op)
    out = _quad(devprim, op, [c[0] for c in cases], [c[1] for c in cases])
    for (v, q), o in zip(cases, out):
        GC.check_quad_formula(op, v, q, o)


@pytest.mark.parametrize("op", [GC.Q_DBL, GC.Q_ADD, GC.Q_TO_CACHED], ids=lambda op: GC.Q_NAMES[op])
def test_quad_ops_on_curve_points_gpu(devprim, op):
    """The quad formulas on curve points against oracle.ed25519_go: doubling, P + Q and P - Q (the
    exchanged / negated cached lanes) over the exceptional pairs, and the cached form."""
    cases = GC.quad_real_cases(op)
    out = _quad(devprim, op, [c[0] for c in cases], [c[1] for c in cases])
    for (v, q, exp), o in zip(cases, out):
        GC.check_quad_real(op, v, q, exp, o)


def test_quad_identities_and_a_lone_quad_gpu(devprim):
    """quad_identity / quad_identity_cached lane by lane, and one launch with n = 1: a lone active
    quad beside 60 idle lanes, as in zip_final_kernel."""
    z4 = ((GC.ZERO,) * 4,) * 21
    one, two = (1,) + (0,) * 9, (2,) + (0,) * 9
    for o in _quad(devprim, GC.Q_IDENTITY, z4, z4):
        assert [tuple(x) for x in o] == [GC.ZERO, one, one, GC.ZERO]
    for o in _quad(devprim, GC.Q_IDENTITY_CACHED, z4, z4):
        assert [tuple(x) for x in o] == [one, one, GC.ZERO, two]
    for op in (GC.Q_DBL, GC.Q_ADD):
        v, q, exp = GC.quad_real_cases(op)[-2]
        (o,) = _quad(devprim, op, [v], [q], lone=True)
        GC.check_quad_real(op, v, q, exp, o)
    a, b, prog, exp = GC.chain_cases()[0]
    (o,) = _quad(devprim, GC.Q_CHAIN, [a], [b], prog=np.array([prog], np.uint32), lone=True)
    GC.check_extended([GC.val(c) % GC.P for c in o], o, exp, ("lone chain", prog))


def test_comb_take_gpu(devprim):
    """comb_take on a synthetic window: digit 0, +-j for every row and the largest row; lanes
    (YmX, YpX, XY2d, 2) of row |j|, or (YpX, YmX, -XY2d, 2) for a negative digit, limbs equal
    exactly (row limbs at the int32 extremes, where the negation wraps).  A digit outside the
    window is refused before the launch."""
    rows, digits = GC.comb_take_cases()
    n = len(digits)
    z4 = ((GC.ZERO,) * 4,) * n
    window, dg = _i32(rows), _i32(digits)
    assert window.shape == (GC.COMB_ROWS, 32)
    out = _quad(devprim, GC.Q_COMB_TAKE, z4, z4, window=window, dg=dg)
    for d, o in zip(digits, out):
        assert [tuple(x) for x in o] == [tuple(x) for x in GC.comb_take_expected(rows[abs(d)], d)], d
    bad = dg.copy()
    bad[3] = GC.COMB_ROWS
    a, o = np.zeros((n, 8, 10), np.int32), np.zeros((n, 4, 10), np.int32)
    rc = devprim.devprim_quad(GC.Q_COMB_TAKE, SZ(n), _p(a), _p(window), SZ(len(rows)), _p(bad), None, _p(o))
    assert rc == HIP_ERROR_INVALID_VALUE


def test_quad_chains_on_curve_points_gpu(devprim):
    """Chains from quad_identity: steps of 4 (and 16) doublings and + Q / - Q / nothing, the shape
    of the loops of verify_glat_main_kernel and zip_final_kernel, against oracle.ed25519_go;
    programs whose accumulator passes through the identity mid-chain (+Q then -Q, an order-8
    point doubled three times, an order-4 point); the final limbs are carried."""
    cases = GC.chain_cases()
    prog = np.array([c[2] for c in cases], np.uint32)
    assert prog.shape == (len(cases), GC.CHAIN_STEPS)
    out = _quad(devprim, GC.Q_CHAIN, [c[0] for c in cases], [c[1] for c in cases], prog=prog)
    for (a, b, pr, exp), o in zip(cases, out):
        GC.check_extended([GC.val(c) % GC.P for c in o], o, exp, ("chain", pr, a))
