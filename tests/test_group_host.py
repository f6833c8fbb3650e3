"""The group layer on the host build (tests/native/hostsim.cpp, hostsim_ge): the point formulas of
ge25519.h and the group helpers of verify_core.h, one call per case, on the cases of
tests/group_cases.py — free limb vectors at the ends of the ranges each function's magnitude
contract allows, and curve points (exceptional pairs included) in non-canonical limbs — and
fe_mul with a 4-sum first operand, the allowance quad.h's doubling uses.  Every comparison is
exact, against Python integers and oracle.ed25519_go.  tests/test_gpu_group.py runs the same cases
on the device, where other branches of the field code are compiled."""
import ctypes
import os
import sys

import pytest

import group_cases as GC
import prim_cases as PC
from oracle import ed25519_go as E

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


def _ge(l, op, neg, ins):
    """(limbs[4][10], values[4]) of hostsim_ge on one case."""
    flat = (ctypes.c_int32 * 80)(*[x for c in ins for x in c])
    out = (ctypes.c_int32 * 40)()
    enc = ctypes.create_string_buffer(128)
    assert l.hostsim_ge(op, neg, flat, out, enc) == 0, op
    o = list(out)
    return [o[10 * k:10 * k + 10] for k in range(4)], [int.from_bytes(enc.raw[32 * k:32 * k + 32], "little") for k in range(4)]


def _fe_raw(l, op, a0, b0, a1=None, b1=None):
    A = lambda c: (ctypes.c_int32 * 10)(*c)
    o0, o1 = (ctypes.c_int32 * 10)(), (ctypes.c_int32 * 10)()
    e0, e1 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    if op < PC.FE_MUL_X2:
        l.hostsim_fe_raw(op, A(a0), A(b0), o0, e0)
        return list(o0), int.from_bytes(e0.raw, "little")
    l.hostsim_fe_raw_x2(op, 0, A(a0), A(b0), A(a1), A(b1), o0, e0, o1, e1)
    return (list(o0), int.from_bytes(e0.raw, "little")), (list(o1), int.from_bytes(e1.raw, "little"))


def _check_product(got, exp, what):
    limbs, value = got
    assert value == exp % E.P, what
    for i in range(10):
        assert PC.in_carried_output_range(i, limbs[i]), (what, i, limbs[i])


def test_fe_mul_takes_a_4sum_first_operand(hostsim):
    """fe25519.h: fe_mul's f operand may be a sum of FOUR carried values (g at most three) — what
    quad_dbl passes as F = B - A - 2C.  The schedule's bounds with nsum_a = 4, nsum_b = 3 (every
    pre-multiplied copy inside int32, the worst column inside the tool's limit), then fe_mul and
    fe_mul_x2 (the 4-sums in both f slots) at the all-extreme pairs and 300 draws: product mod p,
    carried limbs."""
    sys.path.insert(0, TOOLS)
    try:
        import gen_fe_asm
    finally:
        sys.path.remove(TOOLS)
    worst = gen_fe_asm.check_bounds(gen_fe_asm.mul_products(), 4, 3)
    assert worst < 2**62.5
    with pytest.raises(AssertionError):  # the allowance is one-sided: a 4-sum g leaves int32
        gen_fe_asm.check_bounds(gen_fe_asm.mul_products(), 3, 4)
    val = PC.limb_val
    pairs = PC.fused_4sum_pairs()
    n = len(pairs)
    for j, (f, g) in enumerate(pairs):
        _check_product(_fe_raw(hostsim, PC.FE_MUL, f, g), val(f) * val(g), ("fe_mul", f, g))
        f1, g1 = pairs[(j + 7) % n]
        r0, r1 = _fe_raw(hostsim, PC.FE_MUL_X2, f, g, f1, g1)
        _check_product(r0, val(f) * val(g), ("fe_mul_x2", 0, f, g, f1, g1))
        _check_product(r1, val(f1) * val(g1), ("fe_mul_x2", 1, f, g, f1, g1))


@pytest.mark.parametrize("op", sorted(GC.GE_WIDTHS), ids=lambda op: GC.GE_NAMES[op])
def test_ge_formulas_at_the_limb_extremes(hostsim, op):
    """Each point formula as a polynomial identity on free limb vectors at the width its contract
    allows, all-low and all-high in every slot: every output coordinate's canonical value, and
    every output limb inside the range the function's comment promises."""
    for neg, ins in GC.ge_formula_cases(op):
        limbs, encs = _ge(hostsim, op, neg, ins)
        GC.check_ge_formula(op, neg, ins, limbs, encs)


@pytest.mark.parametrize("op", range(10), ids=lambda op: GC.GE_NAMES[op])
def test_ge_ops_on_curve_points(hostsim, op):
    """Every addition, doubling and conversion on curve points in non-canonical limbs against
    oracle.ed25519_go: P + P through the addition formulas, P + (-P), the identity on either side,
    small-order + large; extended outputs have Z != 0 and T Z = X Y; ge_p3_to_niels returns exactly
    the affine (y + x, y - x, 2dxy)."""
    for neg, ins, exp in GC.ge_real_cases(op):
        limbs, encs = _ge(hostsim, op, neg, ins)
        GC.check_ge_real(op, neg, ins, exp, limbs, encs)


def test_hostsim_ge_rejects_an_unknown_op(hostsim):
    flat, out, enc = (ctypes.c_int32 * 80)(), (ctypes.c_int32 * 40)(), ctypes.create_string_buffer(128)
    assert hostsim.hostsim_ge(10, 0, flat, out, enc) == -1


def test_case_generators_cover_what_they_claim():
    """The quad and chain generators run only on the device; their own coverage assertions (the
    extremes in every slot, partial last blocks, the exceptional programs) hold here too."""
    for op in (GC.Q_DBL, GC.Q_ADD, GC.Q_TO_CACHED):
        assert len(GC.quad_formula_cases(op)) >= 900
        assert len(GC.quad_real_cases(op)) % 16 != 0
    rows, digits = GC.comb_take_cases()
    assert len(digits) == 2 * len(rows) - 1
    assert len(GC.chain_cases()) % 16 != 0
    assert GC.split_limbs(E.P // 3, True) is not None and GC.split_limbs(2**255) is None
