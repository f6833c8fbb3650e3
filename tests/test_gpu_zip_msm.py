"""The ZIP-215 batch mode's multi-scalar multiplication, stage by stage (csrc/zip215.hip zip_msm: the
column sums of c, the two-pass counting sort, zip_accum_kernel's bucket ownership, the bucket
weights, the three-level wavefront reduction, the final check), through tmed_test_zip_msm: the
product's own launches on the product's scratch, over rows and digits the test chooses.

Every expected value is an oracle.ed25519_go integer (tests/zip_msm_cases.py): window w must equal
sum_i digit[w][i] (-P_i) over the rows of the group only, as an affine point with a consistent T;
ctot must equal sum c_i mod L; the flag must say whether [8](sum_w 2^(16 w) W_w + [ctot] B) = O.
All comparisons are exact."""
import numpy as np
import pytest

import zip_msm_cases as ZC
from oracle import ed25519_go as E
from tmed._native import TMED_EINVAL, TmedError

pytestmark = pytest.mark.gpu


def run(engine, case):
    pts, dig, c = ZC.case_arrays(case)
    return engine.zip_msm(pts, dig, c, case["lo"], case["cnt"])


def check(engine, case, name="", want=None):
    """One zip_msm call against the integers: 16 windows, ctot, flag."""
    win, ctot, flag = run(engine, case)
    want = ZC.expected_windows(case) if want is None else want
    bad = [w for w in range(ZC.WIN) if not ZC.same_point(ZC.device_point(win[w]), want[w])]
    assert not bad, (name, "windows", bad, [int(v) for w in bad for v in case["dig"][w][:4]])
    got_c = sum(int(v) << (32 * i) for i, v in enumerate(ctot))
    assert got_c == ZC.expected_ctot(case), (name, "ctot", hex(got_c))
    assert flag == ZC.expected_flag(case), (name, "flag", flag)
    return win, ctot, flag


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("rows_kind", ["A", "R"])
def test_one_hot_digits(engine, rows_kind, flip):
    """One non-zero digit per window at every magnitude where the bucket's owner changes (lane,
    wave, block, reduction level, sort byte), both signs, on the A rows and on the R rows."""
    for k, case in enumerate(ZC.onehot_cases(rows_kind, flip)):
        check(engine, case, "one-hot %s flip=%d k=%d" % (rows_kind, flip, k))


def test_digit_pairs(engine):
    """Two rows per window whose digits share a low byte (0x0101 against 0x0201), share a high byte
    or lie on either side of a boundary, in both row orders."""
    for k, case in enumerate(ZC.pair_cases()):
        check(engine, case, "pairs k=%d" % k)


@pytest.mark.parametrize("lane0", [5, 64, 256])
def test_weighted_bucket_sums(engine, lane0):
    """All g buckets of three neighbouring lanes filled with distinct points (T = sum q B_q), around
    lane 5, the wave boundary (lanes 63..65) and the block boundary (lanes 255..257); the top
    window's buckets with runs of 1, 2, 3 and 5 entries split between its two lanes.  At lane 5 the
    expected values are also computed by per-row scalar multiplication and sum."""
    case = ZC.weighted_case(lane0)
    want = ZC.expected_windows(case)
    if lane0 == 5:
        per_row = ZC.expected_windows_per_row(case)
        assert all(E.pt_equal(a, b) for a, b in zip(want, per_row))
    check(engine, case, "weighted lane0=%d" % lane0, want)


def test_runs(engine):
    """130 rows share one digit per window while the lanes beside it are empty (the wave-uniform trip
    count, the prefetch of row i + 1 and entry i + 2); the run holds P then -P, the same point
    twice, the identity, small-order and mixed-order points."""
    case = ZC.run_case()
    check(engine, case, "runs")
    # and every prefix length of the run's head: 1, 2 (P - P = O), 3, 4 (the doubled point), 5, ...
    for cnt in (1, 2, 3, 4, 5, 9, 12, 65, 129):
        check(engine, dict(case, cnt=cnt), "runs cnt=%d" % cnt)


@pytest.mark.parametrize("cnt", ZC.SORT_CNTS)
def test_sort_boundaries(engine, cnt):
    """Entry counts that end at, or one past, a sort tile (4096 entries) and the four-tile block of
    zip_sort_hist_kernel, with digits from at most 40 values so equal keys span tiles."""
    case = ZC.sort_case(cnt)
    assert len(np.unique(np.abs(case["dig"].astype(np.int32)))) <= 40
    check(engine, case, "sort cnt=%d" % cnt)


def test_sub_ranges(engine):
    """(lo, cnt) groups of a chunk of 300 whose every row has non-zero digits and c: the windows and
    ctot are those of the group alone."""
    for lo, cnt in ZC.SUB_RANGES:
        check(engine, ZC.subrange_case(lo, cnt), "sub-range (%d, %d)" % (lo, cnt))


def test_small_group_after_a_large_one(engine):
    """A group of 8193 directly followed by groups of 3 on the same context: keys, values and
    histograms of the large sort lie beyond the new range."""
    check(engine, ZC.sort_case(8193), "large")
    check(engine, ZC.subrange_case(5, 3), "3 of 300 after 8193")
    check(engine, ZC.sort_case(8193), "large again")
    big = ZC.sort_case(8193)
    check(engine, dict(big, lo=4000, cnt=3), "3 of 8193 after 8193")
    check(engine, ZC.subrange_case(0, 3, n=3, seed=3), "chunk of 3 after 8193")


def test_ctot(engine):
    for name, case in ZC.ctot_cases():
        win, ctot, flag = check(engine, case, "ctot " + name, want=[E.IDENTITY] * ZC.WIN)
        assert sum(int(v) << (32 * i) for i, v in enumerate(ctot)) < ZC.L


def test_flag(engine):
    for name, case, flag in ZC.flag_cases():
        assert check(engine, case, "flag " + name)[2] == flag, name


def test_contract_errors(engine):
    """Outside the product's contract: a top A digit outside 0..4097, a group outside the chunk, a
    row that does not decode."""
    case = ZC.subrange_case(0, 3, n=3, seed=3)
    for bad in (-1, 4098):
        dig = case["dig"].copy()
        dig[15, 1] = bad
        pts, _, c = ZC.case_arrays(case)
        with pytest.raises(TmedError) as ei:
            engine.zip_msm(pts, dig, c, 0, 3)
        assert ei.value.code == TMED_EINVAL
    pts, dig, c = ZC.case_arrays(case)
    for lo, cnt in ((0, 0), (0, 4), (3, 1), (2, 2)):
        with pytest.raises(TmedError) as ei:
            engine.zip_msm(pts, dig, c, lo, cnt)
        assert ei.value.code == TMED_EINVAL
    off = pts.copy()
    y = 2
    while E.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    off[4] = np.frombuffer(y.to_bytes(32, "little"), np.uint8)
    with pytest.raises(TmedError) as ei:
        engine.zip_msm(off, dig, c, 0, 3)
    assert ei.value.code == TMED_EINVAL
    check(engine, case, "after the errors")
