"""The ZIP-215 finish of the key-cached routes on the device (csrc/zip_finish.hip
keyset_finish_zip_kernel, launch_finish_zip; csrc/zip_finish.h zip_finish_one) through
tmed_test_finish_zip215, which fills the context's own fin buffer in fin_store's layout and runs the
product's launcher.  The rows are tests/zip_finish_cases.py's, the same arrays the host build decides
in tests/test_zip_finish_host.py: P = R, P = R + T for every small-order T, P = R + Q, every
non-canonical R that decodes, R off the curve, Z = 0 planted with X = 0, bits_in = 0, limbs at the
ends of the carried range, the golden ZIP-215 tuples.  Sizes around one wave (63, 64, 65), one block
(255, 256, 257) and 4,099 (17 blocks, the last one partial); with and without a shuffled perm; with
fin_base 0 and 4096; bytes no position owns stay 0xAA."""
import numpy as np
import pytest

import zip_finish_cases as ZC
from tmed._native import TmedError

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.mark.parametrize("m", ZC.SIZES)
def test_finish_zip215_rows(engine, m):
    c = ZC.case(m)
    for base in (0, 4096):
        for perm in (None, ZC.shuffled_perm(m, base, 100 + m + base)):
            out = engine.finish_zip215(c["xyz"], c["r"], c["bits_in"], base, perm)
            ZC.check(c, out, base, perm)


def test_every_planted_kind_runs_on_the_device(engine):
    """The largest case holds every planted row once (the small ones rotate through them)."""
    c = ZC.case(ZC.SIZES[-1])
    assert set(n for n, *_ in ZC.planted()) <= set(c["names"])
    out = engine.finish_zip215(c["xyz"], c["r"], c["bits_in"])
    for p, name in enumerate(c["names"]):
        assert out[p] == c["exp"][p], "%s (position %d): the device gives %d" % (name, p, out[p])


def test_default_finish_still_compares_encodings(engine):
    """The same rows through tmed_test_finish: the Go rule's finish accepts P = R + T only for T the
    identity, so the two entries differ exactly where the rules do."""
    pl = [r for r in ZC.planted() if r[0].startswith("P = R + T, T of order")]
    xyz = np.array([xl + yl + zl for _, xl, yl, zl, _, _, _ in pl], np.int32)
    r = np.frombuffer(b"".join(rb for _, _, _, _, rb, _, _ in pl), np.uint8).reshape(len(pl), 32)
    bits = np.ones(len(pl), np.uint8)
    go = engine.finish(xyz, r, bits)
    zp = engine.finish_zip215(xyz, r, bits)
    assert zp.tolist() == [1] * 8
    assert go.tolist() == [int(n.endswith("order 1")) for n, *_ in pl]


def test_finish_zip215_refuses_bad_shapes(engine):
    c = ZC.case(64)
    bad_perm = ZC.shuffled_perm(64, 0, 1).copy()
    bad_perm[5] = 64
    for base, perm in ((2 * (1 << 20) - 32, None), (0, bad_perm)):
        with pytest.raises(TmedError) as e:
            engine.finish_zip215(c["xyz"], c["r"], c["bits_in"], base, perm)
        assert e.value.code == EINVAL
    with pytest.raises(TmedError):
        engine.finish_zip215(np.zeros((0, 30), np.int32), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8))
