"""GPU: every row of the fixed-base tables of B and of a key set's combs.

A batch reads these tables at scalar-chosen rows, so decisions sample them: a window's last row, or
the rows beside the d0 >= 32768 carry of b26_fill_kernel / b24_fill_kernel, come up about once in
2^16 to 2^26 signatures.  Here the device checks each table whole (tmed_test_table_chain: row (w, 0)
the identity, row (w, j) = row (w, j - 1) + row (w, 1), row (w + 1, 1) = 2^r row (w, 1)), and rows read
back (tmed_test_b_table_entry) are compared with j 2^(rw) B from Python integers: row (w, 1) of every
window, which the chain hangs from, and the rows where the fill kernels branch.  With the chain these
cover every row by induction.  A corrupted copy shows the chain check can fail."""
import os
import re

import numpy as np
import pytest

from conftest import engine_with_env
from test_gpu_btables import _golden_arrays, _limbs_to_int, _niels

pytestmark = pytest.mark.gpu

BCOMB, B16, BCOMB16, B26, B24 = range(5)


def _kernels_h():
    """The table constants of kernels.h, evaluated from its text."""
    path = os.path.join(os.path.dirname(__file__), "..", "tendermint-fork_amd", "csrc", "kernels.h")
    with open(path) as f:
        text = f.read()
    out = {}
    for name in ("kCombWindows", "kCombEntries", "kB16Entries", "kB26Entries", "kB24Windows", "kB24Entries"):
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, text)
        out[name] = eval(re.sub(r"(\d)u\b", r"\1", m.group(1)), {})
    out["kCombABits"] = int(re.search(r"#define TMED_COMBA_BITS (\d+)", text).group(1))
    return out


K = _kernels_h()
# (windows, rows per window, bits between windows) by table
SHAPE = {BCOMB: (K["kCombWindows"], K["kCombEntries"], 8), B16: (1, K["kB16Entries"], 16),
         BCOMB16: (16, K["kB16Entries"], 16), B26: (2, K["kB26Entries"], 128),
         B24: (K["kB24Windows"], K["kB24Entries"], 24)}
# a key's radix-2^12 comb (kernels.h kCombA*): W - 1 windows of 2^(B-1) + 1 rows and the top window
_AB = K["kCombABits"]
_AW = 253 // _AB
_ATOP = (((1 << (253 - _AB * (_AW - 1) - 1)) + 1 + 127) // 128) * 128 + 1
COMBA_ROWS = (_AW - 1) * ((1 << (_AB - 1)) + 1) + _ATOP


def test_constants_read_from_the_header():
    assert SHAPE == {BCOMB: (32, 129, 8), B16: (1, 32769, 16), BCOMB16: (16, 32769, 16),
                     B26: (2, (1 << 25) + 1, 128), B24: (11, (1 << 23) + 1, 24)}
    assert (_AB, _AW, _ATOP, COMBA_ROWS) == (12, 21, 4225, 20 * 2049 + 4225)


@pytest.fixture(scope="module")
def table_engines(golden, engine):
    """A default context and one without the radix-2^26 / 2^24 tables, each after one key-set load
    and one throughput batch (the load acquires the radix-2^24 comb, the batch builds the key set's
    radix-2^12 combs).  (`engine`: the session's context keeps the shared radix-2^26 tables alive.)"""
    vs, karr, idx, sigs, msgs, offs, exp = _golden_arrays(golden)
    es = {}
    for name, env in (("default", {}), ("radix16", {"TMED_B26": 0, "TMED_B24": 0})):
        eng = engine_with_env(TMED_GLAT_MAX=0, TMED_LAT_MAX=0, TMED_SLAB_SLOTS=4096, **env)
        h = eng.keyset_load(karr)
        out = eng.verify_keyset_arrays(h, idx, sigs, msgs, offs)
        assert (out == exp).all()
        es[name] = (eng, h, len(karr))
    yield es
    for eng, h, _ in es.values():
        eng.keyset_free(h)
        eng.close()


def _tables(name):
    return (BCOMB, B16, BCOMB16, B26, B24) if name == "default" else (BCOMB, B16, BCOMB16)


@pytest.mark.parametrize("name", ["default", "radix16"])
def test_chain_holds_on_every_b_table(table_engines, name):
    """No failing row, and as many rows checked as the header's constants imply (a kernel that
    skipped rows would not pass)."""
    eng = table_engines[name][0]
    assert (eng.b_window_bits(), eng.keyset_b_window_bits()) == ((26, 24) if name == "default" else (16, 16))
    for t in _tables(name):
        rows, bad, first = eng.table_chain(t)
        assert bad == 0, (t, bad, first)
        assert rows == SHAPE[t][0] * SHAPE[t][1], t


@pytest.mark.parametrize("name", ["default", "radix16"])
def test_chain_holds_on_the_key_combs(table_engines, golden, name):
    """Both combs of a key set of the golden keys: small-order, non-canonical and undecodable ones
    among them (an undecodable key's rows are all the identity)."""
    from oracle import ed25519_go as E
    eng, h, nkeys = table_engines[name]
    karr = _golden_arrays(golden)[1]
    pts = [E.decode(bytes(k)) for k in karr]
    assert any(p is None for p in pts) and any(p is not None and E.pt_equal(E.pt_mul(8, p), E.IDENTITY) for p in pts)
    rows, bad, first = eng.table_chain(handle=h, radix_bits=8)
    assert bad == 0, (bad, first)
    assert rows == nkeys * K["kCombWindows"] * K["kCombEntries"]
    if name == "default":
        assert eng.keyset_a_window_bits(h) == _AB
        rows, bad, first = eng.table_chain(handle=h, radix_bits=_AB)
        assert bad == 0, (bad, first)
        assert rows == nkeys * COMBA_ROWS
    else:
        assert eng.keyset_a_window_bits(h) == 8
        with pytest.raises(Exception):
            eng.table_chain(handle=h, radix_bits=_AB)  # never built on this context
    with pytest.raises(Exception):
        eng.table_chain(handle=h + 1000, radix_bits=8)
    with pytest.raises(Exception):
        eng.table_chain(handle=h, radix_bits=16)


def _anchor_js(t, w):
    windows, entries, _ = SHAPE[t]
    last = entries - 1
    js = {1, 2, 32767, 32768, 32769, 65535, 65536, 65537, last - 1, last}
    if t == B24:
        if w % 2:  # 24 w = 16 v + 8: J = 256 j crosses 2^15 at j = 128 and reaches 2^31 at j = 2^23
            js |= {127, 128, 129}
        if w == windows - 1:
            js |= {4096, 4097}
    return sorted(j for j in js if 1 <= j <= last)


@pytest.mark.parametrize("name", ["default", "radix16"])
def test_anchor_rows_equal_python_integers(table_engines, name):
    """Row (w, 1) of every window, and the rows the chain cannot vouch for alone or where the fill
    kernels branch, against j 2^(r w) B.  The radix-2^24 comb's window 10 is what the code makes it:
    j 2^240 B up to j = 32767 (S < L needs j <= 4097), the identity from 2^15 up."""
    from oracle import ed25519_go as E
    eng = table_engines[name][0]
    checked = 0
    for t in _tables(name):
        windows, entries, step = SHAPE[t]
        for w in range(windows):
            assert tuple(_limbs_to_int(eng.b_table_entry(t, w, 0)[10 * c:10 * c + 10]) % E.P for c in range(3)) == (1, 1, 0)
            for j in _anchor_js(t, w):
                row = eng.b_table_entry(t, w, j)
                got = tuple(_limbs_to_int(row[10 * c:10 * c + 10]) % E.P for c in range(3))
                if t == B24 and w == windows - 1 and j >= 32768:
                    assert got == (1, 1, 0), (t, w, j)
                else:
                    assert got == _niels(E.pt_mul(j << (step * w), E.BASE)), (t, w, j)
                checked += 1
    assert checked == (32 * 4 + 4 + 16 * 4 + (2 * 10 + 11 * 10 + 5 * 3 + 2 if name == "default" else 0))


@pytest.mark.parametrize("table,window,j", [(BCOMB, 0, 2), (BCOMB, 17, 64), (BCOMB, 31, 127),
                                            (B16, 0, 2), (B16, 0, 12345), (B16, 0, 32767),
                                            (BCOMB16, 0, 2), (BCOMB16, 7, 32766), (BCOMB16, 15, 32767)])
def test_chain_reports_a_corrupted_row(table_engines, table, window, j):
    """The negative control: one limb of row (w, j) of a copy off by one fails that row (against its
    predecessor) and the next (built on it), and nothing else."""
    eng = table_engines["default"][0]
    rows, bad, first = eng.table_chain(table, corrupt=(window, j))
    assert rows == SHAPE[table][0] * SHAPE[table][1]
    assert bad == 2 and set(first) == {(window, j), (window, j + 1)}, (bad, first)
    assert eng.table_chain(table)[1] == 0  # the table itself was not touched


def test_out_of_range_and_absent_tables_are_errors(table_engines):
    eng, eng16 = table_engines["default"][0], table_engines["radix16"][0]
    for t, (windows, entries, _) in SHAPE.items():
        eng.b_table_entry(t, windows - 1, entries - 1)
        for w, j in ((windows, 0), (windows - 1, entries), (0, 0xffffffff), (0xffffffff, 1)):
            with pytest.raises(Exception):
                eng.b_table_entry(t, w, j)
    for t in (-1, 5):
        with pytest.raises(Exception):
            eng.b_table_entry(t, 0, 0)
        with pytest.raises(Exception):
            eng.table_chain(t)
    for t in (B26, B24):  # absent on this context
        with pytest.raises(Exception):
            eng16.b_table_entry(t, 0, 1)
        with pytest.raises(Exception):
            eng16.table_chain(t)
        with pytest.raises(Exception):
            eng.table_chain(t, corrupt=(0, 2))  # the negative control copies a table: the small ones only
    with pytest.raises(Exception):
        eng.table_chain(BCOMB, corrupt=(32, 2))
    with pytest.raises(Exception):
        eng.table_chain(BCOMB, corrupt=(0, 129))
