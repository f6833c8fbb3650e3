"""The joint radix-4 table of the half-size main kernel on the device: decisions of
verify_main_hs_kernel (the throughput kernels, TMED_GLAT_MAX=0) through tmed_verify_batch against
the oracle's port on small batches around a wave's size — valid signatures of the C2 stream, one
tuple of every C5 class and the golden edge vectors — a wave mixing window counts 32 and 33, and
the twelve rows build_table_joint stores per lane (tmed_test_joint_rows) against the host build of
the same source (tests/native/joint_host.cpp).  A wave holding the (k, 1) fallback lane (W = 64),
which no signature's hash reaches, runs on the device at a chosen k: tests/test_gpu_hs_k.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import ed25519_go as E
from oracle import port
from tmed._native import lib
from tmed.workload import SMALL_ORDER, c2_messages, c2_seeds, c5_mix

pytestmark = pytest.mark.gpu

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
N_C2 = 600  # c5_mix at 1 %: six tuples, one of each class


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def pool(generic_engines, golden):
    """(pubs, sigs, msgs, offs, expected): the six C5 tuples first, then the golden vectors with a
    64-byte signature, then the untouched C2 signatures; expected by the port, computed once."""
    eng = generic_engines["throughput"]
    seeds = c2_seeds(0, N_C2)
    msgs, offs = c2_messages(0, N_C2)
    sigs, pubs = eng.sign_arrays(seeds, np.concatenate([msgs, np.zeros(16, np.uint8)]), offs)
    idx = c5_mix(pubs, sigs, frac=0.01)
    assert len(idx) == 6
    order = list(idx) + [i for i in range(N_C2) if i not in set(idx.tolist())]
    gv = [v for v in golden if len(v["sig"]) == 128 and len(v["pub"]) == 64]
    assert len(gv) > 500
    P, S, M = [], [], []
    for i in order[:6]:
        P.append(pubs[i].tobytes()); S.append(sigs[i].tobytes()); M.append(msgs[offs[i]:offs[i + 1]].tobytes())
    for v in gv:
        P.append(bytes.fromhex(v["pub"])); S.append(bytes.fromhex(v["sig"])); M.append(bytes.fromhex(v["msg"]))
    for i in order[6:]:
        P.append(pubs[i].tobytes()); S.append(sigs[i].tobytes()); M.append(msgs[offs[i]:offs[i + 1]].tobytes())
    n = len(P)
    pa = np.frombuffer(b"".join(P), np.uint8).reshape(n, 32).copy()
    sa = np.frombuffer(b"".join(S), np.uint8).reshape(n, 64).copy()
    o = np.zeros(n + 1, np.uint64)
    o[1:] = np.cumsum([len(m) for m in M])
    ma = np.frombuffer(b"".join(M) + bytes(16), np.uint8).copy()
    exp = port.verify_batch(pa, sa, ma, o, 8)
    gold = np.array([v["valid"] for v in gv], np.uint8)
    assert (exp[6:6 + len(gv)] == gold).all()
    assert exp[:6].sum() <= 1 and exp[6 + len(gv):].all()  # (a flipped message bit leaves the signature valid)
    return pa, sa, ma, o, exp


def _verify_slice(eng, pool, lo, n):
    pa, sa, ma, o, exp = pool
    offs = (o[lo:lo + n + 1] - o[lo]).astype(np.uint32)
    msgs = ma[int(o[lo]):int(o[lo + n]) + 16]
    out = eng.verify_arrays(pa[lo:lo + n], sa[lo:lo + n], msgs, offs)
    bad = np.nonzero(out != exp[lo:lo + n])[0]
    assert bad.size == 0, (lo, n, bad[:10].tolist())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_batches_equal_the_port(generic_engines, pool, n):
    """Batches of n from the head of the pool (C5 classes and edge vectors), from its tail (valid C2
    signatures) and across the seam between the two."""
    eng = generic_engines["throughput"]
    total = pool[0].shape[0]
    seam = total - (N_C2 - 6)
    for lo in (0, total - n, max(0, seam - n // 2)):
        _verify_slice(eng, pool, lo, n)


def test_every_edge_vector_in_one_batch(generic_engines, pool):
    eng = generic_engines["throughput"]
    _verify_slice(eng, pool, 0, pool[0].shape[0])


def test_a_wave_mixing_window_counts(generic_engines, pool):
    """64 signatures of the C2 stream in one wave, taken from the stream until lanes of W = 32 and
    of W = 33 both occur (tmed_window_stats): the wave runs 33 windows, its W = 32 lanes with a top
    window above their own."""
    eng = generic_engines["throughput"]
    total = pool[0].shape[0]
    for lo in range(total - (N_C2 - 6), total - 64, 64):
        _verify_slice(eng, pool, lo, 64)
        lh, wh = eng.window_stats()
        assert int(lh.sum()) == 64 and int(wh.sum()) == 1
        if lh[32] > 0 and lh[33] > 0:
            assert int(wh[32]) == 0
            return
    raise AssertionError("no 64 consecutive C2 signatures with W = 32 and W = 33 lanes")


def _triples():
    """(A, R, dneg) encodings: random points, A = +-R, small orders, the identity, encodings that do
    not decode (the kernels then run on the identity) — more than one wave, a partial last block."""
    rng = np.random.default_rng(0x7ab1e)
    pts = [E.pt_mul(int.from_bytes(rng.bytes(32), "little") % E.L, E.BASE) for _ in range(24)]
    enc = [E.encode(p) for p in pts]
    bad = next(y.to_bytes(32, "little") for y in range(2, 50) if E.decode(y.to_bytes(32, "little")) is None)
    tr = []
    for k in range(40):
        tr.append((enc[k % 24], enc[(5 * k + 1) % 24], k & 1))
    for k in range(8):
        tr.append((enc[k], enc[k], k & 1))
        tr.append((enc[k], E.encode(E.pt_neg(pts[k])), k & 1))
        tr.append((SMALL_ORDER[k], enc[k], k & 1))
        tr.append((enc[k], SMALL_ORDER[k], (k >> 1) & 1))
        tr.append((SMALL_ORDER[k], SMALL_ORDER[(3 * k + 1) % 8], k & 1))
    tr.append((bad, enc[0], 0))
    tr.append((enc[1], bad, 1))
    tr.append(((E.P + 3).to_bytes(32, "little"), enc[2], 0))  # non-canonical y, decoded permissively
    assert len(tr) > 64 and len(tr) % 64 != 0
    return tr


def test_device_rows_equal_host_rows(generic_engines):
    """The twelve packed rows of every lane, byte for byte (the same integer arithmetic on both
    sides; the host rows are checked against the point code in tests/test_joint_table_host.py)."""
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "joint_host.mk"])
    jh = ctypes.CDLL(os.path.join(NATIVE, "libjointhost.so"))
    tr = _triples()
    n = len(tr)
    a = np.frombuffer(b"".join(t[0] for t in tr), np.uint8).copy()
    r = np.frombuffer(b"".join(t[1] for t in tr), np.uint8).copy()
    dn = np.array([t[2] for t in tr], np.uint8)
    rows = np.zeros((n, 12 * 128), np.uint8)
    rc = lib().tmed_test_joint_rows(generic_engines["throughput"]._h, _p(a), _p(r), _p(dn), n, _p(rows))
    assert rc == 0, rc
    for i, (ae, re_, d) in enumerate(tr):
        host = ctypes.create_string_buffer(12 * 128)
        jh.jointhost_rows(ae, re_, int(d), host)
        got = rows[i].tobytes()
        for j in range(12):
            assert got[128 * j:128 * j + 128] == host.raw[128 * j:128 * j + 128], (i, j)
