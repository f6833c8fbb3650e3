"""Merkle proofs without a device: the restatement (proof_cases.py) against the reference's own
checks, the path arithmetic the host sizing and the kernels share (csrc/merkle_path.h) compiled for
the host against that restatement, the argument / sizing / ENOMEM behaviour of the four C-ABI calls
that runs before any device work, and the static check of the Go binding with its proof tests."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import proof_cases as P
from oracle import merkle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendermint-fork_amd", "csrc")
SMALL_TREES = list(range(0, 70)) + [127, 128, 129, 255, 256, 257, 300]


@pytest.fixture(scope="session")
def proofpath_host(tmp_path_factory):
    """tests/native/proofpath_host.cpp built into a temporary directory."""
    so = str(tmp_path_factory.mktemp("proofpath") / "libproofpath_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "proofpath_host.cpp"), "-o", so])
    l = ctypes.CDLL(so)
    l.pp_split_point.restype = ctypes.c_uint64
    l.pp_split_point.argtypes = [ctypes.c_uint64]
    l.pp_aunt_counts.restype = None
    l.pp_aunt_counts.argtypes = [ctypes.c_uint64, ctypes.c_void_p]
    l.pp_path.restype = ctypes.c_int
    l.pp_path.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint32),
                          ctypes.POINTER(ctypes.c_uint64)]
    l.pp_level_plan.restype = ctypes.c_uint32
    l.pp_level_plan.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_uint64)]
    return l


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _mutate(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


# ---- the restatement against crypto/merkle/tree_test.go:46-102 -------------------------------------

def test_restatement_empty_tree():
    root, proofs = P.proofs_from_byte_slices([])
    assert root.hex() == P.EMPTY_HASH and proofs == []


def test_restatement_hundred_items():
    rng = random.Random(100)
    items = [rng.randbytes(32) for _ in range(100)]
    root, proofs = P.proofs_from_byte_slices(items)
    assert root == M.hash_from_byte_slices(items) and len(proofs) == 100
    for i, item in enumerate(items):
        total, index, lh, aunts = proofs[i]
        assert (total, index) == (100, i)
        assert P.verify(root, item, total, index, lh, aunts) == P.PROOF_OK
        assert P.verify(root, item, total, index, lh, aunts + [rng.randbytes(32)]) == P.PROOF_ROOT_HASH
        assert P.verify(root, item, total, index, lh, aunts[:-1]) == P.PROOF_ROOT_HASH
        assert P.verify(root, _mutate(item), total, index, lh, aunts) == P.PROOF_LEAF_HASH
        assert P.verify(_mutate(root), item, total, index, lh, aunts) == P.PROOF_ROOT_HASH


def test_restatement_shapes_agree():
    """The aunt lists of trailsFromByteSlices have the shape computeHashFromAunts walks."""
    for n in SMALL_TREES:
        _, proofs = P.proofs_from_byte_slices([bytes([i & 255, i >> 8]) for i in range(n)])
        for total, index, _, aunts in proofs:
            assert len(aunts) == len(P.path_sides(index, total)), (index, total)


# ---- csrc/merkle_path.h on the host -----------------------------------------------------------------

def _path(l, index, total):
    d, mask = ctypes.c_uint32(77), ctypes.c_uint64(77)
    ok = l.pp_path(index, total, ctypes.byref(d), ctypes.byref(mask))
    return (d.value, mask.value) if ok else None


def _expected_path(index, total):
    sides = P.path_sides(index, total)
    return None if sides is None else (len(sides), sum(s << k for k, s in enumerate(sides)))


def test_path_header_small_totals(proofpath_host):
    """Every (index, total) with total <= 300, index = -1 and index = total included: the aunt counts
    of the level-wise rule and the (d, mask) walk equal the recursion's."""
    for total in range(0, 301):
        counts = np.full(total + 1, 99, np.uint32)
        proofpath_host.pp_aunt_counts(total, _p(counts))
        assert counts[total] == 99
        for index in range(-1, total + 1):
            exp = _expected_path(index, total)
            assert _path(proofpath_host, index, total) == exp, (index, total)
            if 0 <= index < total:
                assert counts[index] == exp[0], (index, total)
        if total >= 2:
            assert proofpath_host.pp_split_point(total) == M.split_point(total)


def test_path_header_large_totals(proofpath_host):
    for total in (1, 2, 3, 5, 6) + P.LARGE_TOTALS:
        assert proofpath_host.pp_split_point(max(total, 2)) == M.split_point(max(total, 2))
        for index in P.large_indexes(total) + (total, -1):
            assert _path(proofpath_host, index, total) == _expected_path(index, total), (index, total)
    assert _path(proofpath_host, 2 ** 63 - 2, 2 ** 63 - 1)[0] == 62
    assert _path(proofpath_host, 0, 2 ** 63 - 1) == (63, 0)
    for total in (0, -1, -2 ** 63):
        assert _path(proofpath_host, 0, total) is None


# ---- csrc/merkle_levels.h on the host: the plan walked as the kernels walk it -----------------------

PLAN_FORESTS = [[], [0], [1], [0, 0], [2], [3], [0, 1, 2, 3, 5, 0, 1, 33], [1, 257, 1]] + [[n] for n in range(71)]
CAP_LEVELS = 40


def _level_plan(l, counts):
    """(nlevels, lvl_off, tab rows, nodes) of csrc/merkle_levels.h for trees of counts leaves."""
    T = len(counts)
    c = np.asarray(counts, np.uint32)
    lvl_off = np.full(CAP_LEVELS, 2 ** 64 - 1, np.uint64)
    tab = np.full((CAP_LEVELS, T + 1), 2 ** 32 - 1, np.uint32)
    nodes = ctypes.c_uint64(0)
    nlevels = l.pp_level_plan(_p(c), T, CAP_LEVELS, _p(lvl_off), _p(tab), ctypes.byref(nodes))
    assert 1 <= nlevels <= 33
    return nlevels, [int(x) for x in lvl_off[:nlevels]], [[int(x) for x in r] for r in tab[:nlevels]], nodes.value


def _last_tree_at(base, ntrees, j):
    """The kernels' search: the last t with base[t] <= j (trees with nothing there are skipped)."""
    lo, hi = 0, ntrees
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if base[mid] <= j:
            lo = mid
        else:
            hi = mid
    return lo


def _build_levels(counts, nlevels, lvl_off, tab, leaf_hashes, nodes):
    """merkle_level_kernel, level by level, over one node buffer laid out by the plan."""
    T = len(counts)
    buf = [None] * nodes
    buf[:len(leaf_hashes)] = leaf_hashes
    for l in range(nlevels - 1):
        in_base, out_base = tab[l], tab[l + 1]
        for j in range(out_base[T]):
            t = _last_tree_at(out_base, T, j)
            k = j - out_base[t]
            c = in_base[t + 1] - in_base[t]
            src = lvl_off[l] + in_base[t] + 2 * k
            assert 2 * k < c, "an output node without an input"
            if 2 * k + 1 < c:
                buf[lvl_off[l + 1] + j] = hashlib.sha256(b"\x01" + buf[src] + buf[src + 1]).digest()
            else:
                buf[lvl_off[l + 1] + j] = buf[src]  # odd node promoted
    return buf


def _aunts(counts, nlevels, lvl_off, tab, buf, i, n_aunts):
    """merkle_aunts_kernel for leaf i, whose aunt range holds n_aunts hashes."""
    T = len(counts)
    t = _last_tree_at(tab[0], T, i)
    p = i - tab[0][t]
    out = []
    for l in range(nlevels):
        if len(out) >= n_aunts:
            break
        base, c = tab[l][t], tab[l][t + 1] - tab[l][t]
        if c <= 1:
            break
        if p ^ 1 < c:
            out.append(buf[lvl_off[l] + base + (p ^ 1)])
        p >>= 1
    return out


@pytest.mark.parametrize("counts", PLAN_FORESTS, ids=lambda c: "-".join(map(str, c)) or "none")
def test_level_plan_walked_as_the_kernels_do(proofpath_host, counts):
    """The plan of merkle_levels.h, walked in Python exactly as merkle_level_kernel, merkle_emit_kernel
    and merkle_aunts_kernel walk it: the last level holds HashFromByteSlices of every tree, the aunts
    are the restatement's, and the plan keeps its bounds (nodes <= 2 L + 32 T, nlevels <= 33)."""
    T, L = len(counts), sum(counts)
    trees, at = [], 0
    for n in counts:
        trees.append([b"leaf %d" % i + bytes(i % 5) for i in range(at, at + n)])
        at += n
    nlevels, lvl_off, tab, nodes = _level_plan(proofpath_host, counts)
    assert nodes <= 2 * L + 32 * T
    assert tab[0] == [sum(counts[:t]) for t in range(T + 1)] and lvl_off[0] == 0
    assert nodes == sum(r[T] for r in tab) and lvl_off == [sum(r[T] for r in tab[:l]) for l in range(nlevels)]
    leaf_hashes = [hashlib.sha256(b"\x00" + x).digest() for t in trees for x in t]
    buf = _build_levels(counts, nlevels, lvl_off, tab, leaf_hashes, nodes)
    assert None not in buf
    last = tab[nlevels - 1]
    for t, items in enumerate(trees):  # merkle_emit_kernel
        assert last[t + 1] - last[t] == (1 if items else 0)
        root = buf[lvl_off[nlevels - 1] + last[t]] if items else hashlib.sha256(b"").digest()
        assert root == M.hash_from_byte_slices(items), (t, len(items))
    i = 0
    for items in trees:
        n = len(items)
        sized = np.zeros(n + 1, np.uint32)
        proofpath_host.pp_aunt_counts(n, _p(sized))
        _, proofs = P.proofs_from_byte_slices(items)
        for p in range(n):
            assert proofs[p][2] == buf[i]  # Proof.LeafHash is the level-0 node
            assert _aunts(counts, nlevels, lvl_off, tab, buf, i, int(sized[p])) == proofs[p][3], (n, p)
            i += 1


# ---- the C ABI before the device ------------------------------------------------------------------

@pytest.fixture(scope="module")
def abi():
    from tmed.merkle import _bind
    return _bind()


FAKE = np.zeros(64, np.uint8)  # stands in for a context where the call returns before using one


def _forest():
    rng = random.Random(5)
    counts = [0, 1, 2, 0, 3, 5, 8, 13, 0]
    trees = [[rng.randbytes(rng.randrange(0, 9)) for _ in range(n)] for n in counts]
    flat = [x for t in trees for x in t]
    leaf_off = np.zeros(len(flat) + 1, np.uint64)
    leaf_off[1:] = np.cumsum([len(x) for x in flat])
    tree_off = np.zeros(len(counts) + 1, np.uint32)
    tree_off[1:] = np.cumsum(counts)
    data = np.frombuffer(b"".join(flat) + bytes(8), np.uint8)
    exp_off = [0]
    for t in trees:
        for _, _, _, aunts in P.proofs_from_byte_slices(t)[1]:
            exp_off.append(exp_off[-1] + len(aunts))
    return data, leaf_off, tree_off, exp_off


def test_sizing_calls_fill_offsets_on_the_host(abi):
    from tmed._native import TMED_OK
    data, leaf_off, tree_off, exp_off = _forest()
    L, T = len(leaf_off) - 1, len(tree_off) - 1
    need = ctypes.c_size_t(7)
    aunt_off = np.full(L + 1, 9, np.uint64)
    assert abi.tmed_merkle_proofs(_p(FAKE), _p(data), _p(leaf_off), _p(tree_off), T, None, None, _p(aunt_off), None, 0,
                                  ctypes.byref(need)) == TMED_OK
    assert list(aunt_off) == exp_off and need.value == 32 * exp_off[-1]
    # the same trees as transaction blocks: the shape does not depend on the leaves
    aunt_off[:] = 9
    assert abi.tmed_txs_proofs(_p(FAKE), _p(data), _p(leaf_off), _p(tree_off), T, None, None, _p(aunt_off), None, 0,
                               ctypes.byref(need)) == TMED_OK
    assert list(aunt_off) == exp_off and need.value == 32 * exp_off[-1]
    # part sets: 0, 1, 64, 65 and 1000 bytes at part size 64 -> 0, 1, 1, 2, 16 parts
    lens = [0, 1, 64, 65, 1000]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    blob = np.zeros(int(off[-1]) + 8, np.uint8)
    part_off = np.full(len(lens) + 1, 9, np.uint32)
    aunt_off = np.full(21, 9, np.uint64)
    assert abi.tmed_partset_proofs(_p(FAKE), _p(blob), _p(off), len(lens), 64, None, _p(part_off), None, _p(aunt_off),
                                   None, 0, ctypes.byref(need)) == TMED_OK
    assert list(part_off) == [0, 0, 1, 2, 4, 20]
    exp = [0, 0, 0, 1, 2] + [2 + 4 * k for k in range(1, 17)]
    assert list(aunt_off) == exp and need.value == 32 * exp[-1]


def test_small_buffer_is_enomem_and_writes_nothing(abi):
    from tmed._native import TMED_ENOMEM
    data, leaf_off, tree_off, exp_off = _forest()
    L, T = len(leaf_off) - 1, len(tree_off) - 1
    need = ctypes.c_size_t(7)
    aunt_off = np.full(L + 1, 9, np.uint64)
    roots = np.full((T, 32), 9, np.uint8)
    lh = np.full((L, 32), 9, np.uint8)
    aunts = np.full((exp_off[-1], 32), 9, np.uint8)
    for call in (abi.tmed_merkle_proofs, abi.tmed_txs_proofs):
        assert call(_p(FAKE), _p(data), _p(leaf_off), _p(tree_off), T, _p(roots), _p(lh), _p(aunt_off), _p(aunts),
                    32 * exp_off[-1] - 1, ctypes.byref(need)) == TMED_ENOMEM
    off = np.array([0, 1000], np.uint64)
    part_off = np.full(2, 9, np.uint32)
    assert abi.tmed_partset_proofs(_p(FAKE), _p(np.zeros(1008, np.uint8)), _p(off), 1, 64, _p(roots), _p(part_off),
                                   _p(lh), _p(aunt_off), _p(aunts), 32 * 64 - 1, ctypes.byref(need)) == TMED_ENOMEM
    assert need.value == 7 and (aunt_off == 9).all() and (roots == 9).all() and (lh == 9).all()
    assert (aunts == 9).all() and (part_off == 9).all()


def test_generators_einval(abi):
    from tmed._native import TMED_EINVAL, TMED_OK
    data, leaf_off, tree_off, _ = _forest()
    L, T = len(leaf_off) - 1, len(tree_off) - 1
    need = ctypes.c_size_t(0)
    aunt_off = np.zeros(L + 1, np.uint64)
    part_off = np.zeros(T + 1, np.uint32)

    def gen(call, ctx=_p(FAKE), d=_p(data), lo=leaf_off, to=tree_off, ao=_p(aunt_off), ln=ctypes.byref(need)):
        return call(ctx, d, None if lo is None else _p(lo), None if to is None else _p(to), T, None, None, ao, None,
                    0, ln)

    for call in (abi.tmed_merkle_proofs, abi.tmed_txs_proofs):
        assert gen(call) == TMED_OK
        assert gen(call, ctx=None) == TMED_EINVAL
        assert gen(call, lo=None) == TMED_EINVAL
        assert gen(call, to=None) == TMED_EINVAL
        assert gen(call, ao=None) == TMED_EINVAL
        assert gen(call, ln=None) == TMED_EINVAL
        assert gen(call, d=None) == TMED_EINVAL  # leaves with bytes but no array
        bad = tree_off.copy()
        bad[0] = 1
        assert gen(call, to=bad) == TMED_EINVAL
        bad = tree_off.copy()
        bad[3] = bad[2] - 1
        assert gen(call, to=bad) == TMED_EINVAL
        bad = leaf_off.copy()
        bad[5] = bad[4] - 1 if bad[4] else 2 ** 40
        assert gen(call, lo=bad) == TMED_EINVAL
        # no trees: nothing but the empty offsets
        assert call(_p(FAKE), None, None, None, 0, None, None, _p(aunt_off), None, 0, ctypes.byref(need)) == TMED_OK
    # a full call needs roots and leaf hashes
    aunts = np.zeros((128, 32), np.uint8)
    assert abi.tmed_merkle_proofs(_p(FAKE), _p(data), _p(leaf_off), _p(tree_off), T, None, None, _p(aunt_off),
                                  _p(aunts), aunts.size, ctypes.byref(need)) == TMED_EINVAL
    off = np.array([0, 10, 5], np.uint64)
    blob = np.zeros(32, np.uint8)

    def ps(ctx=_p(FAKE), d=_p(blob), o=off[:2], part=64, po=_p(part_off), ao=_p(aunt_off), ln=ctypes.byref(need), n=1):
        return abi.tmed_partset_proofs(ctx, d, None if o is None else _p(np.ascontiguousarray(o)), n, part, None, po,
                                       None, ao, None, 0, ln)

    assert ps() == TMED_OK
    assert ps(ctx=None) == TMED_EINVAL and ps(part=0) == TMED_EINVAL and ps(o=None) == TMED_EINVAL
    assert ps(po=None) == TMED_EINVAL and ps(ao=None) == TMED_EINVAL and ps(ln=None) == TMED_EINVAL
    assert ps(d=None) == TMED_EINVAL
    assert ps(o=off, n=2) == TMED_EINVAL  # offsets decrease
    assert ps(o=None, n=0) == TMED_OK


def test_verify_einval(abi):
    from tmed._native import TMED_EINVAL, TMED_OK
    n = 3
    roots = np.zeros((2, 32), np.uint8)
    leaves = np.zeros(16, np.uint8)
    arrs = dict(leaf_off=np.array([0, 1, 2, 3], np.uint64), lh=np.zeros((n, 32), np.uint8),
                totals=np.ones(n, np.int64), indexes=np.zeros(n, np.int64),
                aunt_off=np.array([0, 1, 1, 2], np.uint64), aunts=np.zeros((2, 32), np.uint8),
                root_of=np.array([0, 1, 1], np.uint32), codes=np.zeros(n, np.uint8))

    def call(ctx=_p(FAKE), n_=n, r=_p(roots), n_roots=2, lv=_p(leaves), **kw):
        a = {k: (None if k in kw and kw[k] is None else _p(kw.get(k, v))) for k, v in arrs.items()}
        return abi.tmed_merkle_proofs_verify(ctx, n_, r, n_roots, a["root_of"], lv, a["leaf_off"], a["lh"], a["totals"],
                                             a["indexes"], a["aunt_off"], a["aunts"], a["codes"])

    assert call(ctx=None) == TMED_EINVAL
    assert call(n_=0) == TMED_OK
    for k in ("leaf_off", "lh", "totals", "indexes", "aunt_off", "aunts", "codes"):
        assert call(**{k: None}) == TMED_EINVAL, k
    assert call(r=None) == TMED_EINVAL and call(lv=None) == TMED_EINVAL
    assert call(root_of=np.array([0, 2, 1], np.uint32)) == TMED_EINVAL  # a root index out of range
    assert call(root_of=None) == TMED_EINVAL                           # NULL means i, and there are 2 roots
    assert call(leaf_off=np.array([0, 2, 1, 3], np.uint64)) == TMED_EINVAL
    assert call(aunt_off=np.array([0, 2, 1, 2], np.uint64)) == TMED_EINVAL
    assert call(leaf_off=np.array([0, 1, 2, 2 ** 33], np.uint64)) == TMED_EINVAL  # a leaf past 2^32 - 65 bytes


def test_wrappers_refuse_wrong_shapes():
    from tmed.merkle import verify_proofs, verify_proofs_packed
    z = np.zeros
    with pytest.raises(ValueError):
        verify_proofs(None, [(bytes(32), b"x", (1, 0, bytes(31), []))])
    with pytest.raises(ValueError):
        verify_proofs_packed(None, z((1, 32), np.uint8), z(8, np.uint8), z(2, np.uint64), z((1, 32), np.uint8),
                             z(1, np.int64), z(1, np.int64), np.array([0, 3], np.uint64), z((2, 32), np.uint8))


# ---- the Go binding with its proof tests ------------------------------------------------------------

def test_go_binding_with_proof_tests_clean():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import go_cgo_check as gc
    try:
        header = gc.Header()
    except RuntimeError as e:  # no clang: nothing to check against
        pytest.skip(str(e))
    go_dir = os.path.dirname(gc.GO_FILE)
    extra = []
    for name in ("tmedgpu_test.go", "proofs_test.go"):
        with open(os.path.join(go_dir, name)) as f:
            extra.append((name, f.read()))
    with open(gc.GO_FILE) as f:
        go = f.read()
    with open(gc.INTEGRATION) as f:
        md = f.read()
    errs, pkg = gc.check_binding(go, header, extra=extra)
    assert errs + gc.check_snippets(md, header, pkg) == []
    for fn in ("MerkleProofs", "PartSetProofs", "TxsProofs", "VerifyProofs"):
        assert "func (e *Engine) %s(" % fn in go
    assert "tmed_merkle_proofs_verify" in header.funcs and "TMED_PROOF_ROOT_HASH" in header.macros
