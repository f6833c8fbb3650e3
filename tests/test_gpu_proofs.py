"""GPU parity of the Merkle proof calls (tmed_merkle_proofs, tmed_partset_proofs, tmed_txs_proofs,
tmed_merkle_proofs_verify) against the recursive restatement in proof_cases.py: exact bytes of
roots, leaf hashes, aunt offsets and aunts; exact codes of Proof.Verify."""
import hashlib
import random

import numpy as np
import pytest

import proof_cases as P
from oracle import merkle as M

pytestmark = pytest.mark.gpu

TREE_SIZES = list(range(0, 70)) + [127, 128, 129, 255, 256, 257, 300]
_CACHE = {}


def _pack(groups):
    flat = [bytes(x) for g in groups for x in g]
    item_off = np.zeros(len(flat) + 1, np.uint64)
    item_off[1:] = np.cumsum([len(x) for x in flat])
    group_off = np.zeros(len(groups) + 1, np.uint32)
    group_off[1:] = np.cumsum([len(g) for g in groups])
    return np.frombuffer(b"".join(flat) + bytes(8), np.uint8), item_off, group_off


def _expected(groups, proofs_of=P.proofs_from_byte_slices):
    """The restatement's (roots, leaf_hashes, aunt_off, aunts) for a call's trees, as arrays."""
    roots, lhs, aunts, ao = [], [], [], [0]
    for g in groups:
        root, proofs = proofs_of(g)
        roots.append(root)
        base = len(lhs)
        for total, index, lh, au in proofs:
            assert total == len(g) and index == len(lhs) - base
            lhs.append(lh)
            aunts.extend(au)
            ao.append(len(aunts))
    u8 = lambda hs: np.frombuffer(b"".join(hs), np.uint8).reshape(-1, 32)  # noqa: E731
    return u8(roots), u8(lhs), np.asarray(ao, np.uint64), u8(aunts)


def _same(got, exp):
    roots, lh, ao, au = got
    assert ao.tolist() == exp[2].tolist()
    assert roots.shape == exp[0].shape and (roots == exp[0]).all()
    assert lh.shape == exp[1].shape and (lh == exp[1]).all()
    assert au.shape == exp[3].shape and (au == exp[3]).all()


def _forest():
    """Trees of TREE_SIZES leaves of lengths 0..200, an empty tree after every fifth tree (so empty
    trees stand between non-empty ones, and one opens the call), with the restatement's proofs."""
    if "forest" not in _CACHE:
        rng = random.Random(21)
        lens = iter(list(range(201)) * 20)
        trees = []
        for k, n in enumerate(TREE_SIZES):
            trees.append([rng.randbytes(next(lens)) for _ in range(n)])
            if k % 5 == 4:
                trees.append([])
        _CACHE["forest"] = (trees, _pack(trees), _expected(trees))
    return _CACHE["forest"]


def _verify_inputs(packed, exp, group_off):
    """The arrays of verify_proofs_packed for every proof of a generator's call (root_of = the tree)."""
    data, item_off, _ = packed
    roots, lh, ao, au = exp
    counts = np.diff(group_off.astype(np.int64))
    root_of = np.repeat(np.arange(len(counts), dtype=np.uint32), counts)
    totals = np.repeat(counts, counts).astype(np.int64)
    indexes = (np.arange(len(root_of)) - np.repeat(group_off[:-1].astype(np.int64), counts)).astype(np.int64)
    return dict(roots=roots, data=data, leaf_off=item_off, leaf_hashes=lh, totals=totals, indexes=indexes,
                aunt_off=ao, aunts=au, root_of=root_of)


# ---- generators -----------------------------------------------------------------------------------

def test_merkle_proofs_forest_gpu(engine):
    from tmed.merkle import merkle_proofs, merkle_proofs_packed, merkle_roots_packed, verify_proofs_packed
    trees, packed, exp = _forest()
    assert [] in trees[1:-1] and len(trees[-1]) == 300
    got = merkle_proofs_packed(engine, *packed)
    _same(got, exp)
    assert (got[0] == merkle_roots_packed(engine, *packed)).all()
    assert bytes(got[0][0]).hex() == P.EMPTY_HASH  # the call opens with the empty tree
    # the list form, on the trees of 0..9 leaves
    small = merkle_proofs(engine, trees[:11])
    for t, (root, proofs) in zip(trees[:11], small):
        eroot, eproofs = P.proofs_from_byte_slices(t)
        assert root == eroot and proofs == eproofs
    # every generated proof verifies, many proofs sharing each root
    codes = verify_proofs_packed(engine, **_verify_inputs(packed, got, packed[2]))
    assert len(codes) == sum(TREE_SIZES) and not codes.any()


def test_merkle_proofs_deep_tree_gpu(engine):
    """One tree of 65,537 four-byte leaves: depth 17, one leaf past a power of two (its last leaf has
    a single aunt, the left subtree's root)."""
    from tmed.merkle import merkle_proofs_packed, merkle_roots_packed, verify_proofs_packed
    n = 65537
    tree = [i.to_bytes(4, "little") for i in range(n)]
    packed = _pack([tree])
    exp = _expected([tree])
    assert int(exp[2][-1] - exp[2][-2]) == 1 and int(exp[2][1]) == 17
    got = merkle_proofs_packed(engine, *packed)
    _same(got, exp)
    assert (got[0] == merkle_roots_packed(engine, *packed)).all()
    assert not verify_proofs_packed(engine, **_verify_inputs(packed, got, packed[2])).any()


@pytest.mark.parametrize("part_size", [64, 100, 65536])
def test_partset_proofs_gpu(engine, part_size):
    from tmed.merkle import partset_proofs, partset_proofs_packed, partset_roots_packed, verify_proofs_packed
    rng = random.Random(part_size)
    blocks = [b"", b"\x01", rng.randbytes(part_size - 1), rng.randbytes(part_size), rng.randbytes(part_size + 1),
              rng.randbytes(7 * part_size // 2), rng.randbytes(3 * 65536 + 17)]
    parts = [[b[i:i + part_size] for i in range(0, len(b), part_size)] for b in blocks]
    exp = _expected(parts)
    off = np.zeros(len(blocks) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blocks])
    data = np.frombuffer(b"".join(blocks) + bytes(8), np.uint8)
    roots, part_off, lh, ao, au = partset_proofs_packed(engine, data, off, part_size)
    _same((roots, lh, ao, au), exp)
    pdata, poff, pgroups = _pack(parts)
    assert part_off.tolist() == pgroups.tolist()
    assert (roots == partset_roots_packed(engine, data, off, part_size)).all()
    for b, r in zip(blocks, roots):
        assert bytes(r) == P.partset_proofs(b, part_size)[0] == M.partset_root(b, part_size)
    # PartSet.AddPart's check (types/part_set.go:284): each part against its block's root
    assert not verify_proofs_packed(engine, **_verify_inputs((pdata, poff, pgroups), (roots, lh, ao, au),
                                                             part_off)).any()
    got = partset_proofs(engine, blocks[:5], part_size)
    assert got == [P.partset_proofs(b, part_size) for b in blocks[:5]]


def test_txs_proofs_gpu(engine):
    """Blocks of 0, 1, 2, 3 and 33 transactions of lengths 0..300; TxProof.Validate's check
    (types/tx.go:109-124) verifies tx.Hash() as the leaf."""
    from tmed.merkle import txs_hashes_packed, txs_proofs, txs_proofs_packed, verify_proofs_packed
    rng = random.Random(33)
    lens = iter([0, 300, 1, 299, 55, 56, 63, 64, 65, 119, 120] + [rng.randrange(0, 301) for _ in range(40)])
    blocks = [[rng.randbytes(next(lens)) for _ in range(n)] for n in (0, 1, 2, 3, 33)]
    packed = _pack(blocks)
    exp = _expected(blocks, P.txs_proofs)
    got = txs_proofs_packed(engine, *packed)
    _same(got, exp)
    assert (got[0] == txs_hashes_packed(engine, *packed)).all()
    assert txs_proofs(engine, blocks) == [P.txs_proofs(b) for b in blocks]
    digests = [[hashlib.sha256(t).digest() for t in b] for b in blocks]
    assert not verify_proofs_packed(engine, **_verify_inputs(_pack(digests), got, packed[2])).any()


# ---- verifier -------------------------------------------------------------------------------------

def _flip(b: bytes, bit: int) -> bytes:
    a = bytearray(b)
    a[bit >> 3] ^= 1 << (bit & 7)
    return bytes(a)


def test_verify_mutations_gpu(engine):
    """Every mutation of the issue on proofs of trees of 1, 2, 5, 129 and 300 leaves (first, middle
    and last leaf): the code is the restatement's."""
    from tmed.merkle import verify_proofs
    trees, _, _ = _forest()
    rng = random.Random(7)
    items, why = [], []
    for tree in (t for t in trees if len(t) in (1, 2, 5, 129, 300)):
        root, proofs = P.proofs_from_byte_slices(tree)
        n = len(tree)
        for i in sorted({0, n // 2, n - 1}):
            total, index, lh, au = proofs[i]
            leaf = tree[i]
            muts = [("intact", root, leaf, (total, index, lh, au)),
                    ("extra aunt", root, leaf, (total, index, lh, au + [rng.randbytes(32)])),
                    ("index = total", root, leaf, (total, total, lh, au)),
                    ("index = -1", root, leaf, (total, -1, lh, au)),
                    ("total = 0", root, leaf, (0, index, lh, au)),
                    ("total = -1", root, leaf, (-1, index, lh, au)),
                    ("total + 1", root, leaf, (total + 1, index, lh, au)),
                    ("wrong leaf hash", root, leaf, (total, index, _flip(lh, 255), au)),
                    ("wrong leaf", root, leaf + b"\0", (total, index, lh, au)),
                    ("wrong root", _flip(root, 0), leaf, (total, index, lh, au)),
                    ("negative total before negative index", root, leaf, (-5, -1, lh, au)),
                    ("negative index before the leaf hash", root, leaf + b"x", (total, -1, lh, au))]
            if au:
                muts += [("flipped aunt bit", root, leaf, (total, index, lh, [_flip(au[0], 9)] + au[1:])),
                         ("flipped last aunt", root, leaf, (total, index, lh, au[:-1] + [_flip(au[-1], 200)])),
                         ("missing aunt", root, leaf, (total, index, lh, au[:-1])),
                         ("missing first aunt", root, leaf, (total, index, lh, au[1:]))]
            if n > 1:
                muts.append(("another valid index", root, leaf, (total, (index + 1) % n, lh, au)))
            for m in muts:
                items.append(m[1:])
                why.append((n, i, m[0]))
    exp = [P.verify(root, leaf, *proof) for root, leaf, proof in items]
    got = verify_proofs(engine, items)
    wrong = [(w, g, e) for w, g, e in zip(why, got, exp) if g != e]
    assert not wrong, wrong[:10]
    assert set(exp) == {0, 1, 2, 3, 4}
    for (n, i, name), e in zip(why, exp):
        if name == "intact":
            assert e == P.PROOF_OK
        elif name in ("flipped aunt bit", "extra aunt", "missing aunt", "index = total", "total = 0", "wrong root"):
            assert e == P.PROOF_ROOT_HASH, (n, i, name)


def test_verify_large_totals_gpu(engine):
    """Synthetic proofs at totals past 2^32 with random aunts, 0..65 of them, and the root the
    restatement computes: code 0 exactly where it returns a hash (the aunt count is the path
    length), 4 elsewhere.  Aunt counts of 100 and 101 (ValidateBasic's limit and one more) give 4."""
    from tmed.merkle import verify_proofs
    rng = random.Random(63)
    pool = [rng.randbytes(32) for _ in range(101)]
    items, exp, depths = [], [], set()
    for total in (2 ** 32 + 1, 2 ** 62 + 3, 2 ** 63 - 1):
        for index in P.large_indexes(total):
            leaf = rng.randbytes(rng.randrange(0, 70))
            lh = M.leaf_hash(leaf)
            for na in list(range(66)) + [100, 101]:
                aunts = pool[na % 7:na % 7 + na] if na <= 65 else pool[:na]
                root = P.compute_hash_from_aunts(index, total, lh, aunts)
                if root is not None:
                    depths.add(na)
                exp.append(P.PROOF_OK if root is not None else P.PROOF_ROOT_HASH)
                items.append((root or pool[3], leaf, (total, index, lh, aunts)))
    assert exp.count(P.PROOF_OK) == 9 and {33, 63, 62} <= depths
    got = verify_proofs(engine, items)
    assert got == exp, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e][:10]


# ---- sequencing -----------------------------------------------------------------------------------

def test_proofs_after_submitted_window_gpu(engine):
    """A blocksync window is submitted, then a proofs call and a verify call run (they collect the
    window first), then blocksync_wait: the proofs are the same bytes and the window's results
    are the oracle's."""
    import tmed.types as T
    from commit_cases import oracle_result, pbid, same, to_product
    from oracle import commit as C
    from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of
    from tmed.merkle import merkle_proofs_packed, verify_proofs_packed
    chain = "proof-chain"
    vs, seeds = make_valset([seed_of("pf", i) for i in range(8)], [10] * 8)
    bids, heights, ocommits, pcommits = [], [], [], []
    for b in range(3):
        bid = make_block_id("pf%d" % b)
        flags = [C.FLAG_COMMIT] * 8
        flags[b] = C.FLAG_ABSENT
        cm = make_commit(vs, seeds, chain, 10 + b, 0, bid, flags=flags)
        if b == 1:
            s = bytearray(cm.signatures[0].signature)
            s[7] ^= 4
            cm.signatures[0].signature = bytes(s)
        pv, pc = to_product(vs, cm)
        bids.append(bid)
        heights.append(10 + b)
        ocommits.append(cm)
        pcommits.append(pc)
    trees, packed, exp = _forest()
    w = T.BlocksyncWindow(pv, chain, [pbid(b) for b in bids], heights, pcommits)
    w.submit(engine, 1)
    got = merkle_proofs_packed(engine, *packed)
    codes = verify_proofs_packed(engine, **_verify_inputs(packed, got, packed[2]))
    T.blocksync_wait(engine)
    _same(got, exp)
    assert not codes.any()
    for b in range(3):
        assert same(w.errors()[b], oracle_result(1, vs, chain, bids[b], heights[b], ocommits[b], 0, 0)), b
    assert list(w.codes()) == [0, 4, 0]
