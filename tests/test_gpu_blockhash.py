"""GPU parity of Commit.Hash (tmed_commit_hashes) and Data.Hash (tmed_txs_hashes) against the
restatement in blockhash_cases.py (bit-exact roots)."""
import random

import numpy as np
import pytest

import blockhash_cases as B
import tmed.types as T
from commit_cases import oracle_result, pbid, same, to_product
from oracle import commit as C
from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of
from tmed._native import TMED_EINVAL, TmedError

pytestmark = pytest.mark.gpu

N_SIGS = (0, 1, 2, 3, 5, 64, 65, 175, 257)


def _sig_lists():
    """Commits of N_SIGS signatures cut from the sweep walk (572 of its 585 signatures)."""
    sweep = B.cycle_sigs()
    out, at = [], 0
    for n in N_SIGS:
        out.append(sweep[at:at + n])
        at += n
    assert at <= len(sweep)
    return out


def _product_commit(sigs):
    return T.Commit(1, 0, T.BlockID(), [T.CommitSig(f, a, (s, ns), sig) for f, a, s, ns, sig in sigs])


def test_commit_hashes_gpu(engine):
    """One call: commits of 0..257 signatures as Commit objects and as PackedCommits (absent
    entries keep their address rows with length 0), one PackedCommit with address_lens=None."""
    from tmed.merkle import commit_hashes
    lists = _sig_lists()
    all20 = [(f, a if len(a) == 20 else B._pattern(20, i), s, ns, sig)
             for i, (f, a, s, ns, sig) in enumerate(B.cycle_sigs()[100:300])]
    commits = [_product_commit(l) for l in lists] + [B.packed_commit(l) for l in lists]
    commits.append(B.packed_commit(all20, address_lens=None))
    exp = [B.commit_hash(l) for l in lists] * 2 + [B.commit_hash(all20)]
    got = commit_hashes(engine, commits)
    assert None not in got  # every ok is 1
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, k
    assert got[0].hex() == B.EMPTY_HASH


def test_commit_hashes_not_reproducible_gpu(engine):
    """ok = 0 (None) for a 65-byte signature, a 19-byte address, seconds 253402300800, nanos -1 and
    10^9, interleaved with good commits that stay exact; addresses = NULL with a length of 20 is
    TMED_EINVAL."""
    from tmed.merkle import CommitHashBatch, commit_hashes
    good = B.cycle_sigs()[:40]
    addr = bytes(range(20))
    bad = [(2, addr, 1700000000, 5, bytes(65)),
           (2, addr[:19], 1700000000, 5, bytes(64)),
           (2, addr, B.MAX_SECONDS, 5, bytes(64)),
           (2, addr, 1700000000, -1, bytes(64)),
           (2, addr, 1700000000, 10 ** 9, bytes(64))]
    commits, exp = [], []
    for k, b in enumerate(bad):
        g = good[3 * k:3 * k + 7 + k]
        commits += [B.packed_commit(g), B.packed_commit(g[:k + 1] + [b] + g[k + 1:])]
        exp += [B.commit_hash(g), None]
    commits.append(_product_commit(good))
    exp.append(B.commit_hash(good))
    commits.insert(1, _product_commit([bad[0]] + good[:2]))
    exp.insert(1, None)
    assert commit_hashes(engine, commits) == exp
    batch = CommitHashBatch([B.packed_commit(good)])
    out, ok = batch.run(engine)
    assert ok[0] == 1 and bytes(out[0]) == B.commit_hash(good)
    batch.cs[0].addresses = None
    with pytest.raises(TmedError) as ei:
        batch.run(engine)
    assert ei.value.code == TMED_EINVAL


def test_txs_hashes_gpu(engine):
    """Blocks of 0..129 transactions of lengths 0..200 and one of 70,000 bytes; the running
    concatenation puts transactions at every dword misalignment."""
    from tmed.merkle import txs_hashes
    rng = random.Random(11)
    blocks, lens = [], iter(list(range(201)) + [rng.randrange(0, 201) for _ in range(100)])
    for n in (0, 1, 2, 3, 7, 64, 129):
        blocks.append([rng.randbytes(next(lens)) for _ in range(n)])
    blocks[4][3] = rng.randbytes(70000)
    blocks.append([])
    starts, at = set(), 0
    for b in blocks:
        for t in b:
            starts.add(at % 4)
            at += len(t)
    assert starts == {0, 1, 2, 3}
    got = txs_hashes(engine, blocks)
    for b, g in zip(blocks, got):
        assert g == B.txs_hash(b), len(b)
    assert got[0].hex() == got[-1].hex() == B.EMPTY_HASH


def test_commit_hashes_after_submitted_window_gpu(engine):
    """A blocksync window of 3 blocks x 8 validators is submitted, then commit_hashes runs (it
    collects the window first), then blocksync_wait: hashes and outcomes equal the oracle's."""
    from tmed.merkle import commit_hashes
    chain = "hash-chain"
    vs, seeds = make_valset([seed_of("bh", i) for i in range(8)], [10] * 8)
    bids, heights, ocommits, pcommits = [], [], [], []
    for b in range(3):
        bid = make_block_id("bh%d" % b)
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
    w = T.BlocksyncWindow(pv, chain, [pbid(b) for b in bids], heights, pcommits)
    w.submit(engine, 1)
    got = commit_hashes(engine, pcommits)
    T.blocksync_wait(engine)
    for b in range(3):
        sigs = [(s.flag, s.address, s.timestamp[0], s.timestamp[1], s.signature) for s in ocommits[b].signatures]
        assert got[b] == B.commit_hash(sigs), b
        exp = oracle_result(1, vs, chain, bids[b], heights[b], ocommits[b], 0, 0)
        assert same(w.errors()[b], exp), b
    assert list(w.codes()) == [0, 4, 0]


def test_commit_hash_equals_old_route_gpu(engine):
    """commit_hashes == merkle_roots over the host-marshalled leaves (the only route before)."""
    from tmed.merkle import commit_hashes, merkle_roots
    sigs = B.cycle_sigs()[200:375]
    assert len(sigs) == 175
    assert commit_hashes(engine, [B.packed_commit(sigs)]) == merkle_roots(engine, [B.commit_leaves(sigs)])
