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


_SWEEP = []


def _full_sweep():
    """The 57,330 cases of B.full_sweep(), generated once."""
    if not _SWEEP:
        _SWEEP.extend(B.full_sweep())
    return _SWEEP


def test_commit_hashes_full_sweep_gpu(engine):
    """The whole CommitSig sweep through the device encoder (commitsig_leaf.h's device branches), in
    one call: 234 PackedCommits of 245 signatures.  A mismatch names the commit index i; its cases
    are full_sweep()[245 i : 245 i + 245], replayable through the host encoder."""
    from tmed.merkle import commit_hashes
    sweep = _full_sweep()
    assert len(sweep) == 57330
    lists = [sweep[at:at + 245] for at in range(0, len(sweep), 245)]
    assert len(lists) == 234 and all(len(l) == 245 for l in lists)
    got = commit_hashes(engine, [B.packed_commit(l) for l in lists])
    wrong = [i for i, (g, l) in enumerate(zip(got, lists)) if g != B.commit_hash(l)]
    assert not wrong, "commits (245 cases each, from case 245 * index) with another root: %s" % wrong


def test_commit_hashes_threaded_pack_gpu(engine):
    """One call of more than 65,536 signatures, where merkle.hip's pack_threads leaves 1 and the
    scan and the packing run on the host threads: the sweep and a second pass over its first part,
    cut into 400 commits of 0..400 signatures, as Commit objects, PackedCommits and PackedCommits
    with address_lens=None; every 17th commit holds one signature the flat arrays cannot
    reproduce (65-byte signature, 19-byte address, nanos 10^9 in rotation) and is None, the
    others are exact, the empty ones the empty hash."""
    from tmed.merkle import commit_hashes
    sweep = _full_sweep()
    rng = random.Random(17)
    sizes = [rng.randint(0, 400) for _ in range(400)]
    for i in (0, 34, 104, 399):
        sizes[i] = 0
    total = sum(sizes)
    assert len(sweep) <= total <= 2 * len(sweep)
    stream = sweep + sweep[:total - len(sweep)]
    addr = bytes(range(20))
    bad = [(2, addr, 1700000000, 5, bytes(65)), (2, addr[:19], 1700000000, 5, bytes(64)),
           (2, addr, 1700000000, 10 ** 9, bytes(64))]
    commits, exp, at, good_sigs, nbad = [], [], 0, 0, 0
    for i, n in enumerate(sizes):
        sigs = stream[at:at + n]
        at += n
        kind = i % 3
        if kind == 2:  # address_lens=None: every address 20 bytes
            sigs = [(f, a if len(a) == 20 else B._pattern(20, at + j), s, ns, sig)
                    for j, (f, a, s, ns, sig) in enumerate(sigs)]
        if i % 17 == 16:
            b = bad[nbad % 3]
            nbad += 1
            sigs = sigs[:n // 2] + [b] + sigs[n // 2:]
            if kind == 2 and len(b[1]) != 20:
                kind = 1
            exp.append(None)
        else:
            good_sigs += len(sigs)
            exp.append(B.commit_hash(sigs))
        commits.append(_product_commit(sigs) if kind == 0 else
                       B.packed_commit(sigs, address_lens="explicit" if kind == 1 else None))
    assert at == total and nbad >= 3
    assert good_sigs >= 65536  # below it the single-threaded path would pass this test silently
    got = commit_hashes(engine, commits)
    wrong = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not wrong, wrong
    assert all(got[i].hex() == B.EMPTY_HASH for i in (0, 34, 104, 399))
