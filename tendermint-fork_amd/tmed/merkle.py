"""Batched Merkle hashing on the GPU — host mirror of the reference's
``crypto/merkle.HashFromByteSlices`` (crypto/merkle/tree.go:9-22), ``ValidatorSet.Hash``
(types/validator_set.go:347-353), ``Header.Hash`` (types/block.go:440-475) and the
``PartSet`` root (types/part_set.go:166-194), each over many objects per call through the
C ABI (csrc/merkle.hip).  Same inputs and outputs as the Go functions, one list entry per
object; ``Header.Hash``'s nil is ``None``.  ``Commit.Hash`` (types/block.go:894-912) and
``Data.Hash`` (types/block.go:1004-1012 -> ``Txs.Hash``, types/tx.go:47-55), the two hashes
``Block.ValidateBasic`` recomputes per block, are ``commit_hashes`` and ``txs_hashes``.
``merkle_proofs`` / ``partset_proofs`` / ``txs_proofs`` are ``merkle.ProofsFromByteSlices``
(crypto/merkle/proof.go:35-48: the root and every leaf's ``Proof``, i.e. the whole of
``NewPartSetFromData`` and the tree of ``Txs.Proof``) and ``verify_proofs`` is ``Proof.Verify``
(proof.go:52-68) for many proofs, as codes."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from ._native import TMED_OK, TmedError, lib

BLOCK_PART_SIZE_BYTES = 65536  # types/params.go:19 BlockPartSizeBytes


class _HeaderBlockID(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_void_p), ("hash_len", ctypes.c_uint32), ("psh_total", ctypes.c_uint32),
                ("psh_hash", ctypes.c_void_p), ("psh_hash_len", ctypes.c_uint32)]


class _HeaderC(ctypes.Structure):
    _fields_ = [("version_block", ctypes.c_uint64), ("version_app", ctypes.c_uint64),
                ("chain_id", ctypes.c_char_p), ("chain_id_len", ctypes.c_uint32), ("height", ctypes.c_int64),
                ("time_seconds", ctypes.c_int64), ("time_nanos", ctypes.c_int32), ("last_block_id", _HeaderBlockID),
                ("hashes", ctypes.c_void_p * 9), ("hash_lens", ctypes.c_uint32 * 9)]


HEADER_HASH_FIELDS = ("last_commit_hash", "data_hash", "validators_hash", "next_validators_hash",
                      "consensus_hash", "app_hash", "last_results_hash", "evidence_hash", "proposer_address")


def _bind():
    l = lib()
    if l.tmed_merkle_roots.argtypes is None:
        P, SZ = ctypes.c_void_p, ctypes.c_size_t
        l.tmed_merkle_roots.restype = ctypes.c_int
        l.tmed_merkle_roots.argtypes = [P, P, P, P, SZ, P]
        l.tmed_valset_hashes.restype = ctypes.c_int
        l.tmed_valset_hashes.argtypes = [P, P, P, P, SZ, P]
        l.tmed_header_hashes.restype = ctypes.c_int
        l.tmed_header_hashes.argtypes = [P, ctypes.POINTER(_HeaderC), SZ, P, P]
        l.tmed_partset_roots.restype = ctypes.c_int
        l.tmed_partset_roots.argtypes = [P, P, P, SZ, ctypes.c_uint32, P]
        l.tmed_commit_hashes.restype = ctypes.c_int
        l.tmed_commit_hashes.argtypes = [P, P, SZ, P, P]
        l.tmed_txs_hashes.restype = ctypes.c_int
        l.tmed_txs_hashes.argtypes = [P, P, P, P, SZ, P]
        PSZ = ctypes.POINTER(SZ)
        l.tmed_merkle_proofs.restype = ctypes.c_int
        l.tmed_merkle_proofs.argtypes = [P, P, P, P, SZ, P, P, P, P, SZ, PSZ]
        l.tmed_partset_proofs.restype = ctypes.c_int
        l.tmed_partset_proofs.argtypes = [P, P, P, SZ, ctypes.c_uint32, P, P, P, P, P, SZ, PSZ]
        l.tmed_txs_proofs.restype = ctypes.c_int
        l.tmed_txs_proofs.argtypes = [P, P, P, P, SZ, P, P, P, P, SZ, PSZ]
        l.tmed_merkle_proofs_verify.restype = ctypes.c_int
        l.tmed_merkle_proofs_verify.argtypes = [P, SZ, P, SZ, P, P, P, P, P, P, P, P, P]
    return l


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def merkle_roots(engine, trees: Sequence[Sequence[bytes]]) -> list:
    """HashFromByteSlices(tree) for every tree (list of byte-slice lists)."""
    flat, leaf_lens, counts = [], [], []
    for t in trees:
        counts.append(len(t))
        for leaf in t:
            flat.append(bytes(leaf))
            leaf_lens.append(len(leaf))
    leaf_off = np.zeros(len(leaf_lens) + 1, np.uint64)
    np.cumsum(np.asarray(leaf_lens, np.uint64), out=leaf_off[1:])
    tree_off = np.zeros(len(counts) + 1, np.uint32)
    np.cumsum(np.asarray(counts, np.uint32), out=tree_off[1:])
    data = np.frombuffer(b"".join(flat) + b"\0" * 8, np.uint8)
    roots = np.zeros((max(len(trees), 1), 32), np.uint8)
    if not trees:
        return []
    rc = _bind().tmed_merkle_roots(engine._h, _p(data), _p(leaf_off), _p(tree_off), len(trees), _p(roots))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_merkle_roots")
    return [bytes(r) for r in roots[:len(trees)]]


def merkle_roots_packed(engine, data: np.ndarray, leaf_off: np.ndarray, tree_off: np.ndarray) -> np.ndarray:
    """HashFromByteSlices of trees [tree_off[t], tree_off[t+1]) over leaves data[leaf_off[i] ..
    leaf_off[i+1]) (u8 array with 8 spare bytes at its end, u64 offsets, u32 tree offsets)."""
    n = tree_off.shape[0] - 1
    roots = np.zeros((max(n, 1), 32), np.uint8)
    if n <= 0:
        return roots[:0]
    rc = _bind().tmed_merkle_roots(engine._h, _p(data), _p(np.ascontiguousarray(leaf_off, np.uint64)),
                                   _p(np.ascontiguousarray(tree_off, np.uint32)), n, _p(roots))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_merkle_roots")
    return roots[:n]


def valset_hashes_arrays(engine, pubkeys: np.ndarray, powers: np.ndarray, set_off: np.ndarray) -> np.ndarray:
    """ValidatorSet.Hash of sets [set_off[s], set_off[s+1]) over (pubkeys u8[N,32], powers i64[N])."""
    n_sets = set_off.shape[0] - 1
    out = np.zeros((max(n_sets, 1), 32), np.uint8)
    if n_sets <= 0:
        return out[:0]
    pk = np.ascontiguousarray(pubkeys, np.uint8).reshape(-1, 32)
    pw = np.ascontiguousarray(powers, np.int64)
    so = np.ascontiguousarray(set_off, np.uint32)
    rc = _bind().tmed_valset_hashes(engine._h, _p(pk) if pk.size else None, _p(pw) if pw.size else None, _p(so),
                                    n_sets, _p(out))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_valset_hashes")
    return out[:n_sets]


def valset_hashes(engine, valsets: Sequence) -> list:
    """ValidatorSet.Hash() of every tmed.types.ValidatorSet (ed25519 validators)."""
    pubs, pows, off = [], [], [0]
    for vs in valsets:
        for v in vs.validators:
            pubs.append(np.frombuffer(v.pub_key, np.uint8))
            pows.append(v.voting_power)
        off.append(len(pubs))
    pk = np.array(pubs, np.uint8).reshape(-1, 32) if pubs else np.zeros((0, 32), np.uint8)
    return [bytes(r) for r in valset_hashes_arrays(engine, pk, np.array(pows, np.int64), np.array(off, np.uint32))]


class HeaderBatch:
    """Headers packed into C structs once (repeated timing of the C call alone)."""

    def __init__(self, headers: Sequence[dict]):
        n = self.n = len(headers)
        self.hs = (_HeaderC * max(n, 1))()
        self.keep = []
        for i, h in enumerate(headers):
            cid = h["chain_id"].encode()
            bh, pt, ph = h["last_block_id"]
            bh, ph = bytes(bh), bytes(ph)
            self.keep.extend([cid, bh, ph])
            c = self.hs[i]
            c.version_block, c.version_app = h["version_block"], h["version_app"]
            c.chain_id, c.chain_id_len = cid, len(cid)
            c.height = h["height"]
            c.time_seconds, c.time_nanos = h["time"]
            c.last_block_id = _HeaderBlockID(ctypes.cast(ctypes.c_char_p(bh), ctypes.c_void_p), len(bh), pt,
                                             ctypes.cast(ctypes.c_char_p(ph), ctypes.c_void_p), len(ph))
            for k, name in enumerate(HEADER_HASH_FIELDS):
                v = bytes(h[name])
                self.keep.append(v)
                c.hashes[k] = ctypes.cast(ctypes.c_char_p(v), ctypes.c_void_p)
                c.hash_lens[k] = len(v)
        self.out = np.zeros((max(n, 1), 32), np.uint8)
        self.ok = np.zeros(max(n, 1), np.uint8)

    def run(self, engine) -> list:
        if self.n == 0:
            return []
        rc = _bind().tmed_header_hashes(engine._h, self.hs, self.n, _p(self.out), _p(self.ok))
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_header_hashes")
        return [bytes(self.out[i]) if self.ok[i] else None for i in range(self.n)]


def header_hashes(engine, headers: Sequence[dict]) -> list:
    """Header.Hash of every header (dict with the fields of oracle/merkle.py's header_leaves);
    None where the reference returns nil (empty ValidatorsHash)."""
    return HeaderBatch(headers).run(engine)


def partset_roots_packed(engine, data: np.ndarray, off: np.ndarray, part_size: int = BLOCK_PART_SIZE_BYTES):
    """Roots of blocks data[off[b] .. off[b+1]) (u8 array, u64 offsets): an n x 32 array."""
    n = off.shape[0] - 1
    roots = np.zeros((max(n, 1), 32), np.uint8)
    if n <= 0:
        return roots[:0]
    rc = _bind().tmed_partset_roots(engine._h, _p(data), _p(np.ascontiguousarray(off, np.uint64)), n, part_size,
                                    _p(roots))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_partset_roots")
    return roots[:n]


def partset_roots(engine, blocks: Sequence[bytes], part_size: int = BLOCK_PART_SIZE_BYTES) -> list:
    """NewPartSetFromData(block, part_size).Hash() for every block's bytes."""
    n = len(blocks)
    if n == 0:
        return []
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(np.asarray([len(b) for b in blocks], np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(bytes(b) for b in blocks) + b"\0" * 8, np.uint8)
    return [bytes(r) for r in partset_roots_packed(engine, data, off, part_size)]


class CommitHashBatch:
    """Commits (tmed.types.Commit or PackedCommit) held as tmed_commit structs over their arrays,
    built once (repeated timing of the C call alone)."""

    def __init__(self, commits: Sequence):
        from .types import _CommitC, _commit_c
        n = self.n = len(commits)
        self.keep = []
        self.cs = (_CommitC * max(n, 1))()
        for i, c in enumerate(commits):
            self.cs[i] = _commit_c(c, self.keep)
        self.out = np.zeros((max(n, 1), 32), np.uint8)
        self.ok = np.zeros(max(n, 1), np.uint8)

    def run(self, engine):
        """(hashes u8[n,32], ok u8[n])"""
        if self.n:
            rc = _bind().tmed_commit_hashes(engine._h, ctypes.cast(self.cs, ctypes.c_void_p), self.n, _p(self.out),
                                            _p(self.ok))
            if rc != TMED_OK:
                raise TmedError(rc, "tmed_commit_hashes")
        return self.out[:self.n], self.ok[:self.n]


def commit_hashes_packed(engine, flags, addresses, ts_seconds, ts_nanos, sigs, sig_lens, commit_off,
                         address_lens=None):
    """Commit.Hash of commits [commit_off[c], commit_off[c+1]) over flat signature arrays (flags u8[N],
    addresses u8[N,20], ts_seconds i64[N], ts_nanos i32[N], sigs u8[N,64], sig_lens u32[N] or None,
    address_lens u32[N] or None): a CommitHashBatch whose structs point into those arrays."""
    from .types import BlockID, PackedCommit
    off = np.asarray(commit_off, np.int64)
    cs = []
    for c in range(off.shape[0] - 1):
        a, b = int(off[c]), int(off[c + 1])
        sl = np.full(b - a, 64, np.uint32) if sig_lens is None else sig_lens[a:b]
        cs.append(PackedCommit(0, 0, BlockID(), flags[a:b], addresses[a:b], ts_seconds[a:b], ts_nanos[a:b],
                               sigs[a:b], sl, None if address_lens is None else address_lens[a:b]))
    return CommitHashBatch(cs)


def commit_hashes(engine, commits: Sequence) -> list:
    """Commit.Hash() of every commit (tmed.types.Commit or PackedCommit); None where the flat arrays
    cannot reproduce it (a signature longer than 64 bytes, an address of another length than 0 or
    20) or the reference's Marshal fails and Hash panics (timestamp out of range): the caller
    runs the Go method for those."""
    out, ok = CommitHashBatch(commits).run(engine)
    return [bytes(out[i]) if ok[i] else None for i in range(len(commits))]


def txs_hashes_packed(engine, txs: np.ndarray, tx_off: np.ndarray, block_off: np.ndarray) -> np.ndarray:
    """Data.Hash of blocks [block_off[b], block_off[b+1]) over transactions txs[tx_off[i] .. tx_off[i+1])
    (u8 array, u64 offsets, u32 block offsets): an n_blocks x 32 array."""
    n = block_off.shape[0] - 1
    out = np.zeros((max(n, 1), 32), np.uint8)
    if n <= 0:
        return out[:0]
    rc = _bind().tmed_txs_hashes(engine._h, _p(txs), _p(np.ascontiguousarray(tx_off, np.uint64)),
                                 _p(np.ascontiguousarray(block_off, np.uint32)), n, _p(out))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_txs_hashes")
    return out[:n]


def txs_hashes(engine, blocks: Sequence[Sequence[bytes]]) -> list:
    """Data.Hash() = Txs.Hash() of every block's transactions."""
    if not blocks:
        return []
    flat = [bytes(t) for b in blocks for t in b]
    tx_off = np.zeros(len(flat) + 1, np.uint64)
    np.cumsum(np.asarray([len(t) for t in flat], np.uint64), out=tx_off[1:])
    block_off = np.zeros(len(blocks) + 1, np.uint32)
    np.cumsum(np.asarray([len(b) for b in blocks], np.uint32), out=block_off[1:])
    data = np.frombuffer(b"".join(flat) + b"\0" * 8, np.uint8)
    return [bytes(r) for r in txs_hashes_packed(engine, data, tx_off, block_off)]


# ---- Merkle proofs: ProofsFromByteSlices / Proof.Verify (crypto/merkle/proof.go:35-68) ----------
PROOF_OK, PROOF_NEGATIVE_TOTAL, PROOF_NEGATIVE_INDEX, PROOF_LEAF_HASH, PROOF_ROOT_HASH = range(5)


def _run_proofs(what: str, call, n_trees: int, n_leaves: int):
    """The sizing call (aunts = NULL: aunt_off and the byte count, on the host) and the real one.
    call(roots, leaf_hashes, aunt_off, aunts, aunts_cap, aunts_len) -> rc, pointers as c_void_p."""
    aunt_off = np.zeros(n_leaves + 1, np.uint64)
    need = ctypes.c_size_t(0)
    rc = call(None, None, _p(aunt_off), None, 0, ctypes.byref(need))
    if rc != TMED_OK:
        raise TmedError(rc, what + " (sizing)")
    roots = np.zeros((max(n_trees, 1), 32), np.uint8)
    leaf_hashes = np.zeros((max(n_leaves, 1), 32), np.uint8)
    aunts = np.zeros((need.value // 32 + 1, 32), np.uint8)
    rc = call(_p(roots), _p(leaf_hashes), _p(aunt_off), _p(aunts), need.value, ctypes.byref(need))
    if rc != TMED_OK:
        raise TmedError(rc, what)
    return roots[:n_trees], leaf_hashes[:n_leaves], aunt_off, aunts[:need.value // 32]


def merkle_proofs_packed(engine, data: np.ndarray, leaf_off: np.ndarray, tree_off: np.ndarray):
    """ProofsFromByteSlices of the trees of merkle_roots_packed: (roots u8[T,32], leaf_hashes
    u8[L,32], aunt_off u64[L+1] in hashes, aunts u8[A,32]); leaf i's aunts are
    aunts[aunt_off[i]:aunt_off[i+1]], its Total and Index its tree's leaf count and its position."""
    n = tree_off.shape[0] - 1
    if n <= 0:
        return (np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), np.zeros(1, np.uint64),
                np.zeros((0, 32), np.uint8))
    lo = np.ascontiguousarray(leaf_off, np.uint64)
    to = np.ascontiguousarray(tree_off, np.uint32)
    l, h = _bind(), engine._h
    return _run_proofs("tmed_merkle_proofs",
                       lambda r, lh, ao, a, cap, ln: l.tmed_merkle_proofs(h, _p(data), _p(lo), _p(to), n, r, lh, ao, a,
                                                                          cap, ln), n, int(to[-1]))


def partset_proofs_packed(engine, data: np.ndarray, off: np.ndarray, part_size: int = BLOCK_PART_SIZE_BYTES):
    """NewPartSetFromData of blocks data[off[b] .. off[b+1]): (roots, part_off u32[n+1], leaf_hashes,
    aunt_off, aunts); block b's parts are leaves part_off[b] .. part_off[b+1]."""
    n = off.shape[0] - 1
    if n <= 0:
        return (np.zeros((0, 32), np.uint8), np.zeros(1, np.uint32), np.zeros((0, 32), np.uint8),
                np.zeros(1, np.uint64), np.zeros((0, 32), np.uint8))
    do = np.ascontiguousarray(off, np.uint64)
    lens = (do[1:] - do[:-1]).astype(np.int64)
    n_leaves = int(((lens + part_size - 1) // part_size).sum())
    part_off = np.zeros(n + 1, np.uint32)
    l, h = _bind(), engine._h
    out = _run_proofs("tmed_partset_proofs",
                      lambda r, lh, ao, a, cap, ln: l.tmed_partset_proofs(h, _p(data), _p(do), n, part_size, r,
                                                                          _p(part_off), lh, ao, a, cap, ln),
                      n, n_leaves)
    return (out[0], part_off) + out[1:]


def txs_proofs_packed(engine, txs: np.ndarray, tx_off: np.ndarray, block_off: np.ndarray):
    """The trees of Txs.Proof (leaves SHA-256(tx)) for the blocks of txs_hashes_packed: (roots,
    leaf_hashes, aunt_off, aunts); leaf_hashes[i] = leafHash(tx_i.Hash())."""
    n = block_off.shape[0] - 1
    if n <= 0:
        return (np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8), np.zeros(1, np.uint64),
                np.zeros((0, 32), np.uint8))
    to = np.ascontiguousarray(tx_off, np.uint64)
    bo = np.ascontiguousarray(block_off, np.uint32)
    l, h = _bind(), engine._h
    return _run_proofs("tmed_txs_proofs",
                       lambda r, lh, ao, a, cap, ln: l.tmed_txs_proofs(h, _p(txs), _p(to), _p(bo), n, r, lh, ao, a,
                                                                       cap, ln), n, int(bo[-1]))


def verify_proofs_packed(engine, roots: np.ndarray, data: np.ndarray, leaf_off: np.ndarray, leaf_hashes: np.ndarray,
                         totals: np.ndarray, indexes: np.ndarray, aunt_off: np.ndarray, aunts: np.ndarray,
                         root_of: Optional[np.ndarray] = None) -> np.ndarray:
    """Proof.Verify for n proofs: codes u8[n] (PROOF_*).  Proof i proves leaf data[leaf_off[i] ..
    leaf_off[i+1]) under roots[root_of[i]] (root_of None: roots[i]) with Total totals[i], Index
    indexes[i], LeafHash leaf_hashes[i] and Aunts aunts[aunt_off[i]:aunt_off[i+1]]."""
    n = leaf_off.shape[0] - 1
    codes = np.zeros(max(n, 1), np.uint8)
    if n <= 0:
        return codes[:0]
    r = np.ascontiguousarray(roots, np.uint8).reshape(-1, 32)
    lh = np.ascontiguousarray(leaf_hashes, np.uint8).reshape(-1, 32)
    au = np.ascontiguousarray(aunts, np.uint8).reshape(-1, 32)
    if lh.shape[0] < n:
        raise ValueError("one leaf hash per proof")
    lo = np.ascontiguousarray(leaf_off, np.uint64)
    ao = np.ascontiguousarray(aunt_off, np.uint64)
    if ao.shape[0] != n + 1 or int(ao[-1]) > au.shape[0]:
        raise ValueError("aunt_off does not fit the aunts")
    tt = np.ascontiguousarray(totals, np.int64)
    ix = np.ascontiguousarray(indexes, np.int64)
    ro = None if root_of is None else np.ascontiguousarray(root_of, np.uint32)
    if tt.shape[0] != n or ix.shape[0] != n or (ro is not None and ro.shape[0] != n):
        raise ValueError("one total, one index and one root index per proof")
    rc = _bind().tmed_merkle_proofs_verify(engine._h, n, _p(r), r.shape[0], None if ro is None else _p(ro), _p(data),
                                           _p(lo), _p(lh), _p(tt), _p(ix), _p(ao), _p(au) if au.size else None,
                                           _p(codes))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_merkle_proofs_verify")
    return codes[:n]


def _flatten(groups):
    flat = [bytes(x) for g in groups for x in g]
    item_off = np.zeros(len(flat) + 1, np.uint64)
    np.cumsum(np.asarray([len(x) for x in flat], np.uint64), out=item_off[1:])
    group_off = np.zeros(len(groups) + 1, np.uint32)
    np.cumsum(np.asarray([len(g) for g in groups], np.uint32), out=group_off[1:])
    return np.frombuffer(b"".join(flat) + b"\0" * 8, np.uint8), item_off, group_off


def _proof_lists(roots, group_off, leaf_hashes, aunt_off, aunts) -> list:
    out = []
    for t in range(roots.shape[0]):
        a, b = int(group_off[t]), int(group_off[t + 1])
        proofs = [(b - a, i - a, bytes(leaf_hashes[i]),
                   [bytes(x) for x in aunts[int(aunt_off[i]):int(aunt_off[i + 1])]]) for i in range(a, b)]
        out.append((bytes(roots[t]), proofs))
    return out


def merkle_proofs(engine, trees: Sequence[Sequence[bytes]]) -> list:
    """ProofsFromByteSlices(tree) for every tree: [(root, [(total, index, leaf_hash, aunts), ...])]."""
    if not trees:
        return []
    data, leaf_off, tree_off = _flatten(trees)
    roots, lh, ao, au = merkle_proofs_packed(engine, data, leaf_off, tree_off)
    return _proof_lists(roots, tree_off, lh, ao, au)


def partset_proofs(engine, blocks: Sequence[bytes], part_size: int = BLOCK_PART_SIZE_BYTES) -> list:
    """NewPartSetFromData(block, part_size) for every block's bytes: [(root, [(total, index,
    leaf_hash, aunts) per part])]; part p's bytes are block[p * part_size:(p + 1) * part_size]."""
    if not blocks:
        return []
    off = np.zeros(len(blocks) + 1, np.uint64)
    np.cumsum(np.asarray([len(b) for b in blocks], np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(bytes(b) for b in blocks) + b"\0" * 8, np.uint8)
    roots, part_off, lh, ao, au = partset_proofs_packed(engine, data, off, part_size)
    return _proof_lists(roots, part_off, lh, ao, au)


def txs_proofs(engine, blocks: Sequence[Sequence[bytes]]) -> list:
    """The proofs of Txs.Proof for every transaction of every block: [(Data.Hash, [(total, index,
    leafHash(tx.Hash()), aunts) per tx])]."""
    if not blocks:
        return []
    data, tx_off, block_off = _flatten(blocks)
    roots, lh, ao, au = txs_proofs_packed(engine, data, tx_off, block_off)
    return _proof_lists(roots, block_off, lh, ao, au)


def verify_proofs(engine, items: Sequence) -> list:
    """Proof.Verify(root, leaf) for every (root, leaf, (total, index, leaf_hash, aunts)): the codes
    (PROOF_OK, or the first check that fails).  Hashes are 32 bytes each."""
    if not items:
        return []
    roots, leaves, lhs, tots, idxs, aunts, ao = [], [], [], [], [], [], [0]
    for root, leaf, (total, index, leaf_hash, au) in items:
        if len(root) != 32 or len(leaf_hash) != 32 or any(len(a) != 32 for a in au):
            raise ValueError("root, leaf hash and aunts are 32 bytes each")
        roots.append(bytes(root))
        leaves.append(bytes(leaf))
        lhs.append(bytes(leaf_hash))
        tots.append(total)
        idxs.append(index)
        aunts.extend(bytes(a) for a in au)
        ao.append(len(aunts))
    leaf_off = np.zeros(len(leaves) + 1, np.uint64)
    np.cumsum(np.asarray([len(x) for x in leaves], np.uint64), out=leaf_off[1:])
    data = np.frombuffer(b"".join(leaves) + b"\0" * 8, np.uint8)
    u8 = lambda hs: np.frombuffer(b"".join(hs), np.uint8).reshape(-1, 32)  # noqa: E731
    return [int(c) for c in verify_proofs_packed(engine, u8(roots), data, leaf_off, u8(lhs), np.asarray(tots, np.int64),
                                                 np.asarray(idxs, np.int64), np.asarray(ao, np.uint64), u8(aunts))]
