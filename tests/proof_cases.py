"""Merkle proofs restated from the reference (TEST INFRASTRUCTURE ONLY), in its own recursive
shape, which is deliberately not the device's level-wise one:

* ``crypto/merkle/proof.go:35-48``    ProofsFromByteSlices
* ``crypto/merkle/proof.go:216-237``  trailsFromByteSlices (split-point recursion over ProofNodes)
* ``crypto/merkle/proof.go:197-212``  FlattenAunts (a leaf's aunts, bottom-up)
* ``crypto/merkle/proof.go:151-181``  computeHashFromAunts
* ``crypto/merkle/proof.go:52-68``    Proof.Verify (as the code of the first check that fails)
* ``types/part_set.go:166-194``       NewPartSetFromData; ``types/tx.go:80-93`` Txs.Proof

Built on oracle/merkle.py's leaf_hash, inner_hash and split_point.
"""
from __future__ import annotations

import hashlib

from oracle.merkle import empty_hash, inner_hash, leaf_hash, split_point

PROOF_OK, PROOF_NEGATIVE_TOTAL, PROOF_NEGATIVE_INDEX, PROOF_LEAF_HASH, PROOF_ROOT_HASH = range(5)

EMPTY_HASH = "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"  # tree_test.go:47

# the totals past 2^32 the issue names, and the indexes tried at each
LARGE_TOTALS = (2 ** 32, 2 ** 32 + 1, 2 ** 62 + 3, 2 ** 63 - 1)


class ProofNode:
    __slots__ = ("hash", "parent", "left", "right")

    def __init__(self, h):
        self.hash, self.parent, self.left, self.right = h, None, None, None

    def flatten_aunts(self):
        out, n = [], self
        while n is not None:
            if n.left is not None:
                out.append(n.left.hash)
            elif n.right is not None:
                out.append(n.right.hash)
            n = n.parent
        return out


def trails_from_byte_slices(items):
    if len(items) == 0:
        return [], ProofNode(empty_hash())
    if len(items) == 1:
        t = ProofNode(leaf_hash(bytes(items[0])))
        return [t], t
    k = split_point(len(items))
    lefts, left_root = trails_from_byte_slices(items[:k])
    rights, right_root = trails_from_byte_slices(items[k:])
    root = ProofNode(inner_hash(left_root.hash, right_root.hash))
    left_root.parent = root
    left_root.right = right_root
    right_root.parent = root
    right_root.left = left_root
    return lefts + rights, root


def proofs_from_byte_slices(items):
    """(root, [(total, index, leaf_hash, aunts)])"""
    trails, root = trails_from_byte_slices(list(items))
    return root.hash, [(len(items), i, t.hash, t.flatten_aunts()) for i, t in enumerate(trails)]


def compute_hash_from_aunts(index, total, leaf_hash_, aunts):
    """None is Go's nil."""
    if index >= total or index < 0 or total <= 0:
        return None
    if total == 1:
        return None if len(aunts) != 0 else leaf_hash_
    if len(aunts) == 0:
        return None
    num_left = split_point(total)
    if index < num_left:
        left = compute_hash_from_aunts(index, num_left, leaf_hash_, aunts[:-1])
        return None if left is None else inner_hash(left, aunts[-1])
    right = compute_hash_from_aunts(index - num_left, total - num_left, leaf_hash_, aunts[:-1])
    return None if right is None else inner_hash(aunts[-1], right)


def verify(root, leaf, total, index, leaf_hash_, aunts):
    """Proof{total, index, leaf_hash_, aunts}.Verify(root, leaf) as a code (root is 32 bytes, so a nil
    computed hash never equals it)."""
    if total < 0:
        return PROOF_NEGATIVE_TOTAL
    if index < 0:
        return PROOF_NEGATIVE_INDEX
    if leaf_hash(bytes(leaf)) != bytes(leaf_hash_):
        return PROOF_LEAF_HASH
    if compute_hash_from_aunts(index, total, bytes(leaf_hash_), [bytes(a) for a in aunts]) != bytes(root):
        return PROOF_ROOT_HASH
    return PROOF_OK


def path_sides(index, total):
    """The shape of computeHashFromAunts' recursion alone: None where it returns nil whatever the
    aunts; else one entry per aunt it consumes, bottom-up (Proof.Aunts order): 1 = the aunt is the
    left input of innerHash, 0 = the right one."""
    if index >= total or index < 0 or total <= 0:
        return None
    if total == 1:
        return []
    k = split_point(total)
    if index < k:
        return path_sides(index, k) + [0]
    return path_sides(index - k, total - k) + [1]


def partset_proofs(data: bytes, part_size: int):
    return proofs_from_byte_slices([data[i:i + part_size] for i in range(0, len(data), part_size)])


def txs_proofs(txs):
    """The tree of Txs.Proof: leaves are tx.Hash() = SHA-256(tx)."""
    return proofs_from_byte_slices([hashlib.sha256(bytes(t)).digest() for t in txs])


def large_indexes(total):
    return (0, total - 1, total // 2)
