"""Host mirror of ``Vote.Verify`` (reference ``types/vote.go:147-156``) and the checks
``VoteSet.addVote`` runs in front of it (``types/vote_set.go:156-218``) over the C ABI
``tmed_verify_votes``: batches of free-standing votes, each batch against a validator set, one
outcome code per vote (kernel in ``csrc/votes.hip``, the encoder and the checks in
``csrc/vote_free.h``, the same source on the host through ``tmed_verify_votes_host`` and
``tmed_votes_sign_bytes``).  ``VoteSet``'s state (duplicates, conflicting votes, maj23) stays with
the caller.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from . import types as T
from ._native import TMED_OK, TmedError

(VOTE_OK, VOTE_INDEX_NEGATIVE, VOTE_ADDRESS_EMPTY, VOTE_UNEXPECTED_STEP, VOTE_INDEX_NOT_IN_SET,
 VOTE_ADDRESS_NOT_IN_SET, VOTE_ADDRESS_NOT_OF_KEY, VOTE_PANIC, VOTE_INVALID_SIGNATURE, VOTE_GO_PATH) = range(10)
VOTES_ADDVOTE = 1
CODE_NAMES = ["OK", "INDEX_NEGATIVE", "ADDRESS_EMPTY", "UNEXPECTED_STEP", "INDEX_NOT_IN_SET", "ADDRESS_NOT_IN_SET",
              "ADDRESS_NOT_OF_KEY", "PANIC", "INVALID_SIGNATURE", "GO_PATH"]


@dataclass
class Vote:
    """types.Vote (types/vote.go:50-59); timestamp = (Unix seconds, nanoseconds)."""
    type: int
    height: int
    round: int
    block_id: T.BlockID
    timestamp: tuple
    validator_address: bytes
    validator_index: int
    signature: bytes = b""


@dataclass
class VoteRequest:
    """One batch: votes against a validator set.  ``addvote``: the checks of VoteSet.addVote against the
    VoteSet's step (height, round, type) in front of Vote.Verify; else Vote.Verify with the key at
    each vote's validator_index."""
    chain_id: str
    vals: T.ValidatorSet
    votes: List[Vote]
    addvote: bool = False
    height: int = 0
    round: int = 0
    type: int = 0


# The sentinel errors of types/vote.go:20-26 that addVote wraps (fmt.Errorf("...: %w", Err...)).
class ErrVoteUnexpectedStep(T.GoError):
    def __init__(self):
        super().__init__("unexpected step")


class ErrVoteInvalidValidatorIndex(T.GoError):
    def __init__(self):
        super().__init__("invalid validator index")


class ErrVoteInvalidValidatorAddress(T.GoError):
    def __init__(self):
        super().__init__("invalid validator address")


class ErrVoteInvalidSignature(T.GoError):
    def __init__(self):
        super().__init__("invalid signature")


class VotePanic(RuntimeError):
    """VoteSignBytes panics for this vote (TMED_VOTE_PANIC): a malformed BlockID hash."""


class VoteGoPath(RuntimeError):
    """The caller runs the reference's own path for this vote (TMED_VOTE_GO_PATH)."""


_ERRORS = {VOTE_INDEX_NEGATIVE: ErrVoteInvalidValidatorIndex, VOTE_ADDRESS_EMPTY: ErrVoteInvalidValidatorAddress,
           VOTE_UNEXPECTED_STEP: ErrVoteUnexpectedStep, VOTE_INDEX_NOT_IN_SET: ErrVoteInvalidValidatorIndex,
           VOTE_ADDRESS_NOT_IN_SET: ErrVoteInvalidValidatorAddress, VOTE_ADDRESS_NOT_OF_KEY: ErrVoteInvalidValidatorAddress,
           VOTE_INVALID_SIGNATURE: ErrVoteInvalidSignature, VOTE_PANIC: VotePanic, VOTE_GO_PATH: VoteGoPath}


def to_error(code: int):
    """None for VOTE_OK, else the ErrVote* value addVote wraps (VotePanic / VoteGoPath objects for those codes)."""
    return None if code == VOTE_OK else _ERRORS[code]()


class _VotesC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t)] + [(f, ctypes.c_void_p) for f in (
        "types", "heights", "rounds", "block_hashes", "block_hash_lens", "psh_totals", "psh_hashes", "psh_hash_lens",
        "ts_seconds", "ts_nanos", "addresses", "address_lens", "validator_indexes", "sigs", "sig_lens")]


class _VoteRequestC(ctypes.Structure):
    _fields_ = [("chain_id", ctypes.c_char_p), ("chain_id_len", ctypes.c_uint32), ("vals", ctypes.POINTER(T._ValsetC)),
                ("votes", ctypes.POINTER(_VotesC)), ("flags", ctypes.c_uint32), ("height", ctypes.c_int64),
                ("round", ctypes.c_int32), ("msg_type", ctypes.c_int32)]


def _bind():
    l = T._bind()
    if l.tmed_verify_votes.argtypes is None:
        P = ctypes.c_void_p
        l.tmed_verify_votes.restype = ctypes.c_int
        l.tmed_verify_votes.argtypes = [P, ctypes.POINTER(_VoteRequestC), ctypes.c_size_t, P]
        l.tmed_verify_votes_host.restype = ctypes.c_int
        l.tmed_verify_votes_host.argtypes = [ctypes.POINTER(_VoteRequestC), ctypes.c_size_t, P, P, P]
        l.tmed_votes_sign_bytes.restype = ctypes.c_int
        l.tmed_votes_sign_bytes.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(_VotesC), P, ctypes.c_size_t,
                                            P, ctypes.POINTER(ctypes.c_size_t), P]
        l.tmed_votes_last_prepare_ms.restype = ctypes.c_float
        l.tmed_votes_last_prepare_ms.argtypes = [P]
    return l


class PackedVotes:
    """tmed_votes: the votes' fields as flat arrays (every length array present)."""

    def __init__(self, votes: Sequence[Vote]):
        n = self.n = len(votes)
        m = max(n, 1)
        self.types = np.zeros(m, np.int32)
        self.heights = np.zeros(m, np.int64)
        self.rounds = np.zeros(m, np.int32)
        self.block_hashes = np.zeros((m, 32), np.uint8)
        self.block_hash_lens = np.zeros(m, np.uint32)
        self.psh_totals = np.zeros(m, np.uint32)
        self.psh_hashes = np.zeros((m, 32), np.uint8)
        self.psh_hash_lens = np.zeros(m, np.uint32)
        self.ts_seconds = np.zeros(m, np.int64)
        self.ts_nanos = np.zeros(m, np.int32)
        self.addresses = np.zeros((m, 20), np.uint8)
        self.address_lens = np.zeros(m, np.uint32)
        self.validator_indexes = np.zeros(m, np.int32)
        self.sigs = np.zeros((m, 64), np.uint8)
        self.sig_lens = np.zeros(m, np.uint32)
        for i, v in enumerate(votes):
            self.types[i], self.heights[i], self.rounds[i] = v.type, v.height, v.round
            for arr, lens, b, w in ((self.block_hashes, self.block_hash_lens, v.block_id.hash, 32),
                                    (self.psh_hashes, self.psh_hash_lens, v.block_id.psh_hash, 32),
                                    (self.addresses, self.address_lens, v.validator_address, 20),
                                    (self.sigs, self.sig_lens, v.signature, 64)):
                b = bytes(b)
                lens[i] = len(b)
                if b:
                    arr[i, :min(len(b), w)] = np.frombuffer(b[:w], np.uint8)
            self.psh_totals[i] = v.block_id.psh_total
            self.ts_seconds[i], self.ts_nanos[i] = v.timestamp
            self.validator_indexes[i] = v.validator_index
        self.c = _VotesC(n, *[T._ptr(getattr(self, f)) for f, _ in _VotesC._fields_[1:]])

    _DTYPES = dict(types=np.int32, heights=np.int64, rounds=np.int32, block_hashes=np.uint8, block_hash_lens=np.uint32,
                   psh_totals=np.uint32, psh_hashes=np.uint8, psh_hash_lens=np.uint32, ts_seconds=np.int64,
                   ts_nanos=np.int32, addresses=np.uint8, address_lens=np.uint32, validator_indexes=np.int32,
                   sigs=np.uint8, sig_lens=np.uint32)

    @classmethod
    def from_arrays(cls, **arrays):
        """The same from ready arrays, one per field of tmed_votes (bulk workloads)."""
        self = cls.__new__(cls)
        if set(arrays) != set(cls._DTYPES):
            raise ValueError("PackedVotes.from_arrays: one array per tmed_votes field")
        self.n = int(np.asarray(arrays["types"]).shape[0])
        for f, dt in cls._DTYPES.items():
            setattr(self, f, np.ascontiguousarray(arrays[f], dt))
        self.c = _VotesC(self.n, *[T._ptr(getattr(self, f)) for f, _ in _VotesC._fields_[1:]])
        return self


class PreparedVotes:
    """Requests packed into C structs once (repeated timing of the C call alone); one tmed_valset per
    ValidatorSet object."""

    def __init__(self, requests: Sequence[VoteRequest]):
        self.requests = list(requests)
        n = self.n = len(self.requests)
        self.keep = []
        self.reqs = (_VoteRequestC * max(n, 1))()
        vcs = {}
        self.total = 0
        for q, r in enumerate(self.requests):
            vc = vcs.get(id(r.vals))
            if vc is None:
                vc = vcs[id(r.vals)] = T._valset_c(r.vals, self.keep)
            pv = r.votes if isinstance(r.votes, PackedVotes) else PackedVotes(r.votes)
            cid = r.chain_id.encode() if isinstance(r.chain_id, str) else bytes(r.chain_id)
            self.keep.extend([vc, pv, cid])
            self.reqs[q] = _VoteRequestC(cid, len(cid), ctypes.pointer(vc), ctypes.pointer(pv.c),
                                         VOTES_ADDVOTE if r.addvote else 0, r.height, r.round, r.type)
            self.total += pv.n
        self.codes = np.zeros(max(self.total, 1), np.uint8)
        self.msg_lens = np.zeros(max(self.total, 1), np.uint32)
        self.device_route = np.zeros(max(n, 1), np.uint8)

    def run(self, engine):
        """tmed_verify_votes on ``engine``; ``engine=None``: tmed_verify_votes_host (prechecks only)."""
        l = _bind()
        if engine is None:
            rc = l.tmed_verify_votes_host(self.reqs, self.n, T._ptr(self.codes), T._ptr(self.msg_lens),
                                          T._ptr(self.device_route))
        else:
            rc = l.tmed_verify_votes(engine._h, self.reqs, self.n, T._ptr(self.codes))
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_verify_votes")
        return self.codes[:self.total]


def verify_votes(engine, requests: Sequence[VoteRequest]):
    """One outcome code per vote (``VOTE_*``), the requests' votes behind each other, from ONE device
    batch.  engine=None: the checks in front of the signature only, on the host (0 = the signature
    would decide).  ``to_error(code)`` gives the reference's error value."""
    pv = PreparedVotes(requests)
    return pv.run(engine).copy()


def last_prepare_ms(engine) -> float:
    """vote_prepare_kernel's device time in the engine's last verify_votes call."""
    return float(_bind().tmed_votes_last_prepare_ms(engine._h))


def sign_bytes_arrays(chain_id, votes):
    """``VoteSignBytes`` of every vote as (flat u8 array, u32 offsets[n+1], malformed u8[n]): the two
    tmed_votes_sign_bytes calls (size, fill) and nothing else."""
    l = _bind()
    pv = votes if isinstance(votes, PackedVotes) else PackedVotes(votes)
    cid = chain_id.encode() if isinstance(chain_id, str) else bytes(chain_id)
    off = np.zeros(pv.n + 1, np.uint32)
    bad = np.zeros(max(pv.n, 1), np.uint8)
    total = ctypes.c_size_t(0)
    rc = l.tmed_votes_sign_bytes(cid, len(cid), ctypes.byref(pv.c), None, 0, T._ptr(off), ctypes.byref(total), T._ptr(bad))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_votes_sign_bytes")
    out = np.zeros(total.value + 16, np.uint8)
    rc = l.tmed_votes_sign_bytes(cid, len(cid), ctypes.byref(pv.c), T._ptr(out), total.value, T._ptr(off),
                                 ctypes.byref(total), T._ptr(bad))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_votes_sign_bytes")
    return out[:total.value], off, bad[:pv.n]


def sign_bytes(chain_id, votes: Sequence[Vote]):
    """``VoteSignBytes(chainID, vote)`` of every vote (tmed_votes_sign_bytes): a list of bytes, None where
    the vote's BlockID is malformed (the reference panics)."""
    flat, off, bad = sign_bytes_arrays(chain_id, votes)
    raw = flat.tobytes()
    return [None if bad[i] else raw[off[i]:off[i + 1]] for i in range(len(bad))]
