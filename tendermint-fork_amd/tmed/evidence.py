"""Host mirror of ``VerifyDuplicateVote`` (reference ``evidence/verify.go:162-222``),
``DuplicateVoteEvidence.Hash`` / ``Bytes`` (``types/evidence.go:90-103``) and ``EvidenceList.Hash``
(``:431-442``) over the C ABI ``tmed_verify_duplicate_votes`` / ``tmed_evidence_hashes``: batches of
duplicate-vote evidence, each batch against the validator set of its height, one outcome code per
evidence (kernels in ``csrc/evidence.hip``, the checks and the ``Bytes()`` encoder in
``csrc/evidence_free.h``, the same source on the host through ``tmed_verify_duplicate_votes_host``
and ``tmed_evidence_bytes``).  ``ValidateBasic``, the age checks and the pool's lookups stay with
the caller.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import types as T
from ._native import TMED_OK, TmedError
from .votes import ErrVoteInvalidSignature, PackedVotes, Vote, _VotesC

(DUPVOTE_OK, DUPVOTE_NOT_A_VALIDATOR, DUPVOTE_HRS_MISMATCH, DUPVOTE_ADDRESS_MISMATCH, DUPVOTE_SAME_BLOCK_ID,
 DUPVOTE_ADDRESS_NOT_OF_KEY, DUPVOTE_VALIDATOR_POWER, DUPVOTE_TOTAL_POWER, DUPVOTE_PANIC, DUPVOTE_VOTE_A_SIGNATURE,
 DUPVOTE_VOTE_B_SIGNATURE, DUPVOTE_GO_PATH) = range(12)
CODE_NAMES = ["OK", "NOT_A_VALIDATOR", "HRS_MISMATCH", "ADDRESS_MISMATCH", "SAME_BLOCK_ID", "ADDRESS_NOT_OF_KEY",
              "VALIDATOR_POWER", "TOTAL_POWER", "PANIC", "VOTE_A_SIGNATURE", "VOTE_B_SIGNATURE", "GO_PATH"]


@dataclass
class DuplicateVoteEvidence:
    """types.DuplicateVoteEvidence (types/evidence.go:35-47); timestamp = (Unix seconds, nanoseconds)."""
    vote_a: Vote
    vote_b: Vote
    total_voting_power: int = 0
    validator_power: int = 0
    timestamp: tuple = T.ZERO_TIME


@dataclass
class EvidenceRequest:
    """One batch: evidences against the validator set of their height."""
    chain_id: str
    vals: T.ValidatorSet
    evidence: List[DuplicateVoteEvidence]


# One class per failing check of VerifyDuplicateVote; str() is the reference's message where it
# depends on nothing the code does not carry.
class ErrNotAValidator(T.GoError):
    def __init__(self):
        super().__init__("address was not a validator at the evidence's height")


class ErrHRSMismatch(T.GoError):
    def __init__(self):
        super().__init__("h/r/s does not match")


class ErrAddressMismatch(T.GoError):
    def __init__(self):
        super().__init__("validator addresses do not match")


class ErrSameBlockID(T.GoError):
    def __init__(self):
        super().__init__("block IDs are the same - not a real duplicate vote")


class ErrAddressNotOfKey(T.GoError):
    def __init__(self):
        super().__init__("address doesn't match pubkey")


class ErrValidatorPower(T.GoError):
    def __init__(self):
        super().__init__("validator power from evidence and our validator set does not match")


class ErrTotalPower(T.GoError):
    def __init__(self):
        super().__init__("total voting power from the evidence and our validator set does not match")


class ErrVoteASignature(ErrVoteInvalidSignature):
    """fmt.Errorf("verifying VoteA: %w", ErrVoteInvalidSignature)"""

    def __str__(self):
        return "verifying VoteA: invalid signature"


class ErrVoteBSignature(ErrVoteInvalidSignature):
    """fmt.Errorf("verifying VoteB: %w", ErrVoteInvalidSignature)"""

    def __str__(self):
        return "verifying VoteB: invalid signature"


class EvidencePanic(RuntimeError):
    """VoteSignBytes panics for the vote under test (TMED_DUPVOTE_PANIC): a malformed BlockID hash."""


class EvidenceGoPath(RuntimeError):
    """The caller runs the reference's own path for this evidence (TMED_DUPVOTE_GO_PATH)."""


_ERRORS = {DUPVOTE_NOT_A_VALIDATOR: ErrNotAValidator, DUPVOTE_HRS_MISMATCH: ErrHRSMismatch,
           DUPVOTE_ADDRESS_MISMATCH: ErrAddressMismatch, DUPVOTE_SAME_BLOCK_ID: ErrSameBlockID,
           DUPVOTE_ADDRESS_NOT_OF_KEY: ErrAddressNotOfKey, DUPVOTE_VALIDATOR_POWER: ErrValidatorPower,
           DUPVOTE_TOTAL_POWER: ErrTotalPower, DUPVOTE_PANIC: EvidencePanic, DUPVOTE_VOTE_A_SIGNATURE: ErrVoteASignature,
           DUPVOTE_VOTE_B_SIGNATURE: ErrVoteBSignature, DUPVOTE_GO_PATH: EvidenceGoPath}


def to_error(code: int):
    """None for DUPVOTE_OK, else an object of the class of the check that failed."""
    return None if code == DUPVOTE_OK else _ERRORS[int(code)]()


class _DupEvidenceC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("votes", _VotesC), ("total_voting_powers", ctypes.c_void_p),
                ("validator_powers", ctypes.c_void_p), ("ts_seconds", ctypes.c_void_p), ("ts_nanos", ctypes.c_void_p)]


class _DupRequestC(ctypes.Structure):
    _fields_ = [("chain_id", ctypes.c_char_p), ("chain_id_len", ctypes.c_uint32), ("vals", ctypes.POINTER(T._ValsetC)),
                ("ev", ctypes.POINTER(_DupEvidenceC))]


def _bind():
    l = T._bind()
    if l.tmed_verify_duplicate_votes.argtypes is None:
        P = ctypes.c_void_p
        l.tmed_verify_duplicate_votes.restype = ctypes.c_int
        l.tmed_verify_duplicate_votes.argtypes = [P, ctypes.POINTER(_DupRequestC), ctypes.c_size_t, P]
        l.tmed_verify_duplicate_votes_host.restype = ctypes.c_int
        l.tmed_verify_duplicate_votes_host.argtypes = [ctypes.POINTER(_DupRequestC), ctypes.c_size_t, P, P, P, P, P]
        l.tmed_evidence_bytes.restype = ctypes.c_int
        l.tmed_evidence_bytes.argtypes = [ctypes.POINTER(_DupEvidenceC), P, ctypes.c_size_t, P,
                                          ctypes.POINTER(ctypes.c_size_t), P]
        l.tmed_evidence_hashes.restype = ctypes.c_int
        l.tmed_evidence_hashes.argtypes = [P, ctypes.POINTER(_DupEvidenceC), P, P, ctypes.c_size_t, P, P, P, P, P, P]
        l.tmed_evidence_kernel_times.restype = ctypes.c_int
        l.tmed_evidence_kernel_times.argtypes = [P, ctypes.POINTER(ctypes.c_float * 2)]
    return l


class PackedEvidence:
    """tmed_dup_evidence: the evidences' votes (VoteA at 2i, VoteB at 2i + 1) and own fields as flat arrays."""

    def __init__(self, evidence: Sequence[DuplicateVoteEvidence]):
        votes = []
        for e in evidence:
            votes += [e.vote_a, e.vote_b]
        self._fill(PackedVotes(votes), [e.total_voting_power for e in evidence], [e.validator_power for e in evidence],
                   [e.timestamp[0] for e in evidence], [e.timestamp[1] for e in evidence])

    def _fill(self, votes: PackedVotes, total, power, sec, nanos):
        n = self.n = votes.n // 2
        if votes.n != 2 * n:
            raise ValueError("PackedEvidence: two votes per evidence")
        self.votes = votes
        for name, values, dt in (("total_voting_powers", total, np.int64), ("validator_powers", power, np.int64),
                                 ("ts_seconds", sec, np.int64), ("ts_nanos", nanos, np.int32)):
            arr = np.zeros(max(n, 1), dt)
            arr[:n] = np.asarray(values, dt)
            setattr(self, name, arr)
        self.c = _DupEvidenceC(n, votes.c, T._ptr(self.total_voting_powers), T._ptr(self.validator_powers),
                               T._ptr(self.ts_seconds), T._ptr(self.ts_nanos))

    @classmethod
    def from_arrays(cls, votes: PackedVotes, total_voting_powers, validator_powers, ts_seconds, ts_nanos):
        """The same from a PackedVotes of 2n votes and one array per evidence field (bulk workloads)."""
        self = cls.__new__(cls)
        self._fill(votes, np.asarray(total_voting_powers), np.asarray(validator_powers), np.asarray(ts_seconds),
                   np.asarray(ts_nanos))
        return self


def _packed(evidence) -> PackedEvidence:
    return evidence if isinstance(evidence, PackedEvidence) else PackedEvidence(evidence)


class PreparedEvidence:
    """Requests packed into C structs once (repeated timing of the C call alone); one tmed_valset per
    ValidatorSet object."""

    def __init__(self, requests: Sequence[EvidenceRequest]):
        self.requests = list(requests)
        n = self.n = len(self.requests)
        self.keep = []
        self.reqs = (_DupRequestC * max(n, 1))()
        vcs = {}
        self.total = 0
        for q, r in enumerate(self.requests):
            vc = vcs.get(id(r.vals))
            if vc is None:
                vc = vcs[id(r.vals)] = T._valset_c(r.vals, self.keep)
            pe = _packed(r.evidence)
            cid = r.chain_id.encode() if isinstance(r.chain_id, str) else bytes(r.chain_id)
            self.keep.extend([vc, pe, cid])
            self.reqs[q] = _DupRequestC(cid, len(cid), ctypes.pointer(vc), ctypes.pointer(pe.c))
            self.total += pe.n
        m = max(self.total, 1)
        self.codes = np.zeros(m, np.uint8)
        self.vote_states = np.zeros(2 * m, np.uint8)
        self.found = np.zeros(m, np.int32)
        self.msg_lens = np.zeros(2 * m, np.uint32)
        self.device_route = np.zeros(max(n, 1), np.uint8)

    def run(self, engine):
        """tmed_verify_duplicate_votes on ``engine``; ``engine=None``: tmed_verify_duplicate_votes_host
        (the pre-codes; vote_states, found, msg_lens and device_route are filled beside them)."""
        l = _bind()
        if engine is None:
            rc = l.tmed_verify_duplicate_votes_host(self.reqs, self.n, T._ptr(self.codes), T._ptr(self.vote_states),
                                                    T._ptr(self.found), T._ptr(self.msg_lens), T._ptr(self.device_route))
        else:
            rc = l.tmed_verify_duplicate_votes(engine._h, self.reqs, self.n, T._ptr(self.codes))
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_verify_duplicate_votes")
        return self.codes[:self.total]


def verify_duplicate_votes(engine, requests: Sequence[EvidenceRequest]):
    """One outcome code per evidence (``DUPVOTE_*``), the requests' evidences behind each other, from ONE
    device batch.  engine=None: the checks in front of the signatures only, on the host.
    ``to_error(code)`` gives an object of the failing check's class."""
    return PreparedEvidence(requests).run(engine).copy()


def verify_duplicate_vote(engine, chain_id, vals, evidence: DuplicateVoteEvidence):
    """VerifyDuplicateVote(e, chainID, valSet): None, or the error value of the failing check (as the
    reference returns it); EvidencePanic / EvidenceGoPath are raised: the caller runs the Go function."""
    err = to_error(verify_duplicate_votes(engine, [EvidenceRequest(chain_id, vals, [evidence])])[0])
    if isinstance(err, RuntimeError):
        raise err
    return err


def last_kernel_times(engine):
    """(evidence_lookup_kernel ms, evidence_prepare_kernel ms) of the engine's last verify_duplicate_votes."""
    ms = (ctypes.c_float * 2)()
    rc = _bind().tmed_evidence_kernel_times(engine._h, ctypes.byref(ms))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_evidence_kernel_times")
    return float(ms[0]), float(ms[1])


def evidence_bytes_arrays(evidence):
    """``Bytes()`` of every evidence as (flat u8 array, u32 offsets[n+1], ok u8[n]): the two
    tmed_evidence_bytes calls (size, fill) and nothing else."""
    l = _bind()
    pe = _packed(evidence)
    off = np.zeros(pe.n + 1, np.uint32)
    ok = np.zeros(max(pe.n, 1), np.uint8)
    total = ctypes.c_size_t(0)
    rc = l.tmed_evidence_bytes(ctypes.byref(pe.c), None, 0, T._ptr(off), ctypes.byref(total), T._ptr(ok))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_evidence_bytes")
    out = np.zeros(total.value + 16, np.uint8)
    rc = l.tmed_evidence_bytes(ctypes.byref(pe.c), T._ptr(out), total.value, T._ptr(off), ctypes.byref(total), T._ptr(ok))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_evidence_bytes")
    return out[:total.value], off, ok[:pe.n]


def evidence_bytes(evidence: Sequence[DuplicateVoteEvidence]):
    """``DuplicateVoteEvidence.Bytes()`` of every evidence (tmed_evidence_bytes): a list of bytes, None
    where the struct cannot reproduce them (the reference panics, or bytes that are not carried)."""
    flat, off, ok = evidence_bytes_arrays(evidence)
    raw = flat.tobytes()
    return [raw[off[i]:off[i + 1]] if ok[i] else None for i in range(len(ok))]


def evidence_hashes_packed(engine, evidence, items: np.ndarray, list_off: np.ndarray, opaque: Optional[np.ndarray] = None,
                           opaque_off: Optional[np.ndarray] = None):
    """tmed_evidence_hashes on ready arrays: (ev_hashes u8[n,32], roots u8[T,32], ev_ok u8[n], list_ok u8[T])."""
    pe = _packed(evidence)
    items = np.ascontiguousarray(items, np.int64)
    list_off = np.ascontiguousarray(list_off, np.uint32)
    T_ = max(list_off.shape[0] - 1, 0)
    evh = np.zeros((max(pe.n, 1), 32), np.uint8)
    roots = np.zeros((max(T_, 1), 32), np.uint8)
    ev_ok = np.zeros(max(pe.n, 1), np.uint8)
    list_ok = np.zeros(max(T_, 1), np.uint8)
    if opaque is not None:
        opaque = np.ascontiguousarray(opaque, np.uint8)
        opaque_off = np.ascontiguousarray(opaque_off, np.uint64)
    rc = _bind().tmed_evidence_hashes(engine._h, ctypes.byref(pe.c), T._ptr(items) if items.size else None,
                                      T._ptr(list_off) if T_ else None, T_,
                                      T._ptr(opaque) if opaque is not None and opaque.size else None,
                                      T._ptr(opaque_off) if opaque_off is not None else None, T._ptr(evh), T._ptr(roots),
                                      T._ptr(ev_ok), T._ptr(list_ok))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_evidence_hashes")
    return evh[:pe.n], roots[:T_], ev_ok[:pe.n], list_ok[:T_]


def evidence_hashes(engine, evidence: Sequence[DuplicateVoteEvidence], lists: Sequence[Sequence] = ()):
    """``DuplicateVoteEvidence.Hash()`` of every evidence and ``EvidenceList.Hash()`` of every list.  A list
    item is an index into ``evidence`` or a ``bytes`` object (an evidence of another kind, already
    marshalled by the caller).  Returns (hashes, roots): lists of 32-byte values, None where the struct
    cannot reproduce the hash (ev_ok / list_ok = 0: the caller runs the Go method)."""
    items, list_off, blobs = [], [0], []
    for lst in lists:
        for it in lst:
            if isinstance(it, (bytes, bytearray)):
                items.append(-1 - len(blobs))
                blobs.append(bytes(it))
            else:
                items.append(int(it))
        list_off.append(len(items))
    op_off = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(np.asarray([len(b) for b in blobs], np.uint64), out=op_off[1:])
    opaque = np.frombuffer(b"".join(blobs) + b"\0" * 8, np.uint8)
    evh, roots, ev_ok, list_ok = evidence_hashes_packed(engine, evidence, np.asarray(items, np.int64),
                                                        np.asarray(list_off, np.uint32), opaque if blobs else None,
                                                        op_off if blobs else None)
    return ([bytes(h) if ok else None for h, ok in zip(evh, ev_ok)],
            [bytes(r) if ok else None for r, ok in zip(roots, list_ok)])
