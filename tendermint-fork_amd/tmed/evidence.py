"""Host mirror of ``VerifyDuplicateVote`` (reference ``evidence/verify.go:162-222``),
``DuplicateVoteEvidence.Hash`` / ``Bytes`` (``types/evidence.go:90-103``) and ``EvidenceList.Hash``
(``:431-442``) over the C ABI ``tmed_verify_duplicate_votes`` / ``tmed_evidence_hashes``: batches of
duplicate-vote evidence, each batch against the validator set of its height, one outcome code per
evidence (kernels in ``csrc/evidence.hip``, the checks and the ``Bytes()`` encoder in
``csrc/evidence_free.h``, the same source on the host through ``tmed_verify_duplicate_votes_host``
and ``tmed_evidence_bytes``).  ``ValidateBasic``, the age checks and the pool's lookups stay with
the caller.

``VerifyLightClientAttack`` (``evidence/verify.go:113-154``), ``GetByzantineValidators`` and
``LightClientAttackEvidence.Hash`` (``types/evidence.go:233-309``) follow at the end of the module, over
``tmed_verify_light_client_attacks`` / ``tmed_byzantine_validators`` (kernels in ``csrc/lca.hip``, the rule
in ``csrc/lca_free.h``, the replay in ``csrc/lca_host.h``).
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


def to_error(code, request=None):
    """None for DUPVOTE_OK, else an object of the class of the check that failed.  Given one result of
    ``verify_light_client_attacks`` and its ``LcaRequest``: VerifyLightClientAttack's error value."""
    if isinstance(code, _LcaResultC):
        return _lca_to_error(code, request)
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


# --------------------------------------------------------------------------- LightClientAttackEvidence

(LCA_OK, LCA_TRUSTING, LCA_NOT_DERIVED, LCA_COMMIT, LCA_TOTAL_POWER, LCA_TIME_NOT_VIOLATED, LCA_SAME_HASH,
 LCA_AMNESIA_HAS_VALIDATORS, LCA_BYZ_COUNT, LCA_BYZ_ADDRESS, LCA_BYZ_POWER, LCA_PANIC, LCA_GO_PATH) = range(13)
LCA_CODE_NAMES = ["OK", "TRUSTING", "NOT_DERIVED", "COMMIT", "TOTAL_POWER", "TIME_NOT_VIOLATED", "SAME_HASH",
                  "AMNESIA_HAS_VALIDATORS", "BYZ_COUNT", "BYZ_ADDRESS", "BYZ_POWER", "PANIC", "GO_PATH"]
LCA_LUNATIC, LCA_EQUIVOCATION, LCA_AMNESIA = range(3)
BYZ_OK, BYZ_PANIC = range(2)


@dataclass
class LightClientAttackEvidence:
    """types.LightClientAttackEvidence (types/evidence.go:190-198).  ``conflicting_header`` is a header
    dict as ``tmed.merkle.header_hashes`` takes it.  ``byzantine_validators``: None (a nil slice), a list of
    ``tmed.types.Validator`` (address and voting_power are read; the address may be of any length), or
    (addresses u8[n,20], powers i64[n]) arrays."""
    conflicting_header: dict
    conflicting_commit: object      # tmed.types.Commit or PackedCommit
    conflicting_vals: T.ValidatorSet
    common_height: int
    byzantine_validators: object = None
    total_voting_power: int = 0
    timestamp: tuple = T.ZERO_TIME


@dataclass
class LcaRequest:
    """The arguments of one VerifyLightClientAttack call: the evidence, commonHeader.Height, the trusted
    SignedHeader (header dict and commit) and commonVals."""
    evidence: LightClientAttackEvidence
    common_header_height: int
    trusted_header: dict
    trusted_commit: object
    common_vals: T.ValidatorSet


class _LcaRequestC(ctypes.Structure):
    _fields_ = [("conflicting_header", ctypes.c_void_p), ("conflicting_commit", ctypes.POINTER(T._CommitC)),
                ("conflicting_vals", ctypes.POINTER(T._ValsetC)), ("common_height", ctypes.c_int64),
                ("total_voting_power", ctypes.c_int64), ("n_byz", ctypes.c_size_t), ("byz_is_nil", ctypes.c_uint8),
                ("byz_addresses", ctypes.c_void_p), ("byz_address_lens", ctypes.c_void_p), ("byz_powers", ctypes.c_void_p),
                ("common_header_height", ctypes.c_int64), ("trusted_header", ctypes.c_void_p),
                ("trusted_commit", ctypes.POINTER(T._CommitC)), ("common_vals", ctypes.POINTER(T._ValsetC))]


class _ByzResultC(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("state", ctypes.c_int), ("count", ctypes.c_uint32)]


class _LcaResultC(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int), ("kind", ctypes.c_int), ("commit", T._ResultC), ("expected", ctypes.c_int64),
                ("actual", ctypes.c_int64), ("idx", ctypes.c_int32), ("val_idx", ctypes.c_int32),
                ("n_byz_expected", ctypes.c_uint32), ("verified_trusting", ctypes.c_uint32),
                ("verified_light", ctypes.c_uint32), ("hash", ctypes.c_uint8 * 32)]


def _bind_lca():
    l = T._bind()
    if l.tmed_byzantine_validators.argtypes is None:
        P, RQ = ctypes.c_void_p, ctypes.POINTER(_LcaRequestC)
        l.tmed_byzantine_validators.restype = ctypes.c_int
        l.tmed_byzantine_validators.argtypes = [P, RQ, ctypes.c_size_t, P, P, ctypes.POINTER(_ByzResultC)]
        l.tmed_byzantine_validators_host.restype = ctypes.c_int
        l.tmed_byzantine_validators_host.argtypes = [RQ, ctypes.c_size_t, P, P, ctypes.POINTER(_ByzResultC)]
        l.tmed_lca_kernel_times.restype = ctypes.c_int
        l.tmed_lca_kernel_times.argtypes = [P, ctypes.POINTER(ctypes.c_float * 2)]
        l.tmed_verify_light_client_attacks.restype = ctypes.c_int
        l.tmed_verify_light_client_attacks.argtypes = [P, RQ, ctypes.c_size_t, ctypes.c_uint32, P, P,
                                                       ctypes.POINTER(_LcaResultC)]
        l.tmed_verify_light_client_attacks_with.restype = ctypes.c_int
        l.tmed_verify_light_client_attacks_with.argtypes = [RQ, ctypes.c_size_t, ctypes.c_uint32, P, P,
                                                            ctypes.POINTER(_LcaResultC), P, P, P, P, T.VERIFY_FN, P]
    return l


class PreparedLca:
    """Requests packed into C structs once (repeated timing of the C call alone).  One tmed_valset per
    ValidatorSet object, one tmed_commit per Commit object; request q's two headers are 2q and 2q + 1 of
    one HeaderBatch."""

    def __init__(self, requests: Sequence[LcaRequest]):
        from .merkle import HeaderBatch, _HeaderC
        self.requests = list(requests)
        n = self.n = len(self.requests)
        self.keep = []
        hs = []
        for r in self.requests:
            hs += [r.evidence.conflicting_header, r.trusted_header]
        self.headers = HeaderBatch(hs)
        self.reqs = (_LcaRequestC * max(n, 1))()
        self.res = (_LcaResultC * max(n, 1))()
        self.bres = (_ByzResultC * max(n, 1))()
        vcs, ccs = {}, {}

        def valset(vs):
            c = vcs.get(id(vs))
            if c is None:
                c = vcs[id(vs)] = T._valset_c(vs, self.keep)
                self.keep.append(vs)
            return ctypes.pointer(c)

        def commit(cm):
            c = ccs.get(id(cm))
            if c is None:
                c = ccs[id(cm)] = T._commit_c(cm, self.keep)
                self.keep.append(cm)
            return ctypes.pointer(c)

        self.byz_off = np.zeros(n + 1, np.uint64)
        hsz = ctypes.sizeof(_HeaderC)
        hbase = ctypes.addressof(self.headers.hs)
        for q, rq in enumerate(self.requests):
            e = rq.evidence
            r = self.reqs[q]
            r.conflicting_header = hbase + 2 * q * hsz
            r.trusted_header = hbase + (2 * q + 1) * hsz
            r.conflicting_commit = commit(e.conflicting_commit)
            r.trusted_commit = commit(rq.trusted_commit)
            r.conflicting_vals = valset(e.conflicting_vals)
            r.common_vals = valset(rq.common_vals)
            r.common_height, r.total_voting_power = e.common_height, e.total_voting_power
            r.common_header_height = rq.common_header_height
            bv = e.byzantine_validators
            r.byz_is_nil = 1 if bv is None else 0
            if bv is not None:
                if isinstance(bv, tuple):
                    addrs = np.ascontiguousarray(bv[0], np.uint8).reshape(-1, 20)
                    pows = np.ascontiguousarray(bv[1], np.int64)
                    lens = None
                else:
                    m = max(len(bv), 1)
                    addrs, pows, lens = np.zeros((m, 20), np.uint8), np.zeros(m, np.int64), np.zeros(m, np.uint32)
                    for k, v in enumerate(bv):
                        lens[k] = len(v.address)
                        if len(v.address) == 20:
                            addrs[k] = np.frombuffer(v.address, np.uint8)
                        pows[k] = v.voting_power
                    pows = pows[:len(bv)] if len(bv) else pows
                r.n_byz = len(bv) if not isinstance(bv, tuple) else pows.shape[0]
                self.keep.extend([addrs, pows, lens])
                r.byz_addresses, r.byz_powers = T._ptr(addrs), T._ptr(pows)
                if lens is not None:
                    r.byz_address_lens = T._ptr(lens)
            self.byz_off[q + 1] = self.byz_off[q] + r.conflicting_commit.contents.n_sigs
        self.byz = np.full(max(int(self.byz_off[n]), 1), -2, np.int32)

    def _lists(self, counts):
        return [self.byz[int(self.byz_off[q]):int(self.byz_off[q]) + int(counts[q])].tolist() for q in range(self.n)]

    def byzantine(self, engine):
        """tmed_byzantine_validators on ``engine`` (None: tmed_byzantine_validators_host): [(kind, state, list)]."""
        l = _bind_lca()
        if engine is None:
            rc = l.tmed_byzantine_validators_host(self.reqs, self.n, T._ptr(self.byz), T._ptr(self.byz_off), self.bres)
        else:
            rc = l.tmed_byzantine_validators(engine._h, self.reqs, self.n, T._ptr(self.byz), T._ptr(self.byz_off), self.bres)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_byzantine_validators")
        lists = self._lists([self.bres[q].count for q in range(self.n)])
        return [(self.bres[q].kind, self.bres[q].state, lists[q]) for q in range(self.n)]

    def run(self, engine, flags: int = 0):
        rc = _bind_lca().tmed_verify_light_client_attacks(engine._h, self.reqs, self.n, flags, T._ptr(self.byz),
                                                          T._ptr(self.byz_off), self.res)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_verify_light_client_attacks")
        return self.res

    def run_with(self, verifier, conflicting_hashes, conflicting_ok, trusted_hashes, trusted_ok, flags: int = 0):
        """tmed_verify_light_client_attacks_with: ``verifier`` as for tmed.types.verify_commits; the header
        hashes as arrays (n x 32 u8 with n ok bytes, twice)."""
        arrs = [np.ascontiguousarray(a, np.uint8) for a in (conflicting_hashes, conflicting_ok, trusted_hashes, trusted_ok)]

        def cb(user, pubs, sigs, lens, msgs, offs, m, out):
            try:
                P = ctypes.POINTER(ctypes.c_uint8)
                pa = np.ctypeslib.as_array(ctypes.cast(pubs, P), (m * 32,)).reshape(m, 32)
                sa = np.ctypeslib.as_array(ctypes.cast(sigs, P), (m * 64,)).reshape(m, 64)
                la = np.ctypeslib.as_array(ctypes.cast(lens, ctypes.POINTER(ctypes.c_uint32)), (m,))
                oa = np.ctypeslib.as_array(ctypes.cast(offs, ctypes.POINTER(ctypes.c_uint32)), (m + 1,))
                ma = np.ctypeslib.as_array(ctypes.cast(msgs, P), (int(oa[-1]) + 1,))
                np.ctypeslib.as_array(ctypes.cast(out, P), (m,))[:] = verifier(pa.copy(), sa.copy(), la.copy(),
                                                                               ma.copy(), oa.copy())
                return 0
            except Exception:  # never raise across the ABI
                return -3

        rc = _bind_lca().tmed_verify_light_client_attacks_with(
            self.reqs, self.n, flags, T._ptr(self.byz), T._ptr(self.byz_off), self.res, *[T._ptr(a) for a in arrs],
            T.VERIFY_FN(cb), None)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_verify_light_client_attacks_with")
        return self.res

    def codes(self):
        return np.array([self.res[q].code for q in range(self.n)], np.int32)

    def lists(self):
        """The computed list of every request (valid where the request reached validateABCIEvidence)."""
        return self._lists([self.res[q].n_byz_expected for q in range(self.n)])

    def hashes(self):
        return [bytes(self.res[q].hash) for q in range(self.n)]

    def errors(self):
        return [_lca_to_error(self.res[q], r) for q, r in enumerate(self.requests)]


class ErrLcaTrusting(T.GoError):
    def __init__(self, reason):
        self.reason = reason
        super().__init__("skipping verification of conflicting block failed: %s" % reason)


class ErrLcaNotDerived(T.GoError):
    def __init__(self):
        super().__init__("common height is the same as conflicting block height so expected the conflicting"
                         " block to be correctly derived yet it wasn't")


class ErrLcaCommit(T.GoError):
    def __init__(self, reason):
        self.reason = reason
        super().__init__("invalid commit from conflicting block: %s" % reason)


class ErrLcaTotalPower(T.GoError):
    def __init__(self, ev_total, vals_total):
        super().__init__("total voting power from the evidence and our validator set does not match (%d != %d)"
                         % (ev_total, vals_total))


class ErrLcaTimeNotViolated(T.GoError):
    def __init__(self, conflicting_time, trusted_time):
        from .light import go_time
        super().__init__("conflicting block doesn't violate monotonically increasing time (%s is after %s)"
                         % (go_time(conflicting_time), go_time(trusted_time)))


class ErrLcaSameHash(T.GoError):
    def __init__(self):
        super().__init__("trusted header hash matches the evidence's conflicting header hash")


class ErrLcaAmnesiaHasValidators(T.GoError):
    def __init__(self, got):
        super().__init__("expected nil validators from an amnesia light client attack but got %d" % got)


class ErrLcaByzCount(T.GoError):
    def __init__(self, exp, got):
        super().__init__("expected %d byzantine validators from evidence but got %d" % (exp, got))


class ErrLcaByzAddress(T.GoError):
    def __init__(self, exp, got):
        super().__init__("evidence contained an unexpected byzantine validator address; expected: %s, got: %s"
                         % (bytes(exp).hex().upper(), bytes(got).hex().upper()))


class ErrLcaByzPower(T.GoError):
    def __init__(self, exp, got):
        super().__init__("evidence contained unexpected byzantine validator power; expected %d, got %d" % (exp, got))


def _claimed(bv, idx):
    """(address, power) of entry idx of a claimed list."""
    if isinstance(bv, tuple):
        return bytes(np.asarray(bv[0], np.uint8).reshape(-1, 20)[idx]), int(bv[1][idx])
    return bytes(bv[idx].address), bv[idx].voting_power


def _lca_to_error(r, rq: LcaRequest):
    """VerifyLightClientAttack's error value for one result (None: verified); EvidencePanic and
    EvidenceGoPath objects are returned, not raised: the caller runs the Go function for that request."""
    code, e = r.code, rq.evidence
    if code == LCA_OK:
        return None
    if code == LCA_TRUSTING:
        return ErrLcaTrusting(T._to_error(r.commit.code, r.commit, rq.common_vals, None, e.conflicting_commit))
    if code == LCA_NOT_DERIVED:
        return ErrLcaNotDerived()
    if code == LCA_COMMIT:
        return ErrLcaCommit(T._to_error(r.commit.code, r.commit, e.conflicting_vals, e.conflicting_commit.block_id,
                                        e.conflicting_commit))
    if code == LCA_TOTAL_POWER:
        return ErrLcaTotalPower(r.expected, r.actual)
    if code == LCA_TIME_NOT_VIOLATED:
        return ErrLcaTimeNotViolated(e.conflicting_header["time"], rq.trusted_header["time"])
    if code == LCA_SAME_HASH:
        return ErrLcaSameHash()
    if code == LCA_AMNESIA_HAS_VALIDATORS:
        return ErrLcaAmnesiaHasValidators(r.actual)
    if code == LCA_BYZ_COUNT:
        return ErrLcaByzCount(r.expected, r.actual)
    if code in (LCA_BYZ_ADDRESS, LCA_BYZ_POWER):
        vals = rq.common_vals if r.kind == LCA_LUNATIC else e.conflicting_vals
        v = vals.validators[r.val_idx]
        addr, power = _claimed(e.byzantine_validators, r.idx)
        return ErrLcaByzAddress(v.address, addr) if code == LCA_BYZ_ADDRESS else ErrLcaByzPower(v.voting_power, power)
    if code == LCA_PANIC:
        return EvidencePanic("VerifyLightClientAttack panics")
    if code == LCA_GO_PATH:
        return EvidenceGoPath("a header time outside the Timestamp range")
    raise RuntimeError("tmed: unknown light-client-attack outcome %d" % code)


def byzantine_validators(engine, requests: Sequence[LcaRequest]):
    """GetByzantineValidators for every request with one call (engine=None: on the host, one thread):
    [(kind, state, indices)], the indices into common_vals (LCA_LUNATIC) or conflicting_vals
    (LCA_EQUIVOCATION) in the reference's order; -1 is a nil entry; state BYZ_PANIC: the reference panics."""
    return PreparedLca(requests).byzantine(engine)


def verify_light_client_attacks(engine, requests: Sequence[LcaRequest], verifier=None, hashes=None,
                                stats: Optional[list] = None):
    """VerifyLightClientAttack for every request with one call: one Go-style error (or None) per request,
    as ``to_error`` builds it.  verifier / hashes = (conflicting_hashes, conflicting_ok, trusted_hashes,
    trusted_ok): tmed_verify_light_client_attacks_with (the CPU test-suite).  stats, if a list, receives
    (code, kind, computed list, Hash()) per request."""
    pl = PreparedLca(requests)
    if verifier is None:
        pl.run(engine)
    else:
        pl.run_with(verifier, *hashes)
    if stats is not None:
        ls, hs = pl.lists(), pl.hashes()
        stats.extend((int(pl.res[q].code), int(pl.res[q].kind), ls[q], hs[q]) for q in range(pl.n))
    return pl.errors()


def last_lca_kernel_times(engine):
    """(lca_lookup_kernel ms, lca_rank_kernel ms) of the engine's last byzantine_validators /
    verify_light_client_attacks."""
    ms = (ctypes.c_float * 2)()
    rc = _bind_lca().tmed_lca_kernel_times(engine._h, ctypes.byref(ms))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_lca_kernel_times")
    return float(ms[0]), float(ms[1])
