"""Host mirror of ``state.MedianTime`` (reference ``state/state.go:268-285`` over
``tmtime.WeightedMedian``, ``types/time/time.go:35-58``) over the C ABI ``tmed_median_times``
(kernels in ``csrc/median.hip``, the same rule on the host in ``csrc/median_host.h``): the block
time ``validateBlock`` compares ``block.Time`` with (``state/validation.go:123-129``) and
``State.MakeBlock`` stamps on a proposal, for many (commit, validator set) pairs per call.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import types as T
from ._native import TMED_OK, TmedError
from .merkle import HeaderBatch, _HeaderC

MEDIAN_OK, MEDIAN_ZERO_TIME, MEDIAN_GO_PATH = 0, 1, 2


class _MedianRequestC(ctypes.Structure):
    _fields_ = [("commit", ctypes.POINTER(T._CommitC)), ("vals", ctypes.POINTER(T._ValsetC))]


class _MedianResultC(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int), ("seconds", ctypes.c_int64), ("nanos", ctypes.c_int32),
                ("entered", ctypes.c_uint32), ("on_device", ctypes.c_uint8)]


def _bind():
    l = T._bind()
    if l.tmed_median_times.argtypes is None:
        l.tmed_median_times.restype = ctypes.c_int
        l.tmed_median_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(_MedianRequestC), ctypes.c_size_t,
                                        ctypes.POINTER(_MedianResultC)]
        l.tmed_median_times_host.restype = ctypes.c_int
        l.tmed_median_times_host.argtypes = [ctypes.POINTER(_MedianRequestC), ctypes.c_size_t,
                                             ctypes.POINTER(_MedianResultC)]
    return l


def _valset_c(vals, keep):
    """The fields of tmed_valset the call reads: n, addresses, powers (total_power stays 0: MedianTime
    sums the entering powers itself, and a set whose total panics in Go must still reach GO_PATH)."""
    pubs, powers, addrs = vals.packed()
    keep.extend([pubs, powers, addrs, vals])
    return T._ValsetC(len(vals.validators), T._ptr(pubs), T._ptr(powers), T._ptr(addrs), 0, 0, None, None)


class PreparedMedian:
    """(commit, validator set) pairs packed into C structs once (repeated timing of the C call alone;
    ``median_times`` packs per call).  One tmed_valset per ValidatorSet object and one tmed_commit per
    commit object: the library stages each distinct pointer once."""

    def __init__(self, pairs: Sequence[tuple]):
        self.pairs = list(pairs)
        n = self.n = len(self.pairs)
        self.keep = []
        self.reqs = (_MedianRequestC * max(n, 1))()
        self.res = (_MedianResultC * max(n, 1))()
        vcs, ccs = {}, {}
        for q, (commit, vals) in enumerate(self.pairs):
            cc = ccs.get(id(commit))
            if cc is None:
                cc = ccs[id(commit)] = T._commit_c(commit, self.keep)
            vc = vcs.get(id(vals))
            if vc is None:
                vc = vcs[id(vals)] = _valset_c(vals, self.keep)
            self.keep.extend([cc, vc])
            self.reqs[q] = _MedianRequestC(ctypes.pointer(cc), ctypes.pointer(vc))

    def run(self, engine):
        """tmed_median_times on ``engine``; ``engine=None``: tmed_median_times_host."""
        l = _bind()
        if engine is None:
            rc = l.tmed_median_times_host(self.reqs, self.n, self.res)
        else:
            rc = l.tmed_median_times(engine._h, self.reqs, self.n, self.res)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_median_times")
        return self.res

    def results(self):
        return [(int(r.code), (int(r.seconds), int(r.nanos))) for r in self.res[:self.n]]

    def on_device(self):
        return np.array([r.on_device for r in self.res[:self.n]], np.uint8)

    def entered(self):
        return np.array([r.entered for r in self.res[:self.n]], np.int64)


def median_times(engine, pairs: Sequence[tuple]):
    """MedianTime(commit, vals) for every (commit, vals) of ``pairs`` in one call.

    commit: a ``tmed.types.Commit`` or ``PackedCommit``; vals: a ``tmed.types.ValidatorSet``.
    engine: an Engine (the device path), or None for the host function.
    Returns ``(code, (seconds, nanos))`` per pair: ``MEDIAN_OK`` with the median as (Unix seconds,
    nanoseconds); ``MEDIAN_ZERO_TIME`` with Go's zero ``time.Time`` (``tmed.types.ZERO_TIME``) when
    no signature entered; ``MEDIAN_GO_PATH`` when the caller must run the reference's function (the
    time is then meaningless).
    """
    pm = PreparedMedian(pairs)
    pm.run(engine)
    return pm.results()


# --------------------------------------------------------------------------- validateBlock
#
# ``validateBlock`` (reference ``state/validation.go:15-151``) with the ``Block.ValidateBasic`` it runs
# first (``types/block.go:55-106``) over the C ABI ``tmed_validate_blocks`` (replay in
# ``csrc/validate_host.h``, device work in ``csrc/validate.hip`` and the kernels of the hash, commit and
# median calls): many blocks per call, one Go-style error (or ``None``) per block.

(VB_OK, VB_HEADER_BASIC, VB_COMMIT_BASIC, VB_LAST_COMMIT_HASH, VB_DATA_HASH, VB_EVIDENCE_BASIC, VB_EVIDENCE_HASH,
 VB_VERSION, VB_CHAIN_ID, VB_HEIGHT_INITIAL, VB_HEIGHT, VB_LAST_BLOCK_ID, VB_APP_HASH, VB_CONSENSUS_HASH,
 VB_LAST_RESULTS_HASH, VB_VALIDATORS_HASH, VB_NEXT_VALIDATORS_HASH, VB_INITIAL_HAS_SIGS, VB_LAST_COMMIT,
 VB_PROPOSER_SIZE, VB_PROPOSER_UNKNOWN, VB_TIME_NOT_AFTER, VB_TIME_NOT_MEDIAN, VB_TIME_NOT_GENESIS,
 VB_HEIGHT_BELOW_INITIAL, VB_EVIDENCE_OVERFLOW, VB_GO_PATH) = range(27)
VB_CODE_NAMES = ["OK", "HEADER_BASIC", "COMMIT_BASIC", "LAST_COMMIT_HASH", "DATA_HASH", "EVIDENCE_BASIC", "EVIDENCE_HASH",
                 "VERSION", "CHAIN_ID", "HEIGHT_INITIAL", "HEIGHT", "LAST_BLOCK_ID", "APP_HASH", "CONSENSUS_HASH",
                 "LAST_RESULTS_HASH", "VALIDATORS_HASH", "NEXT_VALIDATORS_HASH", "INITIAL_HAS_SIGS", "LAST_COMMIT",
                 "PROPOSER_SIZE", "PROPOSER_UNKNOWN", "TIME_NOT_AFTER", "TIME_NOT_MEDIAN", "TIME_NOT_GENESIS",
                 "HEIGHT_BELOW_INITIAL", "EVIDENCE_OVERFLOW", "GO_PATH"]
KNOW_APP_HASH, KNOW_CONSENSUS_HASH, KNOW_LAST_RESULTS_HASH, KNOW_VALIDATORS, KNOW_NEXT_VALIDATORS = 1, 2, 4, 8, 16
KNOW_ALL = 31
VB_LINK_PREV = 1


@dataclass
class BlockState:
    """The fields of ``State`` that validateBlock reads.  ``known``: a mask of KNOW_*; a check whose bit
    is clear is skipped and reported in the result's ``skipped`` (its set may then be None)."""
    version_block: int
    version_app: int
    chain_id: str
    initial_height: int
    last_block_height: int
    last_block_id: T.BlockID
    last_block_time: tuple
    app_hash: bytes
    consensus_hash: bytes          # HashConsensusParams(state.ConsensusParams)
    last_results_hash: bytes
    validators: Optional[T.ValidatorSet]
    next_validators: Optional[T.ValidatorSet]
    last_validators: Optional[T.ValidatorSet]
    evidence_max_bytes: int
    known: int = KNOW_ALL


@dataclass
class Block:
    """A block as validateBlock reads it.  ``header``: a header dict (the fields of ``oracle/merkle.py``'s
    ``header_leaves``); ``evidence``: DuplicateVoteEvidence objects, or ``bytes`` for an evidence of
    another kind already marshalled; the three ``basic`` fields are what the caller's Go ValidateBasic
    methods returned."""
    header: dict
    last_commit: object            # tmed.types.Commit or PackedCommit; None: a nil LastCommit
    txs: Sequence[bytes] = ()
    evidence: Sequence = ()
    evidence_byte_size: int = 0    # block.Evidence.ByteSize()
    header_basic_ok: bool = True
    commit_basic_ok: bool = True
    evidence_basic_bad: int = -1


class _BlockStateC(ctypes.Structure):
    _fields_ = [("version_block", ctypes.c_uint64), ("version_app", ctypes.c_uint64), ("chain_id", ctypes.c_char_p),
                ("chain_id_len", ctypes.c_uint32), ("initial_height", ctypes.c_int64),
                ("last_block_height", ctypes.c_int64), ("last_block_id", T._BlockIDC),
                ("last_block_time_seconds", ctypes.c_int64), ("last_block_time_nanos", ctypes.c_int32),
                ("app_hash", ctypes.c_void_p), ("app_hash_len", ctypes.c_uint32), ("consensus_hash", ctypes.c_void_p),
                ("last_results_hash", ctypes.c_void_p), ("last_results_hash_len", ctypes.c_uint32),
                ("validators", ctypes.POINTER(T._ValsetC)), ("next_validators", ctypes.POINTER(T._ValsetC)),
                ("last_validators", ctypes.POINTER(T._ValsetC)), ("evidence_max_bytes", ctypes.c_int64),
                ("known", ctypes.c_uint32)]


class _BlockRequestC(ctypes.Structure):
    _fields_ = [("header", ctypes.POINTER(_HeaderC)), ("last_commit", ctypes.POINTER(T._CommitC)),
                ("state", ctypes.POINTER(_BlockStateC)), ("evidence_byte_size", ctypes.c_int64),
                ("header_basic_ok", ctypes.c_uint8), ("commit_basic_ok", ctypes.c_uint8),
                ("evidence_basic_bad", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class _BlockBatchC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("blocks", ctypes.POINTER(_BlockRequestC)), ("txs", ctypes.c_void_p),
                ("tx_off", ctypes.c_void_p), ("block_off", ctypes.c_void_p), ("ev", ctypes.c_void_p),
                ("items", ctypes.c_void_p), ("list_off", ctypes.c_void_p), ("opaque", ctypes.c_void_p),
                ("opaque_off", ctypes.c_void_p)]


class _BlockResultC(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int), ("skipped", ctypes.c_uint32), ("hash_len", ctypes.c_uint32),
                ("hash", ctypes.c_uint8 * 32), ("commit", T._ResultC), ("median_seconds", ctypes.c_int64),
                ("median_nanos", ctypes.c_int32), ("idx", ctypes.c_int32), ("proposer_idx", ctypes.c_int32),
                ("verified", ctypes.c_uint32)]


def _bind_vb():
    l = _bind()
    if l.tmed_validate_blocks.argtypes is None:
        P = ctypes.c_void_p
        l.tmed_validate_blocks.restype = ctypes.c_int
        l.tmed_validate_blocks.argtypes = [P, ctypes.POINTER(_BlockBatchC), ctypes.POINTER(_BlockResultC)]
        l.tmed_validate_blocks_with.restype = ctypes.c_int
        l.tmed_validate_blocks_with.argtypes = [ctypes.POINTER(_BlockBatchC), ctypes.POINTER(_BlockResultC), P, P, P, P, P,
                                                P, P, P, P, ctypes.POINTER(_MedianResultC), P, T.VERIFY_FN, P]
        l.tmed_validate_kernel_ms.restype = ctypes.c_float
        l.tmed_validate_kernel_ms.argtypes = [P]
        l.tmed_validate_stats.restype = ctypes.c_int
        l.tmed_validate_stats.argtypes = [P, ctypes.POINTER(ctypes.c_uint64 * 3)]
    return l


class ErrBlockBasic(T.GoError):
    """Block.ValidateBasic failed in a check the caller ran in Go (the Go method has the text)."""


class ErrEvidenceOverflow(T.GoError):  # types/evidence.go:536-550
    def __init__(self, max_bytes, got):
        self.max, self.got = max_bytes, got
        super().__init__("Too much evidence: Max %d, got %d" % (max_bytes, got))


class BlockGoPath:
    """TMED_VB_GO_PATH: the structs cannot decide this block; the caller runs the Go function."""

    def __repr__(self):
        return "BlockGoPath()"

    def __eq__(self, o):
        return isinstance(o, BlockGoPath)


class PreparedBlocks:
    """Requests ``(Block, BlockState, link_prev)`` packed into C structs once (repeated timing of the C
    call alone; ``validate_blocks`` packs per call).  One tmed_valset per ValidatorSet object, one
    tmed_block_state per BlockState object, one tmed_commit per commit object."""

    def __init__(self, requests: Sequence[tuple]):
        from .evidence import PackedEvidence
        self.requests = [tuple(r) if len(r) == 3 else (r[0], r[1], False) for r in requests]
        n = self.n = len(self.requests)
        self.keep = []
        self.headers = HeaderBatch([blk.header for blk, _, _ in self.requests])
        self.reqs = (_BlockRequestC * max(n, 1))()
        self.res = (_BlockResultC * max(n, 1))()
        vcs, ccs, scs = {}, {}, {}

        def valset(vs):
            if vs is None:
                return None
            c = vcs.get(id(vs))
            if c is None:
                c = vcs[id(vs)] = T._valset_c(vs, self.keep)
                self.keep.append(vs)
            return ctypes.pointer(c)

        def cbytes(b):
            b = bytes(b)
            self.keep.append(b)
            return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p), len(b)

        def state(st):
            c = scs.get(id(st))
            if c is None:
                c = scs[id(st)] = _BlockStateC()
                self.keep.append(st)
                cid = st.chain_id.encode()
                self.keep.append(cid)
                c.version_block, c.version_app = st.version_block, st.version_app
                c.chain_id, c.chain_id_len = cid, len(cid)
                c.initial_height, c.last_block_height = st.initial_height, st.last_block_height
                c.last_block_id = T._block_id_c(st.last_block_id, self.keep)
                c.last_block_time_seconds, c.last_block_time_nanos = st.last_block_time
                c.app_hash, c.app_hash_len = cbytes(st.app_hash)
                if len(st.consensus_hash) != 32:
                    raise ValueError("consensus_hash must be HashConsensusParams (32 bytes)")
                c.consensus_hash, _ = cbytes(st.consensus_hash)
                c.last_results_hash, c.last_results_hash_len = cbytes(st.last_results_hash)
                for name in ("validators", "next_validators", "last_validators"):
                    p = valset(getattr(st, name))
                    if p is not None:
                        setattr(c, name, p)
                c.evidence_max_bytes, c.known = st.evidence_max_bytes, st.known
            return ctypes.pointer(c)

        flat, block_off, dup, items, list_off, blobs = [], [0], [], [], [0], []
        for q, (blk, st, link) in enumerate(self.requests):
            r = self.reqs[q]
            r.header = ctypes.pointer(self.headers.hs[q])
            if blk.last_commit is not None:
                cc = ccs.get(id(blk.last_commit))
                if cc is None:
                    cc = ccs[id(blk.last_commit)] = T._commit_c(blk.last_commit, self.keep)
                    self.keep.append(cc)
                r.last_commit = ctypes.pointer(cc)
            r.state = state(st)
            r.evidence_byte_size = blk.evidence_byte_size
            r.header_basic_ok, r.commit_basic_ok = int(blk.header_basic_ok), int(blk.commit_basic_ok)
            r.evidence_basic_bad, r.flags = blk.evidence_basic_bad, VB_LINK_PREV if link else 0
            flat.extend(bytes(t) for t in blk.txs)
            block_off.append(len(flat))
            for e in blk.evidence:
                if isinstance(e, (bytes, bytearray)):
                    items.append(-1 - len(blobs))
                    blobs.append(bytes(e))
                else:
                    items.append(len(dup))
                    dup.append(e)
            list_off.append(len(items))
        self.tx_off = np.zeros(len(flat) + 1, np.uint64)
        np.cumsum(np.asarray([len(t) for t in flat], np.uint64), out=self.tx_off[1:])
        self.txs = np.frombuffer(b"".join(flat) + b"\0" * 8, np.uint8)
        self.block_off = np.asarray(block_off, np.uint32)
        self.pe = PackedEvidence(dup)
        self.items = np.asarray(items + [0], np.int64)
        self.list_off = np.asarray(list_off, np.uint32)
        self.op_off = np.zeros(len(blobs) + 1, np.uint64)
        np.cumsum(np.asarray([len(b) for b in blobs], np.uint64), out=self.op_off[1:])
        self.opaque = np.frombuffer(b"".join(blobs) + b"\0" * 8, np.uint8)
        self.batch = _BlockBatchC(n, self.reqs, T._ptr(self.txs), T._ptr(self.tx_off), T._ptr(self.block_off),
                                  ctypes.cast(ctypes.pointer(self.pe.c), ctypes.c_void_p), T._ptr(self.items),
                                  T._ptr(self.list_off), T._ptr(self.opaque), T._ptr(self.op_off))

    def run(self, engine):
        rc = _bind_vb().tmed_validate_blocks(engine._h, ctypes.byref(self.batch), self.res)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_validate_blocks")
        return self.res

    def run_with(self, verifier, commit_hashes, commit_ok, data_hashes, evidence_hashes, evidence_ok, header_hashes,
                 header_ok, validators_hashes, next_validators_hashes, medians, proposer_idx):
        """tmed_validate_blocks_with: ``verifier`` as for tmed.types.verify_commits; the hashes as arrays
        (n x 32 u8, ok arrays n u8); medians: ``(code, (seconds, nanos))`` per block; proposer_idx: i32[n]."""
        n = max(self.n, 1)
        arrs = [np.ascontiguousarray(a, np.uint8) for a in (commit_hashes, commit_ok, data_hashes, evidence_hashes,
                                                           evidence_ok, header_hashes, header_ok, validators_hashes,
                                                           next_validators_hashes)]
        med = (_MedianResultC * n)()
        for q, (code, (sec, nanos)) in enumerate(medians):
            med[q] = _MedianResultC(code, sec, nanos, 0, 0)
        prop = np.ascontiguousarray(proposer_idx, np.int32)

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

        rc = _bind_vb().tmed_validate_blocks_with(ctypes.byref(self.batch), self.res, *[T._ptr(a) for a in arrs], med,
                                                  T._ptr(prop), T.VERIFY_FN(cb), None)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_validate_blocks_with")
        return self.res

    def codes(self):
        return np.array([self.res[q].code for q in range(self.n)], np.int32)

    def errors(self):
        return [block_error(self.res[q], self.requests, q) for q in range(self.n)]


def _hexu(b) -> str:
    return bytes(b).hex().upper()


def block_error(r, requests, q):
    """The reference's error value for result ``r`` of request q (None: the block is valid)."""
    from .light import go_time
    blk, st, link = requests[q]
    h, code = blk.header, r.code
    got = _hexu(bytes(r.hash)[:r.hash_len])
    if code == VB_OK:
        return None
    if code == VB_GO_PATH:
        return BlockGoPath()
    if code == VB_HEADER_BASIC:  # the Go methods have the texts of the three basic checks
        return ErrBlockBasic("invalid header: Header.ValidateBasic failed")
    if code == VB_COMMIT_BASIC:
        return ErrBlockBasic("nil LastCommit" if blk.last_commit is None else "wrong LastCommit: Commit.ValidateBasic failed")
    if code == VB_EVIDENCE_BASIC:
        return ErrBlockBasic("invalid evidence (#%d): Evidence.ValidateBasic failed" % r.idx)
    if code == VB_LAST_COMMIT_HASH:
        return T.GoError("wrong Header.LastCommitHash. Expected %s, got %s" % (got, _hexu(h["last_commit_hash"])))
    if code == VB_DATA_HASH:
        return T.GoError("wrong Header.DataHash. Expected %s, got %s" % (got, _hexu(h["data_hash"])))
    if code == VB_EVIDENCE_HASH:
        return T.GoError("wrong Header.EvidenceHash. Expected %s, got %s" % (_hexu(h["evidence_hash"]), got))
    if code == VB_VERSION:
        return T.GoError("wrong Block.Header.Version. Expected {%d %d}, got {%d %d}"
                         % (st.version_block, st.version_app, h["version_block"], h["version_app"]))
    if code == VB_CHAIN_ID:
        return T.GoError("wrong Block.Header.ChainID. Expected %s, got %s" % (st.chain_id, h["chain_id"]))
    if code == VB_HEIGHT_INITIAL:  # the reference prints the two in this order
        return T.GoError("wrong Block.Header.Height. Expected %d for initial block, got %d"
                         % (h["height"], st.initial_height))
    last_height = requests[q - 1][0].header["height"] if link else st.last_block_height
    last_time = requests[q - 1][0].header["time"] if link else st.last_block_time
    if code == VB_HEIGHT:
        return T.GoError("wrong Block.Header.Height. Expected %d, got %d" % (last_height + 1, h["height"]))
    if code == VB_LAST_BLOCK_ID:
        want = st.last_block_id
        if link:
            want = T.BlockID(bytes(r.hash)[:r.hash_len], want.psh_total, want.psh_hash)
        return T.GoError("wrong Block.Header.LastBlockID.  Expected %s, got %s" % (want, T.BlockID(*h["last_block_id"])))
    if code == VB_APP_HASH:
        return T.GoError("wrong Block.Header.AppHash.  Expected %s, got %s" % (_hexu(st.app_hash), _hexu(h["app_hash"])))
    if code == VB_CONSENSUS_HASH:
        return T.GoError("wrong Block.Header.ConsensusHash.  Expected %s, got %s"
                         % (_hexu(st.consensus_hash), _hexu(h["consensus_hash"])))
    if code == VB_LAST_RESULTS_HASH:
        return T.GoError("wrong Block.Header.LastResultsHash.  Expected %s, got %s"
                         % (_hexu(st.last_results_hash), _hexu(h["last_results_hash"])))
    if code == VB_VALIDATORS_HASH:
        return T.GoError("wrong Block.Header.ValidatorsHash.  Expected %s, got %s" % (got, _hexu(h["validators_hash"])))
    if code == VB_NEXT_VALIDATORS_HASH:
        return T.GoError("wrong Block.Header.NextValidatorsHash.  Expected %s, got %s"
                         % (got, _hexu(h["next_validators_hash"])))
    if code == VB_INITIAL_HAS_SIGS:
        return T.GoError("initial block can't have LastCommit signatures")
    if code == VB_LAST_COMMIT:
        bid = st.last_block_id
        if link:  # a linked request passed LAST_BLOCK_ID: the header's hash is the previous block's
            bid = T.BlockID(bytes(h["last_block_id"][0]), bid.psh_total, bid.psh_hash)
        return T._to_error(r.commit.code, r.commit, st.last_validators, bid, blk.last_commit)
    if code == VB_PROPOSER_SIZE:
        return T.GoError("expected ProposerAddress size 20, got %d" % len(h["proposer_address"]))
    if code == VB_PROPOSER_UNKNOWN:
        return T.GoError("block.Header.ProposerAddress %s is not a validator" % _hexu(h["proposer_address"]))
    if code == VB_TIME_NOT_AFTER:
        return T.GoError("block time %s not greater than last block time %s" % (go_time(h["time"]), go_time(last_time)))
    if code == VB_TIME_NOT_MEDIAN:
        return T.GoError("invalid block time. Expected %s, got %s"
                         % (go_time((r.median_seconds, r.median_nanos)), go_time(h["time"])))
    if code == VB_TIME_NOT_GENESIS:
        return T.GoError("block time %s is not equal to genesis time %s" % (go_time(h["time"]), go_time(last_time)))
    if code == VB_HEIGHT_BELOW_INITIAL:
        return T.GoError("block height %d lower than initial height %d" % (h["height"], st.initial_height))
    if code == VB_EVIDENCE_OVERFLOW:
        return ErrEvidenceOverflow(st.evidence_max_bytes, blk.evidence_byte_size)
    raise RuntimeError("tmed: unknown block outcome %d" % code)


def validate_blocks(engine, requests: Sequence[tuple], stats: Optional[list] = None):
    """validateBlock for every ``(Block, BlockState)`` or ``(Block, BlockState, link_prev)`` of ``requests``
    in one call (tmed_validate_blocks).  link_prev (requests 1..): the state's last block hash, height and
    time are the previous request's block's, its hash computed on the device in this call.  Returns one
    Go-style error per block: None, a ``GoError`` (``ErrBlockBasic``, ``ErrEvidenceOverflow``, the
    VerifyCommit errors of ``tmed.types``), a ``GoPanic`` where VerifyCommit panics, or ``BlockGoPath()``.
    stats, if a list, receives ``(skipped, verified, proposer_idx)`` per block."""
    pb = PreparedBlocks(requests)
    pb.run(engine)
    if stats is not None:
        stats.extend((int(r.skipped), int(r.verified), int(r.proposer_idx)) for r in pb.res[:pb.n])
    return pb.errors()


def validate_kernel_ms(engine) -> float:
    """block_check_kernel's device time (ms) in the engine's last validate_blocks."""
    return float(_bind_vb().tmed_validate_kernel_ms(engine._h))


def validate_stats(engine):
    """(set hashes computed, sets staged for the proposer lookup, blocks checked) of the engine's last
    validate_blocks (tmed_validate_stats)."""
    out = (ctypes.c_uint64 * 3)()
    rc = _bind_vb().tmed_validate_stats(engine._h, ctypes.byref(out))
    if rc != TMED_OK:
        raise TmedError(rc, "tmed_validate_stats")
    return tuple(int(v) for v in out)
