"""Host mirror of the light client's ``light.Verify`` (reference ``light/verifier.go:135-151``) over
the C ABI ``tmed_light_verify`` (replay in ``csrc/light_host.h``, device work in ``csrc/commit.hip``
and ``csrc/merkle.hip``): many (trusted, untrusted) pairs per call, one Go-style error (or ``None``)
per pair, with the reference's error types: ``ErrOldHeaderExpired``, ``ErrInvalidHeader(reason)``
and ``ErrNewValSetCantBeTrusted(reason)`` are what ``light/client.go:746-767`` type-switches on to
drive the bisection; anything else is a plain ``GoError``.  Errors are built as
``tmed.types.verify_commits`` builds its own.
"""
from __future__ import annotations

import ctypes
import json
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import types as T
from ._native import TMED_OK, TmedError
from .merkle import HeaderBatch, _HeaderC
from .types import GoError

(OK, OLD_HEADER_EXPIRED, HEADER_BASIC, WRONG_CHAIN, COMMIT_HEIGHT, COMMIT_HEADER_HASH, HEIGHT_NOT_GREATER,
 TIME_NOT_AFTER, TIME_FROM_FUTURE, VALS_HASH, NEXT_VALS_HASH, TRUSTING, COMMIT, GO_PATH) = range(14)
LIGHT_ORDERED = 1
SECOND = 1_000_000_000  # time.Duration is int64 nanoseconds


@dataclass
class LightPair:
    """The arguments of one light.Verify call.  ``trusted`` and ``header`` are header dicts with the
    fields of ``oracle/merkle.py``'s ``header_leaves`` (of ``trusted`` only chain_id, height, time and
    next_validators_hash are read); times are (Unix seconds, nanoseconds); durations nanoseconds."""
    trusted: dict
    trusted_vals: Optional[T.ValidatorSet]
    header: dict
    commit: object            # tmed.types.Commit or PackedCommit
    vals: T.ValidatorSet
    trusting_period: int
    now: tuple
    max_clock_drift: int
    trust_level: tuple = (1, 3)
    basic_ok: bool = True     # Header.ValidateBasic() == nil and Commit.ValidateBasic() == nil


# --------------------------------------------------------------------------- errors

class ErrOldHeaderExpired(GoError):  # light/errors.go:14-21
    def __init__(self, at, now):
        self.at, self.now = tuple(at), tuple(now)
        super().__init__("old header has expired at %s (now: %s)" % (go_time(self.at), go_time(self.now)))


class ErrNewValSetCantBeTrusted(GoError):  # light/errors.go:25-31
    def __init__(self, reason):
        self.reason = reason
        super().__init__("cant trust new val set: %s" % reason)


class ErrInvalidHeader(GoError):  # light/errors.go:35-41
    def __init__(self, reason):
        self.reason = reason
        super().__init__("invalid header: %s" % reason)


class GoPath:
    """TMED_LIGHT_GO_PATH: the structs cannot express this request; the caller runs the Go function."""

    def __repr__(self):
        return "GoPath()"

    def __eq__(self, o):
        return isinstance(o, GoPath)


def go_time(t) -> str:
    """Time.String() of a UTC time without a monotonic reading: 2006-01-02 15:04:05.999999999 +0000 UTC."""
    sec, nanos = t
    days, rem = divmod(sec, 86400)
    # civil date of a day count from 1970-01-01 (proleptic Gregorian, any year)
    z = days + 719468
    era, doe = divmod(z, 146097)
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    day, month = doy - (153 * mp + 2) // 5 + 1, mp + 3 if mp < 10 else mp - 9
    year = yoe + era * 400 + (1 if month <= 2 else 0)
    frac = (".%09d" % nanos).rstrip("0") if nanos else ""
    return "%04d-%02d-%02d %02d:%02d:%02d%s +0000 UTC" % (year, month, day, rem // 3600, rem // 60 % 60, rem % 60, frac)


def go_duration(ns: int) -> str:
    """Duration.String() (time/time.go): 72h3m0.5s, 1.5ms, 0s."""
    if ns == 0:
        return "0s"
    neg, u = ns < 0, abs(ns)
    if u < SECOND:
        for unit, name in ((1, "ns"), (1000, "µs"), (1000000, "ms")):
            if u < unit * 1000:
                s = ("%d.%09d" % (u // unit, u % unit * (SECOND // unit))).rstrip("0").rstrip(".") if unit > 1 else str(u)
                return ("-" if neg else "") + s + name
    secs, frac = divmod(u, SECOND)
    s = (("%d.%09d" % (secs % 60, frac)).rstrip("0").rstrip(".") if frac else str(secs % 60)) + "s"
    mins = secs // 60
    if mins:
        s = "%dm" % (mins % 60) + s
        if mins // 60:
            s = "%dh" % (mins // 60) + s
    return ("-" if neg else "") + s


def _goq(s: str) -> str:  # %q of a printable string
    return json.dumps(s, ensure_ascii=False)


def _hexu(b) -> str:
    return bytes(b).hex().upper()


# --------------------------------------------------------------------------- ABI

class _LightRequestC(ctypes.Structure):
    _fields_ = [("chain_id", ctypes.c_char_p), ("chain_id_len", ctypes.c_uint32),
                ("trusted_height", ctypes.c_int64), ("trusted_time_seconds", ctypes.c_int64),
                ("trusted_time_nanos", ctypes.c_int32),
                ("trusted_next_vals_hash", ctypes.c_void_p), ("trusted_next_vals_hash_len", ctypes.c_uint32),
                ("trusted_vals", ctypes.POINTER(T._ValsetC)),
                ("header", ctypes.POINTER(_HeaderC)), ("commit", ctypes.POINTER(T._CommitC)),
                ("vals", ctypes.POINTER(T._ValsetC)), ("basic_ok", ctypes.c_uint8),
                ("trusting_period_ns", ctypes.c_int64), ("max_clock_drift_ns", ctypes.c_int64),
                ("now_seconds", ctypes.c_int64), ("now_nanos", ctypes.c_int32),
                ("trust_num", ctypes.c_int64), ("trust_den", ctypes.c_int64)]


class _LightResultC(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int), ("adjacent", ctypes.c_int), ("expired_seconds", ctypes.c_int64),
                ("expired_nanos", ctypes.c_int32), ("hash_len", ctypes.c_uint32), ("hash", ctypes.c_uint8 * 32),
                ("commit", T._ResultC), ("verified_trusting", ctypes.c_uint32), ("verified_light", ctypes.c_uint32)]


def _bind():
    l = T._bind()
    if l.tmed_light_verify.argtypes is None:
        P = ctypes.c_void_p
        l.tmed_light_verify.restype = ctypes.c_int
        l.tmed_light_verify.argtypes = [P, ctypes.POINTER(_LightRequestC), ctypes.c_size_t, ctypes.c_uint32,
                                        ctypes.POINTER(_LightResultC)]
        l.tmed_light_verify_with.restype = ctypes.c_int
        l.tmed_light_verify_with.argtypes = [ctypes.POINTER(_LightRequestC), ctypes.c_size_t, ctypes.c_uint32, P, P, P,
                                             ctypes.POINTER(_LightResultC), T.VERIFY_FN, P]
    return l


class PreparedLight:
    """Pairs packed into C structs once (repeated timing of the C call alone; ``verify`` packs per call).
    One tmed_valset per ValidatorSet object, one tmed_commit per Commit object."""

    def __init__(self, pairs: Sequence[LightPair]):
        self.pairs = list(pairs)
        n = self.n = len(self.pairs)
        self.keep = []
        self.headers = HeaderBatch([p.header for p in self.pairs])
        self.reqs = (_LightRequestC * max(n, 1))()
        self.res = (_LightResultC * max(n, 1))()
        vcs, ccs = {}, {}

        def valset(vs):
            if vs is None:
                return None
            c = vcs.get(id(vs))
            if c is None:
                c = vcs[id(vs)] = T._valset_c(vs, self.keep)
                self.keep.append(vs)
            return ctypes.pointer(c)

        for q, p in enumerate(self.pairs):
            cc = ccs.get(id(p.commit))
            if cc is None:
                cc = ccs[id(p.commit)] = T._commit_c(p.commit, self.keep)
            cid = p.trusted["chain_id"].encode()
            nvh = bytes(p.trusted["next_validators_hash"])
            self.keep.extend([cid, nvh, cc])
            r = self.reqs[q]
            r.chain_id, r.chain_id_len = cid, len(cid)
            r.trusted_height = p.trusted["height"]
            r.trusted_time_seconds, r.trusted_time_nanos = p.trusted["time"]
            r.trusted_next_vals_hash = ctypes.cast(ctypes.c_char_p(nvh), ctypes.c_void_p)
            r.trusted_next_vals_hash_len = len(nvh)
            tv, uv = valset(p.trusted_vals), valset(p.vals)
            if tv is not None:
                r.trusted_vals = tv
            r.header = ctypes.pointer(self.headers.hs[q])
            r.commit = ctypes.pointer(cc)
            r.vals = uv
            r.basic_ok = 1 if p.basic_ok else 0
            r.trusting_period_ns, r.max_clock_drift_ns = p.trusting_period, p.max_clock_drift
            r.now_seconds, r.now_nanos = p.now
            r.trust_num, r.trust_den = p.trust_level

    def run(self, engine, flags: int = 0):
        rc = _bind().tmed_light_verify(engine._h, self.reqs, self.n, flags, self.res)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_light_verify")
        return self.res

    def run_with(self, verifier, header_hashes, header_ok, vals_hashes, flags: int = 0):
        """tmed_light_verify_with: ``verifier`` as for tmed.types.verify_commits; the hashes as arrays
        (n x 32 u8, n u8, n x 32 u8)."""
        hh = np.ascontiguousarray(header_hashes, np.uint8)
        ho = np.ascontiguousarray(header_ok, np.uint8)
        vh = np.ascontiguousarray(vals_hashes, np.uint8)

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

        rc = _bind().tmed_light_verify_with(self.reqs, self.n, flags, T._ptr(hh), T._ptr(ho), T._ptr(vh), self.res,
                                            T.VERIFY_FN(cb), None)
        if rc != TMED_OK:
            raise TmedError(rc, "tmed_light_verify_with")
        return self.res

    def codes(self):
        return np.array([self.res[q].code for q in range(self.n)], np.int32)

    def errors(self):
        return [to_error(self.res[q], p) for q, p in enumerate(self.pairs)]


def to_error(r: _LightResultC, p: LightPair):
    """The reference's error value for one result (None: verified)."""
    code, h, t = r.code, p.header, p.trusted
    if code == OK:
        return None
    if code == OLD_HEADER_EXPIRED:
        return ErrOldHeaderExpired((r.expired_seconds, r.expired_nanos), p.now)
    if code == GO_PATH:
        return GoPath()
    basic = "untrustedHeader.ValidateBasic failed: "
    if code == HEADER_BASIC:  # the Go method has the text
        return ErrInvalidHeader(GoError(basic + "invalid header or commit"))
    if code == WRONG_CHAIN:
        return ErrInvalidHeader(GoError(basic + "header belongs to another chain %s, not %s"
                                        % (_goq(h["chain_id"]), _goq(t["chain_id"]))))
    if code == COMMIT_HEIGHT:
        return ErrInvalidHeader(GoError(basic + "header and commit height mismatch: %d vs %d"
                                        % (h["height"], p.commit.height)))
    if code == COMMIT_HEADER_HASH:
        return ErrInvalidHeader(GoError(basic + "commit signs block %s, header is block %s"
                                        % (_hexu(p.commit.block_id.hash), _hexu(bytes(r.hash)[:r.hash_len]))))
    if code == HEIGHT_NOT_GREATER:
        return ErrInvalidHeader(GoError("expected new header height %d to be greater than one of old header %d"
                                        % (h["height"], t["height"])))
    if code == TIME_NOT_AFTER:
        return ErrInvalidHeader(GoError("expected new header time %s to be after old header time %s"
                                        % (go_time(h["time"]), go_time(t["time"]))))
    if code == TIME_FROM_FUTURE:
        return ErrInvalidHeader(GoError("new header has a time from the future %s (now: %s; max clock drift: %s)"
                                        % (go_time(h["time"]), go_time(p.now), go_duration(p.max_clock_drift))))
    if code == VALS_HASH:
        return ErrInvalidHeader(GoError(
            "expected new header validators (%s) to match those that were supplied (%s) at height %d"
            % (_hexu(h["validators_hash"]), _hexu(bytes(r.hash)[:r.hash_len]), h["height"])))
    if code == NEXT_VALS_HASH:
        return GoError("expected old header next validators (%s) to match those from new header (%s)"
                       % (_hexu(t["next_validators_hash"]), _hexu(h["validators_hash"])))
    if code == TRUSTING:
        e = T._to_error(r.commit.code, r.commit, p.trusted_vals, None, p.commit)
        return ErrNewValSetCantBeTrusted(e) if isinstance(e, T.ErrNotEnoughVotingPowerSigned) else e
    if code == COMMIT:
        e = T._to_error(r.commit.code, r.commit, p.vals, p.commit.block_id, p.commit)
        return e if isinstance(e, T.GoPanic) else ErrInvalidHeader(e)
    raise RuntimeError("tmed: unknown light outcome %d" % code)


def verify(engine, pairs: Sequence[LightPair], flags: int = 0, verifier=None, hashes=None, stats: Optional[list] = None):
    """light.Verify for every pair with one call.

    engine: an Engine (tmed_light_verify: hashes and signatures on the device).  verifier: a Python
    batch verifier as for ``tmed.types.verify_commits`` (tmed_light_verify_with, the CPU test-suite);
    ``hashes`` = (header_hashes, header_ok, vals_hashes) then supplies the hashes.  flags: 0 or
    LIGHT_ORDERED.  stats, if a list, receives (verified_trusting, verified_light) per pair.
    Returns one Go-style error (or None, or GoPath()) per pair."""
    pl = PreparedLight(pairs)
    if verifier is None:
        pl.run(engine, flags)
    else:
        pl.run_with(verifier, *hashes, flags=flags)
    if stats is not None:
        stats.extend((int(pl.res[q].verified_trusting), int(pl.res[q].verified_light)) for q in range(pl.n))
    return pl.errors()
