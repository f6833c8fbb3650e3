"""Host mirror of ``state.MedianTime`` (reference ``state/state.go:268-285`` over
``tmtime.WeightedMedian``, ``types/time/time.go:35-58``) over the C ABI ``tmed_median_times``
(kernels in ``csrc/median.hip``, the same rule on the host in ``csrc/median_host.h``): the block
time ``validateBlock`` compares ``block.Time`` with (``state/validation.go:123-129``) and
``State.MakeBlock`` stamps on a proposal, for many (commit, validator set) pairs per call.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import types as T
from ._native import TMED_OK, TmedError

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
