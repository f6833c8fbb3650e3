"""The key-grouped visiting order of a key-cached chunk (csrc/kernels.hip launch_key_order:
key_hist_kernel, key_scan_kernel, key_scatter_kernel), restated in plain numpy: the bin rule, the
properties every output of the stage must have (check), and the index distributions
tests/test_gpu_keyed_stages.py sends through tmed_test_key_order.  No GPU here; the checker itself is
tested on doctored outputs in tests/test_keyed_stage_checkers.py.

The order inside a bin is free (LDS-atomic ranks), so the stage is checked by its properties, all
exact: the permutation loses and repeats nothing, bins do not decrease along it, and every bin's
cursor ends at the cumulative count."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xFFFFFFFF


def kernel_constants():
    """kKeyBins, kKeyTile (kernels.hip) and kKeyOrderMaxKeys (kernels.h), read by name."""
    out = {}
    for name in ("kernels.hip", "kernels.h"):
        with open(os.path.join(ROOT, "tendermint-fork_amd", "csrc", name)) as f:
            src = f.read()
        m = re.search(r"constexpr uint32_t kKeyBins = (\d+), kKeyTile = (\d+);", src)
        if m:
            out["kKeyBins"], out["kKeyTile"] = int(m.group(1)), int(m.group(2))
        m = re.search(r"constexpr uint32_t kKeyOrderMaxKeys = 1u << (\d+);", src)
        if m:
            out["kKeyOrderMaxKeys"] = 1 << int(m.group(1))
    return out


K = kernel_constants()
# the values the cases below rest on
assert K == {"kKeyBins": 4096, "kKeyTile": 4096, "kKeyOrderMaxKeys": 1 << 24}, K
BINS, TILE, MAX_KEYS = K["kKeyBins"], K["kKeyTile"], K["kKeyOrderMaxKeys"]


def shift_of(nkeys):
    """The smallest s with ((nkeys - 1) >> s) + 2 <= 4096."""
    s = 0
    while ((nkeys - 1) >> s) + 2 > BINS:
        s += 1
    return s


def nbins_of(nkeys):
    """The bins of the keys, plus one for every index past the set."""
    return ((nkeys - 1) >> shift_of(nkeys)) + 2


def bins_of(val_idx, nkeys):
    """Bin of every index: v >> shift, any v >= nkeys in the last bin."""
    v = np.asarray(val_idx, dtype=np.uint64)
    s = shift_of(nkeys)
    return np.where(v < nkeys, v >> np.uint64(s), np.uint64(nbins_of(nkeys) - 1)).astype(np.int64)


def reference_order(val_idx, nkeys, base):
    """One valid output of the stage: numpy's stable argsort of the bins -> (perm, cursor)."""
    b = bins_of(val_idx, nkeys)
    perm = (np.argsort(b, kind="stable") + base).astype(np.uint32)
    cursor = np.cumsum(np.bincount(b, minlength=nbins_of(nkeys))).astype(np.uint32)
    return perm, cursor


def check(val_idx, n, nkeys, base, perm, cursor, nbins, shift):
    """Asserts everything a correct launch_key_order leaves behind for val_idx[0..n)."""
    val_idx = np.asarray(val_idx, dtype=np.uint32)
    assert val_idx.shape == (n,) and perm.shape == (n,)
    assert shift == shift_of(nkeys), ("shift", shift, shift_of(nkeys))
    assert nbins == nbins_of(nkeys), ("nbins", nbins, nbins_of(nkeys))
    assert cursor.shape == (nbins,)
    p = perm.astype(np.int64)
    assert not (p == SENTINEL).any(), "a position the scatter never wrote: %s" % np.flatnonzero(p == SENTINEL)[:8]
    rel = p - base
    assert ((rel >= 0) & (rel < n)).all(), "an entry outside [base, base + n): %s" % rel[(rel < 0) | (rel >= n)][:8]
    # nothing lost, nothing twice
    assert (np.sort(rel) == np.arange(n)).all(), "not a permutation of [base, base + n)"
    b = bins_of(val_idx, nkeys)
    along = b[rel]
    assert (np.diff(along) >= 0).all(), "bins decrease along perm at %s" % np.flatnonzero(np.diff(along) < 0)[:8]
    ends = np.cumsum(np.bincount(b, minlength=nbins))
    assert ends[-1] == n
    bad = np.flatnonzero(cursor.astype(np.int64) != ends)
    assert bad.size == 0, "cursor != cumulative count at bins %s" % bad[:8]


# ---- the cases ------------------------------------------------------------------------------------
GRID_N = (1, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)
GRID_NKEYS = (1, 2, 1023, 1024, 2048, 3072, 4094, 4095, 4096, 4097, 8190, 8191, 10000, 1 << 24)
GRID_BASES = (0, 4096, 1 << 20)
# what the grid must reach: the scan at 1, 2, 3 and 4 bins a lane, and exactly 4096 bins
GRID_NBINS = {1024, 1025, 2049, 3073, 4096}
GRID_SHIFTS = {0, 1, 2, 13}


def uniform(n, nkeys, seed):
    return np.random.default_rng(seed).integers(0, nkeys, n, dtype=np.uint64).astype(np.uint32)


def distributions(nkeys, n=12289):
    """(name, val_idx) for a key set of nkeys keys: the batches a uniform draw never gives."""
    rng = np.random.default_rng(1000 + nkeys)
    s = shift_of(nkeys)
    out = [
        ("one key", np.full(n, nkeys // 3, np.uint32)),  # one bin takes whole tiles
        ("all past the set", np.where(rng.random(n) < 0.5, nkeys, SENTINEL).astype(np.uint32)),
        ("first and last key", np.where(rng.random(n) < 0.5, 0, nkeys - 1).astype(np.uint32)),
        ("descending", ((n - 1 - np.arange(n, dtype=np.int64)) * nkeys // n).astype(np.uint32)),
    ]
    if nkeys <= 1 << 16:
        out.append(("each key once", rng.permutation(nkeys).astype(np.uint32)))
    if s > 0:  # the two keys either side of the first bin edge
        out.append(("bin edge", np.where(rng.random(n) < 0.5, (1 << s) - 1, 1 << s).astype(np.uint32)))
    v = uniform(n, nkeys, 2000 + nkeys)
    bad = rng.random(n) < 0.01
    v[bad] = np.where(rng.random(int(bad.sum())) < 0.5, nkeys, SENTINEL).astype(np.uint32)
    out.append(("1% bad", v))
    return out
