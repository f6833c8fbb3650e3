"""The structural stages between a key-cached batch and its decisions, on the device, each alone and
then together (all comparisons exact):

 * the key-grouped visiting order (csrc/kernels.hip launch_key_order: key_hist_kernel,
   key_scan_kernel, key_scatter_kernel) through tmed_test_key_order, checked by the properties of
   tests/key_order_cases.py: every bin count the scan takes another path at, shifts above 0 on
   shuffled indices, whole tiles in one bin, only out-of-range indices, scratch left by another shape;
 * the batched finish (launch_finish, verify_finish_kernel, verify_core.h finish_group) through
   tmed_test_finish on the rows of tests/finish_cases.py: the change of G at 65,536 / 65,537 and
   131,072 / 131,073, G = 16, the lanes that own one slot fewer, perm far from the identity, the
   compare rule steered from the point's side, and Z = 0 inside a lane's group;
 * the chunk loop of launch_verify_keyset with the order on (a 4,096-slot slab: chunks of 4096, 4096,
   4096 and 1) on the three key-cached throughput kernels, and the second kFinCap block (n > 2^20),
   against the port.

The checkers are shown to fail on doctored outputs in tests/test_keyed_stage_checkers.py, the same
finish cases run on the host build in tests/test_kernel_host.py."""
import numpy as np
import pytest

import finish_cases as FC
import key_order_cases as KO
from conftest import engine_with_env
from oracle import port

pytestmark = pytest.mark.gpu


# ---- 1, 2: the key-grouped visiting order ---------------------------------------------------------
def _run_order(eng, v, nkeys, base):
    perm, cursor, nbins, shift = eng.key_order(v, nkeys, base)
    KO.check(v, len(v), nkeys, base, perm, cursor, nbins, shift)
    return nbins, shift


def test_key_order_grid(engine):
    """Uniform indices over the (n, nkeys) grid at three index bases."""
    rule = {(KO.nbins_of(k), KO.shift_of(k)) for k in KO.GRID_NKEYS}
    assert KO.GRID_NBINS <= {b for b, _ in rule} and {s for _, s in rule} == KO.GRID_SHIFTS
    seen = set()
    for nkeys in KO.GRID_NKEYS:
        for n in KO.GRID_N:
            for base in KO.GRID_BASES:
                seen.add(_run_order(engine, KO.uniform(n, nkeys, 31 * n + nkeys % 9973 + base), nkeys, base))
    assert seen == rule


@pytest.mark.parametrize("nkeys", [10000, 4095])
def test_key_order_distributions(engine, nkeys):
    """The batches a uniform draw never gives, at shift 2 (2,501 bins) and at exactly 4,096 bins."""
    names = set()
    for k, (name, v) in enumerate(KO.distributions(nkeys)):
        _run_order(engine, v, nkeys, (0, 4096, 1 << 20)[k % 3])
        names.add(name)
    assert {"one key", "all past the set", "first and last key", "descending", "each key once", "1% bad"} <= names
    assert ("bin edge" in names) == (KO.shift_of(nkeys) > 0)


def test_key_order_on_scratch_left_by_another_shape(engine):
    """Calls back to back with different (n, nkeys) on one context: no cursor of the earlier call
    survives into the later one, whichever has more bins."""
    shapes = [(12289, 4095), (300, 2), (4097, 10000), (12289, 1 << 24), (4096, 1), (8192, 8190), (257, 1023)]
    for i, (n, nkeys) in enumerate(shapes + shapes[::-1]):
        _run_order(engine, KO.uniform(n, nkeys, 50 + i), nkeys, 4096 * (i % 2))


def test_key_order_refuses_what_the_launcher_refuses(engine):
    from tmed._native import TmedError
    v = np.zeros(16, np.uint32)
    for n_keys in (0, KO.MAX_KEYS + 1):
        with pytest.raises(TmedError):
            engine.key_order(v, n_keys)
    with pytest.raises(TmedError):
        engine.key_order(np.zeros((1 << 20) + 1, np.uint32), 5)
    with pytest.raises(TmedError):
        engine.key_order(v, 5, 0xFFFFFFFF - 8)
    _run_order(engine, KO.uniform(16, KO.MAX_KEYS, 1), KO.MAX_KEYS, 0xFFFFFFFF - 16)


# ---- 3, 4: the batched finish ---------------------------------------------------------------------
FINISH_M = (1, 255, 256, 257, 65535, 65536, 65537, 131072, 131073, (1 << 20) - 15, 1 << 20)
FINISH_GL = {1: (1, 1), 255: (1, 255), 256: (1, 256), 257: (1, 257), 65535: (1, 65535), 65536: (1, 65536),
             65537: (2, 32769), 131072: (2, 65536), 131073: (3, 43691), (1 << 20) - 15: (16, 65536),
             1 << 20: (16, 65536)}


@pytest.fixture(scope="module")
def finish_bulk():
    """The 2^20 pooled rows every finish case is a prefix of, built once."""
    return FC.bulk(FC.FIN_CAP)


def _finish(eng, c, base, perm):
    return eng.finish(c["xyz"], c["r"], c["bits_in"], base, perm)


@pytest.mark.parametrize("m", FINISH_M)
def test_finish_at_its_group_boundaries(engine, finish_bulk, m):
    """Every bit of the finish at fin_base 0 and 4096, with perm NULL and with a seeded shuffle of all
    fin_base + m indices (the 2^20 case once each way)."""
    assert FC.groups(m) == FINISH_GL[m]
    c = FC.case(m, FC.FIN_CAP)
    assert (c["G"], c["L"]) == FINISH_GL[m] and c["full"] == (m >= 64)
    runs = [(0, False), (4096, True)] if m == 1 << 20 else [(0, False), (0, True), (4096, False), (4096, True)]
    for base, shuffled in runs:
        perm = FC.shuffled_perm(m, base, m % 1000 + base) if shuffled else None
        out = _finish(engine, c, base, perm)
        FC.check(c, out, base, perm)


@pytest.mark.parametrize("m", [65537, 1 << 20])
def test_finish_guard_keeps_the_group(engine, finish_bulk, m):
    """Z = 0 as the first, a middle and the last slot of a lane's group, in two slots and in every slot,
    in lane 0, the last lane that owns G slots, the first that owns G - 1 and the last lane: rejected,
    and every neighbour in the same group keeps its bit (G = 2 and G = 16)."""
    c = FC.case(m, FC.FIN_CAP)
    assert len(c["guards"]) >= 3 * len(FC.GUARDS)
    assert sum(len(near) for _, _, _, near in c["guards"]) >= (40 if c["G"] == 16 else 6)
    perm = FC.shuffled_perm(m, 0, 77) if m == 65537 else None
    out = _finish(engine, c, 0, perm)
    FC.check_guards(c, out, 0, perm)
    FC.check(c, out, 0, perm)


def test_finish_refuses_bad_shapes(engine):
    from tmed._native import TmedError
    c = FC.case(257, 4099)
    for base, perm in ((2 * FC.FIN_CAP - 256, None), (0, np.full(257, 257, np.uint32))):
        with pytest.raises(TmedError):
            _finish(engine, c, base, perm)
    with pytest.raises(TmedError):
        engine.finish(np.zeros((0, 30), np.int32), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8))


# ---- 5, 6: the chunk loop end to end --------------------------------------------------------------
NK, N5, POOL6, N6 = 700, 12289, 8192, (1 << 20) + 4097
MSG = 128  # every message fills its 128-byte slot, so a tiled batch keeps fixed offsets


@pytest.fixture(scope="module")
def signed():
    """700 keys (two comb chunks, 512 + 188) and 12,289 port-signed tuples by keys in random order,
    1 % corrupted, with the port's decisions."""
    rng = np.random.default_rng(0x5EED)
    seeds = rng.integers(0, 256, (NK, 32), dtype=np.uint8)
    _, pubs = port.sign_batch(seeds, np.zeros(8 * NK + 16, np.uint8), np.arange(NK + 1, dtype=np.uint64) * 8, 8)
    vi = rng.integers(0, NK, N5).astype(np.uint32)
    vi[:4] = [0, NK - 1, 511, 512]
    offs = np.arange(N5 + 1, dtype=np.uint64) * MSG
    msgs = rng.integers(0, 256, N5 * MSG + 16, dtype=np.uint8)
    sigs, _ = port.sign_batch(seeds[vi], msgs, offs, 16)
    bad = rng.random(N5) < 0.01
    sigs[bad, rng.integers(0, 64, int(bad.sum()))] ^= 0x10
    exp = port.verify_batch(pubs[vi], sigs, msgs, offs, 16)
    assert 0 < (exp == 0).sum() <= bad.sum() and exp[:POOL6].sum() < POOL6
    return dict(pubs=pubs, vi=vi, sigs=sigs, msgs=msgs, exp=exp)


def _device_run(eng, h, vi, sigs, msgs, n, times):
    """The batch from device arrays, `times` times, each into an out array pre-filled with 0xAA (a
    lost index keeps it) -> the outs."""
    import torch
    dev = torch.device("cuda", 0)
    d_vi = torch.from_numpy(vi.view(np.int32)).to(dev)
    d_sig = torch.from_numpy(sigs).to(dev)
    d_msg = torch.from_numpy(msgs).to(dev)
    d_off = torch.from_numpy((np.arange(n + 1, dtype=np.uint32) * MSG).view(np.int32)).to(dev)
    outs = []
    for _ in range(times):
        d_out = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        eng.verify_keyset_device(h, d_vi, d_sig, d_msg, d_off, d_out, n, 0)
        torch.cuda.synchronize(dev)
        outs.append(d_out.cpu().numpy())
    return outs


def _with_bad_indices(vi, exp, n, seed):
    rng = np.random.default_rng(seed)
    at = rng.choice(n, 12, replace=False)
    vi, exp = vi.copy(), exp.copy()
    vi[at[::2]] = NK
    vi[at[1::2]] = 0xFFFFFFFF
    exp[at] = 0
    return vi, exp


@pytest.mark.parametrize("env,b_bits,a_bits", [({}, 24, 12), ({"TMED_KS_ACOMB": 0}, 24, 8), ({"TMED_B24": 0}, 16, 8)])
def test_chunk_loop_with_the_order_on(signed, env, b_bits, a_bits):
    """12,289 signatures by 700 keys through a 4,096-slot slab: four chunks (4096, 4096, 4096, 1), each
    with its own key order at its own base, one finish over all of them; twice per context, so the
    default context runs keyset_straus_b24 then keyset_straus_ab24.  Indices 700 and 2^32 - 1 give 0."""
    eng = engine_with_env(TMED_LAT_MAX=0, TMED_SLAB_SLOTS=4096, **env)
    try:
        h = eng.keyset_load(signed["pubs"])
        try:
            assert eng.keyset_b_window_bits() == b_bits
            vi, exp = _with_bad_indices(signed["vi"], signed["exp"], N5, 5)
            for out in _device_run(eng, h, vi, signed["sigs"], signed["msgs"], N5, 2):
                bad = np.flatnonzero(out != exp)
                assert bad.size == 0, (bad[:8], out[bad[:8]], exp[bad[:8]])
            assert eng.keyset_a_window_bits(h) == a_bits
        finally:
            eng.keyset_free(h)
    finally:
        eng.close()


def test_second_fin_block(signed):
    """2^20 + 4,097 signatures (a pool of 8,192 tuples tiled): the second kFinCap block holds 4,097, its
    key order, fin slots and finish all at base 2^20."""
    reps = -(-N6 // POOL6)
    vi = np.tile(signed["vi"][:POOL6], reps)[:N6]
    exp = np.tile(signed["exp"][:POOL6], reps)[:N6]
    sigs = np.tile(signed["sigs"][:POOL6], (reps, 1))[:N6]
    msgs = np.concatenate([np.tile(signed["msgs"][:POOL6 * MSG], reps)[:N6 * MSG], np.zeros(16, np.uint8)])
    vi, exp = _with_bad_indices(vi, exp, N6, 6)
    vi[[(1 << 20) - 1, 1 << 20, N6 - 1]] = [NK, 0xFFFFFFFF, NK]  # either side of the block edge, and the last
    exp[[(1 << 20) - 1, 1 << 20, N6 - 1]] = 0
    eng = engine_with_env(TMED_LAT_MAX=0)
    try:
        h = eng.keyset_load(signed["pubs"])
        try:
            out, = _device_run(eng, h, vi, sigs, msgs, N6, 1)
            bad = np.flatnonzero(out != exp)
            assert bad.size == 0, (bad[:8], out[bad[:8]], exp[bad[:8]])
        finally:
            eng.keyset_free(h)
    finally:
        eng.close()
