"""The host entry points' call frame on the device: the contract the three raw host batches share
(tmed_verify_batch, tmed_verify_batch_keyset, tmed_verify_batch_zip215: argument checks, staging
buffers that grow and are reused, the sig_lens mask, kernel timing), and the one staging arena of
tmed_commit_hashes, tmed_header_hashes, tmed_median_times and tmed_verify_votes, whose calls follow
each other in both orders and from two threads on one context.  Expected decisions come from the C
port (oracle.port) and the restatements the neighbouring suites use."""
import ctypes
import random
import threading

import numpy as np
import pytest

import blockhash_cases as B
import median_cases as MC
import tmed.state as S
import tmed.types as T
import tmed.votes as V
import vote_cases as VC
from conftest import engine_with_env
from oracle import merkle as M
from oracle import port
from test_merkle_oracle import kat_header
from tmed._native import TMED_EINVAL, TMED_ENOKEYSET, TMED_OK, lib
from tmed.merkle import CommitHashBatch, HeaderBatch

pytestmark = pytest.mark.gpu

ENTRIES = ("generic", "keyed", "zip215")
N_KEYS = 16
GLAT_MAX = 24576            # tmed_ctx::glat_max's default: one more takes the throughput kernels
UNTIMED_MAX = 1024          # ctx.h kLatencyUntimedMax
POOL = GLAT_MAX + 1


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Pool:
    """POOL signed tuples over N_KEYS keys, some signatures damaged, and what the oracle says of each
    under both rules; any prefix is a batch."""

    def __init__(self):
        rng = np.random.default_rng(20)
        kseeds = rng.integers(0, 256, (N_KEYS, 32), dtype=np.uint8)
        self.idx = rng.integers(0, N_KEYS, POOL).astype(np.uint32)
        lens = rng.integers(0, 96, POOL)
        self.offs = np.zeros(POOL + 1, np.uint32)
        self.offs[1:] = np.cumsum(lens)
        self.msgs = rng.integers(0, 256, int(self.offs[-1]) + 16, dtype=np.uint8)
        self.sigs, self.pubs = port.sign_batch(kseeds[self.idx], self.msgs, self.offs.astype(np.uint64), 8)
        self.sigs[2::5, 7] ^= 0x20    # R
        self.sigs[4::11, 40] ^= 1     # S
        self.kpubs = np.frombuffer(b"".join(port.pubkey_from_seed(s.tobytes()) for s in kseeds), np.uint8).reshape(-1, 32)
        assert (self.kpubs[self.idx] == self.pubs).all()
        o64 = self.offs.astype(np.uint64)
        self.exp = {"generic": port.verify_batch(self.pubs, self.sigs, self.msgs, o64, 8)}
        self.exp["keyed"] = self.exp["generic"]
        self.exp["zip215"] = port.verify_batch(self.pubs, self.sigs, self.msgs, o64, 8, zip215=True)
        assert self.exp["generic"][0] == 1 and self.exp["generic"][2] == 0
        assert 0 < self.exp["generic"][:3].sum() < 3


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.fixture(scope="module")
def ctx():
    """This module's own context (kernel timing off, as tmed_init leaves it)."""
    e = engine_with_env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def handle(ctx, pool):
    h = ctx.keyset_load(pool.kpubs)
    yield h
    ctx.keyset_free(h)


def raw(eng, entry, handle, keys, sigs, sig_lens, msgs, offs, n, out):
    """The C call itself: keys are 32-byte encodings (generic, zip215) or u32 indexes (keyed)."""
    l = lib()
    if entry == "keyed":
        return l.tmed_verify_batch_keyset(eng._h, handle, _ptr(keys), _ptr(sigs), _ptr(sig_lens), _ptr(msgs), _ptr(offs),
                                          n, _ptr(out))
    fn = l.tmed_verify_batch if entry == "generic" else l.tmed_verify_batch_zip215
    return fn(eng._h, _ptr(keys), _ptr(sigs), _ptr(sig_lens), _ptr(msgs), _ptr(offs), n, _ptr(out))


def run_prefix(eng, entry, handle, pool, n, sig_lens=None, offs=None):
    """(rc, out) of the first n tuples of the pool; out starts as 0xAA."""
    out = np.full(max(n, 4), 0xAA, np.uint8)
    keys = pool.idx if entry == "keyed" else pool.pubs
    rc = raw(eng, entry, handle, keys, pool.sigs, sig_lens, pool.msgs, pool.offs if offs is None else offs, n, out)
    return rc, out


def check_prefix(eng, entry, handle, pool, n):
    rc, out = run_prefix(eng, entry, handle, pool, n)
    assert rc == TMED_OK
    bad = np.nonzero(out[:n] != pool.exp[entry][:n])[0]
    assert bad.size == 0, (entry, n, bad[:8])


# ---- the raw batch contract -------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_batch_leaves_out_untouched(ctx, handle, pool, entry):
    rc, out = run_prefix(ctx, entry, handle, pool, 0)
    assert rc == TMED_OK and (out == 0xAA).all()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", [1, 3, 1024, 1025])
def test_sizes(ctx, handle, pool, entry, n):
    check_prefix(ctx, entry, handle, pool, n)


def test_generic_just_past_the_latency_kernels(ctx, handle, pool):
    assert POOL == GLAT_MAX + 1
    check_prefix(ctx, "generic", handle, pool, POOL)


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_messages_and_no_message_array(ctx, handle, entry):
    """Every message empty, msgs NULL: accepted, decisions equal the oracle's."""
    n = 5
    rng = np.random.default_rng(21)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    offs = np.zeros(n + 1, np.uint32)
    sigs, pubs = port.sign_batch(seeds, np.zeros(16, np.uint8), offs.astype(np.uint64), 1)
    sigs[3, 9] ^= 2
    exp = port.verify_batch(pubs, sigs, np.zeros(16, np.uint8), offs.astype(np.uint64), 1, zip215=entry == "zip215")
    assert exp.tolist() == [1, 1, 1, 0, 1]
    h, keys = handle, pubs
    if entry == "keyed":
        h, keys = ctx.keyset_load(pubs), np.arange(n, dtype=np.uint32)
    try:
        out = np.full(n, 0xAA, np.uint8)
        assert raw(ctx, entry, h, keys, sigs, None, None, offs, n, out) == TMED_OK
        assert out.tolist() == exp.tolist()
    finally:
        if entry == "keyed":
            ctx.keyset_free(h)


@pytest.mark.parametrize("entry", ENTRIES)
def test_decreasing_offset_is_refused(ctx, handle, pool, entry):
    offs = pool.offs[:9].copy()
    offs[5] = offs[4] - 1 if offs[4] else offs[6] + 1
    assert offs[5] < offs[4] or offs[6] < offs[5]
    rc, out = run_prefix(ctx, entry, handle, pool, 8, offs=offs)
    assert rc == TMED_EINVAL and (out == 0xAA).all()
    check_prefix(ctx, entry, handle, pool, 8)


@pytest.mark.parametrize("entry", ENTRIES)
def test_short_signature_is_rejected(ctx, handle, pool, entry):
    """sig_lens[i] = 63 on a valid signature gives 0 (crypto/ed25519/ed25519.go:150-152); the others stay."""
    n = 8
    exp = pool.exp[entry][:n].copy()
    assert exp[0] == 1 and exp[1] == 1
    lens = np.full(n, 64, np.uint32)
    lens[1] = 63
    exp[1] = 0
    rc, out = run_prefix(ctx, entry, handle, pool, n, sig_lens=lens)
    assert rc == TMED_OK and out[:n].tolist() == exp.tolist()


def test_keyed_refusals(ctx, handle, pool):
    """An unknown handle, and a key index equal to the set's size; a valid call follows each."""
    rc, out = run_prefix(ctx, "keyed", handle + 1000, pool, 8)
    assert rc == TMED_ENOKEYSET and (out == 0xAA).all()
    check_prefix(ctx, "keyed", handle, pool, 8)
    idx = pool.idx[:8].copy()
    idx[6] = N_KEYS
    out = np.full(8, 0xAA, np.uint8)
    assert raw(ctx, "keyed", handle, idx, pool.sigs, None, pool.msgs, pool.offs, 8, out) == TMED_EINVAL
    assert (out == 0xAA).all()
    check_prefix(ctx, "keyed", handle, pool, 8)


@pytest.mark.parametrize("entry", ENTRIES)
def test_buffers_grow_and_are_reused(pool, entry):
    """8, then 4,096, then 8 signatures on a context of its own."""
    eng = engine_with_env()
    try:
        h = eng.keyset_load(pool.kpubs) if entry == "keyed" else 0
        for n in (8, 4096, 8):
            check_prefix(eng, entry, h, pool, n)
    finally:
        eng.close()


def test_kernel_timing_rule(ctx, handle, pool):
    """Timing off: a generic batch of up to kLatencyUntimedMax records no events and reports 0; a larger
    one and every keyed one report their kernel time."""
    check_prefix(ctx, "generic", handle, pool, UNTIMED_MAX + 1)
    assert ctx.last_kernel_ms() > 0
    check_prefix(ctx, "generic", handle, pool, UNTIMED_MAX)
    assert ctx.last_kernel_ms() == 0
    check_prefix(ctx, "keyed", handle, pool, 3)
    assert ctx.last_kernel_ms() > 0
    check_prefix(ctx, "generic", handle, pool, UNTIMED_MAX)
    assert ctx.last_kernel_ms() == 0
    check_prefix(ctx, "keyed", handle, pool, UNTIMED_MAX + 1)
    assert ctx.last_kernel_ms() > 0


# ---- the staging arena ------------------------------------------------------------------------------

ZERO_TIME = (B.ZERO_TIME_SECONDS, 0)
KINDS = ("commit_1x300", "median", "votes_keyed", "votes_generic", "headers", "commit_2x5")


class Kit:
    """The inputs of the arena's call kinds, built once, and each kind's oracle check."""

    def __init__(self):
        sweep = B.cycle_sigs()
        self.c300 = sweep[:300]
        self.c5 = sweep[300:305]
        self.absent5 = [(T.FLAG_ABSENT, b"", ZERO_TIME[0], ZERO_TIME[1], b"")] * 5
        rng = random.Random(22)
        self.pairs = [MC.random_pair(rng, 3), MC.random_pair(rng, 600)]   # 600 > kMedWaveMax: the workgroup shape
        self.vals, self.vfields, self.named = VC.pool(130, 6)             # two full 64-vote workgroups and two votes
        self.vote_exp = [VC.expected(VC.request(self.vals, self.vfields, self.named), v) for _, v in self.named]
        self.headers = [kat_header(), dict(kat_header(), height=2**40, chain_id="x" * 50),
                        dict(kat_header(), time=(0, 999999999), last_block_id=(b"", 0, b""))]

    def runner(self, kind, eng):
        """A callable that makes the call on eng and returns its result; its C structs are its own."""
        if kind == "commit_1x300":
            b = CommitHashBatch([B.packed_commit(self.c300)])
            return lambda: _hashes(*b.run(eng))
        if kind == "commit_2x5":
            b = CommitHashBatch([B.packed_commit(self.c5), B.packed_commit(self.absent5)])
            b.cs[1].sigs = None
            b.cs[1].addresses = None
            return lambda: _hashes(*b.run(eng))
        if kind == "median":
            pm = S.PreparedMedian(self.pairs)

            def run():
                pm.run(eng)
                return pm.results(), [int(d) for d in pm.on_device()]
            return run
        if kind == "headers":
            hb = HeaderBatch(self.headers)
            return lambda: hb.run(eng)
        vals = self.vals
        if kind == "votes_keyed":
            n = len(vals.validators)
            h = eng.keyset_load(vals.packed()[0])  # freed with the context
            vals = T.ValidatorSet(vals.validators, keyset=h, keyset_index=np.arange(n, dtype=np.uint32))
        pv = V.PreparedVotes([VC.request(vals, self.vfields, self.named)])
        return lambda: [int(c) for c in pv.run(eng)]

    def check(self, kind, got):
        if kind == "commit_1x300":
            assert got == [B.commit_hash(self.c300)]
        elif kind == "commit_2x5":
            assert got == [B.commit_hash(self.c5), B.commit_hash(self.absent5)]
        elif kind == "median":
            res, dev = got
            for r, (c, v) in zip(res, self.pairs):
                assert MC.same(r, MC.reference(c, v)), (len(c.signatures), r)
            assert dev == [int(MC.fast_path(c, v)) for c, v in self.pairs] == [1, 1]
        elif kind == "headers":
            assert got == [M.header_hash(h) for h in self.headers] and None not in got
        else:
            assert got == self.vote_exp and set(got) == set(range(10))


def _hashes(out, ok):
    return [bytes(out[i]) if ok[i] else None for i in range(len(ok))]


@pytest.fixture(scope="module")
def kit():
    return Kit()


@pytest.fixture(scope="module")
def fresh(kit):
    """Each kind's result on a context that has made no other call."""
    out = {}
    for kind in KINDS:
        eng = engine_with_env()
        try:
            out[kind] = kit.runner(kind, eng)()
        finally:
            eng.close()
        kit.check(kind, out[kind])
    return out


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_arena_call_sequence(ctx, kit, fresh, order):
    """The arena's users behind each other on one context: each finds the regions the one before
    filled (the all-absent commit of commit_2x5 packs no signature and no address rows at all)."""
    kinds = KINDS if order == "forward" else KINDS[::-1]
    runners = {k: kit.runner(k, ctx) for k in kinds}
    for k in kinds:
        got = runners[k]()
        assert got == fresh[k], k
        kit.check(k, got)


def test_arena_two_threads(ctx, kit, fresh):
    """Two threads on one context, each alternating two call kinds 20 times."""
    plans = [("commit_1x300", "median"), ("votes_generic", "headers")]
    results, errors = [[] for _ in plans], []

    def work(t):
        try:
            runners = [(k, kit.runner(k, ctx)) for k in plans[t]]
            for _ in range(20):
                for k, r in runners:
                    results[t].append((k, r()))
        except BaseException as e:  # noqa: B902 (reported below, on the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(len(plans))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(len(plans)):
        assert len(results[t]) == 40
        for k, got in results[t]:
            assert got == fresh[k], k
