"""state.MedianTime on the device: tmed_median_times (csrc/median.hip) against the restatement in
median_cases.py over the CPU suite's corpus in one call, at every lane-count boundary of the two
kernel shapes, on key patterns chosen against the bit search, in a call that mixes sizes, routes and
shared sets, and after a submitted blocksync window."""
import os
import random
import re

import pytest

import median_cases as MC
import tmed
import tmed.state as S
import tmed.types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """The shape constants of csrc/median.hip, by name."""
    with open(os.path.join(ROOT, "tendermint-fork_amd", "csrc", "median.hip")) as f:
        src = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (kMed\w+) = (\d+);", src)}


K = kernel_constants()
WAVE = 64
WAVE_MAX = K["kMedWaveMax"]                    # the threshold between the two shapes
WAVE_GROUP = WAVE * K["kMedWaveGroups"]        # the wave shape's workgroup (kMedWaveGroups commits)
BLOCK_LANES = WAVE * K["kMedBlockWaves"]       # the block shape's workgroup
BLOCK_CAP = K["kMedBlockCap"]                  # per-lane element count x workgroup size
MAX_VOTES = 10000                              # types.MaxVotesCount


def check(engine, pairs, want=None, device=None):
    """One call over pairs; outcomes equal `want` (default: the dict-lookup reference), on_device
    equals `device` (default: the fast-path rule)."""
    pm = S.PreparedMedian(pairs)
    pm.run(engine)
    got, dev = pm.results(), pm.on_device()
    for q, (c, v) in enumerate(pairs):
        w = MC.reference(c, v) if want is None else want[q]
        assert MC.same(got[q], w), (q, len(c.signatures), got[q], w)
        d = MC.fast_path(c, v) if device is None else device[q]
        assert dev[q] == int(d), (q, len(c.signatures), dev[q])
    return pm


def test_corpus_in_one_call_gpu(engine):
    """Every corpus case in one call: sizes, fast-path and host-route pairs mixed; outcomes equal
    the literal restatement, on_device is 1 exactly for the pairs the fast-path rule admits."""
    cases = MC.corpus()
    pairs = [(c, v) for _, c, v in cases]
    pm = check(engine, pairs, want=[MC.expected(c, v) for c, v in pairs])
    dev = pm.on_device()
    assert 0 < dev.sum() < len(pairs)
    codes = {r[0] for r, d in zip(pm.results(), dev) if d}
    assert codes == {S.MEDIAN_OK, S.MEDIAN_ZERO_TIME, S.MEDIAN_GO_PATH}  # each decided on the device too
    host = S.PreparedMedian(pairs)
    host.run(None)
    assert host.results() == pm.results() and list(host.entered()) == list(pm.entered())
    assert engine.last_kernel_ms() > 0


def test_lane_count_boundaries_gpu(engine):
    """Aligned commits one below, at and one above the wavefront, both shapes' workgroup sizes, the
    wave shape's capacity (the threshold between the shapes) and the block shape's register
    capacity; one of MaxVotesCount; one of 20,001, past any capacity (the strided loop)."""
    assert (WAVE_MAX, WAVE_GROUP, BLOCK_LANES, BLOCK_CAP) == (WAVE * K["kMedWavePerLane"], 256, 1024,
                                                              BLOCK_LANES * K["kMedBlockPerLane"])
    assert WAVE_MAX < MAX_VOTES <= BLOCK_CAP < 20001
    rng = random.Random(3)
    sizes = sorted({b + d for b in (WAVE, 2 * WAVE, WAVE_GROUP, WAVE_MAX, BLOCK_LANES, BLOCK_CAP) for d in (-1, 0, 1)})
    sizes += [1, MAX_VOTES, 20001]
    pairs = [MC.random_pair(rng, n) for n in sizes]
    pairs += [MC.random_pair(rng, n, flag_kinds=(2,)) for n in (WAVE_MAX + 1, BLOCK_CAP + 1, 20001)]
    check(engine, pairs, device=[True] * len(pairs))
    # the wave shape's last workgroup full, one commit short and one commit over
    for m in (K["kMedWaveGroups"] - 1, K["kMedWaveGroups"], K["kMedWaveGroups"] + 1):
        check(engine, [MC.random_pair(rng, 65) for _ in range(m)], device=[True] * m)
    # the last element alone carries the weight: the highest lane, and the strided loop's last turn
    for n in (WAVE_MAX, WAVE_MAX + 1, BLOCK_CAP, BLOCK_CAP + 1, 20001):
        vals = MC.valset(n, [0] * (n - 1) + [9], "last")
        times = [MC.t_plus(-i) for i in range(n)]
        pm = check(engine, [(MC.commit_for(vals, times), vals)], device=[True])
        assert pm.results()[0] == (S.MEDIAN_OK, times[-1])


@pytest.mark.parametrize("n", [175, MAX_VOTES])
def test_adversarial_keys_gpu(engine, n):
    """Key and weight patterns against the bit search, on both shapes."""
    lo, hi = MC.MIN_TIME, MC.MAX_TIME
    near = [MC.t_plus(0, i) for i in range(n)]
    pairs = []

    def add(powers, times, tag):
        vals = MC.valset(n, powers, "adv-" + tag)
        pairs.append((MC.commit_for(vals, times), vals))

    top = max(range(n), key=lambda i: MC.unix_nano(near[(i * 7) % n]))
    shuffled = [near[(i * 7) % n] for i in range(n)]
    bottom = min(range(n), key=lambda i: MC.unix_nano(shuffled[i]))
    add([5 if i == top else 0 for i in range(n)], shuffled, "largest")      # all weight on the largest key
    add([5 if i == bottom else 0 for i in range(n)], shuffled, "smallest")  # ... on the smallest
    add([1 if i == top else 0 for i in range(n)], shuffled, "largest1")     # total 1: median 0
    # keys equal except for the sign (the bias bit): -1 ns and 0 ns, and the two ends of int64
    add([1] * n, [(-1, MC.NANOS - 1) if i % 2 else (0, 0) for i in range(n)], "sign")
    add([1] * n, [(-1, MC.NANOS - 1) if i % 3 else (0, 0) for i in range(n)], "sign3")
    add([1] * n, [lo if i % 2 else hi for i in range(n)], "ends")
    add([2 if i == 0 else 1 for i in range(n)], [hi if i else lo for i in range(n)], "ends1")
    # keys equal except for bit 0
    add([1] * n, [(MC.T1[0], MC.T1[1] ^ (i & 1)) for i in range(n)], "bit0")
    add([3 if i % 2 else 2 for i in range(n)], [(MC.T1[0], MC.T1[1] ^ (i & 1)) for i in range(n)], "bit0w")
    # alternating huge and tiny weights, keys ascending: the last weight is chosen so that the sum up
    # to key j is the median - 1, the median, the median + 1; the total stays below 2^63
    huge = (MC.INT64_MAX - n) // (n // 2 + 4)
    j = (n // 2 + 2) & ~1
    want_at = {}
    for d in (1, 0, -1):
        for odd in (0, 1):
            powers = [huge if i % 2 == 0 else 1 for i in range(n - 1)]
            prefix = sum(powers[:j + 1])
            powers.append(2 * (prefix + d) - sum(powers) + odd)
            assert powers[-1] > 0 and sum(powers) <= MC.INT64_MAX and sum(powers) // 2 == prefix + d
            add(powers, near, "huge%d%d" % (d, odd))
            want_at[len(pairs) - 1] = near[j + 1] if d == 1 else near[j]
    pm = check(engine, pairs, device=[True] * len(pairs))
    assert all(r[0] == S.MEDIAN_OK for r in pm.results())
    for q, t in want_at.items():
        assert pm.results()[q][1] == t, q


def test_mixed_call_gpu(engine):
    """300 commits of random sizes in [1, 400] and two of 10,000 in one call over three validator
    sets shared by pointer; where a commit is as long as its set it takes the kernels, else the host
    route.  Results equal those of one call per pair."""
    rng = random.Random(5)
    sets = [MC.valset(175), MC.valset(400), MC.valset(MAX_VOTES)]
    pairs = []
    for k in range(300):
        vals = sets[k % 2]
        full = len(vals.validators)
        n = full if rng.random() < 0.5 else rng.randrange(1, 401)
        c, _ = MC.random_pair(rng, full, vals)
        if n <= full:
            c.signatures = c.signatures[:n]
        else:  # more signatures than validators: the extra ones match nothing
            c.signatures += [T.CommitSig(2, MC.validator("extra", i, 1).address, MC.t_plus(-40), b"") for i in range(n - full)]
        pairs.append((c, vals))
    for at in (100, 250):
        pairs.insert(at, MC.random_pair(rng, MAX_VOTES, sets[2]))
    pm = check(engine, pairs)
    dev = pm.on_device()
    assert 100 < dev.sum() < 250 and dev[100] == 1 and dev[250] == 1
    batch = pm.results()
    for q in list(range(0, len(pairs), 7)) + [100, 250]:
        assert tmed.median_times(engine, [pairs[q]])[0] == batch[q], q


def test_after_a_submitted_blocksync_window_gpu(engine):
    """A blocksync window is submitted, then tmed_median_times runs (it collects the window first),
    then blocksync_wait: the window's results are intact and the medians equal the restatement."""
    from commit_cases import oracle_result, pbid, same, to_product
    from oracle.fixtures import make_block_id, make_commit, make_valset, seed_of
    chain = "median-bs"
    vs, seeds = make_valset([seed_of("mbs", i) for i in range(8)], [10] * 8)
    bids, heights, ocommits, pcommits = [], [], [], []
    for b in range(3):
        bid = make_block_id("mbs%d" % b)
        cm = make_commit(vs, seeds, chain, 10 + b, 0, bid)
        if b == 1:
            s = bytearray(cm.signatures[0].signature)
            s[7] ^= 4
            cm.signatures[0].signature = bytes(s)
        pv, pc = to_product(vs, cm)
        bids.append(bid)
        heights.append(10 + b)
        ocommits.append(cm)
        pcommits.append(pc)
    w = T.BlocksyncWindow(pv, chain, [pbid(b) for b in bids], heights, pcommits)
    w.submit(engine, 1)
    # the window's own commits against its own set, as validateBlock pairs them
    pairs = [(pc, pv) for pc in pcommits]
    check(engine, pairs, want=[MC.expected(c, v) for c, v in pairs], device=[True] * 3)
    T.blocksync_wait(engine)
    for b in range(3):
        assert same(w.errors()[b], oracle_result(1, vs, chain, bids[b], heights[b], ocommits[b], 0, 0)), b
    assert list(w.codes()) == [0, 4, 0]
