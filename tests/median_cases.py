"""state.MedianTime restated in Python, and the cases the host function and the kernels are checked
on (tests/test_median_host.py, tests/test_gpu_median.py).

`median_time` + `weighted_median` follow the reference line by line (state/state.go:268-285,
types/time/time.go:35-58, types/validator_set.go:270-278): the linear GetByAddress, nil slots for
the signatures that do not enter, the sort by UnixNano, the `median <= weight` walk.  `expected`
adds what include/tmed25519.h sets on top: the inputs on which Go's int64 arithmetic would decide
(GO_PATH) and the code for "nothing entered".  `reference` is the same value through a dict lookup,
for the commits of 10,000 signatures where the linear scan is too slow in Python; the CPU suite
shows it equal to the restatement on the whole corpus.
"""
import hashlib
import json
import os
import random

import tmed.types as T
from tmed.state import MEDIAN_GO_PATH, MEDIAN_OK, MEDIAN_ZERO_TIME

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NANOS = 10 ** 9
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T1 = (1700000000, 123456789)
MIN_TIME = (-9223372037, 145224192)   # UnixNano == INT64_MIN
MAX_TIME = (9223372036, 854775807)    # UnixNano == INT64_MAX
SIZES = (0, 1, 2, 3, 8, 63, 64, 65, 175)


def unix_nano(t):
    return t[0] * NANOS + t[1]


# ----------------------------------------------------------------------------- the restatement

def get_by_address(vals, address):
    """ValidatorSet.GetByAddress (types/validator_set.go:270-278): the first match of a linear scan."""
    for idx, val in enumerate(vals.validators):
        if val.address == address:  # bytes.Equal
            return idx, val
    return -1, None


def weighted_median(weighted_times, total_voting_power, tie=None):
    """tmtime.WeightedMedian (types/time/time.go:35-58).  weighted_times: (time, weight) or None per
    slot.  sort.Slice is not stable: `tie` (a random.Random) orders equal keys at random."""
    median = abs(total_voting_power) // 2 * (1 if total_voting_power >= 0 else -1)  # Go's int64 division
    def less_key(wt):  # nil slots last, then by UnixNano (time.go:38-46)
        return (1, 0, 0) if wt is None else (0, unix_nano(wt[0]), tie.random() if tie else 0)
    res = T.ZERO_TIME
    for wt in sorted(weighted_times, key=less_key):
        if wt is not None:
            if median <= wt[1]:
                res = wt[0]
                break
            median -= wt[1]
    return res


def entering(commit, vals, lookup=get_by_address):
    """The slots MedianTime builds (state.go:269-283) and the total it sums."""
    sigs = commit.signatures
    weighted = [None] * len(sigs)
    total = 0
    for i in range(len(sigs)):
        cs = sigs[i]
        if cs.flag == T.FLAG_ABSENT:  # commitSig.Absent()
            continue
        _, val = lookup(vals, cs.address)
        if val is not None:
            total += val.voting_power
            weighted[i] = (cs.timestamp, val.voting_power)
    return weighted, total


def median_time(commit, vals, tie=None):
    weighted, total = entering(commit, vals)
    return weighted_median(weighted, total, tie)


def _outcome(weighted, tie=None):
    """(code, time) of include/tmed25519.h for the slots of one pair."""
    got = [wt for wt in weighted if wt is not None]
    total = 0
    for (t, w) in got:
        total += w
        if not (0 <= t[1] < NANOS) or not (INT64_MIN <= unix_nano(t) <= INT64_MAX) or w < 0 or total > INT64_MAX:
            return MEDIAN_GO_PATH, None
    if not got:
        return MEDIAN_ZERO_TIME, T.ZERO_TIME
    return MEDIAN_OK, weighted_median(weighted, total, tie)


def expected(commit, vals, tie=None):
    return _outcome(entering(commit, vals)[0], tie)


def reference(commit, vals):
    """`expected` with GetByAddress as a dict of first matches (large commits)."""
    first = {}
    for val in vals.validators:
        first.setdefault(val.address, val)
    return _outcome(entering(commit, vals, lambda _, a: (0, first.get(a)))[0])


def fast_path(commit, vals):
    """The pairs the kernels take (include/tmed25519.h): equal sizes, every non-absent signature's
    20-byte address equal to the set's address at the same index, and no address twice in the set."""
    sigs = commit.signatures
    if len(sigs) != len(vals.validators) or len({v.address for v in vals.validators}) != len(vals.validators):
        return False
    return all(sigs[i].flag == T.FLAG_ABSENT or sigs[i].address == vals.validators[i].address
               for i in range(len(sigs)))


def same(got, want):
    """A call's (code, time) against `expected`'s: the time of a GO_PATH outcome is not compared."""
    return got[0] == want[0] and (want[0] == MEDIAN_GO_PATH or tuple(got[1]) == tuple(want[1]))


# ----------------------------------------------------------------------------- building pairs

_VALS = {}


def validator(tag, i, power):
    return T.Validator(hashlib.sha256(b"median-%s-%d" % (tag.encode(), i)).digest(), power)


def valset(n, powers=None, tag="v"):
    """n validators with distinct keys; the same objects for the same (n, powers, tag)."""
    key = (n, None if powers is None else tuple(powers), tag)
    if key not in _VALS:
        powers = [1 + (i * 7919) % 100 for i in range(n)] if powers is None else powers
        _VALS[key] = T.ValidatorSet([validator(tag, i, powers[i]) for i in range(n)])
    return _VALS[key]


def commit_for(vals, times, flags=None):
    """The aligned commit: signature i is validator i's, flag 2 unless given."""
    n = len(vals.validators)
    flags = [T.FLAG_COMMIT] * n if flags is None else flags
    return T.Commit(1, 0, T.BlockID(), [T.CommitSig(flags[i], vals.validators[i].address, tuple(times[i]), b"")
                                        for i in range(n)])


def t_plus(seconds, nanos=0, base=T1):
    s, ns = divmod(unix_nano(base) + seconds * NANOS + nanos, NANOS)
    return (s, ns)


def random_pair(rng, n, vals=None, flag_kinds=(1, 2, 3, 0, 7)):
    vals = valset(n) if vals is None else vals
    times = [t_plus(rng.randrange(-30, 30), rng.randrange(NANOS)) for _ in range(n)]
    flags = [rng.choice(flag_kinds) for _ in range(n)]
    return commit_for(vals, times, flags), vals


def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "weighted_median_cases.json")) as f:
        g = json.load(f)
    t1 = tuple(g["t1"])
    return t1, g["cases"]


def golden_pair(case, t1):
    """A pinned case as a commit: slot i is signature i of validator i, a nil slot an absent signature."""
    slots = case["slots"]
    vals = valset(len(slots), [5 if s is None else s[1] for s in slots], "golden-" + case["name"])
    times = [t1 if s is None else t_plus(s[0], 0, t1) for s in slots]
    flags = [T.FLAG_ABSENT if s is None else T.FLAG_COMMIT for s in slots]
    return commit_for(vals, times, flags), vals


def corpus():
    """[(name, commit, vals)]: every kind of input the rule distinguishes, at sizes from SIZES."""
    rng = random.Random(20240607)
    out = []
    add = lambda name, commit, vals: out.append((name, commit, vals))
    for n in SIZES:  # flags of all four kinds, random powers and times
        for k in range(3):
            add("random n=%d #%d" % (n, k), *random_pair(rng, n))
    t1, cases = golden_cases()
    for case in cases:
        add("pinned " + case["name"], *golden_pair(case, t1))
    three = [t_plus(0), t_plus(5), t_plus(10)]
    add("odd total", commit_for(valset(3, [1, 1, 1]), three), valset(3, [1, 1, 1]))
    add("even total", commit_for(valset(3, [1, 1, 2]), three), valset(3, [1, 1, 2]))
    add("total 1", commit_for(valset(3, [0, 1, 0]), three[::-1]), valset(3, [0, 1, 0]))
    add("total 1, the weight on the smallest key", commit_for(valset(3, [1, 0, 0]), three), valset(3, [1, 0, 0]))
    z8 = valset(8, [0] * 8)
    add("total 0", commit_for(z8, [t_plus(8 - i, i) for i in range(8)]), z8)
    add("crossing on cumsum == median", commit_for(valset(3, [5, 5, 10]), three), valset(3, [5, 5, 10]))
    add("crossing one past the median", commit_for(valset(3, [5, 6, 10]), three), valset(3, [5, 6, 10]))
    add("crossing one short of the median", commit_for(valset(3, [5, 4, 10]), three), valset(3, [5, 4, 10]))
    add("zero weights before the crossing",
        commit_for(valset(8, [0, 0, 3, 0, 4, 0, 0, 1]), [t_plus(i) for i in range(8)]), valset(8, [0, 0, 3, 0, 4, 0, 0, 1]))
    for n in (1, 64, 175):
        add("all timestamps equal n=%d" % n, commit_for(valset(n), [T1] * n), valset(n))
    add("equal keys in groups", commit_for(valset(63), [t_plus(i % 4) for i in range(63)]), valset(63))
    add("before 1970", commit_for(valset(8), [(-5 - i, 999999999 - i) for i in range(8)]), valset(8))
    add("either side of 1970", commit_for(valset(3), [(-1, 999999999), (0, 0), (0, 1)]), valset(3))
    add("keys differ in nanos only", commit_for(valset(65), [(T1[0], 65 - i) for i in range(65)]), valset(65))
    add("keys differ in seconds only", commit_for(valset(65), [(T1[0] + (i * 37) % 65, 5) for i in range(65)]), valset(65))
    add("smallest and largest UnixNano", commit_for(valset(2, [1, 1]), [MAX_TIME, MIN_TIME]), valset(2, [1, 1]))
    add("smallest, largest and one between", commit_for(valset(3, [1, 1, 1]), [MAX_TIME, T1, MIN_TIME]), valset(3, [1, 1, 1]))
    add("only the largest UnixNano", commit_for(valset(1, [3]), [MAX_TIME]), valset(1, [3]))
    add("go path: the zero time as a timestamp (its UnixNano is no int64)", commit_for(valset(2, [1, 4]), [T.ZERO_TIME, T1]), valset(2, [1, 4]))
    # GO_PATH: each condition on an entering signature, and the same values where they do not enter
    for name, t in (("UnixNano below int64", (MIN_TIME[0], MIN_TIME[1] - 1)), ("UnixNano above int64", (MAX_TIME[0], MAX_TIME[1] + 1)),
                    ("seconds far below", (INT64_MIN, 0)), ("seconds far above", (INT64_MAX, 0)),
                    ("seconds that wrap back into range", ((1 << 64) // NANOS + 1, 0)),
                    ("negative nanos", (T1[0], -1)), ("nanos of a whole second", (T1[0], NANOS)), ("nanos int32 min", (T1[0], -(1 << 31)))):
        times = [t_plus(i) for i in range(8)]
        times[5] = t
        add("go path: " + name, commit_for(valset(8), times), valset(8))
        add("absent: " + name, commit_for(valset(8), times, [2] * 5 + [1, 2, 2]), valset(8))
    neg = valset(3, [4, -1, 4])
    add("go path: negative weight", commit_for(neg, three), neg)
    add("absent: negative weight", commit_for(neg, three, [2, 1, 2]), neg)
    big = valset(3, [1 << 62, 1, 1 << 62])
    add("go path: total past int64", commit_for(big, three), big)
    add("total of exactly int64 max", commit_for(valset(3, [1 << 62, (1 << 62) - 1, 0]), three), valset(3, [1 << 62, (1 << 62) - 1, 0]))
    add("absent: total past int64", commit_for(big, three, [2, 2, 1]), big)
    for n in (63, 64, 65, 175):  # the overflow where the sum crosses lanes and wavefronts
        many = valset(n, [INT64_MAX // n + 1] * n)
        add("go path: total past int64 n=%d" % n, commit_for(many, [t_plus(i) for i in range(n)]), many)
    # addresses
    v8 = valset(8)
    c = commit_for(v8, [t_plus(i) for i in range(8)])
    c.signatures[3].address = validator("stranger", 0, 1).address
    add("address not in the set", c, v8)
    c = commit_for(v8, [t_plus(8 - i) for i in range(8)])
    c.signatures[3].address = v8.validators[2].address
    add("address twice in the commit", c, v8)
    for length in (0, 19):
        c = commit_for(v8, [t_plus(i) for i in range(8)])
        c.signatures[6].address = c.signatures[6].address[:length]
        add("address of length %d" % length, c, v8)
        c = commit_for(v8, [t_plus(i) for i in range(8)], [2] * 6 + [1, 2])
        c.signatures[6].address = c.signatures[6].address[:length]
        add("absent with an address of length %d" % length, c, v8)
    add("more signatures than validators", commit_for(v8, [t_plus(i) for i in range(8)]), valset(3, tag="v"))
    add("fewer signatures than validators", commit_for(valset(3), three), v8)
    v65 = valset(65)
    c = commit_for(v65, [t_plus(i % 7, i) for i in range(65)])
    c.signatures = c.signatures[1:] + c.signatures[:1]
    add("rotated by one", c, v65)
    for n in (1, 8, 64, 175):
        add("all absent n=%d" % n, commit_for(valset(n), [T1] * n, [1] * n), valset(n))
    c = commit_for(v8, [T1] * 8)
    for i, cs in enumerate(c.signatures):
        cs.address = validator("stranger", i, 1).address
    add("no address in the set", c, v8)
    twins = T.ValidatorSet([validator("twin", i if i != 4 else 1, p) for i, p in enumerate([3, 50, 3, 3, 1, 3, 3, 3])])
    add("address twice in the set", commit_for(twins, [t_plus(i) for i in range(8)]), twins)
    add("unknown flags enter", commit_for(v8, [t_plus(i) for i in range(8)], [0, 7, 255, 4, 3, 2, 1, 128]), v8)
    return out
