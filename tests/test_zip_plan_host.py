"""The bisection plan of the ZIP-215 batch mode without a device (csrc/zip_plan.h, the group
bookkeeping of zip215_verify_device): which groups of a chunk run a batch equation, which are
decided signature by signature.  tests/native/zip_plan_host.cpp drives the header with a callback
that knows the failing indices, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer; a direct Python restatement of the rule gives the expected equation
counts and singly decided groups.  With the minimum group size scaled down to 2: every chunk size
from 1 to 64 with every set of at most 3 failing indices, and random larger sets.  The device side
(the equations themselves, the stats of real calls) is tests/test_gpu_zip215.py."""
import bisect
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tendermint-fork_amd", "csrc")
MIN_GROUP = 2


def plan(n, fails, min_group):
    """The rule, restated: level by level from the whole chunk, one equation per group; a failing
    group is halved while at most half of its level's groups fail (a level of one group always
    counts as sparse) and it holds at least two minimum groups; else it is decided singly.
    -> (equations [(level, lo, cnt, ok)], singly decided groups [(lo, cnt)])."""
    level, eqs, single, depth = [(0, n)], [], [], 0
    while level:
        failed = []
        for lo, cnt in level:
            i = bisect.bisect_left(fails, lo)  # fails is sorted: the first failing index >= lo
            ok = not (i < len(fails) and fails[i] < lo + cnt)
            eqs.append((depth, lo, cnt, ok))
            if not ok:
                failed.append((lo, cnt))
        dense = len(level) >= 2 and 2 * len(failed) > len(level)
        level = []
        for lo, cnt in failed:
            if not dense and cnt >= 2 * min_group:
                level += [(lo, cnt // 2), (lo + cnt // 2, cnt - cnt // 2)]
            else:
                single.append((lo, cnt))
        depth += 1
    return eqs, single


def check_trace(n, fails, eqs, single, min_group):
    """The properties of one plan (asserted on the program's own trace)."""
    assert eqs[0] == (0, 0, n, not fails)
    if not fails:
        assert len(eqs) == 1 and not single  # one equation, no single checks
    by_level = {}
    for lv, lo, cnt, ok in eqs:
        assert cnt >= 1 and 0 <= lo and lo + cnt <= n
        assert ok == (not any(lo <= f < lo + cnt for f in fails))
        by_level.setdefault(lv, []).append((lo, cnt, ok))
    assert sorted(by_level) == list(range(len(by_level)))
    for lv, groups in by_level.items():
        # the equations of one level are disjoint sub-ranges of the chunk
        spans = sorted((lo, lo + cnt) for lo, cnt, _ in groups)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (n, fails, lv)
        if lv == 0:
            continue
        # the two halves of a split tile their parent exactly
        assert len(groups) % 2 == 0
        parents = {(lo, cnt) for lo, cnt, ok in by_level[lv - 1] if not ok}
        for (alo, acnt, _), (blo, bcnt, _) in zip(groups[::2], groups[1::2]):
            assert alo + acnt == blo and (alo, acnt + bcnt) in parents and acnt == (acnt + bcnt) // 2
            assert min(acnt, bcnt) >= min_group
    # a failed equation is split or decided singly, never both, never neither
    for lv, lo, cnt, ok in eqs:
        if not ok:
            split = any(g[0] == lo and g[1] == cnt // 2 for g in by_level.get(lv + 1, []))
            assert split != ((lo, cnt) in single), (n, fails, lo, cnt)
    # every failing index lies in exactly one singly decided group; no index is covered twice
    cover = [0] * n
    for lo, cnt in single:
        assert (lo, cnt) in {(e[1], e[2]) for e in eqs if not e[3]}
        for x in range(lo, lo + cnt):
            cover[x] += 1
    assert max(cover) <= 1 and all(cover[f] == 1 for f in fails), (n, fails, single)


@pytest.fixture(scope="module")
def zip_plan_host(tmp_path_factory):
    """tests/native/zip_plan_host.cpp built with the sanitizers into a temporary directory."""
    exe = str(tmp_path_factory.mktemp("zip_plan") / "zip_plan_host")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "zip_plan_host.cpp"), "-o", exe])
    return exe


def _traces(exe, cases, tmp_path):
    """[(eqs, single)] of the program's trace mode for cases (n, min_group, fails)."""
    src = tmp_path / "cases.txt"
    src.write_text("".join("%d %d %d %s\n" % (n, mg, len(f), " ".join(map(str, f))) for n, mg, f in cases))
    out = subprocess.run([exe, "trace", str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = []
    for line in out.stdout.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "case":
            res.append(([], [], int(t[2]), int(t[3])))
        elif t[0] == "e":
            res[-1][0].append((int(t[1]), int(t[2]), int(t[3]), t[4] == "1"))
        else:
            res[-1][1].append((int(t[1]), int(t[2])))
    assert len(res) == len(cases)
    for eqs, single, n_eq, n_single in res:
        assert len(eqs) == n_eq and len(single) == n_single
    return [(r[0], r[1]) for r in res]


def test_every_small_chunk_with_up_to_three_failures(zip_plan_host):
    """N = 1..64, every set of at most 3 failing indices (722,864 plans): the program checks the
    properties of every trace itself (it exits non-zero otherwise); its equation count and singly
    decided groups equal the restatement's, case by case."""
    out = subprocess.run([zip_plan_host, "all", "64", "3", str(MIN_GROUP)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert lines.pop() == ""
    it = iter(lines)
    count = 0
    for n in range(1, 65):
        for k in range(0, min(3, n) + 1):
            for fails in itertools.combinations(range(n), k):
                eqs, single = plan(n, fails, MIN_GROUP)
                want = " ".join([str(len(eqs))] + ["%d:%d" % g for g in single])
                assert next(it) == want, (n, fails)
                count += 1
    assert next(it, None) is None and count == 722864


def test_traces_of_small_chunks(zip_plan_host, tmp_path):
    """The properties, asserted here on the program's full traces: N = 1..64 with every set of at
    most 2 failing indices, every set of 3 for N <= 20, and the traces equal the restatement's."""
    cases = [(n, MIN_GROUP, f) for n in range(1, 65) for k in range(0, 3) for f in itertools.combinations(range(n), k)]
    cases += [(n, MIN_GROUP, f) for n in range(3, 21) for f in itertools.combinations(range(n), 3)]
    for (n, mg, fails), (eqs, single) in zip(cases, _traces(zip_plan_host, cases, tmp_path)):
        check_trace(n, fails, eqs, single, mg)
        assert (eqs, single) == plan(n, fails, mg), (n, fails)


def test_random_larger_sets(zip_plan_host, tmp_path):
    """Random sets of 4 .. N failing indices, clustered and spread, N up to 700, minimum group sizes
    2, 3 and 16; and the product's own sizes: 2^14 as the minimum group, chunks at and around the
    first sizes that are split."""
    rng = random.Random(215)
    cases = []
    for _ in range(1500):
        n = rng.choice([rng.randrange(4, 65), rng.randrange(65, 700)])
        mg = rng.choice([2, 2, 3, 16])
        k = rng.choice([4, 5, 8, max(4, n // 3), n])
        if rng.random() < 0.5:  # clustered in a window of the chunk
            a = rng.randrange(n)
            pop = range(a, min(n, a + max(k, n // 8)))
        else:
            pop = range(n)
        cases.append((n, mg, tuple(sorted(rng.sample(pop, min(k, len(pop)))))))
    for n in (1, 16383, 32767, 32768, 32769, 65536, 70000, 1 << 20):
        for fails in ((), (0,), (n - 1,), (n // 2 - 1,), (n // 2,), (0, n - 1), (1234 % n, n // 2, n - 1)):
            cases.append((n, 1 << 14, tuple(sorted(set(f for f in fails if f >= 0)))))
    big = 0
    for (n, mg, fails), (eqs, single) in zip(cases, _traces(zip_plan_host, cases, tmp_path)):
        if n <= 700:
            check_trace(n, fails, eqs, single, mg)
        assert (eqs, single) == plan(n, fails, mg), (n, fails)
        big += len(eqs) > 7
    assert big >= 100
    # what tests/test_gpu_zip215.py sees of the product: one failure in 70,000 takes 5 equations and
    # 17,500 single checks; a chunk below 2^15 is never split; one failure in 2^20 takes 13 equations
    assert [len(plan(70000, (52345,), 1 << 14)[0]), plan(70000, (52345,), 1 << 14)[1]] == [5, [(35000, 17500)]]
    assert plan(32767, (5,), 1 << 14) == ([(0, 0, 32767, False)], [(0, 32767)])
    assert len(plan(1 << 20, (77,), 1 << 14)[0]) == 13
