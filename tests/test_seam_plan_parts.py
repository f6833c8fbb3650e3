"""The commit seam's planner (csrc/seam_host.h seam_plan) hands on the same plan as before its
per-worker state became one record (PlanPart) and its regions three functions.

tests/native/seam_race.cpp prints `plan`, a digest of everything seam_plan hands on (every Plan with
the vof of its Trusting requests, the results of the requests it decided, the candidates' runs,
offsets, aliases, template sharing and part boundaries, the staging group, the template rows), and
`digest`, the requests' outcomes after the finish.  The constants below are the values of the PARENT
of the commit that introduced PlanPart: this same harness source compiled against that commit's
csrc (a `git worktree` of it), run plain and under ThreadSanitizer with the jitter below, which gave
the same values.  A change that moves the plan on purpose regenerates them the same way, from the tree
before it.  The harness draws from std::mt19937_64 directly (`rng()`, `rng() % n`; no
std::*_distribution), so the values do not depend on the standard library.

Shapes (KIND:HEADERS:VALIDATORS, see the harness) and what they reach, at 1, 5 and 8 host threads:
  pairs:600:48     aliases, group segments, rows built in the merge, the part-wise finish
  pairs:1:40000    2 requests, under 1,024 but 80,000 signatures: workers by signature count, two parts
                   run, the pair split across them: pairing on (a Trusting request) with zero aliases
  pairs:3:12000    6 requests: at 8 threads six parts run with one request each (no alias), at 5
                   threads the last part holds requests 4 and 5 (one pair's aliases)
  light:1200:48    no Trusting request: no pairing, rows built in the merge
  decided:600:48   the first 160 requests decided before any candidate: at 8 threads part 0
                   (requests 0..149) has no run, no alias, no segment and no row
  all of them one after another, then pairs:600:48 again, on one Plans / Cands / Group / Templates
`parts` is what the plan publishes for the part-wise finish (Cands::preq): the worker count when the
batch has aliases and several workers, else 0.  About 2 % of the stand-in verifier's bits are false,
so the 48-validator shapes accept some commits and reject others; a commit of 12,000 or 40,000
signatures never verifies whole at that rate, so those shapes' requests all end rejected (accepted 0)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tendermint-fork_amd", "csrc")
NATIVE = os.path.join(HERE, "native")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")

ALL = "pairs:600:48,pairs:1:40000,pairs:3:12000,light:1200:48,decided:600:48,pairs:600:48"
JITTER = {1: "0", 5: "50", 8: "200"}

# (shape, threads) -> (plan, digest) of the parent; the outcome digest does not depend on the threads
PARENT = {
    ("pairs:600:48", 1): ("75890e95f06a91de", "5ab0cbcf85c0714b"),
    ("pairs:600:48", 5): ("ff56261fdbbb228f", "5ab0cbcf85c0714b"),
    ("pairs:600:48", 8): ("7866c96afc31e11a", "5ab0cbcf85c0714b"),
    ("pairs:1:40000", 1): ("49f30e546f926b81", "8907503e938e7915"),
    ("pairs:1:40000", 5): ("c341488699de7288", "8907503e938e7915"),
    ("pairs:1:40000", 8): ("c341488699de7288", "8907503e938e7915"),
    ("pairs:3:12000", 1): ("2fdf028a784d716b", "fabc2d53324be21b"),
    ("pairs:3:12000", 5): ("abd77824b768b240", "fabc2d53324be21b"),
    ("pairs:3:12000", 8): ("7d2a0729880c10ce", "fabc2d53324be21b"),
    ("light:1200:48", 1): ("a90d4615b0f8d865", "fd8bccd02192e297"),
    ("light:1200:48", 5): ("d4aa6973d4bffcb3", "fd8bccd02192e297"),
    ("light:1200:48", 8): ("d4aa6973d4bffcb3", "fd8bccd02192e297"),
    ("decided:600:48", 1): ("7ad1184ab8b55d59", "e9e55a4b0b7ed003"),
    ("decided:600:48", 5): ("dbba90e571e60f81", "e9e55a4b0b7ed003"),
    ("decided:600:48", 8): ("02b30fae4c18730f", "e9e55a4b0b7ed003"),
    (ALL, 1): ("f022edb5579fcc3f", "618806a93ef42173"),
    (ALL, 5): ("70f0352a614c65ce", "618806a93ef42173"),
    (ALL, 8): ("aa06ed4c56663c3a", "618806a93ef42173"),
}


def _aliased(shape, threads):
    """Whether the shape has aliases at this worker count: a Trusting request and its Light partner
    in one part."""
    kind, headers, _ = shape.split(":")
    if kind == "light":
        return False
    if headers == "1":
        return threads == 1  # two requests, two parts
    if headers == "3":
        return threads != 8  # 8 threads: six parts of one request; 5: the last part holds two
    return True


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("seam_plan_parts")
    exes = {}
    for name, flags in (("plain", []), ("tsan", ["-fsanitize=thread"])):
        exes[name] = str(d / ("seam_race_" + name))
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-I", CSRC, os.path.join(NATIVE, "seam_race.cpp"),
                        "-x", "c++", os.path.join(CSRC, "signbytes.hip"), "-o", exes[name], "-lpthread"],
                       check=True, capture_output=True, timeout=300)
    return exes


@pytest.mark.parametrize("threads", [1, 5, 8])
@pytest.mark.parametrize("shape", ["pairs:600:48", "pairs:1:40000", "pairs:3:12000", "light:1200:48",
                                   "decided:600:48", ALL])
def test_plan_equals_parent(harness, shape, threads):
    for build in ("plain", "tsan"):
        env = dict(os.environ, TMED_HOST_THREADS=str(threads), TSAN_OPTIONS="halt_on_error=1")
        jitter = JITTER[threads] if build == "tsan" else "0"
        r = subprocess.run([harness[build], "0", "0", "3", jitter, "7", "1", shape], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        print(build, r.stdout)
        lines = r.stdout.strip().split("\n")
        parts_of = shape.split(",")
        assert len(lines) == len(parts_of), r.stdout
        for line, one in zip(lines, parts_of):
            w = line.split()
            f = {k: int(w[w.index(k) + 1]) for k in ("requests", "candidates", "aliases", "parts", "accepted")}
            kind, headers, validators = one.split(":")
            assert f["requests"] == int(headers) * (1 if kind == "light" else 2), line
            assert f["candidates"] > 0, line
            assert (f["aliases"] > 0) == _aliased(one, threads), line
            assert f["parts"] == (threads if _aliased(one, threads) and threads > 1 else 0), line
            if validators == "48":  # (the docstring: larger commits never verify whole)
                assert 0 < f["accepted"] < f["requests"], line
        w = lines[-1].split()
        assert (w[w.index("plan") + 1], w[w.index("digest") + 1]) == PARENT[(shape, threads)], (build, r.stdout)
