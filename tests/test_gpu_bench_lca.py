"""bench_commits.py --config lca as a command, at a reduced shape."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_lca_cli_at_a_reduced_shape():
    """Both routes agree before anything is timed, and the result line carries the figures of both routes and
    the two kernels' times."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench_commits.py"), "--config", "lca", "--lca-shapes",
                        "1x130,5x33", "--reps", "2"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert r["config"] == "lca" and r["runs"] == 2
    assert [s["shape"] for s in r["shapes"]] == ["1x130", "5x33"]
    for s in r["shapes"]:
        assert s["routes_agree"] is True and s["signatures"] in (130, 165)
        for k in ("new_ms", "old_ms", "new_evidences_per_s", "old_evidences_per_s", "lookup_kernel_ms", "rank_kernel_ms",
                  "old_verify_commits_ms", "old_header_hashes_ms", "old_byzantine_host_ms", "speedup"):
            assert s[k] is not None and s[k] >= 0, k
