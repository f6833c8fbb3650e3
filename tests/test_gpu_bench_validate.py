"""bench_commits.py --config vb as a command, at a tiny shape."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_vb_cli_at_a_tiny_shape():
    """8 linked blocks x 16 validators: the command runs, the fused call and the composed route decide every
    block alike, and the result line carries its fields."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench_commits.py"), "--config", "vb", "--vb-shapes", "8x16",
                        "--runs", "2"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert r["config"] == "vb" and r["runs"] == 2 and len(r["shapes"]) == 1
    s = r["shapes"][0]
    assert (s["blocks"], s["validators"]) == (8, 16)
    assert s["outcome_mismatches"] == 0 and s["all_ok"] is True
    assert (s["sets_hashed"], s["sets_staged"], s["blocks_checked"]) == (1, 1, 8)
    assert s["signatures_verified"] == 8 * 16
    assert len(s["fused_call_ms_runs"]) == 2 and len(s["composed_route_ms_runs"]) == 2
    assert len(s["composed_seven_calls_ms_runs"]) == 2 and len(s["composed_host_ms_runs"]) == 2
    for k in ("fused_call_ms", "composed_route_ms", "composed_seven_calls_ms", "composed_host_ms", "fused_blocks_per_s", "composed_blocks_per_s", "block_check_kernel_ms"):
        assert s[k] is not None and s[k] > 0, k
