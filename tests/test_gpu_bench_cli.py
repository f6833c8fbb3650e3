"""bench.py as a command: a plain run times exactly --steps steps, measures no other leg and, with
--dump-outputs, leaves the decisions of its last timed step on disk.  One child process, on a small
batch (the kernels have their own tests) whose size is no multiple of a block, with the C5 mix so
that the decisions are not all alike; they are checked against the C port on the same inputs,
rebuilt here from the seeded workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N = 4099
FULL_ONLY = ("roofline", "cpu_baseline", "cpu_baseline_all_cores", "c2_keyset_variant", "c1_verifycommit_p50",
             "c5", "zip215_batch_mode", "c4_shard", "c3_light_client")


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_decisions(tmp_path):
    from oracle import port
    from tmed.workload import c2_messages, c2_seeds, c5_mix
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--sigs", str(N), "--mix", "c5", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["checked"] == N
    assert r["metric"] == "ed25519 verifies/sec at 1/8 MI355X" and r["unit"] == "verifies/s" and r["higher_is_better"]
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(N / (r["ms_per_step"] * 1e-3), rel=1e-2)
    assert all(r[k] is None for k in FULL_ONLY), [k for k in FULL_ONLY if r[k] is not None]
    assert os.listdir(out) == ["decisions.npy"]
    dec = np.load(out / "decisions.npy")
    assert dec.dtype == np.float32 and dec.shape == (N,)

    seeds = c2_seeds(0, N)
    msgs, offs = c2_messages(0, N)
    o = offs.astype(np.uint64)
    nt = min(16, os.cpu_count() or 1)
    sigs, pubs = port.sign_batch(seeds, msgs, o, nt)
    c5_mix(pubs, sigs, seed=0x5EED)
    exp = port.verify_batch(pubs, sigs, msgs, o, nt)
    assert 0 < exp.sum() < N
    assert (dec == exp).all(), int((dec != exp).sum())
    assert r["valid"] == int(exp.sum()) and not r["all_valid"]
