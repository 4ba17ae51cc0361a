"""bench.py ``--dump-outputs``: a plain single-process run (CPU rehearsal) writes the outputs of
its last timed step, the same arrays for the same arguments, and leaves the ``--full`` fields
of the result line empty."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    env = dict(os.environ, BENCH_DEVICE="cpu")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_are_the_last_steps_results_and_repeat(tmp_path):
    line, a = _run(tmp_path / "a", 3)
    _, b = _run(tmp_path / "b", 3)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "updates/s" and line["dtype"] == "fp32"
    assert line["reference_eager_same_gpu_updates_per_s"] is None and line["sync_ms"] is None
    assert sorted(a) == ["accuracy", "num_correct", "num_total"]
    assert a["accuracy"].dtype == np.float32
    assert a["num_correct"].dtype == np.float64 and a["num_total"].dtype == np.float64
    # --steps is the number of timed updates: the states count exactly 3 batches of 8192
    assert a["num_total"] == 3 * 8192
    assert 0 <= a["num_correct"] <= 0.01 * 3 * 8192  # random logits over 1000 classes
    assert a["accuracy"] == np.float32(a["num_correct"] / a["num_total"])
    for name in a:
        assert np.array_equal(a[name], b[name]), name
