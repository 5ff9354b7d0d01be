"""bench.py's plain run on the GPU: the line holds the contract fields and none of --full's
measurements, --steps sets the timed frames, and --dump-outputs writes the last timed step's
read-outs, the same arrays in every run with the same arguments (the notebook-size
configuration: N = 500, P = 100, a few frames)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = {"most_likely_class": (1,), "class_probabilities": (2,), "current_state_mean": (3,)}
FULL_ONLY = ("stages_ms_per_step", "nodedup", "ess_last", "dyn_rows_last", "replay", "bank", "spread", "cutoff",
             "cpu_baseline", "ms_per_frame_without_timing_events")


def _start(out):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.Popen([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--config", "1", "--steps", "4",
                             "--warmup", "2", "--dump-outputs", str(out)],
                            cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(proc, out):
    stdout, stderr = proc.communicate(timeout=170)
    assert proc.returncode == 0, stderr[-2000:]
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, stdout[:2000]
    return json.loads(lines[0]), {n: np.load(out / f"{n}.npy") for n in NAMES}


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    procs = [_start(tmp_path / t) for t in "ab"]       # two runs with the same arguments, side by side
    try:
        rec, a = _finish(procs[0], tmp_path / "a")
        rec_b, b = _finish(procs[1], tmp_path / "b")
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rec["steps"] == 4 and rec["warmup"] == 2 and rec["full"] is False
    assert rec["unit"] == "particle-steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["ms_per_step"] > 0
    # value is particles x timed steps / the timed region, ms_per_step the same region per step
    assert rec["value"] == pytest.approx(rec["config"]["P_total"] * 1e3 / rec["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in rec]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{n}.npy" for n in NAMES)
    for n, shape in NAMES.items():
        assert a[n].dtype == np.float64 and a[n].shape == shape and np.all(np.isfinite(a[n])), n
    assert np.array_equal(a["class_probabilities"], np.asarray(rec["posterior_last"]))
    assert a["most_likely_class"][0] == np.argmax(a["class_probabilities"])
    assert abs(a["class_probabilities"].sum() - 1.0) < 1e-12
    # the same arguments: the same inputs, so the same outputs bit for bit
    assert rec_b["posterior_last"] == rec["posterior_last"]
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
