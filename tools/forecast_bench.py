#!/usr/bin/env python
"""Cost of the forecast roll-out (GPMDM_PF.forecast, csrc/forecast.h) beside the two existing
calls it chains: predict() and the filtered-pose read-out.

On one GPU, for the config-2 model of gpmdm_amd.synthetic (N = 2000, D = 62, d = 3, C = 2) at
P = 100k and the config-1 (notebook) model (N = 500) at P = 100, Philox, after 5 warm-up frames,
event-times in one run
  * forecast(H) for H in {1, 8, 32}, with and without the pose read-out (gpmdm_pf_forecast with
    class_prob / state_mean [/ obs_mean / obs_spread] outputs: the roll-out's launches and the
    copy-back of the H result rows);
  * gpmdm_pf_predict (class grouping, the dynamics-GP tiles, the mean) and gpmdm_pf_observation
    with no host outputs (the read-out's kernels alone).
The per-step cost is (t(32) - t(8)) / 24; the yardstick is predict + read-out (with the pose)
or predict alone (without), and the target per-step cost <= 1.25 x the yardstick: the margin is
for the three O(P) roll-out kernels and their launch gaps beside the O(P N) tiles.
Writes profiles/forecast/README.txt with the commit hash and one JSON line per configuration.

    python tools/forecast_bench.py [--out profiles/forecast]
"""
import argparse
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from gpmdm_amd import GPMDM, GPMDM_PF, _lib, synthetic  # noqa: E402

HORIZONS = (1, 8, 32)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        f = ROOT / "COMMIT"
        return f.read_text().strip() if f.exists() else "unrecorded"


def build_model(c, device):
    data = synthetic.make_sequences(c["C"], c["S"], c["L"], c["D"], c["d"], seed=0)
    hp = synthetic.default_hyperparameters(c["D"], c["d"], 0.1)
    m = GPMDM(D=c["D"], d=c["d"], n_classes=c["C"], dyn_target="full", dyn_back_step=1, device=device, **hp)
    for k in range(c["C"]):
        for y in data.sequences[k]:
            m.add_data(y, k)
    m.init_X()
    return m, data


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def run(cfg, P, calls):
    c = synthetic.CONFIGS[cfg]
    dev = torch.device("cuda:0")
    m, data = build_model(c, dev)
    C, D, d = c["C"], c["D"], c["d"]
    T = torch.from_numpy(synthetic.markov_matrix(C))
    zs = data.observation_stream(5, seed=1)
    torch.manual_seed(0)
    pf = GPMDM_PF(m, T, P, rng="philox", seed=11)
    for k in range(5):
        pf.update(zs[k])
    lib, h = _lib.load(), pf._h
    Hmax = max(HORIZONS)
    bufs = [np.zeros((Hmax, n)) for n in (C, d, D, D)]
    with_pose = _lib.ForecastOut(*(_lib.dptr(b) for b in bufs))
    without = _lib.ForecastOut(_lib.dptr(bufs[0]), _lib.dptr(bufs[1]))
    pred = np.zeros(d)

    def forecast(H, out):
        _lib.check(lib.gpmdm_pf_forecast(h, H, _lib.GPMDM_FORECAST_SAMPLE, None, ctypes.byref(out), pf._stream()),
                   "forecast")

    def predict():
        _lib.check(lib.gpmdm_pf_predict(h, _lib.dptr(pred), pf._stream()), "predict")

    def readout():
        _lib.check(lib.gpmdm_pf_observation(h, None, None, pf._stream()), "read-out")

    for fn in (predict, readout, lambda: forecast(Hmax, with_pose)):   # buffers allocated, kernels loaded
        fn()
    r = {"config": cfg, "N": C * c["S"] * c["L"], "D": D, "d": d, "C": C, "P": P, "rng": "philox",
         "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "calls": calls,
         "predict_ms": event_ms(predict, calls), "readout_ms": event_ms(readout, calls)}
    for name, out in (("pose", with_pose), ("no_pose", without)):
        for H in HORIZONS:
            r[f"forecast_{name}_H{H}_ms"] = event_ms(lambda: forecast(H, out), max(calls // H, 3))
        r[f"step_{name}_ms"] = (r[f"forecast_{name}_H32_ms"] - r[f"forecast_{name}_H8_ms"]) / 24
    r["yardstick_pose_ms"] = r["predict_ms"] + r["readout_ms"]
    r["yardstick_no_pose_ms"] = r["predict_ms"]
    r["step_pose_over_yardstick"] = r["step_pose_ms"] / r["yardstick_pose_ms"]
    r["step_no_pose_over_yardstick"] = r["step_no_pose_ms"] / r["yardstick_no_pose_ms"]
    r["target_1p25_met"] = bool(r["step_pose_over_yardstick"] <= 1.25)
    return r


def table(rs):
    lines = ["Forecast roll-out against predict() + the pose read-out (tools/forecast_bench.py), event times in ms",
             f"commit {rs[0]['commit']}  device {rs[0]['device']}", ""]
    for r in rs:
        lines += [f"config {r['config']}: N={r['N']} D={r['D']} d={r['d']} C={r['C']} P={r['P']} ({r['calls']} calls)",
                  f"  predict launches            {r['predict_ms']:.4f}",
                  f"  read-out launches           {r['readout_ms']:.4f}"]
        for name, label in (("pose", "with the pose read-out"), ("no_pose", "without")):
            lines.append(f"  forecast(H), {label}: " + "  ".join(
                f"H={H} {r[f'forecast_{name}_H{H}_ms']:.4f}" for H in HORIZONS))
            lines.append(f"    per step (t(32) - t(8)) / 24 = {r[f'step_{name}_ms']:.4f}"
                         f"  = {r[f'step_{name}_over_yardstick']:.3f} x the yardstick"
                         f" {r[f'yardstick_{name}_ms']:.4f}")
        lines.append(f"  target (per step with the pose <= 1.25 x (predict + read-out)): "
                     f"{'met' if r['target_1p25_met'] else 'NOT met'}")
        lines.append("")
    lines += ["JSON:"] + [json.dumps(r) for r in rs]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "forecast"))
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    rs = [run(2, 100_000, a.calls), run(1, 100, a.calls)]
    for r in rs:
        if a.commit:
            r["commit"] = a.commit
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    text = table(rs)
    (out / "README.txt").write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
