#!/usr/bin/env python
"""Cost of forecasts and fixed-lag smoothing in a filter bank (GPMDM_PF_Bank.forecast, smoothed;
gpmdm_bank_forecast, gpmdm_bank_smoothed, csrc/forecast.h, csrc/smooth.h).

On one GPU, Philox, after 5 warm-up frames, three repeats of every figure (the median is
reported, all three are kept), for the notebook bank (config 1: N = 500, F = 39, Pf = 100) and
one large bank of config 2's model (N = 2000, F = 8, Pf = 12 500):
  * forecast: event times of bank.forecast(H) for H in {8, 32} with and without the pose, the
    per-step cost (t(32) - t(8)) / 24, beside the same forecast on the F single filters one after
    another (what the bank call replaces) and beside the bank's predict() + pose read-out;
  * frame: update + the read-outs at smoothing lag 0, 8 and 64 (host clock around frames that
    end in the read-out's wait);
  * read-out: smoothed() for every lag of the lag-64 bank, and one lag with the pose.
--frames-only measures the lag-0 frame alone, and --tree imports gpmdm_amd from another checkout
(one built from the parent commit) to do so: the yardstick for "the off path is unchanged".
Run the two trees in alternation.  Every run appends one JSON line per shape to <out>/runs.jsonl.

    python tools/bank_rollout_bench.py [--out DIR] [--frames-only] [--tree DIR --label parent]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
SHAPES = {"f39_p100_n500": (1, 39, 100, 1000), "f8_p12500_n2000": (2, 8, 12_500, 100)}   # config, F, Pf, frames per window
REPEATS, WARMUP, LAGS = 3, 5, (0, 8, 64)


def commit_hash(root):
    try:
        return subprocess.run(["git", "-C", str(root), "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        f = root / "COMMIT"
        return f.read_text().strip() if f.exists() else "unrecorded"


def build_model(pkg, c, device):
    synthetic = pkg.synthetic
    data = synthetic.make_sequences(c["C"], c["S"], c["L"], c["D"], c["d"], seed=0)
    hp = synthetic.default_hyperparameters(c["D"], c["d"], 0.1)
    m = pkg.GPMDM(D=c["D"], d=c["d"], n_classes=c["C"], dyn_target="full", dyn_back_step=1, device=device, **hp)
    for k in range(c["C"]):
        for y in data.sequences[k]:
            m.add_data(y, k)
    m.init_X()
    return m, data


def med(vals):
    return {"median": statistics.median(vals), "runs": vals}


def event_ms(fn, n):
    fn()                                            # buffers allocated, kernels loaded
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / n)
    return med(out)


def frame_ms(bank, Zs, frames):
    """ms per frame of update + the read-outs (the read-out's wait ends the frame)."""
    def frame(k):
        bank.update(Zs[k % len(Zs)])
        bank.class_probabilities()
    for k in range(WARMUP):
        frame(k)
    out, k0 = [], WARMUP
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(k0, k0 + frames):
            frame(k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / frames * 1e3)
        k0 += frames
    return med(out)


def run(pkg, name, parent_only):
    cfg, F, P, frames = SHAPES[name]
    synthetic = pkg.synthetic
    c = synthetic.CONFIGS[cfg]
    m, data = build_model(pkg, c, torch.device("cuda:0"))
    T = torch.from_numpy(synthetic.markov_matrix(c["C"]))
    zs = np.asarray(data.observation_stream(64 + F, seed=1), dtype=np.float64)
    Zs = [np.stack([zs[(k + f) % 64] for f in range(F)]) for k in range(64)]
    rec = {"shape": name, "config": cfg, "N": c["C"] * c["S"] * c["L"], "D": c["D"], "d": c["d"], "F": F, "P": P,
           "frames_per_window": frames, "repeats": REPEATS, "warmup_frames": WARMUP,
           "device": torch.cuda.get_device_name(0), "unit": "ms"}
    if parent_only:
        rec["frame_lag0"] = frame_ms(pkg.GPMDM_PF_Bank(m, T, F, P, seed=11), Zs, frames)
        return rec
    for L in LAGS:
        bank = pkg.GPMDM_PF_Bank(m, T, F, P, seed=11, smoothing_lag=L)
        rec[f"frame_lag{L}"] = frame_ms(bank, Zs, frames)
    for L in LAGS[1:]:
        rec[f"frame_lag{L}_over_lag0"] = rec[f"frame_lag{L}"]["median"] / rec["frame_lag0"]["median"]
    # the last bank: lag 64, its ring full
    for k in range(64):
        bank.update(Zs[k])
    calls = 20 if F * P <= 10_000 else 5
    rec["smoothed_all_lags"] = event_ms(lambda: bank.smoothed(), calls)
    rec["smoothed_all_lags_with_particles"] = event_ms(lambda: bank.smoothed(particles=True), max(calls // 4, 2))
    rec["smoothed_one_lag_with_pose"] = event_ms(lambda: bank.smoothed(8, observation=True), calls)
    # forecasts: the bank, and the F single filters holding its clouds one after another
    st = bank.export_state()
    singles = []
    for f in range(F):
        pf = pkg.GPMDM_PF(m, T, P, rng="philox", seed=11 + f)
        pf.load_state(st["states"][f], st["classes"][f], ll=st["ll"][f], log_w=st["log_w"][f], w=st["w"][f],
                      resample_idx=st["resample_idx"][f], frame=st["frame"])   # (the frame keys the draws)
        singles.append(pf)

    def all_singles(H, pose):
        for f, pf in enumerate(singles):
            pf.forecast(H, observation=pose, seed=11 + f)

    for pose, tag in ((True, "pose"), (False, "no_pose")):
        for H in (8, 32):
            n = max(calls * 8 // H, 2)
            rec[f"bank_forecast_{tag}_H{H}"] = event_ms(lambda: bank.forecast(H, observation=pose), n)
            rec[f"singles_forecast_{tag}_H{H}"] = event_ms(lambda: all_singles(H, pose), max(n // 4, 2))
        for who in ("bank", "singles"):
            rec[f"{who}_step_{tag}"] = (rec[f"{who}_forecast_{tag}_H32"]["median"] -
                                        rec[f"{who}_forecast_{tag}_H8"]["median"]) / 24
        rec[f"singles_over_bank_H8_{tag}"] = (rec[f"singles_forecast_{tag}_H8"]["median"] /
                                              rec[f"bank_forecast_{tag}_H8"]["median"])
        rec[f"singles_over_bank_step_{tag}"] = rec[f"singles_step_{tag}"] / rec[f"bank_step_{tag}"]
    rec["bank_predict"] = event_ms(lambda: bank.predict(), calls * 4)
    rec["bank_pose_readout"] = event_ms(lambda: bank.current_observation(), calls * 4)
    rec["step_pose_over_predict_plus_readout"] = rec["bank_step_pose"] / (
        rec["bank_predict"]["median"] + rec["bank_pose_readout"]["median"])
    fb = bank.forecast(3, particles=True)
    rec["bank_rows_equal_singles_bitwise"] = bool(all(
        np.array_equal(fb.states[f].numpy(), pf.forecast(3, particles=True, seed=11 + f).states.numpy())
        for f, pf in enumerate(singles)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bank_rollout"))
    ap.add_argument("--tree", default=None, help="import gpmdm_amd from this checkout (the parent commit's build): "
                                                 "the lag-0 frame only")
    ap.add_argument("--frames-only", action="store_true", help="the lag-0 frame only")
    ap.add_argument("--label", default="branch", help="recorded with every line")
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    root = Path(a.tree).resolve() if a.tree else ROOT
    sys.path.insert(0, str(root))
    import gpmdm_amd as pkg
    from gpmdm_amd import _lib, synthetic  # noqa: F401  (pkg._lib, pkg.synthetic)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "runs.jsonl", "a") as fh:
        for name in a.shapes:
            r = run(pkg, name, parent_only=a.tree is not None or a.frames_only)
            r["tree"], r["commit"] = a.label, a.commit or commit_hash(root)
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
