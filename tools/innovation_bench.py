#!/usr/bin/env python
"""Cost of the innovations and of the GP's predictive variance (GPMDM_PF.innovation,
current_observation(gp_variance=True); csrc/obs_innov.h).

On one GPU, for the config-2 model (P = 100k) and the notebook size (config 1: N = 500, P = 100) of
gpmdm_amd.synthetic, Philox, 5 warm-up frames, event times, three repeats of everything:
  * the frame (update plus the three read-outs) with predictive=True against predictive=False, two
    filters in one process stepped in alternating order;
  * innovation() against current_observation() on the same cloud: device time as the event time
    of back-to-back launches of the two entry points without host outputs (the kernels alone, as
    tools/obs_readout_bench.py times the read-out), and the wall-clock of the whole Python calls
    (argument arrays, launches, copy-back, wait);
  * current_observation(gp_variance=True) against the plain call, likewise (the gather's launches).
Prints one JSON line per configuration and writes profiles/innovation/config{1,2}.json.

    python tools/innovation_bench.py [--configs 2 1] [--out profiles/innovation]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from gpmdm_amd import GPMDM, GPMDM_PF, _lib, synthetic  # noqa: E402


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
    """Event time per call of n back-to-back launch-only calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e3 / n


def frame_ms(pf, zs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for z in zs:
        pf.update(z)
        pf.class_probabilities()
        pf.current_state_mean()
        pf.log_likelihood()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / len(zs)


def run(cfg, frames, calls, repeats):
    c = synthetic.CONFIGS[cfg]
    dev = torch.device("cuda:0")
    m, data = build_model(c, dev)
    P = c["P"]
    T = torch.from_numpy(synthetic.markov_matrix(c["C"]))
    zs = data.observation_stream(5 + 2 * repeats * frames, seed=1)
    pfs = {}
    for on in (False, True):
        torch.manual_seed(0)
        pfs[on] = GPMDM_PF(m, T, P, rng="philox", seed=11, predictive=on)
        for k in range(5):
            pfs[on].update(zs[k])
    res = {False: [], True: []}
    k0 = 5
    for r in range(repeats):
        for on in ((False, True) if r % 2 == 0 else (True, False)):      # alternate the order
            res[on].append(frame_ms(pfs[on], zs[k0:k0 + frames]))
        k0 += frames
    pf = pfs[True]
    pf.innovation()
    pf.current_observation(gp_variance=True)             # scratch allocated, kernels loaded
    lib, h, s = _lib.load(), pf._h, pf._stream()
    launch = {
        "innovation": lambda: _lib.check(lib.gpmdm_pf_innovation(h, None, s), "innovation"),
        "observation": lambda: _lib.check(lib.gpmdm_pf_observation(h, None, None, s), "read-out"),
        "gather": lambda: _lib.check(lib.gpmdm_pf_observation_gp(h, None, s), "gather"),
    }
    call = {"innovation": pf.innovation, "observation": pf.current_observation,
            "observation_gp": lambda: pf.current_observation(gp_variance=True)}
    ev = {k: [] for k in launch}
    wall = {k: [] for k in call}
    for r in range(repeats):
        for k, fn in launch.items():
            ev[k].append(event_ms(fn, calls))
        for k, fn in call.items():
            wall[k].append(wall_ms(fn, calls))
    best = {k: min(v) for k, v in ev.items()}
    return {
        "config": cfg, "N": c["C"] * c["S"] * c["L"], "D": c["D"], "d": c["d"], "P": P, "rng": "philox",
        "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "frames": frames, "calls": calls,
        "frame_ms_predictive_off": res[False], "frame_ms_predictive_on": res[True],
        "innovation_event_ms": ev["innovation"], "observation_event_ms": ev["observation"],
        "gather_event_ms": ev["gather"],
        "innovation_wall_ms": wall["innovation"], "observation_wall_ms": wall["observation"],
        "observation_gp_wall_ms": wall["observation_gp"],
        "innovation_over_observation": best["innovation"] / best["observation"],
        "gp_variance_extra_wall_ms": min(wall["observation_gp"]) - min(wall["observation"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "innovation"))
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    for cfg in a.configs:
        r = run(cfg, a.frames, a.calls, a.repeats)
        if a.commit:
            r["commit"] = a.commit
        (out / f"config{cfg}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
