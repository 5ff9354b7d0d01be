#!/usr/bin/env python
"""Cost of fixed-lag smoothing (GPMDM_PF(smoothing_lag=L) / smoothed(), csrc/smooth.h).

On one GPU, for the config-2 model of gpmdm_amd.synthetic (N = 2000, D = 62, d = 3, C = 2) at
P = 100k and the config-1 (notebook) model (N = 500) at P = 100, Philox, 5 warm-up frames,
event times in one run:
  1. the frame (update + the two read-outs of the notebook's loop) with smoothing_lag 0, 8 and
     64: the record launch's cost per frame, beside the non-observation frame time;
  2. smoothed() over all 65 lags of a full lag-64 history, without the pose (class fractions,
     mean state, distinct ancestors; the trace, the reduce and the copy-back of the rows);
  3. one lag with the pose (lag 0 and lag 8), beside current_observation() on the same cloud
     (both with their copy-back and host wait).
Writes profiles/smooth/README.txt with the commit hash and one JSON line per configuration.

    python tools/smooth_bench.py [--out profiles/smooth]
    python tools/smooth_bench.py --tree OTHER_CHECKOUT    # the plain frame time of another
                                                          # build of the package (A/B), no file
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
LAGS = (0, 8, 64)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        f = ROOT / "COMMIT"
        return f.read_text().strip() if f.exists() else "unrecorded"


def build_model(g, c, device):
    data = g.synthetic.make_sequences(c["C"], c["S"], c["L"], c["D"], c["d"], seed=0)
    hp = g.synthetic.default_hyperparameters(c["D"], c["d"], 0.1)
    m = g.GPMDM(D=c["D"], d=c["d"], n_classes=c["C"], dyn_target="full", dyn_back_step=1, device=device, **hp)
    for k in range(c["C"]):
        for y in data.sequences[k]:
            m.add_data(y, k)
    m.init_X()
    return m, data


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def frame_ms(g, m, T, zs, P, frames, **kw):
    """The notebook's per-frame loop, event-timed over ``frames`` frames after 5 warm-up ones
    (three repeats: the run-to-run spread on this box)."""
    torch.manual_seed(0)
    pf = g.GPMDM_PF(m, T, P, rng="philox", seed=11, **kw)

    def frame(i):
        pf.update(zs[i % len(zs)])
        pf.class_probabilities()
        pf.current_state_mean()

    for k in range(5):
        frame(k)
    return pf, [event_ms(frame, frames) for _ in range(3)]


def run(g, cfg, P, frames, calls, plain):
    c = g.synthetic.CONFIGS[cfg]
    dev = torch.device("cuda:0")
    m, data = build_model(g, c, dev)
    C, D, d = c["C"], c["D"], c["d"]
    T = torch.from_numpy(g.synthetic.markov_matrix(C))
    zs = data.observation_stream(80, seed=1)
    r = {"config": cfg, "N": C * c["S"] * c["L"], "D": D, "d": d, "C": C, "P": P, "rng": "philox",
         "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "frames": frames, "calls": calls}
    if plain:
        r["frame_plain_ms"] = frame_ms(g, m, T, zs, P, frames)[1]
        return r
    pf = None
    for L in LAGS:
        pf, r[f"frame_lag{L}_ms"] = frame_ms(g, m, T, zs, P, frames, smoothing_lag=L)
    for L in LAGS[1:]:
        r[f"overhead_lag{L}_ms"] = min(r[f"frame_lag{L}_ms"]) - min(r["frame_lag0_ms"])
    # pf: the lag-64 filter; fill its history
    for k in range(max(0, 64 - pf.smoothing_depth)):
        pf.update(zs[k % len(zs)])
    assert pf.smoothing_depth == 64
    lib, h = g._lib.load(), pf._h
    n = 65
    cp, sm, da = np.zeros((n, C)), np.zeros((n, d)), np.zeros(n, dtype=np.int64)
    om, osp = np.zeros((1, D)), np.zeros((1, D))
    rows = g._lib.SmoothedOut(class_prob=g._lib.dptr(cp), state_mean=g._lib.dptr(sm), distinct=g._lib.i64ptr(da))
    pose = g._lib.SmoothedOut(class_prob=g._lib.dptr(cp), state_mean=g._lib.dptr(sm), distinct=g._lib.i64ptr(da),
                              obs_mean=g._lib.dptr(om), obs_spread=g._lib.dptr(osp))

    def smoothed(a, b, out):
        g._lib.check(lib.gpmdm_pf_smoothed(h, a, b, ctypes.byref(out), pf._stream()), "smoothed")

    def readout(_):
        g._lib.check(lib.gpmdm_pf_observation(h, g._lib.dptr(om), g._lib.dptr(osp), pf._stream()), "read-out")

    for fn in (lambda: smoothed(0, 64, rows), lambda: smoothed(8, 8, pose), lambda: readout(0)):   # buffers, kernels
        fn()
    r["smoothed_65_lags_ms"] = event_ms(lambda i: smoothed(0, 64, rows), calls)
    r["distinct_ancestors"] = [int(da[k]) for k in (0, 1, 8, 64)]
    r["smoothed_lag0_pose_ms"] = event_ms(lambda i: smoothed(0, 0, pose), calls)
    r["smoothed_lag8_pose_ms"] = event_ms(lambda i: smoothed(8, 8, pose), calls)
    r["smoothed_lag8_no_pose_ms"] = event_ms(lambda i: smoothed(8, 8, rows), calls)
    r["current_observation_ms"] = event_ms(readout, calls)
    return r


def table(rs):
    f3 = lambda v: " ".join(f"{x:.4f}" for x in v)   # noqa: E731
    lines = ["Fixed-lag smoothing (tools/smooth_bench.py), event times in ms; frame = update + the two read-outs,",
             "three repeats each",
             f"commit {rs[0]['commit']}  device {rs[0]['device']}", ""]
    for r in rs:
        lines.append(f"config {r['config']}: N={r['N']} D={r['D']} d={r['d']} C={r['C']} P={r['P']} "
                     f"({r['frames']} frames, {r['calls']} calls)")
        for L in LAGS:
            lines.append(f"  frame, smoothing_lag={L:<3d}        {f3(r[f'frame_lag{L}_ms'])}")
        for L in LAGS[1:]:
            lines.append(f"  overhead of lag {L:<3d} (min - min)  {r[f'overhead_lag{L}_ms']:+.4f}")
        lines += [f"  smoothed(), 65 lags, no pose    {r['smoothed_65_lags_ms']:.4f}"
                  f"   (distinct ancestors at lags 0, 1, 8, 64: {r['distinct_ancestors']})",
                  f"  smoothed(lag=8), no pose        {r['smoothed_lag8_no_pose_ms']:.4f}",
                  f"  smoothed(lag=8), with the pose  {r['smoothed_lag8_pose_ms']:.4f}",
                  f"  smoothed(lag=0), with the pose  {r['smoothed_lag0_pose_ms']:.4f}",
                  f"  current_observation()           {r['current_observation_ms']:.4f}", ""]
    lines += ["JSON:"] + [json.dumps(r) for r in rs]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "smooth"))
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    ap.add_argument("--tree", default=None, help="another checkout of the package: its plain frame time only")
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.tree).resolve() if a.tree else ROOT))
    import gpmdm_amd as g
    from gpmdm_amd import _lib, synthetic  # noqa: F401  (g._lib, g.synthetic)
    rs = [run(g, 2, 100_000, a.frames, a.calls, bool(a.tree)), run(g, 1, 100, a.frames * 10, a.calls, bool(a.tree))]
    for r in rs:
        if a.commit:
            r["commit"] = a.commit
    if a.tree:
        for r in rs:
            print(json.dumps(r), flush=True)
        return
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    text = table(rs)
    (out / "README.txt").write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
