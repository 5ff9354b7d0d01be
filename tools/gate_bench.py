#!/usr/bin/env python
"""Cost of gating inside update (GPMDM_PF(gate=k); csrc/obs_gate.h).

On one GPU, for the config-2 model (P = 100k) and the notebook size (config 1: N = 500, P = 100) of
gpmdm_amd.synthetic, Philox, 5 warm-up frames, event times, three repeats of everything.  Three
filters with the same seeds in one process, stepped in alternating order on the same stream:
  * off:    predictive=True, no gate -- the frame the gate is measured against;
  * clean:  gate on with a threshold no joint reaches: the innovation launches, the decision and
            the two launches that return at once (what every gated-mode frame pays);
  * gated:  the same threshold, and one joint of every frame far off: the re-weigh tile and its
            finish run (what a frame that rejects something pays on top).
The frame is update plus the three read-outs.  Beside them, on the gated filter's cloud, the event
time of back-to-back launch-only calls of the pose read-out (gpmdm_pf_observation) and of the
innovation launches (gpmdm_pf_innovation): the K loop the re-weigh tile shares, and the statistic
the gate launches.  ``reweigh_over_readout`` = (gated - clean) / read-out.
Prints one JSON line per configuration and writes profiles/gate/config{1,2}.json.

    python tools/gate_bench.py [--configs 2 1] [--out profiles/gate]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from gpmdm_amd import GPMDM_PF, _lib, synthetic  # noqa: E402
from innovation_bench import build_model, commit_hash, event_ms, frame_ms  # noqa: E402

THRESHOLD = 1e3      # |zscore| no joint of the clean stream reaches
SHIFT = 1e9          # added to joint 0 of every frame the `gated` filter sees


def run(cfg, frames, calls, repeats):
    c = synthetic.CONFIGS[cfg]
    dev = torch.device("cuda:0")
    m, data = build_model(c, dev)
    P = c["P"]
    T = torch.from_numpy(synthetic.markov_matrix(c["C"]))
    zs = np.asarray(data.observation_stream(5 + repeats * frames, seed=1), dtype=np.float64)
    bad = zs.copy()
    bad[:, 0] += SHIFT
    kinds = {"off": dict(predictive=True), "clean": dict(gate=THRESHOLD), "gated": dict(gate=THRESHOLD)}
    pfs = {}
    for kind, kw in kinds.items():
        torch.manual_seed(0)
        pfs[kind] = GPMDM_PF(m, T, P, rng="philox", seed=11, **kw)
        for k in range(5):
            pfs[kind].update(bad[k] if kind == "gated" else zs[k])
    assert pfs["clean"].gate_report().n_gated == 0 and pfs["gated"].gate_report().n_gated == 1
    res = {k: [] for k in kinds}
    order = list(kinds)
    k0 = 5
    for r in range(repeats):
        for kind in order:
            res[kind].append(frame_ms(pfs[kind], (bad if kind == "gated" else zs)[k0:k0 + frames]))
        order = order[1:] + order[:1]                       # rotate the order
        k0 += frames
    assert pfs["clean"].gate_report().n_gated == 0 and pfs["gated"].gate_report().n_gated == 1
    pf = pfs["gated"]
    pf.innovation()
    pf.current_observation()                                # scratch allocated, kernels loaded
    lib, h, s = _lib.load(), pf._h, pf._stream()
    launch = {
        "innovation": lambda: _lib.check(lib.gpmdm_pf_innovation(h, None, s), "innovation"),
        "observation": lambda: _lib.check(lib.gpmdm_pf_observation(h, None, None, s), "read-out"),
    }
    ev = {k: [event_ms(fn, calls) for _ in range(repeats)] for k, fn in launch.items()}
    best = {k: min(v) for k, v in res.items()}
    extra_clean, extra_gated = best["clean"] - best["off"], best["gated"] - best["clean"]
    return {
        "config": cfg, "N": c["C"] * c["S"] * c["L"], "D": c["D"], "d": c["d"], "P": P, "rng": "philox",
        "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "frames": frames, "calls": calls,
        "frame_ms_predictive": res["off"], "frame_ms_gate_clean": res["clean"], "frame_ms_gate_gated": res["gated"],
        "innovation_event_ms": ev["innovation"], "observation_event_ms": ev["observation"],
        "gate_clean_extra_ms": extra_clean, "gate_gated_extra_ms": extra_gated,
        "clean_extra_over_innovation": extra_clean / min(ev["innovation"]),
        "reweigh_over_readout": extra_gated / min(ev["observation"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gate"))
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
