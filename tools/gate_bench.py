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

``--filters F``: the same three frames for a bank of F filters (GPMDM_PF_Bank(gate=k), every filter
its own stream; ``gated``: filter 0 rejects a joint) and, beside them, the loop of F single gated
filters the bank's gate replaces; writes profiles/gate/bank{F}_config{cfg}.json.

    python tools/gate_bench.py [--configs 2 1] [--out profiles/gate]
    python tools/gate_bench.py --filters 39 [--configs 1]
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


class SingleLoop:
    """F single gated filters stepped one after another: what a bank's gate replaces."""

    def __init__(self, pfs):
        self.pfs = pfs

    def update(self, Z):
        for pf, z in zip(self.pfs, Z):
            pf.update(z)

    def class_probabilities(self):
        return [pf.class_probabilities() for pf in self.pfs]

    def current_state_mean(self):
        return [pf.current_state_mean() for pf in self.pfs]

    def log_likelihood(self):
        return [pf.log_likelihood() for pf in self.pfs]


def run_bank(cfg, F, frames, repeats):
    """--filters F: a bank of F filters (each its own stream) with predictive=True only, gated with
    nothing rejected, gated with filter 0 rejecting joint 0 of every frame, and the loop of F single
    gated filters on that last stream; the same rotation and figures as ``run``."""
    from gpmdm_amd import GPMDM_PF_Bank
    c = synthetic.CONFIGS[cfg]
    dev = torch.device("cuda:0")
    m, data = build_model(c, dev)
    P = c["P"]
    T = torch.from_numpy(synthetic.markov_matrix(c["C"]))
    n = 5 + repeats * frames
    zs = np.stack([np.asarray(data.observation_stream(n, seed=1 + f), dtype=np.float64) for f in range(F)], 1)
    bad = zs.copy()
    bad[:, 0, 0] += SHIFT
    kinds = {"off": dict(predictive=True), "clean": dict(predictive=True, gate=THRESHOLD),
             "gated": dict(predictive=True, gate=THRESHOLD), "loop": None}
    runs = {}
    for kind, kw in kinds.items():
        if kw is None:
            torch.manual_seed(0)
            runs[kind] = SingleLoop([GPMDM_PF(m, T, P, rng="philox", seed=11 + f, gate=THRESHOLD) for f in range(F)])
        else:
            runs[kind] = GPMDM_PF_Bank(m, T, F, P, seed=11, **kw)
        for k in range(5):
            runs[kind].update(zs[k] if kind in ("off", "clean") else bad[k])

    def verdicts():
        assert not runs["clean"].gate_report().n_gated.any()
        assert runs["gated"].gate_report().n_gated.tolist() == [1] + [0] * (F - 1)
        assert [pf.gate_report().n_gated for pf in runs["loop"].pfs] == [1] + [0] * (F - 1)

    verdicts()
    res = {k: [] for k in kinds}
    order = list(kinds)
    k0 = 5
    for r in range(repeats):
        for kind in order:
            res[kind].append(frame_ms(runs[kind], (zs if kind in ("off", "clean") else bad)[k0:k0 + frames]))
        order = order[1:] + order[:1]                       # rotate the order
        k0 += frames
    verdicts()
    best = {k: min(v) for k, v in res.items()}
    return {
        "config": cfg, "N": c["C"] * c["S"] * c["L"], "D": c["D"], "d": c["d"], "P": P, "filters": F, "rng": "philox",
        "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "frames": frames,
        "frame_ms_bank_predictive": res["off"], "frame_ms_bank_gate_clean": res["clean"],
        "frame_ms_bank_gate_gated": res["gated"], "frame_ms_single_loop_gated": res["loop"],
        "gate_clean_extra_ms": best["clean"] - best["off"], "gate_gated_extra_ms": best["gated"] - best["clean"],
        "loop_over_bank": best["loop"] / best["gated"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=0,
                    help="F > 0: the bank mode (run_bank; default config 1); writes bank{F}_config{cfg}.json")
    ap.add_argument("--configs", type=int, nargs="+", default=None, help="default: 2 1")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gate"))
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    for cfg in a.configs or ([1] if a.filters > 0 else [2, 1]):
        r = run_bank(cfg, a.filters, a.frames, a.repeats) if a.filters > 0 else run(cfg, a.frames, a.calls, a.repeats)
        if a.commit:
            r["commit"] = a.commit
        name = f"bank{a.filters}_config{cfg}.json" if a.filters > 0 else f"config{cfg}.json"
        (out / name).write_text(json.dumps(r, indent=1) + "\n")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
