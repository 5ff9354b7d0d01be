#!/usr/bin/env python
"""Cost of marginal backward smoothing (GPMDM_PF.smoothed_marginal, csrc/backsmooth.h).

On one GPU, for the config-1 (notebook) model of gpmdm_amd.synthetic (N = 500) at P = 100 and the
config-2 model (N = 2000, D = 62, d = 3, C = 2) at P = 100k, Philox, a full lag-64 history:
  1. smoothed_marginal(lag) for lag 1, 8 and 64, event-timed with its copy-back and host wait
     (lag l costs l backward steps: the recursion starts at the current frame);
  2. pair evaluations per second, 2 l P^2 / time (each pair is evaluated once per pass), beside an
     fp64-VALU estimate: the MI355X issues 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz
     = 39.3e12 lane-instructions/s, and a pair costs about 3 d + 31 of them per pass (3 per
     dimension, ~25 for exp2, 6 for the running sum);
  3. ess and ess_distinct at those lags beside smoothed()'s distinct_ancestors.
Appends its section to profiles/smooth/README.txt (replacing an earlier one).

    python tools/backsmooth_bench.py [--out profiles/smooth] [--calls 3]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from smooth_bench import build_model, commit_hash, event_ms  # noqa: E402

LAGS = (1, 8, 64)
MARK = "Marginal backward smoothing (tools/backsmooth_bench.py)"
LANE_RATE = 256 * 4 * 16 * 2.4e9


def run(g, cfg, P, calls):
    c = g.synthetic.CONFIGS[cfg]
    m, data = build_model(g, c, torch.device("cuda:0"))
    C, D, d = c["C"], c["D"], c["d"]
    T = torch.from_numpy(g.synthetic.markov_matrix(C))
    zs = data.observation_stream(80, seed=1)
    torch.manual_seed(0)
    pf = g.GPMDM_PF(m, T, P, rng="philox", seed=11, smoothing_lag=64)
    for k in range(70):
        pf.update(zs[k % len(zs)])
    assert pf.smoothing_depth == 64
    r = {"config": cfg, "N": C * c["S"] * c["L"], "D": D, "d": d, "C": C, "P": P, "rng": "philox",
         "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "calls": calls}
    gen = pf.smoothed()
    r["distinct_ancestors"] = [int(gen.distinct_ancestors[l]) for l in LAGS]
    pf.smoothed_marginal(1)                       # buffers, kernels
    for l in LAGS:
        n = calls if l < 64 else max(1, calls // 3)
        r[f"lag{l}_ms"] = event_ms(lambda i: pf.smoothed_marginal(l), n)
        s = pf.smoothed_marginal(l)
        r[f"lag{l}_ess"] = float(s.ess[0])
        r[f"lag{l}_ess_distinct"] = float(s.ess_distinct[0])
        r[f"lag{l}_mass"] = float(s.mass[0])
        r[f"lag{l}_pair_evals_per_s"] = 2.0 * l * P * P / (r[f"lag{l}_ms"] * 1e-3)
    r["valu_estimate_pair_evals_per_s"] = LANE_RATE / (3 * d + 31)
    return r


def table(rs):
    lines = [MARK + ": event times in ms of smoothed_marginal(lag) with its copy-back and wait",
             f"commit {rs[0]['commit']}  device {rs[0]['device']}", ""]
    for r in rs:
        lines.append(f"config {r['config']}: N={r['N']} D={r['D']} d={r['d']} C={r['C']} P={r['P']} ({r['calls']} calls)")
        for l, da in zip(LAGS, r["distinct_ancestors"]):
            lines.append(f"  lag {l:<3d} {r[f'lag{l}_ms']:12.4f} ms  {r[f'lag{l}_pair_evals_per_s']:.3e} pair evaluations/s"
                         f"   ess {r[f'lag{l}_ess']:.1f}  ess_distinct {r[f'lag{l}_ess_distinct']:.1f}"
                         f"  (distinct_ancestors {da})  mass - 1 = {r[f'lag{l}_mass'] - 1:+.1e}")
        lines += [f"  fp64-VALU estimate {r['valu_estimate_pair_evals_per_s']:.3e} pair evaluations/s "
                  f"(39.3e12 lane-instructions/s over 3 d + 31 per pair and pass)", ""]
    lines += ["JSON:"] + [json.dumps(r) for r in rs]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "smooth"))
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import gpmdm_amd as g
    from gpmdm_amd import _lib, synthetic  # noqa: F401  (g._lib, g.synthetic)
    rs = [run(g, 1, 100, a.calls * 8), run(g, 2, 100_000, a.calls)]
    for r in rs:
        if a.commit:
            r["commit"] = a.commit
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    f = out / "README.txt"
    old = f.read_text() if f.exists() else ""
    if MARK in old:
        old = old[:old.index(MARK)]
    text = table(rs)
    f.write_text((old.rstrip("\n") + "\n\n" if old.strip() else "") + text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
