#!/usr/bin/env python
"""Cost of MAP trajectory decoding (GPMDM_PF.map_path, csrc/mappath.h).

On one GPU, for the config-1 (notebook) model of gpmdm_amd.synthetic (N = 500) at P = 100 and the
config-2 model (N = 2000, D = 62, d = 3, C = 2) at P = 100k, Philox, a full lag-64 history:
  1. map_path(lag) for lag 1, 8 and 64, event-timed with its copy-back and host wait (a warmed
     call first, then several calls per size);
  2. the compact sizes (the distinct resampling ancestors the recursion runs on), the pairs
     evaluated, sum_l n_{l+1} n_l, and pair evaluations per second beside an fp64-VALU estimate:
     the MI355X issues 256 CUs x 4 SIMDs x 16 fp64 lanes per clock at 2.4 GHz = 39.3e12
     lane-instructions/s, and a pair costs about 3 d + 4 of them (3 per dimension, the exponent
     fma, the compare and two selects);
  3. smoothed_marginal(lag) from the same build in the same process: what "a fraction of" means;
  4. the frame time with map recording off and on (the extra record launch).
Appends its section to profiles/smooth/README.txt (replacing an earlier one).

    python tools/map_bench.py [--out profiles/smooth] [--calls 3]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from smooth_bench import build_model, commit_hash, event_ms, frame_ms  # noqa: E402

LAGS = (1, 8, 64)
MARK = "MAP trajectory decoding (tools/map_bench.py)"
LANE_RATE = 256 * 4 * 16 * 2.4e9


def run(g, cfg, P, calls, frames):
    c = g.synthetic.CONFIGS[cfg]
    m, data = build_model(g, c, torch.device("cuda:0"))
    C, D, d = c["C"], c["D"], c["d"]
    T = torch.from_numpy(g.synthetic.markov_matrix(C))
    zs = data.observation_stream(80, seed=1)
    torch.manual_seed(0)
    pf = g.GPMDM_PF(m, T, P, rng="philox", seed=11, smoothing_lag=64, map_path=True)
    for k in range(70):
        pf.update(zs[k % len(zs)])
    assert pf.smoothing_depth == 64
    r = {"config": cfg, "N": C * c["S"] * c["L"], "D": D, "d": d, "C": C, "P": P, "rng": "philox",
         "commit": commit_hash(), "device": torch.cuda.get_device_name(0), "calls": calls}
    pf.map_path(1)                                # buffers, kernels
    pf.smoothed_marginal(1)
    for l in LAGS:
        n = calls if l < 64 else max(1, calls // 3)
        r[f"lag{l}_ms"] = event_ms(lambda i: pf.map_path(l), calls)
        mp = pf.map_path(l)
        sizes = [int(x) for x in mp.distinct]
        pairs = sum(a * b for a, b in zip(sizes[1:], sizes[:-1]))
        r[f"lag{l}_distinct_first_last"] = [sizes[0], sizes[-1]]
        r[f"lag{l}_pairs"] = pairs
        r[f"lag{l}_pair_evals_per_s"] = pairs / (r[f"lag{l}_ms"] * 1e-3)
        r[f"lag{l}_log_joint"] = mp.log_joint
        r[f"lag{l}_marginal_ms"] = event_ms(lambda i: pf.smoothed_marginal(l), n)
    r["valu_estimate_pair_evals_per_s"] = LANE_RATE / (3 * d + 4)
    r["frame_smoothing_ms"] = frame_ms(g, m, T, zs, P, frames, smoothing_lag=64)[1]
    r["frame_recording_ms"] = frame_ms(g, m, T, zs, P, frames, smoothing_lag=64, map_path=True)[1]
    return r


def table(rs):
    lines = [MARK + ": event times in ms of map_path(lag) with its copy-back and wait",
             f"commit {rs[0]['commit']}  device {rs[0]['device']}", ""]
    for r in rs:
        lines.append(f"config {r['config']}: N={r['N']} D={r['D']} d={r['d']} C={r['C']} P={r['P']} ({r['calls']} calls)")
        for l in LAGS:
            lines.append(f"  lag {l:<3d} {r[f'lag{l}_ms']:12.4f} ms   smoothed_marginal {r[f'lag{l}_marginal_ms']:12.4f} ms"
                         f"   distinct rows lag 0 / lag {l}: {r[f'lag{l}_distinct_first_last'][0]} / "
                         f"{r[f'lag{l}_distinct_first_last'][1]}   pairs {r[f'lag{l}_pairs']:.3e}"
                         f"  {r[f'lag{l}_pair_evals_per_s']:.3e} pair evaluations/s")
        lines += [f"  fp64-VALU estimate {r['valu_estimate_pair_evals_per_s']:.3e} pair evaluations/s "
                  f"(39.3e12 lane-instructions/s over 3 d + 4 per pair)",
                  "  frame, smoothing_lag=64, recording off: " + " ".join(f"{x:.4f}" for x in r["frame_smoothing_ms"]) + " ms",
                  "  frame, smoothing_lag=64, recording on:  " + " ".join(f"{x:.4f}" for x in r["frame_recording_ms"]) + " ms",
                  ""]
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
    rs = [run(g, 1, 100, a.calls * 8, 400), run(g, 2, 100_000, a.calls, 40)]
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
