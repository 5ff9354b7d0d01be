#!/usr/bin/env python
"""Cost of the filtered-pose read-out (GPMDM_PF.current_observation, csrc/obs_readout.h).

On one GPU, for the config-2 and config-3 models of gpmdm_amd.synthetic at P = 100k, Philox:
after 5 warm-up frames,
  * event-times 50 launches of the read-out (gpmdm_pf_observation with no host outputs: the
    kernels alone, the host copy excluded -- as stage_times excludes it for the frame);
  * times gpmdm_predict_obs (GPMDM.map_x_to_y on device tensors: the full P x N x N
    observation pass that was the only way to the pose before) on the same exported cloud;
  * times the frame's OBS_GEMM stage over 20 frames (stage_times);
and writes profiles/obs_readout/config{2,3}.json with the commit hash.

    python tools/obs_readout_bench.py [--configs 2 3] [--out profiles/obs_readout]
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
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
    N, D, d = c["C"] * c["S"] * c["L"], c["D"], c["d"]
    T = torch.from_numpy(synthetic.markov_matrix(c["C"]))
    zs = data.observation_stream(5 + 20, seed=1)
    torch.manual_seed(0)
    pf = GPMDM_PF(m, T, P, rng="philox", seed=11)
    for k in range(5):
        pf.update(zs[k])
    lib, h = _lib.load(), pf._h

    def readout():
        _lib.check(lib.gpmdm_pf_observation(h, None, None, pf._stream()), "read-out")

    readout()                                       # buffers allocated, kernels loaded
    readout_ms = event_ms(readout, calls)
    mean, spread = pf.current_observation()
    st = pf.export_state()
    X = torch.from_numpy(st["states"]).to(dev)
    mu, _ = m.map_x_to_y(X)                         # warm-up; also the cross-check below
    ref = mu.mean(0).cpu().numpy()
    predict_ms = event_ms(lambda: m.map_x_to_y(X), 10)
    pf.stage_times()
    pf.enable_timing(True, stages=("obs_gemm",))
    for k in range(20):
        pf.update(zs[5 + k])
    pf.enable_timing(False)
    t, n = pf.stage_times()["obs_gemm"]
    obs_gemm_ms = t / max(n, 1)
    cols = 16 * -(-D // 16)
    flops = 2.0 * N * cols * P
    return {
        "config": cfg, "N": N, "D": D, "d": d, "P": P, "rng": "philox", "commit": commit_hash(),
        "device": torch.cuda.get_device_name(0),
        "readout_ms": readout_ms, "readout_calls": calls,
        "predict_obs_ms": predict_ms, "obs_gemm_ms": obs_gemm_ms, "obs_gemm_frames": int(n),
        "readout_over_obs_gemm": readout_ms / obs_gemm_ms if obs_gemm_ms else None,
        "readout_over_predict_obs": readout_ms / predict_ms if predict_ms else None,
        "target_quarter_of_obs_gemm_met": bool(obs_gemm_ms and readout_ms <= 0.25 * obs_gemm_ms),
        "mfma_flops_per_call": flops, "generated_values_per_call": float(N) * P * -(-D // 64),
        "readout_tflops": flops / (readout_ms * 1e-3) / 1e12,
        "mean_vs_predict_obs_nrel": float(np.max(np.abs(mean.numpy() - ref)) / np.max(np.abs(ref))),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "obs_readout"))
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    for cfg in a.configs:
        r = run(cfg, a.particles, a.calls)
        if a.commit:
            r["commit"] = a.commit
        (out / f"config{cfg}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
