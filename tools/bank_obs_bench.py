#!/usr/bin/env python
"""Cost of per-filter observation masks and of the pose read-out in a filter bank
(GPMDM_PF_Bank.update(Z, observed=...), current_observation; gpmdm_bank_set_obs_masks,
gpmdm_bank_observation).

On one GPU, for the config-1 model of gpmdm_amd.synthetic (N = 500) at F = 39, P = 100 and the
config-2 model (N = 2000) at F = 8, P = 8000, after 20 warm-up frames, five windows each of
  * the unmasked frame (bank.update(Z));
  * the masked frame with constant masks (installed once: the mask's bytes do not change);
  * the masked frame with masks that change every frame (the capture-stream case: one
    gpmdm_bank_set_obs_masks install per frame);
  * the bank's pose read-out (gpmdm_bank_observation with no host outputs: the two launches
    alone) against F single-filter read-outs of the same clouds run one after another.
A window is a host clock around frames that end in a device synchronise (the frames), or a pair
of device events (the read-outs).  Writes profiles/bank_obs/<shape>.json with the commit hash,
every window's value and the median.

    python tools/bank_obs_bench.py [--out profiles/bank_obs] [--tree DIR --label parent]

--tree imports gpmdm_amd from another checkout (one built from the parent commit, for its
unmasked figure): the masked frames and the bank read-out are then skipped.
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
SHAPES = {"f39_p100_n500": (1, 39, 100, 2000), "f8_p8000_n2000": (2, 8, 8000, 200)}   # config, F, P, frames per window
WINDOWS, WARMUP = 5, 20


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


def summary(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "windows": vals}


def frame_windows(step, frames):
    """ms per frame of `frames` calls of step(k), WINDOWS times, after WARMUP calls."""
    for k in range(WARMUP):
        step(k)
    out, k0 = [], WARMUP
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(k0, k0 + frames):
            step(k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / frames * 1e3)
        k0 += frames
    return summary(out)


def event_windows(fn, calls):
    fn()                                            # buffers allocated, kernels loaded
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return summary(out)


def run(pkg, name, parent_only):
    cfg, F, P, frames = SHAPES[name]
    synthetic, _lib = pkg.synthetic, pkg._lib
    c = synthetic.CONFIGS[cfg]
    dev = torch.device("cuda:0")
    m, data = build_model(pkg, c, dev)
    D = c["D"]
    T = torch.from_numpy(synthetic.markov_matrix(c["C"]))
    zs = np.asarray(data.observation_stream(256 + F, seed=1), dtype=np.float64)
    Zs = [np.stack([zs[(k + f) % 256] for f in range(F)]) for k in range(256)]
    j = np.arange(D)
    # four masks per filter: every third joint missing (three phases) and joints 0-15 missing
    pats = [j % 3 != 0, j % 3 != 1, j % 3 != 2, j >= 16]
    rot = [np.stack([pats[(f + k) % 4] for f in range(F)]) for k in range(4)]
    Zm = [[np.where(rot[r], Z, np.nan) for Z in Zs] for r in range(4)]
    lib = _lib.load()
    rec = {"shape": name, "config": cfg, "N": c["C"] * c["S"] * c["L"], "D": D, "d": c["d"], "F": F, "P": P,
           "frames_per_window": frames, "windows": WINDOWS, "warmup_frames": WARMUP,
           "device": torch.cuda.get_device_name(0), "unit": "ms"}

    bank = pkg.GPMDM_PF_Bank(m, T, F, P, seed=11)
    rec["unmasked_frame"] = frame_windows(lambda k: bank.update(Zs[k % 256]), frames)
    if not parent_only:
        rec["masked_frame_constant_masks"] = frame_windows(lambda k: bank.update(Zm[0][k % 256], observed=rot[0]), frames)
        rec["masked_frame_changing_masks"] = frame_windows(
            lambda k: bank.update(Zm[k % 4][k % 256], observed=rot[k % 4]), frames)
        bank.update(Zs[0])                           # (observed=None again)
        rec["unmasked_frame_after"] = frame_windows(lambda k: bank.update(Zs[k % 256]), frames)
    st = bank.export_state()
    calls = 200 if F * P <= 10_000 else 50
    if not parent_only:
        def bank_readout():
            _lib.check(lib.gpmdm_bank_observation(bank._h, None, None, bank._stream()), "read-out")
        rec["bank_readout"] = event_windows(bank_readout, calls)
    singles = []
    for f in range(F):
        pf = pkg.GPMDM_PF(m, T, P, rng="philox", seed=11 + f)
        pf.load_state(st["states"][f], st["classes"][f])
        singles.append(pf)

    def single_readouts():
        for pf in singles:
            _lib.check(lib.gpmdm_pf_observation(pf._h, None, None, pf._stream()), "read-out")
    rec["single_readouts_in_sequence"] = event_windows(single_readouts, max(calls // 4, 10))
    if not parent_only:
        pose = bank.current_observation()
        rec["bank_pose_equals_singles_bitwise"] = bool(all(
            np.array_equal(pose[0][f].numpy(), pf.current_observation()[0].numpy()) and
            np.array_equal(pose[1][f].numpy(), pf.current_observation()[1].numpy()) for f, pf in enumerate(singles)))
        rec["readout_singles_over_bank"] = rec["single_readouts_in_sequence"]["median"] / rec["bank_readout"]["median"]
        u = rec["unmasked_frame"]["median"]
        rec["masked_constant_over_unmasked"] = rec["masked_frame_constant_masks"]["median"] / u
        rec["masked_changing_over_unmasked"] = rec["masked_frame_changing_masks"]["median"] / u
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bank_obs"))
    ap.add_argument("--tree", default=None, help="import gpmdm_amd from this checkout (the parent commit's build): "
                                                 "unmasked frame and single read-outs only")
    ap.add_argument("--label", default="branch", help="file name prefix of the records")
    ap.add_argument("--commit", default=None, help="recorded instead of git's HEAD (a tree without its history)")
    a = ap.parse_args()
    root = Path(a.tree).resolve() if a.tree else ROOT
    sys.path.insert(0, str(root))
    import gpmdm_amd as pkg
    from gpmdm_amd import _lib, synthetic  # noqa: F401  (pkg._lib, pkg.synthetic)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    for name in a.shapes:
        r = run(pkg, name, parent_only=a.tree is not None)
        r["tree"], r["commit"] = a.label, a.commit or commit_hash(root)
        (out / f"{a.label}_{name}.json").write_text(json.dumps(r, indent=1) + "\n")
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
