#!/usr/bin/env python3
"""CPU estimate of what the dense observation tile's block skip leaves to multiply (DESIGN.md
§3.4 "Flush and skip in the dense tile"): the oracle filter on a bench.py configuration's model
and mocap stream, a few frames, and per frame the share of the dense tile's MFMAs whose A
fragment -- 16 particles x 4 training rows of kernel values, flushed at the model's tau -- holds
a non-zero value.  Also at whole K-step granularity (32 particles x 16 rows), to show why the
branch sits at sub-step granularity.

    python tools/obs_skip_reach.py [--config 2] [--particles 3200] [--frames 8] [--tile 32]

Particles are taken in (class, index) order and cut into tiles of --tile.  An MFMA group of
training rows 4 kk .. 4 kk + 3 counts with the number of 16-column tiles still active at its
K-step (R's upper triangle: the column tiles at or right of the rows, plus the mean tiles), as
the dense kernel runs them.  No GPU, no library: numpy and the oracle only."""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--particles", type=int, default=3200)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--tile", type=int, default=32)
    args = ap.parse_args()

    import bench
    from gpmdm_amd import synthetic
    from obs_flush_ref import tau_numpy
    from oracle import gpmdm_oracle as O
    from sklearn.decomposition import PCA

    w = bench.workload(args.config)
    data = synthetic.make_sequences(w["C"], w["S"], w["L"], w["D"], w["d"], seed=0)
    Y = np.concatenate([y for c in data.sequences for y in c]).astype(np.float64)
    X = PCA(n_components=w["d"]).fit_transform(Y)
    hp = synthetic.default_hyperparameters(w["D"], w["d"], 0.1)
    N, D, C, d = Y.shape[0], w["D"], w["C"], w["d"]
    m = O.OracleModel(X=X, Y=Y, seq_lengths=[[w["L"]] * w["S"]] * C,
                      y_log_lengthscales=np.log(hp["y_lengthscales_init"]), y_log_lambdas=np.log(hp["y_lambdas_init"]),
                      y_log_sigma_n=np.log(0.1), x_log_lengthscales=np.log(hp["x_lengthscales_init"]),
                      x_log_lambdas=np.log(hp["x_lambdas_init"]), x_log_sigma_n=np.log(0.1),
                      x_log_lin_coeff=np.log(hp["x_lin_coeff_init"])).precompute("inverse")
    sigma2 = 0.1 ** 2 + m.sigma_n_num_Y ** 2
    tau = tau_numpy(N, sigma2, m.Ky_inv @ Y, np.max(np.abs(Y), axis=0))
    print(f"config {args.config}: N={N} D={D} d={d}, tau = {tau:.3e} (cutoff distance {np.sqrt(-np.log(tau)):.2f} l)")

    # MFMA weight of a 4-row group: the 16-column tiles active at its K-step
    rows16 = -(-N // 16) * 16
    tiles_at = np.array([(-(-N // 16) - r // 16) + -(-D // 16) for r in range(0, rows16, 4)], dtype=np.float64)
    T = synthetic.markov_matrix(C)
    P, PT = args.particles - args.particles % C, args.tile
    rng = np.random.RandomState(0)
    parts = [rng.randint(0, m.X_for_class(c).shape[0], P // C) for c in range(C)]
    s, cls = O.init_particles(m, P, parts)
    z = data.observation_stream(64, seed=1)
    for f in range(args.frames):
        E, nrm, u = rng.exponential(size=(P, C)), rng.randn(P, d), rng.rand(P)
        cls1 = O.switch_classes(cls, T, E)
        prop = O.propagate_dynamics(m, s, cls1, nrm)
        k = O.rbf_kernel(m.X, prop, m.y_log_lengthscales)              # N x P
        k = np.where(k < tau, 0.0, k)
        order = np.lexsort((np.arange(P), cls1))
        nz = np.zeros((rows16, -(-P // 16) * 16), dtype=bool)
        nz[:N, :P] = k[:, order] != 0.0
        g4 = nz.reshape(rows16 // 4, 4, -1, 16).any(axis=(1, 3))       # (4-row group, 16-particle block)
        fine = float((g4 * tiles_at[:, None]).sum() / (tiles_at.sum() * g4.shape[1]))
        npt = -(-nz.shape[1] // PT) * PT
        nzp = np.zeros((rows16, npt), dtype=bool)
        nzp[:, :nz.shape[1]] = nz
        g16 = nzp.reshape(rows16 // 16, 16, -1, PT).any(axis=(1, 3))   # (K-step, particle tile)
        t16 = tiles_at.reshape(-1, 4).sum(axis=1)
        coarse = float((g16 * t16[:, None]).sum() / (t16.sum() * g16.shape[1]))
        print(f"frame {f}: MFMAs remaining at 16 x 4: {fine:.3f}   at {PT} x 16 (whole K-steps): {coarse:.3f}   "
              f"non-zero values: {nz[:N, :P].mean():.3f}")
        r = O.step(m, T, s, cls, z[f % 64], E, nrm, u)
        s, cls = r.states, r.classes


if __name__ == "__main__":
    main()
