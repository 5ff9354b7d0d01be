"""Shared helpers of the bank forecast / smoothing GPU tests (test_gpu_bank_forecast.py,
test_gpu_bank_smoothing.py, test_gpu_bank_rollout.py): the shapes of test_gpu_bank_obs.py, a bank
with its F single filters from the same particles, and per-filter views of a bank result."""
import math
import types

import numpy as np
import torch

# (config, F, Pf, resample): a 256-block and a 64-particle read-out tile span three filters, the
# small resample path; a filter's second block holds one particle; the multi-kernel path with
# blocks and tiles straddling the filter boundary; F = 1
SHAPES = [("config1", 5, 100, "multinomial"), ("config1", 3, 257, "systematic"),
          ("config2", 2, 1500, "multinomial"), ("config1", 1, 300, "multinomial")]
KEYS = ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame")
FC_EXACT = ("class_probabilities", "observation_mean", "observation_spread", "states", "classes")
FC_FIELDS = FC_EXACT + ("state_mean",)
SM_FIELDS = ("class_probabilities", "state_mean", "distinct_ancestors", "observation_mean", "observation_spread",
             "ancestors", "states", "classes")


def frame_z(fx, F, k):
    """Frame k's observations, one row of the fixture's z per filter."""
    z = np.asarray(fx["z"], dtype=np.float64)
    return np.stack([z[(k + 7 * f) % z.shape[0]] for f in range(F)])


def bank_and_singles(m, T, F, P, resample="multinomial", seed=500, **kw):
    """A bank and F single Philox filters keyed seed + f that hold the bank's initial clouds."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank
    bank = GPMDM_PF_Bank(m, T, F, P, seed=seed, resample=resample, **kw)
    st0 = bank.export_state()
    singles = []
    for f in range(F):
        pf = GPMDM_PF(m, T, P, rng="philox", seed=seed + f, resample=resample, **kw)
        pf.load_state(st0["states"][f], st0["classes"][f])
        singles.append(pf)
    return bank, singles


def update_all(bank, singles, Z):
    bank.update(Z)
    for f, pf in enumerate(singles):
        pf.update(Z[f])


def row(res, f, fields):
    """Filter f's row of a bank Forecast / Smoothed as an object with the single filter's shapes."""
    out = types.SimpleNamespace(**{k: (None if getattr(res, k) is None else getattr(res, k)[f]) for k in fields})
    for k in ("lags", "frames"):
        if hasattr(res, k):
            setattr(out, k, getattr(res, k))
    return out


def same(a, b, fields, what=""):
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            assert x is None and y is None, (what, k)
        else:
            assert x.shape == y.shape and np.array_equal(x.numpy(), y.numpy()), (what, k)


def export_row(st, f):
    """Filter f's part of a bank's export_state() as a single filter's export."""
    out = {k: st[k][f] for k in KEYS if k != "frame"}
    out["frame"] = st["frame"]
    return out


def fsum_mean(x):
    """Correctly rounded column sums of (..., P, d) divided once by P: (..., d)."""
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape(-1, x.shape[-2], x.shape[-1])
    out = np.array([[math.fsum(c[:, j]) / c.shape[0] for j in range(c.shape[1])] for c in flat])
    return out.reshape(x.shape[:-2] + (x.shape[-1],))


def mean_bound(x):
    """P 2^-53 mean_p |x_pj|: the worst case of any summation order of P fp64 terms plus the
    division (test_gpu_smoothing.py's bound)."""
    x = np.asarray(x, dtype=np.float64)
    return x.shape[-2] * 2.0 ** -53 * np.abs(x).mean(-2)


def tensor_T(fx):
    return torch.tensor(fx["T"])
