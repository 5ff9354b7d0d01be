"""GPU: either entry point serves an F = 1 handle.

A single filter is a bank of one: gpmdm_pf_forecast / gpmdm_bank_forecast and gpmdm_pf_smoothed /
gpmdm_bank_smoothed run the same kernels (csrc/forecast.h, csrc/smooth.h), so on one single-filter
handle the two calls of a pair give bitwise the same fields -- except the forecast's
``state_mean``: the ``pf`` entry sums it in class-grouped order inside the finish, the ``bank``
entry per filter in particle order, whatever F.  Each is held to its definition,
``|state_mean - fsum mean of the call's states| <= P 2^-53 mean_p |x_pj|`` (bank_rollout_common).
"""
import ctypes

import numpy as np
import pytest
import torch

from bank_rollout_common import fsum_mean, mean_bound
from conftest import product_model

pytestmark = pytest.mark.gpu

H, LAG, UPDATES = 3, 3, 5


@pytest.fixture(scope="module")
def m1(fx_config1):
    return product_model(fx_config1)


def _forecast(pf, entry, mode):
    from gpmdm_amd import _lib
    P, C, d, D = pf._num_particles, pf.num_classes, pf.latent_dim, pf.observation_dim
    a = dict(class_prob=np.zeros((H, C)), state_mean=np.zeros((H, d)), obs_mean=np.zeros((H, D)),
             obs_spread=np.zeros((H, D)), states=np.zeros((H, P, d)), classes=np.zeros((H, P), dtype=np.int64))
    out = _lib.ForecastOut(*(_lib.i64ptr(v) if k == "classes" else _lib.dptr(v) for k, v in a.items()))
    _lib.check(getattr(_lib.load(), entry)(pf._h, H, _lib.FORECAST_MODES[mode], None, ctypes.byref(out), pf._stream()),
               entry)
    return a


def _smoothed(pf, entry, n):
    from gpmdm_amd import _lib
    P, C, d, D = pf._num_particles, pf.num_classes, pf.latent_dim, pf.observation_dim
    a = dict(class_prob=np.zeros((n, C)), state_mean=np.zeros((n, d)), distinct=np.zeros(n, dtype=np.int64),
             obs_mean=np.zeros((n, D)), obs_spread=np.zeros((n, D)), ancestors=np.zeros((n, P), dtype=np.int64),
             states=np.zeros((n, P, d)), classes=np.zeros((n, P), dtype=np.int64))
    out = _lib.SmoothedOut(*(_lib.i64ptr(v) if v.dtype == np.int64 else _lib.dptr(v) for v in a.values()))
    _lib.check(getattr(_lib.load(), entry)(pf._h, 0, n - 1, ctypes.byref(out), pf._stream()), entry)
    return a


@pytest.mark.parametrize("P", [300, 1, 33])
def test_either_entry_point_serves_a_single_filter(m1, fx_config1, P):
    """Config 1, one Philox filter (P = 300: the second 256-block holds 44 live threads; one
    particle; a partial wave) with smoothing lag 3 after 5 updates: forecast H = 3 in both modes
    and smoothed over every lag, pose and particles on, through both entry points."""
    from gpmdm_amd import GPMDM_PF
    fx = fx_config1
    pf = GPMDM_PF(m1, torch.tensor(fx["T"]), P, rng="philox", seed=11, smoothing_lag=LAG)
    for k in range(UPDATES):
        pf.update(fx["z"][k])
    for mode in ("sample", "mean"):
        a, b = _forecast(pf, "gpmdm_pf_forecast", mode), _forecast(pf, "gpmdm_bank_forecast", mode)
        for k in a:
            if k != "state_mean":
                assert np.array_equal(a[k], b[k]), (mode, k)
        for name, r in (("pf", a), ("bank", b)):
            err, bound = np.abs(r["state_mean"] - fsum_mean(r["states"])), mean_bound(r["states"])
            print(P, mode, name, "state_mean err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (mode, name, err, bound)
    assert pf.smoothing_depth == LAG
    a, b = _smoothed(pf, "gpmdm_pf_smoothed", LAG + 1), _smoothed(pf, "gpmdm_bank_smoothed", LAG + 1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.all(a["distinct"] >= 1) and np.any(a["states"] != 0)   # (a read-out took place)
