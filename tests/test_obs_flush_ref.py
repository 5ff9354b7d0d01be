"""Self-checks of tests/obs_flush_ref.py and the host side of the flush / skip entry points (no
GPU)."""
import re
from pathlib import Path

import numpy as np

import extended_ref as E
import obs_flush_ref as F

ROOT = Path(__file__).resolve().parents[1]


def test_flushed_oracle_without_tau_is_the_triangular_oracle():
    p = E.recipe_model(3)
    om = E.oracle_of(p)
    xs, _ = E.regime_points(p)
    a, b = F.oracle_obs_triangular_flushed(om, xs), E.oracle_obs_triangular(om, xs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_flush_is_partial_on_the_cutoff_recipe_and_moves_the_oracle_below_its_own_error():
    """The "cutoff" recipe's query points hold kernel values on both sides of a tau of the size
    the models report, and flushing them moves the fp64 oracle's vc by far less than the margin
    the accuracy tests allow it."""
    p = E.recipe_model(3, L=55, x_scale=3.0, ls_range=(0.4, 0.6))
    om = E.oracle_of(p)
    xs, _ = E.regime_points(p)
    N = p["X"].shape[0]
    sigma2 = float(np.exp(p["y_log_sigma_n"])) ** 2
    tau = F.tau_numpy(N, sigma2, om.Ky_inv @ om.Y, np.max(np.abs(p["Y"]), axis=0))
    assert 1e-27 < tau < 1e-22
    k = F.kernel_values(p, xs)
    part = np.any((k > 0) & (k < tau), axis=0) & np.any(k >= tau, axis=0)
    assert part.sum() >= 60
    (_, v0), (_, v1) = F.oracle_obs_triangular_flushed(om, xs), F.oracle_obs_triangular_flushed(om, xs, tau)
    assert np.max(np.abs(v1 - v0) / np.abs(v0)) <= 2.0 ** -52


def test_tau_numpy_bounds():
    """tau_q alone when M = 0; the mean bound takes over for a heavy column."""
    N, s2 = 100, 0.0225
    y = np.array([1.0, 2.0])
    t0 = F.tau_numpy(N, s2, np.zeros((N, 2)), y)
    vc = s2 / (N + s2)
    assert t0 == np.sqrt(s2) * 0.5 * (np.nextafter(vc, 1.0) - vc) / (2.001 * np.sqrt(100.0))
    M = np.zeros((N, 2))
    M[:, 1] = 1e12
    assert F.tau_numpy(N, s2, M, y) == 0.5 * (np.nextafter(2.0, 1e308) - 2.0) / (N * 1e12)


def test_entry_points_in_header_and_binding():
    from gpmdm_amd import _lib
    header = (ROOT / "include" / "gpmdm_hip.h").read_text()
    src = Path(_lib.__file__).read_text()
    for name in ("gpmdm_model_set_obs_flush", "gpmdm_model_obs_flush", "gpmdm_pf_set_obs_skip"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert f'"{name}"' in src, name
