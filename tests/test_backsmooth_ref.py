"""The marginal backward smoother's reference (tests/backsmooth_ref.py) checked on cases whose
answer is known without it (no GPU): one source, identical sources, mass conservation, a 2 x 2
two-lag case against the enumeration of every path, a zero of T that cuts a target off, and the
fp64 restatement that serves the GPU tests as yardstick."""
import itertools

import numpy as np
import pytest

import backsmooth_ref as R
from extended_ref import LD


def _case(n_s, n_t, C=2, d=3, seed=0, spread=1.0):
    """Random clouds, a row-stochastic T without zeros, and made-up moments: mu near the source,
    v in [0.05, 0.5] (the reference takes the moments as given)."""
    rng = np.random.RandomState(seed)
    Xs, Xt = rng.randn(n_s, d), spread * rng.randn(n_t, d)
    cs, ct = rng.randint(0, C, n_s), rng.randint(0, C, n_t)
    T = rng.uniform(0.1, 1.0, (C, C))
    T /= T.sum(1, keepdims=True)
    mu = np.stack([Xs * (0.9 - 0.1 * c) + 0.05 * c for c in range(C)])
    var = rng.uniform(0.05, 0.5, (C, n_s, d))
    wt = rng.uniform(0.1, 1.0, n_t)
    return T, Xs, cs, Xt, ct, wt / wt.sum(), mu, var


def test_one_source_takes_every_reached_weight():
    T, Xs, cs, Xt, ct, wt, mu, var = _case(1, 40)
    ws, ld, _ = R.backward_step(T, Xs, cs, None, Xt, ct, wt, mu, var)
    assert abs(ws[0] - R.ld_sum(wt)) <= 40 * 2.0 ** -63
    lf = R.log_f(T, Xs, cs, Xt, ct, mu, var)
    assert np.all(np.abs(ld - lf[0]) <= 2.0 ** -60 * np.abs(lf[0]))      # D_j = 1 * f_0j


def test_identical_sources_share_equally_and_mass_is_kept():
    T, Xs, cs, Xt, ct, wt, mu, var = _case(6, 30, seed=1)
    Xs[:] = Xs[0]
    cs[:] = cs[0]
    mu[:, :] = mu[:, :1]
    var[:, :] = var[:, :1]
    for dedup in (True, False):
        ws, _, _ = R.backward_step(T, Xs, cs, None, Xt, ct, wt, mu, var, dedup=dedup)
        assert np.all(np.abs(ws - R.ld_sum(wt) / 6) <= 2.0 ** -58) and np.all(ws == ws[0])
    T, Xs, cs, Xt, ct, wt, mu, var = _case(50, 70, seed=2)
    a = np.random.RandomState(5).uniform(0.1, 1, 50)
    a /= a.sum()
    for aa in (None, a):
        ws, _, _ = R.backward_step(T, Xs, cs, aa, Xt, ct, wt, mu, var)
        assert abs(ws.sum() - R.ld_sum(wt)) <= 2.0 ** -56       # sum_i a_i f_ij / D_j = 1 for every j


def test_distinct_row_grouping_changes_nothing():
    T, Xs, cs, Xt, ct, wt, mu, var = _case(40, 30, seed=3)
    pick_s, pick_t = np.random.RandomState(1).randint(0, 8, 40), np.random.RandomState(2).randint(0, 6, 30)
    args = (T, Xs[pick_s], cs[pick_s], None, Xt[pick_t], ct[pick_t], wt, mu[:, pick_s], var[:, pick_s])
    a, la, _ = R.backward_step(*args, dedup=True)
    b, lb, _ = R.backward_step(*args, dedup=False)
    assert np.all(np.abs(a - b) <= 2.0 ** -58 * b) and np.all(np.abs(la - lb) <= 2.0 ** -58 * np.abs(lb))


def test_two_lags_against_every_path():
    """2 particles per frame, 3 frames: w_2 from two backward steps equals the sum over the four
    (j1, j0) continuations of the product of normalised transition weights."""
    d, C = 2, 2
    rng = np.random.RandomState(7)
    X = [rng.randn(2, d) for _ in range(3)]                 # frames t-2, t-1, t
    c = [rng.randint(0, C, 2) for _ in range(3)]
    T = np.array([[0.7, 0.3], [0.2, 0.8]])
    mom = [(np.stack([x * 0.8 + 0.1 * k for k in range(C)]), rng.uniform(0.1, 0.4, (C, 2, d))) for x in X]
    w = np.full(2, LD(1) / 2)
    for l in (0, 1):
        w, _, _ = R.backward_step(T, X[1 - l], c[1 - l], None, X[2 - l], c[2 - l], w, *mom[1 - l])
    f = [np.exp(R.log_f(T, X[s], c[s], X[s + 1], c[s + 1], *mom[s])) for s in (0, 1)]
    half = LD(1) / 2
    brute = np.zeros(2, dtype=LD)
    for i, j1, j0 in itertools.product(range(2), repeat=3):
        D0 = half * (f[1][0, j0] + f[1][1, j0])
        D1 = half * (f[0][0, j1] + f[0][1, j1])
        brute[i] += half * (half * f[1][j1, j0] / D0) * (half * f[0][i, j1] / D1)
    assert np.all(np.abs(w - brute) <= 2.0 ** -58 * brute)
    assert abs(w.sum() - 1) <= 2.0 ** -58


def test_a_zero_of_T_cuts_a_target_off():
    T, Xs, cs, Xt, ct, wt, mu, var = _case(20, 25, seed=4)
    cs[:] = 0
    T = np.array([[1.0, 0.0], [0.5, 0.5]])
    ct[:3] = 1                                              # nobody reaches class 1
    ct[3:] = 0
    ws, ld, info = R.backward_step(T, Xs, cs, None, Xt, ct, wt, mu, var)
    assert np.all(ld[:3] == -np.inf) and np.all(np.isfinite(ld[3:].astype(np.float64)))
    assert abs(ws.sum() - R.ld_sum(wt[3:])) <= 2.0 ** -56  # the cut-off targets' mass is missing
    assert np.isfinite(info["G"])
    # a source with an unusable variance reaches nobody of that class
    var[0, 5, 1] = 0.0
    ws2, _, _ = R.backward_step(T, Xs, cs, None, Xt, ct, wt, mu, var)
    assert ws2[5] == 0 and abs(ws2.sum() - R.ld_sum(wt[3:])) <= 2.0 ** -56


@pytest.mark.parametrize("spread", [1.0, 30.0])
def test_fp64_restatement_is_a_yardstick(spread):
    """The same statements in fp64 stay inside the band, far inside it."""
    T, Xs, cs, Xt, ct, wt, mu, var = _case(60, 50, seed=6, spread=spread)
    ws, ld, info = R.backward_step(T, Xs, cs, None, Xt, ct, wt, mu, var)
    w64, l64, _ = R.backward_step(T, Xs, cs, None, Xt, ct, wt, mu, var, dtype=np.float64)
    band = R.band_rel(info)
    assert info["G"] <= 1e6 and band <= 1e-9
    err = np.abs(w64 - ws) / (ws * band + LD(1e-300))
    print("G", info["G"], "fp64 err / band", float(err.max()), float(np.abs(l64 - ld).max() / band))
    assert err.max() <= 1 and np.abs(l64 - ld).max() <= band


def test_rows():
    w = np.array([0.1, 0.2, 0.3, 0.4])
    X = np.arange(8.0).reshape(4, 2)
    r = R.rows(w, X, [0, 1, 1, 0], [2, 2, 0, 1], 2)
    assert np.allclose(r["class_probabilities"].astype(float), [0.5, 0.5])
    assert np.allclose(r["state_mean"].astype(float), w @ X)
    assert np.isclose(float(r["ess"]), 1 / 0.3) and np.isclose(float(r["ess_distinct"]), 1 / (2 * 0.01 + 2 * 0.04 + 0.09 + 0.16))
    assert np.isclose(float(R.rows(w, X, [0, 1, 1, 0], None, 2)["ess_distinct"]), 1 / 0.3)
