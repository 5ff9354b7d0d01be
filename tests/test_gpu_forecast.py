"""``GPMDM_PF.forecast`` (gpmdm_pf_forecast, csrc/forecast.h): the filter's proposal rolled out
H steps on a scratch copy of the cloud.

The reference is the oracle, one step at a time and resynced: step h starts from the device's
own cloud of step h - 1 (the exported filter state for h = 1) with the restated forecast draws
of ``forecast_ref``.  Bounds:

* classes: the oracle's switch exactly;
* states: ``nrel < 1e-6`` against the oracle's propagate (the state bound of
  ``assert_step_matches``); mean mode ``nrel < 1e-9`` against the dynamics-GP mean (the bound
  of test_predict_device_vs_oracle);
* ``class_probabilities[h] = bincount(classes_h) / P`` to 1e-15;
* ``|state_mean[h, j] - mean_p x_pj| <= P 2^-52 mean_p |x_pj|``: any summation order of P fp64
  terms errs by at most (P - 1) 2^-53 sum |x|, and the bound covers the device's and numpy's;
* the pose rows: the two bounds of test_gpu_obs_readout.py::_check (1e-9 normwise for the mean;
  ``4 delta sqrt(var) + delta^2`` with delta = 1e-9 max |mu| for the spread).
"""
import ctypes

import numpy as np
import pytest
import torch

import forecast_ref as R
from conftest import nrel, oracle_model, product_model, synthetic_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


@pytest.fixture(scope="module")
def om2(fx_config2):
    return oracle_model(fx_config2)


def _oracle_of(m, Y, C, S, L):
    from oracle import gpmdm_oracle as O
    lp = {k: (getattr(m, k).detach().cpu().numpy() if getattr(m, k).dim() else float(getattr(m, k)))
          for k in ("y_log_lengthscales", "y_log_lambdas", "y_log_sigma_n", "x_log_lengthscales",
                    "x_log_lambdas", "x_log_sigma_n", "x_log_lin_coeff")}
    return O.OracleModel(X=m.X.detach().cpu().numpy().copy(), Y=Y, seq_lengths=[[L] * S] * C,
                         sigma_n_num_X=m.sigma_n_num_X, sigma_n_num_Y=m.sigma_n_num_Y, **lp).precompute()


def _check_rows(fc, st, om, T, seed, mode, what):
    """Every row of a forecast made with particles=True against the oracle, resynced."""
    T = np.asarray(T, dtype=np.float64)
    C = T.shape[0]
    states, classes = fc.states.numpy(), fc.classes.numpy()
    H, P, _ = states.shape
    x0, c0 = st["states"], st["classes"]
    for h in range(1, H + 1):
        x1, c1 = states[h - 1], classes[h - 1]
        if mode == "sample":
            rc, rx = R.sample_step(om, T, x0, c0, seed, st["frame"], h)
            tol = 1e-6
        else:
            rc, rx, tol = c0, R.mean_step(om, x0, c0), 1e-9
        assert np.array_equal(c1, rc), (what, h, int(np.sum(c1 != rc)))
        print(what, h, "states nrel", nrel(x1, rx))
        assert nrel(x1, rx) < tol, (what, h, nrel(x1, rx))
        prob = fc.class_probabilities[h - 1].numpy()
        assert np.max(np.abs(prob - np.bincount(c1, minlength=C) / P)) <= 1e-15, (what, h)
        err = np.abs(fc.state_mean[h - 1].numpy() - x1.mean(0))
        assert np.all(err <= P * 2.0 ** -52 * np.abs(x1).mean(0)), (what, h, err)
        if fc.observation_mean is not None:
            mu = om.map_x_to_y(x1)[0]
            ref_mean, ref_var = mu.mean(0), mu.var(0)
            mean, spread = fc.observation_mean[h - 1].numpy(), fc.observation_spread[h - 1].numpy()
            print(what, h, "pose nrel", nrel(mean, ref_mean))
            assert nrel(mean, ref_mean) < 1e-9, (what, h, nrel(mean, ref_mean))
            delta = 1e-9 * np.max(np.abs(mu))
            e, bound = np.abs(spread - ref_var), 4 * delta * np.sqrt(ref_var) + delta ** 2
            assert np.all(spread >= 0), (what, h)
            assert np.all(e <= bound), (what, h, float(np.max(e - bound)), float(np.max(e)))
        x0, c0 = x1, c1


def _same(a, b, fields=("class_probabilities", "state_mean", "observation_mean", "observation_spread", "states",
                        "classes")):
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            assert x is None and y is None, k
        else:
            assert np.array_equal(x.numpy(), y.numpy()), k


@pytest.mark.parametrize("P", [1, 33, 777, 5000])
def test_steps_against_the_oracle(m2, om2, fx_config2, P):
    """Config 2 after two updates: a single particle, a partial 16-row tile, several tiles with
    a partial last one, many blocks."""
    from gpmdm_amd import GPMDM_PF
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, rng="philox", seed=7)
    Y = m2.get_Y()
    for k in range(2):
        pf.update(Y[200 + k])
    st = pf.export_state()
    fc = pf.forecast(4, particles=True)
    assert fc.states.shape == (4, P, 3) and fc.classes.shape == (4, P) and fc.classes.dtype == torch.int64
    assert fc.observation_mean.shape == (4, 62) and fc.class_probabilities.shape == (4, 2)
    _check_rows(fc, st, om2, fx_config2["T"], 7, "sample", P)


@pytest.mark.parametrize("d,D,C", [(1, 5, 2), (13, 17, 2), (4, 150, 5), (3, 20, 9)])
def test_shapes(d, D, C):
    """The smallest and a wide latent dimension, D below one column tile and over three column
    groups, five classes, and nine (two dynamics-tile launches per step); N = C * 90 is no
    multiple of 16.  Sample and mean mode."""
    from gpmdm_amd import GPMDM_PF
    S, L, P = 3, 30, 200
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=L, S=S, seed=50 + d)
    om = _oracle_of(m, Y, C, S, L)
    pf = GPMDM_PF(m, T, P, rng="philox", seed=3)
    for k in range(2):
        pf.update(Y[40 + k])
    st = pf.export_state()
    _check_rows(pf.forecast(3, particles=True), st, om, T.numpy(), 3, "sample", (d, D, C))
    _check_rows(pf.forecast(3, particles=True, mode="mean"), st, om, T.numpy(), 3, "mean", (d, D, C, "mean"))


def test_absorbing_chain_leaves_an_empty_class():
    """T = [[1, 0], [1, 0]]: from the first step on class 1 is an empty segment."""
    from gpmdm_amd import GPMDM_PF
    C, d, D, S, L, P = 2, 4, 20, 3, 30, 200
    m, _, Y = synthetic_model(C=C, d=d, D=D, L=L, S=S, seed=61)
    T = np.array([[1.0, 0.0], [1.0, 0.0]])
    om = _oracle_of(m, Y, C, S, L)
    pf = GPMDM_PF(m, torch.tensor(T), P, rng="philox", seed=3)
    st = pf.export_state()
    assert len(np.unique(st["classes"])) == 2
    fc = pf.forecast(3, particles=True)
    assert np.array_equal(fc.class_probabilities.numpy(), np.tile([1.0, 0.0], (3, 1)))
    assert not fc.classes.numpy().any()
    _check_rows(fc, st, om, T, 3, "sample", "absorbing")


def test_mean_mode(m2, om2, fx_config2):
    """Classes frozen, x <- mu_c(x); the first state mean is predict()'s up to summation order."""
    from gpmdm_amd import GPMDM_PF
    P = 777
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, rng="philox", seed=7)
    Y = m2.get_Y()
    for k in range(2):
        pf.update(Y[200 + k])
    st = pf.export_state()
    fc = pf.forecast(3, mode="mean", particles=True)
    for h in range(3):
        assert np.array_equal(fc.classes[h].numpy(), st["classes"]), h
    _check_rows(fc, st, om2, fx_config2["T"], 7, "mean", "mean")
    one = pf.forecast(1, mode="mean", particles=True)
    assert np.array_equal(one.states[0].numpy(), fc.states[0].numpy())
    pred = pf.predict().numpy()
    mu = one.states[0].numpy()
    err = np.abs(one.state_mean[0].numpy() - pred)
    assert np.all(err <= P * 2.0 ** -52 * np.abs(mu).mean(0)), err


def test_determinism(m2, fx_config2):
    from gpmdm_amd import GPMDM_PF
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), 3000, rng="philox", seed=11)
    Y = m2.get_Y()
    pf.update(Y[400])
    a, b = pf.forecast(8, particles=True), pf.forecast(8, particles=True)
    _same(a, b)
    short = pf.forecast(3, particles=True)
    for k in ("class_probabilities", "state_mean", "observation_mean", "observation_spread", "states", "classes"):
        assert np.array_equal(getattr(a, k)[:3].numpy(), getattr(short, k).numpy()), k
    # the outputs do not depend on which of them are asked for
    bare = pf.forecast(8, observation=False)
    assert bare.observation_mean is None and bare.observation_spread is None and bare.states is None
    _same(a, bare, ("class_probabilities", "state_mean"))
    _same(a, pf.forecast(8), ("class_probabilities", "state_mean", "observation_mean", "observation_spread"))
    _same(a, pf.forecast(8, observation=False, particles=True), ("class_probabilities", "state_mean", "states",
                                                                 "classes"))
    # another seed, and the same seed one frame later, draw differently
    other = pf.forecast(8, particles=True, seed=12)
    assert not np.array_equal(other.states.numpy(), a.states.numpy())
    _same(a, pf.forecast(8, particles=True, seed=11))
    pf.update(Y[401])
    later = pf.forecast(8, particles=True)
    assert not np.array_equal(later.states.numpy(), a.states.numpy())
    assert not np.array_equal(later.classes.numpy(), a.classes.numpy())


@pytest.mark.parametrize("rng,P", [("philox", 3000), ("torch", 20_000)])
def test_forecast_has_no_side_effects(m2, fx_config2, rng, P):
    """Eight frames with a forecast after construction and after every frame leave the filter
    exactly where eight frames without leave it (a Philox filter's pre-switch, and at P = 20 000
    a replay filter's draws ahead with a pre-switch, are pending behind each forecast); torch's
    generator and the health counters are not touched."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Y = m2.get_Y()
    out, health = [], []
    for look in (False, True):
        torch.manual_seed(12)
        pf = GPMDM_PF(m2, T, P, rng=rng, seed=19 if rng == "philox" else None)
        if look:
            pf.forecast(3)
        for k in range(8):
            pf.update(Y[300 + k])
            if look:
                g = torch.get_rng_state()
                pf.forecast(3)
                assert torch.equal(g, torch.get_rng_state()), k
        out.append(pf.export_state())
        health.append(pf.health())
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert np.array_equal(out[0][key], out[1][key]), key
    assert health[0] == health[1]


@pytest.mark.parametrize("row0", [100, 1300])
def test_it_forecasts(m2, fx_config2, row0):
    """Guards against a vacuous stream only: after six updates on rows row0..row0+5 of the
    fixture's Y, the forecast pose is nearer the true future frame than the last seen pose at
    every horizon 1..8.  (The oracle at P = 1000: forecast errors 0.30-1.45 against 0.97-4.72
    for holding the last pose from row 100; 0.43-1.68 against 1.32-8.99 from row 1300.)"""
    from gpmdm_amd import GPMDM_PF
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), 2000, rng="philox", seed=41)
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    for k in range(6):
        pf.update(Y[row0 + k])
    pose = pf.forecast(8).observation_mean.numpy()
    last = row0 + 5
    for h in range(1, 9):
        err, hold = np.linalg.norm(pose[h - 1] - Y[last + h]), np.linalg.norm(Y[last] - Y[last + h])
        print(row0, h, err, hold)
        assert err < hold, (row0, h, err, hold)


def test_shards_banks_and_call_order(m2, fx_config2):
    """A devices=[0]*2 loopback filter forecasts its replicated cloud: bitwise the one-rank
    filter's; a bank is refused; between a switch and its resample the call is out of order."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    P = 3001

    def make(**kw):
        torch.manual_seed(6)
        return GPMDM_PF(m2, T, P, rng="philox", seed=9, **kw)

    one, two = make(), make(devices=[0] * 2, transport="loopback")
    _same(one.forecast(3, particles=True), two.forecast(3, particles=True))
    for k in range(2):
        one.update(Y[600 + k])
        two.update(Y[600 + k])
    _same(one.forecast(3, particles=True), two.forecast(3, particles=True))

    lib = _lib.load()
    bank = GPMDM_PF_Bank(m2, T, 2, 300, seed=4)
    prob = np.zeros((2, 2))
    out = _lib.ForecastOut(class_prob=_lib.dptr(prob))
    with pytest.raises(ValueError):
        _lib.check(lib.gpmdm_pf_forecast(bank._h, 2, 0, None, ctypes.byref(out), bank._stream()), "bank")

    h, s = one._h, one._stream()
    before = one.forecast(2)
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    assert lib.gpmdm_pf_forecast(h, 2, 0, None, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    z = np.ascontiguousarray(Y[602])
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), None, s), "propagate")
    assert lib.gpmdm_pf_forecast(h, 2, 0, None, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    after = one.forecast(2)
    assert not np.array_equal(before.state_mean.numpy(), after.state_mean.numpy())
