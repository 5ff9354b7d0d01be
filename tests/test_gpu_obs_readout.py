"""The filtered-pose read-out (``GPMDM_PF.current_observation``, gpmdm_pf_observation): the
observation GP's mean (gpmdm.py:955-957) averaged over the particle cloud, and the cloud's
spread, by the mean-only tile kernel of csrc/obs_readout.h.

The reference is the oracle's ``map_x_to_y(states)[0]`` on the filter's own exported cloud,
reduced in numpy.

* mean: ``nrel(mean, ref.mean(0)) < 1e-9`` -- the bound of test_predict_device_vs_oracle and
  its reasoning (fp64 GP means against BLAS whose threading, and so summation order, varies
  by box; the device's own error is ~N ulps of the largest term);
* spread: with delta = 1e-9 max|ref mu| (the mean bound), ``|spread_j - var_j| <= 4 delta
  sqrt(var_j) + delta^2`` -- the first-order propagation of a per-particle error delta into
  (1/P) sum (mu - mean)^2 (2 delta sqrt(var) by Cauchy-Schwarz, plus delta^2), with a
  factor 2 of slack;
* a collapsed cloud (every particle at one training latent) has spread >= 0 and
  <= 1e-24 max(mean^2): a one-pass E[mu^2] - mean^2 leaves ~1e-16 mean^2 there.
"""
import numpy as np
import pytest
import torch

from conftest import nrel, oracle_model, product_model, synthetic_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


@pytest.fixture(scope="module")
def om2(fx_config2):
    return oracle_model(fx_config2)


def _check(pf, om, what):
    """mean and spread of pf's cloud against the oracle on the same cloud; returns them."""
    st = pf.export_state()
    mu = om.map_x_to_y(st["states"])[0]
    ref_mean, ref_var = mu.mean(0), mu.var(0)
    mean, spread = (t.numpy() for t in pf.current_observation())
    assert nrel(mean, ref_mean) < 1e-9, (what, nrel(mean, ref_mean))
    assert np.array_equal(pf.current_observation_mean().numpy(), mean), what
    delta = 1e-9 * np.max(np.abs(mu))
    err, bound = np.abs(spread - ref_var), 4 * delta * np.sqrt(ref_var) + delta ** 2
    assert np.all(spread >= 0), what
    assert np.all(err <= bound), (what, float(np.max(err - bound)), float(np.max(err)))
    return mean, spread


@pytest.mark.parametrize("P", [1, 33, 777, 20_000])
def test_readout_config2(m2, om2, fx_config2, P):
    """d = 3, D = 62 (one column group, 14 padded columns), N = 2000: a single particle, a
    partial tile, several tiles with a partial last one, and 313 tiles (the finish's runs);
    on the initial cloud (spread over the training latents) and after two updates."""
    from gpmdm_amd import GPMDM_PF
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, rng="philox", seed=7)
    _check(pf, om2, (P, "init"))
    Y = m2.get_Y()
    for k in range(2):
        pf.update(Y[200 + k])
    _check(pf, om2, (P, "updated"))


@pytest.mark.parametrize("d,D", [(1, 5), (13, 17), (4, 150)])
def test_readout_shapes(d, D):
    """The smallest and a wide latent dimension (13: above the tuned tiles' register-resident
    range), D below one 16-column tile, and D = 150: three column groups, the last one partial.
    N = 180 is no multiple of the 16-row K-step."""
    from gpmdm_amd import GPMDM_PF
    from oracle import gpmdm_oracle as O
    C, S, L, P = 2, 3, 30, 200
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=L, S=S, seed=50 + d)
    lp = {k: (getattr(m, k).detach().cpu().numpy() if getattr(m, k).dim() else float(getattr(m, k)))
          for k in ("y_log_lengthscales", "y_log_lambdas", "y_log_sigma_n", "x_log_lengthscales",
                    "x_log_lambdas", "x_log_sigma_n", "x_log_lin_coeff")}
    om = O.OracleModel(X=m.X.detach().cpu().numpy().copy(), Y=Y, seq_lengths=[[L] * S] * C,
                       sigma_n_num_X=m.sigma_n_num_X, sigma_n_num_Y=m.sigma_n_num_Y, **lp).precompute()
    pf = GPMDM_PF(m, T, P, rng="philox", seed=3)
    _check(pf, om, (d, D, "init"))
    for k in range(2):
        pf.update(Y[40 + k])
    _check(pf, om, (d, D, "updated"))


def test_collapsed_cloud_has_no_spread(m2, om2, fx_config2):
    from gpmdm_amd import GPMDM_PF
    P = 777
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, rng="philox", seed=7)
    x = np.asarray(fx_config2["X"][1234], dtype=np.float64)
    pf.load_state(np.tile(x, (P, 1)), np.zeros(P, dtype=np.int64))
    mean, spread = (t.numpy() for t in pf.current_observation())
    ref = om2.map_x_to_y(x[None, :])[0][0]
    assert nrel(mean, ref) < 1e-9, nrel(mean, ref)
    assert np.all(spread >= 0)
    assert np.all(spread <= 1e-24 * np.max(mean ** 2)), float(np.max(spread))


def test_imputation_end_to_end(m2, om2, fx_config2):
    """Joints 20-40 masked out (NaN) for six frames, rows 100-105 of the fixture's Y: the
    read-out on the masked joints is the oracle's on the same cloud (the check), and beats
    predicting them by the training mean (0: meanY = 0) -- which only guards against a vacuous
    stream: with the oracle alone (P = 2000, two seeds, also rows 1300-1305) the read-out's
    error on the masked joints is 0.18-0.31 per frame against 3.3-4.0 for the mean."""
    from gpmdm_amd import GPMDM_PF
    P, D = 2000, 62
    obs = np.ones(D, dtype=bool)
    obs[20:41] = False
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, rng="philox", seed=41)
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    for k in range(6):
        z = Y[100 + k].copy()
        truth = z[~obs].copy()
        z[~obs] = np.nan
        pf.update(z, observed=np.isfinite(z))
        mean, _ = _check(pf, om2, ("impute", k))
        assert np.linalg.norm(mean[~obs] - truth) < np.linalg.norm(truth), k
    assert pf.health() == {k: 0 for k in pf.health()}


@pytest.mark.parametrize("rng,P", [("philox", 3000), ("torch", 20_000)])
def test_readout_has_no_side_effects(m2, fx_config2, rng, P):
    """Eight frames with a read-out after construction and after every frame leave the filter
    exactly where eight frames without leave it -- a Philox filter's pre-switch stays pending
    behind it, and at P = 20 000 a replay filter draws ahead (ParallelFrameDraws) with a
    pre-switch; two consecutive read-outs are bitwise equal."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Y = m2.get_Y()
    out = []
    for read in (False, True):
        torch.manual_seed(12)
        pf = GPMDM_PF(m2, T, P, rng=rng, seed=19 if rng == "philox" else None)
        if read:
            pf.current_observation()
        for k in range(8):
            pf.update(Y[300 + k])
            if read:
                a = pf.current_observation()
                b = pf.current_observation()
                assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a, b)), k
        out.append(pf.export_state())
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert np.array_equal(out[0][key], out[1][key]), key


def test_readout_with_mask_cutoff_shards_and_banks(m2, om2, fx_config2):
    """A mask or the cutoff shape the weights, never the read-out's columns: a masked cutoff
    filter's read-out is the oracle's on its cloud; a devices=[0]*2 loopback filter's equals the
    one-rank filter's bitwise; a bank is refused."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    obs = np.arange(62) % 3 != 2
    P = 3001
    mc = product_model(fx_config2)
    mc.enable_obs_cutoff(True)
    pf = GPMDM_PF(mc, T, P, rng="philox", seed=5, obs_cutoff=True)
    for k in range(2):
        z = np.where(obs, Y[500 + k], np.nan)
        pf.update(z, observed=obs)
    _check(pf, om2, "masked cutoff")

    def make(**kw):
        torch.manual_seed(6)
        return GPMDM_PF(m2, T, P, rng="philox", seed=9, **kw)

    one, two = make(), make(devices=[0] * 2, transport="loopback")
    for got in ((one.current_observation(), two.current_observation()),):
        assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(*got))
    for k in range(2):
        one.update(Y[600 + k], observed=obs)
        two.update(Y[600 + k], observed=obs)
    a, b = one.current_observation(), two.current_observation()
    assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a, b))

    bank = GPMDM_PF_Bank(m2, T, 2, 300, seed=4)
    buf = np.zeros(62)
    with pytest.raises(ValueError):
        _lib.check(_lib.load().gpmdm_pf_observation(bank._h, _lib.dptr(buf), None, bank._stream()), "bank")
