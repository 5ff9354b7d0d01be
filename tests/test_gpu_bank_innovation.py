"""Innovations and the GP's predictive variance for filter banks (``GPMDM_PF_Bank.innovation``,
gpmdm_bank_innovation, gpmdm_bank_observation_gp): the filter is a grid dimension of the single
filter's kernels, so every field of row f is bitwise the single filter
``GPMDM_PF(rng='philox', seed=seed + f, predictive=True)`` stepped on ``Z[f]`` with ``M[f]`` from
the same particles -- filter 0 under a per-filter mask, filter 1 fully observed, filter 2 blacked
out in the second frame (its NaN pattern included)."""
import numpy as np
import pytest
import torch

from conftest import product_model
from test_gpu_innovation import same, same_innovation

pytestmark = pytest.mark.gpu

D = 62


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _row(inn, f):
    return type(inn)(*(None if t is None else t[f] for t in inn))


@pytest.mark.parametrize("Pf", [100, 1500])
def test_bank_rows_are_the_single_filters(m2, fx_config2, Pf):
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank
    F, seed = 3, 700
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    bank = GPMDM_PF_Bank(m2, T, F, Pf, seed=seed, predictive=True)
    st0 = bank.export_state()
    singles = []
    for f in range(F):
        pf = GPMDM_PF(m2, T, Pf, rng="philox", seed=seed + f, predictive=True)
        pf.load_state(st0["states"][f], st0["classes"][f])
        singles.append(pf)
    j = np.arange(D)
    for k in range(3):
        M = np.stack([j % 3 != 2, np.ones(D, bool), np.zeros(D, bool) if k == 1 else j >= 16])
        Z = np.where(M, np.stack([Y[500 + k + 40 * f] for f in range(F)]), np.nan)
        bank.update(Z, observed=M)
        for f, pf in enumerate(singles):
            pf.update(Z[f], observed=M[f])
        inn = bank.innovation(particles=True)
        assert tuple(inn.mean.shape) == (F, D) and tuple(inn.n_valid.shape) == (F,)
        assert tuple(inn.states.shape) == (F, Pf, 3) and tuple(inn.variance_common.shape) == (F, Pf)
        assert same(inn.observed.numpy(), M), k
        for f, pf in enumerate(singles):
            one = pf.innovation(particles=True)
            assert same_innovation(_row(inn, f), one, particles=True) == [], (k, f)
        if k == 1:
            assert int(inn.n_valid[2]) == 0 and int(inn.n_valid[0]) == Pf and int(inn.n_valid[1]) == Pf
            assert np.all(np.isnan(inn.variance_common[2].numpy()))
            for name in ("gp_variance", "variance", "residual", "zscore", "log_density"):
                assert np.all(np.isnan(getattr(inn, name)[2].numpy())), name
            assert np.all(np.isfinite(inn.mean[2].numpy())) and np.all(np.isfinite(inn.spread[2].numpy()))
        assert same_innovation(inn, bank.innovation(particles=True), particles=True) == [], k
        got = bank.current_observation(gp_variance=True)
        plain = bank.current_observation()
        assert same(got[0].numpy(), plain[0].numpy()) and same(got[1].numpy(), plain[1].numpy()), k
        for f, pf in enumerate(singles):
            for a, b in zip(got, pf.current_observation(gp_variance=True)):
                assert same(a[f].numpy(), b.numpy()), (k, f)
    sb = bank.export_state()
    for f, pf in enumerate(singles):
        s = pf.export_state()
        for key in ("states", "classes", "ll", "w", "resample_idx"):
            assert same(sb[key][f], s[key]), (f, key)


def test_bank_call_on_a_single_filter_and_refusals(m2, fx_config2):
    """gpmdm_bank_innovation / gpmdm_bank_observation_gp on an F = 1 handle are bitwise the pf calls;
    the pf calls refuse a bank."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    from gpmdm_amd.pf import _innovation_call
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    pf = GPMDM_PF(m2, T, 300, rng="philox", seed=8, predictive=True)
    for k in range(2):
        pf.update(Y[50 + k])
    a = _innovation_call(pf, "gpmdm_pf_innovation", (), True)
    b = _innovation_call(pf, "gpmdm_bank_innovation", (), True)
    assert same_innovation(a, b, particles=True) == []
    lib, g1, g2 = _lib.load(), np.zeros(D), np.zeros(D)
    _lib.check(lib.gpmdm_pf_observation_gp(pf._h, _lib.dptr(g1), pf._stream()), "pf")
    _lib.check(lib.gpmdm_bank_observation_gp(pf._h, _lib.dptr(g2), pf._stream()), "bank")
    assert same(g1, g2) and np.all(g1 > 0)
    bank = GPMDM_PF_Bank(m2, T, 2, 100, seed=4, predictive=True)
    bank.update(np.stack([Y[50], Y[90]]))
    with pytest.raises(ValueError):
        _innovation_call(bank, "gpmdm_pf_innovation", (2,), False)
    with pytest.raises(ValueError):
        _lib.check(lib.gpmdm_pf_observation_gp(bank._h, _lib.dptr(np.zeros(2 * D)), bank._stream()), "bank")
    with pytest.raises(ValueError):
        _lib.check(lib.gpmdm_pf_set_predictive(bank._h, 1), "bank")
    off = GPMDM_PF_Bank(m2, T, 2, 100, seed=4)
    off.update(np.stack([Y[50], Y[90]]))
    with pytest.raises(ValueError):
        off.innovation()
    with pytest.raises(ValueError):
        off.current_observation(gp_variance=True)
