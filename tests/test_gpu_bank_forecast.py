"""GPU: ``GPMDM_PF_Bank.forecast`` (gpmdm_bank_forecast, csrc/forecast.h).

The bank changes the schedule, not the numbers: row f of every field is bitwise
``GPMDM_PF(rng='philox', seed=seed + f).forecast(H, seed=seed + f)`` of a single filter that
holds filter f's cloud at the same frame (built from the bank's export, then given the same
updates) -- with one exception.  The single filter sums ``state_mean`` in class-grouped order;
a bank sums each filter's new cloud in particle order in blocks cut within the filter.  So the
bank's ``state_mean`` is held to its own definition:

* ``|state_mean[f, h, j] - fsum mean of states[f, h, :, j]| <= Pf 2^-53 mean_p |x_pj|`` (any
  summation order of Pf fp64 terms errs by at most (Pf - 1) 2^-53 sum |x|, and the division adds
  half an ulp of the mean: test_gpu_smoothing.py's bound), and within twice that of the single
  filter's value (each side within the bound of the exact mean);
* bitwise reproducible, independent of H, and identical between a full bank and its shards.

One shape is pinned against the oracle directly, without the single filter, with
test_gpu_forecast.py's ``_check_rows`` and its tolerances.
"""
import numpy as np
import pytest
import torch

import test_gpu_forecast as TF
from bank_rollout_common import (FC_EXACT, FC_FIELDS, KEYS, SHAPES, bank_and_singles, frame_z, fsum_mean, mean_bound,
                                 row, same, update_all)
from conftest import oracle_model, product_model, synthetic_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m1(fx_config1):
    return product_model(fx_config1)


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _model(request, cfg):
    return request.getfixturevalue("m1" if cfg == "config1" else "m2"), request.getfixturevalue("fx_" + cfg)


def _check_state_mean(fb, f, single_mean, what):
    x = fb.states[f].numpy()
    err = np.abs(fb.state_mean[f].numpy() - fsum_mean(x))
    bound = mean_bound(x)
    print(what, f, "state_mean err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound), (what, f, err, bound)
    assert np.all(np.abs(fb.state_mean[f].numpy() - single_mean.numpy()) <= 2 * bound), (what, f)


def _against_singles(bank, singles, m, H, mode, seed, base_seed, what):
    """bank.forecast(H, seed=seed) against singles[f].forecast(H, seed=(seed or base_seed) + f)."""
    F, P = len(singles), bank.num_particles
    fb = bank.forecast(H, mode=mode, particles=True, seed=seed)
    assert fb.class_probabilities.shape == (F, H, bank.num_classes) and fb.state_mean.shape == (F, H, m.d)
    assert fb.observation_mean.shape == fb.observation_spread.shape == (F, H, m.D)
    assert fb.states.shape == (F, H, P, m.d) and fb.classes.shape == (F, H, P) and fb.classes.dtype == torch.int64
    assert all(getattr(fb, k).is_contiguous() for k in FC_FIELDS)
    for f, pf in enumerate(singles):
        fs = pf.forecast(H, mode=mode, particles=True, seed=(base_seed if seed is None else seed) + f)
        same(row(fb, f, FC_FIELDS), fs, FC_EXACT, (what, f))
        _check_state_mean(fb, f, fs.state_mean, what)
    return fb


@pytest.mark.parametrize("cfg,F,P,resample", SHAPES)
def test_bank_forecast_equals_single_filters(request, cfg, F, P, resample):
    """After 0 and after 3 updates, H = 3, sample and mean mode, pose and particles on."""
    m, fx = _model(request, cfg)
    bank, singles = bank_and_singles(m, torch.tensor(fx["T"]), F, P, resample, seed=500)
    for updates in (0, 3):
        for k in range(updates):
            update_all(bank, singles, frame_z(fx, F, k))
        for mode in ("sample", "mean"):
            _against_singles(bank, singles, m, 3, mode, None, 500, (cfg, F, P, updates, mode))


@pytest.mark.parametrize("cfg,F,P,resample", SHAPES)
def test_prefix_seed_and_reproducibility(request, cfg, F, P, resample):
    """forecast(2) is the first two rows of forecast(5) (state_mean included: it does not depend
    on H); an explicit seed s equals the singles' seed s + f; two calls give the same bits; the
    outputs do not depend on which of them are asked for."""
    m, fx = _model(request, cfg)
    bank, singles = bank_and_singles(m, torch.tensor(fx["T"]), F, P, resample, seed=500)
    for k in range(3):
        update_all(bank, singles, frame_z(fx, F, k))
    a = bank.forecast(5, particles=True)
    same(a, bank.forecast(5, particles=True), FC_FIELDS, "twice")
    short = bank.forecast(2, particles=True)
    for k in FC_FIELDS:
        assert np.array_equal(getattr(a, k)[:, :2].numpy(), getattr(short, k).numpy()), k
    bare = bank.forecast(5, observation=False)
    assert bare.observation_mean is None and bare.states is None and bare.classes is None
    same(a, bare, ("class_probabilities", "state_mean"), "bare")
    explicit = _against_singles(bank, singles, m, 3, "sample", 9000, 500, (cfg, "seed"))
    assert not np.array_equal(explicit.states.numpy(), a.states[:, :3].numpy())
    same(a, bank.forecast(5, particles=True, seed=500), FC_FIELDS, "the bank's own seed")


@pytest.mark.parametrize("d,D,C", [(13, 17, 2), (3, 20, 9)])
def test_odd_model_shapes(d, D, C):
    """Odd d and odd C (the `j + 1 < d` and `j + 1 < C` draw pairs; nine classes: two dynamics
    launches per step and, at 77 particles, classes that are empty in some filters only)."""
    F, P = 3, 77
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=30, S=3, seed=50 + d)
    bank, singles = bank_and_singles(m, T, F, P, seed=3)
    for k in range(2):
        update_all(bank, singles, np.stack([Y[40 + k + 5 * f] for f in range(F)]))
    for mode in ("sample", "mean"):
        fb = _against_singles(bank, singles, m, 3, mode, None, 3, (d, D, C, mode))
    counts = np.stack([[np.bincount(fb.classes[f, h].numpy(), minlength=C) for h in range(3)] for f in range(F)])
    assert np.array_equal(fb.class_probabilities.numpy(), counts / np.float64(P))


def test_steps_against_the_oracle(m2, fx_config2):
    """Config 2, F = 2, Pf = 1500 after two updates: each filter's rows against the oracle,
    resynced step by step, with the forecast draws of forecast_ref keyed seed + f."""
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P, seed = fx_config2, 2, 1500, 17
    om = oracle_model(fx)
    bank = GPMDM_PF_Bank(m2, torch.tensor(fx["T"]), F, P, seed=seed)
    for k in range(2):
        bank.update(frame_z(fx, F, k))
    st = bank.export_state()
    for mode in ("sample", "mean"):
        fc = bank.forecast(3, mode=mode, particles=True)
        for f in range(F):
            stf = dict(states=st["states"][f], classes=st["classes"][f], frame=st["frame"])
            TF._check_rows(row(fc, f, FC_FIELDS), stf, om, fx["T"], seed + f, mode, ("bank", f, mode))


def test_forecast_leaves_the_bank_unchanged(m1, fx_config1):
    """A bank that forecasts after construction and after every frame is, export and read-outs,
    bitwise a bank that never did (a pre-switch is pending behind each call)."""
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P = fx_config1, 5, 100
    out = []
    for look in (False, True):
        bank = GPMDM_PF_Bank(m1, torch.tensor(fx["T"]), F, P, seed=19)
        frames = []
        if look:
            bank.forecast(3)
        for k in range(3):
            bank.update(frame_z(fx, F, k))
            if look:
                bank.forecast(3, particles=True)
                bank.forecast(2, mode="mean")
            frames.append((bank.export_state(), bank.class_probabilities().numpy(), bank.current_state_mean().numpy(),
                           bank.log_likelihood().numpy(), [t.numpy() for t in bank.current_observation()]))
        out.append((frames, bank.health()))
    (a, ha), (b, hb) = out
    assert ha == hb
    for k in range(3):
        for key in KEYS:
            assert np.array_equal(a[k][0][key], b[k][0][key]), (k, key)
        for i in (1, 2, 3):
            assert np.array_equal(a[k][i], b[k][i]), (k, i)
        assert all(np.array_equal(x, y) for x, y in zip(a[k][4], b[k][4])), k


def test_sharded_bank_is_rank_invariant(m1, fx_config1):
    """shard=(3, r) banks of F = 5 give, for their filters, bitwise the rows of the full bank,
    state_mean included, with the default and with an explicit seed."""
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P = fx_config1, 5, 100
    T = torch.tensor(fx["T"])
    full = GPMDM_PF_Bank(m1, T, F, P, seed=9)
    parts = [GPMDM_PF_Bank(m1, T, F, P, seed=9, shard=(3, r)) for r in range(3)]
    for k in range(3):
        Z = frame_z(fx, F, k)
        for b in [full] + parts:
            b.update(Z)
    for kw in (dict(), dict(mode="mean"), dict(seed=4321)):
        a = full.forecast(3, particles=True, **kw)
        for p in parts:
            lo, hi = p.filter_range
            b = p.forecast(3, particles=True, **kw)
            for k in FC_FIELDS:
                assert np.array_equal(getattr(a, k)[lo:hi].numpy(), getattr(b, k).numpy()), (kw, lo, k)
