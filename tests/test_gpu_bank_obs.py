"""GPU: per-filter observation masks and the pose read-out of filter banks
(``GPMDM_PF_Bank.update(Z, observed=...)``, ``current_observation``; gpmdm_bank_set_obs_masks,
gpmdm_bank_observation).

A masked bank must be bit-identical, filter by filter, to F single masked filters
(``GPMDM_PF(rng='philox', seed=seed + f).update(z, observed=mask_f)``) from the same particles:
the bank changes the schedule (tiles that mix filters read each particle's own filter's row
of lambda^2 and of z; the finish takes the three scalars from a per-filter table), not the
numbers.  One test pins the bank against the oracle on the restricted model directly
(test_gpu_obs_mask's reference), without going through the single filter.

Shapes: no P here is a multiple of 64 (nor of the 16- and 32-particle tiles), so tiles mix
filters; P <= 1024 takes the deferred finish inside k_small_resample, P = 1500 the
multi-kernel path.  On config 2 (N = 2000) the 62 mean columns straddle two column blocks, so
both S partials are live.  Filter f uses mask (f + k) % 6 on frame k: the masks differ across
the filters of a tile and change every frame; Z carries NaN at every missing position.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_step_matches, nrel, oracle_model, product_model, synthetic_model

pytestmark = pytest.mark.gpu

D2 = 62
KEYS = ("states", "classes", "ll", "w", "resample_idx")


def _masks(D):
    """test_gpu_obs_mask._masks's four, then all observed and the blackout."""
    j = np.arange(D)
    return [
        j % 3 != 2,                               # every third joint missing
        j >= 16,                                  # joints 0-15 missing: a whole 16-column mean tile
        j < 16,                                   # only joints 0-15 observed
        j == 37,                                  # one joint observed
        np.ones(D, dtype=bool),
        np.zeros(D, dtype=bool),
    ]


MASKS = _masks(D2)
BLACKOUT = 5


def _frame(fx, F, k):
    """Frame k's (Z with NaN at the missing positions, observed (F, D), mask indices)."""
    z = np.asarray(fx["z"], dtype=np.float64)
    which = [(f + k) % len(MASKS) for f in range(F)]
    obs = np.stack([MASKS[i] for i in which])
    Z = np.stack([z[(k + 7 * f) % z.shape[0]] for f in range(F)])
    return np.where(obs, Z, np.nan), obs, which


@pytest.fixture(scope="module")
def m1(fx_config1):
    return product_model(fx_config1)


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _bank_and_singles(m, fx, F, P, resample="multinomial", seed=500, **kw):
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank
    T = torch.tensor(fx["T"])
    bank = GPMDM_PF_Bank(m, T, F, P, seed=seed, resample=resample, **kw)
    st0 = bank.export_state()
    singles = []
    for f in range(F):
        pf = GPMDM_PF(m, T, P, rng="philox", seed=seed + f, resample=resample, **kw)
        pf.load_state(st0["states"][f], st0["classes"][f])
        singles.append(pf)
    return bank, singles


def _assert_same(bank, singles, what, readouts=True):
    b = bank.export_state()
    for f, pf in enumerate(singles):
        s = pf.export_state()
        for key in KEYS:
            assert np.array_equal(b[key][f], s[key]), (what, f, key)
    if readouts:
        post, mean, lik = bank.class_probabilities(), bank.current_state_mean(), bank.log_likelihood()
        for f, pf in enumerate(singles):
            assert np.array_equal(post[f].numpy(), pf.class_probabilities().numpy()), (what, f)
            assert np.array_equal(mean[f].numpy(), pf.current_state_mean().numpy()), (what, f)
            assert lik[f].item() == pf.log_likelihood(), (what, f)
    return b


SHAPES = [("config1", 5, 100, "multinomial"), ("config1", 3, 257, "systematic"),
          ("config2", 2, 1500, "multinomial"), ("config1", 1, 300, "multinomial")]


def _model(request, cfg):
    return request.getfixturevalue("m1" if cfg == "config1" else "m2"), request.getfixturevalue("fx_" + cfg)


@pytest.mark.parametrize("cfg,F,P,resample", SHAPES)
def test_masked_bank_equals_independent_masked_filters(request, cfg, F, P, resample):
    m, fx = _model(request, cfg)
    bank, singles = _bank_and_singles(m, fx, F, P, resample)
    for k in range(4):
        Z, obs, which = _frame(fx, F, k)
        bank.update(Z, observed=np.isfinite(Z))    # the documented idiom
        for f, pf in enumerate(singles):
            pf.update(Z[f], observed=obs[f])
        b = _assert_same(bank, singles, (cfg, F, P, k))
        assert bank.health() == {key: 0 for key in bank.health()}, k
        for f, i in enumerate(which):
            if i == BLACKOUT:
                assert np.array_equal(b["ll"][f], np.zeros(P)), (k, f)
                assert np.array_equal(b["w"][f], np.full(P, 1.0 / P)), (k, f)
            else:
                assert np.all(np.isfinite(b["ll"][f])), (k, f)


def test_mask_forms_and_restoration(m1, fx_config1):
    """Per-filter masks, observed=None, one (D,) mask for every filter, per-filter masks again:
    bitwise the singles given the same; the None frame is bitwise an unmasked bank's frame from
    the same imported state."""
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P = fx_config1, 3, 257
    bank, singles = _bank_and_singles(m1, fx, F, P)
    plain = GPMDM_PF_Bank(m1, torch.tensor(fx["T"]), F, P, seed=500)   # never masked
    for k, form in enumerate(("rows", "none", "one", "rows")):
        Z, obs, _ = _frame(fx, F, k)
        if form == "none":
            Z = np.nan_to_num(Z, nan=0.25)
            plain.import_state(bank.export_state())
            plain.update(Z)
            bank.update(Z, observed=None)
            for pf, z in zip(singles, Z):
                pf.update(z)
            a, b = plain.export_state(), bank.export_state()
            for key in KEYS + ("log_w", "frame"):
                assert np.array_equal(a[key], b[key]), key
        elif form == "one":
            one = MASKS[0]
            Z = np.where(one[None, :], np.nan_to_num(Z, nan=0.25), np.nan)
            bank.update(Z, observed=one)
            for pf, z in zip(singles, Z):
                pf.update(z, observed=one)
        else:
            bank.update(Z, observed=obs)
            for pf, z, o in zip(singles, Z, obs):
                pf.update(z, observed=o)
        _assert_same(bank, singles, (k, form))


def test_masked_cutoff_bank(fx_config1):
    """The cutoff kernel's tiles mix filters and run in the switch's class grouping: each
    particle reads its own filter's rows, and the finish finds an output's filter through the
    grouping.  Bitwise F single masked cutoff filters."""
    fx, F, P = fx_config1, 3, 1000
    m = product_model(fx)
    bank, singles = _bank_and_singles(m, fx, F, P, seed=700, obs_cutoff=True)
    for k in range(3):
        Z, obs, _ = _frame(fx, F, k + 3)           # (the blackout among them: filter 2, then 1, 0)
        bank.update(Z, observed=obs)
        for f, pf in enumerate(singles):
            pf.update(Z[f], observed=obs[f])
        _assert_same(bank, singles, ("cutoff", k), readouts=False)
    assert bank.health() == {key: 0 for key in bank.health()}


def _restricted(om, obs):
    o = copy.copy(om)
    o.Y = om.Y[:, obs]
    o.y_log_lambdas = np.asarray(om.y_log_lambdas)[obs]
    return o


def test_masked_bank_vs_restricted_oracle(m2, fx_config2):
    """One resynced masked step per filter against gpmdm_oracle.step on the restricted model
    (Y[:, obs], y_log_lambdas[obs]) with Philox draws keyed seed + f: conftest's own
    tolerances.  Pins the bank without the single filter."""
    from gpmdm_amd import GPMDM_PF_Bank
    from oracle import gpmdm_oracle as O
    from oracle import philox as X
    fx, F, P, seed = fx_config2, 2, 1500, 17
    om = oracle_model(fx)
    T = np.asarray(fx["T"], dtype=np.float64)
    C, d = T.shape[0], m2.d
    bank = GPMDM_PF_Bank(m2, torch.tensor(T), F, P, seed=seed)
    Z, obs, _ = _frame(fx, F, 0)
    bank.update(Z, observed=obs)                   # a masked warm-up frame
    pre, frame = bank.export_state(), bank.frame
    Z, obs, _ = _frame(fx, F, 1)
    bank.update(Z, observed=np.isfinite(Z))
    post = bank.export_state()
    probs, means = bank.class_probabilities().numpy(), bank.current_state_mean().numpy()
    for f in range(F):
        E = X.switch_draws(seed + f, frame, P, C, 0)
        nrm = X.dynamics_normals(seed + f, frame, P, d, 0)
        u = X.resample_uniforms(seed + f, frame, P, 0)
        r = O.step(_restricted(om, obs[f]), T, pre["states"][f], pre["classes"][f], Z[f][obs[f]], E, nrm, u,
                   normals_by_particle=True)
        assert_step_matches({k: post[k][f] for k in KEYS}, r, probs[f], means[f], u, "multinomial", ("bank", f))
    assert bank.health() == {key: 0 for key in bank.health()}


@pytest.mark.parametrize("cfg,F,P,resample", SHAPES)
def test_bank_pose_equals_single_filters(request, cfg, F, P, resample):
    m, fx = _model(request, cfg)
    bank, singles = _bank_and_singles(m, fx, F, P, resample)

    def same(what):
        mean, spread = (t.numpy() for t in bank.current_observation())
        assert mean.shape == spread.shape == (F, m.D)
        assert np.array_equal(bank.current_observation_mean().numpy(), mean), what
        for f, pf in enumerate(singles):
            sm, ss = (t.numpy() for t in pf.current_observation())
            assert np.array_equal(mean[f], sm), (what, f)
            assert np.array_equal(spread[f], ss), (what, f)

    same("init")
    for k in range(2):
        Z, obs, _ = _frame(fx, F, k)
        bank.update(Z, observed=obs)
        for f, pf in enumerate(singles):
            pf.update(Z[f], observed=obs[f])
    same("updated")


def test_bank_pose_vs_oracle_three_column_groups():
    """D = 150: three column groups, the last partial; every row against the oracle's
    map_x_to_y on that filter's cloud with test_gpu_obs_readout._check's two bounds (mean:
    1e-9 normwise; spread: 4 delta sqrt(var) + delta^2 with delta = 1e-9 max|mu|)."""
    from gpmdm_amd import GPMDM_PF_Bank
    from oracle import gpmdm_oracle as O
    C, S, L, d, D, F, P = 2, 3, 30, 4, 150, 3, 200
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=L, S=S, seed=54)
    lp = {k: (getattr(m, k).detach().cpu().numpy() if getattr(m, k).dim() else float(getattr(m, k)))
          for k in ("y_log_lengthscales", "y_log_lambdas", "y_log_sigma_n", "x_log_lengthscales",
                    "x_log_lambdas", "x_log_sigma_n", "x_log_lin_coeff")}
    om = O.OracleModel(X=m.X.detach().cpu().numpy().copy(), Y=Y, seq_lengths=[[L] * S] * C,
                       sigma_n_num_X=m.sigma_n_num_X, sigma_n_num_Y=m.sigma_n_num_Y, **lp).precompute()
    bank = GPMDM_PF_Bank(m, T, F, P, seed=3)
    masks = _masks(D)

    def check(what):
        st = bank.export_state()
        mean, spread = (t.numpy() for t in bank.current_observation())
        again = bank.current_observation()
        assert np.array_equal(again[0].numpy(), mean) and np.array_equal(again[1].numpy(), spread), what
        for f in range(F):
            mu = om.map_x_to_y(st["states"][f])[0]
            ref_mean, ref_var = mu.mean(0), mu.var(0)
            assert nrel(mean[f], ref_mean) < 1e-9, (what, f, nrel(mean[f], ref_mean))
            delta = 1e-9 * np.max(np.abs(mu))
            err, bound = np.abs(spread[f] - ref_var), 4 * delta * np.sqrt(ref_var) + delta ** 2
            assert np.all(spread[f] >= 0), (what, f)
            assert np.all(err <= bound), (what, f, float(np.max(err - bound)), float(np.max(err)))

    check("init")
    for k in range(2):
        obs = np.stack([masks[(f + k) % 4] for f in range(F)])
        bank.update(np.where(obs, np.stack([Y[40 + k + 5 * f] for f in range(F)]), np.nan), observed=obs)
    check("updated")


def test_bank_pose_has_no_side_effects(m1, fx_config1):
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P = fx_config1, 5, 100
    out = []
    for read in (False, True):
        bank = GPMDM_PF_Bank(m1, torch.tensor(fx["T"]), F, P, seed=19)
        if read:
            bank.current_observation()
        for k in range(6):
            Z, obs, _ = _frame(fx, F, k)
            bank.update(Z, observed=obs)
            if read:
                a, b = bank.current_observation(), bank.current_observation()
                assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a, b)), k
        out.append(bank.export_state())
    for key in KEYS + ("log_w", "frame"):
        assert np.array_equal(out[0][key], out[1][key]), key


def test_sharded_masked_bank_is_rank_invariant(m1, fx_config1):
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P = fx_config1, 7, 300
    T = torch.tensor(fx["T"])
    full = GPMDM_PF_Bank(m1, T, F, P, seed=9)
    parts = [GPMDM_PF_Bank(m1, T, F, P, seed=9, shard=(3, r)) for r in range(3)]
    for k in range(3):
        Z, obs, _ = _frame(fx, F, k)
        full.update(Z, observed=obs)
        for p in parts:
            p.update(Z, observed=obs)             # each shard takes its own rows of both
    a = full.export_state()
    pose = [t.numpy() for t in full.current_observation()]
    for p in parts:
        lo, hi = p.filter_range
        b = p.export_state()
        for key in KEYS:
            assert np.array_equal(a[key][lo:hi], b[key]), key
        for x, y in zip(pose, p.current_observation()):
            assert y.shape == (hi - lo, m1.D)
            assert np.array_equal(x[lo:hi], y.numpy())


def test_bank_obs_errors(m1, fx_config1):
    from gpmdm_amd import GPMDM_PF_Bank, _lib
    fx, F, P, D = fx_config1, 3, 100, m1.D
    T = torch.tensor(fx["T"])
    bank = GPMDM_PF_Bank(m1, T, F, P, seed=2)
    Z = np.asarray(fx["z"], dtype=np.float64)[:F]
    for shape in ((F, D - 1), (F + 1, D), (2, F, D)):
        with pytest.raises(ValueError, match="observed"):
            bank.update(Z, observed=np.ones(shape, dtype=bool))
    lib, s = _lib.load(), bank._stream()
    flags = np.ones((F, D), dtype=np.uint8)
    ptr = ctypes.c_void_p(flags.ctypes.data)
    assert lib.gpmdm_bank_set_obs_masks(bank._h, ptr) == _lib.GPMDM_OK            # between frames
    assert lib.gpmdm_pf_switch(bank._h, None, None, s) == _lib.GPMDM_OK
    assert lib.gpmdm_bank_set_obs_masks(bank._h, ptr) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_bank_set_obs_masks(bank._h, None) == _lib.GPMDM_E_STATE
    zc = np.ascontiguousarray(Z)
    assert lib.gpmdm_pf_propagate(bank._h, _lib.dptr(zc), None, s) == _lib.GPMDM_OK
    assert lib.gpmdm_bank_set_obs_masks(bank._h, ptr) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_pf_resample(bank._h, None, s) == _lib.GPMDM_OK
    assert lib.gpmdm_bank_set_obs_masks(bank._h, None) == _lib.GPMDM_OK           # between frames again
    bank.update(Z)
    assert np.all(np.isfinite(bank.export_state()["ll"]))
    # the read-out before init: a handle that holds no particles yet
    Tn = np.ascontiguousarray(T.numpy(), dtype=np.float64)
    h = ctypes.c_void_p()
    _lib.check(lib.gpmdm_bank_create(m1.handle, _lib.dptr(Tn), 2, 50, ctypes.c_uint64(1),
                                     _lib.GPMDM_RESAMPLE_MULTINOMIAL, ctypes.byref(h)), "create")
    try:
        buf = np.zeros((2, D))
        assert lib.gpmdm_bank_observation(h, _lib.dptr(buf), None, s) == _lib.GPMDM_E_STATE
    finally:
        lib.gpmdm_pf_destroy(h)
