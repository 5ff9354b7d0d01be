"""Masked observations (``GPMDM_PF.update(z, observed=...)``, gpmdm_pf_set_obs_mask): missing
joints.

The reference for a masked frame is the oracle itself on the *restricted model*: a shallow
copy of ``conftest.oracle_model(fx)`` with ``Y = Y[:, obs]`` and ``y_log_lambdas =
y_log_lambdas[obs]`` (``Ky_inv`` and the dynamics members are shared: the observation kernel
matrix depends on the latents only, so nothing is recomputed).  ``gpmdm_oracle.step`` on it
is the reference's likelihood (gpmdm_pf.py:170-192), float32 constant included, at D_obs
dimensions.  Tolerances are ``conftest.assert_step_matches``'s own.

The config-2 fixture (N = 2000) puts the 62 mean columns across two 512-column blocks of the
observation image, so both likelihood partials are live.  P = 300 takes the deferred
small-filter finish (k_small_resample), P = 5000 the multi-kernel path with a partial last
tile.  ``z`` carries NaN at every missing position throughout.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_step_matches, nrel, oracle_model, product_model

pytestmark = pytest.mark.gpu

D2 = 62


def _masks(D):
    j = np.arange(D)
    return {
        "every_third_missing": j % 3 != 2,
        "first_tile_missing": j >= 16,            # joints 0-15: a whole 16-column mean tile
        "first_tile_only": j < 16,                # joints 16-61 missing
        "one_joint": j == 37,
    }


MASKS = _masks(D2)


@pytest.fixture(scope="module")
def m2c(fx_config2):
    m = product_model(fx_config2)
    m.enable_obs_cutoff(True)                      # dense filters on it run the dense kernel
    return m


@pytest.fixture(scope="module")
def om2(fx_config2):
    return oracle_model(fx_config2)


def restricted(om, obs):
    o = copy.copy(om)
    o.Y = om.Y[:, obs]
    o.y_log_lambdas = np.asarray(om.y_log_lambdas)[obs]
    return o


def _draws(seed, frame, P, C, d, resample="multinomial"):
    from oracle import philox as X
    E = X.switch_draws(seed, frame, P, C, 0)
    nrm = X.dynamics_normals(seed, frame, P, d, 0)
    u = X.resample_uniforms(seed, frame, P, 0) if resample == "multinomial" else X.systematic_u0(seed, frame, 0)
    return E, nrm, u


def _oracle_step(om, T, pre, z, seed, frame):
    from oracle import gpmdm_oracle as O
    P, C, d = pre["states"].shape[0], T.shape[0], pre["states"].shape[1]
    E, nrm, u = _draws(seed, frame, P, C, d)
    return O.step(om, T, pre["states"], pre["classes"], z, E, nrm, u, normals_by_particle=True), u


def _with_nan(z, obs):
    z = np.array(z, dtype=np.float64)
    z[~obs] = np.nan
    return z


def _masked_steps(pf, om, T, Y, obs, seed, what, n_steps=2):
    """One masked warm-up frame, then resynced masked steps against the restricted oracle."""
    omr = restricted(om, obs)
    pf.update(_with_nan(Y[10], obs), observed=obs)
    for k in range(n_steps):
        pre = pf.export_state()
        frame = pf.frame
        z = _with_nan(Y[11 + k] + 0.01, obs)
        pf.update(z, observed=np.isfinite(z))      # the documented idiom
        post = pf.export_state()
        r, u = _oracle_step(omr, T, pre, z[obs], seed, frame)
        assert_step_matches(post, r, pf.class_probabilities().numpy(), pf.current_state_mean().numpy(), u,
                            "multinomial", (what, k))
        assert pf.health() == {k2: 0 for k2 in pf.health()}, (what, k)


@pytest.mark.parametrize("P", [300, 5000])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_masked_philox_steps_vs_restricted_oracle(m2c, om2, fx_config2, mask, P):
    from gpmdm_amd import GPMDM_PF
    T = np.asarray(fx_config2["T"], dtype=np.float64)
    pf = GPMDM_PF(m2c, torch.tensor(T), P, rng="philox", seed=17)
    _masked_steps(pf, om2, T, m2c.get_Y(), MASKS[mask], 17, (mask, P))


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_masked_cutoff_steps(m2c, om2, fx_config2, mask):
    """The cutoff kernel with a mask: against the restricted oracle, then against the dense
    masked filter from the same loaded state (test_cutoff_vs_dense_same_state's 1e-5 normwise
    bound on ll)."""
    from gpmdm_amd import GPMDM_PF
    T = np.asarray(fx_config2["T"], dtype=np.float64)
    P, obs, Y = 5000, MASKS[mask], m2c.get_Y()
    cut = GPMDM_PF(m2c, torch.tensor(T), P, rng="philox", seed=17, obs_cutoff=True)
    _masked_steps(cut, om2, T, Y, obs, 17, (mask, "cutoff"))
    st = cut.export_state()
    dense = GPMDM_PF(m2c, torch.tensor(T), P, rng="philox", seed=17)
    dense.import_state(st)
    z = _with_nan(Y[20], obs)
    cut.update(z, observed=obs)
    dense.update(z, observed=obs)
    sc, sd = cut.export_state(), dense.export_state()
    assert np.array_equal(sc["classes"], sd["classes"])
    assert nrel(sc["ll"], sd["ll"]) < 1e-5, nrel(sc["ll"], sd["ll"])
    assert nrel(sc["w"], sd["w"]) < 1e-5, nrel(sc["w"], sd["w"])


def test_masked_replay_step_with_explicit_draws(fx_config1):
    """rng='torch': one masked update_with_draws step on config 1 against the restricted
    oracle's step with the same explicit draws."""
    from gpmdm_amd import GPMDM_PF
    from oracle import gpmdm_oracle as O
    f = fx_config1
    m, om = product_model(f), oracle_model(f)
    obs = np.arange(om.D) % 3 != 2
    pf = GPMDM_PF(m, torch.tensor(f["T"]), 100, rng="torch")
    args = (f["traj_E"][0], f["traj_normals"][0], f["traj_u"][0])
    pf.load_state(f["traj_pre_states"][0], f["traj_pre_classes"][0])
    z = _with_nan(f["z"][0], obs)
    pf.update_with_draws(z, *args, observed=obs)
    r = O.step(restricted(om, obs), f["T"], f["traj_pre_states"][0], f["traj_pre_classes"][0], z[obs], *args)
    assert_step_matches(pf.export_state(), r, pf.class_probabilities().numpy(), pf.current_state_mean().numpy(),
                        f["traj_u"][0], "multinomial", "replay")
    assert pf.health() == {k: 0 for k in pf.health()}


def test_observed_none_restores_the_full_update(m2c, om2, fx_config2):
    """Frames full / masked / full: the third frame is the full update again -- bitwise the
    same whether or not the state went through an export / import resync before it, and the
    full model's oracle step."""
    from gpmdm_amd import GPMDM_PF
    T = np.asarray(fx_config2["T"], dtype=np.float64)
    P, seed, Y, obs = 1500, 23, m2c.get_Y(), MASKS["every_third_missing"]
    torch.manual_seed(8)                           # (the initial cloud)
    a = GPMDM_PF(m2c, torch.tensor(T), P, rng="philox", seed=seed)
    torch.manual_seed(8)
    b = GPMDM_PF(m2c, torch.tensor(T), P, rng="philox", seed=seed)
    for pf in (a, b):
        pf.update(Y[40])
        pf.update(_with_nan(Y[41], obs), observed=obs)
    pre = a.export_state()
    b.import_state(b.export_state())
    a.update(Y[42])
    b.update(Y[42], observed=None)
    sa, sb = a.export_state(), b.export_state()
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert np.array_equal(sa[key], sb[key]), key
    r, u = _oracle_step(om2, T, pre, np.asarray(Y[42], dtype=np.float64), seed, pre["frame"])
    assert_step_matches(sa, r, a.class_probabilities().numpy(), a.current_state_mean().numpy(), u,
                        "multinomial", "full again")


def test_mask_follows_a_rebuilt_model(fx_config1):
    """The mask's lambda^2 and scalars are the current model's: after the model's
    y_log_lambdas change in place (the filter rebinds on its next call) a frame with the same
    mask is the restricted oracle's step on the new parameters."""
    from gpmdm_amd import GPMDM_PF
    f = fx_config1
    m, om = product_model(f), oracle_model(f)
    T = np.asarray(f["T"], dtype=np.float64)
    P, seed, obs = 300, 37, MASKS["every_third_missing"]
    pf = GPMDM_PF(m, torch.tensor(T), P, rng="philox", seed=seed)
    z0 = _with_nan(f["z"][0], obs)
    pf.update(z0, observed=obs)
    shift = 0.3 * np.cos(np.arange(D2))
    with torch.no_grad():
        m.y_log_lambdas.add_(torch.as_tensor(shift, dtype=m.y_log_lambdas.dtype, device=m.y_log_lambdas.device))
    om2 = copy.copy(om)
    om2.y_log_lambdas = np.asarray(om.y_log_lambdas) + shift
    pre = pf.export_state()
    z1 = _with_nan(f["z"][1], obs)
    pf.update(z1, observed=obs)
    r, u = _oracle_step(restricted(om2, obs), T, pre, z1[obs], seed, pre["frame"])
    assert_step_matches(pf.export_state(), r, pf.class_probabilities().numpy(), pf.current_state_mean().numpy(), u,
                        "multinomial", "rebuilt model")


@pytest.mark.parametrize("P,cutoff", [(300, False), (5000, True)])
def test_blackout_is_a_prediction_step(m2c, om2, fx_config2, P, cutoff):
    """No dimension observed: w exactly 1/P, ll exactly 0, no observation kernel (the cutoff's
    work counters do not move), classes and states the oracle's switch + dynamics."""
    from gpmdm_amd import GPMDM_PF
    from oracle import gpmdm_oracle as O
    T = np.asarray(fx_config2["T"], dtype=np.float64)
    seed, Y = 29, m2c.get_Y()
    pf = GPMDM_PF(m2c, torch.tensor(T), P, rng="philox", seed=seed, obs_cutoff=cutoff)
    if cutoff:
        pf.set_obs_cutoff(True, stats=True)
    pf.update(Y[50])
    stats = pf.obs_cutoff_stats(reset=False) if cutoff else None
    pre = pf.export_state()
    frame = pf.frame
    pf.update(np.full(D2, np.nan), observed=np.zeros(D2, dtype=bool))
    post = pf.export_state()
    assert np.array_equal(post["ll"], np.zeros(P))
    assert np.array_equal(post["w"], np.full(P, 1.0 / P))
    if cutoff:
        assert stats["run"] > 0 and pf.obs_cutoff_stats(reset=False) == stats
    E, nrm, u = _draws(seed, frame, P, 2, m2c.d)
    cls1 = O.switch_classes(pre["classes"], T, E)
    st1 = O.propagate_dynamics(om2, pre["states"], cls1, np.concatenate([nrm[cls1 == c] for c in range(2)], 0))
    ll = np.zeros(P)
    log_w, w = O.normalise(ll)
    idx = O.multinomial_resample_indices(w, u)
    r = O.StepResult(cls1, st1, ll, log_w, w, idx, st1[idx], cls1[idx], O.class_probabilities(ll, log_w, cls1[idx], 2),
                     O.current_state_mean(st1[idx], w), O.log_likelihood_readout(ll, log_w))
    assert_step_matches(post, r, pf.class_probabilities().numpy(), pf.current_state_mean().numpy(), u,
                        "multinomial", ("blackout", P))
    assert pf.health() == {k: 0 for k in pf.health()}
    pf.update(Y[52])                                # and the filter goes on
    assert np.all(np.isfinite(pf.export_state()["ll"]))


def test_sharded_masked_filters_are_bitwise_one_rank(m2c):
    """A loopback devices=[0]*4 filter and a logical shard=(2, r) pair, each with a mask, are
    bitwise the one-rank masked filter."""
    from gpmdm_amd import GPMDM_PF, _lib
    T = torch.tensor([[0.9, 0.1], [0.1, 0.9]])
    P, seed, Y, obs = 4001, 31, m2c.get_Y(), MASKS["every_third_missing"]

    def make(**kw):
        torch.manual_seed(6)                        # (the initial cloud)
        return GPMDM_PF(m2c, T, P, rng="philox", seed=seed, **kw)

    ref = make()
    multi = make(devices=[0] * 4, transport="loopback")
    pair = [make(shard=(2, r)) for r in range(2)]
    blackout = np.zeros(D2, dtype=bool)
    for k, obs_k in enumerate((obs, obs, blackout, obs)):     # (a blackout frame among them)
        z = _with_nan(Y[60 + 3 * k], obs_k)
        ref.update(z, observed=obs_k)
        multi.update(z, observed=obs_k)
        for pf in pair:
            pf._set_mask(pf._check_mask(obs_k))
        full = torch.cat([pf._stage_propagate(z) for pf in pair], 0)
        for pf in pair:
            pf._recv.copy_(full)
            pf._stage_resample()
        a = ref.export_state()
        for pf in [multi] + pair:
            b = pf.export_state()
            for key in ("states", "classes", "ll", "w", "resample_idx"):
                assert np.array_equal(a[key], b[key]), (k, key)
    # ranks whose masks differ are refused
    lib = _lib.load()
    other = np.ascontiguousarray(~obs, dtype=np.uint8)
    assert lib.gpmdm_pf_set_obs_mask(multi._peers[0][0], ctypes.c_void_p(other.ctypes.data)) == 0
    multi._mask_key = None
    with pytest.raises(ValueError):
        multi._each("gpmdm_pf_switch", None, None, what="switch")
        multi._propagate(np.zeros(D2), None, multi._stream())


def test_mask_errors(m2c, fx_config2):
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = m2c.get_Y()
    pf = GPMDM_PF(m2c, T, 500, rng="philox", seed=3)
    for bad in (np.ones(D2 - 1, dtype=bool), np.ones(D2 + 1, dtype=bool), np.ones((2, D2), dtype=bool)):
        with pytest.raises(ValueError):
            pf.update(Y[0], observed=bad)
    bank = GPMDM_PF_Bank(m2c, T, 2, 300, seed=4)
    lib = _lib.load()
    flags = np.ones(D2, dtype=np.uint8)
    ptr = ctypes.c_void_p(flags.ctypes.data)
    with pytest.raises(ValueError):
        _lib.check(lib.gpmdm_pf_set_obs_mask(bank._h, ptr), "bank mask")
    # inside a step, through the staged calls
    s = pf._stream()
    assert lib.gpmdm_pf_set_obs_mask(pf._h, ptr) == _lib.GPMDM_OK      # between frames
    assert lib.gpmdm_pf_switch(pf._h, None, None, s) == _lib.GPMDM_OK
    assert lib.gpmdm_pf_set_obs_mask(pf._h, ptr) == _lib.GPMDM_E_STATE
    z = np.ascontiguousarray(Y[1], dtype=np.float64)
    assert lib.gpmdm_pf_propagate(pf._h, _lib.dptr(z), None, s) == _lib.GPMDM_OK
    assert lib.gpmdm_pf_set_obs_mask(pf._h, ptr) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_pf_set_obs_mask(pf._h, None) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_pf_resample(pf._h, None, s) == _lib.GPMDM_OK
    assert lib.gpmdm_pf_set_obs_mask(pf._h, None) == _lib.GPMDM_OK     # between frames again
    pf.update(Y[2])
    assert np.all(np.isfinite(pf.export_state()["ll"]))
