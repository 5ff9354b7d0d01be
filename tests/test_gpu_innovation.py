"""Per-joint innovations (``GPMDM_PF.innovation``, gpmdm_pf_innovation) and the GP's predictive
variance (``current_observation(gp_variance=True)``, gpmdm_pf_observation_gp): csrc/obs_innov.h.

The reference is tests/innov_ref.py (np.longdouble) on the oracle's ``map_x_to_y(states)[0]`` of
the propagated cloud the call exports, and on the device's own ``variance_common``.

Bounds (mu: the oracle's means, P x D; var_j: their variance over p; il2_j = lambda_j^-2):

* mean, spread: tests/test_gpu_obs_readout.py's -- ``nrel(mean) < 1e-9`` and, with
  delta = 1e-9 max|mu|, ``|spread_j - var_j| <= 4 delta sqrt(var_j) + delta^2``;
* variance_common: ``nrel < 1e-6`` against the oracle's ``map_x_to_y(states)[1][:, j] / il2_j``
  (the suite's bound for predictive variances);
* gp_variance: within ``(n 2^-53 + 2^-52)`` relative of ``il2_j fsum(vc) / n`` over the n valid
  particles (any summation order of n positive terms, one division, one product);
* variance = spread + gp_variance: the two bounds added, plus 2^-52 |variance| for the sum;
* residual = z - mean: ``delta_m = 1e-9 max|mean|`` (the mean's bound) plus 2^-52 |residual|;
* zscore = residual / sqrt(variance): first order,
  ``delta_m / sqrt(variance) + |residual| dvar / (2 variance^1.5) + 2^-50 |zscore|``
  with dvar the variance's bound;
* log_density: ``1e-5 max(1, max_j |ref|)``, the tolerance the suite holds ll (a sum of D such
  terms) to.  The bound needs well-conditioned inputs: a perturbation delta of mu_pj moves
  particle p's log term by ``s_pj = |z_j - mu_pj| delta / (vc_p il2_j)``, and the mixture's log by
  the share-weighted mean of s_pj.  ``_conditioned`` computes, from the reference alone, that
  weighted mean and the largest s_pj among the particles that carry the mixture (share >= 1e-6),
  and asserts both below 1e-6: an ill-conditioned input fails there, not behind the tolerance.
"""
import math

import numpy as np
import pytest
import torch

import innov_ref as R
from conftest import nrel, oracle_model, product_model, synthetic_model

pytestmark = pytest.mark.gpu

FIELDS = ("mean", "spread", "gp_variance", "variance", "residual", "zscore", "log_density", "n_valid", "observed")


def il2_of(m):
    return (torch.exp(m._host("y_log_lambdas")) ** -2).numpy().astype(np.float64).reshape(-1)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def same_innovation(a, b, particles=False):
    names = FIELDS + (("states", "variance_common") if particles else ())
    return [n for n in names if not same(getattr(a, n).numpy(), getattr(b, n).numpy())]


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


@pytest.fixture(scope="module")
def om2(fx_config2):
    return oracle_model(fx_config2)


def _conditioned(ref, mu, vc, z, il2, observed, what):
    """The log_density bound's precondition, from the reference alone (module docstring)."""
    delta = 1e-9 * np.max(np.abs(mu))
    valid = vc > 0
    obs = np.ones(mu.shape[1], bool) if observed is None else np.asarray(observed, bool)
    zz = np.where(obs, z, 0.0)
    s = np.abs(zz[None, :] - mu[valid]) * delta / (vc[valid][:, None] * il2[None, :])
    share = np.exp(np.asarray(ref.elem[valid] - (ref.log_density + np.log(R.LD(ref.n_valid)))[None, :], dtype=np.float64))
    share, s = share[:, obs], s[:, obs]
    weighted = float(np.max(np.sum(share * s, axis=0)))
    carriers = float(np.max(np.where(share >= 1e-6, s, 0.0)))
    print(f"{what}: log_density sensitivity weighted {weighted:.3e}, carriers {carriers:.3e}")
    assert np.allclose(share.sum(0), 1.0, rtol=1e-9), what          # (the shares are a partition)
    assert weighted < 1e-6 and carriers < 1e-6, (what, weighted, carriers)


def check_against_reference(inn, om, il2, z, observed, what, oracle_vc=True, mu_scale=1.0):
    """Every field of ``inn`` (taken with particles=True) against innov_ref; returns the reference.
    ``mu_scale``: the factor between the product model's K_y^-1 and the oracle's (the indefinite
    model: beta = K_y^-1 Y, so the means, scale with it)."""
    st, vc = inn.states.numpy(), inn.variance_common.numpy()
    P, D = st.shape[0], il2.shape[0]
    mu, var_o = om.map_x_to_y(st)
    mu = mu_scale * np.asarray(mu, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    ref = R.innovation(mu, vc, z, observed, il2)
    f = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    obs = np.ones(D, bool) if observed is None else np.asarray(observed, bool)
    assert same(inn.observed.numpy(), obs), what
    assert int(inn.n_valid) == ref.n_valid, (what, int(inn.n_valid), ref.n_valid)
    mean, spread = inn.mean.numpy(), inn.spread.numpy()
    print(f"{what}: mean nrel {nrel(mean, f(ref.mean)):.3e}")
    assert nrel(mean, f(ref.mean)) < 1e-9, (what, nrel(mean, f(ref.mean)))
    delta = 1e-9 * np.max(np.abs(mu))
    b_spread = 4 * delta * np.sqrt(f(ref.spread)) + delta ** 2
    assert np.all(spread >= 0) and np.all(np.abs(spread - f(ref.spread)) <= b_spread), what
    if oracle_vc and ref.n_valid == P:
        e = nrel(vc, np.asarray(var_o, dtype=np.float64)[:, 0] / il2[0])
        print(f"{what}: variance_common nrel {e:.3e}")
        assert e < 1e-6, (what, e)
    for name in ("residual", "zscore", "log_density"):
        assert same(np.isnan(getattr(inn, name).numpy()), ~obs | (name != "residual" and ref.n_valid == 0)), (what, name)
    if ref.n_valid == 0:
        for name in ("gp_variance", "variance"):
            assert np.all(np.isnan(getattr(inn, name).numpy())), (what, name)
        return ref
    n = ref.n_valid
    gpv, var = inn.gp_variance.numpy(), inn.variance.numpy()
    b_gpv = (n * 2.0 ** -53 + 2.0 ** -52) * f(ref.gp_variance)
    assert np.all(np.abs(gpv - f(ref.gp_variance)) <= b_gpv), (what, float(np.max(np.abs(gpv / f(ref.gp_variance) - 1))))
    b_var = b_spread + b_gpv + 2.0 ** -52 * f(ref.variance)
    assert np.all(np.abs(var - f(ref.variance)) <= b_var), what
    d_m = 1e-9 * np.max(np.abs(f(ref.mean)))
    res, zs, ld = (getattr(inn, k).numpy()[obs] for k in ("residual", "zscore", "log_density"))
    r_res, r_zs, r_ld, r_var = f(ref.residual)[obs], f(ref.zscore)[obs], f(ref.log_density)[obs], f(ref.variance)[obs]
    assert np.all(np.abs(res - r_res) <= d_m + 2.0 ** -52 * np.abs(r_res)), what
    b_zs = d_m / np.sqrt(r_var) + np.abs(r_res) * b_var[obs] / (2 * r_var ** 1.5) + 2.0 ** -50 * np.abs(r_zs)
    assert np.all(np.abs(zs - r_zs) <= b_zs), (what, float(np.max(np.abs(zs - r_zs) - b_zs)))
    if obs.any():
        _conditioned(ref, mu, vc, z, il2, observed, what)
        tol = 1e-5 * max(1.0, float(np.max(np.abs(r_ld))))
        err = float(np.max(np.abs(ld - r_ld)))
        print(f"{what}: log_density err {err:.3e} (bound {tol:.3e}), max |ref| {float(np.max(np.abs(r_ld))):.3f}")
        assert err <= tol, (what, err, tol)
    return ref


def check_same_code_same_bits(pf, inn, make_twin, what):
    """The propagated cloud is the resample's source, mean / spread are the pose read-out's bits on
    it, and a second call repeats the first."""
    st = pf.export_state()
    assert same(st["states"], inn.states.numpy()[st["resample_idx"]]), what
    twin = make_twin()
    twin.load_state(inn.states.numpy(), np.zeros(inn.states.shape[0], dtype=np.int64))
    mean, spread = twin.current_observation()
    assert same(mean.numpy(), inn.mean.numpy()) and same(spread.numpy(), inn.spread.numpy()), what
    assert same_innovation(inn, pf.innovation(particles=True), particles=True) == [], what


def check_posterior(pf, inn, il2, what):
    """current_observation(gp_variance=True): the gathered vc of the resampled cloud."""
    plain = pf.current_observation()
    mean, spread, gpv = pf.current_observation(gp_variance=True)
    assert same(mean.numpy(), plain[0].numpy()) and same(spread.numpy(), plain[1].numpy()), what
    assert len(pf.current_observation(spread=False, gp_variance=True)) == 2
    vc = inn.variance_common.numpy()[pf.export_state()["resample_idx"]]
    vc = vc[vc > 0]
    ref = np.asarray(il2.astype(R.LD) * (R.LD(math.fsum(vc)) / len(vc)), dtype=np.float64) if len(vc) else None
    if ref is None:
        assert np.all(np.isnan(gpv.numpy())), what
        return
    assert np.all(np.abs(gpv.numpy() - ref) <= (len(vc) * 2.0 ** -53 + 2.0 ** -52) * ref), what


@pytest.mark.parametrize("P", [1, 33, 777, 1500])
def test_definitions_config2(m2, om2, fx_config2, P):
    """N = 2000, D = 62, d = 3: a single particle, a partial tile, several tiles with a partial last
    one; P <= 1024 takes the deferred finish inside the one-workgroup resample, 1500 k_obs_ll."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    torch.manual_seed(100 + P)                      # (the initial cloud is drawn from torch's generator)
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=7, predictive=True)
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    r0 = 200
    if P == 1:
        # one particle cannot track from a random start; it starts at the latent of the row before
        # its frames, inside a sequence (the conditioning of log_density asks for a particle near
        # the observation: 1.6e-7 from row 700, 1.0e-6 across the sequence boundary at row 200)
        r0 = 701
        pf.load_state(np.asarray(fx_config2["X"][r0 - 1:r0], dtype=np.float64), np.zeros(1, dtype=np.int64))
    for k in range(2):
        pf.update(Y[r0 + k])
    inn = pf.innovation(particles=True)
    il2 = il2_of(m2)
    check_against_reference(inn, om2, il2, Y[r0 + 1], None, f"config2 P={P}")
    check_same_code_same_bits(pf, inn, lambda: GPMDM_PF(m2, T, P, rng="philox", seed=1), f"config2 P={P}")
    check_posterior(pf, inn, il2, f"config2 P={P}")
    plain = pf.innovation()
    assert plain.states is None and plain.variance_common is None and same_innovation(plain, inn) == []


@pytest.mark.parametrize("d,D", [(1, 5), (13, 17), (4, 150)])
def test_definitions_shapes(d, D):
    """D below one 16-column tile, d above 4, three column groups with a partial last one; N = 180
    is no multiple of the 16-row K-step; P = 200: four tiles, the last partial."""
    from gpmdm_amd import GPMDM_PF
    from oracle import gpmdm_oracle as O
    C, S, L, P = 2, 3, 30, 200
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=L, S=S, seed=50 + d)
    lp = {k: (getattr(m, k).detach().cpu().numpy() if getattr(m, k).dim() else float(getattr(m, k)))
          for k in ("y_log_lengthscales", "y_log_lambdas", "y_log_sigma_n", "x_log_lengthscales",
                    "x_log_lambdas", "x_log_sigma_n", "x_log_lin_coeff")}
    om = O.OracleModel(X=m.X.detach().cpu().numpy().copy(), Y=Y, seq_lengths=[[L] * S] * C,
                       sigma_n_num_X=m.sigma_n_num_X, sigma_n_num_Y=m.sigma_n_num_Y, **lp).precompute()
    torch.manual_seed(7)
    pf = GPMDM_PF(m, T, P, rng="philox", seed=3, predictive=True)
    for k in range(2):
        pf.update(Y[40 + k])
    inn = pf.innovation(particles=True)
    il2 = il2_of(m)
    check_against_reference(inn, om, il2, Y[41], None, f"synthetic d={d} D={D}")
    check_same_code_same_bits(pf, inn, lambda: GPMDM_PF(m, T, P, rng="philox", seed=1), f"synthetic d={d} D={D}")
    check_posterior(pf, inn, il2, f"synthetic d={d} D={D}")


def test_masks(m2, om2, fx_config2):
    """Joints 20-40 NaN: NaN exactly there in the three z-dependent fields, the imputation's error
    bar finite everywhere; then a blackout frame."""
    from gpmdm_amd import GPMDM_PF
    P, D = 777, 62
    torch.manual_seed(8)
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, rng="philox", seed=11, predictive=True)
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    il2 = il2_of(m2)
    pf.update(Y[300])
    z = Y[301].copy()
    z[20:41] = np.nan
    obs = np.isfinite(z)
    pf.update(z, observed=obs)
    inn = pf.innovation(particles=True)
    check_against_reference(inn, om2, il2, z, obs, "masked")
    for name in ("residual", "zscore", "log_density"):
        assert same(np.isnan(getattr(inn, name).numpy()), ~obs), name
    for name in ("mean", "spread", "gp_variance", "variance"):
        assert np.all(np.isfinite(getattr(inn, name).numpy())), name
    check_posterior(pf, inn, il2, "masked")
    none = np.zeros(D, dtype=bool)
    pf.update(np.full(D, np.nan), observed=none)
    inn = pf.innovation(particles=True)
    assert int(inn.n_valid) == 0 and np.all(np.isnan(inn.variance_common.numpy()))
    check_against_reference(inn, om2, il2, np.zeros(D), none, "blackout")
    for name in ("gp_variance", "variance", "residual", "zscore", "log_density"):
        assert np.all(np.isnan(getattr(inn, name).numpy())), name
    assert np.all(np.isnan(pf.current_observation(gp_variance=True)[2].numpy()))


def test_invalid_particles(fx_config1, monkeypatch):
    """The indefinite model of test_health_counts_indefinite_model (K_y^-1 scaled by 9): particles
    with vc <= 0 are left out and counted, as the health counter counts them."""
    from gpmdm_amd import GPMDM_PF, model as model_mod
    f = fx_config1
    orig = model_mod._chol_inv_factor
    monkeypatch.setattr(model_mod, "_chol_inv_factor", lambda K, what: 3.0 * orig(K, what) if what == "K_y" else orig(K, what))
    bad = product_model(f)
    monkeypatch.setattr(model_mod, "_chol_inv_factor", orig)
    P = 1000
    torch.manual_seed(9)
    pf = GPMDM_PF(bad, torch.tensor(f["T"]), P, rng="philox", seed=3, predictive=True)
    # every second particle far from the training latents (k^T K_y^-1 k small: vc stays positive
    # under the scaled inverse), the others on them (vc = 1 - 9 q < 0): both kinds in one cloud
    st = pf.export_state()
    pf.load_state(st["states"] * np.where(np.arange(P) % 2, 6.0, 1.0)[:, None], st["classes"])
    before = pf.health()["obs_var_nonpositive"]
    z = np.asarray(f["z"][0], dtype=np.float64)
    pf.update(z)
    inn = pf.innovation(particles=True)
    vc = inn.variance_common.numpy()
    n_valid = int(np.sum(vc > 0))
    print(f"indefinite: n_valid {n_valid} of {P}")
    assert 0 < n_valid < P, n_valid               # (the cloud above holds both kinds)
    assert int(inn.n_valid) == n_valid
    assert P - n_valid == pf.health()["obs_var_nonpositive"] - before
    check_against_reference(inn, oracle_model(f), il2_of(bad), z, None, "indefinite", oracle_vc=False, mu_scale=9.0)


def _frames(m, T, Y, P, predictive, n=8, **kw):
    from gpmdm_amd import GPMDM_PF
    torch.manual_seed(12)
    pf = GPMDM_PF(m, T, P, predictive=predictive, **kw)
    out, inns = [], []
    for k in range(n):
        pf.update(Y[300 + k])
        if predictive:
            inns.append(pf.innovation(particles=True))
            pf.current_observation(gp_variance=True)
        out.append([pf.class_probabilities().numpy(), pf.current_state_mean().numpy(), np.float64(pf.log_likelihood()),
                    *(t.numpy() for t in pf.current_observation())])
    return pf, out, inns


@pytest.mark.parametrize("kw,P", [(dict(rng="philox", seed=19), 3000), (dict(rng="torch"), 100),
                                  (dict(rng="philox", seed=23, obs_cutoff=True), 1500)],
                         ids=["philox3000", "torch100", "cutoff1500"])
def test_invisible_to_the_filter(fx_config2, om2, kw, P):
    """Eight frames with the switch on and both calls after every frame leave the filter exactly
    where eight frames without leave it."""
    m = product_model(fx_config2)
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m.get_Y(), dtype=np.float64)
    on, out_on, inns = _frames(m, T, Y, P, True, **kw)
    off, out_off, _ = _frames(m, T, Y, P, False, **kw)
    for k, (a, b) in enumerate(zip(out_on, out_off)):
        assert all(same(x, y) for x, y in zip(a, b)), k
    sa, sb = on.export_state(), off.export_state()
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert same(sa[key], sb[key]), key
    assert on.health() == off.health() and on.frame == off.frame
    if kw.get("obs_cutoff"):
        # the cutoff kernel's vc (split tiles' chains included) against the oracle
        st, vc = inns[-1].states.numpy(), inns[-1].variance_common.numpy()
        var = np.asarray(om2.map_x_to_y(st)[1], dtype=np.float64)
        e = nrel(vc, var[:, 0] / il2_of(m)[0])
        print(f"cutoff variance_common nrel {e:.3e}")
        assert e < 1e-6, e


@pytest.mark.parametrize("P", [100, 1500])
def test_between_weigh_and_resample(m2, fx_config2, P):
    """gpmdm_pf_innovation after gpmdm_pf_propagate and before gpmdm_pf_resample (P = 100: a
    pending deferred finish is flushed) returns what it returns after the resample, and the frame
    is the frame without the call."""
    from gpmdm_amd import GPMDM_PF, _lib
    from gpmdm_amd.pf import _innovation_call
    lib = _lib.load()
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    states = []
    for peek in (True, False):
        torch.manual_seed(4)                        # (the initial cloud is drawn from torch's generator)
        pf = GPMDM_PF(m2, T, P, rng="philox", seed=31, predictive=True)
        h, s = pf._h, pf._stream()
        for k in range(3):
            z = np.ascontiguousarray(Y[400 + k])
            _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
            _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), None, s), "propagate")
            mid = _innovation_call(pf, "gpmdm_pf_innovation", (), True) if peek else None
            with pytest.raises(RuntimeError):       # the posterior needs the resample
                _lib.check(lib.gpmdm_pf_observation_gp(h, None, s), "observation_gp")
            _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
            pf._readout = None
            if peek:
                assert same_innovation(mid, pf.innovation(particles=True), particles=True) == [], k
        states.append((pf.export_state(), pf.class_probabilities().numpy(), pf.log_likelihood(), pf.health()))
    (sa, pa, la, ha), (sb, pb, lb, hb) = states
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert same(sa[key], sb[key]), key
    assert same(pa, pb) and la == lb and ha == hb


CLEAN_ROWS = (200, 201, 202)   # the filter is stepped on the first two, the third is scored


def test_it_sees_a_corrupted_joint(m2, om2, fx_config2):
    """One joint shifted by ten standard deviations (of the clean frame's reference variance) is
    the largest |zscore| and the smallest log_density; non-vacuous because the clean frame's
    largest reference |zscore| is below 5 (asserted; 3.7 on these rows and seeds)."""
    from gpmdm_amd import GPMDM_PF
    P, j0 = 1000, 17
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    il2 = il2_of(m2)

    def run(z):
        torch.manual_seed(3)                        # (the initial cloud is drawn from torch's generator)
        pf = GPMDM_PF(m2, T, P, rng="philox", seed=5, predictive=True)
        for r in CLEAN_ROWS[:-1]:
            pf.update(Y[r])
        pf.update(z)
        return pf.innovation(particles=True)

    clean = run(Y[CLEAN_ROWS[-1]])
    ref = check_against_reference(clean, om2, il2, Y[CLEAN_ROWS[-1]], None, "clean")
    zmax = float(np.max(np.abs(np.asarray(ref.zscore, dtype=np.float64))))
    print(f"clean frame: max |zscore| {zmax:.3f}")
    assert zmax < 5, zmax
    z = Y[CLEAN_ROWS[-1]].copy()
    z[j0] += 10 * np.sqrt(float(ref.variance[j0]))
    bad = run(z)
    assert same(bad.states.numpy(), clean.states.numpy())         # (the propagated cloud does not see z)
    assert int(np.argmax(np.abs(bad.zscore.numpy()))) == j0
    assert int(np.argmin(bad.log_density.numpy())) == j0


def test_errors(m2, fx_config2):
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    off = GPMDM_PF(m2, T, 100, rng="philox", seed=2)
    off.update(Y[10])
    with pytest.raises(ValueError):
        off.innovation()
    with pytest.raises(ValueError):
        off.current_observation(gp_variance=True)
    assert len(off.current_observation()) == 2
    pf = GPMDM_PF(m2, T, 100, rng="philox", seed=2, predictive=True)
    with pytest.raises(RuntimeError):           # no frame weighed yet
        pf.innovation()
    pf.update(Y[10])
    pf.innovation()
    pf.reset()
    with pytest.raises(RuntimeError):
        pf.innovation()
    with pytest.raises(RuntimeError):
        pf.current_observation(gp_variance=True)
    pf.update(Y[10])
    pf.innovation()
    pf.set_predictive(False)
    pf.update(Y[11])
    with pytest.raises(ValueError):
        pf.innovation()
    pf.set_predictive(True)
    with pytest.raises(RuntimeError):           # switched on: the last frame kept nothing
        pf.innovation()
    sharded = GPMDM_PF(m2, T, 100, rng="philox", seed=2, shard=(2, 0), exchange=lambda recv, send: None,
                       predictive=True)
    with pytest.raises(ValueError):
        sharded.innovation()
