"""Gating inside ``update`` (``GPMDM_PF(gate=k)``, gpmdm_pf_set_gate / gpmdm_pf_gate_report):
csrc/obs_gate.h.

References: tests/gate_ref.py (np.longdouble) on the oracle's ``map_x_to_y(states)[0]`` of the
propagated cloud and the device's own ``variance_common``; the *masked twin*, the same filter
without the gate whose last frame is ``update(z, observed=used)``; and, where nothing is gated,
the filter with ``predictive=True`` and no gate, bit for bit.

Bounds: ll against either reference ``nrel < 1e-5`` over the finite entries and the weights 1e-5
absolute -- the suite's bounds for ll and weights (tests/test_gpu_obs_mask.py,
conftest.assert_step_matches) -- with identical NaN positions.  Every decision is checked to be
out of reach of the device's z-score error first: from tests/innov_ref.py on the ungated twin's
cloud, each z-score the test wants rejected clears the threshold by at least 1 and each it wants
kept stays at least 1 below, while the device's z-score bound (``b_zs`` in
tests/test_gpu_innovation.py) is of order 1e-8.
"""
import math

import numpy as np
import pytest
import torch

import gate_ref as G
import innov_ref as R
from conftest import nrel, oracle_model, product_model, synthetic_model

pytestmark = pytest.mark.gpu

KEYS = ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame")
ROWS = (200, 201, 202)          # test_it_sees_a_corrupted_joint's: stepped on two, the third is scored


def il2_of(m):
    return (torch.exp(m._host("y_log_lambdas")) ** -2).numpy().astype(np.float64).reshape(-1)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def readouts(pf):
    return [pf.class_probabilities().numpy(), pf.current_state_mean().numpy(), np.float64(pf.log_likelihood()),
            *(t.numpy() for t in pf.current_observation())]


def report_equal(a, b):
    return all(same(x.numpy() if hasattr(x, "numpy") else x, y.numpy() if hasattr(y, "numpy") else y)
               for x, y in zip(a, b))


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


@pytest.fixture(scope="module")
def om2(fx_config2):
    return oracle_model(fx_config2)


def make(m, T, P, torch_seed=3, **kw):
    from gpmdm_amd import GPMDM_PF
    torch.manual_seed(torch_seed)                   # (the initial cloud is drawn from torch's generator)
    kw.setdefault("rng", "philox")
    if kw["rng"] == "philox":
        kw.setdefault("seed", 5)
    return GPMDM_PF(m, T, P, **kw)


def reference_cloud(m, om, T, P, warm, z_clean, il2, mu_scale=1.0, **kw):
    """The ungated predictive twin stepped on ``warm`` and then ``z_clean``: its propagated cloud's
    oracle means, the device's vc, and innov_ref on the clean frame (the variance does not see z)."""
    tw = make(m, T, P, predictive=True, **kw)
    for z in warm:
        tw.update(z)
    tw.update(z_clean)
    inn = tw.innovation(particles=True)
    mu = mu_scale * f64(om.map_x_to_y(inn.states.numpy())[0])
    vc = inn.variance_common.numpy()
    return mu, vc, R.innovation(mu, vc, z_clean, None, il2)


def check_decisive(ref, obs, want, k, lo, hi, what):
    """From the reference: the joints in ``want`` have |z| > hi, every other observed one |z| < lo."""
    zs = np.abs(f64(ref.zscore))
    obs = np.ones(zs.shape[0], bool) if obs is None else np.asarray(obs, bool)
    keep = obs & ~want
    print(f"{what}: k {k}, kept max |z| {float(np.max(zs[keep], initial=0.0)):.3f}, "
          f"rejected min |z| {float(np.min(zs[want], initial=np.inf)):.3f}")
    assert lo <= k <= hi
    assert np.all(zs[keep] < lo), (what, float(np.max(zs[keep])))
    assert np.all(zs[want] > hi), (what, float(np.min(zs[want])))


def check_gated_frame(pf, m, om, T, P, warm, z, obs, want, il2, what, mu_scale=1.0, limit=0.5, twin=True, **kw):
    """After ``pf.update(z[, observed=obs])`` gated ``want``: the report, ll against gate_ref and
    against the masked twin, the weights, the NaN positions and the resample's source."""
    D = il2.shape[0]
    obs_b = np.ones(D, bool) if obs is None else np.asarray(obs, bool)
    used = obs_b & ~want
    rep = pf.gate_report()
    inn = pf.innovation(particles=True)
    assert same(rep.gated.numpy(), want) and same(rep.exceeded.numpy(), want), (what, rep.gated.numpy().nonzero())
    assert same(rep.used.numpy(), used) and rep.overflow is False and rep.n_gated == int(want.sum()), what
    assert same(rep.zscore.numpy(), inn.zscore.numpy()), what         # bitwise innovation()'s
    assert same(inn.observed.numpy(), obs_b), what                    # (the caller's mask, not the gate's)
    assert rep.n_valid == int(inn.n_valid), what
    ex, gated, used_r, overflow = G.decide(rep.zscore.numpy(), obs, rep.threshold, limit)
    assert same(gated, want) and same(used_r, used) and not overflow, what
    st = pf.export_state()
    ll, w = st["ll"], st["w"]
    vc = inn.variance_common.numpy()
    mu = mu_scale * f64(om.map_x_to_y(inn.states.numpy())[0])
    ref = f64(G.reweigh(mu, vc, np.where(obs_b, z, 0.0), used, il2))
    ok = vc > 0
    assert same(np.isnan(ll), ~ok) and same(np.isnan(ref), ~ok), what
    e_ref = nrel(ll[ok], ref[ok])
    print(f"{what}: ll vs gate_ref nrel {e_ref:.3e}")
    assert e_ref < 1e-5, (what, e_ref)
    assert same(st["states"], inn.states.numpy()[st["resample_idx"]]), what
    if not twin:
        return rep, st
    tw = make(m, T, P, predictive=True, **kw)
    for zz in warm:
        tw.update(zz)
    tw.update(z, observed=used)
    ts = tw.export_state()
    assert same(np.isnan(ts["ll"]), np.isnan(ll)) and same(np.isnan(ts["w"]), np.isnan(w)), what
    e_ll, e_w = nrel(ll[ok], ts["ll"][ok]), float(np.max(np.abs(w[ok] - ts["w"][ok])))
    print(f"{what}: vs masked twin ll nrel {e_ll:.3e}, w abs {e_w:.3e}")
    assert e_ll < 1e-5 and e_w < 1e-5, (what, e_ll, e_w)
    return rep, st


# ---- 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1000, 1500])
def test_corrupted_joint(m2, om2, fx_config2, P):
    """P = 1000: the deferred finish, flushed; P = 1500: k_obs_ll and its block maxima, several
    tiles with a partial last one."""
    T = torch.tensor(fx_config2["T"])
    Y = f64(m2.get_Y())
    il2 = il2_of(m2)
    j0, D = 17, Y.shape[1]
    warm = [Y[r] for r in ROWS[:-1]]
    mu, vc, clean = reference_cloud(m2, om2, T, P, warm, Y[ROWS[-1]], il2)
    z = Y[ROWS[-1]].copy()
    z[j0] += 10 * np.sqrt(float(clean.variance[j0]))
    want = np.arange(D) == j0
    check_decisive(R.innovation(mu, vc, z, None, il2), None, want, 6.0, 5.0, 7.0, f"corrupted P={P}")
    pf = make(m2, T, P, gate=6)
    assert pf.predictive is True and pf.gate == 6.0 and pf.gate_limit == 0.5
    for zz in warm:
        pf.update(zz)
        rep = pf.gate_report()
        assert rep.n_gated == 0 and not rep.overflow and rep.used.all()
    pf.update(z)
    check_gated_frame(pf, m2, om2, T, P, warm, z, None, want, il2, f"corrupted P={P}")


# ---- 2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,P", [(dict(rng="philox", seed=19), 3000), (dict(rng="torch"), 100),
                                  (dict(rng="philox", seed=23, obs_cutoff=True), 1500)],
                         ids=["philox3000", "torch100", "cutoff1500"])
def test_clean_streams_are_the_ungated_filter(fx_config2, kw, P):
    m = product_model(fx_config2)
    T = torch.tensor(fx_config2["T"])
    Y = f64(m.get_Y())
    off = make(m, T, P, torch_seed=12, predictive=True, **kw)
    out_off, zmax = [], 0.0
    for k in range(8):
        off.update(Y[300 + k])
        zmax = max(zmax, float(np.max(np.abs(off.innovation().zscore.numpy()))))
        out_off.append(readouts(off))
    thr = 1 + math.ceil(zmax)
    print(f"clean stream: max |z| {zmax:.3f}, threshold {thr}")
    on = make(m, T, P, torch_seed=12, gate=thr, **kw)
    for k in range(8):
        on.update(Y[300 + k])
        rep = on.gate_report()
        assert rep.n_gated == 0 and rep.overflow is False and not rep.gated.any() and rep.used.all(), k
        assert all(same(x, y) for x, y in zip(readouts(on), out_off[k])), k
    sa, sb = on.export_state(), off.export_state()
    for key in KEYS:
        assert same(sa[key], sb[key]), key
    assert on.health() == off.health() and on.frame == off.frame
    if kw.get("obs_cutoff"):
        assert on.obs_cutoff_auto() == off.obs_cutoff_auto()
        assert on.obs_cutoff_stats(reset=False) == off.obs_cutoff_stats(reset=False)


# ---- 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bad", [31, 32])
def test_the_cap(m2, om2, fx_config2, n_bad):
    """D = 62, limit 0.5: 31 shifted joints are all rejected, 32 are an overflow and the frame is
    bitwise the ungated frame on the same corrupted z."""
    P = 1500
    T = torch.tensor(fx_config2["T"])
    Y = f64(m2.get_Y())
    il2 = il2_of(m2)
    D = Y.shape[1]
    assert D == 62 and G.cap_of(0.5, D) == 31
    warm = [Y[r] for r in ROWS[:-1]]
    mu, vc, clean = reference_cloud(m2, om2, T, P, warm, Y[ROWS[-1]], il2)
    want = np.arange(D) < n_bad
    # ten standard deviations away from the cloud's mean, on the side the clean residual is on
    # (so that |z| >= 10 at every shifted joint, whatever the clean z-score)
    side = np.where(f64(clean.residual) < 0, -1.0, 1.0)
    z = Y[ROWS[-1]] + np.where(want, 10 * side * np.sqrt(f64(clean.variance)), 0.0)
    check_decisive(R.innovation(mu, vc, z, None, il2), None, want, 6.0, 5.0, 7.0, f"cap {n_bad}")
    pf = make(m2, T, P, gate=6.0, gate_limit=0.5)
    for zz in warm:
        pf.update(zz)
    pf.update(z)
    if n_bad == 31:
        rep, _ = check_gated_frame(pf, m2, om2, T, P, warm, z, None, want, il2, "cap 31")
        assert int(rep.used.sum()) == 31
        return
    rep = pf.gate_report()
    assert rep.overflow is True and rep.n_gated == 0 and not rep.gated.any() and rep.used.all()
    assert same(rep.exceeded.numpy(), want)
    off = make(m2, T, P, predictive=True)
    for zz in warm:
        off.update(zz)
    off.update(z)
    assert all(same(x, y) for x, y in zip(readouts(pf), readouts(off)))
    sa, sb = pf.export_state(), off.export_state()
    for key in KEYS:
        assert same(sa[key], sb[key]), key
    assert pf.health() == off.health()


# ---- 4 ---------------------------------------------------------------------------------------
def test_with_a_callers_mask(m2, om2, fx_config2):
    P, j0 = 1500, 17
    T = torch.tensor(fx_config2["T"])
    Y = f64(m2.get_Y())
    il2 = il2_of(m2)
    D = Y.shape[1]
    warm = [Y[r] for r in ROWS[:-1]]
    mu, vc, clean = reference_cloud(m2, om2, T, P, warm, Y[ROWS[-1]], il2)
    obs = np.ones(D, bool)
    obs[20:41] = False
    z = Y[ROWS[-1]].copy()
    z[j0] += 10 * np.sqrt(float(clean.variance[j0]))
    z[~obs] = np.nan
    z[25] = 1e30                                     # unobserved: never looked at
    want = np.arange(D) == j0
    check_decisive(R.innovation(mu, vc, np.where(obs, z, 0.0), obs, il2), obs, want, 6.0, 5.0, 7.0, "masked")
    pf = make(m2, T, P, gate=6.0)
    for zz in warm:
        pf.update(zz)
    pf.update(z, observed=obs)
    rep, _ = check_gated_frame(pf, m2, om2, T, P, warm, z, obs, want, il2, "masked")
    assert same(rep.used.numpy(), obs & ~rep.gated.numpy())
    assert same(np.isnan(rep.zscore.numpy()), ~obs)
    # a blackout frame with the gate on
    pf.update(np.full(D, np.nan), observed=np.zeros(D, bool))
    rep = pf.gate_report()
    assert rep.n_gated == 0 and rep.n_valid == 0 and rep.overflow is False
    assert not rep.used.any() and not rep.gated.any() and not rep.exceeded.any() and np.all(np.isnan(rep.zscore.numpy()))
    st = pf.export_state()
    assert np.all(st["ll"] == 0.0) and np.all(st["w"] == 1.0 / P)


# ---- 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,D", [(1, 5), (13, 17), (4, 150)])
def test_shapes(d, D):
    """D below one 16-column tile, d above 4, three column groups with a partial last one (the last
    joint sits in it); N = 180 is no multiple of the K-step; P = 200: four tiles, the last partial."""
    from oracle import gpmdm_oracle as O
    C, S, L, P = 2, 3, 30, 200
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=L, S=S, seed=50 + d)
    lp = {k: (getattr(m, k).detach().cpu().numpy() if getattr(m, k).dim() else float(getattr(m, k).detach()))
          for k in ("y_log_lengthscales", "y_log_lambdas", "y_log_sigma_n", "x_log_lengthscales",
                    "x_log_lambdas", "x_log_sigma_n", "x_log_lin_coeff")}
    om = O.OracleModel(X=m.X.detach().cpu().numpy().copy(), Y=Y, seq_lengths=[[L] * S] * C,
                       sigma_n_num_X=m.sigma_n_num_X, sigma_n_num_Y=m.sigma_n_num_Y, **lp).precompute()
    il2 = il2_of(m)
    kw = dict(torch_seed=7, seed=3)
    warm = [Y[40]]
    # the threshold from the clean twin's two frames, as in test 2
    tw = make(m, T, P, predictive=True, **kw)
    zmax = 0.0
    for zz in (Y[40], Y[41]):
        tw.update(zz)
        zmax = max(zmax, float(np.max(np.abs(tw.innovation().zscore.numpy()))))
    thr = 1 + math.ceil(zmax)
    mu, vc, clean = reference_cloud(m, om, T, P, warm, Y[41], il2, **kw)
    want = np.zeros(D, bool)
    want[[0, D - 1]] = True
    z = Y[41] + np.where(want, (2 * thr + 2) * np.sqrt(f64(clean.variance)), 0.0)
    check_decisive(R.innovation(mu, vc, z, None, il2), None, want, thr, thr - 1 + 1e-9, thr + 1, f"d={d} D={D}")
    pf = make(m, T, P, gate=thr, **kw)
    pf.update(Y[40])
    assert pf.gate_report().n_gated == 0
    pf.update(z)
    check_gated_frame(pf, m, om, T, P, warm, z, None, want, il2, f"synthetic d={d} D={D}", **kw)


# ---- 6 ---------------------------------------------------------------------------------------
def test_invalid_particles(fx_config1, monkeypatch):
    """The indefinite model and the cloud of test_gpu_innovation.py::test_invalid_particles: after a
    gated frame ll' is NaN exactly where vc <= 0 and gate_ref's elsewhere (means scaled by 9)."""
    from gpmdm_amd import model as model_mod
    f = fx_config1
    orig = model_mod._chol_inv_factor
    monkeypatch.setattr(model_mod, "_chol_inv_factor", lambda K, what: 3.0 * orig(K, what) if what == "K_y" else orig(K, what))
    bad = product_model(f)
    monkeypatch.setattr(model_mod, "_chol_inv_factor", orig)
    om = oracle_model(f)
    P, T, il2 = 1000, torch.tensor(f["T"]), il2_of(bad)
    z0 = f64(f["z"][0])
    D = z0.shape[0]

    def start(**kw):
        pf = make(bad, T, P, torch_seed=9, seed=3, **kw)
        st = pf.export_state()
        pf.load_state(st["states"] * np.where(np.arange(P) % 2, 6.0, 1.0)[:, None], st["classes"])
        return pf

    tw = start(predictive=True)
    tw.update(z0)
    inn = tw.innovation(particles=True)
    vc = inn.variance_common.numpy()
    assert 0 < int(np.sum(vc > 0)) < P
    mu = 9.0 * f64(om.map_x_to_y(inn.states.numpy())[0])
    clean = R.innovation(mu, vc, z0, None, il2)
    want = np.arange(D) == 0
    z = z0.copy()
    z[0] += 1000 * np.sqrt(float(clean.variance[0]))
    zs = np.abs(f64(R.innovation(mu, vc, z, None, il2).zscore))
    thr = 0.5 * (zs[0] + float(np.max(zs[1:])))       # midway between the shifted joint and the rest
    check_decisive(R.innovation(mu, vc, z, None, il2), None, want, thr, thr - 1, thr + 1, "indefinite")
    pf = start(gate=thr)
    pf.update(z)
    rep, st = check_gated_frame(pf, bad, om, T, P, [], z, None, want, il2, "indefinite", mu_scale=9.0, twin=False)
    assert same(np.isnan(st["ll"]), ~(vc > 0))
    assert rep.n_valid == int(pf.innovation().n_valid) == int(np.sum(vc > 0))


# ---- 7 ---------------------------------------------------------------------------------------
def test_staged_calls_and_repeatability(m2, om2, fx_config2):
    from gpmdm_amd import _lib
    lib = _lib.load()
    P, j0 = 1500, 17
    T = torch.tensor(fx_config2["T"])
    Y = f64(m2.get_Y())
    il2 = il2_of(m2)
    warm = [Y[r] for r in ROWS[:-1]]
    mu, vc, clean = reference_cloud(m2, om2, T, P, warm, Y[ROWS[-1]], il2)
    z = np.ascontiguousarray(Y[ROWS[-1]].copy())
    z[j0] += 10 * np.sqrt(float(clean.variance[j0]))

    whole = make(m2, T, P, gate=6.0)
    for zz in warm:
        whole.update(zz)
    checkpoint = whole.export_state()
    whole.update(z)
    rep_w, st_w = whole.gate_report(), whole.export_state()
    assert rep_w.n_gated == 1 and bool(rep_w.gated[j0])

    staged = make(m2, T, P, gate=6.0)
    for zz in warm:
        staged.update(zz)
    h, s = staged._h, staged._stream()
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), None, s), "propagate")
    mid = staged.gate_report()
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    staged._readout = None
    after = staged.gate_report()
    assert report_equal(mid, after) and report_equal(after, rep_w)
    st_s = staged.export_state()
    for key in KEYS:
        assert same(st_s[key], st_w[key]), key
    assert all(same(x, y) for x, y in zip(readouts(staged), readouts(whole)))

    # the same frame again from the checkpoint
    again = make(m2, T, P, torch_seed=99, gate=6.0)
    again.load_state(checkpoint["states"], checkpoint["classes"], ll=checkpoint["ll"], log_w=checkpoint["log_w"],
                     w=checkpoint["w"], resample_idx=checkpoint["resample_idx"], frame=checkpoint["frame"])
    with pytest.raises(RuntimeError):
        again.gate_report()                         # no frame weighed since the import
    again.update(z)
    st_a = again.export_state()
    for key in KEYS:
        assert same(st_a[key], st_w[key]), key
    assert report_equal(again.gate_report(), rep_w)


# ---- 8 ---------------------------------------------------------------------------------------
def test_errors_and_switches(m2, fx_config2):
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    lib = _lib.load()
    T = torch.tensor(fx_config2["T"])
    Y = f64(m2.get_Y())
    P = 300
    pf = make(m2, T, P, gate=60.0)             # (thresholds no clean frame reaches: every frame below is ungated)
    with pytest.raises(RuntimeError):               # before the first update
        pf.gate_report()
    pf.update(Y[10])
    assert pf.gate_report().threshold == 60.0 and pf.gate_report().n_gated == 0
    with pytest.raises(ValueError):
        pf.set_predictive(False)
    assert lib.gpmdm_pf_set_predictive(pf._h, 0) == _lib.GPMDM_E_STATE      # the library refuses too
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.gpmdm_pf_set_gate(pf._h, bad, 0.5) == _lib.GPMDM_E_INVALID
    for bad in (0.0, -0.1, 1.5, float("nan")):
        assert lib.gpmdm_pf_set_gate(pf._h, 6.0, bad) == _lib.GPMDM_E_INVALID
    assert pf.gate_report().threshold == 60.0       # (a refused call changes nothing)
    # mid-step
    s = pf._stream()
    _lib.check(lib.gpmdm_pf_switch(pf._h, None, None, s), "switch")
    assert lib.gpmdm_pf_set_gate(pf._h, 5.0, 0.5) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_propagate(pf._h, _lib.dptr(np.ascontiguousarray(Y[11])), None, s), "propagate")
    assert lib.gpmdm_pf_set_gate(pf._h, 5.0, 0.5) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_resample(pf._h, None, s), "resample")
    pf._readout = None
    # a new threshold invalidates the report
    pf.set_gate(50.0, 0.25)
    assert pf.gate == 50.0 and pf.gate_limit == 0.25
    with pytest.raises(RuntimeError):
        pf.gate_report()
    pf.update(Y[12])
    assert pf.gate_report().threshold == 50.0 and pf.gate_report().n_gated == 0
    # set_gate(None): the ungated frame, bit for bit
    off = make(m2, T, P, predictive=True)
    for r in (10, 11, 12):
        off.update(Y[r])
    pf.set_gate(None)
    assert pf.gate is None and pf.predictive is True
    with pytest.raises(ValueError):
        pf.gate_report()
    assert lib.gpmdm_pf_gate_report(pf._h, _lib.GateOut(), s) == _lib.GPMDM_E_INVALID
    pf.update(Y[13])
    off.update(Y[13])
    sa, sb = pf.export_state(), off.export_state()
    for key in KEYS:
        assert same(sa[key], sb[key]), key
    pf.set_predictive(False)                        # allowed again
    with pytest.raises(ValueError):
        pf.set_gate(6.0)
    assert lib.gpmdm_pf_set_gate(pf._h, 6.0, 0.5) == _lib.GPMDM_E_STATE    # the predictive switch is off
    # banks and sharded filters
    bank = GPMDM_PF_Bank(m2, T, 2, 100, seed=3, predictive=True)
    assert lib.gpmdm_pf_set_gate(bank._h, 6.0, 0.5) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_gate_report(bank._h, _lib.GateOut(), s) == _lib.GPMDM_E_INVALID
    sharded = GPMDM_PF(m2, T, 100, rng="philox", seed=2, shard=(2, 0), exchange=lambda recv, send: None,
                       predictive=True)
    assert lib.gpmdm_pf_set_gate(sharded._h, 6.0, 0.5) == _lib.GPMDM_E_INVALID
    with pytest.raises(ValueError):
        sharded.set_gate(6.0)
    with pytest.raises(ValueError):
        GPMDM_PF(m2, T, 100, rng="philox", seed=2, shard=(2, 0), exchange=lambda recv, send: None, gate=6.0)
