"""``GPMDM_PF.smoothed_marginal`` (gpmdm_pf_smoothed_marginal, csrc/backsmooth.h): the marginal
backward smoother over the filter's history ring.

The reference is ``backsmooth_ref.smoothed_marginal`` on the filter's own ``export_state()`` after
every update (the root: the export before the first one), with the dynamics moments of
``model.map_x_dynamics_for_class`` on each exported cloud.  Bounds (u = 2^-53; the band (a + b G) u
is derived in backsmooth_ref.py's docstring and DESIGN.md §3.6, G and K the largest over the steps
so far, G <= 1e6 and band <= 1e-9 asserted):

* lag-0 weights: exactly 1 / P;
* ``weights[l]``: |dw_i| <= ref_i r_l + 1e-300, r_l = (a + b G) u l -- and bitwise equal to chaining
  ``backward_step`` over the same exports, which ties test_gpu_backward_step.py's scripted edge
  cases to the smoother;
* ``class_probabilities``, ``state_mean``, ``mass`` (sums S = sum_i w_i t_i): |dS| <= (r_l + (P + 2) u)
  sum_i |w_i t_i| -- the weights' band plus any order of P fp64 additions and the products;
* ``ess``, ``ess_distinct`` (mass^2 / sum m w^2): relative 4 r_l + (3 P + 8) u.

The achieved error / band of the weights is printed beside the fp64 numpy yardstick's (P <= 777).
"""
import ctypes

import numpy as np
import pytest
import torch

import backsmooth_ref as R
from conftest import product_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _moments(m, C):
    def f(X):
        mom = [m.map_x_dynamics_for_class(torch.from_numpy(np.ascontiguousarray(X)), c) for c in range(C)]
        return [x[0].cpu().numpy() for x in mom], [x[1].cpu().numpy() for x in mom]
    return f


def _check(s, hist, root_has_anc, T, m, C, frame, what, yardstick):
    from gpmdm_amd import backward_step
    lags = s.lags.numpy()
    assert lags[0] == 0 and np.array_equal(s.frames.numpy(), frame - lags), what
    P = len(hist[-1]["classes"])
    ref = R.smoothed_marginal(hist, root_has_anc, T, _moments(m, C), int(lags[-1]), C)
    y64 = R.smoothed_marginal(hist, root_has_anc, T, _moments(m, C), int(lags[-1]), C, np.float64) if yardstick else None
    W = s.weights.numpy()
    assert np.all(W[0] == 1.0 / P), what
    chain = np.full(P, 1.0 / P)
    for l in lags:
        r, info = ref[l], ref[l]["info"]
        rl = R.band_rel(info, steps=l) if l else 0.0
        assert info["G"] <= 1e6 and rl <= 1e-9, (what, l, info, rl)
        assert W[l].tobytes() == chain.tobytes(), (what, l, "chained backward_step")
        tol = r["weights"] * rl + R.LD(1e-300)
        e = float((np.abs(W[l] - r["weights"]) / tol).max()) if l else 0.0      # (lag 0 is exact: above)
        ey = float((np.abs(y64[l]["weights"] - r["weights"]) / tol).max()) if yardstick and l else float("nan")
        print(f"{what} lag {l}: G {info['G']:.3g} band {rl:.2e} weights err/band {e:.3g} (fp64 numpy {ey:.3g}) "
              f"ess {float(s.ess[l]):.1f} ess_distinct {float(s.ess_distinct[l]):.1f}")
        assert e <= 1, (what, l, e)
        rr, e_src = r["rows"], hist[-1 - l]
        w_abs = np.abs(r["weights"])
        lin = rl + (P + 2) * R.U
        for c in range(C):
            bound = lin * w_abs[np.asarray(e_src["classes"]) == c].sum() + R.LD(1e-300)
            assert abs(s.class_probabilities[l, c].item() - rr["class_probabilities"][c]) <= bound, (what, l, c)
        bound = lin * (w_abs[:, None] * np.abs(np.asarray(e_src["states"], dtype=R.LD))).sum(0) + R.LD(1e-300)
        assert np.all(np.abs(s.state_mean[l].numpy() - rr["state_mean"]) <= bound), (what, l)
        assert abs(s.mass[l].item() - rr["mass"]) <= lin * w_abs.sum(), (what, l)
        assert abs(s.mass[l].item() - 1) <= 1e-9, (what, l)          # a real history loses no mass
        q = 4 * rl + (3 * P + 8) * R.U
        assert abs(s.ess[l].item() - rr["ess"]) <= q * rr["ess"], (what, l)
        assert abs(s.ess_distinct[l].item() - rr["ess_distinct"]) <= q * rr["ess_distinct"], (what, l)
        assert s.ess_distinct[l].item() <= s.ess[l].item() * (1 + 1e-12)
        if l < lags[-1]:
            src = hist[-2 - l]
            chain = backward_step(m, T, src["states"], src["classes"], e_src["states"], e_src["classes"], chain)[0].numpy()


def _same(a, b, rows=slice(None)):
    for k in ("lags", "frames", "class_probabilities", "state_mean", "mass", "ess", "ess_distinct", "weights"):
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            assert x is None and y is None, k
        else:
            assert x.numpy()[rows].tobytes() == y.numpy().tobytes(), k


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("P", [1, 33, 777, 5000])
def test_against_the_reference(m2, fx_config2, P, L):
    """One particle, a partial wave, a ragged last block, several blocks; 2 L + 3 frames, so the
    ring wraps.  Read after frame 2 (the oldest slot in reach is the cleared ring's root for
    L >= 2) and after the last frame (every slot a resample's); every lag, one lag, a range, twice
    in a row; a twin filter that is never read stays bitwise identical to the end."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Tn = np.ascontiguousarray(T.numpy(), dtype=np.float64)
    torch.manual_seed(12)                       # (the initial cloud is drawn from torch's generator)
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L)
    torch.manual_seed(12)
    twin = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L)
    Y = m2.get_Y()
    n = 2 * L + 3
    hist = [pf.export_state()]
    for k in range(1, n + 1):
        pf.update(Y[200 + k - 1])
        twin.update(Y[200 + k - 1])
        hist.append(pf.export_state())
        if k not in (2, n):
            continue
        depth = min(L, k)
        assert pf.smoothing_depth == depth
        g, fr, health = torch.get_rng_state(), pf.frame, pf.health()
        s = pf.smoothed_marginal(particles=True)
        assert torch.equal(g, torch.get_rng_state()) and pf.frame == fr and pf.health() == health
        assert s.weights.shape == (depth + 1, P) and s.class_probabilities.shape == (depth + 1, 2)
        assert s.state_mean.shape == (depth + 1, 3) and s.weights.dtype == s.ess.dtype == torch.float64
        assert s.lags.dtype == s.frames.dtype == torch.int64
        _check(s, hist[-(depth + 1):], k > L, Tn, m2, 2, k, (P, L, k), yardstick=P <= 777)
        _same(s, pf.smoothed_marginal(particles=True))
        _same(s, pf.smoothed_marginal(depth, particles=True), slice(depth, depth + 1))
        _same(s, pf.smoothed_marginal((1, depth), particles=True), slice(1, depth + 1))
        bare = pf.smoothed_marginal()
        assert bare.weights is None and bare.mass.numpy().tobytes() == s.mass.numpy().tobytes()
        with pytest.raises(ValueError, match="depth"):
            pf.smoothed_marginal(depth + 1)
    a, b = pf.export_state(), twin.export_state()
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(pf.class_probabilities().numpy(), twin.class_probabilities().numpy())
    assert pf.health() == twin.health()


def test_refusals(m2, fx_config2):
    """Smoothing off, a lag above the depth, a bank handle, a call inside a frame."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    lib = _lib.load()
    off = GPMDM_PF(m2, T, 50, rng="philox", seed=2)
    with pytest.raises(ValueError, match="smoothing is off"):
        off.smoothed_marginal()
    mass = np.zeros(1)
    out = _lib.MarginalOut(mass=_lib.dptr(mass))
    assert lib.gpmdm_pf_smoothed_marginal(off._h, 0, 0, ctypes.byref(out), off._stream()) == _lib.GPMDM_E_INVALID
    pf = GPMDM_PF(m2, T, 300, rng="philox", seed=2, smoothing_lag=2)
    pf.update(Y[50])
    with pytest.raises(ValueError, match="depth"):
        pf.smoothed_marginal(2)
    assert lib.gpmdm_pf_smoothed_marginal(pf._h, 0, 2, ctypes.byref(out), pf._stream()) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_smoothed_marginal(pf._h, 1, 0, ctypes.byref(out), pf._stream()) == _lib.GPMDM_E_INVALID
    bank = GPMDM_PF_Bank(m2, T, 2, 300, seed=4, smoothing_lag=2)
    assert lib.gpmdm_pf_smoothed_marginal(bank._h, 0, 0, ctypes.byref(out), bank._stream()) == _lib.GPMDM_E_INVALID
    assert b"bank" in lib.gpmdm_last_error()
    h, s = pf._h, pf._stream()
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    assert lib.gpmdm_pf_smoothed_marginal(h, 0, 0, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(np.ascontiguousarray(Y[51])), None, s), "propagate")
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    assert len(pf.smoothed_marginal().lags) == 3 and mass[0] == 0.0
