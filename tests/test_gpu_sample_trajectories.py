"""``GPMDM_PF.sample_trajectories`` (gpmdm_pf_sample_trajectories, csrc/backsample.h): backward
simulation over the filter's history ring.

Histories come from the filter's own ``export_state()`` after every update (the root: the export
before the first one).  Checked per read:

* ``indices`` is BITWISE the chain of ``backward_sample_step`` calls on the exports with
  sample_ref's Philox uniforms (key = the seed, counter (m, frame, 6, l)) and
  j_0 = min(P - 1, floor(u P)) -- the check of the counter layout and of the ring's slots;
* every draw passes sample_ref's acceptance rule against the extended-precision cumulative
  distribution (eps = ``backsmooth_ref.band_rel`` <= 1e-9, G <= 1e6 asserted); at most 1 draw in
  1000 per test may be near a boundary (accepted, but not the reference's own index) and never
  more than 3.  The seeds are fixed; each read prints the device's near-boundary count and, up to
  P = 777, the fp64 numpy yardstick's (host arithmetic on the same moments; none for these seeds
  when the tests were written);
* ``classes`` / ``states``: exactly the exports' rows at ``indices``; ``alive``, ``distinct``: exact;
  ``class_probabilities``: bitwise bincount / alive; ``|state_mean - fsum mean| <= n 2^-53 mean|x|``;
* the pose rows: bitwise ``current_observation()`` of a filter of n particles handed the lag's
  ``states`` and ``classes`` through ``load_state``.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import sample_ref as S
from conftest import product_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _moments(m, X, C=2):
    mom = [m.map_x_dynamics_for_class(torch.from_numpy(np.ascontiguousarray(X)), c) for c in range(C)]
    return [x[0].cpu().numpy() for x in mom], [x[1].cpu().numpy() for x in mom]


def _check(st, hist, T, m, seed, frame, what, yardstick):
    """One read against the window's exports (oldest first).  Returns the near-boundary count."""
    from gpmdm_amd import backward_sample_step
    lag = len(hist) - 1
    P = len(hist[-1]["classes"])
    ix = st.indices.numpy()
    n = ix.shape[1]
    assert ix.shape == (lag + 1, n) and ix.dtype == np.int64
    assert np.array_equal(st.lags.numpy(), np.arange(lag + 1)) and np.array_equal(st.frames.numpy(), frame - np.arange(lag + 1))
    u = S.uniforms(seed, frame, n, lag)
    assert np.array_equal(ix[0], S.start(u[0], P)), what
    near = near64 = 0
    for l in range(lag):
        src, e = hist[-2 - l], hist[-1 - l]
        assert np.all(ix[l] >= 0), what                     # (T has no zeros: nobody dies)
        Xt, ct = np.ascontiguousarray(e["states"][ix[l]]), np.ascontiguousarray(e["classes"][ix[l]])
        k, _ = backward_sample_step(m, T, src["states"], src["classes"], Xt, ct, u[l + 1])
        assert ix[l + 1].tobytes() == k.numpy().tobytes(), (what, l, "indices against chained backward_sample_step")
        mu, var = _moments(m, src["states"])
        a, b, info = S.check_draws(T, src["states"], src["classes"], None, Xt, ct, u[l + 1], ix[l + 1], mu, var,
                                   what=(what, l), yardstick=yardstick)
        near, near64 = near + a, near64 + b
    print(f"{what}: near-boundary draws {near} (fp64 numpy {near64 if yardstick else 'not run'}) of {lag * n}")
    for l in range(lag + 1):
        e = hist[-1 - l]
        assert np.array_equal(st.classes[l].numpy(), e["classes"][ix[l]]), (what, l)
        assert st.states[l].numpy().tobytes() == np.ascontiguousarray(e["states"][ix[l]]).tobytes(), (what, l)
        assert st.alive[l].item() == n and st.distinct[l].item() == len(np.unique(ix[l])), (what, l)
        cp = np.bincount(e["classes"][ix[l]], minlength=2) / n
        assert st.class_probabilities[l].numpy().tobytes() == cp.tobytes(), (what, l)
        X = e["states"][ix[l]]
        for q in range(X.shape[1]):
            ref = math.fsum(X[:, q]) / n
            assert abs(st.state_mean[l, q].item() - ref) <= n * 2.0 ** -53 * float(np.abs(X[:, q]).mean()), (what, l, q)
    return near


def _same(a, b):
    for k in ("lags", "frames", "indices", "classes", "states", "class_probabilities", "state_mean", "alive", "distinct"):
        assert getattr(a, k).numpy().tobytes() == getattr(b, k).numpy().tobytes(), k


@pytest.mark.parametrize("n", [1, 64, 300])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("P", [1, 33, 777, 5000])
def test_against_the_chain_and_the_reference(m2, fx_config2, P, L, n):
    """One particle, a partial wave, a ragged last block, several ranges; 2 L + 3 frames, so the
    ring wraps.  Read after frame 2 and after the last frame; the same call twice, a shorter window
    and fewer trajectories, another seed, the filter's own seed; torch's generator, the frame
    counter and the health counters untouched; a twin filter that is never read stays bitwise
    identical to the end."""
    from gpmdm_amd import GPMDM_PF, SampledTrajectories
    T = torch.tensor(fx_config2["T"])
    Tn = np.ascontiguousarray(T.numpy(), dtype=np.float64)
    torch.manual_seed(12)                       # (the initial cloud is drawn from torch's generator)
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L)
    torch.manual_seed(12)
    twin = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L)
    other = GPMDM_PF(m2, T, n, rng="philox", seed=1)
    Y = m2.get_Y()
    frames = 2 * L + 3
    hist = [pf.export_state()]
    near = draws = 0
    for k in range(1, frames + 1):
        pf.update(Y[200 + k - 1])
        twin.update(Y[200 + k - 1])
        hist.append(pf.export_state())
        if k not in (2, frames):
            continue
        depth = min(L, k)
        g, fr, health = torch.get_rng_state(), pf.frame, pf.health()
        st = pf.sample_trajectories(n, seed=99)
        assert torch.equal(g, torch.get_rng_state()) and pf.frame == fr == k and pf.health() == health
        assert isinstance(st, SampledTrajectories) and st.states.shape == (depth + 1, n, 3)
        assert st.observation_mean is None and st.observation_spread is None
        near += _check(st, hist[-(depth + 1):], Tn, m2, 99, k, (P, L, n, k), yardstick=P <= 777)
        draws += depth * n
        _same(st, pf.sample_trajectories(n, seed=99))
        _same(st, pf.sample_trajectories(n, depth, seed=99))
        # trajectory m depends on neither n nor the window
        few = pf.sample_trajectories(min(7, n), 1, seed=99)
        assert np.array_equal(few.indices.numpy(), st.indices.numpy()[:2, :min(7, n)])
        assert few.states.numpy().tobytes() == np.ascontiguousarray(st.states.numpy()[:2, :min(7, n)]).tobytes()
        # the key: another seed, and the filter's own
        own = pf.sample_trajectories(n)
        _same(own, pf.sample_trajectories(n, seed=7))
        if P >= 33 and n >= 64:
            assert not np.array_equal(own.indices.numpy(), st.indices.numpy())
        # the pose of each lag
        posed = pf.sample_trajectories(n, seed=99, observation=True)
        _same(st, posed)
        for l in range(depth + 1):
            other.load_state(posed.states[l].numpy(), posed.classes[l].numpy())
            mean, spread = other.current_observation()
            assert np.array_equal(posed.observation_mean[l].numpy(), mean.numpy()), (P, L, n, k, l)
            assert np.array_equal(posed.observation_spread[l].numpy(), spread.numpy()), (P, L, n, k, l)
        with pytest.raises(ValueError, match="depth"):
            pf.sample_trajectories(n, depth + 1)
    assert near <= S.near_cap(draws), near
    a, b = pf.export_state(), twin.export_state()
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(pf.class_probabilities().numpy(), twin.class_probabilities().numpy())
    assert pf.health() == twin.health()


def test_the_distribution(m2, fx_config2):
    """20 000 trajectories over P = 300, L = 2: at every lag the class fractions and the mean state
    agree with the marginal smoother's within five standard errors of an n-sample mean (the
    trajectories are independent draws whose lag-l marginal is the smoother's w_l, up to the
    rounding band).  The seed is fixed; a correct sampler fails one such comparison with
    probability below 1e-5 (a five-sigma two-sided Gaussian tail is 5.7e-7; n = 20 000 draws of
    bounded terms are Gaussian to well within the remaining factor)."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    torch.manual_seed(5)
    P, L, n = 300, 2, 20_000
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=21, smoothing_lag=L)
    Y = m2.get_Y()
    hist = []
    for k in range(4):
        pf.update(Y[400 + k])
        hist.append(pf.export_state())
    st = pf.sample_trajectories(n, seed=1234)
    sm = pf.smoothed_marginal(particles=True)
    assert st.alive.tolist() == [n] * (L + 1)
    for l in range(L + 1):
        w = sm.weights[l].numpy()
        X = hist[-1 - l]["states"]
        for c in range(2):
            p = sm.class_probabilities[l, c].item()
            got = st.class_probabilities[l, c].item()
            print(f"lag {l} class {c}: sampled {got:.5f} marginal {p:.5f} bound {5 * math.sqrt(p * (1 - p) / n) + 1e-12:.5f}")
            assert abs(got - p) <= 5 * math.sqrt(max(p * (1 - p), 0.0) / n) + 1e-12, (l, c, got, p)
        for q in range(3):
            mean = sm.state_mean[l, q].item()
            se = math.sqrt(float((w * (X[:, q] - mean) ** 2).sum()) / n)
            got = st.state_mean[l, q].item()
            print(f"lag {l} coordinate {q}: sampled {got:.6f} marginal {mean:.6f} bound {5 * se:.6f}")
            assert abs(got - mean) <= 5 * se, (l, q, got, mean, se)


def test_a_masked_and_gated_filter(m2, fx_config2):
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Tn = np.ascontiguousarray(T.numpy(), dtype=np.float64)
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    torch.manual_seed(3)
    pf = GPMDM_PF(m2, T, 300, rng="philox", seed=11, smoothing_lag=3, gate=3.0)
    observed = np.ones(m2.D, dtype=bool)
    observed[::4] = False
    hist = [pf.export_state()]
    for k in range(5):
        z = Y[300 + k].copy()
        if k in (1, 3):
            z[1] += 40.0                         # an outlier joint: the gate rejects it
        pf.update(z, observed=observed if k % 2 == 0 else None)
        hist.append(pf.export_state())
    st = pf.sample_trajectories(64, observation=True)
    assert len(st.lags) == 4 and st.observation_mean.shape == (4, m2.D)
    near = _check(st, hist[-4:], Tn, m2, 11, 5, "masked, gated", yardstick=True)
    assert near <= S.near_cap(3 * 64)


def test_refusals(m2, fx_config2):
    """Smoothing off, a lag above the depth, n = 0, n P above 2^36, a bank handle, a call inside a
    frame."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    lib = _lib.load()
    al = np.full(8, -5, dtype=np.int64)
    out = _lib.SampleOut(alive=_lib.i64ptr(al))
    off = GPMDM_PF(m2, T, 50, rng="philox", seed=2)
    with pytest.raises(ValueError, match="smoothing is off"):
        off.sample_trajectories(4)
    assert lib.gpmdm_pf_sample_trajectories(off._h, 4, 1, None, ctypes.byref(out), off._stream()) == _lib.GPMDM_E_INVALID
    assert b"smoothing is off" in lib.gpmdm_last_error()
    pf = GPMDM_PF(m2, T, 300, rng="philox", seed=2, smoothing_lag=2)
    with pytest.raises(ValueError, match="depth"):
        pf.sample_trajectories(4)                # depth 0: no window yet
    pf.update(Y[50])
    with pytest.raises(ValueError, match="depth"):
        pf.sample_trajectories(4, 2)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="n must be"):
            pf.sample_trajectories(bad)
    h, s = pf._h, pf._stream()
    assert lib.gpmdm_pf_sample_trajectories(h, 4, 2, None, ctypes.byref(out), s) == _lib.GPMDM_E_INVALID
    assert b"depth" in lib.gpmdm_last_error()
    assert lib.gpmdm_pf_sample_trajectories(h, 4, 0, None, ctypes.byref(out), s) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_sample_trajectories(h, 0, 1, None, ctypes.byref(out), s) == _lib.GPMDM_E_INVALID
    assert b"n must be" in lib.gpmdm_last_error()
    # n P above 2^36: refused on the sizes, before any launch or allocation of that size
    big = GPMDM_PF(m2, T, 262144, rng="philox", seed=2, smoothing_lag=1)
    with pytest.raises(ValueError, match="2\\^36"):
        big.sample_trajectories(262145)
    assert lib.gpmdm_pf_sample_trajectories(big._h, 262145, 1, None, ctypes.byref(out), big._stream()) == \
        _lib.GPMDM_E_INVALID
    assert b"2^36" in lib.gpmdm_last_error()
    bank = GPMDM_PF_Bank(m2, T, 2, 300, seed=4, smoothing_lag=2)
    assert lib.gpmdm_pf_sample_trajectories(bank._h, 4, 1, None, ctypes.byref(out), bank._stream()) == \
        _lib.GPMDM_E_INVALID
    assert b"bank" in lib.gpmdm_last_error()
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    assert lib.gpmdm_pf_sample_trajectories(h, 4, 1, None, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(np.ascontiguousarray(Y[51])), None, s), "propagate")
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    assert np.all(al == -5)                      # no refused call wrote anything
    assert lib.gpmdm_pf_sample_trajectories(h, 4, 2, None, ctypes.byref(out), s) == _lib.GPMDM_OK
    assert al[:3].tolist() == [4, 4, 4]
