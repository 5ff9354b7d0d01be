"""``GPMDM_PF.map_path`` (gpmdm_pf_map_path, csrc/mappath.h): MAP trajectory decoding over the
filter's history ring.

Histories come from the filter's own ``export_state()`` after every update (the root: the export
before the first one).  With ``particles=True``:

* ``delta`` and ``backpointers`` are BITWISE the chained ``map_step`` calls on the exports with
  l = ``ll[resample_idx]`` -- the check of the ring's log-likelihood plane and of the
  de-duplication (the recursion runs on each slot's distinct ancestors, ``map_step`` on all P rows);
* the path is the host backtrack of those arrays, ``distinct`` the distinct ancestors per slot;
* ``delta`` stays within map_ref's band B(l) (the steps' bands added; derived in its docstring),
  |delta - ref| <= B(l) + 4 u |ref|, G <= 1e6 and each step's band <= 1e-9 asserted;
* the reference's score of the device's path is >= the reference's optimum - 2 B(0) (for every
  path the two scores differ by at most B(0)); and the path is the reference's when every gap
  along it exceeds 2 B.
"""
import ctypes

import numpy as np
import pytest
import torch

import map_ref as R
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


def _chain(mp, hist, root_has_anc, T, m, what):
    """The bitwise part: chained map_step, the host backtrack, distinct.  hist: the window's
    exports, oldest first."""
    from gpmdm_amd import map_step
    n = len(hist) - 1
    P = len(hist[-1]["classes"])
    D, Bp = mp.delta.numpy(), mp.backpointers.numpy()
    assert D.shape == (n + 1, P) and Bp.shape == (n, P) and Bp.dtype == np.int64
    assert np.all(D[n] == 0.0), what
    delta = None
    for l in range(n - 1, -1, -1):
        src, e = hist[-2 - l], hist[-1 - l]
        delta, psi = (t.numpy() for t in map_step(m, T, src["states"], src["classes"], e["states"], e["classes"],
                                                   delta, R.slot_ll(e)))
        assert D[l].tobytes() == delta.tobytes(), (what, l, "delta against chained map_step")
        assert Bp[l].tobytes() == psi.tobytes(), (what, l, "psi against chained map_step")
    path = R.backtrack(D[0], list(Bp))
    assert np.array_equal(mp.indices.numpy(), path), what
    assert np.array_equal(mp.lags.numpy(), np.arange(n + 1))
    for l in range(n + 1):
        e, j = hist[-1 - l], int(path[l])
        if j < 0:
            assert mp.classes[l].item() == -1 and np.all(np.isnan(mp.states[l].numpy())) and mp.scores[l].item() == -np.inf
            continue
        assert mp.classes[l].item() == int(e["classes"][j]), (what, l)
        assert mp.states[l].numpy().tobytes() == np.ascontiguousarray(e["states"][j]).tobytes(), (what, l)
        assert mp.scores[l].item() == D[l, j], (what, l)
        has_anc = l < n or root_has_anc
        assert mp.distinct[l].item() == (len(np.unique(e["resample_idx"])) if has_anc else P), (what, l)
    assert mp.log_joint == (D[0, path[0]] if path[0] >= 0 else -np.inf)


def _against_ref(mp, hist, T, m, C, what, yardstick):
    n = len(hist) - 1
    mom = _moments(m, C)
    ref = R.map_path(hist, T, mom, n)
    y64 = R.map_path(hist, T, mom, n, np.float64) if yardstick else None
    D = mp.delta.numpy()
    for l in range(n):
        info, B = ref["info"][l], ref["B"][l]
        assert info["G"] <= 1e6 and R.band_step(info) <= 1e-9, (what, l, info)
        r = ref["delta"][l]
        cut = r.astype(np.float64) == -np.inf
        assert np.array_equal(D[l] == -np.inf, cut), (what, l)
        tol = B + 4 * R.U * np.abs(np.where(cut, 0, r))
        e = float((np.abs(np.where(cut, 0, D[l]) - np.where(cut, 0, r)) / tol).max())
        ey = float((np.abs(np.where(cut, 0, y64["delta"][l]) - np.where(cut, 0, r)) / tol).max()) if yardstick else float("nan")
        print(f"{what} lag {l}: G {info['G']:.3g} K {info['K']:.3g} band {B:.2e} delta err/band {e:.3g} "
              f"(fp64 numpy {ey:.3g}) distinct {int(mp.distinct[l])} min gap {float(ref['gap'][l].min()):.3g}")
        assert e <= 1, (what, l, e)
    B0 = ref["B"][0]
    path = mp.indices.numpy()
    if np.isfinite(float(ref["log_joint"])):
        score = R.path_score(hist, T, mom, path)
        assert float(ref["log_joint"] - score) <= 2 * B0, (what, float(ref["log_joint"] - score), B0)
        assert abs(mp.log_joint - float(ref["log_joint"])) <= B0 + 4 * R.U * abs(float(ref["log_joint"])), what
    # the path itself, when the reference's choices are all clear of the band
    d0 = np.unique(ref["delta"][0].astype(np.float64))
    clear = len(d0) < 2 or d0[-1] - d0[-2] > 2 * B0
    for l in range(n):
        clear = clear and ref["path"][l] >= 0 and ref["gap"][l][ref["path"][l]] > 2 * ref["B"][l]
    print(f"{what}: path {path.tolist()} reference {ref['path'].tolist()} gaps allow the comparison: {bool(clear)}")
    if clear:
        assert np.array_equal(path, ref["path"]), what


def _same(a, b):
    for k in ("lags", "frames", "indices", "classes", "states", "scores", "distinct", "delta", "backpointers"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or x.numpy().tobytes() == y.numpy().tobytes()), k
    assert np.float64(a.log_joint).tobytes() == np.float64(b.log_joint).tobytes()


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("P", [1, 33, 777, 5000])
def test_against_the_chain_and_the_reference(m2, fx_config2, P, L):
    """One particle, a partial wave, a ragged last block, several blocks; 2 L + 3 frames, so the
    ring wraps.  Read after frame 2 (for L >= 2 the oldest slot in reach is the cleared ring's
    root: no ancestors) and after the last frame (every slot a resample's); the whole depth, a
    shorter window, twice in a row; a twin filter without recording that is never read stays
    bitwise identical to the end."""
    from gpmdm_amd import GPMDM_PF, MapPath
    T = torch.tensor(fx_config2["T"])
    Tn = np.ascontiguousarray(T.numpy(), dtype=np.float64)
    torch.manual_seed(12)                       # (the initial cloud is drawn from torch's generator)
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L, map_path=True)
    torch.manual_seed(12)
    twin = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L)
    assert pf.map_recording and not twin.map_recording
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
        mp = pf.map_path(particles=True)
        assert torch.equal(g, torch.get_rng_state()) and pf.frame == fr and pf.health() == health
        assert isinstance(mp, MapPath) and mp.states.shape == (depth + 1, 3) and mp.observation_mean is None
        assert np.array_equal(mp.frames.numpy(), k - np.arange(depth + 1))
        window = hist[-(depth + 1):]
        _chain(mp, window, k > L, Tn, m2, (P, L, k))
        _against_ref(mp, window, Tn, m2, 2, (P, L, k), yardstick=P <= 777)
        _same(mp, pf.map_path(particles=True))
        _same(mp, pf.map_path(depth, particles=True))
        bare = pf.map_path(observation=True)
        assert bare.delta is None and bare.backpointers is None
        assert bare.indices.numpy().tobytes() == mp.indices.numpy().tobytes() and bare.log_joint == mp.log_joint
        y = m2.map_x_to_y(bare.states)[0].cpu()
        assert bare.observation_mean.shape == (depth + 1, m2.D) and torch.equal(bare.observation_mean, y.to(torch.float64))
        if depth > 1:                            # a shorter window is a recursion of its own
            short = pf.map_path(1, particles=True)
            _chain(short, hist[-2:], True, Tn, m2, (P, L, k, "lag 1"))
        with pytest.raises(ValueError, match="depth"):
            pf.map_path(depth + 1)
    a, b = pf.export_state(), twin.export_state()
    for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(pf.class_probabilities().numpy(), twin.class_probabilities().numpy())
    assert pf.health() == twin.health()


def test_a_masked_and_gated_filter(m2, fx_config2):
    """The plane holds the log-likelihoods the frames' normalisers read: masked joints and a gated
    outlier included.  set_map_path after construction, a later set_smoothing keeps it."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Tn = np.ascontiguousarray(T.numpy(), dtype=np.float64)
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    torch.manual_seed(3)
    pf = GPMDM_PF(m2, T, 300, rng="philox", seed=11, smoothing_lag=2, gate=3.0)
    assert not pf.map_recording
    pf.set_map_path(True)
    assert pf.map_recording and pf.smoothing_depth == 0
    pf.set_smoothing(3)                          # keeps the flag, resizes the plane, clears the history
    assert pf.map_recording and pf.smoothing_lag == 3
    observed = np.ones(m2.D, dtype=bool)
    observed[::4] = False
    hist = [pf.export_state()]
    gated = 0
    for k in range(5):
        z = Y[300 + k].copy()
        if k in (1, 3):
            z[1] += 40.0                         # an outlier joint: the gate rejects it
        pf.update(z, observed=observed if k % 2 == 0 else None)
        gated += int(pf.gate_report().n_gated)
        hist.append(pf.export_state())
    assert gated >= 1
    mp = pf.map_path(particles=True)
    assert len(mp.lags) == 4
    _chain(mp, hist[-4:], True, Tn, m2, "masked, gated")
    _against_ref(mp, hist[-4:], Tn, m2, 2, "masked, gated", yardstick=True)
    pf.set_map_path(False)
    assert not pf.map_recording and pf.smoothing_depth == 3      # the rest of the history stays
    with pytest.raises(ValueError, match="recording is off"):
        pf.map_path()


def test_refusals(m2, fx_config2):
    """Smoothing or recording off, a lag outside [1, depth], a bank handle, calls inside a frame,
    and the history limit counting the plane."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    lib = _lib.load()
    lj = np.zeros(1)
    out = _lib.MapOut(log_joint=_lib.dptr(lj))
    off = GPMDM_PF(m2, T, 50, rng="philox", seed=2)
    with pytest.raises(ValueError, match="smoothing is off"):
        off.map_path()
    assert lib.gpmdm_pf_map_path(off._h, 1, ctypes.byref(out), off._stream()) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_set_map(off._h, 1) == _lib.GPMDM_E_INVALID and b"smoothing" in lib.gpmdm_last_error()
    rec_off = GPMDM_PF(m2, T, 50, rng="philox", seed=2, smoothing_lag=2)
    rec_off.update(Y[50])
    with pytest.raises(ValueError, match="recording is off"):
        rec_off.map_path()
    assert lib.gpmdm_pf_map_path(rec_off._h, 1, ctypes.byref(out), rec_off._stream()) == _lib.GPMDM_E_INVALID
    assert b"recording is off" in lib.gpmdm_last_error()
    pf = GPMDM_PF(m2, T, 300, rng="philox", seed=2, smoothing_lag=2, map_path=True)
    on = ctypes.c_int(0)
    assert lib.gpmdm_pf_map_recording(pf._h, ctypes.byref(on)) == 0 and on.value == 1
    with pytest.raises(ValueError, match="depth"):
        pf.map_path()                            # depth 0: no window yet
    pf.update(Y[50])
    with pytest.raises(ValueError, match="depth"):
        pf.map_path(2)
    assert lib.gpmdm_pf_map_path(pf._h, 2, ctypes.byref(out), pf._stream()) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_map_path(pf._h, 0, ctypes.byref(out), pf._stream()) == _lib.GPMDM_E_INVALID
    bank = GPMDM_PF_Bank(m2, T, 2, 300, seed=4, smoothing_lag=2)
    assert lib.gpmdm_pf_map_path(bank._h, 1, ctypes.byref(out), bank._stream()) == _lib.GPMDM_E_INVALID
    assert b"bank" in lib.gpmdm_last_error()
    assert lib.gpmdm_pf_set_map(bank._h, 1) == _lib.GPMDM_E_INVALID and b"bank" in lib.gpmdm_last_error()
    h, s = pf._h, pf._stream()
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    assert lib.gpmdm_pf_map_path(h, 1, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_pf_set_map(h, 0) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(np.ascontiguousarray(Y[51])), None, s), "propagate")
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    assert lj[0] == 0.0
    assert len(pf.map_path().lags) == 3 and np.isfinite(pf.map_path().log_joint)
    # the 1 GiB history limit counts the plane: d = 3, P = 262144 holds 128 slots without it, 102 with it
    big = GPMDM_PF(m2, T, 262144, rng="philox", seed=2, smoothing_lag=110)
    assert lib.gpmdm_pf_set_map(big._h, 1) == _lib.GPMDM_E_INVALID and b"1 GiB" in lib.gpmdm_last_error()
    big.set_smoothing(100)
    big.set_map_path(True)
    with pytest.raises(ValueError, match="1 GiB"):
        big.set_smoothing(110)
