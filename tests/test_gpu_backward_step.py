"""``gpmdm_amd.backward_step`` (gpmdm_backward_step, csrc/backsmooth.h): one step of the marginal
backward smoother on scripted clouds, every weight and every log-denominator against the
extended-precision reference of tests/backsmooth_ref.py.

The moments the reference takes as exact are ``model.map_x_dynamics_for_class(Xs, c)`` -- the
launches the step itself issues on the same rows.  Band (derived in backsmooth_ref.py's docstring
and DESIGN.md §3.6; u = 2^-53):

    |ws_i - ref_i| <= ref_i (a + b G) u + 1e-300,
    |log_den_j - ref_j| <= (a + b G) u + 4 u |ref_j|    (the conversion to natural logarithms),

with G <= 1e6 and (a + b G) u <= 1e-9 asserted for every case, -inf denominators matching
exactly, and the achieved error / band printed beside the fp64 numpy yardstick's.  Every call is
made twice and must return the same bits.
"""
import numpy as np
import pytest
import torch

import backsmooth_ref as R
from conftest import synthetic_model

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (257, 255), (1000, 777)]
MODELS = {"d1C2": dict(C=2, d=1, D=4, L=25), "d3C5": dict(C=5, d=3, D=6, L=14), "d32C1": dict(C=1, d=32, D=8, L=40)}
_models = {}


def _model(key):
    if key not in _models:
        _models[key] = synthetic_model(seed=31, **MODELS[key])[:2]
    return _models[key]


def _clouds(key, n_s, n_t, seed):
    """Sources around the training cloud's scale; targets a short move away from some source."""
    m, T = _model(key)
    C, d = MODELS[key]["C"], MODELS[key]["d"]
    rng = np.random.RandomState(seed)
    Xs = 0.6 * rng.randn(n_s, d)
    Xt = 0.9 * Xs[rng.randint(0, n_s, n_t)] + 0.2 * rng.randn(n_t, d)
    cs, ct = rng.randint(0, C, n_s), rng.randint(0, C, n_t)
    wt = rng.uniform(0.2, 1.0, n_t)
    return m, T.numpy().copy(), Xs, cs, Xt, ct, wt / wt.sum()


def _check(m, T, Xs, cs, Xt, ct, wt, a=None, what=""):
    from gpmdm_amd import backward_step
    C = T.shape[0]
    mom = [m.map_x_dynamics_for_class(torch.from_numpy(Xs), c) for c in range(C)]
    mu, var = [x[0].cpu().numpy() for x in mom], [x[1].cpu().numpy() for x in mom]
    ws, ld = (t.numpy() for t in backward_step(m, T, Xs, cs, Xt, ct, wt, a))
    ws2, ld2 = (t.numpy() for t in backward_step(m, T, Xs, cs, Xt, ct, wt, a))
    assert ws.tobytes() == ws2.tobytes() and ld.tobytes() == ld2.tobytes(), what
    ref_w, ref_l, info = R.backward_step(T, Xs, cs, a, Xt, ct, wt, mu, var)
    y_w, y_l, _ = R.backward_step(T, Xs, cs, a, Xt, ct, wt, mu, var, dtype=np.float64)
    band = R.band_rel(info)
    assert info["G"] <= 1e6 and band <= 1e-9, (what, info, band)
    tol_w = ref_w * band + R.LD(1e-300)
    cut = ref_l == -np.inf
    assert np.array_equal(ld == -np.inf, cut), what
    tol_l = band + 4 * R.U * np.abs(np.where(cut, 0, ref_l))
    e_w, e_y = np.abs(ws - ref_w) / tol_w, np.abs(y_w - ref_w) / tol_w
    e_l = np.abs(np.where(cut, 0, ld) - np.where(cut, 0, ref_l)) / tol_l
    e_ly = np.abs(np.where(cut, 0, y_l) - np.where(cut, 0, ref_l)) / tol_l
    print(f"{what}: G {info['G']:.3g} band {band:.2e}  weights err/band {float(e_w.max()):.3g} "
          f"(fp64 numpy {float(e_y.max()):.3g})  log_den {float(e_l.max()):.3g} (fp64 numpy {float(e_ly.max()):.3g})")
    assert np.all(np.isfinite(ws)) and np.all(ws >= 0), what
    assert e_w.max() <= 1, (what, float(e_w.max()))
    assert e_l.max() <= 1, (what, float(e_l.max()))
    return ws, ld, ref_w, info


@pytest.mark.parametrize("n_s,n_t", SIZES)
@pytest.mark.parametrize("key", list(MODELS))
def test_against_the_reference(key, n_s, n_t):
    """d = 1, 3, 32 (the largest dynamics tile), C = 1, 2, 5; one pair, one row against many, a
    partial wave either side of 64, one block either side of 256, several blocks with ragged
    class segments."""
    args = _clouds(key, n_s, n_t, seed=n_s + 3 * n_t)
    ws, _, ref_w, _ = _check(*args, what=f"{key} {n_s}x{n_t}")
    assert abs(ws.sum() - 1) <= 1e-9                       # T has no zeros: every target is reached


def test_empty_classes():
    m, T, Xs, cs, Xt, ct, wt = _clouds("d3C5", 150, 170, seed=5)
    ct[ct == 2] = 4                                         # no class-2 target
    _check(m, T, Xs, cs, Xt, ct, wt, what="no class-2 target")
    m, T, Xs, cs, Xt, ct, wt = _clouds("d3C5", 150, 170, seed=6)
    cs[cs == 0] = 1
    cs[cs == 3] = 1                                         # no class-0 or class-3 source
    _check(m, T, Xs, cs, Xt, ct, wt, what="no class-0/3 source")


def test_zeros_in_T_cut_targets_off():
    m, T, Xs, cs, Xt, ct, wt = _clouds("d3C5", 200, 180, seed=7)
    T[:, 2] = 0.0                                           # nobody reaches class 2
    T[0, 1] = T[3, 4] = 0.0
    T /= T.sum(1, keepdims=True)
    assert (ct == 2).sum() >= 5
    ws, ld, ref_w, _ = _check(m, T, Xs, cs, Xt, ct, wt, what="zeros in T")
    assert np.all(ld[ct == 2] == -np.inf) and np.all(np.isfinite(ld[ct != 2]))
    assert abs(ws.sum() - wt[ct != 2].sum()) <= 1e-9       # the mass of the cut-off targets is missing


def test_nonuniform_source_weights():
    m, T, Xs, cs, Xt, ct, wt = _clouds("d3C5", 260, 130, seed=8)
    a = np.random.RandomState(3).uniform(1e-6, 1.0, 260)
    a[7] = 0.0                                              # a source of weight zero gets weight zero
    a /= a.sum()
    ws, _, _, _ = _check(m, T, Xs, cs, Xt, ct, wt, a, what="non-uniform a")
    assert ws[7] == 0.0


def test_repeated_sources_get_the_same_bits():
    m, T, Xs, cs, Xt, ct, wt = _clouds("d3C5", 300, 270, seed=9)
    pick = np.random.RandomState(4).randint(0, 40, 300)     # 40 distinct rows, copies across blocks
    Xs, cs = Xs[pick], cs[pick]
    ws, _, _, _ = _check(m, T, Xs, cs, Xt, ct, wt, what="repeated sources")
    for u in np.unique(pick):
        assert len(set(ws[pick == u].tobytes()[8 * i:8 * i + 8] for i in range((pick == u).sum()))) == 1, u


def test_a_far_target_stays_in_the_log_domain():
    """One target 850 sigma from every source's mean (d = 1): f ~ exp(-3.6e5) underflows to 0 in
    fp64, its denominator does not in the log domain, and its weight is shared out as usual.
    (850, not 1000: at 1000 sigma G reaches 5e5 and the band's b G u passes the 1e-9 it may not.)"""
    m, T, Xs, cs, Xt, ct, wt = _clouds("d1C2", 120, 90, seed=10)
    Xs = 0.3 + 0.01 * np.random.RandomState(11).randn(120, 1)
    mom = [m.map_x_dynamics_for_class(torch.from_numpy(Xs), c) for c in range(2)]
    mu = np.stack([x[0].cpu().numpy() for x in mom])
    var = np.stack([x[1].cpu().numpy() for x in mom])
    Xt = 0.9 * Xs[:90] + 0.05
    Xt[0, 0] = mu.max() + 850.0 * np.sqrt(var.max())
    ws, ld, ref_w, info = _check(m, T, Xs, cs, Xt, ct, wt, what="far target")
    assert info["G"] >= 0.5 * 850.0 ** 2 and np.isfinite(ld[0]) and ld[0] < -3.6e5
    assert abs(ws.sum() - 1) <= 1e-9
