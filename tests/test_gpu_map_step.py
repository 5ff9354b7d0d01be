"""``gpmdm_amd.map_step`` (gpmdm_map_step, csrc/mappath.h): one step of the MAP trajectory
recursion on scripted clouds, every score and every back-pointer against the extended-precision
reference of tests/map_ref.py.  Models, sizes and clouds are test_gpu_backward_step.py's.

The moments the reference takes as exact are ``model.map_x_dynamics_for_class(Xs, c)`` -- the
launches the step itself issues on the same rows.  With B the step's band (derived in
map_ref.py's docstring; u = 2^-53):

    |delta_j - ref_j| <= B + 4 u |ref_j|, -inf entries matching exactly,
    psi_j = ref_j wherever the reference's gap to the best other distinct source exceeds 2 B,

with G <= 1e6 and B <= 1e-9 asserted for every case, the number of entries whose gap is at or below
2 B asserted to be 0, and the achieved error / band printed beside the fp64 numpy yardstick's.
Every call is made twice and must return the same bits.
"""
import numpy as np
import pytest
import torch

import map_ref as R
from test_gpu_backward_step import MODELS, SIZES, _clouds, _model

pytestmark = pytest.mark.gpu


def _moments(m, Xs, C):
    mom = [m.map_x_dynamics_for_class(torch.from_numpy(np.ascontiguousarray(Xs)), c) for c in range(C)]
    return [x[0].cpu().numpy() for x in mom], [x[1].cpu().numpy() for x in mom]


def _check(m, T, Xs, cs, Xt, ct, delta=None, ll=None, what="", B0=0.0):
    """Returns (delta, psi, reference delta in longdouble, B): B0 is the band the sources' scores
    carry already (a chained step)."""
    from gpmdm_amd import map_step
    C = T.shape[0]
    mu, var = _moments(m, Xs, C)
    de, ps = (t.numpy() for t in map_step(m, T, Xs, cs, Xt, ct, delta, ll))
    de2, ps2 = (t.numpy() for t in map_step(m, T, Xs, cs, Xt, ct, delta, ll))
    assert de.tobytes() == de2.tobytes() and ps.tobytes() == ps2.tobytes(), what
    assert ps.dtype == np.int64 and de.dtype == np.float64
    ref_d, ref_p, gap, info = R.map_step(T, Xs, cs, delta, Xt, ct, ll, mu, var)
    y_d, y_p, _, _ = R.map_step(T, Xs, cs, delta, Xt, ct, ll, mu, var, dtype=np.float64)
    B = B0 + R.band_step(info)
    assert info["G"] <= 1e6 and R.band_step(info) <= 1e-9, (what, info, B)
    cut = ref_d.astype(np.float64) == -np.inf
    assert np.array_equal(de == -np.inf, cut), what
    assert np.array_equal(ps == -1, cut) and np.array_equal(ref_p == -1, cut), what
    assert not np.isnan(de).any(), what
    tol = B + 4 * R.U * np.abs(np.where(cut, 0, ref_d))
    e = np.abs(np.where(cut, 0, de) - np.where(cut, 0, ref_d)) / tol
    ey = np.abs(np.where(cut, 0, y_d) - np.where(cut, 0, ref_d)) / tol
    close = int((gap <= 2 * B).sum())
    fin = gap[np.isfinite(gap)]
    print(f"{what}: G {info['G']:.3g} K {info['K']:.3g} band {B:.2e}  delta err/band {float(e.max()):.3g} "
          f"(fp64 numpy {float(ey.max()):.3g})  min gap {float(fin.min()) if fin.size else np.inf:.3g}  "
          f"gaps <= 2 B: {close}  psi differing from fp64 numpy: {int((ps != y_p).sum())}")
    assert e.max() <= 1, (what, float(e.max()))
    assert close == 0, (what, close)
    decided = gap > 2 * B
    assert np.array_equal(ps[decided], ref_p[decided]), what
    assert np.all((ps >= -1) & (ps < len(cs))), what
    return de, ps, ref_d, B


@pytest.mark.parametrize("n_s,n_t", SIZES)
@pytest.mark.parametrize("key", list(MODELS))
def test_against_the_reference(key, n_s, n_t):
    """d = 1, 3, 32, C = 1, 2, 5; one pair, one row against many, a partial tile either side of 64,
    a block either side of 256, several blocks with ragged class segments and 5 and 16 ranges;
    scores and log-likelihoods set, so every addend of the recursion is exercised."""
    m, T, Xs, cs, Xt, ct, _ = _clouds(key, n_s, n_t, seed=n_s + 3 * n_t)
    rng = np.random.RandomState(n_s + 7 * n_t)
    delta, ll = -30.0 * rng.rand(n_s), -20.0 * rng.rand(n_t)
    de, ps, _, _ = _check(m, T, Xs, cs, Xt, ct, delta, ll, what=f"{key} {n_s}x{n_t}")
    assert np.all(ps >= 0)                                  # T has no zeros: every target is reached
    d0, p0, _, _ = _check(m, T, Xs, cs, Xt, ct, what=f"{key} {n_s}x{n_t} (defaults)")
    from gpmdm_amd import map_step
    dz, pz = map_step(m, T, Xs, cs, Xt, ct, np.zeros(n_s), np.zeros(n_t))
    assert dz.numpy().tobytes() == d0.tobytes() and pz.numpy().tobytes() == p0.tobytes()   # None means zeros


def test_empty_classes():
    m, T, Xs, cs, Xt, ct, _ = _clouds("d3C5", 150, 170, seed=5)
    ct[ct == 2] = 4                                         # no class-2 target
    _check(m, T, Xs, cs, Xt, ct, what="no class-2 target")
    m, T, Xs, cs, Xt, ct, _ = _clouds("d3C5", 150, 170, seed=6)
    cs[cs == 0] = 1
    cs[cs == 3] = 1                                         # no class-0 or class-3 source
    _check(m, T, Xs, cs, Xt, ct, what="no class-0/3 source")


def test_zeros_in_T_cut_targets_off():
    m, T, Xs, cs, Xt, ct, _ = _clouds("d3C5", 200, 180, seed=7)
    T[:, 2] = 0.0                                           # nobody reaches class 2
    T[0, 1] = T[3, 4] = 0.0
    T /= T.sum(1, keepdims=True)
    assert (ct == 2).sum() >= 5
    de, ps, _, _ = _check(m, T, Xs, cs, Xt, ct, what="zeros in T")
    assert np.all(ps[ct == 2] == -1) and np.all(de[ct == 2] == -np.inf)
    assert np.all(ps[ct != 2] >= 0) and np.all(np.isfinite(de[ct != 2]))
    assert not np.any((cs[ps[ct == 1]] == 0)) and not np.any((cs[ps[ct == 4]] == 3))   # the forbidden switches


def test_a_minus_inf_and_a_nan_likelihood():
    m, T, Xs, cs, Xt, ct, _ = _clouds("d3C5", 130, 140, seed=8)
    ll = -10.0 * np.random.RandomState(1).rand(140)
    ll[3], ll[77], ll[139] = -np.inf, np.nan, np.inf
    de, ps, _, _ = _check(m, T, Xs, cs, Xt, ct, None, ll, what="-inf / NaN / +inf ll")
    for j in (3, 77, 139):
        assert de[j] == -np.inf and ps[j] == -1
    # a source without a score (delta = -inf, NaN) is never chosen
    delta = -5.0 * np.random.RandomState(2).rand(130)
    delta[::3] = -np.inf
    delta[1::9] = np.nan
    de, ps, _, _ = _check(m, T, Xs, cs, Xt, ct, delta, None, what="-inf / NaN delta")
    assert np.all(np.isfinite(delta[ps]))


def test_scores_spanning_1e5():
    m, T, Xs, cs, Xt, ct, _ = _clouds("d3C5", 300, 280, seed=9)
    delta = np.random.RandomState(3).uniform(-1e5, 1e5, 300)
    delta[np.argsort(delta)[-40:]] = 1e5 - 40.0 * np.random.RandomState(4).rand(40)   # a contested top
    _check(m, T, Xs, cs, Xt, ct, delta, -50.0 * np.random.RandomState(5).rand(280), what="delta in +-1e5")


@pytest.mark.parametrize("order", ["low first", "high first"])
def test_copies_return_the_lower_index_exactly(order):
    """Bitwise copies of one source at indices either side of a tile boundary (63 | 64) and in two
    different ranges (n_s = 1000 against 777 targets: 16 ranges of 63 rows), written in both
    orders: the winner's copies tie exactly, and the lower index is returned."""
    m, T, Xs, cs, Xt, ct, _ = _clouds("d3C5", 1000, 777, seed=10)
    delta = -3.0 * np.random.RandomState(6).rand(1000)
    groups = [(63, 64), (10, 700), (200, 201, 950)]
    for g in groups:
        src = g[0] if order == "low first" else g[-1]
        for i in g:
            Xs[i], cs[i], delta[i] = Xs[src], cs[src], delta[src]
        delta[list(g)] += 40.0                              # these rows win wherever their class is reachable
    de, ps, _, _ = _check(m, T, Xs, cs, Xt, ct, delta, None, what=f"copies, {order}")
    lows = {g[0] for g in groups}
    highs = {i for g in groups for i in g[1:]}
    won = set(ps.tolist())
    assert won & lows and not won & highs, (sorted(won & lows), sorted(won & highs))
    for g in groups:                                        # a copy alone gives the same bits
        keep = np.ones(1000, dtype=bool)
        keep[list(g[:-1])] = False
        from gpmdm_amd import map_step
        d1, p1 = (t.numpy() for t in map_step(m, T, Xs[keep], cs[keep], Xt, ct, delta[keep], None))
        back = np.nonzero(keep)[0]
        p1 = np.where(p1 >= 0, back[np.maximum(p1, 0)], -1)
        assert d1.tobytes() == de.tobytes()
        assert np.array_equal(np.where(p1 == g[-1], g[0], p1), ps)


def test_two_chained_steps():
    """delta of one step is the next one's scores: against the reference's two steps, the bands
    adding."""
    m, T, X0, c0, X1, c1, _ = _clouds("d3C5", 260, 240, seed=11)
    rng = np.random.RandomState(12)
    X2 = 0.9 * X1[rng.randint(0, 240, 250)] + 0.2 * rng.randn(250, 3)
    c2 = rng.randint(0, 5, 250)
    l1, l2 = -8.0 * rng.rand(240), -8.0 * rng.rand(250)
    d1, _, ref1, B1 = _check(m, T, X0, c0, X1, c1, None, l1, what="chain, step 1")
    mu, var = _moments(m, X1, 5)
    from gpmdm_amd import map_step
    d2, p2 = (t.numpy() for t in map_step(m, T, X1, c1, X2, c2, d1, l2))
    r2, rp2, gap2, info2 = R.map_step(T, X1, c1, ref1, X2, c2, l2, mu, var)
    B2 = B1 + R.band_step(info2)
    e = np.abs(d2 - r2) / (B2 + 4 * R.U * np.abs(r2))
    print(f"chain, step 2: band {B2:.2e} delta err/band {float(e.max()):.3g} min gap {float(gap2.min()):.3g}")
    assert e.max() <= 1 and (gap2 <= 2 * B2).sum() == 0
    assert np.array_equal(p2, rp2)
