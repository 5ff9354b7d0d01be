"""``gpmdm_amd.backward_sample_step`` (gpmdm_backward_sample_step, csrc/backsample.h): one step of
backward simulation on scripted clouds of config 2's model (d = 3, C = 2), against the
extended-precision cumulative distribution of tests/sample_ref.py.

The moments the reference takes as exact are ``model.map_x_dynamics_for_class(Xs, c)`` -- the
launches the step itself issues on the same rows.  A device index k is accepted for uniform u when
its term is positive in the reference and F(k - 1) - eps <= u <= F(k) + eps with eps =
``backsmooth_ref.band_rel`` (eps <= 1e-9 and G <= 1e6 asserted).  A draw is near a boundary when
the accepted k is not the reference's own; per test at most 1 draw in 1000 may be, and never more
than 3.  The scripted uniforms sit mid-interval, at the edges or on a regular grid; the random
ones use fixed numpy seeds, and every check prints the device's and the fp64 numpy yardstick's
near-boundary counts (the yardstick is host arithmetic on the same moments; it had none for
these seeds when the tests were written).

Sizes follow the range length R = ``_lib.GPMDM_BACKSAMPLE_RANGE``: one source, a partial wave and
one either side of the LDS tile (63, 64, 65), one range and one either side of it, and two whole
ranges with a ragged third.
"""
import ctypes

import numpy as np
import pytest
import torch

import sample_ref as S
from conftest import product_model
from gpmdm_amd import _lib

pytestmark = pytest.mark.gpu

R = _lib.GPMDM_BACKSAMPLE_RANGE
SIZES = [1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 7]


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _moments(m, X, C=2):
    mom = [m.map_x_dynamics_for_class(torch.from_numpy(np.ascontiguousarray(X)), c) for c in range(C)]
    return [x[0].cpu().numpy() for x in mom], [x[1].cpu().numpy() for x in mom]


_cache = {}


def _clouds(m, f, n_s, n_t, seed):
    """Sources in a tight cluster around a training point (every source has a comparable density
    towards every target, so no interval of the distribution is tiny); targets one proposal step
    away from some source.  Built once per (n_s, n_t, seed) and shared."""
    key = (n_s, n_t, seed)
    if key not in _cache:
        rng = np.random.RandomState(seed)
        x0 = np.asarray(f["X"], dtype=np.float64)[100 + seed]
        _, v0 = _moments(m, x0[None, :])
        s = 0.1 * float(np.sqrt(np.mean([v.mean() for v in v0])))
        Xs = x0[None, :] + s * rng.randn(n_s, 3)
        cs, ct = rng.randint(0, 2, n_s), rng.randint(0, 2, n_t)
        mu, var = _moments(m, Xs)
        src = rng.randint(0, n_s, n_t)
        Xt = np.stack([mu[c][k] + np.sqrt(var[c][k]) * rng.randn(3) for c, k in zip(ct, src)])
        T = np.ascontiguousarray(np.asarray(f["T"], dtype=np.float64))
        _cache[key] = (T, Xs, cs, Xt, ct, mu, var)
    return _cache[key]


def _step(m, T, Xs, cs, Xt, ct, u, a=None):
    from gpmdm_amd import backward_sample_step
    k, ld = backward_sample_step(m, T, Xs, cs, Xt, ct, u, a)
    return k.numpy(), ld.numpy()


def _checked(m, T, Xs, cs, Xt, ct, u, mu, var, a=None, what=""):
    k, ld = _step(m, T, Xs, cs, Xt, ct, u, a)
    near, near64, info = S.check_draws(T, Xs, cs, a, Xt, ct, u, k, mu, var, what)
    print(f"{what}: G {info['G']:.3g} eps {info['eps']:.2e} near-boundary draws {near} (fp64 numpy {near64}) of {len(u)}")
    assert near <= S.near_cap(len(u)), (what, near)
    return k, ld, info


@pytest.mark.parametrize("n_s", SIZES)
def test_mid_interval_targets(m2, fx_config2, n_s):
    """u at the middle of source k*'s interval gives k* exactly: the first and the last source of
    positive term, the last source of range 0 and the first of range 1, one in the ragged last
    range, and a spread of others."""
    T, Xs, cs, Xt, ct, mu, var = _clouds(m2, fx_config2, n_s, 16, seed=1)
    F, pos, _, _ = S.cdf(T, Xs, cs, None, Xt, ct, mu, var)
    want = {0, n_s - 1, n_s // 2, R - 1, R, 2 * R + 3, 64, 63}
    ks = sorted(k for k in want if 0 <= k < n_s)
    nr = (n_s + R - 1) // R
    assert all(k in ks for k in (R - 1, R) if k < n_s) and (nr < 3 or ks[-2] >= 2 * R)
    for k in ks:
        assert pos[:, 0].all()                              # T has no zeros: the first and last source are 0, n_s - 1
        lo = np.where(k > 0, F[k - 1], 0)
        assert np.all(F[k] - lo > 1e-6), (n_s, k, float((F[k] - lo).min()))
        u = ((lo + F[k]) / 2).astype(np.float64)
        got, _ = _step(m2, T, Xs, cs, Xt, ct, u)
        assert np.array_equal(got, np.full(16, k)), (n_s, k, got)


def test_edges(m2, fx_config2):
    """u = 0, u = 1 - 2^-53, zeros in T and in a, an unreachable class, duplicate sources."""
    n_s, n_t = R + 40, 64
    T, Xs, cs, Xt, ct, mu, var = _clouds(m2, fx_config2, n_s, n_t, seed=2)
    # zeros in T: class-1 sources never reach class-0 targets
    Tz = np.array([[0.5, 0.5], [0.0, 1.0]])
    for name, u in (("u = 0", np.zeros(n_t)), ("u = 1 - 2^-53", np.full(n_t, 1 - 2.0 ** -53)),
                    ("random u", np.random.RandomState(5).uniform(size=n_t))):
        k, _, info = _checked(m2, Tz, Xs, cs, Xt, ct, u, mu, var, what=f"T with a zero, {name}")
        assert np.all(k >= 0) and not np.any((cs[k] == 1) & (ct == 0)), name
        if name == "u = 0":                                 # the lowest source of positive term
            first0, first = int(np.nonzero(cs == 0)[0][0]), 0
            assert np.array_equal(k, np.where(ct == 0, first0, first))
    # zeros in a: never returned, wherever u falls
    a = np.random.RandomState(6).uniform(0.1, 1.0, n_s)
    zero = np.random.RandomState(7).rand(n_s) < 0.5
    zero[[0, n_s - 1, R - 1, R]] = True
    a[zero] = 0.0
    a /= a.sum()
    for name, u in (("u = 0", np.zeros(n_t)), ("u = 1 - 2^-53", np.full(n_t, 1 - 2.0 ** -53)),
                    ("random u", np.random.RandomState(8).uniform(size=n_t))):
        k, _, _ = _checked(m2, T, Xs, cs, Xt, ct, u, mu, var, a=a, what=f"zeros in a, {name}")
        assert np.all(k >= 0) and np.all(a[k] > 0), name
    # nobody reaches class 0: -1 and -inf there, the neighbours served
    Tn = np.array([[0.0, 1.0], [0.0, 1.0]])
    u = np.random.RandomState(9).uniform(size=n_t)
    k, ld, _ = _checked(m2, Tn, Xs, cs, Xt, ct, u, mu, var, what="unreachable class")
    assert (ct == 0).sum() >= 5 and (ct == 1).sum() >= 5
    assert np.all(k[ct == 0] == -1) and np.all(ld[ct == 0] == -np.inf)
    assert np.all(k[ct == 1] >= 0) and np.all(np.isfinite(ld[ct == 1]))
    # exact duplicates among the sources
    pick = np.random.RandomState(10).randint(0, 40, n_s)
    Xd, cd = np.ascontiguousarray(Xs[pick]), cs[pick]
    mud, vard = _moments(m2, Xd)
    _checked(m2, T, Xd, cd, Xt, ct, u, mud, vard, what="duplicate sources")


def test_a_regular_grid_of_uniforms(m2, fx_config2):
    """4096 copies of one target with u_i = (i + 0.5) / 4096 against 50 sources: each source is
    returned 4096 p_k times to within 1, and the indices never decrease."""
    T, Xs, cs, Xt, ct, mu, var = _clouds(m2, fx_config2, 50, 1, seed=3)
    n = 4096
    Xg, cg = np.repeat(Xt, n, axis=0), np.repeat(ct, n)
    u = (np.arange(n) + 0.5) / n
    k, _ = _step(m2, T, Xs, cs, Xg, cg, u)
    F, _, _, _ = S.cdf(T, Xs, cs, None, Xt, ct, mu, var)
    p = np.diff(np.concatenate([[0], F[:, 0]])).astype(np.float64)
    assert np.all(np.diff(k) >= 0) and k.min() >= 0
    counts = np.bincount(k, minlength=50)
    assert np.all(np.abs(counts - n * p) <= 1), float(np.abs(counts - n * p).max())


def test_independence_of_the_other_targets(m2, fx_config2):
    """A target's index and log_den bits are the same alone, in reversed order, in a subset, and
    from one call to the next."""
    n_s, n_t = R + 1, 257
    T, Xs, cs, Xt, ct, mu, var = _clouds(m2, fx_config2, n_s, n_t, seed=4)
    assert 0 < ct.sum() < n_t
    u = np.random.RandomState(11).uniform(size=n_t)
    k, ld, _ = _checked(m2, T, Xs, cs, Xt, ct, u, mu, var, what="257 targets")
    k2, ld2 = _step(m2, T, Xs, cs, Xt, ct, u)
    assert k.tobytes() == k2.tobytes() and ld.tobytes() == ld2.tobytes()
    kr, lr = _step(m2, T, Xs, cs, Xt[::-1].copy(), ct[::-1].copy(), u[::-1].copy())
    assert np.array_equal(kr[::-1], k) and lr[::-1].tobytes() == ld.tobytes()
    sub = np.random.RandomState(12).permutation(n_t)[:100]
    ks, ls = _step(m2, T, Xs, cs, Xt[sub].copy(), ct[sub].copy(), u[sub].copy())
    assert np.array_equal(ks, k[sub]) and ls.tobytes() == ld[sub].tobytes()
    for j in range(n_t):
        k1, l1 = _step(m2, T, Xs, cs, Xt[j:j + 1].copy(), ct[j:j + 1].copy(), u[j:j + 1].copy())
        assert k1[0] == k[j] and l1.tobytes() == ld[j:j + 1].tobytes(), j


@pytest.mark.parametrize("n_s", [65, 2 * R + 7])
def test_log_den(m2, fx_config2, n_s):
    T, Xs, cs, Xt, ct, mu, var = _clouds(m2, fx_config2, n_s, 300, seed=5)
    a = np.random.RandomState(13).uniform(0.01, 1.0, n_s)
    a /= a.sum()
    u = np.random.RandomState(14).uniform(size=300)
    _, ld, info = _checked(m2, T, Xs, cs, Xt, ct, u, mu, var, a=a, what=f"log_den {n_s}")
    ref = info["log_den"]
    err = float(np.abs(ld - ref).max())
    print(f"log_den {n_s}: max error {err:.3g}, band {info['eps']:.3g}")
    assert err <= info["eps"]


def test_refusals(m2, fx_config2):
    lib = _lib.load()
    T, Xs, cs, Xt, ct, mu, var = _clouds(m2, fx_config2, 65, 300, seed=5)
    cs64, ct64 = cs.astype(np.int64), ct.astype(np.int64)
    idx, ld = np.zeros(300, dtype=np.int64), np.zeros(300)

    def call(n_s=65, n_t=300, cs_=cs64, ct_=ct64, u=None):
        u = np.full(300, 0.5) if u is None else u
        return lib.gpmdm_backward_sample_step(m2.handle, _lib.dptr(T), n_s, _lib.dptr(Xs), _lib.i64ptr(cs_), None, n_t,
                                              _lib.dptr(Xt), _lib.i64ptr(ct_), _lib.dptr(u), _lib.i64ptr(idx),
                                              _lib.dptr(ld), None)

    assert call() == _lib.GPMDM_OK
    for bad in (1.0, -1e-300, 1.5, np.nan):
        u = np.full(300, 0.5)
        u[17] = bad
        assert call(u=u) == _lib.GPMDM_E_INVALID and b"[0, 1)" in lib.gpmdm_last_error(), bad
    for bad in (2, -1):
        c = ct64.copy()
        c[5] = bad
        assert call(ct_=c) == _lib.GPMDM_E_INVALID and b"[0, C)" in lib.gpmdm_last_error()
        c = cs64.copy()
        c[5] = bad
        assert call(cs_=c) == _lib.GPMDM_E_INVALID
    # above 2^36 pairs: refused on the sizes alone (no array of that size exists)
    assert call(n_s=1 << 20, n_t=(1 << 16) + 1) == _lib.GPMDM_E_INVALID and b"2^36" in lib.gpmdm_last_error()
    from gpmdm_amd import backward_sample_step
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        backward_sample_step(m2, T, Xs, cs, Xt, ct, np.full(300, 1.0))
