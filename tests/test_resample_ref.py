"""CPU checks of tests/resample_ref.py, the extended-precision reference that
tests/test_gpu_resample_edges.py holds the device to: it agrees with the fp64 oracle on random
weights, its exact patterns are exact in any summation order, and the oracle's own fp64
indices pass the band check on every banded pattern (so the reference alone stays inside the
band the device is given)."""
import numpy as np
import pytest

import resample_ref as R
from oracle import gpmdm_oracle as O


def _nonties(cdf, u, margin=1e-12):
    """Uniforms that are not within ``margin`` of a CDF value (two correct CDFs may resolve
    those differently)."""
    c = np.asarray(cdf, dtype=np.float64)
    j = np.clip(np.searchsorted(c, u), 0, c.shape[0] - 1)
    near = np.minimum(np.abs(c[j] - u), np.abs(c[np.maximum(j - 1, 0)] - u))
    return near > margin


@pytest.mark.parametrize("P", [1, 2, 257, 5000])
def test_reference_matches_oracle_on_random_weights(P):
    rng = np.random.RandomState(P)
    ll = 5.0 * rng.randn(P)
    n = R.Normalised(ll)
    log_w, w = O.normalise(ll)
    assert np.max(np.abs(np.asarray(n.log_w, dtype=np.float64) - log_w)) <= 64 * R.EPS
    assert np.max(np.abs(np.asarray(n.w, dtype=np.float64) - w) / w) <= R.band_tol(P)
    u = rng.rand(P)
    keep = _nonties(n.cdf, u)
    assert keep.mean() > 0.99 or P < 10
    assert np.array_equal(R.multinomial_indices(n.cdf, u)[keep], O.multinomial_resample_indices(w, u)[keep])
    u0 = rng.rand()
    us = R.sys_u(np.arange(P), u0, P)
    assert np.array_equal(us, (np.arange(P, dtype=np.float64) + u0) / float(P))
    keep = _nonties(n.cdf, us)
    assert np.array_equal(R.systematic_indices(n.cdf, u0)[keep], O.systematic_resample_indices(w, u0)[keep])
    # read-outs at the oracle's ancestors
    C, d = 3, 2
    X, cls = rng.randn(P, d), rng.randint(0, C, P)
    idx = O.multinomial_resample_indices(w, u)
    post, mean, lik, scale = R.readouts(ll, cls, X, idx, C)
    tol = R.band_tol(P)
    assert np.max(np.abs(np.asarray(post, dtype=np.float64) - O.class_probabilities(ll, log_w, cls[idx], C))) <= tol
    assert np.all(np.abs(np.asarray(mean, dtype=np.float64) - O.current_state_mean(X[idx], w))
                  <= tol * np.asarray(scale, dtype=np.float64))
    assert abs(float(lik) - O.log_likelihood_readout(ll, log_w)) <= tol * float(lik)


def test_longdouble_is_extended():
    assert np.finfo(R.LD).nmant >= 63, "the reference needs a longdouble wider than fp64"


@pytest.mark.parametrize("P", R.SMALL_P + R.MULTI_P + R.GUIDE_P)
def test_exact_patterns_are_exact(P):
    """Every partial sum of e is an integer below 2^53 (so any association of the sum gives it
    exactly and the CDF is one correctly rounded division), e itself is exactly 0 or 1 for
    every c, and the fp64 CDF is the extended-precision one correctly rounded."""
    for name, mask in R.exact_patterns(P, large=P in R.GUIDE_P):
        assert mask.any(), (P, name)
        k = np.cumsum(mask.astype(np.int64))
        assert k[-1] < 2 ** 53
        for c in R.EXACT_C:
            ll = R.exact_ll(mask, c)
            assert np.max(ll) == c
            e = np.exp(ll - np.max(ll))
            assert np.array_equal(e, mask.astype(np.float64)), (P, name, c)
            n = R.Normalised(ll)
            assert np.array_equal(np.asarray(n.e, dtype=np.float64), e)
        cum = R.exact_cdf(mask)
        assert np.all(np.diff(cum) >= 0) and cum[-1] == 1.0
        n = R.Normalised(R.exact_ll(mask, 0.0))
        # (half an fp64 ulp: rounding the longdouble quotient again could double-round)
        assert np.all(np.abs(cum.astype(R.LD) - n.cdf) <= R.LD(R.EPS) * n.cdf), (P, name)
        # the oracle's sequential fp64 cumsum lands on the same values
        if P <= 5000:
            rng = np.random.RandomState(P)
            for u in R.edge_uniforms(cum, P, rng):
                assert u.shape == (P,) and np.all((u >= 0) & (u < 1))
                assert np.array_equal(np.searchsorted(cum, u, "left"),
                                      O.multinomial_resample_indices(mask.astype(np.float64), u)), (P, name)


def test_edge_uniforms_hold_the_specials():
    rng = np.random.RandomState(0)
    mask = R.exact_patterns(1025)[0][1]
    cum = R.exact_cdf(mask)
    u = np.concatenate(R.edge_uniforms(cum, 1025, rng))
    for v in (0.0, R.TINY, R.U_MAX):
        assert v in u
    assert np.intersect1d(u, cum).shape[0] >= 299          # CDF values themselves (1.0 clipped)
    assert np.intersect1d(u, np.nextafter(cum, 0.0)).shape[0] >= 299
    assert np.intersect1d(u, np.nextafter(cum, 1.0)).shape[0] >= 299
    # P = 1: one uniform per frame, every special in a frame of its own
    fr = R.edge_uniforms(np.array([1.0]), 1, rng)
    assert sorted(float(f[0]) for f in fr) == sorted([0.0, R.TINY, R.U_MAX, R.U_MAX, R.U_MAX, R.U_MAX])


@pytest.mark.parametrize("P", [1, 257, 1025, 4097, 300001])
def test_device_summation_order_is_exact_on_exact_patterns(P):
    """The claim Part 1 of the GPU tests rests on, checked on a host model of the device's
    own association (wave scans, wave bases, Hillis-Steele block offsets, chunk = 2 above 1024
    blocks): on exact patterns it gives fl(k_i / S) bit for bit."""
    for name, mask in R.exact_patterns(P, large=P > 5000):
        assert np.array_equal(R.device_association_cdf(mask.astype(np.float64)), R.exact_cdf(mask)), (P, name)


def test_device_summation_order_dips_inside_the_band():
    """In the device's association the CDF of general weights is not monotone: the block offset
    of block b and (offset + block sum) of block b - 1 are two associations of one sum, the
    lanes of a wave scan sum in different orders, and a late value can exceed the forced last
    bucket.  The dips are a few ulps, far inside the band, and k_resample's search on such a CDF
    still returns ancestors inside the band that do not decrease with the uniform -- on random
    uniforms and on uniforms placed on the CDF's own values.  (A host model of the summation
    order with numpy's exp; the device itself is held to the same checks in
    tests/test_gpu_resample_edges.py.)"""
    dips = 0
    for P in (5000, 300001):
        tol = R.band_tol(P)
        for name in R.BANDED:
            rng = np.random.RandomState(P + len(name))
            ll = R.banded_ll(name, P, rng)
            n = R.Normalised(ll)
            cdf = R.device_association_cdf(np.exp(ll - np.max(ll)))
            d = np.diff(cdf)
            dips += int(np.sum(d < 0))
            assert d.min() >= -8 * R.EPS, (P, name, d.min())
            assert np.max(np.abs(cdf.astype(R.LD) - n.cdf)) <= tol, (P, name)
            for u in (rng.rand(P), R.near_tie_uniforms(n.cdf, P, rng), R.near_tie_uniforms(cdf, P, rng)):
                idx = R.binary_search(cdf, u)
                assert idx.max() < P
                assert np.max(R.band_excess(n.cdf, u, idx)) <= tol, (P, name)
                assert np.all(np.diff(idx[np.argsort(u, kind="stable")]) >= 0), (P, name)
    assert dips > 0, "the model no longer shows the hazard this test documents"


@pytest.mark.parametrize("P", R.BANDED_P)
@pytest.mark.parametrize("name", R.BANDED)
def test_oracle_indices_pass_the_band_check(name, P):
    """The fp64 oracle (sequential cumsum) stays inside the band on every banded pattern, for
    both resample modes, with its offspring counts and its weights."""
    rng = np.random.RandomState(P + len(name))
    ll = R.banded_ll(name, P, rng)
    assert not np.any(np.isnan(ll)) and np.isfinite(np.max(ll))
    n = R.Normalised(ll)
    tol = R.band_tol(P)
    _, w = O.normalise(ll)
    assert np.max(R.rel_excess(w, n.w)) <= tol
    u = rng.rand(P)
    idx = O.multinomial_resample_indices(w, u)
    assert np.max(R.band_excess(n.cdf, u, idx)) <= tol
    o = np.argsort(u, kind="stable")
    assert np.all(np.diff(idx[o]) >= 0)
    u0 = rng.rand()
    idx = O.systematic_resample_indices(w, u0)
    assert np.max(R.band_excess(n.cdf, R.sys_u(np.arange(P), u0, P), idx)) <= tol
    assert np.all(np.diff(idx) >= 0)
    assert np.max(R.offspring_excess(n.w, idx)) <= P * tol
    # the reference's own indices use none of the band
    assert np.max(R.band_excess(n.cdf, u, R.multinomial_indices(n.cdf, u))) == 0
