"""Self-checks of the innovation reference (tests/innov_ref.py); no GPU."""
import math

import numpy as np

import innov_ref as R

LD = np.longdouble


def _logpdf(z, mu, var):
    return -0.5 * (z - mu) ** 2 / var - 0.5 * np.log(2 * math.pi * var)


def test_single_particle_is_the_gaussian():
    """P = 1: spread 0, variance = vc il2, log_density the closed-form log-pdf, zscore (z - mu) / sd."""
    rng = np.random.default_rng(1)
    D = 7
    mu, z = rng.normal(size=(1, D)), rng.normal(size=D)
    il2, vc = rng.uniform(0.5, 2.0, D), np.array([0.3])
    r = R.innovation(mu, vc, z, None, il2)
    var = vc[0] * il2
    assert r.n_valid == 1
    assert np.all(r.spread == 0)
    assert np.allclose(np.asarray(r.mean, float), mu[0], rtol=0, atol=0)
    assert np.allclose(np.asarray(r.variance, float), var, rtol=1e-15)
    assert np.allclose(np.asarray(r.zscore, float), (z - mu[0]) / np.sqrt(var), rtol=1e-14)
    assert np.allclose(np.asarray(r.log_density, float), [_logpdf(z[j], mu[0, j], var[j]) for j in range(D)],
                       rtol=1e-14)


def test_two_particle_mixture_by_hand():
    """mu = (0, 2), vc = (1, 4), il2 = 1/2, z = 1: mean 1, spread 1, gp_variance 5/4, variance 9/4,
    residual 0; density 1/2 [N(1; 0, 1/2) + N(1; 2, 2)]."""
    r = R.innovation(np.array([[0.0], [2.0]]), np.array([1.0, 4.0]), np.array([1.0]), None, np.array([0.5]))
    assert float(r.mean[0]) == 1.0 and float(r.spread[0]) == 1.0
    assert float(r.gp_variance[0]) == 1.25 and float(r.variance[0]) == 2.25
    assert float(r.residual[0]) == 0.0 and float(r.zscore[0]) == 0.0
    dens = 0.5 * (math.exp(-1.0) / math.sqrt(math.pi) + math.exp(-0.25) / math.sqrt(4 * math.pi))
    assert abs(float(r.log_density[0]) - math.log(dens)) < 1e-15
    # a shifted z: zscore = residual / 1.5
    r = R.innovation(np.array([[0.0], [2.0]]), np.array([1.0, 4.0]), np.array([4.0]), None, np.array([0.5]))
    assert float(r.residual[0]) == 3.0 and abs(float(r.zscore[0]) - 2.0) < 1e-18


def test_pairwise_merge_equals_the_direct_sum():
    """(M, s) pairs merged over random partitions, in order, give the direct log-sum-exp."""
    rng = np.random.default_rng(2)
    for trial in range(20):
        n = int(rng.integers(1, 200))
        a = (rng.normal(size=n) * 30).astype(LD)
        M, s = R.lse_pair(a)
        direct = M + np.log(s)
        cuts = np.sort(rng.integers(0, n + 1, size=int(rng.integers(0, 12))))
        parts = np.split(a, cuts)                   # (empty parts included: the neutral pair)
        acc = (LD(-np.inf), LD(0))
        for p in parts:
            acc = R.lse_merge(acc, R.lse_pair(p))
        got = acc[0] + np.log(acc[1])
        assert abs(got - direct) <= 1e-17 * max(1.0, abs(float(direct))), (trial, float(got - direct))
    assert R.lse_merge((LD(-np.inf), LD(0)), (LD(-np.inf), LD(0))) == (LD(-np.inf), LD(0))


def test_invalid_particles_are_excluded_and_counted():
    rng = np.random.default_rng(3)
    P, D = 9, 4
    mu, z, il2 = rng.normal(size=(P, D)), rng.normal(size=D), rng.uniform(0.5, 2, D)
    vc = rng.uniform(0.1, 1.0, P)
    vc[[1, 4, 7]] = [0.0, -0.2, np.nan]
    keep = np.array([0, 2, 3, 5, 6, 8])
    r = R.innovation(mu, vc, z, None, il2)
    assert r.n_valid == 6
    # mean and spread over all P; the vc-dependent fields over the valid ones only
    assert np.allclose(np.asarray(r.mean, float), mu.mean(0), rtol=1e-15)
    assert np.allclose(np.asarray(r.spread, float), mu.var(0), rtol=1e-13)
    assert np.allclose(np.asarray(r.gp_variance, float), il2 * vc[keep].mean(), rtol=1e-15)
    dens = np.mean([np.exp(_logpdf(z, mu[p], vc[p] * il2)) for p in keep], axis=0)
    assert np.allclose(np.asarray(r.log_density, float), np.log(dens), rtol=1e-13)
    # none valid: NaN, and mean / spread / residual still served
    r0 = R.innovation(mu, np.full(P, -1.0), z, None, il2)
    assert r0.n_valid == 0
    for f in (r0.gp_variance, r0.variance, r0.zscore, r0.log_density):
        assert np.all(np.isnan(np.asarray(f, float)))
    assert np.all(np.isfinite(np.asarray(r0.mean, float))) and np.all(np.isfinite(np.asarray(r0.residual, float)))


def test_masked_joint_is_nan():
    rng = np.random.default_rng(4)
    P, D = 5, 6
    mu, il2, vc = rng.normal(size=(P, D)), rng.uniform(0.5, 2, D), rng.uniform(0.1, 1, P)
    z = rng.normal(size=D)
    obs = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    z[~obs] = np.nan
    r = R.innovation(mu, vc, z, obs, il2)
    full = R.innovation(mu, vc, np.where(obs, z, 0.0), None, il2)
    for f in ("residual", "zscore", "log_density"):
        got = np.asarray(getattr(r, f), float)
        assert np.all(np.isnan(got[~obs])), f
        assert np.array_equal(got[obs], np.asarray(getattr(full, f), float)[obs]), f
    for f in ("mean", "spread", "gp_variance", "variance"):
        assert np.all(np.isfinite(np.asarray(getattr(r, f), float))), f
