"""tests/gate_ref.py against itself and against the oracle (no GPU): the decision rule's edge
cases, and ``reweigh`` against the oracle's likelihood on the restricted model (the construction
tests/test_gpu_obs_mask.py uses for masked frames) -- which pins the reference the GPU tests
compare with to the oracle."""
import copy

import numpy as np

import gate_ref as G


def test_nan_zscores_never_exceed():
    zs = np.array([np.nan, 9.0, np.nan, -9.0, 0.5])
    ex, gated, used, overflow = G.decide(zs, None, 6.0, 0.5)
    assert ex.tolist() == [False, True, False, True, False]
    assert gated.tolist() == ex.tolist() and not overflow          # cap = floor(0.5 * 5) = 2
    assert used.tolist() == [True, False, True, False, True]
    ex, gated, used, overflow = G.decide(np.full(4, np.nan), None, 1.0, 1.0)
    assert not ex.any() and not gated.any() and used.all() and not overflow


def test_unobserved_joints_with_huge_z_are_ignored():
    zs = np.array([1e30, 7.0, 0.1, -1e30, 0.2, 0.3])
    obs = np.array([False, True, True, False, True, True])
    ex, gated, used, overflow = G.decide(zs, obs, 6.0, 0.5)        # cap = floor(0.5 * 4) = 2
    assert ex.tolist() == [False, True, False, False, False, False]
    assert gated.tolist() == ex.tolist() and not overflow
    assert used.tolist() == [False, False, True, False, True, True]


def test_at_the_cap_gated_one_above_overflow():
    D = 62
    assert G.cap_of(0.5, D) == 31
    zs = np.zeros(D)
    zs[:31] = 10.0
    ex, gated, used, overflow = G.decide(zs, None, 6.0, 0.5)
    assert ex.sum() == 31 and (gated == ex).all() and not overflow and used.sum() == 31
    zs[31] = -10.0
    ex, gated, used, overflow = G.decide(zs, None, 6.0, 0.5)
    assert ex.sum() == 32 and not gated.any() and overflow and used.all()


def test_cap_zero_gates_nothing():
    zs = np.array([10.0, 0.0, 0.0])
    ex, gated, used, overflow = G.decide(zs, None, 6.0, 0.3)       # floor(0.9) = 0
    assert ex.tolist() == [True, False, False] and not gated.any() and overflow and used.all()
    ex, gated, used, overflow = G.decide(np.zeros(3), None, 6.0, 0.3)
    assert not ex.any() and not overflow                            # nothing exceeded: no overflow either


def test_limit_one_with_everything_exceeded():
    zs = np.array([10.0, -11.0, 12.0])
    ex, gated, used, overflow = G.decide(zs, None, 6.0, 1.0)
    assert ex.all() and gated.all() and not used.any() and not overflow
    ll = G.reweigh(np.zeros((4, 3)), np.array([0.5, -1.0, 0.0, 2.0]), zs, used, np.ones(3))
    assert ll.tolist() == [0.0] * 4                                 # exactly 0, as a blackout frame


def _oracle(seed=3, C=2, S=2, L=12, d=3, D=7):
    from oracle import gpmdm_oracle as O
    rng = np.random.RandomState(seed)
    N = C * S * L
    X = rng.randn(N, d)
    Y = rng.randn(N, D)
    return O, O.OracleModel(
        X=X, Y=Y, seq_lengths=[[L] * S] * C, y_log_lengthscales=np.log(rng.uniform(1.0, 2.5, d)),
        y_log_lambdas=np.log(rng.uniform(0.5, 2, D)), y_log_sigma_n=np.log(0.15),
        x_log_lengthscales=np.log(rng.uniform(1.0, 2.5, d)), x_log_lambdas=np.log(rng.uniform(0.5, 2, d)),
        x_log_sigma_n=np.log(0.12), x_log_lin_coeff=np.log(rng.uniform(0.2, 0.8, d + 1))).precompute(), rng


def test_reweigh_is_the_oracles_likelihood_on_the_restricted_model():
    O, om, rng = _oracle()
    D = om.D
    st = om.X[rng.choice(om.X.shape[0], 9)] + 0.1 * rng.randn(9, om.d)
    z = om.Y[5] + 0.05 * rng.randn(D)
    il2 = np.exp(np.asarray(om.y_log_lambdas)) ** -2
    mu, var = om.map_x_to_y(st)
    vc = var[:, 0] / il2[0]
    assert np.all(vc > 0)
    for used in (np.ones(D, bool), np.arange(D) != 2, np.arange(D) % 2 == 0, np.arange(D) == D - 1):
        omr = copy.copy(om)
        omr.Y = om.Y[:, used]
        omr.y_log_lambdas = np.asarray(om.y_log_lambdas)[used]
        ref = O.log_likelihoods(omr, st, z[used])
        ll = np.asarray(G.reweigh(mu, vc, z, used, il2), dtype=np.float64)
        err = float(np.max(np.abs(ll - ref) / np.abs(ref)))
        print(f"used {int(used.sum())} of {D}: max rel {err:.3e}")
        assert err < 1e-12, (used, err)


def test_reweigh_is_nan_exactly_where_vc_is_not_positive():
    mu = np.zeros((5, 3))
    vc = np.array([0.5, 0.0, -0.25, np.nan, 1.0])
    ll = np.asarray(G.reweigh(mu, vc, np.ones(3), np.array([True, False, True]), np.array([1.0, 2.0, 4.0])),
                    dtype=np.float64)
    assert np.isnan(ll).tolist() == [False, True, True, True, False]
    const = float(np.float32(np.float32(1.0) * np.float32(1.8378770351409912)))
    # by hand at vc = 1: S' = 1 + 1/4, D' = 2, sum log il2 = log 4
    assert abs(ll[4] - (-0.5 * 1.25 - np.log(4.0) - const)) < 1e-15
