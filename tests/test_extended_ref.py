"""Host tests (no GPU) of the extended-precision reference and of the yardstick the GPU
accuracy tests (tests/test_gpu_gp_accuracy.py) hold the device to.

* the reference against mpmath at 50 digits;
* the fp64 oracle's own per-point error against the reference on the accuracy tests' model
  recipe, every dense latent dimension, with the conditions that make a bound of "a small
  multiple of the oracle's error" meaningful: moderately conditioned kernel matrices,
  predictive variances well above rounding, and a yardstick that stays tight;
* gp_tile.h's table-driven ``exp2_64`` restated in numpy fp64 against longdouble ``exp`` over
  the sweep the GPU test issues, and that the same check rejects a table entry or a
  polynomial coefficient perturbed in its 12th digit.
"""
import re

import numpy as np
import pytest

import extended_ref as E
from extended_ref import LD, EPS64

DENSE_D = list(range(1, 17)) + [24, 32]


def rel(a, ref):
    return np.abs((E.ld(a) - ref) / ref).astype(np.float64)


# ----------------------------------------------------------------------------
# the reference itself
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("tight", [False, True])
def test_reference_vs_mpmath(tight):
    """obs_map / dyn_map of an N = 40, d = 2 model against the same formulas in mpmath at 50
    digits (mpmath's own matrix inverse).

    Everywhere, both GPs: |d vc| <= 4 eps_ld (k_diag + sum_i |k_i (K^-1 k)_i|) and
    |d mu| <= 4 eps_ld abs_scale_mu, with eps_ld = 2^-63 = 1.08e-19: 4.3e-19 of the magnitude
    of the terms summed.  vc = k_diag - |L^-1 k|^2 is a difference of O(1) numbers (O(1e2)
    for the dynamics GP, whose linear kernel is large and nearly cancels), each rounded to
    eps_ld, so a few eps_ld of that magnitude is the format's floor whatever the algorithm.
    ``tight=False``: sigma_y = 0.5 and spread latents, so every observation-GP vc >= 0.05,
    where a relative 1e-17 is within that floor's reach: the observation GP's vc and mu agree
    to 1e-17 relative to themselves.
    ``tight=True``: the accuracy tests' own noise levels (sigma_y = 0.15: vc down to 4e-3, as
    the points that carry the filter's weight), where the floor is 1e-16 relative to vc: two
    decades below the tightest fp64 yardstick (60 eps = 1.3e-14)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    p = E.recipe_model(2, C=2, S=2, L=10, D=3, seed=5, x_scale=None if tight else 2.0)
    if not tight:
        p["y_log_sigma_n"] = p["x_log_sigma_n"] = float(np.log(0.5))
    ref = E.ExtendedModel(p)
    xs, _ = E.regime_points(p, per=3)
    xs = xs[:12]                                   # the underflow regime has mu = 0, vc = 1 exactly
    eps_ld = mp.mpf(float(np.finfo(LD).eps))

    def from_ld(v):                                # exact: a longdouble is the sum of two doubles
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))

    mpf = lambda a: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])  # noqa: E731

    def mp_rbf(A, B, log_ls):
        ls = [mp.exp(mp.mpf(float(v))) for v in log_ls]
        K = mp.zeros(A.shape[0], B.shape[0])
        for i in range(A.shape[0]):
            for j in range(B.shape[0]):
                K[i, j] = mp.exp(-sum(((mp.mpf(float(A[i, k])) - mp.mpf(float(B[j, k]))) / ls[k]) ** 2
                                      for k in range(A.shape[1])))
        return K

    def mp_lin(A, B, log_c):
        c2 = [mp.exp(mp.mpf(float(v))) ** 2 for v in log_c]
        K = mp.zeros(A.shape[0], B.shape[0])
        for i in range(A.shape[0]):
            for j in range(B.shape[0]):
                K[i, j] = sum(c2[k] * mp.mpf(float(A[i, k])) * mp.mpf(float(B[j, k]))
                              for k in range(A.shape[1])) + c2[-1]
        return K

    def check(K, k, M, kd, mu_ref, vc_ref, what, literal):
        Kinv = mp.inverse(K)                       # 50 digits against cond(K) <= 1e6: exact for this purpose
        sol, Minv = Kinv * k, Kinv * M
        for q in range(k.cols):
            vc = kd[q] - sum(k[i, q] * sol[i, q] for i in range(k.rows))
            vsc = kd[q] + sum(abs(k[i, q] * sol[i, q]) for i in range(k.rows))
            dv = abs(from_ld(vc_ref[q]) - vc)
            assert dv <= 4 * eps_ld * vsc, (what, q, float(dv), float(vc))
            if literal:
                assert vc >= mp.mpf("0.05") and dv / vc < mp.mpf("1e-17"), (what, q, float(dv / vc), float(vc))
            for j in range(M.cols):
                mu = sum(k[i, q] * Minv[i, j] for i in range(k.rows))
                sc = sum(abs(k[i, q] * Minv[i, j]) for i in range(k.rows))
                dm = abs(from_ld(mu_ref[q, j]) - mu)
                assert dm <= 4 * eps_ld * sc, (what, q, j, float(dm / sc))
                if literal:
                    assert dm / abs(mu) < mp.mpf("1e-17"), (what, q, j, float(dm / abs(mu)))

    N = p["X"].shape[0]
    sy2 = mp.exp(mp.mpf(p["y_log_sigma_n"])) ** 2
    K = mp_rbf(p["X"], p["X"], p["y_log_lengthscales"]) + sy2 * mp.eye(N)
    mu, vc = ref.obs_map(xs)
    check(K, mp_rbf(p["X"], xs, p["y_log_lengthscales"]), mpf(p["Y"]), [mp.mpf(1)] * len(xs), mu, vc, "obs", not tight)
    sx2 = mp.exp(mp.mpf(p["x_log_sigma_n"])) ** 2
    c2 = [mp.exp(mp.mpf(float(v))) ** 2 for v in p["x_log_lin_coeff"]]
    kd = [1 + sum(c2[k] * mp.mpf(float(x[k])) ** 2 for k in range(2)) + c2[-1] for x in xs]
    for c, (xi, xo) in enumerate(E.xin_xout(p["X"], p["seq_lengths"])):
        n = xi.shape[0]
        K = (mp_rbf(xi, xi, p["x_log_lengthscales"]) + sx2 * mp.eye(n) + mp_lin(xi, xi, p["x_log_lin_coeff"])
             + mp.mpf(float(1e-6)) * mp.eye(n))
        k = mp_rbf(xi, xs, p["x_log_lengthscales"]) + mp_lin(xi, xs, p["x_log_lin_coeff"])
        mu, vc = ref.dyn_map(xs, c)
        check(K, k, mpf(xo), kd, mu, vc, f"dyn {c}", False)


def test_reference_loglik_restates_the_oracle():
    """loglik restates O.log_likelihoods (double-counted log-variance, float32 constant):
    the two agree to the oracle's fp64 rounding, and the cutoff's tau flushes kernel values."""
    from oracle import gpmdm_oracle as O
    p = E.recipe_model(3)
    ref, om = E.ExtendedModel(p), E.oracle_of(p)
    xs, _ = E.regime_points(p, per=6)
    z = p["Y"][11]
    ll, terms = ref.loglik(xs, z)
    assert np.max(np.abs(O.log_likelihoods(om, xs, z) - ll.astype(np.float64)) / terms.astype(np.float64)) < 1e-9
    k = ref.obs_kernel(xs)
    tau = float(np.median(k[k > 0].astype(np.float64)))
    kt = ref.obs_kernel(xs, tau)
    assert np.all(kt[k < tau] == 0) and np.all(kt[k >= tau] == k[k >= tau]) and 0 < np.count_nonzero(kt) < k.size


# ----------------------------------------------------------------------------
# the yardstick and its conditions
# ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def yardsticks():
    out = {}
    for d in DENSE_D:
        p = E.recipe_model(d)
        ref, om = E.ExtendedModel(p), E.oracle_of(p)
        omt = om.with_triangular_dynamics()
        xs, reg = E.regime_points(p)
        mu_r, vc_r = ref.obs_map(xs)
        sc = ref.obs_abs_scale_mu(xs)
        mu_t, vc_t = E.oracle_obs_triangular(om, xs)
        mu_i, vc_i = E.oracle_obs_inverse(om, xs)
        rec = {"cond_y": float(np.linalg.cond(ref.Ky.astype(np.float64))),
               "cond_x": [float(np.linalg.cond(K.astype(np.float64))) for K in ref.Kx],
               "min_vc": float(vc_r.min()), "obs_tri": {}, "obs_inv": {}, "obs_mu": {}, "dyn_tri": {}, "dyn_mu": {}}
        dyn = []
        for c in range(2):
            dmu_r, dvc_r = ref.dyn_map(xs, c)
            dmu, dvar = omt.map_x_dynamics_for_class(xs, c)
            dvc = dvar[:, 0] * np.exp(p["x_log_lambdas"][0]) ** 2
            dyn.append((rel(dvc, dvc_r), E.mu_error(dmu, dmu_r, ref.dyn_abs_scale_mu(xs, c))))
            rec["min_vc"] = min(rec["min_vc"], float(dvc_r.min()))
        for r, name in enumerate(E.REGIMES):
            sel = reg == r
            rec["obs_tri"][name] = float(rel(vc_t, vc_r)[sel].max())
            rec["obs_inv"][name] = float(rel(vc_i, vc_r)[sel].max())
            rec["obs_mu"][name] = float(E.mu_error(mu_t, mu_r, sc)[sel].max())
            rec["dyn_tri"][name] = float(max(dv[sel].max() for dv, _ in dyn))
            rec["dyn_mu"][name] = float(max(dm[sel].max() for _, dm in dyn))
        out[d] = rec
    return out


def test_yardstick_conditions(yardsticks):
    """On the accuracy tests' model recipe, d in {1..16, 24, 32}: 1e2 <= cond(K_y),
    cond(K_x,c) <= 1e6; min vc >= 1e-4; the fp64 oracle in the device's association
    (|R^T k|^2 for the observation GP, with_triangular_dynamics for the dynamics GP) is within
    1e-10 of the reference per point, relative in vc and over abs_scale_mu in the means, in
    every regime.  (Measured here: cond 1e2..5e3, yardstick 60..5000 eps, min vc 6e-4.)  The
    explicit-inverse form is recorded beside it."""
    for d, r in yardsticks.items():
        print(d, {k: (v if not isinstance(v, dict) else {n: f"{x / EPS64:.0f}eps" for n, x in v.items()})
                  for k, v in r.items()})
        for cnd in [r["cond_y"], *r["cond_x"]]:
            assert 1e2 <= cnd <= 1e6, (d, cnd)
        assert r["min_vc"] >= 1e-4, (d, r["min_vc"])
        for key in ("obs_tri", "dyn_tri", "obs_mu", "dyn_mu"):
            for name, v in r[key].items():
                assert v <= 1e-10, (d, key, name, v)
        assert r["obs_tri"]["underflow"] == 0.0 and r["obs_inv"]["underflow"] == 0.0


def test_yardstick_cancellation_case():
    """d = 3 with the latents shifted by 50: the expansion form |a|^2 + |b|^2 - 2 a.b loses
    ~1e-12 in each kernel value (|a|^2 ~ 1e3..1e4), in the oracle too; the reference's
    difference form does not.  The yardstick rises but stays a usable bound (<= 1e-8)."""
    p = E.recipe_model(3, shift=50.0)
    ref, om = E.ExtendedModel(p), E.oracle_of(p)
    xs, reg = E.regime_points(p)
    _, vc_r = ref.obs_map(xs)
    _, vc_t = E.oracle_obs_triangular(om, xs)
    e = rel(vc_t, vc_r)
    print("cancellation yardstick per regime:", [float(e[reg == r].max()) for r in range(5)])
    assert 1e-13 < e[reg < 4].max() <= 1e-8
    assert vc_r.min() >= 1e-4


# ----------------------------------------------------------------------------
# exp2_64 on the host
# ----------------------------------------------------------------------------

def test_exp2_constants_are_the_headers():
    src = (E.ROOT / "gpmdm_amd" / "csrc" / "geometry.h").read_text()
    assert float(re.search(r"kLog2eX64\s*=\s*([0-9.]+)", src).group(1)) == E.K_SCALE
    assert E.exp2_poly() == E._POLY
    tab = E.exp2_table()
    exact = np.exp2(E.ld(np.arange(64)) / 64)
    assert np.all(tab == exact.astype(np.float64)), "kExp2Tab is not the correctly rounded 2^(j/64)"


def host_kernel_values(s, tab, poly=E._POLY):
    """The kernel value of gp_tile.h's generation for a particle at x = sqrt(s) against a
    training row at 0 with l = 1: asq = (x x) 64/ln2, t = -(asq + 0), exp2_64(t)."""
    x = np.sqrt(s)
    return x, E.exp2_64(-((x * x) * E.K_SCALE + 0.0), tab, poly)


def test_exp2_64_host_sweep():
    """The restated exp2_64 over the GPU test's sweep against longdouble exp: normal results
    to 8 (1 + s) eps (the fp64 floor is 0.5 (1 + s) eps: the argument's own rounding),
    subnormal results to that or 2 units of the smallest subnormal, exact 0 beyond, and
    non-increasing in s.  This pins the ALGORITHM's error on the CPU; the GPU may still
    differ in the last place, since the device contracts the multiply-adds this restatement
    rounds separately (only FMA contraction is at stake) -- tests/test_gpu_gp_accuracy.py
    holds the device itself to the same bound."""
    s = E.exp_sweep()
    x, k = host_kernel_values(s, E.exp2_table())
    worst, bad = E.exp_errors(k, x)
    print(f"host exp2_64: {s.size} points, worst err / ((1+s) eps) = {worst:.3f}")
    assert not bad, bad[:10]
    assert worst <= 8.0
    # numpy's own exp on the same argument: the floor the factor 8 is measured against
    floor, _ = E.exp_errors(np.exp(-(x * x)), x)
    print(f"numpy exp(-(x x)): worst err / ((1+s) eps) = {floor:.3f}")
    assert floor <= 1.0


def test_exp2_64_exact_arguments():
    """exp2_64 at exactly representable t, where the argument carries no error: every
    half-integer tie (rint to even on both parities), the table index wrap (n mod 64 = 0, 1,
    63), negative n >> 6, the saturating int conversion and exact underflow.  Normal results
    within 2 eps of 2^(t/64): half an ulp for the table entry, half for the final
    multiply-add, and the polynomial's truncation 2^-55 with its own rounding scaled by
    |p| <= 0.0055."""
    tab = E.exp2_table()
    n = np.concatenate([np.arange(-70, 70), np.arange(-68800, -68500), np.arange(-65700, -65400)]).astype(np.float64)
    t = np.concatenate([n, n + 0.5, np.nextafter(n + 0.5, np.inf), np.nextafter(n + 0.5, -np.inf), n + 0.25, n - 0.37])
    k = E.exp2_64(t, tab)
    ref = np.exp2(E.ld(t) / 64)
    normal = ref >= LD(np.finfo(np.float64).tiny)
    assert rel(k[normal], ref[normal]).max() <= 2 * EPS64, rel(k[normal], ref[normal]).max() / EPS64
    sub = ~normal                                                             # subnormal: that, or one unit
    assert np.all(np.abs(E.ld(k[sub]) - ref[sub]) <= 2 * EPS64 * ref[sub] + LD(5e-324))
    for big in (-1e5, -2.0 ** 31, -2.0 ** 31 - 4096.0, -1e12, -1e300):
        assert E.exp2_64(np.array([big]), tab)[0] == 0.0, big
    assert E.exp2_64(np.array([-68736.0]), tab)[0] == 2.0 ** -1074            # the smallest subnormal, exactly
    assert E.exp2_64(np.array([0.0, -64.0, 64.0]), tab).tolist() == [1.0, 0.5, 2.0]


@pytest.mark.parametrize("what", ["table", "coefficient"])
def test_exp_check_rejects_a_12th_digit_error(what):
    """The sweep's check fails when one kExp2Tab entry, or the polynomial's linear
    coefficient, is off in its 12th significant digit -- an error the normwise map tests
    (1e-7 / 1e-8 of the batch maximum) cannot see."""
    tab, poly = E.exp2_table().copy(), list(E._POLY)
    if what == "table":
        tab[37] *= 1.0 + 1e-12
    else:
        poly[4] *= 1.0 + 1e-9            # 2^(f/64) - 1 ~ 0.0054 at |f| = 1/2: moves the value by 5e-12
    s = E.exp_sweep()
    x, k = host_kernel_values(s, tab, tuple(poly))
    worst, bad = E.exp_errors(k, x)
    assert bad and any(b[0] == "normal" for b in bad)
    # ... while the unperturbed values pass, and the perturbation is far below the old tolerances
    _, k0 = host_kernel_values(s, E.exp2_table())
    assert np.max(np.abs(k - k0)) < 1e-11
