"""Extended-precision reference for the GP kernels (tests only; a plain module, no conftest).

A ``np.longdouble`` (x87, 64-bit mantissa) restatement of what ``oracle/gpmdm_oracle.py``
computes -- the two predictive maps (gpmdm.py:923-963, 1032-1068) and the filter's
per-particle log-likelihood (gpmdm_pf.py:183-192) -- taking the model's fp64 inputs (``X``,
``Y``, the log-hyperparameters, ``sigma_n_num_*``, ``seq_lengths``) as exact.  It deliberately
shares no arithmetic with the code it referees:

* the RBF kernel is evaluated in DIFFERENCE form ``exp(-sum(((x - x') / l)^2))``, not the
  expansion form ``|a|^2 + |b|^2 - 2 a.b`` that the reference, the fp64 oracle and the device
  share, so the expansion's cancellation error is part of what is measured;
* the linear algebra is a hand-written column Cholesky with forward / back substitution
  (``np.linalg`` does not take longdouble): ``vc = k_diag - |L^-1 k|^2``, mean weights by two
  triangular solves.  No inverse is formed.

An fp64 oracle cannot referee fp64 kernels tighter than its own rounding; this module can,
by about three decimal digits (eps = 2^-63 against 2^-52).  The fp64 *yardsticks* at the end
of the module are the oracle restated in the associations the device uses (``|R^T k|^2`` with
``R = U^-1``; the explicit inverse for the cutoff image): the GPU tests hold the device to a
small multiple of the error those achieve against this reference on the same points.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)

# Without a 64-bit mantissa every comparison below is meaningless: fail, do not skip.
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "tests/extended_ref.py needs an extended-precision np.longdouble (eps <= 2^-63); "
    f"this platform's has eps = {np.finfo(LD).eps}")

ROOT = Path(__file__).resolve().parents[1]


def ld(a):
    return np.asarray(a, dtype=LD)


# ----------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------

def rbf(X1, X2, log_ls):
    """exp(-sum_j ((x_j - x'_j) / l_j)^2), difference form (gpmdm.py:436-481, no 1/2)."""
    X1, X2 = ld(X1), ld(X2)
    ls = np.exp(ld(log_ls))
    acc = np.zeros((X1.shape[0], X2.shape[0]), dtype=LD)
    for j in range(X1.shape[1]):
        t = (X1[:, j, None] - X2[None, :, j]) / ls[j]
        acc += t * t
    return np.exp(-acc)


def lin(X1, X2, log_lin_coeff):
    """[x, 1] diag(c^2) [x', 1]^T (gpmdm.py:520-548)."""
    c2 = np.exp(ld(log_lin_coeff)) ** 2
    X1, X2 = ld(X1), ld(X2)
    return (X1 * c2[:-1]) @ X2.T + c2[-1]


def x_diag(Xs, log_lin_coeff):
    """1 + [x, 1] diag(c^2) [x, 1]^T (gpmdm.py:1070-1101, flg_noise=False)."""
    c2 = np.exp(ld(log_lin_coeff)) ** 2
    Xs = ld(Xs)
    return LD(1) + (Xs * Xs) @ c2[:-1] + c2[-1]


# ----------------------------------------------------------------------------
# linear algebra
# ----------------------------------------------------------------------------

def cholesky(A):
    """Lower Cholesky factor, column by column."""
    A = ld(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"not positive definite at column {j}")
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution (B: n x m)."""
    B = ld(B)
    V = np.zeros_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i]
    return V


def solve_upper_t(L, B):
    """L^-T B by back substitution."""
    B = ld(B)
    n = L.shape[0]
    V = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        V[i] = (B[i] - L[i + 1:, i] @ V[i + 1:]) / L[i, i]
    return V


# ----------------------------------------------------------------------------
# model
# ----------------------------------------------------------------------------

def xin_xout(X, seq_lengths):
    """Per class: (Xin_c, Xout_c), target 'full', back step 1 (gpmdm.py:630-718)."""
    out, off = [], 0
    for lens in seq_lengths:
        xi, xo = [], []
        for L in lens:
            seq = X[off:off + L]
            xi.append(seq[:-1])
            xo.append(seq[1:])
            off += L
        out.append((np.concatenate(xi), np.concatenate(xo)))
    return out


class ExtendedModel:
    """The longdouble model: factors once, evaluates any query set.

    ``p`` is a parameter dict as ``recipe_model`` returns (the oracle's constructor names)."""

    def __init__(self, p):
        self.p = p
        X = p["X"]
        N = X.shape[0]
        sy2 = np.exp(LD(p["y_log_sigma_n"])) ** 2 + LD(p.get("sigma_n_num_Y", 0.0)) ** 2
        Ky = rbf(X, X, p["y_log_lengthscales"]) + sy2 * np.eye(N, dtype=LD)
        self.Ky = Ky
        self.Ly = cholesky(Ky)
        self.beta = solve_upper_t(self.Ly, solve_lower(self.Ly, ld(p["Y"])))
        self.lam_y = np.exp(ld(p["y_log_lambdas"])) ** -2
        self.lam_x = np.exp(ld(p["x_log_lambdas"])) ** -2
        sx2 = np.exp(LD(p["x_log_sigma_n"])) ** 2 + LD(p.get("sigma_n_num_X", 0.0)) ** 2
        self.dyn = []
        self.Kx = []
        for xi, xo in xin_xout(X, p["seq_lengths"]):
            n = xi.shape[0]
            K = (rbf(xi, xi, p["x_log_lengthscales"]) + sx2 * np.eye(n, dtype=LD)
                 + lin(xi, xi, p["x_log_lin_coeff"]) + LD(1e-6) * np.eye(n, dtype=LD))
            L = cholesky(K)
            self.Kx.append(K)
            self.dyn.append((xi, L, solve_upper_t(L, solve_lower(L, ld(xo)))))

    def obs_kernel(self, xs, tau=None):
        k = rbf(self.p["X"], xs, self.p["y_log_lengthscales"])          # N x n
        if tau:
            k = np.where(k < LD(tau), LD(0), k)      # the cutoff's definition: flushed before the solves
        return k

    def obs_map(self, xs, tau=None):
        """(mu[n, D], vc[n]): mean and 1 - k^T K_y^-1 k of the observation GP."""
        k = self.obs_kernel(xs, tau)
        V = solve_lower(self.Ly, k)
        return k.T @ self.beta, LD(1) - np.sum(V * V, axis=0)

    def obs_abs_scale_mu(self, xs, tau=None):
        """sum_i |k_i| |beta_ij|: the backward-error scale of a mean."""
        return np.abs(self.obs_kernel(xs, tau)).T @ np.abs(self.beta)

    def cutoff_shift(self, xs, tau):
        """(vc(tau) - vc(0), mu(tau) - mu(0)) of the observation GP, each formed from the flushed
        values delta = k - k_tau themselves (vc(tau) - vc(0) = (L^-1 delta).(L^-1 (k + k_tau)),
        mu(tau) - mu(0) = -delta^T beta), so that shifts of 1e-23 keep their full relative
        precision instead of drowning in the two maps' own 1e-19 rounding."""
        k0, kt = self.obs_kernel(xs), self.obs_kernel(xs, tau)
        delta = k0 - kt
        dV, sV = solve_lower(self.Ly, delta), solve_lower(self.Ly, k0 + kt)
        return np.sum(dV * sV, axis=0), -(delta.T @ self.beta)

    def dyn_kernel(self, xs, c):
        xi = self.dyn[c][0]
        return rbf(xi, xs, self.p["x_log_lengthscales"]) + lin(xi, xs, self.p["x_log_lin_coeff"])

    def dyn_map(self, xs, c):
        """(mu[n, d], vc[n]) of class c's dynamics GP (RBF + linear, +1e-6 I on the block)."""
        _, L, alpha = self.dyn[c]
        k = self.dyn_kernel(xs, c)
        V = solve_lower(L, k)
        return k.T @ alpha, x_diag(xs, self.p["x_log_lin_coeff"]) - np.sum(V * V, axis=0)

    def dyn_abs_scale_mu(self, xs, c):
        return np.abs(self.dyn_kernel(xs, c)).T @ np.abs(self.dyn[c][2])

    def loglik(self, states, z, tau=None):
        """(ll[n], terms[n]): gpmdm_pf.py:183-192 with the reference's quirks (the log-variance
        counted twice, the float32 constant) and the magnitude of the terms ll sums
        (tests/test_gpu_large_configs.py: ll itself can cross 0)."""
        mu, vc = self.obs_map(states, tau)
        return loglik_from_map(mu, vc[:, None] * self.lam_y[None, :], z, dtype=LD)


def mu_error(mu, mu_ref, scale):
    """|mu - mu_ref| / abs_scale_mu per entry (float64).  The scale is floored at the smallest
    normal fp64 number: longdouble's exponent range is wider, so where every fp64 kernel value
    underflows the reference still holds means of 1e-1000 that no fp64 evaluation represents."""
    den = np.maximum(ld(scale), LD(np.finfo(np.float64).tiny))
    return (np.abs(ld(mu) - mu_ref) / den).astype(np.float64)


def vc_error(vc, vc_ref):
    return np.abs((ld(vc) - vc_ref) / vc_ref).astype(np.float64)


def loglik_from_map(mean, var, z, dtype=np.float64):
    """O.log_likelihoods' formula on a given (mean, var), and the terms' magnitude."""
    from oracle import gpmdm_oracle as O
    z = np.asarray(z, dtype=dtype)
    mean, var = np.asarray(mean, dtype=dtype), np.asarray(var, dtype=dtype)
    q = (z[None, :] - mean) ** 2 / var
    mu_term = dtype(-0.5) * np.sum(q + np.log(var), axis=1)
    sig_term = np.sum(-np.log(np.sqrt(var)), axis=1)
    const = dtype(O.loglik_const(z.shape[0]))
    terms = np.sum(q + 2 * np.abs(np.log(var)), axis=1) + abs(const)
    return mu_term + sig_term - const, terms


# ----------------------------------------------------------------------------
# model recipe and query regimes of the accuracy tests
# ----------------------------------------------------------------------------

REGIMES = ("train", "near", "mid", "far", "underflow")


def recipe_model(d, C=2, S=3, L=19, D=7, seed=None, x_scale=None, ls_range=(1.0, 2.0), shift=0.0):
    """Parameter dict of the accuracy tests' model (the oracle's constructor names plus
    ``seq_lengths``): X = randn sqrt(1.5 / d) -- so that the kernel matrix keeps off-diagonal
    mass at every d (conftest.synthetic_model's unit-variance latents decorrelate completely
    at d >= 16: K_y = (1 + sigma^2) I) --, length scales uniform(1, 2), sigma_y = 0.15,
    sigma_x = 0.12, lambdas and linear coefficients as conftest.synthetic_model, Y a smooth
    function of X plus noise.  N = C S L = 114 and S (L - 1) = 54 dynamics rows per class by
    default: neither a multiple of the 16-row K-step."""
    rng = np.random.RandomState(100 + d if seed is None else seed)
    N = C * S * L
    X = rng.randn(N, d) * (np.sqrt(1.5 / d) if x_scale is None else x_scale) + shift
    p = dict(
        y_log_lengthscales=np.log(rng.uniform(*ls_range, d)), y_log_lambdas=np.log(rng.uniform(0.5, 2, D)),
        y_log_sigma_n=float(np.log(0.15)), x_log_lengthscales=np.log(rng.uniform(*ls_range, d)),
        x_log_lambdas=np.log(rng.uniform(0.5, 2, d)), x_log_sigma_n=float(np.log(0.12)),
        x_log_lin_coeff=np.log(rng.uniform(0.2, 0.8, d + 1)))
    W = rng.randn(d, D)
    Y = np.sin((X - shift) @ W + rng.uniform(0, 6, D)) + 0.05 * rng.randn(N, D)
    p.update(X=X, Y=Y, seq_lengths=[[L] * S for _ in range(C)])
    return p


def y_sequences(p):
    out, s = [], 0
    for lens in p["seq_lengths"]:
        cls = []
        for L in lens:
            cls.append(p["Y"][s:s + L])
            s += L
        out.append(cls)
    return out


def hyper(p):
    return {k: v for k, v in p.items() if k not in ("X", "Y", "seq_lengths")}


def oracle_of(p):
    from oracle import gpmdm_oracle as O
    return O.OracleModel(X=p["X"], Y=p["Y"], seq_lengths=p["seq_lengths"], **hyper(p)).precompute()


def regime_points(p, per=30, seed=7):
    """``5 * per`` distinct query points, ``per`` per regime in REGIMES order: exact training
    points; X_i + 1e-3 randn; X_i + 0.3 randn / sqrt(d); X_i + 3 randn / sqrt(d);
    X.max(0) + 60 l (+ a distinct offset), where every kernel value underflows to 0."""
    X = p["X"]
    N, d = X.shape
    rng = np.random.RandomState(seed)
    pick = lambda: X[rng.choice(N, per, replace=N < per)]  # noqa: E731
    lmax = np.maximum(np.exp(p["y_log_lengthscales"]), np.exp(p["x_log_lengthscales"]))
    pts = [pick(),
           pick() + 1e-3 * rng.randn(per, d),
           pick() + 0.3 * rng.randn(per, d) / np.sqrt(d),
           pick() + 3.0 * rng.randn(per, d) / np.sqrt(d),
           X.max(0) + 60.0 * lmax + rng.rand(per, d)]
    return np.concatenate(pts), np.repeat(np.arange(5), per)


# ----------------------------------------------------------------------------
# fp64 yardsticks: the oracle in the associations the device uses
# ----------------------------------------------------------------------------

def oracle_obs_triangular(om, xs):
    """The fp64 oracle's observation map in the device's association (gp_tile.h): R = U^-1
    from the reference's Cholesky recipe, quadratic form |R^T k|^2, mean k^T (R R^T Y).
    Returns (mu[n, D], vc[n])."""
    from oracle import gpmdm_oracle as O
    Ky = O.rbf_kernel(om.X, om.X, om.y_log_lengthscales, om.y_log_sigma_n, om.sigma_n_num_Y, noise=True)
    R = np.linalg.inv(np.linalg.cholesky(Ky).T)
    beta = (R @ R.T) @ om.Y
    Ks = O.rbf_kernel(om.X, xs, om.y_log_lengthscales)
    V = Ks.T @ R
    return Ks.T @ beta, 1.0 - np.sum(V * V, axis=1)


def oracle_obs_inverse(om, xs, tau=None):
    """The fp64 oracle's observation map with the explicit inverse (O.map_x_to_y's own
    expressions), kernel values below ``tau`` flushed to 0 first.  (mu[n, D], vc[n])."""
    from oracle import gpmdm_oracle as O
    Ks = O.rbf_kernel(om.X, xs, om.y_log_lengthscales)
    if tau:
        Ks = np.where(Ks < tau, 0.0, Ks)
    mean = ((om.Y.T @ om.Ky_inv) @ Ks).T
    return mean, 1.0 - np.sum((Ks.T @ om.Ky_inv) * Ks.T, axis=1)


# ----------------------------------------------------------------------------
# exp2_64 (gp_tile.h), restated in numpy fp64
# ----------------------------------------------------------------------------

K_SCALE = 64.0 / np.log(2.0)          # kLog2eX64 (common.h); checked against the header in the tests
_POLY = (1.2417843701716925e-12, 5.732851688640402e-10, 2.1173137155464776e-07,
         5.86490495505617e-05, 0.010830424696249145)


def exp2_table():
    """kExp2Tab as gp_tile.h holds it (parsed from the file, so an edited entry is seen)."""
    src = (ROOT / "gpmdm_amd" / "csrc" / "gp_tile.h").read_text()
    body = re.search(r"kExp2Tab\[64\]\s*=\s*\{([^}]*)\}", src).group(1)
    tab = np.array([float(t) for t in body.replace("\n", " ").split(",") if t.strip()])
    assert tab.shape == (64,)
    return tab


def exp2_poly():
    """The polynomial's coefficients as gp_tile.h's exp2_64 holds them (highest first)."""
    src = (ROOT / "gpmdm_amd" / "csrc" / "gp_tile.h").read_text()
    body = src[src.index("double exp2_64("):]
    body = body[:body.index("ldexp")]
    c = re.findall(r"fma\(\w+,\s*([0-9.e+-]+),\s*([0-9.e+-]+)\)", body)
    first = [float(c[0][0]), float(c[0][1])]
    rest = [float(x) for x in re.findall(r"fma\(p,\s*f,\s*([0-9.e+-]+)\)", body)]
    return tuple(first + rest)


def exp2_64(t, tab, poly=_POLY):
    """gp_tile.h exp2_64: 2^(t/64) by n = rint(t), f = t - n, a degree-5 polynomial for
    2^(f/64) - 1, the table 2^(j/64) and ldexp.  numpy fp64 with separately rounded
    multiplies and adds where the device contracts to fma (numpy has no fma)."""
    t = np.asarray(t, dtype=np.float64)
    n = np.rint(t)
    f = t - n
    p = f * poly[0] + poly[1]
    for c in poly[2:]:
        p = p * f + c
    p = p * f
    ni = np.clip(n, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64).astype(np.int32)   # v_cvt_i32_f64 saturates
    tj = tab[ni & 63]
    return np.ldexp(tj * p + tj, ni >> 6)


def exp_sweep():
    """The s values of the exponential tests (kernel value exp(-s), s = x^2 at x = sqrt(s)):
    20 001 points linear in [0, 760]; the half-integers of t = 64 s / ln 2 with their fp64
    neighbours on both sides where rint(t) mod 64 is 0, 1 or 63 (the Sterbenz split at a tie,
    the table index wrap); the overflow / subnormal / underflow edges.  Sorted ascending."""
    s = [np.linspace(0.0, 760.0, 20001)]
    for n in list(range(0, 400)) + list(range(4000, 4200)) + list(range(65000, 65300)) + list(range(68600, 68900)):
        for h in (n + 0.5,):
            lo, hi = int(np.rint(np.nextafter(h, 0))), int(np.rint(np.nextafter(h, np.inf)))
            if {lo % 64, hi % 64} & {0, 1, 63}:
                sv = h / K_SCALE
                s.append(np.array([np.nextafter(np.nextafter(sv, 0), 0), np.nextafter(sv, 0), sv,
                                   np.nextafter(sv, np.inf), np.nextafter(np.nextafter(sv, np.inf), np.inf)]))
    s.append(np.array([708.0, 708.4, 744.4, 745.0, 745.2, 746.0, 1e3, 1e6, 1e12]))
    return np.unique(np.concatenate(s))


def exp_errors(k, x, scale=1.0):
    """Check kernel values ``k`` (fp64, or longdouble quotients of fp64 values) for
    exp(-(x / scale)^2) against longdouble: returns
    (worst err / ((1 + s) eps) over the normal results, list of failures).  Bounds: normal
    results 8 (1 + s) eps relative; subnormal results that or 2 units of the smallest
    subnormal; exactly 0 once the reference is below a quarter of the smallest subnormal;
    non-increasing in s to within the relative bound."""
    tiny, dmin = np.finfo(np.float64).tiny, 5e-324
    xs = ld(x) / LD(scale)
    s = xs * xs
    ref = np.exp(-s)
    k = ld(k)
    bound = 8.0 * (1.0 + s.astype(np.float64)) * EPS64
    bad = []
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.minimum(np.abs((k - ref) / ref), LD(1e300)).astype(np.float64)
    normal = ref >= LD(tiny)
    sub = (~normal) & (ref >= LD(dmin) / 4)
    zero = ref < LD(dmin) / 4
    for i in np.nonzero(normal & ~(rel <= bound))[0]:
        bad.append(("normal", float(s[i]), float(k[i]), float(rel[i] / bound[i] * 8)))
    units = np.minimum(np.abs(k - ref) / LD(dmin), LD(1e300)).astype(np.float64)
    for i in np.nonzero(sub & ~((rel <= bound) | (units <= 2.0)))[0]:
        bad.append(("subnormal", float(s[i]), float(k[i]), float(units[i])))
    for i in np.nonzero(zero & (k != 0.0))[0]:
        bad.append(("zero", float(s[i]), float(k[i]), 0.0))
    order = np.argsort(s.astype(np.float64), kind="stable")
    ko, bo = k[order], bound[order]
    up = np.nonzero(ko[1:] > ko[:-1] * (1 + 2 * ld(bo[1:])) + 2 * LD(dmin) * (ko[1:] < LD(tiny)))[0]
    for i in up:
        bad.append(("monotone", float(s[order][i + 1]), float(ko[i + 1]), float(ko[i])))
    worst = float(np.max(rel[normal] / ((1.0 + s[normal].astype(np.float64)) * EPS64))) if normal.any() else 0.0
    return worst, bad
