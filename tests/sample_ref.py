"""Extended-precision reference for backward simulation (tests only; a plain module).

An ``np.longdouble`` restatement of gpmdm_hip.h's definition of ``gpmdm_backward_sample_step`` on
``backsmooth_ref.log_f``: the cumulative distribution over the sources, in index order,

    F_j(k) = sum_{i <= k} a_i f_ij / D_j,      D_j = sum_k a_k f_kj,

formed from one exp per pair (largest term 1) and a running sum in longdouble.  ``dtype=np.float64``
gives the fp64 yardstick: the same statements in the device's number format.  The step returns the
lowest k with F_j(k) > u_j.

Acceptance of a device index k for uniform u: k's term is positive in the reference and

    F(k - 1) - eps <= u <= F(k) + eps,        eps = backsmooth_ref.band_rel(info)

(the band of the marginal smoother's denominators: every partial sum is such a sum, so its error
relative to D_j stays inside it).  A draw is *near a boundary* when k is accepted but differs from
the reference's own k.

The uniforms of ``gpmdm_pf_sample_trajectories``: Philox4x32-10 with the filter's key and counter
(trajectory m, frame, stream 6, lag l), ``u01_co`` of the first two words.
"""
from __future__ import annotations

import numpy as np

import backsmooth_ref as B
from extended_ref import LD
from oracle import philox

STREAM_BACK_SAMPLE = 6


def uniforms(seed: int, frame: int, n: int, lag: int) -> np.ndarray:
    """(lag + 1, n): u[l, m] of trajectory m at lag l."""
    k0, k1 = philox.filter_key(seed)
    m = np.arange(n, dtype=np.uint32)[None, :]
    l = np.arange(lag + 1, dtype=np.uint32)[:, None]
    x, y, _, _ = philox.philox4x32_10(m, np.uint32(frame), np.uint32(STREAM_BACK_SAMPLE), l, k0, k1)
    return philox.u01_co(x, y)


def start(u0, P):
    """j_0 = min(P - 1, floor(u P))."""
    return np.minimum(P - 1, np.floor(np.asarray(u0, dtype=np.float64) * P).astype(np.int64))


def cdf(T, Xs, cs, a, Xt, ct, mu, var, dtype=LD):
    """(F, pos, log_den, info): F (n_s, n_t) the cumulative distribution per target (zeros where no
    source reaches it), pos the pairs of positive term, info the band's G and K."""
    n_s, n_t = len(cs), len(ct)
    d = np.asarray(Xs).shape[1]
    a = np.full(n_s, dtype(1) / dtype(n_s), dtype=dtype) if a is None else np.asarray(a, dtype=dtype)
    lf = B.log_f(T, Xs, cs, Xt, ct, mu, var, dtype)
    L = lf + B._log(a, dtype)[:, None]
    pos = L > B.NEG_INF
    M = L.max(axis=0)
    reach = M > B.NEG_INF
    Ms = np.where(reach, M, dtype(0))
    E = np.exp(L - Ms[None, :])
    E[:, ~reach] = 0
    cum = np.cumsum(E, axis=0, dtype=dtype)
    S = cum[-1]
    F = cum / np.where(reach, S, dtype(1))[None, :]
    log_den = np.where(reach, Ms + np.log(np.where(reach, S, dtype(1))), dtype(B.NEG_INF))
    fin = np.isfinite(lf.astype(np.float64))
    G = float(np.abs(lf[fin]).max()) if fin.any() else 0.0

    def mx(x):
        x = np.abs(np.asarray(x, dtype=np.float64))
        x = x[np.isfinite(x)]
        return float(x.max()) if x.size else 0.0

    a64 = np.asarray(a, dtype=np.float64)
    vv = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in var])
    K = (mx(np.log(a64[a64 > 0])) + mx(B._log(np.asarray(T, dtype=np.float64), np.float64)) +
         0.5 * d * mx(np.log(vv[vv > 0])) + 0.5 * d * np.log(2 * np.pi))
    return F, pos, log_den, dict(G=G, K=K, d=d, n_s=n_s, n_t=n_t)


def pick(F, pos, u):
    """The reference's own index per target: the lowest k with F(k) > u; no crossing (u at the top
    by rounding): the last source of positive term; -1 when no source reaches the target."""
    n_s, n_t = F.shape
    out = np.full(n_t, -1, dtype=np.int64)
    for j in range(n_t):
        p = np.nonzero(pos[:, j])[0]
        if p.size == 0 or not F[-1, j] > 0:
            continue
        k = int(np.searchsorted(F[:, j], F.dtype.type(u[j]), side="right"))
        out[j] = k if k < n_s else int(p[-1])
    return out


def accepted(F, pos, k, u, eps):
    """Per target: does index k pass the acceptance rule (for -1: no source reaches the target)."""
    n_s, n_t = F.shape
    ok = np.zeros(n_t, dtype=bool)
    for j in range(n_t):
        kj = int(k[j])
        if kj < 0:
            ok[j] = not pos[:, j].any() or not F[-1, j] > 0
            continue
        lo = F[kj - 1, j] if kj > 0 else F.dtype.type(0)
        ok[j] = bool(pos[kj, j]) and lo - eps <= u[j] <= F[kj, j] + eps
    return ok


def check_draws(T, Xs, cs, a, Xt, ct, u, k, mu, var, what="", yardstick=True):
    """Assert the acceptance rule for every draw; returns (near-boundary draws of the device, of the
    fp64 yardstick (0 when it is not run), info)."""
    F, pos, log_den, info = cdf(T, Xs, cs, a, Xt, ct, mu, var)
    eps = B.band_rel(info)
    assert info["G"] <= 1e6 and eps <= 1e-9, (what, info, eps)
    ok = accepted(F, pos, np.asarray(k), np.asarray(u), eps)
    assert ok.all(), (what, "draws outside the band", np.nonzero(~ok)[0][:10].tolist())
    ref = pick(F, pos, u)
    near64 = 0
    if yardstick:
        F64, pos64, _, _ = cdf(T, Xs, cs, a, Xt, ct, mu, var, dtype=np.float64)
        near64 = int((pick(F64, pos64, u) != ref).sum())
    return int((np.asarray(k) != ref).sum()), near64, dict(info, eps=eps, log_den=log_den, ref=ref)


def near_cap(n_draws):
    """At most 1 draw in 1000 near a boundary, and never more than 3."""
    return min(3, n_draws // 1000)
