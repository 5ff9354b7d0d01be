"""Extended-precision reference for the marginal backward smoother (tests only; a plain module).

An ``np.longdouble`` restatement of gpmdm_hip.h's definitions of ``gpmdm_backward_step`` and
``gpmdm_pf_smoothed_marginal``.  It takes the clouds, ``T`` and the fp64 dynamics moments
(``GPMDM.map_x_dynamics_for_class`` of the source rows: ``mu``, ``var`` of shape (C, n_s, d)) as
exact.  It shares no arithmetic with the device: natural logarithms, a two-pass log-sum-exp
(maximum first), true divisions by v, and sums over the DISTINCT source and target rows with
their multiplicities (post-resample clouds hold few distinct rows; regrouping a sum of
non-negative terms changes it by longdouble rounding only), which is also what keeps the
reference affordable at P = 5000.  ``dtype=np.float64`` gives the fp64 yardstick: the same
statements in the device's number format.

The rounding band (DESIGN.md §3.6 derives it; u = 2^-53, natural logarithms):

    |d w_i| <= w_i (a + b G) u steps + 1e-300,      |d log_den_j| <= (a + b G) u,
    b = 2 d + 16,   a = 4 (d + 6) K + 2 (n_s + n_t) + 2000,

G the largest finite |log f| of the step, K the largest magnitude the other addends of a pair's
exponent reach together: max |log a| + max |log T| + d/2 max |log v| + d/2 log 2 pi + max |log w_t|
over the finite ones.  Per pass the exponent of a pair costs (4 + d) u on the quadratic form
(difference, 1/v, two products and d accumulations, each relative to the form), 2 u on the scale
by 1/2 log2 e and the add of the source's constant: (6 + d)(G + K) u; the constant itself costs
(d + 6) K u.  Two passes, plus 4 G u for the denominator's logarithm, the target's exponent and
its add to the pair's: b = 2 (6 + d) + 4.  The running sums add n u per pass (n positive terms in
sequence; their power-of-two rescaling is exact) and exp2 and its argument's subtraction less than
1000 u per pass.  A step's relative errors carry over linearly to the next (the weights enter
with non-negative coefficients), hence the factor ``steps``.
"""
from __future__ import annotations

import numpy as np

from extended_ref import LD

U = 2.0 ** -53
NEG_INF = -np.inf


def ld_sum(x):
    return np.asarray(x, dtype=LD).sum()


def _log(x, dtype):
    x = np.asarray(x, dtype=dtype)
    out = np.full(x.shape, NEG_INF, dtype=dtype)
    pos = x > 0
    out[pos] = np.log(x[pos])
    return out


def log_f(T, Xs, cs, Xt, ct, mu, var, dtype=LD):
    """log f_kj, (n_s, n_t); -inf where T is 0 or the source's variance is unusable."""
    T, Xs, Xt = (np.asarray(v, dtype=dtype) for v in (T, Xs, Xt))
    cs, ct = np.asarray(cs, dtype=np.int64), np.asarray(ct, dtype=np.int64)
    n_s, d = Xs.shape
    out = np.full((n_s, len(ct)), NEG_INF, dtype=dtype)
    logT = _log(T, dtype)
    for c in np.unique(ct):
        j = np.nonzero(ct == c)[0]
        m, v = np.asarray(mu[c], dtype=dtype), np.asarray(var[c], dtype=dtype)
        ok = np.all((np.asarray(var[c]) > 0) & np.isfinite(np.asarray(var[c], dtype=np.float64)), axis=1)
        vs = np.where(ok[:, None], v, dtype(1))
        acc = np.zeros((n_s, len(j)), dtype=dtype)
        for q in range(d):
            r = Xt[j, q][None, :] - m[:, q][:, None]
            acc += r * r / vs[:, q][:, None] + np.log(vs[:, q])[:, None]
        two_pi = dtype(8) * np.arctan(dtype(1))
        lf = logT[cs, c][:, None] - acc / dtype(2) - dtype(d) / dtype(2) * np.log(two_pi)
        lf[~ok, :] = NEG_INF
        out[:, j] = lf
    return out


def _distinct(X, c):
    """(first index of each distinct row of [X, c], inverse map)."""
    key = np.concatenate([np.ascontiguousarray(X, dtype=np.float64).view(np.int64).reshape(len(c), -1),
                          np.asarray(c, dtype=np.int64)[:, None]], axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return first, inv.reshape(-1)


def backward_step(T, Xs, cs, a, Xt, ct, wt, mu, var, dtype=LD, dedup=True):
    """(ws, log_den, info): the definitions, on distinct rows.  info: G and K of the band."""
    n_s, n_t = len(cs), len(ct)
    d = np.asarray(Xs).shape[1]
    a = np.full(n_s, dtype(1) / dtype(n_s), dtype=dtype) if a is None else np.asarray(a, dtype=dtype)
    wt = np.asarray(wt, dtype=dtype)
    if dedup:
        fs, inv_s = _distinct(Xs, cs)
        ft, inv_t = _distinct(Xt, ct)
    else:
        fs, inv_s, ft, inv_t = np.arange(n_s), np.arange(n_s), np.arange(n_t), np.arange(n_t)
    a_u = np.zeros(len(fs), dtype=dtype)
    np.add.at(a_u, inv_s, a)
    w_u = np.zeros(len(ft), dtype=dtype)
    np.add.at(w_u, inv_t, wt)
    lf = log_f(T, np.asarray(Xs)[fs], np.asarray(cs)[fs], np.asarray(Xt)[ft], np.asarray(ct)[ft],
               [np.asarray(m)[fs] for m in mu], [np.asarray(v)[fs] for v in var], dtype)
    L = lf + _log(a_u, dtype)[:, None]                      # log (a_k f_kj)
    M = L.max(axis=0)
    reach = M > NEG_INF
    Ms = np.where(reach, M, dtype(0))
    E = np.exp(L - Ms[None, :])                             # one exp per pair, largest term 1
    E[:, ~reach] = 0
    S = E.sum(axis=0)
    log_den_u = np.where(reach, Ms + np.log(np.where(reach, S, dtype(1))), dtype(NEG_INF))
    coef = np.where(reach, w_u / np.where(reach, S, dtype(1)), dtype(0))
    # E_ij / S_j = a_i f_ij / D_j for the group; a single source gets its share a_i / a_u of it
    ws_u = (E * coef[None, :]).sum(axis=1)
    share = np.where(a_u[inv_s] > 0, a / np.where(a_u[inv_s] > 0, a_u[inv_s], dtype(1)), dtype(0))
    ws = ws_u[inv_s] * share
    fin = np.isfinite(lf.astype(np.float64))
    G = float(np.abs(lf[fin]).max()) if fin.any() else 0.0

    def mx(x):
        x = np.abs(np.asarray(x, dtype=np.float64))
        x = x[np.isfinite(x)]
        return float(x.max()) if x.size else 0.0

    vv = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in var])
    K = (mx(np.log(np.asarray(a, dtype=np.float64)[np.asarray(a, dtype=np.float64) > 0])) +
         mx(_log(np.asarray(T, dtype=np.float64), np.float64)) + 0.5 * d * mx(np.log(vv[vv > 0])) +
         0.5 * d * np.log(2 * np.pi) +
         mx(np.log(np.asarray(wt, dtype=np.float64)[np.asarray(wt, dtype=np.float64) > 0])))
    return ws, log_den_u[inv_t], dict(G=G, K=K, d=d, n_s=n_s, n_t=n_t)


def band_rel(info, steps=1):
    """(a + b G) u steps: the relative band of a step's weights, the absolute band of log_den."""
    d = info["d"]
    b = 2 * d + 16
    a = 4 * (d + 6) * info["K"] + 2 * (info["n_s"] + info["n_t"]) + 2000
    return (a + b * info["G"]) * U * steps


def rows(w, X, cls, anc, C, dtype=LD):
    """The row fields of weights w on a slot: class masses, sum w X, mass, ess, ess_distinct."""
    w, X = np.asarray(w, dtype=dtype), np.asarray(X, dtype=dtype)
    cls = np.asarray(cls, dtype=np.int64)
    if anc is None:
        m = np.ones(len(w), dtype=np.int64)
    else:
        anc = np.asarray(anc, dtype=np.int64)
        m = np.bincount(anc, minlength=len(w))[anc]
    mass = w.sum()
    return dict(class_probabilities=np.array([w[cls == c].sum() for c in range(C)], dtype=dtype),
                state_mean=(w[:, None] * X).sum(axis=0), mass=mass, ess=mass * mass / (w * w).sum(),
                ess_distinct=mass * mass / (m.astype(dtype) * w * w).sum())


def smoothed_marginal(hist, root_has_anc, T, moments, lag_last, C, dtype=LD):
    """The smoother on exports ``hist`` (oldest first, the last one the current frame; keys
    states, classes, resample_idx).  moments(X) -> (mu, var) of shape (C, n, d), fp64.  Returns per
    lag 0..lag_last the weights, the row fields and the band's (G, K) maxima so far."""
    P = len(hist[-1]["classes"])
    w = np.full(P, dtype(1) / dtype(P), dtype=dtype)
    out, G, K = [], 0.0, 0.0
    for l in range(lag_last + 1):
        e = hist[-1 - l]
        has_anc = l < len(hist) - 1 or root_has_anc
        r = rows(w, e["states"], e["classes"], e["resample_idx"] if has_anc else None, C, dtype)
        out.append(dict(weights=w, rows=r, info=dict(G=G, K=K, d=np.asarray(e["states"]).shape[1], n_s=P, n_t=P)))
        if l < lag_last:
            src = hist[-2 - l]
            mu, var = moments(src["states"])
            w, _, info = backward_step(T, src["states"], src["classes"], None, e["states"], e["classes"], w,
                                       mu, var, dtype)
            G, K = max(G, info["G"]), max(K, info["K"])
    return out
