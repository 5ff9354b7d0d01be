"""Extended-precision reference for MAP trajectory decoding (tests only; a plain module).

An ``np.longdouble`` restatement of gpmdm_hip.h's definitions of ``gpmdm_map_step`` and
``gpmdm_pf_map_path`` on ``backsmooth_ref.log_f``.  Like that module it takes the clouds, ``T`` and
the fp64 dynamics moments (``mu``, ``var`` of shape (C, n_s, d)) as exact and shares no arithmetic
with the device: natural logarithms, true divisions by v.  A maximum does not see copies, so it
runs on the DISTINCT rows -- sources by (x, c, delta), targets by (x, c) -- each named by its
lowest index, which is the definitions' tie rule.  ``dtype=np.float64`` gives the fp64 yardstick.

Besides delta and psi, a step returns for every target the gap between its best candidate and the
best candidate from a *different* distinct source row (inf when there is none): psi is decided by
the arithmetic only where that gap exceeds twice the band.

The band (u = 2^-53, natural logarithms; DESIGN.md §3.6's accounting).  A candidate is
delta_k + log f_kj.  The device forms it in base 2 as fma(q, -1/2 log2 e, g) with q the pair's
quadratic form and g the source record's constant, which here holds delta_k log2 e too.  With

    G = the largest finite |log f| of the step,
    K = max |delta_k| + max |log T| + d/2 max |log v| + d/2 log 2 pi   (finite ones: what g's addends
        reach together),
    L = max finite |l_j|,

the quadratic form costs (4 + d) u relative to itself (difference, 1/v, two products, d
accumulations) and the scale by 1/2 log2 e and the add of g 2 u of the result: (6 + d)(G + K) u.
g itself costs (d + 6) K u (d logarithms and their sum, log T, the two constants' products, the
product delta_k log2 e and its add).  The winner goes back to natural logarithms and takes l_j in
one fma: the constant ln 2's rounding and the fma's, 2 u of a result of at most G + K + L, and the
comparison of candidates that were rounded the same way adds nothing.  Altogether

    |d delta_j| <= [(d + 8)(G + K) + (d + 6) K + 2 L] u =: band_step,

taken with (d + 10) for the device's log2 and the reference's own longdouble rounding (a chained
reference keeps its scores in longdouble from step to step).  A maximum is
1-Lipschitz in its candidates, and delta_k enters a candidate with coefficient 1: the error the
sources' scores carry goes through unchanged, so the bands of successive steps add.  B(l) is the
sum over the steps from the root down to lag l.  For every path p the device's and the reference's
joint scores then differ by at most B(0), which gives the two path checks of the tests: the
reference's score of the device's path is within 2 B(0) of the reference's optimum, and the paths
are equal where every gap along the reference's path exceeds 2 B.
"""
from __future__ import annotations

import numpy as np

from backsmooth_ref import LD, NEG_INF, U, _log, log_f


def _distinct(cols):
    """(first index of each distinct row, inverse map), the distinct rows in increasing first index."""
    key = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).reshape(len(c), -1).view(np.int64)
                          for c in cols], axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return first[order], rank[inv.reshape(-1)]


def _mx(x):
    x = np.abs(np.asarray(x, dtype=np.float64)).ravel()
    x = x[np.isfinite(x)]
    return float(x.max()) if x.size else 0.0


def map_step(T, Xs, cs, delta, Xt, ct, ll, mu, var, dtype=LD):
    """(delta_out, psi, gap, info): the definitions, on distinct rows.  info: G, K, L of the band."""
    Xs, Xt = np.asarray(Xs, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    cs, ct = np.asarray(cs, dtype=np.int64), np.asarray(ct, dtype=np.int64)
    n_s, n_t = len(cs), len(ct)
    d = Xs.shape[1]
    delta = np.zeros(n_s, dtype=dtype) if delta is None else np.asarray(delta, dtype=dtype)   # (a chain keeps its own precision)
    ll = np.zeros(n_t) if ll is None else np.asarray(ll, dtype=np.float64)
    fs, _ = _distinct([Xs, cs.astype(np.float64), delta.astype(np.float64)])
    ft, inv_t = _distinct([Xt, ct.astype(np.float64)])
    lf = log_f(T, Xs[fs], cs[fs], Xt[ft], ct[ft], [np.asarray(m)[fs] for m in mu], [np.asarray(v)[fs] for v in var],
               dtype)
    cand = lf + delta[fs][:, None]
    cand[np.isnan(cand.astype(np.float64))] = NEG_INF          # a NaN candidate never wins
    top = cand.argmax(axis=0)                                  # the first maximum: the lowest index
    best = cand[top, np.arange(len(ft))]
    rest = cand.copy()
    rest[top, np.arange(len(ft))] = NEG_INF
    second = rest.max(axis=0) if len(fs) > 1 else np.full(len(ft), NEG_INF, dtype=dtype)
    reach = best.astype(np.float64) > NEG_INF
    with np.errstate(invalid="ignore"):
        gap_u = np.where(reach, np.where(second.astype(np.float64) > NEG_INF, best - second, np.inf), np.inf)
    best, psi_u, gap = best[inv_t], np.where(reach, fs[top], -1)[inv_t], gap_u[inv_t].astype(np.float64)
    ok = (psi_u >= 0) & np.isfinite(ll)
    out = np.where(ok, np.where(ok, best, dtype(0)) + np.where(ok, ll, 0.0).astype(dtype), dtype(NEG_INF))
    psi = np.where(ok, psi_u, -1)
    gap = np.where(ok, gap, np.inf)
    vv = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in var])
    info = dict(G=_mx(lf), d=d, L=_mx(ll),
                K=_mx(delta) + _mx(_log(np.asarray(T, dtype=np.float64), np.float64)) +
                0.5 * d * _mx(np.log(vv[vv > 0])) + 0.5 * d * np.log(2 * np.pi))
    return out, psi, gap, info


def band_step(info):
    d = info["d"]
    return ((d + 10) * (info["G"] + info["K"]) + (d + 6) * info["K"] + 2 * info["L"]) * U


def slot_ll(e):
    """The ring's plane of an export: the log-likelihood of the proposal each particle copies."""
    return np.asarray(e["ll"], dtype=np.float64)[np.asarray(e["resample_idx"], dtype=np.int64)]


def map_path(hist, T, moments, n, dtype=LD):
    """The window of n lags on exports ``hist`` (oldest first, the last one the current frame; keys
    states, classes, ll, resample_idx).  moments(X) -> (mu, var) of shape (C, rows, d), fp64.
    Returns delta[l], psi[l], gap[l], B[l] for l = 0..n (psi, gap: l < n), the path and log_joint."""
    P = len(hist[-1]["classes"])
    delta, psi, gap, B, infos = [None] * (n + 1), [None] * n, [None] * n, [0.0] * (n + 1), [None] * n
    delta[n] = np.zeros(P, dtype=dtype)
    for l in range(n - 1, -1, -1):
        src, e = hist[-2 - l], hist[-1 - l]
        mu, var = moments(src["states"])
        delta[l], psi[l], gap[l], infos[l] = map_step(T, src["states"], src["classes"], delta[l + 1], e["states"],
                                                      e["classes"], slot_ll(e), mu, var, dtype)
        B[l] = B[l + 1] + band_step(infos[l])
    path = backtrack(delta[0], psi)
    lj = delta[0][path[0]] if path[0] >= 0 else dtype(NEG_INF)
    return dict(delta=delta, psi=psi, gap=gap, B=B, info=infos, path=path, log_joint=lj)


def backtrack(delta0, psi):
    """The lowest index attaining max delta_0, then psi; -1 from the first unreachable lag on."""
    d0 = np.asarray(delta0, dtype=np.float64)
    j = int(np.argmax(d0)) if np.any(d0 > NEG_INF) else -1
    path = [j]
    for p in psi:
        j = int(p[j]) if j >= 0 else -1
        path.append(j)
    return np.array(path, dtype=np.int64)


def path_score(hist, T, moments, path, dtype=LD):
    """sum_l [l_l(p_l) + log f(p_{l+1} -> p_l)] of a path p_0..p_n over the exports."""
    n = len(path) - 1
    tot = dtype(0)
    for l in range(n):
        src, e = hist[-2 - l], hist[-1 - l]
        k, j = int(path[l + 1]), int(path[l])
        mu, var = moments(np.asarray(src["states"])[k:k + 1])
        lf = log_f(T, np.asarray(src["states"])[k:k + 1], np.asarray(src["classes"])[k:k + 1],
                   np.asarray(e["states"])[j:j + 1], np.asarray(e["classes"])[j:j + 1], mu, var, dtype)[0, 0]
        tot = tot + lf + dtype(slot_ll(e)[j])
    return tot
