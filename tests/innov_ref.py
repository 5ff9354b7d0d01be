"""Extended-precision restatement of the innovation table (INTEGRATION.md "Innovations"): from
the particles' observation-GP means ``mu`` (P x D), their ``vc`` (P), the frame's ``z`` (D), its
mask ``observed`` (D) and ``il2`` (D) to every field ``GPMDM_PF.innovation`` returns.
np.longdouble arithmetic, math.fsum for the means.  Shared by tests/test_innov_ref.py (self-checks,
no GPU) and the GPU tests."""
import math
from typing import NamedTuple

import numpy as np

LD = np.longdouble
LN_2PI = LD(math.log(2.0 * math.pi))


class Ref(NamedTuple):
    mean: np.ndarray
    spread: np.ndarray
    gp_variance: np.ndarray
    variance: np.ndarray
    residual: np.ndarray
    zscore: np.ndarray
    log_density: np.ndarray
    n_valid: int
    elem: np.ndarray            # (P, D) longdouble: log N(z_j; mu_pj, vc_p il2_j), -inf on invalid rows


def lse_pair(a):
    """(M, s = sum exp(a - M)) of a 1-D longdouble array; the empty pair is (-inf, 0)."""
    a = np.asarray(a, dtype=LD)
    a = a[np.isfinite(a) | (a == np.inf)]
    if a.size == 0:
        return LD(-np.inf), LD(0)
    M = a.max()
    return M, np.exp(a - M).sum(dtype=LD)


def lse_merge(p, q):
    """(M, s) + (M', s') = (max, s exp(M - max) + s' exp(M' - max))."""
    (M, s), (Mb, sb) = p, q
    mx = max(M, Mb)
    if mx == -np.inf:
        return LD(-np.inf), LD(0)
    return mx, s * np.exp(M - mx) + sb * np.exp(Mb - mx)


def innovation(mu, vc, z, observed, il2) -> Ref:
    mu = np.asarray(mu, dtype=np.float64)
    vc = np.asarray(vc, dtype=np.float64).reshape(-1)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    il2 = np.asarray(il2, dtype=np.float64).reshape(-1)
    P, D = mu.shape
    obs = np.ones(D, dtype=bool) if observed is None else np.asarray(observed, dtype=bool).reshape(-1)
    nan = LD(np.nan)
    mean = np.array([LD(math.fsum(mu[:, j])) / P for j in range(D)], dtype=LD)
    dev = mu.astype(LD) - mean[None, :]
    spread = np.array([(dev[:, j] * dev[:, j]).sum(dtype=LD) / P for j in range(D)], dtype=LD)
    valid = vc > 0.0                               # (False for NaN)
    n_valid = int(valid.sum())
    il2l = il2.astype(LD)
    if n_valid:
        vbar = LD(math.fsum(vc[valid])) / n_valid
        gpv = il2l * vbar
    else:
        gpv = np.full(D, nan, dtype=LD)
    variance = spread + gpv
    zl = np.where(obs, z, 0.0).astype(LD)
    residual = np.where(obs, zl - mean, nan)
    zscore = residual / np.sqrt(variance)
    elem = np.full((P, D), LD(-np.inf), dtype=LD)
    if n_valid:
        var = vc[valid].astype(LD)[:, None] * il2l[None, :]
        t = zl[None, :] - mu[valid].astype(LD)
        elem[valid] = -(t * t) / (2 * var) - (np.log(var) + LN_2PI) / 2
    logd = np.full(D, nan, dtype=LD)
    if n_valid:
        for j in range(D):
            if obs[j]:
                M, s = lse_pair(elem[valid, j])
                logd[j] = M + np.log(s) - np.log(LD(n_valid))
    return Ref(mean, spread, gpv, variance, residual, zscore, logd, n_valid, elem)
