"""Extended-precision restatement of the gate (INTEGRATION.md "Gating"): the decision rule from
the frame's z-scores, and the log-likelihood of the kept joints from the particles'
observation-GP means ``mu`` (P x D), their ``vc`` (P), the frame's ``z`` (D), the kept joints
``used`` (D) and ``il2`` (D).  np.longdouble arithmetic; the constant is formed through
np.float32 as the reference forms it (gpmdm_pf.py:5, 191).  Shared by tests/test_gate_ref.py
(self-checks, no GPU) and the GPU tests."""
import math

import numpy as np

LD = np.longdouble
LOG_2PI_F32 = np.float32(1.8378770351409912)


def cap_of(limit, d_obs) -> int:
    return int(math.floor(float(limit) * float(d_obs)))


def decide(zscore, observed, k, limit):
    """(exceeded, gated, used, overflow): exceeded_j = observed_j and |zscore_j| > k (false for
    NaN); gated = exceeded when 1 <= n_exceeded <= floor(limit D_obs), else empty, with overflow
    when n_exceeded is above the cap; used = observed and not gated."""
    zs = np.asarray(zscore, dtype=np.float64).reshape(-1)
    obs = np.ones(zs.shape[0], dtype=bool) if observed is None else np.asarray(observed, dtype=bool).reshape(-1)
    with np.errstate(invalid="ignore"):
        exceeded = obs & (np.abs(zs) > float(k))
    n, cap = int(exceeded.sum()), cap_of(limit, int(obs.sum()))
    overflow = n > cap
    gated = exceeded.copy() if 1 <= n <= cap else np.zeros_like(exceeded)
    return exceeded, gated, obs & ~gated, overflow


def reweigh(mu, vc, z, used, il2):
    """ll'_p = -1/2 S'_p / vc_p - D' log vc_p - sum_{used} log il2_j - (double)(float32(D'/2) float32 ln 2 pi),
    S'_p = sum_{used} (z_j - mu_pj)^2 / il2_j; NaN where vc_p <= 0; exactly 0 when nothing is used."""
    mu = np.asarray(mu, dtype=np.float64)
    vc = np.asarray(vc, dtype=np.float64).reshape(-1)
    used = np.asarray(used, dtype=bool).reshape(-1)
    P = mu.shape[0]
    Dp = int(used.sum())
    if Dp == 0:
        return np.zeros(P, dtype=LD)
    il2l = np.asarray(il2, dtype=np.float64).reshape(-1)[used].astype(LD)
    t = np.asarray(z, dtype=np.float64).reshape(-1)[used].astype(LD)[None, :] - mu[:, used].astype(LD)
    S = (t * t / il2l[None, :]).sum(axis=1, dtype=LD)
    const = LD(float(np.float32(np.float32(0.5 * Dp) * LOG_2PI_F32)))
    vcl = vc.astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        ll = -S / (2 * vcl) - Dp * np.log(vcl) - np.log(il2l).sum(dtype=LD) - const
    ll[~(vc > 0)] = LD(np.nan)
    return ll
