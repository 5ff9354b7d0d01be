"""Numpy restatement of the fixed-lag smoother's definitions (include/gpmdm_hip.h,
gpmdm_pf_smoothed), for the tests.

``history`` is a list of per-frame ``export_state()`` dicts (``states``, ``classes``,
``resample_idx``), oldest first; its last entry is frame t, its first the root, whose
``resample_idx`` is not read.  Slot p of frame f took the propagated particle
``resample_idx_f[p]``, which came from particle ``resample_idx_f[p]`` of frame f - 1's cloud:

    j_0(p) = p,   j_{l+1}(p) = resample_idx_{t-l}[j_l(p)]

and the lag-l row is read off the traced cloud {states_{t-l}[j_l(p)]}, every current particle
weighing 1/P.  Means are taken with ``math.fsum`` (the correctly rounded sum), divided once.
"""
import math

import numpy as np


def trace(history, lag_last):
    """The ancestors j_l(p), l = 0..lag_last: (lag_last + 1, P) int64."""
    P = len(history[-1]["classes"])
    if not 0 <= lag_last <= len(history) - 1:
        raise ValueError(f"lag {lag_last} is above the depth {len(history) - 1}")
    j = np.arange(P, dtype=np.int64)
    rows = [j]
    for l in range(lag_last):
        j = np.asarray(history[-1 - l]["resample_idx"], dtype=np.int64)[j]
        rows.append(j)
    return np.stack(rows)


def smoothed(history, lag_first=0, lag_last=None):
    """Rows lag_first..lag_last (default: the whole depth) of every field."""
    if lag_last is None:
        lag_last = len(history) - 1
    if not 0 <= lag_first <= lag_last:
        raise ValueError("lags: 0 <= lag_first <= lag_last")
    anc = trace(history, lag_last)[lag_first:]
    C = 1 + max(int(np.max(h["classes"])) for h in history)
    out = dict(lags=np.arange(lag_first, lag_last + 1), ancestors=anc, states=[], classes=[],
               class_counts=[], state_mean=[], distinct_ancestors=[])
    for l, j in zip(out["lags"], anc):
        fr = history[-1 - l]
        x = np.asarray(fr["states"], dtype=np.float64)[j]
        c = np.asarray(fr["classes"], dtype=np.int64)[j]
        P = len(j)
        out["states"].append(x)
        out["classes"].append(c)
        out["class_counts"].append(np.bincount(c, minlength=C))
        out["state_mean"].append(np.array([math.fsum(x[:, k]) / P for k in range(x.shape[1])]))
        out["distinct_ancestors"].append(len(np.unique(j)))
    for k in ("states", "classes", "class_counts", "state_mean", "distinct_ancestors"):
        out[k] = np.asarray(out[k])
    return out


def class_probabilities(ref, C):
    """count / P in fp64, one division, padded to C classes."""
    cnt = ref["class_counts"]
    P = ref["ancestors"].shape[1]
    full = np.zeros((cnt.shape[0], C), dtype=np.int64)
    full[:, :cnt.shape[1]] = cnt
    return full.astype(np.float64) / np.float64(P)
