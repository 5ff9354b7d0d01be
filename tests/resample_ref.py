"""Extended-precision restatement of the filter's normalise / CDF / resample / read-out chain
(gpmdm_pf.py:194-262), and the scripted inputs of tests/test_gpu_resample_edges.py.

Everything here is numpy on the host: ``np.longdouble`` (64-bit mantissa on x86) for the
reference values, fp64 only where the device's own fp64 expression is restated bit for bit
(``sys_u``, ``exact_cdf``).  tests/test_resample_ref.py checks this module against the fp64
oracle and checks the premises the GPU tests rest on (exact patterns really are exact in any
summation order; the band check passes on the oracle's own indices).

The scripted inputs:

* exact patterns (``exact_patterns``): ll in {c, -inf}, so e in {0, 1}, every partial sum of
  e is an integer below 2^53 whatever the association, and the CDF at particle i is the one
  correctly rounded division k_i / S.  The expected ancestors are np.searchsorted(cum, u,
  "left") with no slack.
* banded patterns (``banded_ll``): general weights.  An ancestor i of uniform u is accepted
  iff C[i-1] - tol <= u <= C[i] + tol with tol = (P + 8) 2^-53 (``band_tol``): any order of
  summing P non-negative terms moves a partial sum by at most (P - 1) 2^-53 relative to the
  total, plus exp, the subtraction of the maximum, the offset addition and the division.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
U_MAX = 1.0 - 2.0 ** -53            # the largest fp64 below 1
TINY = 2.0 ** -1074                 # the smallest positive fp64
SUBNORMAL_FLOOR = 2.0 * TINY        # an fp64 e and its quotient each round to a subnormal grid

EXACT_C = (0.0, -1234.5, 700.0)
SYS_U0 = (0.0, 2.0 ** -60, 0.5, U_MAX)
SMALL_P = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
MULTI_P = (1025, 1280, 2047, 2048, 2049, 4097)
GUIDE_P = (262143, 262144, 300001)
BANDED_P = (1000, 5000, 300001)
BLOCK = 256                         # k_norm_exp_scan / cdf_view block
ROWS_BLOCK = 2048                   # k_rows_ll block


def band_tol(P: int) -> float:
    return (P + 8) * EPS


# ---- the reference chain ---------------------------------------------------------------------
class Normalised:
    """M, log_w, e, total, w and the CDF of one ll vector, all np.longdouble."""

    def __init__(self, ll):
        ll = np.asarray(ll, dtype=np.float64)
        finite_or_inf = ll[~np.isnan(ll)]
        self.ll = ll.astype(LD)
        self.M = LD(np.max(finite_or_inf))                   # NaN ignored (fmax)
        with np.errstate(invalid="ignore"):
            self.log_w = self.ll - self.M
            self.e = np.exp(self.log_w)
        self.total = np.sum(self.e, dtype=LD)
        self.w = self.e / self.total
        cdf = np.cumsum(self.e, dtype=LD) / self.total
        cdf[-1] = LD(1.0)                                    # the last bucket forced to 1
        self.cdf = cdf


def multinomial_indices(cdf, u):
    """First index with cdf >= u (torch's search), on the extended-precision CDF."""
    return np.searchsorted(cdf, np.asarray(u, dtype=np.float64).astype(LD), side="left").astype(np.int64)


def sys_u(s, u0, P):
    """Slot s's uniform in fp64, exactly as the device forms it: (float(s) + u0) / float(P)."""
    return (np.asarray(s, dtype=np.float64) + np.float64(u0)) / np.float64(P)


def systematic_indices(cdf, u0):
    P = cdf.shape[0]
    return multinomial_indices(cdf, sys_u(np.arange(P), u0, P))


def readouts(ll, classes_pre, states_pre, idx, C):
    """Posterior, state mean and the (not-a-log) likelihood read-out for ancestors ``idx``:
    the post-resample class / state at slot s weighted by the pre-resample ll / w at slot s,
    as oracle.class_probabilities, current_state_mean and log_likelihood_readout do.  Also
    returns sum_s |x_idx[s]| w[s], the scale of the state mean's rounding bound."""
    n = Normalised(ll)
    cls = np.asarray(classes_pre)[idx]
    X = np.asarray(states_pre, dtype=np.float64)[idx].astype(LD)
    with np.errstate(invalid="ignore"):
        lw = n.ll + n.log_w
        lw = lw - np.max(lw[~np.isnan(lw)])
        e2 = np.exp(lw)
    cl = np.array([np.sum(e2[cls == c], dtype=LD) for c in range(C)], dtype=LD)
    post = cl / np.sum(cl, dtype=LD)
    mean = np.sum(X * n.w[:, None], axis=0, dtype=LD)
    scale = np.sum(np.abs(X) * n.w[:, None], axis=0, dtype=LD)
    return post, mean, np.sum(e2, dtype=LD), scale


def device_association_cdf(e):
    """The fp64 CDF of weights ``e`` summed in the device's association (k_norm_exp_scan's
    64-lane Hillis-Steele scans and sequential wave bases, k_norm_total's chunked 1024-wide
    Hillis-Steele scan of the block sums, CdfView's (offset + local) / S with the last bucket
    forced to 1).  A host model of the summation order only -- ``e`` is the caller's, not the
    device's exp -- used to see what that order does to monotonicity."""
    e = np.asarray(e, dtype=np.float64)
    P = e.shape[0]
    nb = -(-P // BLOCK)
    x = np.zeros(nb * BLOCK)
    x[:P] = e
    x = x.reshape(nb, BLOCK // 64, 64)
    off = 1
    while off < 64:
        y = x.copy()
        x[..., off:] = y[..., off:] + y[..., :-off]
        off *= 2
    wsum = x[..., 63].copy()
    base = np.zeros(nb)
    for w in range(1, BLOCK // 64):
        base = base + wsum[:, w - 1]
        x[:, w, :] += base[:, None]
    local = x.reshape(-1)[:P]
    blocksum = x[:, -1, 63].copy()
    chunk = -(-nb // 1024)
    bs = np.zeros(1024 * chunk)
    bs[:nb] = blocksum
    bs = bs.reshape(1024, chunk)
    part = np.zeros(1024)
    for i in range(chunk):
        part = part + bs[:, i]
    off = 1
    while off < 1024:
        y = part.copy()
        part[off:] = y[off:] + y[:-off]
        off *= 2
    run = np.concatenate([[0.0], part[:-1]])
    boff = np.zeros((1024, chunk))
    for i in range(chunk):
        boff[:, i] = run
        run = run + bs[:, i]
    boff = boff.reshape(-1)[:nb]
    cdf = (boff[np.arange(P) // BLOCK] + local) / part[1023]
    cdf[-1] = 1.0
    return cdf


def binary_search(cdf, u):
    """k_resample's unguided search, step for step (first index with cdf >= u on a monotone
    cdf; defined here for a non-monotone one too, where np.searchsorted is not)."""
    u = np.asarray(u, dtype=np.float64)
    P = cdf.shape[0]
    lo = np.zeros(u.shape[0], dtype=np.int64)
    hi = np.full(u.shape[0], P, dtype=np.int64)
    while np.any(hi > lo):
        act = hi > lo
        mid = lo + (hi - lo) // 2
        less = cdf[np.minimum(mid, P - 1)] < u
        lo = np.where(act & less, mid + 1, lo)
        hi = np.where(act & ~less, mid, hi)
    return lo


def near_tie_uniforms(cdf, P, rng):
    """One frame of P uniforms that sit on the CDF: the fp64 roundings of the reference CDF at
    every 256-block's first, last and two middle particles (where the device's block offset and
    its local scan meet in two associations of one sum) and at up to P/8 other particles, each
    with its two fp64 neighbours, plus edge_uniforms' 0, 2^-1074 and 1 - 2^-53."""
    c64 = np.asarray(cdf, dtype=np.float64)
    ends = c64[np.isin(np.arange(P) % BLOCK, (0, BLOCK // 2 - 1, BLOCK // 2, BLOCK - 1))]
    other = rng.choice(c64, min(P // 8, 20000), replace=False)
    near = np.unique(np.concatenate([ends, other]))
    frames = edge_uniforms(near, P, rng, max_values=near.shape[0])
    assert len(frames) == 1
    return frames[0]


# ---- checks ----------------------------------------------------------------------------------
def band_excess(cdf, u, idx):
    """How far outside [C[i-1], C[i]] each uniform lies for its ancestor (0 inside)."""
    u = np.asarray(u, dtype=np.float64).astype(LD)
    idx = np.asarray(idx, dtype=np.int64)
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], LD(0.0))
    hi = cdf[idx]
    return np.maximum(np.maximum(lo - u, u - hi), LD(0.0))


def offspring_excess(w, idx):
    """The slack x each particle's offspring count needs for floor(P w - x) <= n <= ceil(P w + x)."""
    P = w.shape[0]
    n = np.bincount(idx, minlength=P).astype(LD)
    Pw = LD(P) * w
    return np.maximum(np.maximum(Pw - 1 - n, n - 1 - Pw), LD(0.0))


def rel_excess(got, ref):
    """|got - ref| beyond the subnormal grid, relative to |ref| (0 where both vanish)."""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    ref = np.asarray(ref, dtype=LD)
    err = np.maximum(np.abs(got - ref) - LD(SUBNORMAL_FLOOR), LD(0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, LD(0.0), err / np.abs(ref))
    return r


# ---- exact patterns ---------------------------------------------------------------------------
def exact_patterns(P: int, large: bool = False):
    """(name, mask) pairs; mask[i]: particle i has ll = c (else -inf).  Patterns that would be
    empty at this P are left out.  ``large``: the four patterns run at the guide-table sizes."""
    i = np.arange(P)
    out = [("all_ones", np.ones(P, dtype=bool)),
           ("block_first", i % BLOCK == 0)]
    if P > 300:
        out += [("first_300_zero", i >= 300), ("last_300_zero", i < P - 300)]
    if large:
        return out
    for j in sorted({0, 63, 64, 255, 256, P // 2, P - 2, P - 1}):
        if 0 <= j < P:
            out.append((f"single_{j}", i == j))
    if P >= BLOCK:
        out.append(("block_last", i % BLOCK == BLOCK - 1))
    out.append(("alternate_blocks", (i // BLOCK) % 2 == 0))
    if P >= ROWS_BLOCK:
        out.append(("rows_block_last", i % ROWS_BLOCK == ROWS_BLOCK - 1))
    return out


def exact_ll(mask, c):
    return np.where(mask, np.float64(c), -np.inf)


def exact_cdf(mask):
    """fp64 CDF of an exact pattern: cum_i = fl(k_i / S), the last bucket forced to 1."""
    k = np.cumsum(mask.astype(np.int64))
    cum = k.astype(np.float64) / np.float64(k[-1])
    cum[-1] = 1.0
    return cum


def edge_uniforms(cum, P, rng, max_values=300):
    """Frames of P multinomial uniforms holding 0, 2^-1074, 1 - 2^-53 and, for up to
    ``max_values`` distinct CDF values v, v itself and its two fp64 neighbours (clipped to
    [0, 1)); random fill; shuffled so that wave neighbours differ wildly.  One frame when the
    specials fit into P slots, else as many as they need."""
    vals = np.unique(cum)
    if vals.shape[0] > max_values:
        vals = np.sort(rng.choice(vals, max_values, replace=False))
    sp = np.concatenate([[0.0, TINY, U_MAX], vals, np.nextafter(vals, 0.0), np.nextafter(vals, 1.0)])
    sp = np.clip(sp, 0.0, U_MAX)
    frames = []
    for k in range(0, sp.shape[0], P):
        u = np.concatenate([sp[k:k + P], rng.rand(max(0, P - sp[k:k + P].shape[0]))])
        rng.shuffle(u)
        frames.append(u)
    return frames


def scripted_particles(P, C, d, rng):
    """Distinct finite states in (-1, 1] and classes in 0..C-1 for the scripted rows: a wrong
    gather shows in either."""
    i = np.arange(P, dtype=np.float64)
    X = np.empty((P, d))
    for j in range(d):
        X[:, j] = (1.0 if j % 2 == 0 else -1.0) * (i + 1.0 + j) / (P + d + 1.0)
    cls = rng.randint(0, C, P).astype(np.int64)
    return X, cls


# ---- banded patterns ----------------------------------------------------------------------------
BANDED = ("linspace_900", "sparse_1e4", "geometric_blocks", "randn5", "randn5_block_holes")


def banded_ll(name, P, rng):
    i = np.arange(P)
    if name == "linspace_900":          # subnormal and flushed e
        ll = np.linspace(-900.0, 0.0, P)
        rng.shuffle(ll)
        return ll
    if name == "sparse_1e4":
        ll = -1e4 * rng.rand(P)
        ll[rng.randint(P)] = 0.0
        return ll
    if name == "geometric_blocks":
        return -0.7 * (i // BLOCK).astype(np.float64)
    if name == "randn5":
        return 5.0 * rng.randn(P)
    if name == "randn5_block_holes":    # -inf on the leading halves of the odd blocks
        ll = 5.0 * rng.randn(P)
        ll[((i // BLOCK) % 2 == 1) & (i % BLOCK < BLOCK // 2)] = -np.inf
        return ll
    raise KeyError(name)
