"""The MAP decoder's reference (tests/map_ref.py) checked on cases whose answer is known without
it: brute-force enumeration of every path, copies of a row, and fp64 against longdouble on
scripted clouds with synthetic moments (no GPU)."""
import itertools

import numpy as np

import map_ref as R
from backsmooth_ref import LD, log_f


def _moments(C, d, seed):
    """Smooth synthetic dynamics moments: mu_c(x) = A_c x + b_c, v_c(x) in [0.02, 0.06]."""
    rng = np.random.RandomState(seed)
    A = [0.9 * np.eye(d) + 0.05 * rng.randn(d, d) for _ in range(C)]
    b = [0.1 * rng.randn(d) for _ in range(C)]
    w = [rng.randn(d, d) for _ in range(C)]

    def f(X):
        X = np.asarray(X, dtype=np.float64)
        return ([X @ A[c].T + b[c] for c in range(C)],
                [0.02 + 0.04 * (0.5 + 0.5 * np.sin(X @ w[c].T)) ** 2 for c in range(C)])
    return f


def _history(P, n, C, d, seed, dup=False):
    """n + 1 exports, oldest first: scripted clouds that move as the synthetic dynamics do."""
    rng = np.random.RandomState(seed)
    hist = []
    X = 0.5 * rng.randn(P, d)
    for _ in range(n + 1):
        anc = rng.randint(0, P, P) if dup else np.arange(P)
        X = (0.9 * X + 0.15 * rng.randn(P, d))[anc]
        c = rng.randint(0, C, P)[anc]
        ll = (-5.0 * rng.rand(P))
        hist.append(dict(states=X.copy(), classes=c.copy(), ll=ll, resample_idx=anc))
    return hist


def test_the_recursion_equals_brute_force_enumeration():
    """P = 4, n = 3, C = 2, a zero in T and a -inf log-likelihood: every one of the 4^4 paths is
    scored on its own and the best one (lowest indices first) is the recursion's."""
    P, n, C, d = 4, 3, 2, 2
    mom = _moments(C, d, 1)
    hist = _history(P, n, C, d, 2)
    hist[2]["ll"][1] = -np.inf
    T = np.array([[0.7, 0.3], [0.0, 1.0]])
    got = R.map_path(hist, T, mom, n)
    lf = []
    for l in range(n):
        src, e = hist[-2 - l], hist[-1 - l]
        mu, var = mom(src["states"])
        lf.append(log_f(T, src["states"], src["classes"], e["states"], e["classes"], mu, var, LD))
    best, arg = LD(-np.inf), None
    for p in itertools.product(range(P), repeat=n + 1):        # lexicographic: ties keep the lowest p_0, p_1, ...
        s = LD(0)
        for l in range(n):
            s = s + lf[l][p[l + 1], p[l]] + LD(R.slot_ll(hist[-1 - l])[p[l]])
        if s > best:
            best, arg = s, p
    assert np.isfinite(float(best))
    assert abs(float(got["log_joint"] - best)) <= 1e-15 * abs(float(best))
    assert tuple(got["path"]) == arg
    assert abs(float(R.path_score(hist, T, mom, got["path"]) - best)) <= 1e-15 * abs(float(best))
    # the particle without a likelihood (export 2 of 4 is lag 1) is cut off, and the path avoids it
    assert got["delta"][1][1] == -np.inf and got["psi"][1][1] == -1 and got["path"][1] != 1
    # T[1, 0] = 0: no step of the path goes from class 1 to class 0
    cls = [int(hist[-1 - l]["classes"][got["path"][l]]) for l in range(n + 1)]
    assert all(not (cls[l + 1] == 1 and cls[l] == 0) for l in range(n)), cls


def test_nobody_reaches_a_cut_off_class():
    P, C, d = 6, 2, 2
    mom = _moments(C, d, 3)
    hist = _history(P, 1, C, d, 4)
    hist[0]["classes"][:] = 1
    hist[1]["classes"][:3] = 0
    hist[1]["classes"][3:] = 1
    T = np.array([[0.5, 0.5], [0.0, 1.0]])
    got = R.map_path(hist, T, mom, 1)
    assert np.all(got["psi"][0][:3] == -1) and np.all(got["delta"][0][:3].astype(np.float64) == -np.inf)
    assert np.all(got["psi"][0][3:] >= 0) and got["path"][0] >= 3


def test_copies_return_the_lowest_index():
    P, C, d = 40, 2, 3
    mom = _moments(C, d, 5)
    hist = _history(P, 2, C, d, 6, dup=True)
    T = np.array([[0.8, 0.2], [0.3, 0.7]])
    got = R.map_path(hist, T, mom, 2)
    for l in range(2):
        src = hist[-2 - l]
        key = [tuple(r) + (int(c),) for r, c in zip(src["states"], src["classes"])]
        first = {}
        for i, k in enumerate(key):
            first.setdefault(k, i)
        for j, k in enumerate(got["psi"][l]):
            assert k == first[key[k]], (l, j, k)
        # copies of a target carry the same delta and psi
        e = hist[-1 - l]
        for j in range(P):
            a = int(e["resample_idx"][j])
            twin = int(np.nonzero(e["resample_idx"] == a)[0][0])
            assert got["delta"][l][j] == got["delta"][l][twin] and got["psi"][l][j] == got["psi"][l][twin]


def test_fp64_and_longdouble_agree_on_scripted_clouds():
    """C = 3, d = 3, 400 x 400, 8 steps: the gaps dwarf the band, so both formats pick the same
    back-pointers, and their scores agree to fp64 rounding."""
    P, n, C, d = 400, 8, 3, 3
    mom = _moments(C, d, 7)
    hist = _history(P, n, C, d, 8)
    T = np.array([[0.8, 0.1, 0.1], [0.2, 0.7, 0.1], [0.1, 0.3, 0.6]])
    a, b = R.map_path(hist, T, mom, n), R.map_path(hist, T, mom, n, np.float64)
    gap = min(float(g.min()) for g in a["gap"])
    err = max(float(np.abs(x.astype(LD) - y).max()) for x, y in zip(b["delta"], a["delta"]))
    print(f"minimum gap {gap:.3g}, fp64 - longdouble {err:.3g}, band {a['B'][0]:.3g}")
    assert gap > 2 * a["B"][0]
    assert err <= a["B"][0]
    for x, y in zip(a["psi"], b["psi"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["path"], b["path"])
