"""Host model of the cutoff kernel's K-step lists, and the scripted models that drive them
(tests only; a plain module, no conftest).

The first half restates in plain numpy, in scaled coordinates X / l_y, what decides which K-steps a
particle tile of the cutoff kernel (gpmdm_amd/csrc/obs_cutoff.h) runs:

* ``spatial_order`` and ``kstep_spheres`` of host_image.h (the image's row order and one
  bounding sphere per 16-row K-step);
* the kernel's tile test: centre = mean of the tile's PT particle slots (a ragged tile's empty
  slots hold copies of its first particle, as the kernel's clamp loads them), radius = the
  largest distance to it, padded ``r (1 + 1e-12) + 1e-12``;
* the activity rule: K-step k is inactive iff ``gap > 0 and gap^2 > cut2`` with
  ``gap = |c_tile - c_k| - r_tile - r_k`` and ``cut2 = -ln tau (1 + 1e-12) + 1e-6``
  (capi_model.hip);
* ``cutoff_chunk_begin``, ``cutoff_chunk_positions`` and ``cutoff_split_chunk`` of common.h.

The device forms the tile's sphere in units of 2 x 64 / ln 2 and with fma; this restatement does
not, so the two differ by roundings of 1e-15 scaled units.  Every use therefore also reports the
decisiveness margin min_k | gap_k - sqrt(cut2) |, and the tests require it to be >= 1e-3 scaled
units: nine decades above the device's own 1e-12 paddings.

The second half builds the scripted models (parameter dicts with the names of
extended_ref.recipe_model, so ExtendedModel and oracle_of apply unchanged) and the particle
targets that give each tile a chosen list.

Chain model: T clusters of 16 training latents (the last one 11: N = 16 T - 5, a ragged last
K-step and a ragged last R tile), centres on axis 0.  Cluster 0 stands alone, 40 scaled units
below the others; clusters 1 .. T - 1 are 3.2 scaled units apart; points are centre +
0.12 randn / sqrt(d); training rows are shuffled.  The bisection of ``spatial_order`` then makes
K-step k exactly cluster k.  With sqrt(cut2) between 7.3 and 8.3, a tile whose particles sit
symmetrically on clusters a..b of the chain reaches a - 2 .. b + 2, clipped to 1 .. T - 1: two
neighbours are 6.4 - radii away, the third 9.6 - radii.
"""
from __future__ import annotations

import numpy as np

KBK = 16                         # rows per K-step (common.h kBK)
TPC = 32                         # list entries per chunk (4 waves x 8 tiles, 8 x 4)
SPACING = 3.2
JITTER = 0.12
ISOLATED = 40.0                  # cluster 0's distance from the chain, and the far tile's
MIN_MARGIN = 1e-3


def tile_particles(d):
    """PT of the cutoff kernel at latent dimension d (obs_cutoff.h launch_cut_d)."""
    return 32 if d <= 8 else 64


# ----------------------------------------------------------------------------
# host_image.h
# ----------------------------------------------------------------------------

def spatial_order(X, ls):
    """host_image.h spatial_order: recursive bisection of X / ls along the widest coordinate
    (the first of equal spreads), sorted by (value, training row), the left part a whole number
    of 16-row leaves, ceil(leaves / 2) of them.  Returns perm (image row -> training row)."""
    Xs = np.asarray(X, dtype=np.float64) / np.asarray(ls, dtype=np.float64)[None, :]

    def rec(idx):
        n = idx.size
        if n <= KBK:
            return idx
        v = Xs[idx]
        best = int(np.argmax(v.max(axis=0) - v.min(axis=0)))
        idx = idx[np.lexsort((idx, v[:, best]))]
        leaves = -(-n // KBK)
        left = ((leaves + 1) // 2) * KBK
        return np.concatenate([rec(idx[:left]), rec(idx[left:])])

    return rec(np.arange(Xs.shape[0], dtype=np.int64))


def kstep_spheres(X, ls, perm):
    """host_image.h kstep_spheres: per K-step the centre (the mean of its rows, summed in row
    order) and the radius sqrt(max |row - centre|^2) (1 + 1e-12) + 1e-12.  (T_R, d + 1)."""
    Xs = (np.asarray(X, dtype=np.float64) / np.asarray(ls, dtype=np.float64)[None, :])[perm]
    n, d = Xs.shape
    nks = -(-n // KBK)
    out = np.zeros((nks, d + 1))
    for k in range(nks):
        rows = Xs[k * KBK:(k + 1) * KBK]
        c = np.cumsum(rows, axis=0)[-1] / float(rows.shape[0])       # sequential, as the header
        s = np.zeros(rows.shape[0])
        for j in range(d):
            t = rows[:, j] - c[j]
            s = s + t * t
        out[k, :d] = c
        out[k, d] = np.sqrt(s.max()) * (1.0 + 1e-12) + 1e-12
    return out


def cut2_of(tau):
    """capi_model.hip: the squared cutoff distance with its rounding margin."""
    return -np.log(tau) * (1.0 + 1e-12) + 1e-6


def tau_of(Ky_inv, Y, sigma2):
    """host_image.h obs_cutoff_tau restated: min(tau_q, tau_mu) from M = K_y^-1 Y."""
    N = Y.shape[0]
    vc_min = sigma2 / (N + sigma2)
    h = 0.5 * (np.nextafter(vc_min, 1.0) - vc_min)
    tau = np.sqrt(sigma2) * h / (2.001 * np.sqrt(float(N)))
    M = Ky_inv @ Y
    for j in range(Y.shape[1]):
        m1 = float(np.sum(np.abs(M[:, j])))
        y = float(np.max(np.abs(Y[:, j])))
        if m1 > 0.0 and y > 0.0:
            tau = min(tau, 0.5 * (np.nextafter(y, 1e308) - y) / m1)
    return float(tau)


# ----------------------------------------------------------------------------
# common.h
# ----------------------------------------------------------------------------

def chunk_begin(c, nt, tpc=TPC):
    if c <= 0:
        return 0
    nc = -(-nt // tpc)
    return nt - (nc - c) * tpc


def chunk_positions(c, n_act, T_M, tpc=TPC):
    last = chunk_begin(c + 1, n_act + T_M, tpc) - 1
    return last + 1 if last < n_act else n_act


def split_chunk(n_act, T_M, tpc=TPC):
    nc = -(-(n_act + T_M) // tpc)
    if nc < 2:
        return nc
    fill = 4
    tot = sum(chunk_positions(c, n_act, T_M, tpc) + fill for c in range(nc))
    pre, best_v, best = 0, tot, 1
    for c in range(1, nc):
        pre += chunk_positions(c - 1, n_act, T_M, tpc) + fill
        v = max(pre, tot - pre)
        if v < best_v:
            best_v, best = v, c
    return best


# ----------------------------------------------------------------------------
# the lists
# ----------------------------------------------------------------------------

class TileList:
    """One particle tile's list: ``active`` (ascending K-steps), ``n_act``, ``bounds`` (chunk c
    is list entries bounds[c] .. bounds[c + 1]), ``c_star`` (cutoff_split_chunk) and ``margin``
    (min over every K-step of | gap - sqrt(cut2) |)."""

    def __init__(self, active, T_M, margin):
        self.active = active
        self.n_act = int(active.size)
        self.T_M = T_M
        nt = self.n_act + T_M
        self.n_tiles = nt
        self.n_chunks = -(-nt // TPC)
        self.bounds = [chunk_begin(c, nt) for c in range(self.n_chunks + 1)]
        self.c_star = split_chunk(self.n_act, T_M)
        self.margin = float(margin)

    @property
    def gaps(self):
        """Index gaps of the list: places where it skips K-steps."""
        return int(np.sum(np.diff(self.active) > 1))

    @property
    def finish_from(self):
        """First list entry the likelihood finish chains on for a split tile (obs_ll_value)."""
        return chunk_begin(self.c_star, self.n_tiles)


class ListModel:
    """The image's geometry for one model: ``perm``, ``spheres`` and the cutoff distance."""

    def __init__(self, X, ls, tau, D):
        self.X, self.ls = np.asarray(X, dtype=np.float64), np.asarray(ls, dtype=np.float64)
        self.d = self.X.shape[1]
        self.perm = spatial_order(self.X, self.ls)
        self.spheres = kstep_spheres(self.X, self.ls, self.perm)
        self.T_R = self.spheres.shape[0]
        self.T_M = -(-D // 16)
        self.PT = tile_particles(self.d)
        self.set_tau(tau)

    def set_tau(self, tau):
        self.tau = float(tau)
        self.cut2 = cut2_of(self.tau)
        self.reach = float(np.sqrt(self.cut2))

    def tile(self, states):
        """The list of one tile holding ``states`` (1 .. PT rows, particle order)."""
        xs = np.asarray(states, dtype=np.float64) / self.ls[None, :]
        if xs.shape[0] < self.PT:                                     # the kernel's clamp
            xs = np.concatenate([xs, np.repeat(xs[:1], self.PT - xs.shape[0], axis=0)])
        assert xs.shape[0] == self.PT
        c = np.cumsum(xs, axis=0)[-1] * (1.0 / self.PT)
        r = np.sqrt(np.max(np.sum((xs - c[None, :]) ** 2, axis=1))) * (1.0 + 1e-12) + 1e-12
        dist = np.sqrt(np.sum((c[None, :] - self.spheres[:, :self.d]) ** 2, axis=1))
        gap = dist - r - self.spheres[:, self.d]
        inactive = (gap > 0.0) & (gap * gap > self.cut2)
        return TileList(np.nonzero(~inactive)[0], self.T_M, np.min(np.abs(gap - self.reach)))

    def tiles(self, states, begin=0, end=None):
        """The lists of the consecutive PT-particle tiles of states[begin:end]."""
        end = states.shape[0] if end is None else end
        return [self.tile(states[o:min(o + self.PT, end)]) for o in range(begin, end, self.PT)]

    def stats(self, lists):
        """(run, dense) as the kernel counts them (obs_cutoff.h): per chunk and wave
        sum_tiles kend x MT -- an R tile at list position i multiplies i + 1 positions, a mean
        tile n_act --, and per tile the dense kernel's T_R (T_R + 1) / 2 + T_M T_R, x MT."""
        MT = self.PT // 16
        run = MT * sum(t.n_act * (t.n_act + 1) // 2 + self.T_M * t.n_act for t in lists)
        dense = MT * len(lists) * (self.T_R * (self.T_R + 1) // 2 + self.T_M * self.T_R)
        return run, dense


# ----------------------------------------------------------------------------
# scripted models
# ----------------------------------------------------------------------------

def _params(Xs, d, D, rng):
    """The parameter dict around scaled latents ``Xs`` (rows already in training order): length
    scales uniform(1, 2), sigma_y = 0.15, sigma_x = 0.12, lambdas as the recipe, Y a smooth
    function of the latents plus noise, one class with one sequence (C = 1)."""
    N = Xs.shape[0]
    ls = rng.uniform(1.0, 2.0, d)
    p = dict(
        y_log_lengthscales=np.log(ls), y_log_lambdas=np.log(rng.uniform(0.5, 2, D)),
        y_log_sigma_n=float(np.log(0.15)), x_log_lengthscales=np.log(rng.uniform(1.0, 2.0, d)),
        x_log_lambdas=np.log(rng.uniform(0.5, 2, d)), x_log_sigma_n=float(np.log(0.12)),
        x_log_lin_coeff=np.log(rng.uniform(0.02, 0.08, d + 1)))
    W = rng.randn(d, D)
    Y = np.sin(Xs @ W + rng.uniform(0, 6, D)) + 0.05 * rng.randn(N, D)
    p.update(X=np.ascontiguousarray(Xs * np.exp(p["y_log_lengthscales"])[None, :]), Y=Y, seq_lengths=[[N]])
    return p


class Scripted:
    """A scripted model: ``p`` (the parameter dict), ``centres`` (scaled cluster centres, in the
    order the tests name the clusters), ``members`` (training rows of each cluster), ``ls``."""

    def __init__(self, p, centres, members, kind):
        self.p, self.centres, self.members, self.kind = p, centres, members, kind
        self.ls = np.exp(p["y_log_lengthscales"])
        self.d, self.D = p["X"].shape[1], p["Y"].shape[1]
        self.N = p["X"].shape[0]
        self.T = centres.shape[0]

    def list_model(self, tau):
        return ListModel(self.p["X"], self.ls, tau, self.D)

    def host_tau(self):
        """tau from the fp64 oracle's K_y^-1 (the device's differs in the ninth digit: beta comes
        from another factorisation; the cutoff distance moves by 1e-10)."""
        from oracle import gpmdm_oracle as O
        p = self.p
        Ky = O.rbf_kernel(p["X"], p["X"], p["y_log_lengthscales"], p["y_log_sigma_n"], 0.0, noise=True)
        return tau_of(np.linalg.inv(Ky), p["Y"], float(np.exp(p["y_log_sigma_n"])) ** 2)


def _clusters(centres, sizes, d, rng):
    pts, members, o = [], [], 0
    for c, n in zip(centres, sizes):
        pts.append(c[None, :] + JITTER * rng.randn(n, d) / np.sqrt(d))
        members.append(np.arange(o, o + n))
        o += n
    return np.concatenate(pts), members


def _shuffled(Xs, members, rng):
    """Training rows in shuffled order; ``members`` follow."""
    order = rng.permutation(Xs.shape[0])                # new row r holds old row order[r]
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    return Xs[order], [np.sort(inv[m]) for m in members]


def chain_model(T, d, D, seed=None):
    rng = np.random.RandomState(7000 + 100 * T + 10 * d + D if seed is None else seed)
    centres = np.zeros((T, d))
    centres[1:, 0] = SPACING * np.arange(T - 1)
    centres[0, 0] = -ISOLATED
    centres[:, 0] -= 0.5 * SPACING * (T - 2)            # the chain centred on the origin
    Xs, members = _clusters(centres, [KBK] * (T - 1) + [11], d, rng)
    Xs, members = _shuffled(Xs, members, rng)
    return Scripted(_params(Xs, d, D, rng), centres, members, "chain")


def grid_model(D=7, seed=9100):
    """d = 2, clusters on a 9 x 8 grid with the chain's spacing (cluster g = 8 i + j at
    (3.2 i, 3.2 j)), the last cluster 11 rows."""
    rng = np.random.RandomState(seed)
    ii, jj = np.meshgrid(np.arange(9), np.arange(8), indexing="ij")
    centres = SPACING * np.stack([ii.ravel() - 4.0, jj.ravel() - 3.5], axis=1)
    Xs, members = _clusters(centres, [KBK] * 71 + [11], 2, rng)
    Xs, members = _shuffled(Xs, members, rng)
    return Scripted(_params(Xs, 2, D, rng), centres, members, "grid")


def far_point(sm):
    """A scaled point further than 30 from every training latent (on axis 0: d = 1 has no other)."""
    c = np.zeros(sm.d)
    c[0] = sm.centres[:, 0].max() + ISOLATED
    return c


# ----------------------------------------------------------------------------
# targets
# ----------------------------------------------------------------------------

def span_for(n_act, T, shift=0):
    """Clusters (a, b) of the chain model whose symmetric tile lists ``n_act`` K-steps, or
    "far" for 0.  1: the isolated cluster alone; 3: the chain's first cluster; 5 and up: a - 2 ..
    b + 2 inside the chain (``shift`` moves the window), clipped at its ends from T - 4 on; T:
    the isolated cluster and the chain's end in one tile."""
    if n_act == 0:
        return "far"
    if n_act == 1:
        return 0, 0
    if n_act == 3:
        return (1, 1) if shift % 2 == 0 else (T - 1, T - 1)
    if n_act == 4:
        return 2, 2
    if n_act == T:
        return 0, T - 1
    w = n_act - 4
    if 1 <= w and 3 + w - 1 <= T - 3:
        room = (T - 3) - (3 + w - 1)
        a = 3 + (shift % (room + 1))
        return a, a + w - 1
    assert 5 <= n_act <= T - 1, n_act
    return 1, n_act - 2                                  # 1 .. b + 2


def tile_targets(sm, span, n, rng):
    """Scaled targets of one tile's ``n`` particles on clusters a..b (``span``): particle i and
    its mirror n - 1 - i sit on clusters a + o and b - o, so the tile's centre is the span's;
    by i mod 3: the cluster's centre + 0.02 randn, the midpoint to the neighbouring cluster
    inside the span (k ~ 0.08 to both), an exact training latent.  A short tile (n < PT: the
    ragged last one) holds the span's midpoint first -- the kernel fills its empty slots with
    copies of the first particle -- then a, b, a, b ..."""
    PT, d = tile_particles(sm.d), sm.d
    Xs = sm.p["X"] / sm.ls[None, :]
    if span == "far":
        return far_point(sm)[None, :] + 0.5 * rng.rand(n, d)
    a, b = span
    lone = a == b or (a == 0)                            # no neighbour to stand between
    out = np.zeros((n, d))
    if n < PT:
        out[0] = 0.5 * (sm.centres[a] + sm.centres[b])
        for i in range(1, n):
            out[i] = sm.centres[a if i % 2 else b] + 0.02 * rng.randn(d)
        return out
    half, hw = n // 2, (b - a + 2) // 2
    for i in range(half):
        o = (i * hw) // half
        for idx, c, inward in ((i, a + o, 1), (n - 1 - i, b - o, -1)):
            kind = i % 3
            if kind == 1 and not lone and a <= c + inward <= b:
                out[idx] = 0.5 * (sm.centres[c] + sm.centres[c + inward])
            elif kind == 2:
                out[idx] = Xs[sm.members[c][(i // 3) % sm.members[c].size]]
            else:
                out[idx] = sm.centres[c] + 0.02 * rng.randn(d)
    return out


def chain_targets(sm, lengths, ragged=5, seed=0):
    """One tile per entry of ``lengths`` (its wanted n_act), the last with ``ragged`` particles
    (0: full).  Returns (targets in model units, P x d; the spans)."""
    rng = np.random.RandomState(4242 + seed)
    PT = tile_particles(sm.d)
    out, spans = [], []
    for t, n_act in enumerate(lengths):
        span = span_for(n_act, sm.T, shift=3 * t + seed)
        n = ragged if ragged and t == len(lengths) - 1 else PT
        out.append(tile_targets(sm, span, n, rng))
        spans.append(span)
    return np.ascontiguousarray(np.concatenate(out) * sm.ls[None, :]), spans


def grid_targets(sm, nodes, seed=0):
    """One full tile per grid node: every particle on that one cluster (centre + 0.02 randn, and
    exact training latents)."""
    rng = np.random.RandomState(977 + seed)
    PT = tile_particles(sm.d)
    out = [tile_targets(sm, (g, g), PT, rng) for g in nodes]
    return np.ascontiguousarray(np.concatenate(out) * sm.ls[None, :])


# ----------------------------------------------------------------------------
# the cases (shared by tests/test_cutoff_lists_ref.py and tests/test_gpu_cutoff_lists.py)
# ----------------------------------------------------------------------------

# wanted n_act per tile.  T_M = 1: n_act + 1 = 31, 32, 33, 63, 64, 65 are 30 .. 32 and 62 .. 64;
# 59 .. 61, 64, 65 stand around the first refill of the K-step window (every 60 positions) and
# its look-ahead clamp; 0, 1, 3, 5 are the far tile, the isolated cluster, the chain's end and one
# interior cluster.
LEN_66 = (5, 0, 31, 1, 32, 3, 30, 59, 60, 61, 62, 63, 64, 65)
SWEEP_66 = (5, 31, 60, 0, 32, 64, 1, 61, 65)                       # 8 PT + 5 particles
# T_M = 2: n_act + 2 = 31, 32, 33, 63, 64, 65 are 29 .. 31 and 61 .. 63
LEN_66_TM2 = (5, 0, 29, 1, 30, 3, 31, 59, 60, 61, 62, 63, 64, 65)
# T = 125 adds n_act + 1 = 96, 97 and 119 .. 121, 124, 125 (the second refill, four chunks)
LEN_125 = (0, 1, 3, 5, 30, 31, 32, 62, 63, 64, 95, 96, 59, 60, 61, 65, 119, 120, 121, 124, 125)

_MODELS = {}


def model(kind, T=66, d=3, D=7):
    key = (kind, T, d, D)
    if key not in _MODELS:
        _MODELS[key] = grid_model(D) if kind == "grid" else chain_model(T, d, D)
    return _MODELS[key]


def long_lengths(n_tiles):
    """LEN_125 repeated over ``n_tiles`` tiles (each repeat at other clusters: chain_targets
    shifts the window with the tile's index)."""
    return tuple(LEN_125[t % len(LEN_125)] for t in range(n_tiles))


def case_targets(name):
    """(scripted model, targets P x d, wanted n_act per tile or None) of a named case."""
    if name.startswith("sweep"):                      # "sweep d=<d>"
        d = int(name.split("=")[1])
        sm = model("chain", 66, d, 7)
        return sm, chain_targets(sm, SWEEP_66, seed=d)[0], SWEEP_66
    if name == "lists66":
        sm = model("chain", 66, 3, 7)
        return sm, chain_targets(sm, LEN_66, seed=1)[0], LEN_66
    if name == "tm2":
        sm = model("chain", 66, 3, 20)
        return sm, chain_targets(sm, LEN_66_TM2, seed=2)[0], LEN_66_TM2
    if name.startswith("long"):                       # "long P=<P>": a prefix of the 65-tile cloud
        P = int(name.split("=")[1])
        sm = model("chain", 125, 3, 7)
        want = long_lengths(65)
        return sm, chain_targets(sm, want, ragged=0, seed=3)[0][:P], want[:-(-P // 32)]
    if name == "grid":
        sm = model("grid")
        nodes = GRID_NODES
        return sm, grid_targets(sm, nodes), None
    raise ValueError(name)


GRID_NODES = (8 * 4 + 3, 8 * 2 + 5, 0, 71, 8 * 6 + 1)     # interior nodes, two corners
CASE_NAMES = ("sweep d=1", "sweep d=3", "sweep d=5", "sweep d=9", "lists66", "tm2", "long P=1056", "long P=2080",
              "grid")


def mixed(targets, seed=5):
    """The same targets with the particles permuted, so that every tile mixes distant clusters.
    Returns (permuted targets, order): permuted[i] = targets[order[i]]."""
    order = np.random.RandomState(seed).permutation(targets.shape[0])
    return np.ascontiguousarray(targets[order]), order
