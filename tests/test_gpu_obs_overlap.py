"""The dense observation tile's K-step on scripted activity patterns (gp_tile.h full_step; DESIGN.md
§3.4 "Flush and skip in the dense tile").

A K-step's generated values, their stores into the K* ring and the bits of its activity word are
placed by hand around the branches of its eight (sub-step, row block) fragments, so a value can be
dropped, stored twice or land in the wrong ring slot exactly where the activity pattern changes.  The model
here scripts that pattern: N = 540 training latents in 135 clusters of 4 consecutive rows on a grid
spaced 16 l apart (the flush's cutoff distance is about 7.5 l), so a cluster is one (K-step,
sub-step) block of kernel values, and each 16-particle row block of the cloud (P = 777, a partial
last tile) sits near chosen clusters or near none.  Within one launch there are K-steps with no
active fragment, with exactly one at each position on even and odd K-steps, with all active, and
one-fragment K-steps that are the last before a tile retires and the last of a column block
(``test_scripted_pattern_holds_the_cases`` checks this on the CPU from the kernel values).

What is held, per shape (16 x 256, 16-row tiles over 32 x 512, 32 x 512, 32 x 512 with the
coordinates in LDS, 64 x 512), with the block skip on and off:

* per-particle ll, weights and ancestors equal, bit for bit, the arrays recorded from the commit
  before the K-step was reordered (tests/golden/obs_overlap_parent.npz);
* per-particle ll against the extended-precision reference at the model's tau, under
  test_gpu_obs_skip.test_default_filter_ll_per_particle_with_flush's rule and margin.

The 32 x 512 tiles proper at d <= 12 need GPMDM_OBS_SMALL_TILES=0, which is read once per process:
those cases run in one child process (this file as a script)."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "obs_overlap_parent.npz"
P, N, NCL = 777, 540, 135
# shape -> (environment, dimensions, the golden arrays' shape key): 16-row tiles over the 32 x 512
# image are bitwise its 32-row tiles (capi_internal.h obs_pick), so they share one recording
SHAPES = {
    "16x256": ({}, (1, 3, 8), "16x256"),
    "16x512": ({"GPMDM_OBS_IMAGE16": "0"}, (3, 8), "32x512"),
    "32x512": ({"GPMDM_OBS_IMAGE16": "0", "GPMDM_OBS_SMALL_TILES": "0"}, (3, 8), "32x512"),
    "32x512lds": ({"GPMDM_TILE_SHAPE": "3"}, (13,), "32x512lds"),
    "64x512": ({}, (13, 16), "64x512"),
}
IN_PROCESS = [(s, d) for s in ("16x256", "16x512", "32x512lds", "64x512") for d in SHAPES[s][1]]
CHILD = [("32x512", d) for d in SHAPES["32x512"][1]]
KEYS = ("ll", "w", "resample_idx")


# ----------------------------------------------------------------------------
# the scripted model and cloud (CPU)
# ----------------------------------------------------------------------------

def _grid(d):
    """Cluster centres in units of l: 135 points of a grid spaced 16 apart over min(d, 3) axes,
    around the origin so that the expansion form's |a|^2 + |b|^2 stays small."""
    dims = (NCL,) if d == 1 else (12, 12) if d == 2 else (6, 6, 4)
    idx = np.stack(np.unravel_index(np.arange(NCL), dims), axis=1).astype(np.float64)
    c = np.zeros((NCL, d))
    c[:, :idx.shape[1]] = 16.0 * (idx - (np.array(dims) - 1) // 2)
    # nearest the origin first: the replayed step starts every particle at training row 0, where
    # the dynamics GP's linear kernel is then small and its variance free of cancellation
    return c[np.argsort(np.sum(c * c, axis=1), kind="stable")]


@functools.lru_cache(maxsize=None)
def scripted(d):
    """(parameter dict, targets[P, d], near[P]): the model, the cloud and the cluster each particle
    sits near (-1: none)."""
    import extended_ref as E
    p = E.recipe_model(d, L=90, ls_range=(0.4, 0.6))
    assert p["X"].shape == (N, d)
    rng = np.random.RandomState(500 + d)
    ell = np.exp(p["y_log_lengthscales"])
    cen = _grid(d)
    X = (np.repeat(cen, 4, axis=0) + 0.25 * rng.randn(N, d) / np.sqrt(d)) * ell
    W = rng.randn(d, p["Y"].shape[1])
    p["X"] = X
    p["Y"] = np.sin((X / ell) @ W / 16.0 + rng.uniform(0, 6, p["Y"].shape[1])) + 0.05 * rng.randn(*p["Y"].shape)
    near = row_block_script()
    tg = np.empty((P, d))
    on = near >= 0
    tg[on] = cen[near[on]] + 0.4 * rng.randn(int(on.sum()), d) / np.sqrt(d)
    # particles near no cluster: 10-12 l past the grid along the first axis (every value non-zero
    # and flushed), every fourth of them 60 l out (every value underflows)
    out = np.flatnonzero(~on)
    tg[out] = cen.max(axis=0) + 0.3 * rng.randn(out.size, d) / np.sqrt(d)
    tg[out, 0] += np.where(np.arange(out.size) % 4 == 3, 60.0, 10.0 + 2.0 * rng.rand(out.size))
    return p, tg * ell, near


def row_block_script():
    """near[P]: the cluster (4 K-step + sub-step) each particle sits near, by 16-particle row block."""
    near = np.full(P, -1, dtype=np.int64)

    def put(rb, clusters):
        sl = np.arange(16 * rb, min(16 * rb + 16, P))
        near[sl] = np.asarray(clusters)[np.arange(sl.size) % len(clusters)]

    for rb in range(4):                       # K-step 5: every fragment of the tile active, at MT = 1, 2, 4
        put(rb, [20, 21, 22, 23])
    for j in range(32):                       # one fragment: sub-step kk, row block j % 4, K-step parity par
        q = j // 4
        kk, par = q % 4, (q // 4) % 2
        ks = 2 * ((3 * j) % 16) + par          # distinct within a 64-particle tile
        put(4 + j, [4 * ks + kk])
    put(36, [4 * 33 + 2])                     # the block's last K-step (12 real rows), alone in its tile
    put(40, [4 * 2 + 1])                      # K-step 2: the last of the 512-wide first column block
    put(44, [4 * 7 + 0, 4 * 12 + 3])          # a row block over two K-steps ...
    put(45, [4 * 7 + 0, -1])                  # ... and half of one near nothing
    put(46, [4 * 12 + 3, 4 * 12 + 2, 4 * 30 + 1, -1])
    put(47, [4 * 33 + 0])
    put(48, [4 * 16 + 2])                     # the partial last tile (9 particles)
    return near                               # row blocks 37-39, 41-43: near nothing


def activity(p, xs, tau):
    """act[row block, cluster]: a kernel value >= tau among the block's particles and the cluster's
    rows (fp64 kernel values of the propagated states)."""
    import obs_flush_ref as F
    k = F.kernel_values(p, xs) >= tau                                    # N x P
    k = k.reshape(NCL, 4, P).any(axis=1)
    nrb = -(-P // 16)
    pad = np.zeros((NCL, 16 * nrb), dtype=bool)
    pad[:, :P] = k
    return pad.reshape(NCL, nrb, 16).any(axis=2).T


def check_pattern(act):
    """The cases the launch must hold, for tiles of MT = 1, 2 and 4 row blocks."""
    nrb = act.shape[0]
    a = np.zeros((nrb, 34, 4), dtype=bool)
    a.reshape(nrb, 136)[:, :NCL] = act
    for MT in (1, 2, 4):
        nt = -(-nrb // MT)
        t = np.zeros((nt * MT, 34, 4), dtype=bool)
        t[:nrb] = a
        t = t.reshape(nt, MT, 34, 4).transpose(0, 2, 3, 1)               # tile, K-step, kk, mt
        cnt = t.reshape(nt, 34, 4 * MT).sum(axis=2)
        assert (cnt == 0).any() and (cnt == 4 * MT).any(), MT
        one = cnt == 1
        seen = {(int(ks) % 2, int(kk), int(mt)) for ti, ks in zip(*np.nonzero(one))
                for kk, mt in zip(*np.nonzero(t[ti, ks]))}
        assert len(seen) == 2 * 4 * MT, (MT, sorted(seen))              # every position, even and odd K-steps
        ks_one = set(int(k) for k in np.nonzero(one)[1])
        # a tile retires after K-step ceil((c0 + 16) / 16) - 1 for its first column c0: with four or
        # eight waves' tiles interleaved, every K-step from 3 to 32 is some wave's last before one
        assert 33 in ks_one and 2 in ks_one and len(ks_one & set(range(3, 33))) >= 16, sorted(ks_one)


def test_scripted_pattern_holds_the_cases():
    """CPU: the scripted cloud's activity pattern, from fp64 kernel values of the targets with the
    tau of host_image.h obs_cutoff_tau restated in numpy, holds every case listed above."""
    import extended_ref as E
    import obs_flush_ref as F
    for d in (1, 3, 16):
        p, tg, near = scripted(d)
        om = E.oracle_of(p)
        sigma2 = float(np.exp(p["y_log_sigma_n"])) ** 2
        tau = F.tau_numpy(N, sigma2, om.Ky_inv @ om.Y, np.max(np.abs(p["Y"]), axis=0))
        assert 0.0 < tau < 1e-15
        act = activity(p, tg, tau)
        want = np.zeros_like(act)
        for i in np.flatnonzero(near >= 0):
            want[i // 16, near[i]] = True
        assert np.array_equal(act, want), d
        check_pattern(act)


# ----------------------------------------------------------------------------
# the device
# ----------------------------------------------------------------------------

def run_case(shape, d, skip):
    """One replayed step of the scripted cloud on ``shape`` (the environment must hold the shape's
    switches): the step's arrays and the propagated states."""
    import extended_ref as E
    import test_gpu_obs_skip as S
    from gpmdm_amd import GPMDM
    p, tg, _ = scripted(d)
    m = GPMDM.from_arrays(p["X"], E.y_sequences(p), **E.hyper(p))
    out, _ = S.placed_step(p, m, tg, skip=skip)
    st = out["st"]
    return dict(ll=out["ll"], w=st["w"], resample_idx=st["resample_idx"], states1=out["states1"],
                tau=np.float64(m.obs_flush_tau), rows=out["rows"], z=p["Y"][17])


def run_cases(cases):
    """{f"{shape}_d{d}_{on|off}_{key}": array} for the listed (shape, d) cases."""
    res = {}
    for shape, d in cases:
        for skip in (True, False):
            r = run_case(shape, d, skip)
            for k, v in r.items():
                res[f"{shape}_d{d}_{'on' if skip else 'off'}_{k}"] = np.asarray(v)
    return res


@functools.lru_cache(maxsize=None)
def child_results():
    """The 32 x 512 cases, from a child process with the shape's environment."""
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        path = Path(t) / "child.npz"
        env = dict(os.environ, **SHAPES["32x512"][0])
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path)], env=env, capture_output=True,
                           text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        return dict(np.load(path))


@functools.lru_cache(maxsize=None)
def results(shape, d):
    """{on|off: arrays} of one case, computed once."""
    if (shape, d) in CHILD:
        res = child_results()
    else:
        old = {k: os.environ.get(k) for k in SHAPES[shape][0]}
        os.environ.update(SHAPES[shape][0])
        try:
            res = run_cases([(shape, d)])
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    pre = f"{shape}_d{d}_"
    return {s: {k[len(pre) + len(s) + 1:]: v for k, v in res.items() if k.startswith(pre + s + "_")} for s in ("on", "off")}


@functools.lru_cache(maxsize=None)
def reference(d):
    import extended_ref as E
    p, _, _ = scripted(d)
    return E.ExtendedModel(p), E.oracle_of(p)


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("shape,d", IN_PROCESS + CHILD)
def test_bits_of_the_parent_build(shape, d):
    """ll, weights and ancestors of every particle, skip on and skip off, against the recording."""
    gold = np.load(GOLDEN)
    res = results(shape, d)
    act = activity(scripted(d)[0], res["on"]["states1"], float(res["on"]["tau"]))
    check_pattern(act)
    for s in ("on", "off"):
        for k in KEYS:
            g, v = gold[f"{SHAPES[shape][2]}_d{d}_{k}"], np.ascontiguousarray(res[s][k])
            assert g.shape == v.shape and g.dtype == v.dtype, (shape, d, s, k)
            bad = np.flatnonzero(g.view(np.uint64) != v.view(np.uint64))
            assert bad.size == 0, (shape, d, s, k, f"{bad.size} particles differ, first {bad[:8]}")


@gpu
@pytest.mark.parametrize("shape,d", IN_PROCESS + CHILD)
def test_ll_per_particle_against_the_reference(shape, d):
    """|ll_gpu - ll_ref(tau)| / terms <= MARGIN max(oracle's worst, 16 eps) for every particle
    (test_gpu_obs_skip.test_default_filter_ll_per_particle_with_flush's rule)."""
    import extended_ref as E
    import obs_flush_ref as F
    import test_gpu_gp_accuracy as A
    from extended_ref import ld
    r = results(shape, d)["on"]
    ref, om = reference(d)
    p = ref.p
    tau, states1, z = float(r["tau"]), r["states1"], np.ascontiguousarray(r["z"], dtype=np.float64)
    assert 0.0 < tau < 1e-15
    ll_r, terms = ref.loglik(states1, z, tau)
    lam = np.exp(p["y_log_lambdas"]) ** -2
    mu_o, vc_o = F.oracle_obs_triangular_flushed(om, states1, tau)
    ll_o, _ = E.loglik_from_map(mu_o, vc_o[:, None] * lam[None, :], z)
    e_gpu = (np.abs(ld(r["ll"]) - ll_r) / terms).astype(np.float64)
    e_or = (np.abs(ld(ll_o) - ll_r) / terms).astype(np.float64)
    yard = max(float(np.max(e_or)), A.FLOOR)
    print(f"{shape} d={d}: device {np.max(e_gpu):.3e}, yardstick {yard:.3e}, ratio {np.max(e_gpu) / yard:.2f}")
    assert np.max(e_gpu) <= A.MARGIN * yard, (shape, d, float(np.max(e_gpu)), yard)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    np.savez(sys.argv[1], **run_cases(CHILD))
