"""The dense tile's epilogue, bit for bit against a recording (gp_tile.h k_gp_tile "epilogue";
DESIGN.md §3).

The epilogue stores the mean columns of a predictive map or, in a filter, sums them into the
likelihood partials (one filter's z and lambda^2 per tile, or each particle's own filter's where a
tile mixes filters of a bank, masked or not); zeroes them; sums the squares of the R columns; and
reduces both over the waves.  The other tests that hold it bitwise compare two launches of one build
(bank rows against single filters, narrow dynamics tiles against wide ones), so they cannot see a
change that moves both sides.  This file holds the parts they leave open to arrays recorded from
commit f11690f, before the epilogue's and the K-step's shared parts were given one definition each
(tests/golden/tile_epilogue_parent.npz, written by ``python tests/test_gpu_tile_epilogue.py OUT.npz``
on a build of that commit; ``run_cases`` is the recorder's and the tests').

What is recorded is less than every bit of every output, to keep the fixture under 88 KB: the P x D
observation variance and the bank's states are held by XOR folds (and the variance's first column),
not in full.  A single flipped bit always shows; two flips in one row and one column could cancel.

Predictive maps (the unfused mean store).  N = 540 training rows, D = 600 observation dimensions,
P = 37 query points (a partial last tile at 16, 32 and 64 rows), d = 3 and 13, default tile shapes
and GPMDM_TILE_SHAPE = 1, 2, 3.  With 1140 columns the front padding is 384 at 512-column blocks
and 128 at 256-column blocks: both widths have a block of R columns only, a block holding the R / M
boundary at column 540 and a block of mean columns only (``block_kinds`` restates geometry.h and the
test asserts it for the image it runs).  Recorded per case: of the P x D mean the XOR of the
values' bit patterns over the particles per column and over the columns per particle (a flipped bit
changes one word of each, which locates it); the variance's first column (every column is the
particle's own factor times 1 / lambda_j^2, k_obs_finish) and its XOR over the columns per particle;
the same four of each class's dynamics map (GPMDM_TILE_SHAPE = 3 changes the observation image only,
so its dynamics maps are the default's and are left out).

A bank whose tiles mix filters (the fused sums).  F = 3 filters of 24 particles on a model of
N = 540, D = 62, one ``update``: unmasked, and with three different per-filter masks (one leaves a
single joint observed), dyn_tiles narrow and wide, on every observation shape of
test_gpu_obs_overlap.SHAPES that admits the d.  Recorded per case: ll, w, resample_idx and the two
XOR folds of the states.  Cases the kernels make bitwise equal by design share one recording
(``bank_key``): 16-row tiles over the 32 x 512 image and its 32-row tiles, and at d = 3 narrow and
wide dynamics tiles (the wide shape reduces each 256-column half as the narrow one does); the
recorder asserts they agree before it keeps one.

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
GOLDEN = ROOT / "tests" / "golden" / "tile_epilogue_parent.npz"
N, L, P_MAP, D_MAP = 540, 90, 37, 600
F, PF, D_BANK, SEED = 3, 24, 62, 77
DIMS = (3, 13)
# GPMDM_TILE_SHAPE -> the observation image's block width at d = 3, 13 (capi_model.hip
# gpmdm_model_create: 0 is 32 x 512 or, above d = 12, 64 x 512; 1: 64 x 256; 2: 64 x 512; 3: 32 x 512)
MAP_SHAPES = {0: 512, 1: 256, 2: 512, 3: 512}
MAP_CASES = [(d, s) for d in DIMS for s in MAP_SHAPES]
DYN_TILES = ("narrow", "wide")


def bank_shapes():
    from test_gpu_obs_overlap import SHAPES
    return SHAPES


def bank_cases(child):
    """(shape, d, dyn_tiles, masked) of the cases run in this process, or in the child."""
    return [(s, d, t, mk) for s, (_, dims, _) in bank_shapes().items() if (s == "32x512") == child
            for d in DIMS if d in dims for t in DYN_TILES for mk in (False, True)]


def bank_key(shape, d, tiles, masked):
    return f"bank_{bank_shapes()[shape][2]}_d{d}_{'dyn' if d <= 12 else tiles}_{'masked' if masked else 'plain'}"


# ----------------------------------------------------------------------------
# geometry.h, restated
# ----------------------------------------------------------------------------

def col_offset(n_cols, nb):
    r = n_cols % nb
    return (nb - r) // 16 * 16 if r else 0


def block_kmax(J, n_rows, nb, coff):
    return min((J + 1) * nb - coff, n_rows)


def block_kinds(n_rows, n_m, nb):
    """The kinds of column blocks of an image of [R (n_rows) | M (n_m)] in nb-column blocks."""
    coff = col_offset(n_rows + n_m, nb)
    kinds = []
    for J in range(-(-(n_rows + n_m + coff) // nb)):
        lo, hi = J * nb - coff, (J + 1) * nb - coff
        has_r, has_m = lo < n_rows, hi > n_rows
        assert block_kmax(J, n_rows, nb, coff) == (n_rows if has_m else hi)
        kinds.append("R" if not has_m else "RM" if has_r else "M")
    return coff, kinds


def test_block_kinds_of_the_map_images():
    assert block_kinds(N, D_MAP, 512) == (384, ["R", "RM", "M"])
    assert block_kinds(N, D_MAP, 256) == (128, ["R", "R", "RM", "M", "M"])


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def folds(a):
    """(columns' words, rows' words) of a 2-D float64 array: XOR of the bit patterns over axis 0, 1."""
    u = bits(a)
    return np.bitwise_xor.reduce(u, axis=0), np.bitwise_xor.reduce(u, axis=1)


@functools.lru_cache(maxsize=None)
def params(d, D):
    import extended_ref as E
    return E.recipe_model(d, L=L, D=D, seed=700 + d)


def build_model(d, D, env):
    """The device model with ``env`` in force while it is built (the switches read at build time)."""
    import extended_ref as E
    from gpmdm_amd import GPMDM
    p = params(d, D)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return GPMDM.from_arrays(p["X"], E.y_sequences(p), **E.hyper(p))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def map_pieces(name, mu, var):
    cols, rows = folds(mu)
    return {f"{name}_mu_cols": cols, f"{name}_mu_rows": rows, f"{name}_var0": bits(var[:, 0]),
            f"{name}_var_rows": folds(var)[1]}


def run_map_case(d, shape):
    import torch
    p = params(d, D_MAP)
    assert p["X"].shape == (N, d)
    m = build_model(d, D_MAP, {"GPMDM_TILE_SHAPE": str(shape)})
    assert m.tile_shape == shape
    rng = np.random.RandomState(40 + d)
    xs = torch.from_numpy(p["X"][rng.permutation(N)[:P_MAP]] + 0.3 * rng.randn(P_MAP, d) / np.sqrt(d))
    mu, var = (t.numpy() for t in m.map_x_to_y(xs))
    assert mu.shape == var.shape == (P_MAP, D_MAP)
    out = map_pieces("obs", mu, var)
    if shape != 3:
        for c in range(m.n_classes):
            out.update(map_pieces(f"dyn{c}", *(t.numpy() for t in m.map_x_dynamics_for_class(xs, c))))
    return out


def masks():
    j = np.arange(D_BANK)
    return np.stack([j % 3 != 2, j >= 16, j == 37])          # filter 2: a single joint observed


@functools.lru_cache(maxsize=None)
def bank_model(shape, d):
    return build_model(d, D_BANK, bank_shapes()[shape][0])


def run_bank_case(shape, d, tiles, masked):
    import torch
    from gpmdm_amd import GPMDM_PF_Bank, synthetic
    p = params(d, D_BANK)
    m = bank_model(shape, d)
    bank = GPMDM_PF_Bank(m, torch.tensor(synthetic.markov_matrix(m.n_classes)), F, PF, seed=SEED, dyn_tiles=tiles)
    Z = p["Y"][[17, 120, 300]] + 0.05 * np.random.RandomState(9).randn(F, D_BANK)
    if masked:
        bank.update(np.where(masks(), Z, np.nan), observed=masks())
    else:
        bank.update(Z)
    st = bank.export_state()
    assert np.all(np.isfinite(st["ll"]))
    cols, rows = folds(st["states"].reshape(F * PF, d))
    return {"ll": bits(st["ll"]).ravel(), "w": bits(st["w"]).ravel(),
            "resample_idx": st["resample_idx"].ravel().astype(np.uint64), "states_cols": cols, "states_rows": rows}


def run_cases(maps, banks):
    """{case key: {piece: uint64 words}} for the listed map cases (d, shape) and bank cases (shape, d,
    dyn_tiles, masked); bank cases that share a recording must agree."""
    res = {}
    for d, shape in maps:
        res[f"map_d{d}_shape{shape}"] = run_map_case(d, shape)
    for case in banks:
        r, key = run_bank_case(*case), bank_key(*case)
        if key in res:
            for k, v in r.items():
                assert np.array_equal(res[key][k], v), (case, k, "differs from the case it shares a recording with")
        res[key] = r
    return res


def pack(res):
    """One array per case: its pieces in order (their sizes follow from the case)."""
    return {key: np.concatenate(list(r.values())) for key, r in res.items()}


def compare(key, r, gold):
    g, at = gold[key], 0
    assert g.dtype == np.uint64 and g.size == sum(v.size for v in r.values()), key
    for k, v in r.items():
        bad = np.flatnonzero(g[at:at + v.size] != v)
        assert bad.size == 0, (key, k, f"{bad.size} words differ, first {bad[:8]}")
        at += v.size


@functools.lru_cache(maxsize=None)
def child_results():
    """The 32 x 512 bank cases, from a child process with the shape's environment."""
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        path = Path(t) / "child.npz"
        env = dict(os.environ, **bank_shapes()["32x512"][0])
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(path), "child"], env=env,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        return dict(np.load(path))


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("d,shape", MAP_CASES)
def test_maps_bits_of_the_parent_build(d, shape):
    """The unfused mean store, mean-only and R-only blocks: both maps of 37 points."""
    coff, kinds = block_kinds(N, D_MAP, MAP_SHAPES[shape])
    assert {"R", "RM", "M"} <= set(kinds) and coff == {512: 384, 256: 128}[MAP_SHAPES[shape]]
    (key, r), = run_cases([(d, shape)], []).items()
    compare(key, r, np.load(GOLDEN))


@gpu
@pytest.mark.parametrize("shape,d,tiles,masked", bank_cases(False) + bank_cases(True))
def test_bank_bits_of_the_parent_build(shape, d, tiles, masked):
    """The fused sums where a tile mixes filters, with one lambda^2 row and with the filters' own."""
    case = (shape, d, tiles, masked)
    key = bank_key(*case)
    gold = np.load(GOLDEN)
    if case in bank_cases(True):
        assert np.array_equal(child_results()[key], gold[key]), key
    else:
        compare(key, run_cases([], [case])[key], gold)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    if sys.argv[2:] == ["child"]:
        np.savez(sys.argv[1], **pack(run_cases([], bank_cases(True))))
    else:
        # the recorder: the child's cases first, so that a case run here that shares a recording with
        # one of them is held to it
        rec = child_results()
        mine = pack(run_cases(MAP_CASES, bank_cases(False)))
        for key in set(rec) & set(mine):
            assert np.array_equal(rec[key], mine[key]), (key, "differs from the case it shares a recording with")
        np.savez_compressed(sys.argv[1], **{**rec, **mine})
