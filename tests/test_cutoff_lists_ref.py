"""Self-checks of the cutoff lists' host model and of the scripted cases (tests/cutoff_lists_ref.py).
CPU only: everything here follows from the models and the particle targets alone.

* the numpy ``spatial_order`` / ``kstep_spheres`` against the real header, through a host program
  compiled by hipcc (tests/host/cutoff_order_check.cpp): the permutation exactly, the spheres to
  1e-14;
* the numpy chunk functions against common.h's (the same program, ``--chunks``) and against the
  properties tests/host/cutoff_plan_check.cpp restates;
* on every scripted case: each chain K-step is one cluster, each tile lists exactly the wanted
  number of K-steps, the decisiveness margin of every tile is >= 1e-3 scaled units -- also for the
  mixed (permuted) compositions --, and the cases reach what they are there for: one to four
  chunks in one launch, c* differing between tiles, n_act inside an 8-group of the finish chain
  (whose length is always whole groups at 32 entries per chunk), index gaps in the grid's lists.
"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cutoff_lists_ref as L
from conftest import ROOT

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.fixture(scope="module")
def order_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cutoff_order") / "cutoff_order_check"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", f"-I{ROOT / 'gpmdm_amd' / 'csrc'}",
           f"-I{ROOT / 'include'}", str(ROOT / "tests" / "host" / "cutoff_order_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _header_order(exe, X, ls, tmp_path):
    N, d = X.shape
    f = tmp_path / "latents.txt"
    f.write_text(f"{N} {d}\n" + " ".join(float(v).hex() for v in ls) + "\n"
                 + "\n".join(" ".join(float(v).hex() for v in row) for row in X) + "\n")
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    tok = r.stdout.split()
    i, j = tok.index("perm"), tok.index("spheres")
    perm = np.array([int(t) for t in tok[i + 1:j]], dtype=np.int64)
    sph = np.array([float.fromhex(t) for t in tok[j + 1:-1]]).reshape(-1, d + 1)
    return perm, sph


def _tied_model(d, N=203, seed=3):
    """Latents with repeated coordinate values (ties sort by training row) and two axes of exactly
    equal spread (the first one wins)."""
    rng = np.random.RandomState(seed)
    X = np.round(rng.randn(N, d) * 2.0, 1)
    if d > 1:
        X[0, :2], X[1, :2] = -9.0, 9.0
    return X, rng.uniform(0.5, 2.0, d)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
@pytest.mark.parametrize("which", ["chain d=1", "chain d=3", "chain d=9", "chain T=125", "grid", "ties d=1", "ties d=4"])
def test_order_and_spheres_match_the_header(order_check, tmp_path, which):
    if which.startswith("ties"):
        X, ls = _tied_model(int(which[-1]))
    else:
        sm = {"chain d=1": lambda: L.model("chain", 66, 1, 7), "chain d=3": lambda: L.model("chain", 66, 3, 7),
              "chain d=9": lambda: L.model("chain", 66, 9, 7), "chain T=125": lambda: L.model("chain", 125, 3, 7),
              "grid": lambda: L.model("grid")}[which]()
        X, ls = sm.p["X"], sm.ls
    perm_h, sph_h = _header_order(order_check, X, ls, tmp_path)
    perm = L.spatial_order(X, ls)
    assert np.array_equal(np.sort(perm), np.arange(X.shape[0]))
    assert np.array_equal(perm, perm_h), np.nonzero(perm != perm_h)[0][:10]
    sph = L.kstep_spheres(X, ls, perm)
    assert sph.shape == sph_h.shape
    assert np.max(np.abs(sph - sph_h)) <= 1e-14 * max(1.0, float(np.max(np.abs(sph_h)))), np.max(np.abs(sph - sph_h))


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_chunk_functions_match_the_header(order_check):
    r = subprocess.run([str(order_check), "--chunks"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    lines = r.stdout.strip().splitlines()[:-1]
    assert len(lines) == 2 * 301
    for line in lines:
        T_M, n_act, cs, *begins = (int(t) for t in line.split())
        nt = n_act + T_M
        assert L.split_chunk(n_act, T_M) == cs, line
        assert [L.chunk_begin(c, nt) for c in range(len(begins))] == begins, line


def test_chunk_functions_properties():
    """tests/host/cutoff_plan_check.cpp's restatement, on the numpy functions: the chunks tile
    the list, only the first is partial, positions follow the last R tile's diagonal, the split
    minimises the larger part (a chunk's pipeline fill counted as 4 positions)."""
    for tpc in (32, 16, 8):
        for T_M in (1, 2, 4, 8, 17):
            for n_act in range(0, 701, 1 if tpc == 32 else 7):
                nt = n_act + T_M
                nc = -(-nt // tpc)
                assert L.chunk_begin(0, nt, tpc) == 0 and L.chunk_begin(nc, nt, tpc) == nt
                cost = []
                for c in range(nc):
                    b, e = L.chunk_begin(c, nt, tpc), L.chunk_begin(c + 1, nt, tpc)
                    assert 0 < e - b <= tpc and (c == 0 or e - b == tpc)
                    pos = e if e - 1 < n_act else n_act
                    assert L.chunk_positions(c, n_act, T_M, tpc) == pos
                    cost.append(pos + 4)
                cs = L.split_chunk(n_act, T_M, tpc)
                if nc < 2:
                    assert cs == nc
                else:
                    assert 1 <= cs < nc
                    tot = sum(cost)
                    best = min(max(sum(cost[:c]), tot - sum(cost[:c])) for c in range(1, nc))
                    assert max(sum(cost[:cs]), tot - sum(cost[:cs])) == best


@pytest.mark.parametrize("T,d", [(66, 1), (66, 3), (66, 5), (66, 9), (125, 3)])
def test_chain_ksteps_are_the_clusters(T, d):
    """K-step k of the image holds exactly cluster k's training rows, and the cutoff distance lies
    in the band the targets were designed for."""
    sm = L.model("chain", T, d, 7)
    assert sm.N == 16 * T - 5
    lm = sm.list_model(sm.host_tau())
    assert lm.T_R == T and 7.3 <= lm.reach <= 8.3, lm.reach
    for k in range(T):
        assert np.array_equal(np.sort(lm.perm[16 * k:16 * k + 16]), sm.members[k]), k
    assert lm.spheres[:, d].max() < 0.6


def _lists(name, mix=False):
    sm, targets, want = L.case_targets(name)
    lm = sm.list_model(sm.host_tau())
    if mix:
        targets = L.mixed(targets)[0]
    return sm, lm, lm.tiles(targets), want


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_scripted_lists_are_the_wanted_ones(name):
    sm, lm, lists, want = _lists(name)
    # the chain's margins are about 1 by design; the grid's are whatever its K-steps give
    floor = 0.3 if want is not None else L.MIN_MARGIN
    assert min(t.margin for t in lists) >= floor, [round(t.margin, 3) for t in lists]
    if want is not None:
        assert [t.n_act for t in lists] == list(want)
        for t in lists:                                    # contiguous: a - 2 .. b + 2
            assert t.gaps == 0
    run, dense = lm.stats(lists)
    assert 0 < run < dense


@pytest.mark.parametrize("name", ["lists66", "sweep d=9", "tm2"])
def test_mixed_compositions_are_decisive(name):
    """The permuted clouds of the composition test: every tile mixes distant clusters and lists
    (nearly) every K-step, most of them flushed for each of its particles; still decisive."""
    sm, lm, lists, _ = _lists(name, mix=True)
    assert min(t.margin for t in lists) >= L.MIN_MARGIN
    assert min(t.n_act for t in lists) >= 35


def test_cases_reach_what_they_are_for():
    _, lm, lists, _ = _lists("long P=2080")
    assert {t.n_chunks for t in lists} == {1, 2, 3, 4}          # some chunk-grid workgroups find no chunk
    assert len({t.c_star for t in lists if t.n_chunks >= 2}) >= 2
    _, _, l66, _ = _lists("lists66")
    assert {t.n_chunks for t in l66} == {1, 2, 3}
    _, _, ltm2, _ = _lists("tm2")
    assert ltm2[0].T_M == 2
    assert {t.n_tiles for t in ltm2} >= {31, 32, 33, 63, 64, 65}
    assert {t.n_tiles for t in l66} >= {31, 32, 33, 63, 64, 65}
    assert {t.n_tiles for t in lists} >= {96, 97} and {t.n_act for t in lists} >= {119, 120, 121, 124, 125}
    # the finish chain of a split tile (obs_ll_value): list entries finish_from .. n_tiles in
    # groups of 8 and a remainder.  Every chunk but the first is full, so the chain's length is
    # (n_chunks - c*) x 32: always whole groups -- the remainder loop cannot run at 32 entries
    # per chunk, whatever the list (asserted for every list length, so that a change of the chunk
    # size shows up here) --, while n_act (the switch from q to S) falls strictly inside the last
    # group, T_M entries before its end
    for T_M in (1, 2):
        for n_act in range(0, 4097):
            nt = n_act + T_M
            assert (nt - L.chunk_begin(L.split_chunk(n_act, T_M), nt)) % 8 == 0
    for ls_ in (l66, lists, ltm2):
        split = [t for t in ls_ if t.n_chunks >= 2]
        # (positions grow along the list, so the balanced split leaves the last chunk alone: the
        # chain is 32 entries at every length reached here, starting at c* = 1, 2 or 3)
        assert {t.c_star for t in split} == ({1, 2, 3} if ls_ is lists else {1, 2})
        assert {t.n_chunks - t.c_star for t in split} == {1}
        inside = [t for t in split
                  if t.finish_from < t.n_act < t.finish_from + 8 * ((t.n_tiles - t.finish_from) // 8)
                  and (t.n_act - t.finish_from) % 8]
        assert inside


def test_grid_lists_have_index_gaps():
    sm, lm, lists, _ = _lists("grid")
    assert max(t.gaps for t in lists) >= 3, [t.gaps for t in lists]
    assert all(0 < t.n_act < lm.T_R for t in lists)
    assert min(t.margin for t in lists) >= L.MIN_MARGIN, [t.margin for t in lists]
