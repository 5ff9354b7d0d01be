"""Per-particle tests of the cutoff kernel (gpmdm_amd/csrc/obs_cutoff.h) on scripted K-step lists.

Every other per-point check of this kernel stops at lists of one chunk (test_gpu_gp_accuracy.py:
N = 330, T_R + T_M <= 32), and the tests at longer lists are normwise at 1e-5 against ll ~ -1e5 or
compare one schedule with another.  Here the lists are scripted (tests/cutoff_lists_ref.py): chain
models whose K-steps are clusters, and particle tiles placed so that each tile of one launch has
its own list length -- 0, 1, 3, 5, around 32, 64 and 96 entries, around the K-step window's
refills at 60 and 120 positions, one to four chunks side by side.

The propagated cloud is steered onto the targets through the dynamics GP by three replayed passes
from one loaded state: normals 0 give mu, normals 1 give s = X_one - mu, normals (target - mu) / s
land on the target to 1e-9 l.  Every reference is evaluated at the states read back.

Asserted:
 (a) per particle, ll and vc = variance_common against extended_ref.ExtendedModel with the flush
     at tau: worst device error <= MARGIN x max(worst error of the fp64 explicit-inverse oracle
     on the same points, 16 eps) -- test_gpu_gp_accuracy.py's rule, unchanged -- per list-length
     class (far, 1, 2, 3, 4 chunks); in a far tile vc is exactly 1.0.  The ratios go to
     cutoff_lists.json in the directory GPMDM_ACCURACY_OUT names (default test_out/); a run's file
     is committed as profiles/cutoff_lists/summary.json;
 (b) exact integers: obs_cutoff_stats() after one weigh equals the host model's
     run = MT sum_tiles [n_act (n_act + 1) / 2 + T_M n_act] and dense = MT tiles [T_R (T_R + 1) / 2 +
     T_M T_R] under every split policy: the device's lists are the scripted ones;
 (c) bitwise: each particle's ll and vc under the split policies none, tail, all, chunks and auto;
     in other tile compositions (the same targets permuted so that every tile mixes distant
     clusters and runs dozens of K-steps flushed for each of its particles); on two logical
     shards, which move every tile boundary.
"""
import json
import os
import time
from pathlib import Path

import numpy as np
import pytest
import torch

import cutoff_lists_ref as L
import extended_ref as E
from extended_ref import EPS64, LD, ld

pytestmark = pytest.mark.gpu

MARGIN = 8.0                     # test_gpu_gp_accuracy.py's
FLOOR = 16 * EPS64
STEER_TOL = 1e-9                 # |x' - target| / l per coordinate
SPLITS = ("tail", "all", "chunks", "auto")
RATIOS, TIMES = {}, {}
_REFS, _RUNS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def ratio_log():
    yield
    if RATIOS:
        out = Path(os.environ.get("GPMDM_ACCURACY_OUT") or E.ROOT / "test_out")
        out.mkdir(parents=True, exist_ok=True)
        (out / "cutoff_lists.json").write_text(json.dumps(
            {"margin": MARGIN, "floor_eps": 16,
             "note": "ratio = worst device error / max(worst error of the fp64 explicit-inverse oracle with the "
                     "same flush, 16 eps) against the longdouble reference, per case and list-length class; "
                     "yardstick_eps = that denominator in units of 2^-52; points = particles in the class",
             "ratios": RATIOS, "seconds": TIMES}, indent=1, sort_keys=True))


def held(section, key, e_gpu, e_or):
    """Record and assert max e_gpu <= MARGIN max(max e_or, 16 eps)."""
    yard = max(float(np.max(e_or)), FLOOR)
    ratio = float(np.max(e_gpu)) / yard
    cur = RATIOS.setdefault(section, {}).get(key)
    if cur is None or ratio > cur["ratio"]:
        RATIOS[section][key] = {"ratio": round(ratio, 3), "yardstick_eps": round(yard / EPS64, 1), "points": int(len(e_gpu))}
    assert ratio <= MARGIN, (section, key, f"device {np.max(e_gpu):.3e}, yardstick {yard:.3e}, ratio {ratio:.2f}")


class Ref:
    """A scripted model with its longdouble reference, its fp64 oracle, its device model and its
    host list model (at the device's tau); reference values are kept per state, so a particle that
    lands on the same bits in another run is evaluated once."""

    def __init__(self, sm):
        from gpmdm_amd import GPMDM
        self.sm, p = sm, sm.p
        t0 = time.time()
        self.ref, self.om = E.ExtendedModel(p), E.oracle_of(p)
        TIMES.setdefault("host_factor", {})[f"N={sm.N} d={sm.d} D={sm.D}"] = round(time.time() - t0, 1)
        self.m = GPMDM.from_arrays(p["X"], E.y_sequences(p), **E.hyper(p))
        self.m.enable_obs_cutoff(True)
        self.tau = self.m.obs_cutoff_tau
        host = sm.host_tau()
        assert 0.0 < self.tau < 1e-15 and abs(self.tau - host) <= 1e-6 * self.tau, (self.tau, host)
        self.lm = sm.list_model(self.tau)
        assert self.lm.PT == (32 if sm.d <= 8 else 64)
        self.z = np.ascontiguousarray(p["Y"][17], dtype=np.float64)
        self.lam = np.exp(p["y_log_lambdas"]) ** -2
        self.cache = {}

    def evaluate(self, states):
        """Per particle: (ll_ref, terms, vc_ref, e_oracle_ll, e_oracle_vc)."""
        keys = [r.tobytes() for r in states]
        new = {}
        for k, r in zip(keys, states):
            if k not in self.cache:
                new[k] = r
        if new:
            xs = np.ascontiguousarray(np.stack(list(new.values())))
            mu_r, vc_r = self.ref.obs_map(xs, self.tau)
            ll_r, terms = E.loglik_from_map(mu_r, vc_r[:, None] * self.ref.lam_y[None, :], self.z, dtype=LD)
            mu_o, vc_o = E.oracle_obs_inverse(self.om, xs, self.tau)
            ll_o, _ = E.loglik_from_map(mu_o, vc_o[:, None] * self.lam[None, :], self.z)
            e_ll = (np.abs(ld(ll_o) - ll_r) / terms).astype(np.float64)
            e_vc = E.vc_error(vc_o, vc_r)
            for i, k in enumerate(new):
                self.cache[k] = (ll_r[i], terms[i], vc_r[i], e_ll[i], e_vc[i])
        rows = [self.cache[k] for k in keys]
        return (ld([r[0] for r in rows]), ld([r[1] for r in rows]), ld([r[2] for r in rows]),
                np.array([r[3] for r in rows]), np.array([r[4] for r in rows]))


def ref_of(sm):
    key = (sm.kind, sm.T, sm.d, sm.D)
    if key not in _REFS:
        _REFS[key] = Ref(sm)
    return _REFS[key]


# ---- one rank ---------------------------------------------------------------------------------------
def one_pass(R, pf, states0, normals, draws):
    """load -> one replayed update -> (propagated states, vc, ll, stats) in particle order."""
    P = states0.shape[0]
    pf.load_state(states0, np.zeros(P, dtype=np.int64))
    pf.obs_cutoff_stats(reset=True)
    pf.update_with_draws(R.z, draws[0], normals, draws[1])
    inn = pf.innovation(particles=True)
    st = pf.export_state()
    stats = pf.obs_cutoff_stats()
    states1 = inn.states.numpy().copy()
    assert np.array_equal(st["states"], states1[st["resample_idx"]])          # particle order
    assert all(v == 0 for v in pf.health().values()), pf.health()
    return states1, inn.variance_common.numpy().copy(), st["ll"].copy(), stats


def make_filter(R, P, split):
    from gpmdm_amd import GPMDM_PF
    pf = GPMDM_PF(R.m, torch.tensor([[1.0]]), P, rng="torch", obs_cutoff=True, predictive=True)
    pf.set_obs_cutoff(True, stats=True, split=split)
    return pf


def steer(R, targets, split="none", seed=0):
    """The three passes.  Returns a dict: the normals that land the cloud on the targets, and the
    final pass's states, vc, ll and stats."""
    P, d = targets.shape
    rng = np.random.RandomState(100 + seed)
    draws = (rng.exponential(size=(P, 1)), rng.rand(P))
    pf = make_filter(R, P, split)
    X_mu = one_pass(R, pf, targets, np.zeros((P, d)), draws)[0]
    X_one = one_pass(R, pf, targets, np.ones((P, d)), draws)[0]
    s = X_one - X_mu
    assert np.all(s > 0)
    normals = (targets - X_mu) / s
    states, vc, ll, stats = one_pass(R, pf, targets, normals, draws)
    err = np.max(np.abs(states - targets) / R.sm.ls[None, :])
    assert err <= STEER_TOL, err
    return dict(normals=normals, draws=draws, states=states, vc=vc, ll=ll, stats=stats)


def check_lists(R, states, stats, what, begin=0, end=None):
    """(b), and the decisiveness of the host model at the states read back."""
    lists = R.lm.tiles(states, begin, states.shape[0] if end is None else end)
    margin = min(t.margin for t in lists)
    assert margin >= L.MIN_MARGIN, (what, margin)
    run, dense = R.lm.stats(lists)
    assert (stats["run"], stats["dense"]) == (run, dense), (what, stats, run, dense, [t.n_act for t in lists])
    return lists


def tile_class(t):
    return "far" if t.n_act == 0 else f"{t.n_chunks} chunk" + ("s" if t.n_chunks > 1 else "")


def check_accuracy(R, name, lists, states, ll, vc, begin=0):
    """(a), per list-length class."""
    PT = R.lm.PT
    n = states.shape[0]
    ll_r, terms, vc_r, o_ll, o_vc = R.evaluate(states)
    e_ll = (np.abs(ld(ll) - ll_r) / terms).astype(np.float64)
    e_vc = E.vc_error(vc, vc_r)
    cls = np.array([tile_class(lists[i // PT]) for i in range(n)])
    for c in sorted(set(cls)):
        sel = cls == c
        held("ll", f"{name} | {c}", e_ll[sel], o_ll[sel])
        held("vc", f"{name} | {c}", e_vc[sel], o_vc[sel])
    if (cls == "far").any():
        assert np.all(vc[cls == "far"] == 1.0), (name, "vc in a far tile")


def baseline(name):
    """A case steered under split="none", with (a) and (b) checked once."""
    if name not in _RUNS:
        sm, targets, want = L.case_targets(name)
        R = ref_of(sm)
        t0 = time.time()
        run = steer(R, targets)
        TIMES.setdefault("steer_three_passes_ms", {})[name] = round(1e3 * (time.time() - t0), 1)
        lists = check_lists(R, run["states"], run["stats"], name)
        if want is not None:
            assert [t.n_act for t in lists] == list(want), name
        run.update(R=R, targets=targets, lists=lists)
        _RUNS[name] = run
    return _RUNS[name]


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_scripted_lists_per_particle_and_exact_stats(name):
    """(a) and (b) on every case: T = 66 at d = 1, 3 (coordinates in VGPRs), 5 (in LDS) and 9 (the
    8-wave 64-particle tile) with P = 8 PT + 5 (a ragged last tile); one tile per list length at
    T_M = 1 and at T_M = 2 (D = 20: a second mean tile with 4 real columns); T = 125 at P = 1056 and
    2080 (lists of up to four chunks, two window refills, the multi-kernel finish); the d = 2 grid,
    whose lists have index gaps."""
    run = baseline(name)
    R = run["R"]
    check_accuracy(R, name, run["lists"], run["states"], run["ll"], run["vc"])


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_split_policies_bitwise_per_particle(name):
    """(c), schedules: the same states under tail, all, chunks and auto give each particle's ll and
    vc bit for bit, and the same exact statistics (two workgroups per tile chained by the
    likelihood finish; one workgroup per chunk, some finding none)."""
    run = baseline(name)
    R, P = run["R"], run["targets"].shape[0]
    for split in SPLITS:
        pf = make_filter(R, P, split)
        states, vc, ll, stats = one_pass(R, pf, run["targets"], run["normals"], run["draws"])
        assert np.array_equal(states, run["states"]), (name, split)
        check_lists(R, states, stats, f"{name} {split}")
        for key, got in (("ll", ll), ("vc", vc)):
            bad = np.nonzero(got != run[key])[0]
            assert bad.size == 0, (name, split, key, bad.size, bad[:8], [run["lists"][i // R.lm.PT].n_act for i in bad[:8]])


@pytest.mark.parametrize("split", ["none", "all"])
@pytest.mark.parametrize("name", ["lists66", "sweep d=9", "tm2"])
def test_tile_compositions_bitwise_per_particle(name, split):
    """(c), compositions: the same targets permuted, so that every tile mixes distant clusters and
    runs dozens of active K-steps that are flushed for each single particle.  Particles whose
    state read back is bit-identical to their twin's in the compact tiles (at least 90 %) must have
    the twin's ll and vc bit for bit -- obs_cutoff.h's invariance --; (a) and (b) hold as well."""
    run = baseline(name)
    R = run["R"]
    targets, order = L.mixed(run["targets"])
    mix = steer(R, targets, split=split, seed=1)
    lists = check_lists(R, mix["states"], mix["stats"], f"{name} mixed {split}")
    assert min(t.n_act for t in lists) >= 35
    same = np.all(mix["states"] == run["states"][order], axis=1)
    assert same.mean() >= 0.9, same.mean()
    for key in ("ll", "vc"):
        bad = np.nonzero(same & (mix[key] != run[key][order]))[0]
        assert bad.size == 0, (name, split, key, bad.size, bad[:8])
    check_accuracy(R, f"{name} mixed", lists, mix["states"], mix["ll"], mix["vc"])


# ---- two logical shards -----------------------------------------------------------------------------
def shard_pass(R, P, shard, states0, normals, draws, split):
    """One replayed frame of a logical shard, the test playing the exchange (as
    test_gpu_switch_group.py's Staged): the slice's propagated states, ll and the statistics."""
    from gpmdm_amd import GPMDM_PF, _lib
    import switch_group_ref as G
    d = R.sm.d
    lo, hi = G.shard_bounds(P, *shard)
    pf = GPMDM_PF(R.m, torch.tensor([[1.0]]), P, rng="torch", obs_cutoff=True, shard=shard,
                  exchange=lambda recv, send: None)
    pf.set_obs_cutoff(True, stats=True, split=split)
    pf.load_state(states0, np.zeros(P, dtype=np.int64))
    pf.obs_cutoff_stats(reset=True)
    lib, h, s = _lib.load(), pf._h, pf._stream()
    dev = torch.device("cuda:0")
    send_s = torch.zeros((hi - lo, d + 1), dtype=torch.float64, device=dev)
    send_l = torch.zeros((hi - lo, 1), dtype=torch.float64, device=dev)
    recv_s = torch.zeros((P, d + 1), dtype=torch.float64, device=dev)
    recv_l = torch.zeros((P, 1), dtype=torch.float64, device=dev)
    Ed = np.ascontiguousarray(draws[0])
    nrm = np.ascontiguousarray(normals)
    u = np.ascontiguousarray(draws[1])
    _lib.check(lib.gpmdm_pf_switch(h, _lib.dptr(Ed), None, s), "switch")
    _lib.check(lib.gpmdm_pf_propagate_dynamics(h, _lib.dptr(nrm), s), "propagate_dynamics")
    _lib.check(lib.gpmdm_pf_pack_part(h, send_s.data_ptr(), _lib.GPMDM_PACK_STATES, s), "pack")
    _lib.check(lib.gpmdm_pf_weigh(h, _lib.dptr(R.z), s), "weigh")
    _lib.check(lib.gpmdm_pf_pack_part(h, send_l.data_ptr(), _lib.GPMDM_PACK_LL, s), "pack")
    recv_s[lo:hi].copy_(send_s)
    recv_l[lo:hi].copy_(send_l)
    _lib.check(lib.gpmdm_pf_unpack_part(h, recv_s.data_ptr(), _lib.GPMDM_PACK_STATES, s), "unpack")
    _lib.check(lib.gpmdm_pf_unpack_part(h, recv_l.data_ptr(), _lib.GPMDM_PACK_LL, s), "unpack")
    _lib.check(lib.gpmdm_pf_resample(h, _lib.dptr(u), s), "resample")
    pf._readout = None
    states = send_s.cpu().numpy()[:, 1:].copy()
    ll = send_l.cpu().numpy()[:, 0].copy()
    stats = pf.obs_cutoff_stats()
    assert all(v == 0 for v in pf.health().values()), pf.health()
    return lo, hi, states, ll, stats


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("name", ["lists66", "sweep d=9"])
def test_two_logical_shards_bitwise_per_particle(name, rank):
    """(c), shards: shard (2, r) evaluates its slice in tiles that start at the slice's first
    particle, so every tile boundary of rank 1 moves (P is odd) and tiles straddle two scripted
    lists.  The slice lands where the one-rank run landed (same normals; at least 90 % of the
    states bit-identical), and those particles' ll is the one-rank ll bit for bit; (b) holds on the
    slice's own tiles, under none and all."""
    run = baseline(name)
    R, P = run["R"], run["targets"].shape[0]
    for split in ("none", "all"):
        lo, hi, states, ll, stats = shard_pass(R, P, (2, rank), run["targets"], run["normals"], run["draws"], split)
        full = run["states"].copy()
        full[lo:hi] = states
        check_lists(R, full, stats, f"{name} shard {rank} {split}", lo, hi)
        same = np.all(states == run["states"][lo:hi], axis=1)
        assert same.mean() >= 0.9, same.mean()
        bad = np.nonzero(same & (ll != run["ll"][lo:hi]))[0]
        assert bad.size == 0, (name, rank, split, bad.size, bad[:8] + lo)


# ---- a masked bank: the LROWS instantiation -----------------------------------------------------------
def test_masked_bank_rows_per_particle():
    """Two filters with different observation masks on the T = 66, d = 3 chain (the kernel's LROWS
    instantiation: lam2 read per particle's filter, tiles that straddle the two filters).  Banks
    draw by Philox, so the cloud cannot be steered: both filters start on the scripted targets and
    land where the dynamics GP sends them (along the chain; the lists are whatever the host model
    says for the states read back, decisive or the test says so).  Each row is bitwise the single
    masked filter's, the statistics are exact, and each row's ll (on its observed joints only) and
    vc meet (a)."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    from oracle import gpmdm_oracle as O
    import ctypes
    sm, targets, _ = L.case_targets("lists66")
    R = ref_of(sm)
    F, P, seed = 2, targets.shape[0], 900
    obs = np.ones((F, sm.D), dtype=bool)
    obs[0, [1, 4]] = False
    obs[1, [0, 2, 3, 5]] = False
    Z = np.stack([sm.p["Y"][17], sm.p["Y"][40]])
    T = torch.tensor([[1.0]])
    states0, cls0 = np.stack([targets] * F), np.zeros((F, P), dtype=np.int64)
    bank = GPMDM_PF_Bank(R.m, T, F, P, seed=seed, obs_cutoff=True, predictive=True)
    lib = _lib.load()
    _lib.check(lib.gpmdm_pf_set_obs_cutoff(bank._h, 2), "stats")
    bank.load_state(states0, cls0)
    run, dense = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.gpmdm_pf_obs_cutoff_stats(bank._h, ctypes.byref(run), ctypes.byref(dense), 1, bank._stream()), "stats")
    bank.update(Z, observed=obs)
    inn = bank.innovation(particles=True)
    _lib.check(lib.gpmdm_pf_obs_cutoff_stats(bank._h, ctypes.byref(run), ctypes.byref(dense), 1, bank._stream()), "stats")
    st = bank.export_state()
    states, vc = inn.states.numpy(), inn.variance_common.numpy()
    assert bank.health() == {k: 0 for k in bank.health()}
    # (b): the tiles run over the bank's F P particles in order (C = 1: the grouping is the identity)
    lists = check_lists(R, states.reshape(F * P, sm.d), {"run": run.value, "dense": dense.value}, "masked bank")
    for f in range(F):
        pf = GPMDM_PF(R.m, T, P, rng="philox", seed=seed + f, obs_cutoff=True, predictive=True)
        pf.load_state(states0[f], cls0[f])
        pf.update(Z[f], observed=obs[f])
        s1, i1 = pf.export_state(), pf.innovation(particles=True)
        assert np.array_equal(i1.states.numpy(), states[f]), f
        assert np.array_equal(s1["ll"], st["ll"][f]), f
        assert np.array_equal(i1.variance_common.numpy(), vc[f]), f
        # (a) on the observed joints: the reference and the oracle restricted to them
        o = obs[f]
        mu_r, vc_r = R.ref.obs_map(states[f], R.tau)
        ll_r, terms = E.loglik_from_map(mu_r[:, o], vc_r[:, None] * R.ref.lam_y[None, o], Z[f][o], dtype=LD)
        mu_o, vc_o = E.oracle_obs_inverse(R.om, states[f], R.tau)
        ll_o, _ = E.loglik_from_map(mu_o[:, o], vc_o[:, None] * R.lam[None, o], Z[f][o])
        assert O.loglik_const(int(o.sum())) != O.loglik_const(sm.D)
        held("ll", f"masked bank row {f} (D_obs = {int(o.sum())})", (np.abs(ld(st["ll"][f]) - ll_r) / terms).astype(np.float64),
             (np.abs(ld(ll_o) - ll_r) / terms).astype(np.float64))
        held("vc", f"masked bank row {f} (D_obs = {int(o.sum())})", E.vc_error(vc[f], vc_r), E.vc_error(vc_o, vc_r))
    assert len({t.n_chunks for t in lists}) >= 2
