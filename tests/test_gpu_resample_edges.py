"""Scripted-weight tests of the normaliser, the CDF, the inverse-CDF searches, the scan-form
systematic resampler and the read-out (csrc/pf_kernels.hip: k_norm_*, k_rows_ll, CdfView,
k_guide, k_sys_*, k_resample, k_readout and their one-workgroup twin k_small_resample) against
tests/resample_ref.py.

How the inputs are scripted: a sharded filter with a caller-driven exchange
(``shard=(2, 0), exchange=fn``) takes its pre-resample {class, state} rows and its ll column
from the buffer ``fn`` fills, so ``fn`` overwrites all P rows with the scripted ones (copies on
the current stream, the one the library's kernels are ordered on).  With rng='torch' there is
no ownership reorder, and ``update_with_draws`` supplies the uniforms.  P <= 1024 runs
flush_rows + k_small_resample, P > 1024 k_rows_ll + the multi-kernel path with the rows read in
place, P >= 262144 adds k_guide.  The observation and the propagated cloud are irrelevant.

Part 1 (exact): ll in {c, -inf}.  Every sum is a small integer, so the CDF is one correctly
rounded division in any association and the ancestors must equal np.searchsorted(cum, u,
"left") with no mismatch allowed; gathers, log_w, w, the posterior and the likelihood read-out
are compared bitwise.  u = 0 with leading zero weights selects particle 0, as torch's search
does (cum[0] = 0 >= u); every other slot must have an ancestor of nonzero weight, including
u = 1 - 2^-53 with trailing zeros, which lands on the last nonzero particle and not on the
forced last bucket.

Part 2 (banded): general weights; ancestor i of uniform u is accepted iff
C[i-1] - tol <= u <= C[i] + tol on the extended-precision CDF C, tol = (P + 8) 2^-53 (derived
in resample_ref, not measured), with monotonicity, offspring counts and the read-outs held to
the same tol.  Multinomial filters run each pattern twice: with random uniforms, which never
come within tol of a CDF value, and with uniforms placed on the reference CDF's fp64 values
(every 256-block boundary among them) and their neighbours, where the evaluated CDF's ulp-sized
dips (CdfView) could send the search forms different ways.  The worst fraction of each bound used goes to resample_edges.json in the
directory GPMDM_ACCURACY_OUT names (default test_out/, git-ignored); a run's file is committed
as profiles/resample_edges/summary.json.

Part 3 (one rank and banks, exact): a blacked-out frame gives ll = 0 and w = 1/P exactly,
through the single-rank maximum path (k_obs_ll block maxima, deferred finish) and the bank
layout (blockIdx.y = f, k_norm_max atomics), which cannot take scripted ll.
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import resample_ref as R
from conftest import ROOT, synthetic_model
from oracle import gpmdm_oracle as O
from oracle import philox

pytestmark = pytest.mark.gpu

C, D_LAT, D_OBS = 3, 2, 5
MODES = ("multinomial", "systematic")
USED = {}                                # "P<P>_<mode>" -> {bound: [worst fraction used, pattern]}


@pytest.fixture(scope="module")
def model():
    return synthetic_model(C=C, d=D_LAT, D=D_OBS, L=10, S=3)        # N = 90


@pytest.fixture(scope="module", autouse=True)
def band_log():
    yield
    if USED:
        out = Path(os.environ.get("GPMDM_ACCURACY_OUT") or ROOT / "test_out")
        out.mkdir(parents=True, exist_ok=True)
        (out / "resample_edges.json").write_text(json.dumps(
            {"tol": "(P + 8) * 2^-53", "note": "worst fraction of each bound used over the banded patterns "
             "(cdf_band, w, posterior, likelihood: of tol; offspring: of P tol; mean: of tol sum|x|w)",
             "used": USED}, indent=1, sort_keys=True))


class Scripted:
    """One sharded filter whose exchange hands it the scripted rows and ll column."""

    def __init__(self, model, P, mode, seed=0):
        from gpmdm_amd import GPMDM_PF
        m, T, Y = model
        self.P, self.mode = P, mode
        self.rng = np.random.RandomState(1000 * seed + P % 997)
        dev = torch.device("cuda:0")
        self.rows = torch.zeros((P, D_LAT + 1), dtype=torch.float64, device=dev)
        self.llcol = torch.zeros((P, 1), dtype=torch.float64, device=dev)
        # (P = 1: rank 0 of 2 owns no particle, rank 1 owns it; every rank resamples all P rows)
        self.pf = GPMDM_PF(m, T, P, rng="torch", shard=(2, 0 if P > 1 else 1), exchange=self._fill, resample=mode)
        self.z = np.ascontiguousarray(Y[3], dtype=np.float64)
        self.E = self.rng.exponential(size=(P, C))
        self.nrm = self.rng.randn(P, D_LAT)
        self.calls = 0

    def _fill(self, recv, send):
        src = self.rows if recv.shape[1] > 1 else self.llcol
        assert recv.shape == src.shape
        recv.copy_(src)                  # current stream: ordered before unpack / resample
        self.calls += 1

    def particles(self, X, cls):
        self.X, self.cls = X, cls
        rows = np.concatenate([cls[:, None].astype(np.float64), X], axis=1)
        self.rows.copy_(torch.from_numpy(np.ascontiguousarray(rows)))

    def frame(self, ll, u):
        self.llcol.copy_(torch.from_numpy(np.ascontiguousarray(ll[:, None])))
        n0 = self.calls
        self.pf.update_with_draws(self.z, self.E, self.nrm, np.atleast_1d(np.asarray(u, dtype=np.float64)))
        assert self.calls == n0 + 2, "the exchange must be asked for the rows and for the ll column"
        st = self.pf.export_state()
        return st, self.pf.class_probabilities().numpy(), self.pf.current_state_mean().numpy(), self.pf.log_likelihood()


# ---- Part 1: exact ------------------------------------------------------------------------------
def _check_exact(s, name, mask, cum, c, ll, u_slots, u_arg):
    what = (s.P, s.mode, name, c, float(np.asarray(u_arg).reshape(-1)[0]))
    st, post, mean, lik = s.frame(ll, u_arg)
    idx = st["resample_idx"]
    want = np.searchsorted(cum, u_slots, side="left")
    bad = np.nonzero(idx != want)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], idx[bad[:5]], want[bad[:5]], u_slots[bad[:5]])
    assert np.array_equal(idx[u_slots == 0.0], np.zeros(int(np.sum(u_slots == 0.0)), dtype=np.int64)), what
    assert np.all(mask[idx[u_slots > 0.0]]), (what, "an ancestor of weight zero")
    assert np.array_equal(st["ll"], ll), what
    assert np.array_equal(st["states"], s.X[idx]), what
    assert np.array_equal(st["classes"], s.cls[idx]), what
    assert np.array_equal(st["log_w"], ll - c), what
    S = float(mask.sum())
    assert np.array_equal(st["w"], mask.astype(np.float64) / S), what
    # read-outs: post-resample class at slot s weighted by the pre-resample e2 in {0, 1} at slot s
    cl = np.array([float(np.sum(mask & (s.cls[idx] == k))) for k in range(C)])
    assert np.array_equal(post, cl / cl.sum()), (what, post, cl)
    assert lik == S, (what, lik, S)
    wv = mask.astype(np.float64) / S
    ref_mean = np.sum(s.X[idx].astype(R.LD) * wv[:, None].astype(R.LD), axis=0)
    scale = np.sum(np.abs(s.X[idx]) * wv[:, None], axis=0)
    assert np.all(np.abs(mean.astype(R.LD) - ref_mean) <= R.band_tol(s.P) * scale), (what, mean, ref_mean)


def _run_exact(model, P, mode, large=False):
    s = Scripted(model, P, mode)
    s.particles(*R.scripted_particles(P, C, D_LAT, s.rng))
    slots = np.arange(P)
    for name, mask in R.exact_patterns(P, large=large):
        cum = R.exact_cdf(mask)
        for c in R.EXACT_C:
            ll = R.exact_ll(mask, c)
            if mode == "multinomial":
                for u in R.edge_uniforms(cum, P, s.rng):
                    _check_exact(s, name, mask, cum, c, ll, u, u)
            else:
                for u0 in R.SYS_U0:
                    _check_exact(s, name, mask, cum, c, ll, R.sys_u(slots, u0, P), [u0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", R.SMALL_P)
def test_exact_small_path(model, P, mode):
    _run_exact(model, P, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", R.MULTI_P)
def test_exact_multi_kernel_path(model, P, mode):
    _run_exact(model, P, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", R.GUIDE_P)
def test_exact_guide_table(model, P, mode):
    """262143: the plain search's last size; 262144: the guide table's first; 300001: also
    k_norm_total's chunk = 2 (more than 1024 blocks)."""
    _run_exact(model, P, mode, large=True)


# ---- Part 2: banded -----------------------------------------------------------------------------
def _note(key, bound, frac, name):
    cur = USED.setdefault(key, {})
    if bound not in cur or frac > cur[bound][0]:
        cur[bound] = [float(frac), name]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", R.BANDED_P)
def test_banded(model, P, mode):
    s = Scripted(model, P, mode, seed=1)
    tol = R.band_tol(P)
    key = f"P{P}_{mode}"
    fails = []
    for name in R.BANDED:
        rng = s.rng
        X, cls = rng.randn(P, D_LAT), rng.randint(0, C, P).astype(np.int64)
        s.particles(X, cls)
        ll = R.banded_ll(name, P, rng)
        if mode == "multinomial":
            u_arg = u = rng.rand(P)
        else:
            u_arg = [rng.rand()]
            u = R.sys_u(np.arange(P), u_arg[0], P)
        st, post, mean, lik = s.frame(ll, u_arg)
        idx = st["resample_idx"]
        n = R.Normalised(ll)
        assert np.array_equal(st["ll"], ll), (key, name)
        assert idx.min() >= 0 and idx.max() < P, (key, name)
        assert np.array_equal(st["states"], X[idx]) and np.array_equal(st["classes"], cls[idx]), (key, name)
        rpost, rmean, rlik, scale = R.readouts(ll, cls, X, idx, C)
        fr = {
            "cdf_band": np.max(R.band_excess(n.cdf, u, idx)) / tol,
            "w": np.max(R.rel_excess(st["w"], n.w)) / tol,
            "posterior": np.max(R.rel_excess(post, rpost)) / tol,
            "likelihood": np.max(R.rel_excess(lik, rlik)) / tol,
            "mean": np.max(np.abs(mean.astype(R.LD) - rmean) / scale) / tol,
        }
        if mode == "systematic":
            fr["offspring"] = np.max(R.offspring_excess(n.w, idx)) / (P * tol)
            mono = bool(np.all(np.diff(idx) >= 0))
        else:
            mono = bool(np.all(np.diff(idx[np.argsort(u, kind="stable")]) >= 0))
        if mode == "multinomial":
            # a second frame whose uniforms sit on the CDF itself (every block boundary among
            # them, each value with its two fp64 neighbours): random uniforms never land within
            # tol of a CDF value, these all do, and they are where a CDF that dips by an ulp
            # across a block boundary could send two searches different ways
            u2 = R.near_tie_uniforms(n.cdf, P, rng)
            st2 = s.frame(ll, u2)[0]
            idx2 = st2["resample_idx"]
            assert idx2.min() >= 0 and idx2.max() < P, (key, name, "near ties")
            assert np.array_equal(st2["states"], X[idx2]) and np.array_equal(st2["classes"], cls[idx2]), (key, name)
            fr["cdf_band_near_ties"] = np.max(R.band_excess(n.cdf, u2, idx2)) / tol
            mono = mono and bool(np.all(np.diff(idx2[np.argsort(u2, kind="stable")]) >= 0))
        print(key, name, {k: float(v) for k, v in fr.items()}, "monotone", mono)
        for k, v in fr.items():
            _note(key, k, v, name)
            if not v <= 1.0:
                fails.append((name, k, float(v)))
        if not mono:
            fails.append((name, "monotone", 0.0))
    assert not fails, (key, fails)


def test_last_bucket_reaches_one(model):
    """u = 1 - 2^-53 on general weights.  The unforced last CDF value, (offset + local) / S, and
    S itself are two associations of one sum: in a host model of the device's summation order
    (resample_ref.device_association_cdf without its last line) the quotient falls below
    1 - 2^-53 in about one frame in nine at P = 5000 with ll = 5 randn, and the search would
    then run off the end of the cloud.  Only the forced last bucket prevents that; exact
    patterns cannot show it (their last value is S / S = 1 in any association), and one frame
    per banded pattern shows it only by luck.  64 frames, each with its own weights: every
    ancestor in range and inside the band, the slots that drew 1 - 2^-53 among them."""
    P, frames = 5000, 64
    s = Scripted(model, P, "multinomial", seed=2)
    rng = s.rng
    X, cls = rng.randn(P, D_LAT), rng.randint(0, C, P).astype(np.int64)
    s.particles(X, cls)
    tol = R.band_tol(P)
    for k in range(frames):
        ll = 5.0 * rng.randn(P)
        u = rng.rand(P)
        top = rng.choice(P, 4, replace=False)
        u[top[:2]] = R.U_MAX
        u[top[2:]] = np.nextafter(R.U_MAX, 0.0)
        st = s.frame(ll, u)[0]
        idx = st["resample_idx"]
        assert idx.min() >= 0 and idx.max() < P, (k, idx.max(), idx[top])
        n = R.Normalised(ll)
        assert np.max(R.band_excess(n.cdf, u, idx)) <= tol, k
        assert np.array_equal(st["states"], X[idx]) and np.array_equal(st["classes"], cls[idx]), k


# ---- Part 3: one rank and banks, blacked-out frames -----------------------------------------------
def _uniform_cdf(P):
    cum = np.arange(1, P + 1, dtype=np.float64) / np.float64(P)
    cum[-1] = 1.0
    return cum


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", [777, 1024, 1025, 1500])
def test_blackout_single_rank_exact(model, P, mode):
    from gpmdm_amd import GPMDM_PF
    m, T, Y = model
    rng = np.random.RandomState(P)
    pf = GPMDM_PF(m, T, P, rng="torch", resample=mode)
    cum = _uniform_cdf(P)
    if mode == "multinomial":
        draws = [(u, u) for u in R.edge_uniforms(cum, P, rng)]
    else:
        draws = [([u0], R.sys_u(np.arange(P), u0, P)) for u0 in R.SYS_U0]
    Tn = T.numpy()
    for u_arg, u in draws:
        pre = pf.export_state()
        E, nrm = rng.exponential(size=(P, C)), rng.randn(P, D_LAT)
        pf.update_with_draws(Y[3], E, nrm, np.asarray(u_arg, dtype=np.float64), observed=np.zeros(D_OBS, dtype=bool))
        st = pf.export_state()
        assert np.array_equal(st["ll"], np.zeros(P)) and np.array_equal(st["log_w"], np.zeros(P))
        assert np.array_equal(st["w"], np.full(P, 1.0 / P))
        assert np.array_equal(st["resample_idx"], np.searchsorted(cum, u, side="left")), (P, mode, u_arg[0])
        assert np.array_equal(st["classes"], O.switch_classes(pre["classes"], Tn, E)[st["resample_idx"]])
        assert pf.log_likelihood() == float(P)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Pf", [777, 1500])
def test_blackout_bank_exact(model, Pf, mode):
    """F = 3, filters 0 and 2 blacked out: their ancestors are exact; filter 1 (observed) passes
    the band check against its own exported ll."""
    from gpmdm_amd import GPMDM_PF_Bank
    m, T, Y = model
    F, seed = 3, 4242 + Pf
    bank = GPMDM_PF_Bank(m, T, F, Pf, seed=seed, resample=mode)
    observed = np.ones((F, D_OBS), dtype=bool)
    observed[0] = observed[2] = False
    cum = _uniform_cdf(Pf)
    Tn = T.numpy()
    tol = R.band_tol(Pf)
    for k in range(3):
        pre = bank.export_state()
        frame = bank.frame
        bank.update(np.stack([Y[5 + k]] * F), observed=observed)
        st = bank.export_state()
        for f in range(F):
            if mode == "multinomial":
                u = philox.resample_uniforms(seed, frame, Pf, f)
            else:
                u = R.sys_u(np.arange(Pf), philox.systematic_u0(seed, frame, f), Pf)
            idx = st["resample_idx"][f]
            if f == 1:
                n = R.Normalised(st["ll"][f])
                assert np.max(R.band_excess(n.cdf, u, idx)) <= tol, (Pf, mode, k)
                assert np.max(R.rel_excess(st["w"][f], n.w)) <= tol, (Pf, mode, k)
                continue
            assert np.array_equal(st["ll"][f], np.zeros(Pf)), (Pf, mode, k, f)
            assert np.array_equal(st["w"][f], np.full(Pf, 1.0 / Pf)), (Pf, mode, k, f)
            assert np.array_equal(idx, np.searchsorted(cum, u, side="left")), (Pf, mode, k, f)
            sw = O.switch_classes(pre["classes"][f], Tn, philox.switch_draws(seed, frame, Pf, C, f))
            assert np.array_equal(st["classes"][f], sw[idx]), (Pf, mode, k, f)
