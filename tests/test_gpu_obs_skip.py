"""The dense observation tile's flush and block skip (gp_tile.h; DESIGN.md §3.4 "Flush and skip
in the dense tile").

The filters' likelihood replaces every kernel value below the model's tau by exactly 0, value
by value, and the K loop branches around the MFMAs of every 16-particle x 4-row block of kernel
values that is exactly zero.  What is held here:

* skip on = skip off, bit for bit (``set_obs_skip``: the same kernel runs every block);
* a particle's ll does not depend on its tile-mates or its position;
* the filter flushes and the predictive maps do not;
* the flushed filter's per-particle ll against the extended-precision reference evaluated with
  the same tau, the yardstick an fp64 oracle in the device's association (|R^T k|^2 on the
  flushed values), with tests/test_gpu_gp_accuracy.py's MARGIN and floor.

Clouds are placed through a replayed step: every particle starts at one training latent in one
class, so the propagated state is mean + sqrt(var) * normal with the same mean and variance for
all of them, and the normals (replay draws are the caller's) put each particle where the test
wants it.  The propagated states the device reports are what every assertion is made on.
"""
import functools

import numpy as np
import pytest
import torch

import extended_ref as E
import obs_flush_ref as F
import test_gpu_gp_accuracy as A
from extended_ref import ld

pytestmark = pytest.mark.gpu


def replay_step(m, C, states0, cls0, Ed, nrm, u, z, skip=True):
    """One replayed step (switch, propagate, pack, resample) of a fresh filter over the given
    particles and draws: the packed {ll, class, state} rows, the exported state and the
    read-outs."""
    from gpmdm_amd import GPMDM_PF, _lib, synthetic
    P, d = states0.shape
    pf = GPMDM_PF(m, torch.tensor(synthetic.markov_matrix(C)), P, rng="torch")
    pf.set_obs_skip(skip)
    pf.load_state(np.ascontiguousarray(states0), np.ascontiguousarray(cls0, dtype=np.int64))
    lib, h, s = _lib.load(), pf._h, pf._stream()
    pf._sync_model()
    rows = torch.empty((P, d + 2), dtype=torch.float64, device=m.device)
    Ed, nrm, u, z = (np.ascontiguousarray(a, dtype=np.float64) for a in (Ed, nrm, u, z))
    _lib.check(lib.gpmdm_pf_switch(h, _lib.dptr(Ed), None, s), "switch")
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), _lib.dptr(nrm), s), "propagate")
    _lib.check(lib.gpmdm_pf_pack(h, rows.data_ptr(), s), "pack")
    _lib.check(lib.gpmdm_pf_resample(h, _lib.dptr(u), s), "resample")
    rows = rows.cpu().numpy()
    pf._readout = None
    out = dict(rows=rows, ll=rows[:, 0].copy(), states1=np.ascontiguousarray(rows[:, 2:]), st=pf.export_state(),
               post=pf.class_probabilities().numpy(), mean=pf.current_state_mean().numpy(), lik=pf.log_likelihood())
    assert all(v == 0 for v in pf.health().values())
    return out


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def same_step(on, off, what):
    same_bits(on["rows"], off["rows"], (what, "packed rows (ll, class, state)"))
    for k in ("ll", "log_w", "w", "resample_idx", "states", "classes"):
        same_bits(on["st"][k], off["st"][k], (what, k))
    same_bits(on["post"], off["post"], (what, "class probabilities"))
    same_bits(on["mean"], off["mean"], (what, "state mean"))
    assert np.float64(on["lik"]).tobytes() == np.float64(off["lik"]).tobytes(), (what, "likelihood read-out")


@functools.lru_cache(maxsize=None)
def big_cutoff_model(d):
    """The accuracy tests' "cutoff" recipe past one column block: N = 540 (two 512-column blocks,
    tile retirement and the generate-only tail all run)."""
    from gpmdm_amd import GPMDM
    p = E.recipe_model(d, L=90, x_scale=3.0, ls_range=(0.4, 0.6))
    return p, GPMDM.from_arrays(p["X"], E.y_sequences(p), **E.hyper(p))


# ----------------------------------------------------------------------------
# the threshold a model reports
# ----------------------------------------------------------------------------

def test_python_built_model_reports_obs_cutoff_tau():
    """gpmdm_model_set_obs_flush's tau = host_image.h obs_cutoff_tau restated in numpy on the
    model's own K_y^-1 Y (beta from a fresh solve here, the library's from the precompute: the mean
    bound moves with |beta_j|_1 at the 1e-9 level, as in test_gpu_obs_cutoff.test_tau_is_the_bound)."""
    p, m = big_cutoff_model(3)
    om = E.oracle_of(p)
    sigma2 = float(np.exp(p["y_log_sigma_n"])) ** 2
    want = F.tau_numpy(p["X"].shape[0], sigma2, om.Ky_inv @ om.Y, np.max(np.abs(p["Y"]), axis=0))
    got = m.obs_flush_tau
    assert got > 0.0 and abs(got - want) <= 1e-6 * want, (got, want)


def test_model_without_the_call_reports_no_flush(monkeypatch):
    from gpmdm_amd import GPMDM
    monkeypatch.setattr(GPMDM, "_install_obs_flush", lambda self: None)
    p = E.recipe_model(3)
    m = GPMDM.from_arrays(p["X"], E.y_sequences(p), **E.hyper(p))
    assert m.obs_flush_tau == 0.0


# ----------------------------------------------------------------------------
# skip on = skip off
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("d", [3, 13])
def test_skip_on_equals_off_replayed_step(d, order):
    """Case A: N = 540, P = 777 (a partial last tile), the five regimes' copies sorted along the
    first axis or not, one replayed step with the branch and without it."""
    p, m = big_cutoff_model(d)
    assert 0.0 < m.obs_flush_tau < 1e-15
    xs, _ = E.regime_points(p)
    P, C = 777, len(p["seq_lengths"])
    idx = A.copies(P, 5)
    if order == "sorted":
        idx = idx[np.argsort(xs[idx, 0], kind="stable")]
    rng = np.random.RandomState(31 + d)
    args = (xs[idx], rng.randint(0, C, P), rng.exponential(size=(P, C)), rng.randn(P, d), rng.rand(P), p["Y"][17])
    on, off = replay_step(m, C, *args, skip=True), replay_step(m, C, *args, skip=False)
    assert np.all(np.isfinite(on["ll"]))
    same_step(on, off, (d, order))


def test_skip_on_equals_off_flagship_shape(fx_config2):
    """Case B: the config-2 fixture model (N = 2000, d = 3, D = 62: the benchmark's shape, four
    column blocks), P = 2048, three Philox frames after one warm-up frame on Y[10]."""
    from conftest import product_model
    from gpmdm_amd import GPMDM_PF
    m = product_model(fx_config2)
    assert 0.0 < m.obs_flush_tau < 1e-15
    T = torch.tensor(np.asarray(fx_config2["T"], dtype=np.float64))
    Y = m.get_Y()
    # the initial particles are drawn from torch's global generator, so the two filters start
    # from one exported state: the first filter's after the warm-up frame
    warm = GPMDM_PF(m, T, 2048, rng="philox", seed=11)
    warm.update(Y[10])
    st = warm.export_state()
    pfs = []
    for skip in (True, False):
        pf = GPMDM_PF(m, T, 2048, rng="philox", seed=11)
        pf.set_obs_skip(skip)
        pf.import_state(st)
        pfs.append(pf)
    for k in range(3):
        outs = []
        for pf in pfs:
            pf.update(Y[11 + k] + 0.01)
            outs.append(dict(rows=pf.export_state()["ll"], st=pf.export_state(), post=pf.class_probabilities().numpy(),
                             mean=pf.current_state_mean().numpy(), lik=pf.log_likelihood()))
        same_step(outs[0], outs[1], ("config 2", k))


# ----------------------------------------------------------------------------
# placed clouds
# ----------------------------------------------------------------------------

def placed_step(p, m, targets, skip=True):
    """A replayed step whose propagated states are ``targets`` to rounding: every particle starts
    at X[0] in class 0 and stays there (exponential draws 1e-9 for class 0, 1 for the rest), and
    its normal is (target - mean) / sqrt(var) of class 0's dynamics GP at X[0] (fp64 oracle)."""
    om = E.oracle_of(p)
    P, d = targets.shape
    C = len(p["seq_lengths"])
    x0 = np.repeat(p["X"][:1], P, axis=0)
    mu, var = om.map_x_dynamics_for_class(x0[:1], 0)
    nrm = (targets - mu) / np.sqrt(var)
    Ed = np.ones((P, C))
    Ed[:, 0] = 1e-9
    out = replay_step(m, C, x0, np.zeros(P, dtype=np.int64), Ed, nrm, np.linspace(0.0005, 0.9995, P), p["Y"][17],
                      skip=skip)
    assert np.array_equal(out["rows"][:, 1], np.zeros(P))
    assert np.max(np.abs(out["states1"] - targets)) <= 1e-6 * (1.0 + np.max(np.abs(targets)))
    return out, nrm


def test_ll_does_not_depend_on_tile_mates():
    """The same 64 propagated states in two clouds of 777: once in a run of positions among near
    neighbours (copies displaced by 1e-3 l), once on the odd positions of a stretch whose even
    positions hold the underflow regime, the rest of both clouds other points.  Their states must
    arrive bit for bit the same (same start, same normals) and so must their ll.  The 64 are
    "far" points of the recipe: each has kernel values on both sides of tau."""
    d = 3
    p, m = big_cutoff_model(d)
    xs, reg = E.regime_points(p)
    ell = np.exp(p["y_log_lengthscales"])
    rng = np.random.RandomState(8)
    far, under = xs[reg == 3], xs[reg == 4]
    S = far[rng.randint(0, far.shape[0], 64)] + 0.05 * ell * rng.randn(64, d)
    P = 777
    fill = xs[A.copies(P, 9)]
    a, b = fill.copy(), fill.copy()
    pos_a = 200 + np.arange(64)                        # four whole 16-particle row blocks
    a[136:200] = S + 1e-3 * ell * rng.randn(64, d)     # near neighbours before ...
    a[264:328] = S + 1e-3 * ell * rng.randn(64, d)     # ... and after
    a[pos_a] = S
    pos_b = 301 + 2 * np.arange(64)                    # odd positions, across tiles
    b[300:300 + 128:2] = under[rng.randint(0, under.shape[0], 64)]
    b[pos_b] = S
    (oa, na), (ob, nb) = placed_step(p, m, a), placed_step(p, m, b)
    same_bits(na[pos_a], nb[pos_b], "the normals of the 64")
    same_bits(oa["states1"][pos_a], ob["states1"][pos_b], "the propagated states of the 64")
    k = F.kernel_values(p, oa["states1"][pos_a])
    tau = m.obs_flush_tau
    part = np.any((k > 0) & (k < tau), axis=0) & np.any(k >= tau, axis=0)
    assert part.sum() >= 32, part.sum()
    same_bits(oa["ll"][pos_a], ob["ll"][pos_b], "ll of the same states among other tile-mates")


def test_filter_flushes_and_maps_do_not():
    """Particles 10 l from every training row (past tau's cutoff distance, far inside exp's
    range): the filter gives them, bit for bit, the ll of a particle whose kernel values all
    underflow; map_x_to_y at the same points returns their non-zero tiny means."""
    d = 3
    p, m = big_cutoff_model(d)
    ell = np.exp(p["y_log_lengthscales"])
    tau = m.obs_flush_tau
    P = 96
    rng = np.random.RandomState(4)
    # 10 l beyond the training row that is outermost on the first axis, along that axis: that row
    # is 10 l away and every other row at least as far
    ten = np.repeat(p["X"][np.argmax(p["X"][:, 0])][None, :], 64, axis=0)
    ten[:, 0] += 10.0 * ell[0] + 0.05 * ell[0] * rng.rand(64)
    ten[:, 1:] += 0.05 * ell[1:] * rng.randn(64, d - 1)
    gone = p["X"].max(0) + 60.0 * ell + ell * rng.rand(32, d)
    out, _ = placed_step(p, m, np.concatenate([ten, gone]))
    k = F.kernel_values(p, out["states1"])
    assert np.all(k[:, :64].max(axis=0) < tau) and np.all(k[:, :64].max(axis=0) > 1e-200)
    assert np.all(k[:, 64:] == 0.0)
    same_bits(out["ll"][:64], np.repeat(out["ll"][64:65], 64), "all values flushed = all values underflowed")
    same_bits(out["ll"][64:], np.repeat(out["ll"][64:65], 32), "the underflow regime")
    mu, var = (t.numpy() for t in m.map_x_to_y(torch.from_numpy(np.ascontiguousarray(out["states1"]))))
    assert np.all(np.max(np.abs(mu[:64]), axis=1) > 0.0) and np.all(np.max(np.abs(mu[:64]), axis=1) < 1e-20)
    assert np.all(mu[64:] == 0.0)


# ----------------------------------------------------------------------------
# the default filter against the reference with the same flush
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("d,P", [(1, 777), (3, 777), (4, 777), (8, 777), (9, 777), (16, 777),
                                 (1, 1500), (3, 1500), (4, 1500), (8, 1500), (9, 1500), (16, 1500), (3, 8300)])
def test_default_filter_ll_per_particle_with_flush(d, P):
    """Every particle of the default (dense) filter on the "cutoff" recipe (N = 330, spread
    latents, short length scales): |ll_gpu - ll_ref(tau)| / terms <= MARGIN max(oracle's worst,
    16 eps), the reference evaluated with the model's tau (values below it flushed before the
    solves), the oracle fp64 in the device's association (|R^T k|^2, k^T (R R^T Y)) on the same
    flushed values.  P = 777: the 16 x 256 image; 1500: 16-row tiles over 32 x 512; 8300: 32 x 512
    proper; d > 12: 64 x 512.  The cloud holds particles with some but not all values flushed."""
    c = A.case(d, "cutoff")
    m = c.model()
    tau = m.obs_flush_tau
    assert 0.0 < tau < 1e-15
    states1, ll, z, _ = A.filter_step(c, P, seed=70 + d)
    k0, kt = c.ref.obs_kernel(states1), c.ref.obs_kernel(states1, tau)
    flushed = (k0 != kt)
    some = flushed.any(axis=0) & (kt != 0).any(axis=0)          # some but not all values flushed
    assert some.any()
    ll_r, terms = c.ref.loglik(states1, z, tau)
    lam = np.exp(c.p["y_log_lambdas"]) ** -2
    mu_o, vc_o = F.oracle_obs_triangular_flushed(c.om, states1, tau)
    ll_o, _ = E.loglik_from_map(mu_o, vc_o[:, None] * lam[None, :], z)
    e_gpu = (np.abs(ld(ll) - ll_r) / terms).astype(np.float64)
    e_or = (np.abs(ld(ll_o) - ll_r) / terms).astype(np.float64)
    yard = max(float(np.max(e_or)), A.FLOOR)
    print(f"d={d} P={P}: {int(some.sum())} particles partly flushed, device {np.max(e_gpu):.3e}, yardstick {yard:.3e}, ratio {np.max(e_gpu) / yard:.2f}")
    assert np.max(e_gpu) <= A.MARGIN * yard, (d, P, float(np.max(e_gpu)), yard)
