"""GPU: fixed-lag smoothing for filter banks (``GPMDM_PF_Bank(smoothing_lag=...)``,
``set_smoothing``, ``smoothed``; gpmdm_bank_set_smoothing, gpmdm_bank_smoothed,
csrc/smooth.h).

Every filter of the bank is checked twice: against ``smooth_ref`` on the bank's own per-frame
exports with test_gpu_smoothing.py's ``_check`` (ancestors, classes, states and distinct counts
exact, fractions bitwise count / Pf, means within ``Pf 2^-53 mean |x|`` of the fsum mean), and
bitwise, ``state_mean`` included, against a single filter with the same lag given the same
updates -- blocks cut within the filter are the single filter's blocks.  The pose rows are
bitwise ``current_observation()`` of a bank loaded with the traced clouds.
"""
import numpy as np
import pytest
import torch

import test_gpu_smoothing as TS
from bank_rollout_common import KEYS, SHAPES, SM_FIELDS, bank_and_singles, export_row, frame_z, row, same, update_all
from conftest import product_model, synthetic_model

pytestmark = pytest.mark.gpu

ALL = ("lags", "frames") + SM_FIELDS


@pytest.fixture(scope="module")
def m1(fx_config1):
    return product_model(fx_config1)


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _model(request, cfg):
    return request.getfixturevalue("m1" if cfg == "config1" else "m2"), request.getfixturevalue("fx_" + cfg)


def _check_bank(s, hist, singles, C, frame, what, **kw):
    """Every filter's row of ``s`` (made with particles=True) against smooth_ref on the bank's
    exports ``hist`` and, bitwise, against the single filters' smoothed(**kw)."""
    F = s.class_probabilities.shape[0]
    assert all(getattr(s, k) is None or getattr(s, k).is_contiguous() for k in SM_FIELDS)
    for f in range(F):
        TS._check(row(s, f, SM_FIELDS), [export_row(h, f) for h in hist], C, frame, (what, f))
        if singles is not None:
            same(row(s, f, SM_FIELDS), singles[f].smoothed(**kw), ALL, (what, f))


def _check_pose(s, other, what):
    """Each lag's pose against current_observation() of ``other`` holding that lag's clouds."""
    for i in range(len(s.lags)):
        other.load_state(s.states[:, i].numpy(), s.classes[:, i].numpy())
        mean, spread = other.current_observation()
        assert np.array_equal(s.observation_mean[:, i].numpy(), mean.numpy()), (what, i)
        assert np.array_equal(s.observation_spread[:, i].numpy(), spread.numpy()), (what, i)


@pytest.mark.parametrize("L,frames", [(3, 6), (17, 20)])
@pytest.mark.parametrize("cfg,F,P,resample", SHAPES)
def test_against_the_reference_and_single_filters(request, cfg, F, P, resample, L, frames):
    """The ring wraps (frames > L + 1).  After frame 2 (depth below L) and after the last frame:
    every lag with pose and particles, a lag range, one lag, the bare call; twice in a row."""
    from gpmdm_amd import GPMDM_PF_Bank
    m, fx = _model(request, cfg)
    T = torch.tensor(fx["T"])
    bank, singles = bank_and_singles(m, T, F, P, resample, seed=500, smoothing_lag=L)
    other = GPMDM_PF_Bank(m, T, F, P, seed=1)
    C = bank.num_classes
    assert bank.smoothing_lag == L and bank.smoothing_depth == 0
    hist = [bank.export_state()]
    for k in range(1, frames + 1):
        update_all(bank, singles, frame_z(fx, F, k))
        hist.append(bank.export_state())
        assert bank.smoothing_depth == min(L, k), k
        if k not in (2, frames):
            continue
        depth = min(L, k)
        h = hist[-(depth + 1):]
        kw = dict(observation=True, particles=True)
        s = bank.smoothed(**kw)
        assert np.array_equal(s.lags.numpy(), np.arange(depth + 1)) and s.lags.dim() == s.frames.dim() == 1
        assert s.states.shape == (F, depth + 1, P, m.d) and s.observation_mean.shape == (F, depth + 1, m.D)
        assert s.distinct_ancestors.shape == (F, depth + 1) and s.ancestors.shape == (F, depth + 1, P)
        _check_bank(s, h, singles, C, k, (cfg, F, P, L, k), **kw)
        same(s, bank.smoothed(**kw), ALL, "twice")
        _check_pose(s, other, (cfg, F, P, L, k))
        rng = bank.smoothed((1, depth), **kw)
        _check_bank(rng, h, None, C, k, (cfg, F, P, L, k, "range"))
        for key in SM_FIELDS:
            assert np.array_equal(getattr(s, key)[:, 1:].numpy(), getattr(rng, key).numpy()), key
        one = bank.smoothed(depth, particles=True)
        assert one.observation_mean is None and one.observation_spread is None
        for key in ("class_probabilities", "state_mean", "distinct_ancestors", "ancestors", "states", "classes"):
            assert np.array_equal(getattr(s, key)[:, depth:].numpy(), getattr(one, key).numpy()), key
        bare = bank.smoothed()
        assert bare.states is None and bare.ancestors is None and bare.classes is None
        same(s, bare, ("lags", "frames", "class_probabilities", "state_mean", "distinct_ancestors"), "bare")
        with pytest.raises(ValueError):
            bank.smoothed(depth + 1)


@pytest.mark.parametrize("d,D,C", [(13, 17, 2), (3, 20, 9)])
def test_odd_model_shapes(d, D, C):
    from gpmdm_amd import GPMDM_PF_Bank
    F, P, L = 3, 77, 4
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=30, S=3, seed=70 + d)
    bank, singles = bank_and_singles(m, T, F, P, seed=3, smoothing_lag=L)
    other = GPMDM_PF_Bank(m, T, F, P, seed=1)
    hist = [bank.export_state()]
    for k in range(7):
        update_all(bank, singles, np.stack([Y[40 + k + 5 * f] for f in range(F)]))
        hist.append(bank.export_state())
    kw = dict(observation=True, particles=True)
    s = bank.smoothed(**kw)
    assert s.states.shape == (F, L + 1, P, d) and s.class_probabilities.shape == (F, L + 1, C)
    _check_bank(s, hist[-(L + 1):], singles, C, 7, (d, D, C), **kw)
    _check_pose(s, other, (d, D, C))


def test_clears(m1, fx_config1):
    """reset, load_state, import_state, a model rebind and set_smoothing each leave depth 0 with
    the current clouds as the root (lag 0 reads them, lag 1 is refused); the history grows again
    from there."""
    from gpmdm_amd import GPMDM_PF_Bank, _lib
    fx, F, P, L = fx_config1, 3, 257, 3
    T = torch.tensor(fx["T"])
    m_other = product_model(fx)
    bank = GPMDM_PF_Bank(m1, T, F, P, seed=4, smoothing_lag=L)
    donor = GPMDM_PF_Bank(m1, T, F, P, seed=4)
    donor.update(frame_z(fx, F, 0))
    st = donor.export_state()
    C = bank.num_classes

    def rebind():
        _lib.check(_lib.load().gpmdm_pf_set_model(bank._h, m_other.handle), "set_model")

    def run(n, row0, hist):
        for k in range(n):
            bank.update(frame_z(fx, F, row0 + k))
            hist.append(bank.export_state())
        return hist

    clears = [("reset", bank.reset), ("load_state", lambda: bank.load_state(st["states"], st["classes"])),
              ("import_state", lambda: bank.import_state(st)), ("rebind", rebind),
              ("set_smoothing", lambda: bank.set_smoothing(L))]
    for what, clear in clears:
        run(2, 20, [])
        assert bank.smoothing_depth >= 2, what
        clear()
        assert bank.smoothing_depth == 0 and bank.smoothing_lag == L, what
        with pytest.raises(ValueError):
            bank.smoothed(1)
        root = bank.export_state()
        s = bank.smoothed(particles=True)
        _check_bank(s, [root], None, C, root["frame"], what)
        assert np.array_equal(s.states[:, 0].numpy(), root["states"]), what
        assert np.array_equal(s.classes[:, 0].numpy(), root["classes"]), what
        hist = run(L + 2, 40, [root])
        assert bank.smoothing_depth == L, what
        _check_bank(bank.smoothed(particles=True), hist[-(L + 1):], None, C, hist[-1]["frame"], (what, "regrown"))
    bank.set_smoothing(0)                          # off: the ring is released, the read-out refused
    assert bank.smoothing_lag == 0 and bank.smoothing_depth == 0
    with pytest.raises(ValueError):
        bank.smoothed()
    bank.update(frame_z(fx, F, 60))                # a plain frame again
    bank.set_smoothing(2)
    hist = run(1, 61, [bank.export_state()])
    _check_bank(bank.smoothed(particles=True), hist, None, C, hist[-1]["frame"], "on again")


@pytest.mark.parametrize("cfg,F,P,resample", [SHAPES[0], SHAPES[2]])
def test_smoothing_has_no_side_effects(request, cfg, F, P, resample):
    """Eight frames with smoothing on and a read-out (with the pose) after every frame leave the
    bank, frame by frame, exactly where eight frames of a bank without smoothing leave it: the
    record changes no frame, and smoothed() no later one."""
    from gpmdm_amd import GPMDM_PF_Bank
    m, fx = _model(request, cfg)
    runs = []
    for look in (False, True):
        bank = GPMDM_PF_Bank(m, torch.tensor(fx["T"]), F, P, seed=19, resample=resample,
                             smoothing_lag=5 if look else 0)
        out = []
        for k in range(8):
            bank.update(frame_z(fx, F, k))
            if look:
                fr = bank.frame
                s = bank.smoothed(observation=True)
                assert len(s.lags) == min(5, k + 1) + 1 and bank.frame == fr, k
            out.append((bank.export_state(), bank.class_probabilities().numpy(), bank.current_state_mean().numpy(),
                        bank.log_likelihood().numpy()))
        runs.append((out, bank.health()))
    (a, ha), (b, hb) = runs
    assert ha == hb
    for k in range(8):
        for key in KEYS:
            assert np.array_equal(a[k][0][key], b[k][0][key]), (k, key)
        for i in (1, 2, 3):
            assert np.array_equal(a[k][i], b[k][i]), (k, i)


def test_cutoff_bank_records(fx_config1):
    """A cutoff bank (its observation tiles run in the switch's class grouping, its resample
    behind them) records as well: bitwise the single cutoff filters, and the reference on the
    bank's own exports."""
    fx, F, P, L = fx_config1, 3, 1000, 3
    m = product_model(fx)
    bank, singles = bank_and_singles(m, torch.tensor(fx["T"]), F, P, seed=700, obs_cutoff=True, smoothing_lag=L)
    hist = [bank.export_state()]
    for k in range(5):
        update_all(bank, singles, frame_z(fx, F, k))
        hist.append(bank.export_state())
    kw = dict(observation=True, particles=True)
    _check_bank(bank.smoothed(**kw), hist[-(L + 1):], singles, bank.num_classes, 5, "cutoff", **kw)


def test_sharded_bank_is_rank_invariant(m1, fx_config1):
    """shard=(3, r) banks of F = 5 give, for their filters, bitwise the rows of the full bank."""
    from gpmdm_amd import GPMDM_PF_Bank
    fx, F, P, L = fx_config1, 5, 100, 3
    T = torch.tensor(fx["T"])
    full = GPMDM_PF_Bank(m1, T, F, P, seed=9, smoothing_lag=L)
    parts = [GPMDM_PF_Bank(m1, T, F, P, seed=9, shard=(3, r), smoothing_lag=L) for r in range(3)]
    for k in range(5):
        Z = frame_z(fx, F, k)
        for b in [full] + parts:
            b.update(Z)
    a = full.smoothed(observation=True, particles=True)
    for p in parts:
        lo, hi = p.filter_range
        assert p.smoothing_depth == L
        b = p.smoothed(observation=True, particles=True)
        assert np.array_equal(a.lags.numpy(), b.lags.numpy()) and np.array_equal(a.frames.numpy(), b.frames.numpy())
        for k in SM_FIELDS:
            assert np.array_equal(getattr(a, k)[lo:hi].numpy(), getattr(b, k).numpy()), (lo, k)
