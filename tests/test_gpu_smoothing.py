"""``GPMDM_PF.smoothed`` (gpmdm_pf_smoothed, csrc/smooth.h): fixed-lag smoothing from the
particles' ancestry.

The reference is ``smooth_ref`` on the filter's own ``export_state()`` after every update (the
root: the export before the first one).  Bounds:

* ``ancestors``, ``classes``, ``states`` and ``distinct_ancestors``: exact;
* ``class_probabilities``: bitwise count / P;
* ``|state_mean[l, j] - fsum mean| <= P 2^-53 mean_p |x_pj|``: any summation order of P fp64
  terms errs by at most (P - 1) 2^-53 sum |x|, and the division adds half an ulp of the mean;
* the pose rows: bitwise ``current_observation()`` of a second filter that was handed the
  lag's traced cloud through ``load_state`` (the same kernel on the same cloud in the same
  order; the read-out is reproducible).
"""
import ctypes

import numpy as np
import pytest
import torch

import smooth_ref as R
from conftest import product_model, synthetic_model

pytestmark = pytest.mark.gpu

FIELDS = ("lags", "frames", "class_probabilities", "state_mean", "distinct_ancestors", "observation_mean",
          "observation_spread", "ancestors", "states", "classes")


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def _same(a, b, fields=FIELDS, rows=slice(None)):
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        if x is None or y is None:
            assert x is None and y is None, k
        else:
            assert np.array_equal(x.numpy()[rows], y.numpy()), k


def _check(s, hist, C, frame, what):
    """A Smoothed made with particles=True against smooth_ref on the exports ``hist``."""
    lags = s.lags.numpy()
    ref = R.smoothed(hist, int(lags[0]), int(lags[-1]))
    P = len(hist[-1]["classes"])
    assert s.lags.dtype == s.frames.dtype == s.distinct_ancestors.dtype == s.ancestors.dtype == torch.int64
    assert s.classes.dtype == torch.int64 and s.states.dtype == s.state_mean.dtype == torch.float64
    assert np.array_equal(s.frames.numpy(), frame - lags), what
    assert np.array_equal(s.ancestors.numpy(), ref["ancestors"]), what
    assert np.array_equal(s.classes.numpy(), ref["classes"]), what
    assert np.array_equal(s.states.numpy(), ref["states"]), what
    assert np.array_equal(s.distinct_ancestors.numpy(), ref["distinct_ancestors"]), what
    assert np.array_equal(s.class_probabilities.numpy(), R.class_probabilities(ref, C)), what
    err = np.abs(s.state_mean.numpy() - ref["state_mean"])
    bound = P * 2.0 ** -53 * np.abs(ref["states"]).mean(1)
    print(what, "state_mean err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound), (what, err, bound)
    da = s.distinct_ancestors.numpy()
    assert np.all(np.diff(da) <= 0) and np.all(da >= 1), (what, da)
    if lags[0] == 0:
        assert da[0] == P, what


def _check_pose(s, other, what):
    """Each row's pose against current_observation() of ``other`` holding that row's cloud."""
    for i in range(len(s.lags)):
        other.load_state(s.states[i].numpy(), s.classes[i].numpy())
        mean, spread = other.current_observation()
        assert np.array_equal(s.observation_mean[i].numpy(), mean.numpy()), (what, i)
        assert np.array_equal(s.observation_spread[i].numpy(), spread.numpy()), (what, i)


def _run(pf, Y, frames, row0, hist=None, each=None):
    hist = [pf.export_state()] if hist is None else hist
    for k in range(frames):
        pf.update(Y[row0 + k])
        hist.append(pf.export_state())
        if each is not None:
            each(k + 1, hist)
    return hist


@pytest.mark.parametrize("L", [1, 3, 17])
@pytest.mark.parametrize("P", [1, 33, 777, 5000])
def test_against_the_reference(m2, fx_config2, P, L):
    """One particle, a partial wave, a ragged last block, several blocks above the small
    resampling path; 2 L + 3 frames, so the ring wraps.  After frame 2 (depth below L for
    L > 2) and after the last frame; every lag, one lag and a range; twice in a row."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=7, smoothing_lag=L)
    other = GPMDM_PF(m2, T, P, rng="philox", seed=1)
    assert pf.smoothing_lag == L and pf.smoothing_depth == 0
    Y = m2.get_Y()
    n = 2 * L + 3

    def each(k, hist):
        assert pf.smoothing_depth == min(L, k), k
        if k not in (2, n):
            return
        depth = min(L, k)
        h = hist[-(depth + 1):]
        s = pf.smoothed(observation=True, particles=True)
        assert np.array_equal(s.lags.numpy(), np.arange(depth + 1))
        assert s.states.shape == (depth + 1, P, 3) and s.observation_mean.shape == (depth + 1, 62)
        _check(s, h, 2, k, (P, L, k))
        _same(s, pf.smoothed(observation=True, particles=True))
        _check_pose(s, other, (P, L, k))
        one = pf.smoothed(depth, particles=True)
        assert one.observation_mean is None and one.observation_spread is None
        _check(one, h, 2, k, (P, L, k, "one"))
        _same(s, one, ("lags", "frames", "class_probabilities", "state_mean", "distinct_ancestors", "ancestors",
                       "states", "classes"), slice(depth, depth + 1))
        rng = pf.smoothed((1, depth), observation=True, particles=True)
        _check(rng, h, 2, k, (P, L, k, "range"))
        _same(s, rng, rows=slice(1, depth + 1))
        bare = pf.smoothed()
        assert bare.states is None and bare.ancestors is None and bare.classes is None
        _same(s, bare, ("lags", "frames", "class_probabilities", "state_mean", "distinct_ancestors"))
        with pytest.raises(ValueError):
            pf.smoothed(depth + 1)

    _run(pf, Y, n, 200, each=each)


@pytest.mark.parametrize("d,D,C", [(1, 5, 2), (13, 17, 2), (3, 20, 9)])
def test_model_shapes(d, D, C):
    from gpmdm_amd import GPMDM_PF
    S, Lseq, P, L = 3, 30, 300, 4
    m, T, Y = synthetic_model(C=C, d=d, D=D, L=Lseq, S=S, seed=70 + d)
    pf = GPMDM_PF(m, T, P, rng="philox", seed=3, smoothing_lag=L)
    other = GPMDM_PF(m, T, P, rng="philox", seed=1)
    hist = _run(pf, Y, 7, 40)
    s = pf.smoothed(observation=True, particles=True)
    assert s.states.shape == (L + 1, P, d) and s.class_probabilities.shape == (L + 1, C)
    assert s.observation_spread.shape == (L + 1, D)
    _check(s, hist[-(L + 1):], C, 7, (d, D, C))
    _check_pose(s, other, (d, D, C))


@pytest.mark.parametrize("kw,P", [(dict(rng="philox", seed=5, resample="systematic"), 777),
                                  (dict(rng="torch"), 100), (dict(rng="torch"), 2000)])
def test_resampling_and_draw_modes(m2, fx_config2, kw, P):
    """Systematic resampling; replay draws on the one-workgroup resampling path (P = 100: the
    notebook's filter) and on the large one."""
    from gpmdm_amd import GPMDM_PF
    torch.manual_seed(21)
    L = 3
    pf = GPMDM_PF(m2, torch.tensor(fx_config2["T"]), P, smoothing_lag=L, **kw)
    hist = _run(pf, m2.get_Y(), 6, 500)
    s = pf.smoothed(particles=True)
    _check(s, hist[-(L + 1):], 2, 6, (kw, P))
    _same(s, pf.smoothed(particles=True))


@pytest.mark.parametrize("rng,P", [("philox", 3000), ("torch", 2000)])
def test_smoothing_has_no_side_effects(m2, fx_config2, rng, P):
    """Twelve frames with smoothing on and a read-out (with the pose) after every frame leave
    the filter, frame by frame, exactly where twelve plain frames leave it (a Philox filter's
    pre-switch is pending behind each call); torch's generator and the health counters are not
    touched."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Y = m2.get_Y()
    runs = []
    for look in (False, True):
        torch.manual_seed(12)
        pf = GPMDM_PF(m2, T, P, rng=rng, seed=19 if rng == "philox" else None, smoothing_lag=5 if look else 0)
        out = []
        for k in range(12):
            pf.update(Y[300 + k])
            if look:
                g, fr = torch.get_rng_state(), pf.frame
                s = pf.smoothed(observation=True)
                assert len(s.lags) == min(5, k + 1) + 1
                assert torch.equal(g, torch.get_rng_state()) and pf.frame == fr, k
            out.append((pf.class_probabilities().numpy().copy(), pf.current_state_mean().numpy().copy(),
                        pf.log_likelihood(), pf.export_state()))
        runs.append((out, pf.health()))
    (a, ha), (b, hb) = runs
    assert ha == hb
    for k in range(12):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) and a[k][2] == b[k][2], k
        for key in ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame"):
            assert np.array_equal(a[k][3][key], b[k][3][key]), (k, key)


def test_clears(m2, fx_config2):
    """reset, load_state, import_state, a model rebind and set_smoothing each leave depth 0 with
    the current cloud as the root (lag 0 reads it, lag 1 is refused), and the history grows
    again from there."""
    from gpmdm_amd import GPMDM_PF, _lib
    T = torch.tensor(fx_config2["T"])
    Y = m2.get_Y()
    P, L = 500, 3
    m_other = product_model(fx_config2)
    pf = GPMDM_PF(m2, T, P, rng="philox", seed=4, smoothing_lag=L)
    donor = GPMDM_PF(m2, T, P, rng="philox", seed=4)
    donor.update(Y[100])
    st = donor.export_state()

    def rebind():
        _lib.check(_lib.load().gpmdm_pf_set_model(pf._h, m_other.handle), "set_model")

    clears = [("reset", pf.reset), ("load_state", lambda: pf.load_state(st["states"], st["classes"])),
              ("import_state", lambda: pf.import_state(st)), ("rebind", rebind),
              ("set_smoothing", lambda: pf.set_smoothing(L))]
    for what, clear in clears:
        _run(pf, Y, 2, 120)
        assert pf.smoothing_depth >= 2, what
        clear()
        assert pf.smoothing_depth == 0, what
        with pytest.raises(ValueError):
            pf.smoothed(1)
        root = pf.export_state()
        s = pf.smoothed(particles=True)
        _check(s, [root], 2, root["frame"], what)
        hist = _run(pf, Y, L + 2, 140, hist=[root])
        assert pf.smoothing_depth == L, what
        _check(pf.smoothed(particles=True), hist[-(L + 1):], 2, hist[-1]["frame"], (what, "regrown"))
    # another lag: a new ring
    pf.set_smoothing(1)
    assert pf.smoothing_lag == 1 and pf.smoothing_depth == 0
    hist = _run(pf, Y, 3, 160)
    _check(pf.smoothed(particles=True), hist[-2:], 2, hist[-1]["frame"], "lag 1")
    # off: the ring is released and the read-out refused
    pf.set_smoothing(0)
    assert pf.smoothing_lag == 0 and pf.smoothing_depth == 0
    with pytest.raises(ValueError):
        pf.smoothed()
    pf.update(Y[170])                         # a plain frame again
    pf.set_smoothing(2)
    hist = _run(pf, Y, 1, 171)
    _check(pf.smoothed(particles=True), hist, 2, hist[-1]["frame"], "on again")


def test_refusals(m2, fx_config2):
    """A lag above the maximum, a history above 1 GiB, a bank, a call inside a frame."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    lib = _lib.load()
    pf = GPMDM_PF(m2, T, 20_000, rng="philox", seed=2, smoothing_lag=2)
    with pytest.raises(ValueError):
        pf.set_smoothing(_lib.GPMDM_SMOOTH_MAX_LAG + 1)
    assert lib.gpmdm_pf_set_smoothing(pf._h, _lib.GPMDM_SMOOTH_MAX_LAG + 1) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_set_smoothing(pf._h, -1) == _lib.GPMDM_E_INVALID
    # 4097 frames x 20 000 particles x (3 + 1) doubles = 2.6 GB
    with pytest.raises(ValueError, match="1 GiB"):
        pf.set_smoothing(_lib.GPMDM_SMOOTH_MAX_LAG)
    with pytest.raises(ValueError, match="1 GiB"):
        GPMDM_PF(m2, T, 20_000, rng="philox", seed=2, smoothing_lag=_lib.GPMDM_SMOOTH_MAX_LAG)
    assert pf.smoothing_lag == 2                      # the refused calls changed nothing
    pf.update(Y[50])
    assert pf.smoothing_depth == 1

    bank = GPMDM_PF_Bank(m2, T, 2, 300, seed=4)
    prob = np.zeros((1, 2))
    out = _lib.SmoothedOut(class_prob=_lib.dptr(prob))
    assert lib.gpmdm_pf_set_smoothing(bank._h, 3) == _lib.GPMDM_E_INVALID
    with pytest.raises(ValueError):
        _lib.check(lib.gpmdm_pf_smoothed(bank._h, 0, 0, ctypes.byref(out), bank._stream()), "bank")

    h, s = pf._h, pf._stream()
    before = pf.smoothed()
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    assert lib.gpmdm_pf_smoothed(h, 0, 0, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_pf_set_smoothing(h, 2) == _lib.GPMDM_E_STATE
    z = np.ascontiguousarray(Y[51])
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), None, s), "propagate")
    assert lib.gpmdm_pf_smoothed(h, 0, 0, ctypes.byref(out), s) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    after = pf.smoothed()
    assert len(after.lags) == 3 and len(before.lags) == 2
    assert np.array_equal(after.frames.numpy(), [2, 1, 0])


def test_sharded_filter_reads_rank_0(m2, fx_config2):
    """devices=[0, 0] over the loopback transport: every rank records the replicated cloud, and
    the read-out is bitwise the one-rank filter's."""
    from gpmdm_amd import GPMDM_PF
    T = torch.tensor(fx_config2["T"])
    Y = m2.get_Y()
    P, L = 1003, 3

    def make(**kw):
        torch.manual_seed(6)
        return GPMDM_PF(m2, T, P, rng="philox", seed=9, smoothing_lag=L, **kw)

    one, two = make(), make(devices=[0, 0], transport="loopback")
    hist = [one.export_state()]
    for k in range(8):
        one.update(Y[600 + k])
        two.update(Y[600 + k])
        hist.append(one.export_state())
        assert two.smoothing_depth == min(L, k + 1)
    a = one.smoothed(observation=True, particles=True)
    _check(a, hist[-(L + 1):], 2, 8, "one rank")
    _same(a, two.smoothed(observation=True, particles=True))


def test_lifecycle_of_an_enabled_filter_waits_for_no_other_stream(m2, fx_config2):
    """tests/test_gpu_lifecycle.py's property with smoothing on: while a filter bank keeps a
    stream of its own busy (several frames queued, tens of ms each), an enabled filter is
    created, stepped and read, cleared, rebound and destroyed with a record launch in flight on
    the default stream; after every one of those calls the bank's stream is still busy, so none
    of them synchronised the device."""
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank, _lib
    T = torch.tensor(fx_config2["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    m_other = product_model(fx_config2)
    lib = _lib.load()
    F, frames = 64, 7
    zs = [np.repeat(Y[40 + 3 * k][None, :] + 0.01, F, axis=0) for k in range(frames)]
    bank = GPMDM_PF_Bank(m2, T, F, 8000, seed=5)
    sb = torch.cuda.Stream()
    holder, busy = {}, []

    def disturb(k):
        if k == 1:
            holder["pf"] = GPMDM_PF(m2, T, 5000, rng="philox", seed=3, smoothing_lag=4)
            return "create + init"
        pf = holder["pf"]
        if k == 2:
            pf.update(Y[10])
            s = pf.smoothed(observation=True, particles=True)
            assert s.states.shape == (2, 5000, 3)
            return "update + smoothed"
        if k == 3:
            pf.set_smoothing(4)
            pf.reset()
            return "set_smoothing + reset"
        if k == 4:
            _lib.check(lib.gpmdm_pf_set_model(pf._h, m_other.handle), "set_model")
            return "rebind"
        pf.update(Y[11])
        h = pf._h
        pf._h = None                          # (the wrapper's __del__ must not destroy it again)
        _lib.check(lib.gpmdm_pf_destroy(h), "destroy")
        return "update + destroy"

    torch.cuda.synchronize()
    for k in range(frames):
        with torch.cuda.stream(sb):
            bank.update(zs[k])
        if 1 <= k <= 5:
            before = not sb.query()
            what = disturb(k)
            busy.append((what, before, not sb.query()))
    with torch.cuda.stream(sb):
        post = bank.class_probabilities().numpy()
    assert np.all(np.isfinite(post))
    for what, before, after in busy:
        assert before, f"the bank's stream was idle before {what}: the check would be vacuous"
        assert after, f"{what} waited for the bank's stream (device-wide synchronisation)"


@pytest.mark.parametrize("read", [False, True])
def test_destroy_with_work_in_flight(m2, fx_config2, read):
    """An enabled filter destroyed right after an update (its record launch follows the
    read-out number the lifecycle waits for) or right after a read-out; the next filter on the
    device works."""
    from gpmdm_amd import GPMDM_PF, _lib
    T = torch.tensor(fx_config2["T"])
    Y = m2.get_Y()
    pf = GPMDM_PF(m2, T, 20_000, rng="philox", seed=3, smoothing_lag=8)
    pf.update(Y[10])
    pf.update(Y[11])
    if read:
        pf.smoothed(observation=True, particles=True)
    h = pf._h
    pf._h = None                              # (the wrapper's __del__ must not destroy it again)
    _lib.check(_lib.load().gpmdm_pf_destroy(h), "destroy")
    nxt = GPMDM_PF(m2, T, 500, rng="philox", seed=1, smoothing_lag=2)
    hist = _run(nxt, Y, 2, 12)
    _check(nxt.smoothed(particles=True), hist, 2, 2, "after destroy")
