"""GPU: a launch-only read-out left pending is covered by the next lifecycle call.

``gpmdm_pf_observation(h, NULL, NULL, s)``, ``gpmdm_pf_innovation(h, NULL, s)``,
``gpmdm_pf_observation_gp(h, NULL, s)`` and the banks' forms queue their launches and return:
the event behind them stays pending on the handle until a lifecycle call (rebind, set_smoothing,
destroy: capi_pf.hip quiesce) waits for it.  Two identically seeded handles step side by side; B
makes the three launch-only calls after every frame and then at once a lifecycle call, A makes
neither.  Every read-out of B must stay bitwise A's, and destroying B with the three pending is
clean.

Two of the lifecycle calls also clear state on B, as documented: a rebind and ``set_smoothing``
clear the smoothing history (so the smoothed rows are compared up to B's depth: rows A's longer
history gives bitwise too), and a rebind forgets the frame's predictive variance, so after it
``innovation()`` on B raises until the next update."""
import numpy as np
import pytest
import torch

from conftest import product_model

pytestmark = pytest.mark.gpu

FRAMES, LAG = 4, 2


@pytest.fixture(scope="module")
def models(fx_config2):
    return product_model(fx_config2), product_model(fx_config2)


def _make(kind, m, T):
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank
    torch.manual_seed(13)                # (the initial cloud comes from torch's generator)
    if kind == "filter":
        return GPMDM_PF(m, T, 1500, rng="philox", seed=21, predictive=True, smoothing_lag=LAG)
    return GPMDM_PF_Bank(m, T, 3, 300, seed=21, predictive=True, smoothing_lag=LAG)


def _launch_only(kind, pf):
    from gpmdm_amd import _lib
    lib, h, s = _lib.load(), pf._h, pf._stream()
    p = "gpmdm_pf" if kind == "filter" else "gpmdm_bank"
    _lib.check(getattr(lib, p + "_observation")(h, None, None, s), "observation, launch only")
    _lib.check(getattr(lib, p + "_innovation")(h, None, s), "innovation, launch only")
    _lib.check(getattr(lib, p + "_observation_gp")(h, None, s), "observation_gp, launch only")


def _fields(x):
    """The arrays of a dict, a (named) tuple or a dataclass, by name."""
    if isinstance(x, dict):
        items = x.items()
    elif hasattr(x, "_asdict"):
        items = x._asdict().items()
    elif hasattr(x, "__dataclass_fields__"):
        items = ((k, getattr(x, k)) for k in x.__dataclass_fields__)
    else:
        items = enumerate(x if isinstance(x, tuple) else (x,))
    return {k: np.asarray(v) for k, v in items if v is not None and k != "seed"}


def _same(what, k, a, b):
    fa, fb = _fields(a), _fields(b)
    assert fa.keys() == fb.keys(), (what, k)
    for key in fa:
        assert np.array_equal(fa[key], fb[key], equal_nan=True), (what, k, key)


@pytest.mark.parametrize("kind", ["filter", "bank"])
def test_lifecycle_calls_cover_pending_launch_only_readouts(models, fx_config2, kind):
    from gpmdm_amd import GPMDM_PF, _lib
    m, m_other = models
    T = torch.tensor(fx_config2["T"])
    Y = m.get_Y()
    lib = _lib.load()
    a, b = _make(kind, m, T), _make(kind, m, T)
    for k in range(1, FRAMES + 1):
        z = np.asarray(Y[30 + 2 * k], dtype=np.float64) + 0.01
        if kind == "bank":
            z = np.repeat(z[None, :], 3, axis=0) + 0.002 * np.arange(3)[:, None]
        a.update(z)
        b.update(z)
        _launch_only(kind, b)
        rebound = k == 1
        if k == 1:                       # rebind to the second, identical model
            _lib.check(lib.gpmdm_pf_set_model(b._h, m_other.handle), "set_model")
        elif k == 2:
            b.set_smoothing(LAG)
        # a rebind (frame 1) and set_smoothing (frame 2) start B's history again at its cloud
        assert a.smoothing_depth == min(k, LAG) and b.smoothing_depth == max(0, k - 2), k
        _same("export_state", k, a.export_state(), b.export_state())
        _same("class_probabilities", k, a.class_probabilities(), b.class_probabilities())
        _same("current_observation", k, a.current_observation(), b.current_observation())
        if rebound:                      # the kept predictive variance was the old model's
            with pytest.raises(RuntimeError, match="no frame weighed"):
                b.innovation()
        else:
            _same("innovation", k, a.innovation(), b.innovation())
        lags = (0, b.smoothing_depth)    # (rows that do not depend on the cleared history)
        _same("smoothed", k, a.smoothed(lags, observation=True), b.smoothed(lags, observation=True))
        _same("forecast", k, a.forecast(2, mode="mean"), b.forecast(2, mode="mean"))
    # the three pending at destroy
    _launch_only(kind, b)
    h = b._h
    b._h = None                          # (the wrapper's __del__ must not destroy it again)
    assert lib.gpmdm_pf_destroy(h) == _lib.GPMDM_OK
    d = GPMDM_PF(m, T, 1000, rng="philox", seed=1)
    d.reset()
    assert np.isclose(d.class_probabilities().numpy().sum(), 1.0)
