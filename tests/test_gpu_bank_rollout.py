"""GPU: what the banks' forecast and smoothing share -- the lifecycle waits and the refusals of
gpmdm_bank_forecast / gpmdm_bank_set_smoothing / gpmdm_bank_smoothed."""
import ctypes

import numpy as np
import pytest
import torch

from bank_rollout_common import frame_z
from conftest import product_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m2(fx_config2):
    return product_model(fx_config2)


def test_lifecycle_with_rollouts_in_flight_waits_for_no_other_stream(m2, fx_config2):
    """test_gpu_smoothing.py's lifecycle property for a bank: while another bank keeps a stream
    of its own busy (several frames queued, tens of ms each), a smoothing bank is created,
    stepped, read (smoothed and forecast), re-initialised, rebound and destroyed right behind
    those calls on the default stream; after every one of them the other stream is still busy,
    so none synchronised the device -- and the next bank on the device works."""
    from gpmdm_amd import GPMDM_PF_Bank, _lib
    fx = fx_config2
    T = torch.tensor(fx["T"])
    Y = np.asarray(m2.get_Y(), dtype=np.float64)
    m_other = product_model(fx)
    lib = _lib.load()
    Fb, frames, F, P = 64, 7, 3, 300
    zs = [np.repeat(Y[40 + 3 * k][None, :] + 0.01, Fb, axis=0) for k in range(frames)]
    busy_bank = GPMDM_PF_Bank(m2, T, Fb, 8000, seed=5)
    # a stream of this test's own, destroyed at its end: one taken from torch's pool lives on for
    # the rest of the process and changes which hardware queues the later tests' streams share
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0            # hipStreamNonBlocking
    sb = torch.cuda.ExternalStream(raw.value)
    holder, busy = {}, []

    def disturb(k):
        if k == 1:
            holder["bank"] = GPMDM_PF_Bank(m2, T, F, P, seed=3, smoothing_lag=4)
            return "create + init"
        bank = holder["bank"]
        if k == 2:
            bank.update(frame_z(fx, F, 0))
            s = bank.smoothed(observation=True, particles=True)
            assert s.states.shape == (F, 2, P, 3)
            assert bank.forecast(3, particles=True).states.shape == (F, 3, P, 3)
            return "update + smoothed + forecast"
        if k == 3:
            bank.forecast(2)
            bank.reset()
            bank.smoothed()
            bank.set_smoothing(4)
            return "forecast + reset + smoothed + set_smoothing"
        if k == 4:
            bank.update(frame_z(fx, F, 1))
            bank.smoothed(observation=True)
            bank.forecast(2, mode="mean")
            _lib.check(lib.gpmdm_pf_set_model(bank._h, m_other.handle), "set_model")
            assert bank.smoothing_depth == 0
            return "smoothed + forecast + rebind"
        bank.update(frame_z(fx, F, 2))
        bank.forecast(2)
        bank.smoothed(particles=True)
        h = bank._h
        bank._h = None                        # (the wrapper's __del__ must not destroy it again)
        _lib.check(lib.gpmdm_pf_destroy(h), "destroy")
        return "update + forecast + smoothed + destroy"

    torch.cuda.synchronize()
    for k in range(frames):
        with torch.cuda.stream(sb):
            busy_bank.update(zs[k])
        if 1 <= k <= 5:
            before = not sb.query()
            what = disturb(k)
            busy.append((what, before, not sb.query()))
    with torch.cuda.stream(sb):
        post = busy_bank.class_probabilities().numpy()
    del busy_bank                             # (its handle waits for its own work, then the stream goes)
    sb.synchronize()
    assert hip.hipStreamDestroy(raw) == 0
    assert np.all(np.isfinite(post))
    for what, before, after in busy:
        assert before, f"the busy bank's stream was idle before {what}: the check would be vacuous"
        assert after, f"{what} waited for the busy bank's stream (device-wide synchronisation)"
    nxt = GPMDM_PF_Bank(m2, T, 2, 100, seed=1, smoothing_lag=2)
    nxt.update(frame_z(fx, 2, 0))
    st = nxt.export_state()
    s = nxt.smoothed(particles=True)
    assert np.array_equal(s.states[:, 0].numpy(), st["states"]) and nxt.smoothing_depth == 1
    assert np.all(np.isfinite(nxt.forecast(2).observation_mean.numpy()))


def test_refusals(m2, fx_config2):
    """A horizon or a lag out of range; a call between switch and resample; a history and a
    forecast staging above 1 GiB, refused by arithmetic on F x Pf."""
    from gpmdm_amd import GPMDM_PF_Bank, _lib
    fx = fx_config2
    T = torch.tensor(fx["T"])
    lib = _lib.load()
    F, P = 2, 300
    bank = GPMDM_PF_Bank(m2, T, F, P, seed=4, smoothing_lag=2)
    h, s = bank._h, bank._stream()
    prob = np.zeros((4, F, 2))
    fo = _lib.ForecastOut(class_prob=_lib.dptr(prob))
    so = _lib.SmoothedOut(class_prob=_lib.dptr(prob))
    for H in (0, -1, _lib.GPMDM_FORECAST_MAX_HORIZON + 1):
        assert lib.gpmdm_bank_forecast(h, H, 0, None, ctypes.byref(fo), s) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_bank_forecast(h, 2, 2, None, ctypes.byref(fo), s) == _lib.GPMDM_E_INVALID
    for L in (-1, _lib.GPMDM_SMOOTH_MAX_LAG + 1):
        assert lib.gpmdm_bank_set_smoothing(h, L) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_bank_smoothed(h, 1, 0, ctypes.byref(so), s) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_bank_smoothed(h, 0, 1, ctypes.byref(so), s) == _lib.GPMDM_E_INVALID   # above the depth
    assert bank.smoothing_lag == 2 and bank.smoothing_depth == 0          # the refused calls changed nothing
    # the single-filter calls keep refusing a bank
    assert lib.gpmdm_pf_forecast(h, 2, 0, None, ctypes.byref(fo), s) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_set_smoothing(h, 2) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_smoothed(h, 0, 0, ctypes.byref(so), s) == _lib.GPMDM_E_INVALID

    bank.update(frame_z(fx, F, 0))
    before = bank.smoothed()
    _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
    assert lib.gpmdm_bank_forecast(h, 2, 0, None, ctypes.byref(fo), s) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_bank_smoothed(h, 0, 0, ctypes.byref(so), s) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_bank_set_smoothing(h, 2) == _lib.GPMDM_E_STATE
    z = np.ascontiguousarray(frame_z(fx, F, 1))
    _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), None, s), "propagate")
    assert lib.gpmdm_bank_forecast(h, 2, 0, None, ctypes.byref(fo), s) == _lib.GPMDM_E_STATE
    assert lib.gpmdm_bank_smoothed(h, 0, 0, ctypes.byref(so), s) == _lib.GPMDM_E_STATE
    _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
    after = bank.smoothed()
    assert len(before.lags) == 2 and len(after.lags) == 3
    assert np.array_equal(after.frames.numpy(), [2, 1, 0])
    assert lib.gpmdm_bank_forecast(h, 2, 0, None, ctypes.byref(fo), s) == _lib.GPMDM_OK

    # 4097 frames x 64 x 20 000 particles x (3 + 1) doubles = 168 GB; 32 steps x 1.28 M x 4 doubles = 1.3 GB
    big = GPMDM_PF_Bank(m2, T, 64, 20_000, seed=2)
    with pytest.raises(ValueError, match="1 GiB"):
        big.set_smoothing(_lib.GPMDM_SMOOTH_MAX_LAG)
    assert big.smoothing_lag == 0 and big.smoothing_depth == 0
    with pytest.raises(ValueError, match="1 GiB"):
        big.forecast(32, particles=True)
    big.update(np.repeat(frame_z(fx, 1, 0), 64, axis=0))                  # (and it still steps)
    assert np.all(np.isfinite(big.log_likelihood().numpy()))
