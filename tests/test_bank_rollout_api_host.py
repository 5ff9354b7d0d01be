"""Host side of the banks' forecasts and fixed-lag smoothing (no GPU): Python checks the
arguments before it touches the library, a bank without local filters returns empty results of
the documented shapes, and the header, the binding, the built library and a C99 caller agree on
gpmdm_bank_forecast / gpmdm_bank_set_smoothing / gpmdm_bank_smoothed."""
import ctypes
import subprocess
import types
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmdm_hip.h"


@pytest.fixture
def bare_bank(monkeypatch):
    """A GPMDM_PF_Bank of 4 filters (this rank: filters 1-2) with the attributes argument
    checking reads and a dummy handle; loading the library (or syncing the model) fails the
    test."""
    from gpmdm_amd import _lib, bank as bankmod

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    b = object.__new__(bankmod.GPMDM_PF_Bank)
    b._gpmdm = types.SimpleNamespace(D=5, d=2, n_classes=3)
    b._num_filters, b._num_particles = 4, 10
    b._f_lo, b._f_hi = 1, 3
    b._h = ctypes.c_void_p(1)
    b._readout = None
    b._smoothing_lag = 4
    monkeypatch.setattr(bankmod.GPMDM_PF_Bank, "_sync_model", touched)
    yield b
    b._h = None                                    # (nothing for __del__ to destroy)


def test_arguments_are_checked_before_the_library(bare_bank):
    b = bare_bank
    for bad in (0, -1, 4097, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="horizon"):
            b.forecast(bad)
    for bad in ("median", None, 0):
        with pytest.raises(ValueError, match="mode"):
            b.forecast(3, mode=bad)
    for bad in (-1, 4097, 2.5, True, "3", (1,), (1, 2, 3), (3, 1), (-1, 2), (0, 4097), (0, 1.5)):
        with pytest.raises(ValueError, match="lag"):
            b.smoothed(bad)
    for bad in (-1, 4097, 2.5, True, None):
        with pytest.raises(ValueError, match="lag"):
            b.set_smoothing(bad)
    # good arguments pass the checks (and only then the library is reached)
    for kw in (dict(), dict(mode="mean"), dict(observation=False, particles=True), dict(seed=7)):
        with pytest.raises(AssertionError, match="touched"):
            b.forecast(3, **kw)
    with pytest.raises(AssertionError, match="touched"):
        b.forecast(4096)
    for lag in (None, 0, 4, (0, 4), [2, 2], 4096):
        with pytest.raises(AssertionError, match="touched"):
            b.smoothed(lag, observation=True, particles=True)
    for L in (0, 1, 4096):
        with pytest.raises(AssertionError, match="touched"):
            b.set_smoothing(L)
    # a bank with smoothing off refuses without the library, and reports depth 0
    b._smoothing_lag = 0
    with pytest.raises(ValueError, match="smoothing is off"):
        b.smoothed()
    assert b.smoothing_depth == 0 and b.smoothing_lag == 0


def test_constructor_checks_the_lag_before_the_library(monkeypatch):
    from gpmdm_amd import GPMDM_PF_Bank, _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    model = types.SimpleNamespace(n_classes=2, set_evaluation_mode=lambda: None)
    for bad in (-1, 4097, 1.5, True):
        with pytest.raises(ValueError, match="lag"):
            GPMDM_PF_Bank(model, torch.eye(2), 3, 10, seed=1, smoothing_lag=bad)


def test_a_bank_without_local_filters_returns_the_empty_shapes(bare_bank):
    b = bare_bank
    b._f_lo = b._f_hi = 2
    b._h = None
    H, P, C, d, D = 3, 10, 3, 2, 5
    fc = b.forecast(H, particles=True)
    assert tuple(fc.class_probabilities.shape) == (0, H, C) and tuple(fc.state_mean.shape) == (0, H, d)
    assert tuple(fc.observation_mean.shape) == tuple(fc.observation_spread.shape) == (0, H, D)
    assert tuple(fc.states.shape) == (0, H, P, d) and tuple(fc.classes.shape) == (0, H, P)
    assert fc.classes.dtype == torch.int64
    bare = b.forecast(H, observation=False, mode="mean", seed=5)
    assert bare.observation_mean is None and bare.observation_spread is None and bare.states is None
    assert bare.classes is None and tuple(bare.class_probabilities.shape) == (0, H, C)
    b.set_smoothing(2)
    assert b.smoothing_lag == 2 and b.smoothing_depth == 0
    s = b.smoothed(observation=True, particles=True)
    assert s.lags.tolist() == [0] and s.frames.tolist() == [0]
    assert tuple(s.class_probabilities.shape) == (0, 1, C) and tuple(s.state_mean.shape) == (0, 1, d)
    assert tuple(s.distinct_ancestors.shape) == (0, 1) and s.distinct_ancestors.dtype == torch.int64
    assert tuple(s.observation_mean.shape) == tuple(s.observation_spread.shape) == (0, 1, D)
    assert tuple(s.ancestors.shape) == tuple(s.classes.shape) == (0, 1, P)
    assert tuple(s.states.shape) == (0, 1, P, d)
    with pytest.raises(ValueError, match="depth"):
        b.smoothed(1)
    b.set_smoothing(0)
    with pytest.raises(ValueError, match="smoothing is off"):
        b.smoothed()


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert ("int gpmdm_bank_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed, "
            "const gpmdm_forecast_out* out, void* stream);") in text
    assert "int gpmdm_bank_set_smoothing(gpmdm_pf_t pf, int lag);" in text
    assert ("int gpmdm_bank_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out, "
            "void* stream);") in text
    assert "class_prob [H][F][C]" in text and "states [H][F][P][d]" in text   # the documented layout
    assert _lib._SIGS["gpmdm_bank_forecast"] == _lib._SIGS["gpmdm_pf_forecast"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                       ctypes.POINTER(_lib.ForecastOut), ctypes.c_void_p])
    assert _lib._SIGS["gpmdm_bank_set_smoothing"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _lib._SIGS["gpmdm_bank_smoothed"] == _lib._SIGS["gpmdm_pf_smoothed"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_lib.SmoothedOut), ctypes.c_void_p])
    assert {"gpmdm_bank_forecast", "gpmdm_bank_set_smoothing", "gpmdm_bank_smoothed"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "smooth" not in " ".join(_lib.STAGES) and "forecast" not in " ".join(_lib.STAGES)   # bench.py sums that table


def test_library_exports_the_symbols_and_rejects_null_handles():
    """The built library carries the entry points; a null handle is refused before any HIP call."""
    from gpmdm_amd import _lib
    lib = _lib.load()
    assert lib.gpmdm_bank_forecast(None, 3, 0, None, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()
    assert lib.gpmdm_bank_set_smoothing(None, 3) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_bank_smoothed(None, 0, 0, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const forecast)(gpmdm_pf_t, int, int, const uint64_t*, const gpmdm_forecast_out*, void*) = gpmdm_bank_forecast;
int (*const set_smoothing)(gpmdm_pf_t, int) = gpmdm_bank_set_smoothing;
int (*const smoothed)(gpmdm_pf_t, int, int, const gpmdm_smoothed_out*, void*) = gpmdm_bank_smoothed;
int use(gpmdm_pf_t bank, const double* z, double* prob, double* pose, int64_t* distinct, int64_t* ancestors) {
  gpmdm_forecast_out fc = {0};
  gpmdm_smoothed_out sm = {0};
  const uint64_t seed = 7;
  int lag = 0, depth = 0;
  int rc = gpmdm_bank_set_smoothing(bank, 8);
  if (rc == GPMDM_OK) rc = gpmdm_pf_step(bank, z, NULL, NULL, NULL, NULL);
  fc.class_prob = prob;
  fc.obs_mean = pose;
  if (rc == GPMDM_OK) rc = gpmdm_bank_forecast(bank, 4, GPMDM_FORECAST_SAMPLE, NULL, &fc, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_forecast(bank, GPMDM_FORECAST_MAX_HORIZON, GPMDM_FORECAST_MEAN, &seed, &fc, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_pf_smoothing_depth(bank, &lag, &depth);
  sm.class_prob = prob;
  sm.distinct = distinct;
  sm.ancestors = ancestors;
  if (rc == GPMDM_OK) rc = gpmdm_bank_smoothed(bank, 0, depth, &sm, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_set_smoothing(bank, 0);
  return rc;
}
"""


def test_c_caller_builds_against_the_header(tmp_path):
    """A C99 caller of the three entry points compiles against include/gpmdm_hip.h (an object
    only: no library, no GPU)."""
    user = tmp_path / "bank_user.c"
    user.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(user),
                        "-o", str(tmp_path / "bank_user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
