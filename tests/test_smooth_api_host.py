"""Host side of the smoothing interface (no GPU): Python checks the lag arguments before it
touches the library, and the header, the binding and a C99 caller agree on
gpmdm_pf_set_smoothing / gpmdm_pf_smoothing_depth / gpmdm_pf_smoothed."""
import ctypes
import subprocess
import types
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmdm_hip.h"


@pytest.fixture
def bare_filter(monkeypatch):
    """A GPMDM_PF with the attributes argument checking reads and no library handle; loading
    the library (or syncing the model) fails the test."""
    from gpmdm_amd import _lib, pf as pfmod

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    f = object.__new__(pfmod.GPMDM_PF)
    f._gpmdm = types.SimpleNamespace(D=5, d=2, n_classes=2)
    f._rng = "torch"
    f._peers = []
    f._h = None
    f._num_particles = 10
    f._smoothing_lag = 4
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    return f


def test_arguments_are_checked_before_the_library(bare_filter):
    f = bare_filter
    for bad in (-1, 4097, 2.5, True, "3", (1,), (1, 2, 3), (3, 1), (-1, 2), (0, 4097), (0, 1.5)):
        with pytest.raises(ValueError, match="lag"):
            f.smoothed(bad)
    for bad in (-1, 4097, 2.5, True, None):
        with pytest.raises(ValueError, match="lag"):
            f.set_smoothing(bad)
    # good arguments pass the checks (and only then the library is reached)
    for lag in (None, 0, 4, (0, 4), [2, 2], 4096):
        with pytest.raises(AssertionError, match="touched"):
            f.smoothed(lag, observation=True, particles=True)
    for L in (0, 1, 4096):
        with pytest.raises(AssertionError, match="touched"):
            f.set_smoothing(L)
    # a filter with smoothing off refuses without the library, and reports depth 0
    f._smoothing_lag = 0
    with pytest.raises(ValueError, match="smoothing is off"):
        f.smoothed()
    assert f.smoothing_depth == 0 and f.smoothing_lag == 0


def test_constructor_checks_the_lag_first():
    """smoothing_lag is checked before anything else is looked at (no model, no library)."""
    from gpmdm_amd import GPMDM_PF
    for bad in (-1, 4097, 1.5, True):
        with pytest.raises(ValueError, match="lag"):
            GPMDM_PF(None, None, 10, smoothing_lag=bad)


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert "int gpmdm_pf_set_smoothing(gpmdm_pf_t pf, int lag);" in text
    assert "int gpmdm_pf_smoothing_depth(gpmdm_pf_t pf, int* lag, int* depth);" in text
    assert ("int gpmdm_pf_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out, "
            "void* stream);") in text
    assert ("typedef struct gpmdm_smoothed_out { /* host arrays; any may be NULL; n = lag_last - lag_first + 1 */ "
            "double* class_prob; /* n x C */ double* state_mean; /* n x d */ int64_t* distinct; /* n */ "
            "double* obs_mean; /* n x D */ double* obs_spread; /* n x D */ int64_t* ancestors; /* n x P */ "
            "double* states; /* n x P x d */ int64_t* classes; /* n x P */ } gpmdm_smoothed_out;") in text
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    cp = ctypes.POINTER(ctypes.c_int)
    assert _lib._SIGS["gpmdm_pf_set_smoothing"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _lib._SIGS["gpmdm_pf_smoothing_depth"] == (ctypes.c_int, [ctypes.c_void_p, cp, cp])
    assert _lib._SIGS["gpmdm_pf_smoothed"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_lib.SmoothedOut), ctypes.c_void_p])
    assert _lib.SmoothedOut._fields_ == [("class_prob", dp), ("state_mean", dp), ("distinct", ip), ("obs_mean", dp),
                                         ("obs_spread", dp), ("ancestors", ip), ("states", dp), ("classes", ip)]
    assert f"#define GPMDM_SMOOTH_MAX_LAG {_lib.GPMDM_SMOOTH_MAX_LAG}" in text
    assert _lib.GPMDM_SMOOTH_MAX_LAG == 4096
    assert "smooth" not in " ".join(_lib.STAGES)            # bench.py sums that table
    for name in ("gpmdm_pf_set_smoothing", "gpmdm_pf_smoothing_depth", "gpmdm_pf_smoothed"):
        assert name in _lib.EXPORTED_SYMBOLS


def test_library_exports_the_symbols_and_rejects_null_handles():
    """The built library carries the entry points; a null handle is refused before any HIP call."""
    from gpmdm_amd import _lib
    lib = _lib.load()
    assert lib.gpmdm_pf_set_smoothing(None, 3) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_smoothing_depth(None, None, None) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_smoothed(None, 0, 0, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const smoothed)(gpmdm_pf_t, int, int, const gpmdm_smoothed_out*, void*) = gpmdm_pf_smoothed;
int use(gpmdm_pf_t pf, double* prob, double* pose, int64_t* distinct, int64_t* ancestors) {
  gpmdm_smoothed_out out = {0};
  int lag = 0, depth = 0;
  int rc = gpmdm_pf_set_smoothing(pf, GPMDM_SMOOTH_MAX_LAG);
  if (rc == GPMDM_OK) rc = gpmdm_pf_smoothing_depth(pf, &lag, &depth);
  out.class_prob = prob;
  out.distinct = distinct;
  if (rc == GPMDM_OK) rc = gpmdm_pf_smoothed(pf, 0, depth, &out, NULL);
  out.obs_mean = pose;
  out.ancestors = ancestors;
  if (rc == GPMDM_OK) rc = gpmdm_pf_smoothed(pf, lag, lag, &out, NULL);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
