"""Host side of the masked-observation and filtered-pose interface (no GPU): Python checks the
argument shapes before it touches the library, the binding and the header carry the two entry
points with matching signatures, and the C host still builds against the header."""
import ctypes
import subprocess
import types
from pathlib import Path

import numpy as np
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
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    return f


def test_shapes_are_checked_before_the_library(bare_filter):
    f = bare_filter
    z = np.zeros(5)
    for bad in (np.ones(4, dtype=bool), np.ones(6, dtype=bool), np.ones((2, 5), dtype=bool), [True, False]):
        with pytest.raises(ValueError, match="observed"):
            f.update(z, observed=bad)
        with pytest.raises(ValueError, match="observed"):
            f.update_with_draws(z, None, None, None, observed=bad)
    with pytest.raises(ValueError, match="observation"):
        f.update(np.zeros(4), observed=np.ones(4, dtype=bool))
    with pytest.raises(ValueError, match="observation"):
        f.update_with_draws(np.zeros(6), None, None, None)
    # a good mask passes the check (and only then the library is reached)
    with pytest.raises(AssertionError, match="touched"):
        f.update(z, observed=np.isfinite(z))
    assert f.step.__func__ is f.update.__func__


def test_mask_conversion(bare_filter):
    f = bare_filter
    assert f._check_mask(None) is None
    for given in ([1, 0, 1, 1, 0], np.array([True, False, True, True, False]), np.array([[2.0, 0, 1, -1, 0]]),
                  np.isfinite([0.0, np.nan, 1.0, 2.0, np.inf])):
        m = f._check_mask(given)
        assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and m.tolist() == [1, 0, 1, 1, 0]


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert "int gpmdm_pf_set_obs_mask(gpmdm_pf_t pf, const uint8_t* observed);" in text
    assert "int gpmdm_pf_observation(gpmdm_pf_t pf, double* mean, double* spread, void* stream);" in text
    dp = ctypes.POINTER(ctypes.c_double)
    assert _lib._SIGS["gpmdm_pf_set_obs_mask"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert _lib._SIGS["gpmdm_pf_observation"] == (ctypes.c_int, [ctypes.c_void_p, dp, dp, ctypes.c_void_p])
    assert "obs_readout" not in " ".join(_lib.STAGES)       # bench.py sums that table


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const set_mask)(gpmdm_pf_t, const uint8_t*) = gpmdm_pf_set_obs_mask;
int (*const observation)(gpmdm_pf_t, double*, double*, void*) = gpmdm_pf_observation;
int use(gpmdm_pf_t pf, const double* z, double* pose, double* spread) {
  uint8_t seen[4] = {1, 0, 1, 1};
  int rc = gpmdm_pf_set_obs_mask(pf, seen);
  if (rc == GPMDM_OK) rc = gpmdm_pf_step(pf, z, NULL, NULL, NULL, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_pf_observation(pf, pose, spread, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_pf_set_obs_mask(pf, NULL);
  return rc;
}
"""


def test_c_hosts_build_against_the_header(tmp_path):
    """examples/c_host/pf_main.c and a C99 caller of the two new entry points compile against
    include/gpmdm_hip.h (objects only: no library, no GPU)."""
    user = tmp_path / "user.c"
    user.write_text(C_USER)
    for src in (ROOT / "examples" / "c_host" / "pf_main.c", user):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                            "-o", str(tmp_path / (src.stem + ".o"))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
