"""Host side of the banks' per-filter masks and pose read-out (no GPU): Python checks the
``observed`` shapes before it touches the library, the binding and the header carry the two
entry points with matching signatures, and a C99 caller builds against the header."""
import ctypes
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

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
    b._gpmdm = types.SimpleNamespace(D=5, d=2, n_classes=2)
    b._num_filters, b._num_particles = 4, 10
    b._f_lo, b._f_hi = 1, 3
    b._h = ctypes.c_void_p(1)
    b._readout = None
    monkeypatch.setattr(bankmod.GPMDM_PF_Bank, "_sync_model", touched)
    yield b
    b._h = None                                    # (nothing for __del__ to destroy)


def test_observed_shapes_are_checked_before_the_library(bare_bank):
    b = bare_bank
    Z = np.zeros((4, 5))
    for shape in ((4, 4), (5, 5), (3, 5), (2, 4, 5), (4,), (6,), ()):
        with pytest.raises(ValueError, match="observed"):
            b.update(Z, observed=np.ones(shape, dtype=bool))
        with pytest.raises(ValueError, match="observed"):
            b.update(Z[1:3], observed=np.ones(shape, dtype=bool))
    with pytest.raises(ValueError, match="observations"):
        b.update(np.zeros((3, 5)), observed=np.ones((4, 5), dtype=bool))
    # good masks pass the check (and only then the library is reached)
    for good in (np.ones((4, 5), dtype=bool), np.ones((2, 5), dtype=bool), np.ones(5, dtype=bool), np.isfinite(Z)):
        with pytest.raises(AssertionError, match="touched"):
            b.update(Z, observed=good)
    assert b.step.__func__ is b.update.__func__


def test_mask_conversion(bare_bank):
    b = bare_bank
    assert b._check_masks(None) is None
    full = np.arange(20).reshape(4, 5) % 3 != 0
    m = b._check_masks(full)                       # (F, D): this rank's rows
    assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and m.shape == (2, 5)
    assert np.array_equal(m, full[1:3].astype(np.uint8))
    assert np.array_equal(b._check_masks(full[1:3]), m)        # (F_local, D)
    one = b._check_masks([1, 0, 2.5, 0, -1])      # (D,): one mask for every filter
    assert one.flags["C_CONTIGUOUS"] and one.tolist() == [[1, 0, 1, 0, 1]] * 2
    z = np.array([[0.0, np.nan, 1.0, 2.0, np.inf]] * 2)
    assert b._check_masks(np.isfinite(z)).tolist() == [[1, 0, 1, 1, 0]] * 2


def test_a_bank_without_local_filters_reads_empty_poses(bare_bank):
    b = bare_bank
    b._f_lo = b._f_hi = 2
    b._h = None
    b.update(np.zeros((4, 5)), observed=np.ones((4, 5), dtype=bool))
    mean, spread = b.current_observation()
    assert tuple(mean.shape) == tuple(spread.shape) == (0, 5)
    assert tuple(b.current_observation_mean().shape) == (0, 5)
    assert b.health() == {k: 0 for k in b.health()} and len(b.health()) == 4


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert ("int gpmdm_bank_set_obs_masks(gpmdm_pf_t pf, const uint8_t* observed); "
            "/* F x D bytes, filter-major; NULL: all observed */") in text
    assert ("int gpmdm_bank_observation(gpmdm_pf_t pf, double* mean, double* spread, void* stream); "
            "/* F x D each, filter-major; spread may be NULL */") in text
    dp = ctypes.POINTER(ctypes.c_double)
    assert _lib._SIGS["gpmdm_bank_set_obs_masks"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    assert _lib._SIGS["gpmdm_bank_observation"] == (ctypes.c_int, [ctypes.c_void_p, dp, dp, ctypes.c_void_p])
    assert {"gpmdm_bank_set_obs_masks", "gpmdm_bank_observation"} <= set(_lib.EXPORTED_SYMBOLS)


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const set_masks)(gpmdm_pf_t, const uint8_t*) = gpmdm_bank_set_obs_masks;
int (*const observation)(gpmdm_pf_t, double*, double*, void*) = gpmdm_bank_observation;
int use(gpmdm_pf_t bank, const double* z, double* pose, double* spread) {
  uint8_t seen[2][4] = {{1, 0, 1, 1}, {0, 0, 0, 0}};
  int rc = gpmdm_bank_set_obs_masks(bank, &seen[0][0]);
  if (rc == GPMDM_OK) rc = gpmdm_pf_step(bank, z, NULL, NULL, NULL, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_observation(bank, pose, spread, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_observation(bank, pose, NULL, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_set_obs_masks(bank, NULL);
  return rc;
}
"""


def test_c_caller_builds_against_the_header(tmp_path):
    """A C99 caller of the two new entry points compiles against include/gpmdm_hip.h (an
    object only: no library, no GPU)."""
    user = tmp_path / "bank_user.c"
    user.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(user),
                        "-o", str(tmp_path / "bank_user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
