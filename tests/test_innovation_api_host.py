"""Host side of the innovation interface (no GPU): Python refuses a filter without the predictive
switch before it touches the library, and the header, the binding and a C99 caller agree on
gpmdm_pf_set_predictive / gpmdm_pf_innovation / gpmdm_pf_observation_gp and the banks' calls."""
import ctypes
import subprocess
import types
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmdm_hip.h"
NAMES = ("gpmdm_pf_set_predictive", "gpmdm_pf_innovation", "gpmdm_pf_observation_gp",
         "gpmdm_bank_set_predictive", "gpmdm_bank_innovation", "gpmdm_bank_observation_gp")


def test_a_filter_without_the_switch_refuses_before_the_library(monkeypatch):
    from gpmdm_amd import _lib, pf as pfmod

    def touched(*a, **k):
        raise AssertionError("the library was touched before the switch was checked")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    f = object.__new__(pfmod.GPMDM_PF)
    f._gpmdm = types.SimpleNamespace(D=5, d=2, n_classes=2)
    f._peers, f._h, f._num_particles, f._predictive = [], None, 10, False
    with pytest.raises(ValueError, match="predictive"):
        f.innovation()
    assert f.predictive is False
    f._predictive = True
    with pytest.raises(AssertionError, match="touched"):
        f.innovation(particles=True)


def test_innovation_is_a_named_tuple_in_the_issue_order():
    from gpmdm_amd import Innovation
    assert Innovation._fields == ("mean", "spread", "gp_variance", "variance", "residual", "zscore", "log_density",
                                  "n_valid", "observed", "states", "variance_common")
    assert Innovation._field_defaults == {"states": None, "variance_common": None}


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    for who in ("pf", "bank"):
        assert f"int gpmdm_{who}_set_predictive(gpmdm_pf_t pf, int on);" in text
        assert f"int gpmdm_{who}_innovation(gpmdm_pf_t pf, const gpmdm_innovation_out* out, void* stream);" in text
    assert "int gpmdm_pf_observation_gp(gpmdm_pf_t pf, double* gp_var /* D */, void* stream);" in text
    assert "int gpmdm_bank_observation_gp(gpmdm_pf_t pf, double* gp_var /* F x D */, void* stream);" in text
    assert ("double* mean; /* F x D */ double* spread; /* F x D */ double* gp_variance; /* F x D */ "
            "double* variance; /* F x D */ double* residual; /* F x D */ double* zscore; /* F x D */ "
            "double* log_density; /* F x D */ int64_t* n_valid; /* F */ "
            "uint8_t* observed; /* F x D: the mask the frame was weighed with */ "
            "double* states; /* F x P x d */ double* variance_common; /* F x P */ } gpmdm_innovation_out;") in text
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    assert _lib.InnovationOut._fields_ == [("mean", dp), ("spread", dp), ("gp_variance", dp), ("variance", dp),
                                           ("residual", dp), ("zscore", dp), ("log_density", dp), ("n_valid", ip),
                                           ("observed", ctypes.c_void_p), ("states", dp), ("variance_common", dp)]
    for who in ("pf", "bank"):
        assert _lib._SIGS[f"gpmdm_{who}_set_predictive"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
        assert _lib._SIGS[f"gpmdm_{who}_innovation"] == (
            ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_lib.InnovationOut), ctypes.c_void_p])
        assert _lib._SIGS[f"gpmdm_{who}_observation_gp"] == (ctypes.c_int, [ctypes.c_void_p, dp, ctypes.c_void_p])
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS


def test_library_exports_the_symbols_and_rejects_null_handles():
    """The built library carries the entry points; a null handle is refused before any HIP call."""
    from gpmdm_amd import _lib
    lib = _lib.load()
    for who in ("pf", "bank"):
        assert getattr(lib, f"gpmdm_{who}_set_predictive")(None, 1) == _lib.GPMDM_E_INVALID
        assert getattr(lib, f"gpmdm_{who}_innovation")(None, None, None) == _lib.GPMDM_E_INVALID
        assert getattr(lib, f"gpmdm_{who}_observation_gp")(None, None, None) == _lib.GPMDM_E_INVALID
        assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const innovation)(gpmdm_pf_t, const gpmdm_innovation_out*, void*) = gpmdm_pf_innovation;
int use(gpmdm_pf_t pf, gpmdm_pf_t bank, double* zscore, double* logd, int64_t* n_valid, uint8_t* observed,
        double* gp_var) {
  gpmdm_innovation_out out = {0};
  int rc = gpmdm_pf_set_predictive(pf, 1);
  out.zscore = zscore;
  out.n_valid = n_valid;
  if (rc == GPMDM_OK) rc = gpmdm_pf_innovation(pf, &out, NULL);
  out.log_density = logd;
  out.observed = observed;
  if (rc == GPMDM_OK) rc = gpmdm_pf_observation_gp(pf, gp_var, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_set_predictive(bank, 1);
  if (rc == GPMDM_OK) rc = gpmdm_bank_innovation(bank, &out, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_observation_gp(bank, gp_var, NULL);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
