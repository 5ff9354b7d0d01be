"""Host side of the gating interface (no GPU): Python refuses bad arguments before it touches the
library, and the header, the binding and a C99 caller agree on gpmdm_pf_set_gate /
gpmdm_pf_gate_report and gpmdm_gate_out."""
import ctypes
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmdm_hip.h"
NAMES = ("gpmdm_pf_set_gate", "gpmdm_pf_gate_report")


def _untouchable(monkeypatch):
    from gpmdm_amd import _lib, pf as pfmod

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    return pfmod


def _bare(pfmod, **kw):
    f = object.__new__(pfmod.GPMDM_PF)
    f._gpmdm = types.SimpleNamespace(D=5, d=2, n_classes=2)
    f._peers, f._h, f._num_particles, f._predictive = [], None, 10, True
    f._world, f._gate, f._gate_limit = 1, None, 0.5
    for k, v in kw.items():
        setattr(f, k, v)
    return f


@pytest.mark.parametrize("gate", [0, 0.0, -1.0, True, False, "6", float("nan"), float("inf"), [6.0]])
def test_bad_thresholds_are_refused_before_the_library(monkeypatch, gate):
    pfmod = _untouchable(monkeypatch)
    with pytest.raises(ValueError, match="gate"):
        _bare(pfmod).set_gate(gate)
    with pytest.raises(ValueError, match="gate"):
        pfmod.GPMDM_PF(None, None, 10, gate=gate)


@pytest.mark.parametrize("limit", [0, 0.0, -0.5, 1.0000001, 2, True, "0.5", float("nan"), None])
def test_bad_limits_are_refused_before_the_library(monkeypatch, limit):
    pfmod = _untouchable(monkeypatch)
    with pytest.raises(ValueError, match="gate_limit"):
        _bare(pfmod).set_gate(6.0, limit)
    with pytest.raises(ValueError, match="gate_limit"):
        pfmod.GPMDM_PF(None, None, 10, gate=6.0, gate_limit=limit)


def test_good_arguments_reach_the_library(monkeypatch):
    pfmod = _untouchable(monkeypatch)
    for gate, limit in ((6.0, 0.5), (6, 1), (np.float64(3.5), np.float32(0.25)), (None, 1.0)):
        with pytest.raises(AssertionError, match="touched"):
            _bare(pfmod).set_gate(gate, limit)


def test_sharded_filters_are_refused_before_the_library(monkeypatch):
    pfmod = _untouchable(monkeypatch)
    with pytest.raises(ValueError, match="one rank"):
        pfmod.GPMDM_PF(None, None, 10, gate=6.0, process_group=object())
    with pytest.raises(ValueError, match="one rank"):
        pfmod.GPMDM_PF(None, None, 10, gate=6.0, shard=(2, 0))
    with pytest.raises(ValueError, match="one rank"):
        pfmod.GPMDM_PF(None, None, 10, gate=6.0, shard=(1, 0))
    with pytest.raises(ValueError, match="one rank"):
        _bare(pfmod, _world=2).set_gate(6.0)


def test_devices_of_more_than_one_rank_are_refused_before_the_library(monkeypatch):
    import torch
    pfmod = _untouchable(monkeypatch)
    monkeypatch.setattr(pfmod, "device_shard_plan", lambda P, devices, repeat=False: [(0,), (1,)])
    m = types.SimpleNamespace(set_evaluation_mode=lambda: None, n_classes=2, dtype=torch.float64)
    with pytest.raises(ValueError, match="one rank"):
        pfmod.GPMDM_PF(m, torch.eye(2, dtype=torch.float64), 10, gate=6.0, devices=[0, 1])


def test_predictive_cannot_be_switched_off_while_gated(monkeypatch):
    pfmod = _untouchable(monkeypatch)
    f = _bare(pfmod, _gate=6.0)
    with pytest.raises(ValueError, match="gate"):
        f.set_predictive(False)
    assert f.predictive is True and f.gate == 6.0 and f.gate_limit == 0.5
    with pytest.raises(AssertionError, match="touched"):       # (switching it on again is the library's business)
        f.set_predictive(True)


def test_a_gate_needs_the_predictive_switch(monkeypatch):
    pfmod = _untouchable(monkeypatch)
    with pytest.raises(ValueError, match="predictive"):
        _bare(pfmod, _predictive=False).set_gate(6.0)


def test_gate_report_with_the_gate_off_is_refused_before_the_library(monkeypatch):
    pfmod = _untouchable(monkeypatch)
    with pytest.raises(ValueError, match="gate"):
        _bare(pfmod).gate_report()
    with pytest.raises(AssertionError, match="touched"):
        _bare(pfmod, _gate=6.0).gate_report()


def test_gate_report_is_a_named_tuple_in_the_issue_order():
    from gpmdm_amd import GateReport
    assert GateReport._fields == ("threshold", "zscore", "exceeded", "gated", "used", "n_gated", "n_valid", "overflow")
    assert GateReport._field_defaults == {}


def test_the_bank_takes_no_gate():
    import inspect
    from gpmdm_amd import GPMDM_PF, GPMDM_PF_Bank
    assert "gate" not in inspect.signature(GPMDM_PF_Bank.__init__).parameters
    p = inspect.signature(GPMDM_PF.__init__).parameters
    assert p["gate"].default is None and p["gate_limit"].default == 0.5
    assert p["gate"].kind is p["gate_limit"].kind is inspect.Parameter.KEYWORD_ONLY


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert "int gpmdm_pf_set_gate(gpmdm_pf_t pf, double threshold, double limit); /* threshold <= 0: off */" in text
    assert "int gpmdm_pf_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream);" in text
    assert ("double* zscore; /* D: the frame's, NaN where unobserved */ uint8_t* exceeded; /* D */ "
            "uint8_t* gated; /* D */ uint8_t* used; /* D: the joints the frame's weights rest on */ "
            "int64_t* n_gated; /* 1 */ int64_t* n_valid; /* 1 */ int32_t* overflow; /* 1 */ } gpmdm_gate_out;") in text
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    assert _lib.GateOut._fields_ == [("zscore", dp), ("exceeded", ctypes.c_void_p), ("gated", ctypes.c_void_p),
                                     ("used", ctypes.c_void_p), ("n_gated", ip), ("n_valid", ip),
                                     ("overflow", ctypes.POINTER(ctypes.c_int32))]
    assert _lib._SIGS["gpmdm_pf_set_gate"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double])
    assert _lib._SIGS["gpmdm_pf_gate_report"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_lib.GateOut), ctypes.c_void_p])
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS
    assert "gate" not in _lib.STAGES


def test_library_exports_the_symbols_and_rejects_null_handles():
    """The built library carries the entry points; a null handle is refused before any HIP call."""
    from gpmdm_amd import _lib
    lib = _lib.load()
    assert lib.gpmdm_pf_set_gate(None, 6.0, 0.5) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()
    assert lib.gpmdm_pf_gate_report(None, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const report)(gpmdm_pf_t, const gpmdm_gate_out*, void*) = gpmdm_pf_gate_report;
int use(gpmdm_pf_t pf, double* zscore, uint8_t* gated, uint8_t* used, int64_t* n_gated, int32_t* overflow) {
  gpmdm_gate_out out = {0};
  int rc = gpmdm_pf_set_predictive(pf, 1);
  if (rc == GPMDM_OK) rc = gpmdm_pf_set_gate(pf, 6.0, 0.5);
  out.zscore = zscore;
  out.gated = gated;
  out.used = used;
  out.n_gated = n_gated;
  out.overflow = overflow;
  if (rc == GPMDM_OK) rc = gpmdm_pf_gate_report(pf, &out, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_pf_set_gate(pf, 0.0, 0.5);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
