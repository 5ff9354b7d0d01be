"""Host side of the banks' gating interface (no GPU): Python refuses bad ``gate`` arguments before
it touches the library, a sharded bank takes its own rows of a per-filter sequence, and the header,
the binding and a C99 caller agree on gpmdm_bank_set_gate / gpmdm_bank_gate_report."""
import ctypes
import inspect
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmdm_hip.h"
NAMES = ("gpmdm_bank_set_gate", "gpmdm_bank_gate_report")


@pytest.fixture
def bare_bank(monkeypatch):
    """A predictive GPMDM_PF_Bank of 4 filters (this rank: filters 1-2) with the attributes the
    argument checks read and a dummy handle; loading the library (or syncing the model) fails the
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
    b._predictive, b._gate, b._gate_limit = True, None, 0.5
    monkeypatch.setattr(bankmod.GPMDM_PF_Bank, "_sync_model", touched)
    yield b
    b._h = None                                    # (nothing for __del__ to destroy)


@pytest.mark.parametrize("gate", [0, 0.0, -1.0, True, "6", float("nan"), float("inf"), [6.0], [6.0] * 3, [6.0] * 5,
                                  [6.0, 0.0], [6.0, "6"], [None, float("nan")], [[6.0, 6.0]], (6.0, True),
                                  np.ones((2, 2))])
def test_bad_gates_are_refused_before_the_library(bare_bank, gate):
    with pytest.raises(ValueError, match="gate"):
        bare_bank.set_gate(gate)
    assert bare_bank.gate is None


@pytest.mark.parametrize("limit", [0, 0.0, -0.5, 1.0000001, 2, True, "0.5", float("nan"), None])
def test_bad_limits_are_refused_before_the_library(bare_bank, limit):
    with pytest.raises(ValueError, match="gate_limit"):
        bare_bank.set_gate(6.0, limit)
    with pytest.raises(ValueError, match="gate_limit"):
        bare_bank.set_gate(None, limit)


@pytest.mark.parametrize("gate", [6.0, 6, np.float64(3.5), [6.0, None], (None, None), [1.0, 6.0, None, 2.0],
                                  np.array([6.0, 3.0]), np.array([1.0, 6.0, 3.0, 2.0]), None])
def test_good_gates_reach_the_library(bare_bank, gate):
    with pytest.raises(AssertionError, match="touched"):
        bare_bank.set_gate(gate, 0.25)


def test_rows_of_a_sharded_bank():
    """(F,) sequences: each rank takes its rows, as ``_check_masks`` does; one number serves every
    filter; None entries stay None (sent as +inf)."""
    from gpmdm_amd.pf import _check_bank_gate
    assert _check_bank_gate([1.0, 6.0, None, 2.0], 0.5, 4, 1, 3) == ((6.0, None), 0.5)
    assert _check_bank_gate([6, None], 1, 4, 1, 3) == ((6.0, None), 1.0)
    assert _check_bank_gate(4, 0.25, 4, 1, 3) == ((4.0, 4.0), 0.25)
    assert _check_bank_gate(None, 0.25, 4, 1, 3) == (None, 0.25)
    assert _check_bank_gate([5.0, 6.0], 0.5, 2, 0, 2) == ((5.0, 6.0), 0.5)
    ks, _ = _check_bank_gate(np.array([5.0, 6.0]), 0.5, 2, 0, 2)
    assert ks == (5.0, 6.0) and all(type(k) is float for k in ks)
    assert _check_bank_gate([], 0.5, 4, 2, 2) == ((), 0.5)         # a rank without filters


def test_a_gate_needs_the_predictive_switch(bare_bank):
    from gpmdm_amd import bank as bankmod
    bare_bank._predictive = False
    with pytest.raises(ValueError, match="predictive"):
        bare_bank.set_gate(6.0)
    # the constructor: before the model, the library or a process group is looked at
    model = types.SimpleNamespace(set_evaluation_mode=lambda: None, n_classes=2)
    with pytest.raises(ValueError, match="predictive"):
        bankmod.GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, gate=6.0)
    with pytest.raises(ValueError, match="predictive"):
        bankmod.GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, shard=(2, 1), gate=[6.0, None, 6.0, 6.0])
    with pytest.raises(ValueError, match="gate"):
        bankmod.GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, predictive=True, gate=[6.0] * 3)
    with pytest.raises(ValueError, match="gate_limit"):
        bankmod.GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, predictive=True, gate=6.0, gate_limit=0.0)


def test_predictive_cannot_be_switched_off_while_gated(bare_bank):
    bare_bank._gate = (6.0, None)
    with pytest.raises(ValueError, match="gate"):
        bare_bank.set_predictive(False)
    assert bare_bank.predictive is True and bare_bank.gate == (6.0, None) and bare_bank.gate_limit == 0.5
    with pytest.raises(AssertionError, match="touched"):       # (switching it on again is the library's business)
        bare_bank.set_predictive(True)


def test_gate_report_with_the_gate_off_is_refused_before_the_library(bare_bank):
    with pytest.raises(ValueError, match="gate"):
        bare_bank.gate_report()
    bare_bank._gate = (6.0, None)
    with pytest.raises(AssertionError, match="touched"):
        bare_bank.gate_report()


def test_a_bank_without_local_filters_reports_empty_rows(bare_bank):
    b = bare_bank
    b._f_lo = b._f_hi = 2
    b._h = None
    b.set_gate([6.0, 6.0, None, 6.0])
    assert b.gate == ()
    rep = b.gate_report()
    assert tuple(rep.zscore.shape) == tuple(rep.used.shape) == (0, 5)
    assert tuple(rep.threshold.shape) == tuple(rep.n_gated.shape) == tuple(rep.overflow.shape) == (0,)
    b.set_gate(None)
    assert b.gate is None


def test_the_bank_takes_a_gate(bare_bank):
    """The constructor takes ``gate`` / ``gate_limit`` as keywords only (a keyword group: the named
    parameters of its signature stay the ones tests/test_gate_api_host.py pins), with the defaults
    None and 0.5, and refuses every other unknown keyword; ``set_gate`` names them."""
    from gpmdm_amd import GPMDM_PF_Bank
    p = inspect.signature(GPMDM_PF_Bank.__init__).parameters
    assert p["gating"].kind is inspect.Parameter.VAR_KEYWORD
    assert not any(v.kind is inspect.Parameter.VAR_POSITIONAL for v in p.values())
    model = types.SimpleNamespace(set_evaluation_mode=lambda: None, n_classes=2)
    for kw in (dict(gates=6.0), dict(gate=6.0, limit=0.5), dict(predictive=True, gate_limits=0.5)):
        with pytest.raises(TypeError, match="unexpected keyword"):
            GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, **kw)
    with pytest.raises(TypeError):                  # keywords only
        GPMDM_PF_Bank(model, np.eye(2), 4, 10, 1, "multinomial", None, None, True, "auto", False, 0, True, 6.0)
    # a rank without filters touches no library: the defaults, and what the keywords leave behind
    b = GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, shard=(8, 0))
    assert b.local_filters == 0 and b.gate is None and b.gate_limit == 0.5
    b = GPMDM_PF_Bank(model, np.eye(2), 4, 10, seed=1, shard=(8, 0), predictive=True, gate=6.0, gate_limit=0.25)
    assert b.gate == () and b.gate_limit == 0.25 and b.predictive is True
    p = inspect.signature(GPMDM_PF_Bank.set_gate).parameters
    assert list(p) == ["self", "gate", "limit"] and p["gate"].default is None and p["limit"].default == 0.5


def test_bank_gate_report_is_a_named_tuple_in_the_issue_order():
    import gpmdm_amd
    from gpmdm_amd import BankGateReport, GateReport
    assert BankGateReport._fields == GateReport._fields == (
        "threshold", "zscore", "exceeded", "gated", "used", "n_gated", "n_valid", "overflow")
    assert BankGateReport._field_defaults == {} and "BankGateReport" in gpmdm_amd.__all__


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert ("int gpmdm_bank_set_gate(gpmdm_pf_t pf, const double* thresholds, double limit); "
            "/* F thresholds; all <= 0: off */") in text
    assert ("int gpmdm_bank_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream); "
            "/* arrays F x D, counts F */") in text
    dp = ctypes.POINTER(ctypes.c_double)
    assert _lib._SIGS["gpmdm_bank_set_gate"] == (ctypes.c_int, [ctypes.c_void_p, dp, ctypes.c_double])
    assert _lib._SIGS["gpmdm_bank_gate_report"] == _lib._SIGS["gpmdm_pf_gate_report"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_lib.GateOut), ctypes.c_void_p])
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS


def test_library_exports_the_symbols_and_rejects_null_arguments():
    """The built library carries the entry points; null arguments are refused before any HIP call."""
    from gpmdm_amd import _lib
    lib = _lib.load()
    thr = np.array([6.0])
    assert lib.gpmdm_bank_set_gate(None, _lib.dptr(thr), 0.5) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()
    assert lib.gpmdm_bank_gate_report(None, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <math.h>
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const set_gate)(gpmdm_pf_t, const double*, double) = gpmdm_bank_set_gate;
int (*const report)(gpmdm_pf_t, const gpmdm_gate_out*, void*) = gpmdm_bank_gate_report;
int use(gpmdm_pf_t bank, const double* z, double* zscore, uint8_t* gated, int64_t* n_gated, int32_t* overflow) {
  const double k[3] = {6.0, INFINITY, 3.0};        /* three filters; the second never rejects */
  const double off[3] = {0.0, 0.0, 0.0};
  gpmdm_gate_out out = {0};
  int rc = gpmdm_bank_set_predictive(bank, 1);
  if (rc == GPMDM_OK) rc = gpmdm_bank_set_gate(bank, k, 0.5);
  if (rc == GPMDM_OK) rc = gpmdm_pf_step(bank, z, NULL, NULL, NULL, NULL);
  out.zscore = zscore;                              /* 3 x D */
  out.gated = gated;                                /* 3 x D */
  out.n_gated = n_gated;                            /* 3 */
  out.overflow = overflow;                          /* 3 */
  if (rc == GPMDM_OK) rc = gpmdm_bank_gate_report(bank, &out, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_bank_set_gate(bank, off, 0.5);
  return rc;
}
"""


def test_c_caller_builds_against_the_header(tmp_path):
    user = tmp_path / "bank_gate_user.c"
    user.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(user),
                        "-o", str(tmp_path / "bank_gate_user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
