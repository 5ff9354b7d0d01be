"""Host side of the marginal backward smoother's interface (no GPU): Python checks the arguments,
the particle cap and the shard refusal before it touches the library, and the header, the binding
and a C99 caller agree on gpmdm_backward_step / gpmdm_pf_smoothed_marginal / gpmdm_marginal_out."""
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
    f._world = 1
    f._h = None
    f._num_particles = 10
    f._smoothing_lag = 4
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    return f


def test_arguments_are_checked_before_the_library(bare_filter):
    f = bare_filter
    for bad in (-1, 4097, 2.5, True, "3", (1,), (1, 2, 3), (3, 1), (-1, 2), (0, 4097), (0, 1.5)):
        with pytest.raises(ValueError, match="lag"):
            f.smoothed_marginal(bad)
    for lag in (None, 0, 4, (0, 4), [2, 2], 4096):
        with pytest.raises(AssertionError, match="touched"):
            f.smoothed_marginal(lag, particles=True)
    # the cap: 2^36 pairs per step, P = 262144 is the last size served
    f._num_particles = 262_145
    with pytest.raises(ValueError, match="262144"):
        f.smoothed_marginal()
    f._num_particles = 262_144
    with pytest.raises(AssertionError, match="touched"):
        f.smoothed_marginal()
    # sharded filters (a world above one, or peers of a devices= filter)
    f._world = 2
    with pytest.raises(ValueError, match="one rank"):
        f.smoothed_marginal()
    f._world, f._peers = 1, [(None, 0)]
    with pytest.raises(ValueError, match="one rank"):
        f.smoothed_marginal()
    f._peers = []
    f._smoothing_lag = 0
    with pytest.raises(ValueError, match="smoothing is off"):
        f.smoothed_marginal()


def test_banks_do_not_offer_it():
    from gpmdm_amd import GPMDM_PF_Bank
    assert not hasattr(GPMDM_PF_Bank, "smoothed_marginal")


def test_backward_step_checks_its_arrays_first(monkeypatch):
    from gpmdm_amd import _lib, backward_step

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    model = types.SimpleNamespace(d=2, n_classes=2, device="cpu", handle=None)
    T = np.full((2, 2), 0.5)
    Xs, cs, Xt, ct, wt = np.zeros((3, 2)), np.zeros(3, dtype=np.int64), np.zeros((4, 2)), np.ones(4, dtype=np.int64), np.ones(4)
    bad = [dict(T=np.zeros((3, 3))), dict(Xs=np.zeros((3, 3))), dict(Xt=np.zeros(4)), dict(cs=np.zeros(2, dtype=np.int64)),
           dict(ct=np.full(4, 2)), dict(cs=np.full(3, -1)), dict(cs=np.zeros(3)), dict(wt=np.ones(3)),
           dict(a=np.ones(4)), dict(Xs=np.zeros((0, 2)), cs=np.zeros(0, dtype=np.int64))]
    for kw in bad:
        args = dict(T=T, Xs=Xs, cs=cs, Xt=Xt, ct=ct, wt=wt, a=None)
        args.update(kw)
        with pytest.raises(ValueError):
            backward_step(model, **args)


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    import gpmdm_amd
    text = " ".join(HEADER.read_text().split())
    assert ("int gpmdm_backward_step(gpmdm_model_t model, const double* T, int64_t n_s, const double* Xs, "
            "const int64_t* cs, const double* a, int64_t n_t, const double* Xt, const int64_t* ct, const double* wt, "
            "double* ws_out, double* log_den_out, void* stream);") in text
    assert ("int gpmdm_pf_smoothed_marginal(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_marginal_out* out, "
            "void* stream);") in text
    assert ("typedef struct gpmdm_marginal_out { /* host arrays; any may be NULL; n = lag_last - lag_first + 1 */ "
            "double* class_prob; /* n x C */ double* state_mean; /* n x d */ double* mass; /* n */ double* ess; /* n */ "
            "double* ess_distinct; /* n */ double* weights; /* n x P */ } gpmdm_marginal_out;") in text
    dp, ip, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p
    assert _lib._SIGS["gpmdm_backward_step"] == (
        ctypes.c_int, [vp, dp, ctypes.c_int64, dp, ip, dp, ctypes.c_int64, dp, ip, dp, dp, dp, vp])
    assert _lib._SIGS["gpmdm_pf_smoothed_marginal"] == (
        ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_lib.MarginalOut), vp])
    assert _lib.MarginalOut._fields_ == [("class_prob", dp), ("state_mean", dp), ("mass", dp), ("ess", dp),
                                         ("ess_distinct", dp), ("weights", dp)]
    assert _lib.GPMDM_BACKSMOOTH_MAX_PAIRS == 2 ** 36 == 262_144 ** 2
    assert "smooth" not in " ".join(_lib.STAGES)            # bench.py sums that table
    for name in ("gpmdm_backward_step", "gpmdm_pf_smoothed_marginal"):
        assert name in _lib.EXPORTED_SYMBOLS
    for name in ("backward_step", "MarginalSmoothed"):
        assert name in gpmdm_amd.__all__ and hasattr(gpmdm_amd, name)


def test_library_exports_the_symbols_and_rejects_null_handles():
    from gpmdm_amd import _lib
    lib = _lib.load()
    assert lib.gpmdm_pf_smoothed_marginal(None, 0, 0, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()
    assert lib.gpmdm_backward_step(None, None, 1, None, None, None, 1, None, None, None, None, None, None) == \
        _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const marginal)(gpmdm_pf_t, int, int, const gpmdm_marginal_out*, void*) = gpmdm_pf_smoothed_marginal;
int (*const step)(gpmdm_model_t, const double*, int64_t, const double*, const int64_t*, const double*, int64_t,
                  const double*, const int64_t*, const double*, double*, double*, void*) = gpmdm_backward_step;
int use(gpmdm_model_t m, gpmdm_pf_t pf, const double* T, const double* X, const int64_t* c, double* w, double* ess) {
  gpmdm_marginal_out out = {0};
  int lag = 0, depth = 0;
  int rc = gpmdm_pf_smoothing_depth(pf, &lag, &depth);
  out.ess_distinct = ess;
  out.weights = w;
  if (rc == GPMDM_OK) rc = gpmdm_pf_smoothed_marginal(pf, 0, depth, &out, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_backward_step(m, T, 4, X, c, NULL, 4, X, c, w, w, NULL, NULL);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
