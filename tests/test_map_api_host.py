"""Host side of the MAP decoder's interface (no GPU): Python checks the arguments, the particle cap,
the shard refusal and "recording is off" before it touches the library, and the header, the
binding and a C99 caller agree on gpmdm_pf_set_map / gpmdm_pf_map_recording / gpmdm_map_step /
gpmdm_pf_map_path / gpmdm_map_out."""
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
    f._map_path = True
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    return f


def test_arguments_are_checked_before_the_library(bare_filter):
    f = bare_filter
    for bad in (0, -1, 4097, 2.5, True, "3", (1, 2), [1]):
        with pytest.raises(ValueError, match="lag"):
            f.map_path(bad)
    for lag in (None, 1, 4, 4096):
        with pytest.raises(AssertionError, match="touched"):
            f.map_path(lag, particles=True)
    # the cap: 2^36 pairs per step, P = 262144 is the last size served
    f._num_particles = 262_145
    with pytest.raises(ValueError, match="262144"):
        f.map_path()
    f._num_particles = 262_144
    with pytest.raises(AssertionError, match="touched"):
        f.map_path()
    # sharded filters (a world above one, or peers of a devices= filter)
    f._world = 2
    with pytest.raises(ValueError, match="one rank"):
        f.map_path()
    with pytest.raises(ValueError, match="one rank"):
        f.set_map_path(True)
    f._world, f._peers = 1, [(None, 0)]
    with pytest.raises(ValueError, match="one rank"):
        f.map_path()
    f._peers = []
    f._map_path = False
    assert f.map_recording is False
    with pytest.raises(ValueError, match="recording is off"):
        f.map_path()
    f._map_path = True
    f._smoothing_lag = 0
    with pytest.raises(ValueError, match="smoothing is off"):
        f.map_path()
    with pytest.raises(ValueError, match="smoothing is off"):
        f.set_map_path(True)


def test_the_constructor_refuses_before_the_library(monkeypatch):
    from gpmdm_amd import GPMDM_PF, _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    model = types.SimpleNamespace(n_classes=2, set_evaluation_mode=touched)
    with pytest.raises(ValueError, match="smoothing_lag"):
        GPMDM_PF(model, np.eye(2), 10, map_path=True)
    with pytest.raises(ValueError, match="one rank"):
        GPMDM_PF(model, np.eye(2), 10, smoothing_lag=2, map_path=True, shard=(2, 0))


def test_banks_do_not_offer_it():
    from gpmdm_amd import GPMDM_PF_Bank
    for name in ("map_path", "set_map_path", "map_recording"):
        assert not hasattr(GPMDM_PF_Bank, name)


def test_map_step_checks_its_arrays_first(monkeypatch):
    from gpmdm_amd import _lib, map_step

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    model = types.SimpleNamespace(d=2, n_classes=2, device="cpu", handle=None)
    T = np.full((2, 2), 0.5)
    Xs, cs, Xt, ct = np.zeros((3, 2)), np.zeros(3, dtype=np.int64), np.zeros((4, 2)), np.ones(4, dtype=np.int64)
    bad = [dict(T=np.zeros((3, 3))), dict(Xs=np.zeros((3, 3))), dict(Xt=np.zeros(4)), dict(cs=np.zeros(2, dtype=np.int64)),
           dict(ct=np.full(4, 2)), dict(cs=np.full(3, -1)), dict(cs=np.zeros(3)), dict(ll=np.ones(3)),
           dict(delta=np.ones(4)), dict(Xs=np.zeros((0, 2)), cs=np.zeros(0, dtype=np.int64))]
    for kw in bad:
        args = dict(T=T, Xs=Xs, cs=cs, Xt=Xt, ct=ct, delta=None, ll=None)
        args.update(kw)
        with pytest.raises(ValueError):
            map_step(model, **args)


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    import gpmdm_amd
    text = " ".join(HEADER.read_text().split())
    assert "int gpmdm_pf_set_map(gpmdm_pf_t pf, int on);" in text
    assert "int gpmdm_pf_map_recording(gpmdm_pf_t pf, int* on);" in text
    assert ("int gpmdm_map_step(gpmdm_model_t model, const double* T, int64_t n_s, const double* Xs, "
            "const int64_t* cs, const double* delta_s, int64_t n_t, const double* Xt, const int64_t* ct, "
            "const double* ll_t, double* delta_out, int64_t* psi_out, void* stream);") in text
    assert "int gpmdm_pf_map_path(gpmdm_pf_t pf, int lag, const gpmdm_map_out* out, void* stream);" in text
    assert ("typedef struct gpmdm_map_out { /* host arrays; any may be NULL; n = lag + 1 */ "
            "int64_t* index; /* n: j*_l, the path's particle in slot l */ int64_t* classes; /* n */ "
            "double* states; /* n x d */ double* score; /* n: delta_l(j*_l) */ double* log_joint; /* 1 */ "
            "int64_t* distinct;") in text
    assert ("double* delta; /* n x P: delta_l per particle of slot l */ int64_t* backpointer; /* lag x P: psi_l per "
            "particle of slot l, an index into slot l + 1 */ } gpmdm_map_out;") in text
    dp, ip, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p
    assert _lib._SIGS["gpmdm_pf_set_map"] == (ctypes.c_int, [vp, ctypes.c_int])
    assert _lib._SIGS["gpmdm_pf_map_recording"] == (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int)])
    assert _lib._SIGS["gpmdm_map_step"] == (
        ctypes.c_int, [vp, dp, ctypes.c_int64, dp, ip, dp, ctypes.c_int64, dp, ip, dp, dp, ip, vp])
    assert _lib._SIGS["gpmdm_pf_map_path"] == (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(_lib.MapOut), vp])
    assert _lib.MapOut._fields_ == [("index", ip), ("classes", ip), ("states", dp), ("score", dp), ("log_joint", dp),
                                    ("distinct", ip), ("delta", dp), ("backpointer", ip)]
    assert "map" not in " ".join(_lib.STAGES)               # bench.py sums that table
    for name in ("gpmdm_pf_set_map", "gpmdm_pf_map_recording", "gpmdm_map_step", "gpmdm_pf_map_path"):
        assert name in _lib.EXPORTED_SYMBOLS
    for name in ("map_step", "MapPath"):
        assert name in gpmdm_amd.__all__ and hasattr(gpmdm_amd, name)


def test_library_exports_the_symbols_and_rejects_null_handles():
    from gpmdm_amd import _lib
    lib = _lib.load()
    assert lib.gpmdm_pf_map_path(None, 1, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()
    assert lib.gpmdm_pf_set_map(None, 1) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_map_recording(None, None) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_map_step(None, None, 1, None, None, None, 1, None, None, None, None, None, None) == \
        _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const set_map)(gpmdm_pf_t, int) = gpmdm_pf_set_map;
int (*const recording)(gpmdm_pf_t, int*) = gpmdm_pf_map_recording;
int (*const path)(gpmdm_pf_t, int, const gpmdm_map_out*, void*) = gpmdm_pf_map_path;
int (*const step)(gpmdm_model_t, const double*, int64_t, const double*, const int64_t*, const double*, int64_t,
                  const double*, const int64_t*, const double*, double*, int64_t*, void*) = gpmdm_map_step;
int use(gpmdm_model_t m, gpmdm_pf_t pf, const double* T, const double* X, const int64_t* c, double* delta,
        int64_t* psi, int64_t* index, double* states) {
  gpmdm_map_out out = {0};
  double log_joint = 0.0;
  int lag = 0, depth = 0, on = 0;
  int rc = gpmdm_pf_set_map(pf, 1);
  if (rc == GPMDM_OK) rc = gpmdm_pf_map_recording(pf, &on);
  if (rc == GPMDM_OK) rc = gpmdm_pf_smoothing_depth(pf, &lag, &depth);
  out.index = index;
  out.states = states;
  out.log_joint = &log_joint;
  out.backpointer = psi;
  if (rc == GPMDM_OK && on) rc = gpmdm_pf_map_path(pf, depth, &out, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_map_step(m, T, 4, X, c, NULL, 4, X, c, NULL, delta, psi, NULL);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
