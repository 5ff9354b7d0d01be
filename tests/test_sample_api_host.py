"""Host side of backward simulation's interface (no GPU): Python checks the arguments, the pair
cap, the shard refusal and "smoothing is off" before it touches the library, and the header, the
binding and a C99 caller agree on gpmdm_backward_sample_step / gpmdm_pf_sample_trajectories /
gpmdm_sample_out."""
import ctypes
import re
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
    for bad in (0, -1, 2 ** 31, 2.5, True, "3", None, (1, 2)):
        with pytest.raises(ValueError, match="n must be"):
            f.sample_trajectories(bad)
    for bad in (0, -1, 4097, 2.5, True, "3", (1, 2), [1]):
        with pytest.raises(ValueError, match="lag"):
            f.sample_trajectories(4, bad)
    for bad in (-1, 2 ** 64, 1.5, True, "7"):
        with pytest.raises(ValueError, match="seed"):
            f.sample_trajectories(4, seed=bad)
    for n, lag in ((1, None), (300, 1), (4, 4096)):
        with pytest.raises(AssertionError, match="touched"):
            f.sample_trajectories(n, lag, seed=3, observation=True)
    # the cap: 2^36 trajectory-particle pairs per step
    f._num_particles = 262_144
    with pytest.raises(ValueError, match=r"2\^36"):
        f.sample_trajectories(262_145)
    with pytest.raises(AssertionError, match="touched"):
        f.sample_trajectories(262_144)
    f._num_particles = 10
    # sharded filters (a world above one, or peers of a devices= filter)
    f._world = 2
    with pytest.raises(ValueError, match="one rank"):
        f.sample_trajectories(4)
    f._world, f._peers = 1, [(None, 0)]
    with pytest.raises(ValueError, match="one rank"):
        f.sample_trajectories(4)
    f._peers = []
    f._smoothing_lag = 0
    with pytest.raises(ValueError, match="smoothing is off"):
        f.sample_trajectories(4)


def test_banks_do_not_offer_it():
    from gpmdm_amd import GPMDM_PF_Bank
    assert not hasattr(GPMDM_PF_Bank, "sample_trajectories")


def test_the_step_checks_its_arrays_first(monkeypatch):
    from gpmdm_amd import _lib, backward_sample_step

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", touched)
    model = types.SimpleNamespace(d=2, n_classes=2, device="cpu", handle=None)
    T = np.full((2, 2), 0.5)
    Xs, cs, Xt, ct = np.zeros((3, 2)), np.zeros(3, dtype=np.int64), np.zeros((4, 2)), np.ones(4, dtype=np.int64)
    u = np.full(4, 0.5)
    bad = [dict(T=np.zeros((3, 3))), dict(Xs=np.zeros((3, 3))), dict(Xt=np.zeros(4)), dict(cs=np.zeros(2, dtype=np.int64)),
           dict(ct=np.full(4, 2)), dict(cs=np.full(3, -1)), dict(cs=np.zeros(3)), dict(u=np.ones(3) / 2),
           dict(u=np.array([0.1, 0.2, 1.0, 0.3])), dict(u=np.array([0.1, -0.2, 0.5, 0.3])),
           dict(u=np.array([0.1, np.nan, 0.5, 0.3])), dict(a=np.ones(4)),
           dict(Xs=np.zeros((0, 2)), cs=np.zeros(0, dtype=np.int64))]
    for kw in bad:
        args = dict(T=T, Xs=Xs, cs=cs, Xt=Xt, ct=ct, u=u, a=None)
        args.update(kw)
        with pytest.raises(ValueError):
            backward_sample_step(model, **args)


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    import gpmdm_amd
    text = " ".join(HEADER.read_text().split())
    assert ("int gpmdm_backward_sample_step(gpmdm_model_t model, const double* T, int64_t n_s, const double* Xs, "
            "const int64_t* cs, const double* a, int64_t n_t, const double* Xt, const int64_t* ct, const double* u, "
            "int64_t* idx_out, double* log_den_out, void* stream);") in text
    assert ("int gpmdm_pf_sample_trajectories(gpmdm_pf_t pf, int64_t n, int lag, const uint64_t* seed, "
            "const gpmdm_sample_out* out, void* stream);") in text
    assert f"#define GPMDM_BACKSAMPLE_RANGE {_lib.GPMDM_BACKSAMPLE_RANGE} " in text
    fields = ["int64_t* index;", "int64_t* classes;", "double* states;", "double* class_prob;", "double* state_mean;",
              "int64_t* alive;", "int64_t* distinct;", "double* obs_mean;", "double* obs_spread;"]
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct gpmdm_sample_out {"):text.index("} gpmdm_sample_out;")])
    at = [body.index(f) for f in fields]
    assert at == sorted(at) and body.count(";") == len(fields)
    dp, ip, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p
    assert _lib._SIGS["gpmdm_backward_sample_step"] == (
        ctypes.c_int, [vp, dp, ctypes.c_int64, dp, ip, dp, ctypes.c_int64, dp, ip, dp, ip, dp, vp])
    assert _lib._SIGS["gpmdm_pf_sample_trajectories"] == (
        ctypes.c_int, [vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_lib.SampleOut), vp])
    assert _lib.SampleOut._fields_ == [("index", ip), ("classes", ip), ("states", dp), ("class_prob", dp),
                                       ("state_mean", dp), ("alive", ip), ("distinct", ip), ("obs_mean", dp),
                                       ("obs_spread", dp)]
    assert "trajector" not in " ".join(_lib.STAGES)         # bench.py sums that table
    for name in ("gpmdm_backward_sample_step", "gpmdm_pf_sample_trajectories"):
        assert name in _lib.EXPORTED_SYMBOLS
    for name in ("backward_sample_step", "SampledTrajectories"):
        assert name in gpmdm_amd.__all__ and hasattr(gpmdm_amd, name)
    assert hasattr(gpmdm_amd.GPMDM_PF, "sample_trajectories")


def test_library_exports_the_symbols_and_rejects_null_handles():
    from gpmdm_amd import _lib
    lib = _lib.load()
    assert lib.gpmdm_pf_sample_trajectories(None, 1, 1, None, None, None) == _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()
    assert lib.gpmdm_backward_sample_step(None, None, 1, None, None, None, 1, None, None, None, None, None, None) == \
        _lib.GPMDM_E_INVALID
    assert b"null" in lib.gpmdm_last_error()


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const sample)(gpmdm_pf_t, int64_t, int, const uint64_t*, const gpmdm_sample_out*, void*) =
    gpmdm_pf_sample_trajectories;
int (*const step)(gpmdm_model_t, const double*, int64_t, const double*, const int64_t*, const double*, int64_t,
                  const double*, const int64_t*, const double*, int64_t*, double*, void*) = gpmdm_backward_sample_step;
int use(gpmdm_model_t m, gpmdm_pf_t pf, const double* T, const double* X, const int64_t* c, const double* u,
        int64_t* index, int64_t* classes, double* states, double* rows, int64_t* counts, double* pose) {
  gpmdm_sample_out out = {0};
  const uint64_t seed = 42;
  double log_den[GPMDM_BACKSAMPLE_RANGE > 4 ? 4 : 1];
  int lag = 0, depth = 0;
  int rc = gpmdm_pf_smoothing_depth(pf, &lag, &depth);
  out.index = index;
  out.classes = classes;
  out.states = states;
  out.class_prob = rows;
  out.state_mean = rows + 64;
  out.alive = counts;
  out.distinct = counts + 64;
  out.obs_mean = pose;
  out.obs_spread = pose + 4096;
  if (rc == GPMDM_OK) rc = gpmdm_pf_sample_trajectories(pf, 16, depth, &seed, &out, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_pf_sample_trajectories(pf, 16, depth, NULL, NULL, NULL);
  if (rc == GPMDM_OK) rc = gpmdm_backward_sample_step(m, T, 4, X, c, NULL, 4, X, c, u, index, log_den, NULL);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
