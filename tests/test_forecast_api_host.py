"""Host side of the forecast interface (no GPU): the header, the binding and a C99 caller agree
on gpmdm_pf_forecast; Python checks horizon and mode before it touches the library; and the
restated forecast switch draws (tests/forecast_ref.py) drive class fractions along the Markov
chain, which pins the counter layout on the CPU."""
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
    f._num_particles = 10
    monkeypatch.setattr(pfmod.GPMDM_PF, "_sync_model", touched)
    return f


def test_arguments_are_checked_before_the_library(bare_filter):
    f = bare_filter
    for bad in (0, -1, 4097, 2.5):
        with pytest.raises(ValueError, match="horizon"):
            f.forecast(bad)
    with pytest.raises(ValueError, match="mode"):
        f.forecast(3, mode="median")
    # good arguments pass the checks (and only then the library is reached)
    for kw in ({}, {"mode": "mean"}, {"mode": "sample", "observation": False, "particles": True}):
        with pytest.raises(AssertionError, match="touched"):
            f.forecast(4096, **kw)


def test_binding_matches_the_header():
    from gpmdm_amd import _lib
    text = " ".join(HEADER.read_text().split())
    assert ("int gpmdm_pf_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed, "
            "const gpmdm_forecast_out* out, void* stream);") in text
    assert "enum { GPMDM_FORECAST_SAMPLE = 0, GPMDM_FORECAST_MEAN = 1 };" in text
    assert ("typedef struct gpmdm_forecast_out { /* host arrays; any may be NULL */ double* class_prob; /* H x C */ "
            "double* state_mean; /* H x d */ double* obs_mean; /* H x D */ double* obs_spread; /* H x D */ "
            "double* states; /* H x P x d : the roll-out cloud after each step */ int64_t* classes; /* H x P */ "
            "} gpmdm_forecast_out;") in text
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    assert _lib._SIGS["gpmdm_pf_forecast"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                       ctypes.POINTER(_lib.ForecastOut), ctypes.c_void_p])
    assert _lib.ForecastOut._fields_ == [("class_prob", dp), ("state_mean", dp), ("obs_mean", dp),
                                         ("obs_spread", dp), ("states", dp), ("classes", ip)]
    assert (_lib.GPMDM_FORECAST_SAMPLE, _lib.GPMDM_FORECAST_MEAN) == (0, 1)
    assert f"#define GPMDM_FORECAST_MAX_HORIZON {_lib.GPMDM_FORECAST_MAX_HORIZON}" in text
    assert "forecast" not in _lib.STAGES                    # bench.py sums that table
    assert "gpmdm_pf_forecast" in _lib.EXPORTED_SYMBOLS


C_USER = r"""
#include <stddef.h>
#include "gpmdm_hip.h"
int (*const forecast)(gpmdm_pf_t, int, int, const uint64_t*, const gpmdm_forecast_out*, void*) = gpmdm_pf_forecast;
int use(gpmdm_pf_t pf, double* prob, double* pose, int64_t* classes) {
  const uint64_t seed = 11;
  gpmdm_forecast_out out = {0};
  int rc;
  out.class_prob = prob;
  out.obs_mean = pose;
  rc = gpmdm_pf_forecast(pf, 8, GPMDM_FORECAST_SAMPLE, NULL, &out, NULL);
  out.classes = classes;
  if (rc == GPMDM_OK) rc = gpmdm_pf_forecast(pf, GPMDM_FORECAST_MAX_HORIZON, GPMDM_FORECAST_MEAN, &seed, &out, NULL);
  return rc;
}
"""


def test_c_user_builds_against_the_header(tmp_path):
    src = tmp_path / "user.c"
    src.write_text(C_USER)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", "-c", str(src),
                        "-o", str(tmp_path / "user.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("T", [[[.9, .1], [.1, .9]],
                               [[.8, .15, .05], [.1, .8, .1], [.25, .05, .7]]])
def test_class_chain_follows_the_markov_matrix(T):
    """P = 20 000 particles starting in class 0, switched eight times by the restated forecast
    draws (seed 7, frame 0): the class fractions after h steps stay within 4 binomial standard
    deviations, 4 sqrt(p (1 - p) / P), of row 0 of T^h."""
    import forecast_ref as R
    T = np.asarray(T, dtype=np.float64)
    P, C = 20_000, T.shape[0]
    cls = np.zeros(P, dtype=np.int64)
    Th = np.eye(C)
    for h in range(1, 9):
        cls = R.switch_step(cls, T, 7, 0, h)
        Th = Th @ T
        frac, p = np.bincount(cls, minlength=C) / P, Th[0]
        sig = np.sqrt(p * (1 - p) / P)
        print(h, np.max(np.abs(frac - p) / sig))
        assert np.all(np.abs(frac - p) <= 4 * sig), (h, frac, p)


def test_forecast_draws_are_their_own_streams():
    """The forecast counters share nothing with the filter's own streams or with each other:
    other steps, frames and seeds give other draws; the filter's switch draws differ too."""
    import forecast_ref as R
    from oracle import philox as ph
    a = R.switch_draws(7, 3, 1, 64, 3)
    assert a.shape == (64, 3) and np.all(a > 0)
    for other in (R.switch_draws(7, 3, 2, 64, 3), R.switch_draws(7, 4, 1, 64, 3), R.switch_draws(8, 3, 1, 64, 3),
                  ph.switch_draws(7, 3, 64, 3)):
        assert not np.any(a == other)
    n = R.dynamics_normals(7, 3, 1, 64, 3)
    assert n.shape == (64, 3)
    assert not np.any(n == ph.dynamics_normals(7, 3, 64, 3))
    # odd d: the second normal of the last pair is dropped, the first columns are unchanged
    assert np.array_equal(R.dynamics_normals(7, 3, 1, 64, 4)[:, :3], n)
