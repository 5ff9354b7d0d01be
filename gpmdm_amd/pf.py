"""GPMDM_PF -- drop-in mirror of ``/root/reference/gpmdm/gpmdm_pf.py`` on libgpmdm_hip.

Same constructor, methods and properties as the reference class (gpmdm_pf.py:47-312);
every per-frame computation runs in the HIP library.  Extra keyword options:

* ``rng='torch'`` (default): the random draws come from torch's global CPU generator in
  exactly the reference's order (``gpmdm_amd.replay``), so ``torch.manual_seed(s)``
  reproduces the reference's sampling; ``rng='philox'`` draws on the device (no host
  work per frame; the bench mode);
* ``seed``: Philox key (default: drawn from torch's generator);
* ``resample='multinomial'`` (reference, gpmdm_pf.py:211) or ``'systematic'``;
* ``process_group``: a ``torch.distributed`` group to shard particles over (one process
  per GPU; per frame, the new {class, state} rows are all-gathered while the observation GP
  runs and the likelihoods after it).  The Philox seed and
  the initial particles are broadcast from the group's rank 0, so every rank holds the
  same replicated filter whatever its local torch RNG state; replay mode (``rng='torch'``)
  consumes the host generator on every rank and therefore requires identical torch RNG
  states on all ranks (checked at construction: ``ValueError`` otherwise);
* ``devices=[d0, d1, ...]``: one process drives one rank per GPU (SURVEY §5's config row;
  a notebook uses several GPUs without torchrun): a library handle per device on the
  model's image there (``GPMDM.handle_on``), communicators made together
  (``gpmdm_comm_init_all``), and per frame every rank's stages with their all-gathers grouped
  (``gpmdm_pf_propagate_multi``); rank r owns ``device_shard_plan``'s particle range.  The
  read-outs and exports come from rank 0 (the filter is replicated).  ``devices=[0]`` is the
  plain filter bit for bit.  ``transport='loopback'`` (tests) swaps RCCL for the library's
  in-process loopback communicators (``gpmdm_comm_init_loopback``), which also accept a
  device repeated, e.g. ``devices=[0] * 8``: the multi-rank exchange on one GPU;
* ``shard=(world, rank)``: sharding with a caller-driven exchange (``exchange=`` or the
  staged calls); a Philox filter then needs an explicit ``seed`` (nothing to broadcast).
  ``exchange(recv, send)`` is called twice per frame: with the (P x (d+1)) / (P_r x (d+1))
  ``{class, state[d]}`` rows after the dynamics GP, then with the (P x 1) / (P_r x 1)
  ``{ll}`` column after the observation GP;
* ``dedup`` (default True): evaluate the dynamics GP once per distinct (resampling
  ancestor, new class) pair -- offspring of one ancestor hold bit-identical states -- and
  share the result; bitwise identical to ``dedup=False`` (every particle evaluated) with
  the same dynamics tile shape (``dyn_tiles``).
* ``shard_order`` (default True; multi-rank philox filters): each rank evaluates a slice of
  the particles ordered by resampling ancestor rather than a slice of particle indices, so
  de-duplication keeps ~1/R of the distinct keys per rank; bitwise identical either way.
* ``set_comm(comm)``: hand the library an RCCL communicator (``gpmdm_amd.RcclComm`` or
  any ncclComm_t of ``shard=(world, rank)``'s ranks); ``update`` then exchanges the rows
  itself (``gpmdm_pf_set_comm``: both all-gathers on a library-owned stream, the first
  overlapping the observation GP), the native hosts' path -- no torch.distributed.
* ``dyn_tiles`` (``'auto'``): tile shape of the dynamics-GP pass (``gpmdm_pf_set_dyn_tiles``):
  narrow tiles for de-duplicated rows, wide ones when every particle is evaluated; for
  d <= 12 the two are bitwise identical, above it they differ in summation order only.

Reference quirks kept for parity: log variance counted twice in the
log-likelihood, float32 ``ln 2pi``, non-recursive weights, read-outs pairing
post-resample classes/states with pre-resample weights, ``ll + log_w`` in the posterior,
``log_likelihood()`` returning a sum of exponentials, ``dyn_target`` ignored.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, replay
from .model import GPMDM


# Replay filters from this many particles draw torch's streams as parallel chunks
# (replay.ParallelFrameDraws); below it the serial draws cost less than the threads' hand-offs.
PARALLEL_REPLAY_P = 16384


def device_shard_plan(P: int, devices, repeat: bool = False) -> list:
    """(device, rank, lo, hi) of a one-process multi-device filter (GPMDM_PF(devices=...)):
    rank r runs on devices[r] and owns particles [r P / R, (r + 1) P / R) -- the library's
    own shard rule (gpmdm_pf_create), so the filter is bitwise the one-rank filter's.
    ``repeat``: a device may hold several ranks (the loopback transport; tests)."""
    devs = [int(x) for x in devices]
    if not devs:
        raise ValueError("devices must name at least one GPU")
    if not repeat and len(set(devs)) != len(devs):
        raise ValueError(f"devices must be distinct (one rank per GPU; RCCL refuses two on one device): {devs}")
    if any(x < 0 for x in devs):
        raise ValueError(f"bad device index in {devs}")
    R = len(devs)
    return [(dev, r, P * r // R, P * (r + 1) // R) for r, dev in enumerate(devs)]


@dataclass
class Forecast:
    """``GPMDM_PF.forecast``'s result; row h - 1 is h frames ahead."""
    class_probabilities: torch.Tensor                   # (H, C)
    state_mean: torch.Tensor                            # (H, d)
    observation_mean: Optional[torch.Tensor] = None     # (H, D)
    observation_spread: Optional[torch.Tensor] = None   # (H, D)
    states: Optional[torch.Tensor] = None               # (H, P, d)
    classes: Optional[torch.Tensor] = None              # (H, P) int64


@dataclass
class Smoothed:
    """``GPMDM_PF.smoothed``'s result; row i is lag ``lags[i]``, i.e. frame ``frames[i]``."""
    lags: torch.Tensor                                  # (n,) int64
    frames: torch.Tensor                                # (n,) int64: frame - lag
    class_probabilities: torch.Tensor                   # (n, C)
    state_mean: torch.Tensor                            # (n, d)
    distinct_ancestors: torch.Tensor                    # (n,) int64
    observation_mean: Optional[torch.Tensor] = None     # (n, D)
    observation_spread: Optional[torch.Tensor] = None   # (n, D)
    ancestors: Optional[torch.Tensor] = None            # (n, P) int64
    states: Optional[torch.Tensor] = None               # (n, P, d)
    classes: Optional[torch.Tensor] = None              # (n, P) int64


@dataclass
class MarginalSmoothed:
    """``GPMDM_PF.smoothed_marginal``'s result; row i is lag ``lags[i]``, i.e. frame ``frames[i]``.
    ``ess`` counts copies of a resampled particle as support and is flattered by them;
    ``ess_distinct`` is the effective number of distinct support points, to be read beside
    ``Smoothed.distinct_ancestors``."""
    lags: torch.Tensor                                  # (n,) int64
    frames: torch.Tensor                                # (n,) int64: frame - lag
    class_probabilities: torch.Tensor                   # (n, C)
    state_mean: torch.Tensor                            # (n, d)
    mass: torch.Tensor                                  # (n,)  1 to rounding; never renormalised
    ess: torch.Tensor                                   # (n,)
    ess_distinct: torch.Tensor                          # (n,)
    weights: Optional[torch.Tensor] = None              # (n, P): of frame - lag's recorded cloud


@dataclass
class MapPath:
    """``GPMDM_PF.map_path``'s result; row l is lag ``lags[l]`` = l, i.e. frame ``frames[l]``.
    ``indices[l]`` is the path's particle in frame ``frames[l]``'s recorded cloud (``export_state``'s
    order), ``scores[l]`` its delta_l, ``log_joint`` = ``scores[0]``; ``distinct[l]`` the distinct
    resampling ancestors of that cloud -- the rows the recursion ran on.  With ``log_joint`` = -inf
    the unreachable rows hold index and class -1, NaN states and score -inf."""
    lags: torch.Tensor                                  # (n,) int64
    frames: torch.Tensor                                # (n,) int64: frame - lag
    indices: torch.Tensor                               # (n,) int64
    classes: torch.Tensor                               # (n,) int64
    states: torch.Tensor                                # (n, d)
    scores: torch.Tensor                                # (n,)
    log_joint: float
    distinct: torch.Tensor                              # (n,) int64
    delta: Optional[torch.Tensor] = None                # (n, P)
    backpointers: Optional[torch.Tensor] = None         # (n - 1, P) int64: into the next lag's cloud
    observation_mean: Optional[torch.Tensor] = None     # (n, D)


@dataclass
class SampledTrajectories:
    """``GPMDM_PF.sample_trajectories``'s result; row l is lag ``lags[l]`` = l, i.e. frame ``frames[l]``.
    ``indices[l, m]`` is trajectory m's particle in frame ``frames[l]``'s recorded cloud
    (``export_state``'s order).  A trajectory that no particle of an older frame reaches is dead from
    there on: index and class -1, NaN states; ``alive[l]`` counts the others, over which the row's
    fractions, mean and pose are taken (NaN when none is left), and ``distinct[l]`` the distinct
    particles they sit on."""
    lags: torch.Tensor                                  # (L + 1,) int64
    frames: torch.Tensor                                # (L + 1,) int64: frame - lag
    indices: torch.Tensor                               # (L + 1, n) int64
    classes: torch.Tensor                               # (L + 1, n) int64
    states: torch.Tensor                                # (L + 1, n, d)
    class_probabilities: torch.Tensor                   # (L + 1, C)
    state_mean: torch.Tensor                            # (L + 1, d)
    alive: torch.Tensor                                 # (L + 1,) int64
    distinct: torch.Tensor                              # (L + 1,) int64
    observation_mean: Optional[torch.Tensor] = None     # (L + 1, D)
    observation_spread: Optional[torch.Tensor] = None   # (L + 1, D)


def _step_arrays(model, T, Xs, cs, Xt, ct, name):
    """The arrays ``backward_step`` and ``map_step`` share, checked: (arr, T, Xs, cs, Xt, ct)."""
    d, C = int(model.d), int(model.n_classes)

    def arr(x, shape, what, dtype=np.float64):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        x = np.asarray(x)
        if dtype is np.int64 and x.dtype.kind not in "iu":
            raise ValueError(f"{what} must hold integers, got dtype {x.dtype}")
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.ndim != len(shape) or any(s is not None and s != n for s, n in zip(shape, x.shape)):
            raise ValueError(f"{what} must have shape {tuple('n' if s is None else s for s in shape)}, got {x.shape}")
        return x

    Tm = arr(T, (C, C), "T")
    Xs_, Xt_ = arr(Xs, (None, d), "Xs"), arr(Xt, (None, d), "Xt")
    n_s, n_t = Xs_.shape[0], Xt_.shape[0]
    if n_s < 1 or n_t < 1:
        raise ValueError(f"{name} needs at least one source and one target")
    cs_, ct_ = arr(cs, (n_s,), "cs", np.int64), arr(ct, (n_t,), "ct", np.int64)
    for what, c in (("cs", cs_), ("ct", ct_)):
        if c.min() < 0 or c.max() >= C:
            raise ValueError(f"{what} must lie in [0, {C})")
    if n_s * n_t > _lib.GPMDM_BACKSMOOTH_MAX_PAIRS:
        raise ValueError(f"{name} serves up to 2^36 source-target pairs, got {n_s} x {n_t}")
    return arr, Tm, Xs_, cs_, Xt_, ct_


def map_step(model, T, Xs, cs, Xt, ct, delta=None, ll=None):
    """One step of the MAP trajectory recursion (gpmdm_map_step): sources ``Xs`` (n_s, d), ``cs`` with
    scores ``delta`` (None: zeros), targets ``Xt`` (n_t, d), ``ct`` with observation log-likelihoods
    ``ll`` (None: zeros), transition density ``backward_step``'s f.  Returns ``(delta, backpointers)``
    as CPU tensors: ``delta[j] = ll[j] + max_k [delta[k] + log f(k -> j)]`` and the lowest k attaining
    it (-inf and -1 when no source reaches j or ``ll[j]`` is not finite).  Natural logarithms; the
    rows are used as given (no de-duplication).  A pure, bit-reproducible function of its inputs."""
    arr, Tm, Xs_, cs_, Xt_, ct_ = _step_arrays(model, T, Xs, cs, Xt, ct, "map_step")
    n_s, n_t = Xs_.shape[0], Xt_.shape[0]
    d_ = None if delta is None else arr(delta, (n_s,), "delta")
    l_ = None if ll is None else arr(ll, (n_t,), "ll")
    out, psi = np.zeros(n_t), np.zeros(n_t, dtype=np.int64)
    stream = ctypes.c_void_p(torch.cuda.current_stream(model.device).cuda_stream)
    _lib.check(_lib.load().gpmdm_map_step(model.handle, _lib.dptr(Tm), n_s, _lib.dptr(Xs_), _lib.i64ptr(cs_),
                                          _lib.dptr(d_), n_t, _lib.dptr(Xt_), _lib.i64ptr(ct_), _lib.dptr(l_),
                                          _lib.dptr(out), _lib.i64ptr(psi), stream), "map_step")
    return torch.from_numpy(out), torch.from_numpy(psi)


def backward_sample_step(model, T, Xs, cs, Xt, ct, u, a=None):
    """One step of backward simulation (gpmdm_backward_sample_step): sources ``Xs`` (n_s, d), ``cs``
    with filter weights ``a`` (None: 1 / n_s each), targets ``Xt`` (n_t, d), ``ct`` and one uniform
    ``u[j]`` in [0, 1) per target, transition density ``backward_step``'s f.  Returns ``(indices,
    log_den)`` as CPU tensors: ``indices[j]`` is the lowest k with ``sum_{i <= k} a_i f_ij > u_j D_j``
    (the sources in index order), ``log_den[j] = log D_j``, ``D_j = sum_k a_k f_kj``; -1 and -inf when
    no source reaches j.  A source of term zero is never returned.  A pure, bit-reproducible
    function of its inputs; target j's result does not depend on the other targets."""
    arr, Tm, Xs_, cs_, Xt_, ct_ = _step_arrays(model, T, Xs, cs, Xt, ct, "backward_sample_step")
    n_s, n_t = Xs_.shape[0], Xt_.shape[0]
    u_ = arr(u, (n_t,), "u")
    if not ((u_ >= 0) & (u_ < 1)).all():
        raise ValueError("u must lie in [0, 1)")
    a_ = None if a is None else arr(a, (n_s,), "a")
    idx, ld = np.zeros(n_t, dtype=np.int64), np.zeros(n_t)
    stream = ctypes.c_void_p(torch.cuda.current_stream(model.device).cuda_stream)
    _lib.check(_lib.load().gpmdm_backward_sample_step(model.handle, _lib.dptr(Tm), n_s, _lib.dptr(Xs_),
                                                      _lib.i64ptr(cs_), _lib.dptr(a_), n_t, _lib.dptr(Xt_),
                                                      _lib.i64ptr(ct_), _lib.dptr(u_), _lib.i64ptr(idx), _lib.dptr(ld),
                                                      stream), "backward_sample_step")
    return torch.from_numpy(idx), torch.from_numpy(ld)


def backward_step(model, T, Xs, cs, Xt, ct, wt, a=None):
    """One step of the marginal backward smoother (gpmdm_backward_step): sources ``Xs`` (n_s, d),
    ``cs`` with filter weights ``a`` (None: 1 / n_s each), targets ``Xt`` (n_t, d), ``ct`` with
    smoothing weights ``wt``, transition density f = T[c, c'] N(x'; mu_c'(x), v_c'(x)) with the
    moments of ``model.map_x_dynamics_for_class``.  Returns ``(weights, log_den)`` as CPU tensors:
    ``weights[i] = a_i sum_j wt_j f_ij / D_j`` and ``log_den[j] = log D_j``, ``D_j = sum_k a_k f_kj``
    (-inf, and the target's mass lost, when no source reaches j).  A pure, bit-reproducible
    function of its inputs."""
    arr, Tm, Xs_, cs_, Xt_, ct_ = _step_arrays(model, T, Xs, cs, Xt, ct, "backward_step")
    n_s, n_t = Xs_.shape[0], Xt_.shape[0]
    wt_ = arr(wt, (n_t,), "wt")
    a_ = None if a is None else arr(a, (n_s,), "a")
    ws, ld = np.zeros(n_s), np.zeros(n_t)
    stream = ctypes.c_void_p(torch.cuda.current_stream(model.device).cuda_stream)
    _lib.check(_lib.load().gpmdm_backward_step(model.handle, _lib.dptr(Tm), n_s, _lib.dptr(Xs_), _lib.i64ptr(cs_),
                                               _lib.dptr(a_), n_t, _lib.dptr(Xt_), _lib.i64ptr(ct_), _lib.dptr(wt_),
                                               _lib.dptr(ws), _lib.dptr(ld), stream), "backward_step")
    return torch.from_numpy(ws), torch.from_numpy(ld)


class Innovation(NamedTuple):
    """``GPMDM_PF.innovation``'s result (CPU tensors; a bank's carry a leading filter axis): how
    surprising each joint of the frame just weighed was, against the propagated (pre-resample,
    equally weighted) cloud.  With mu_pj the observation GP's mean at particle p, vc_p its
    ``variance_common`` and il2_j = lambda_j^-2, over the particles with vc_p > 0 (``n_valid``):
    ``gp_variance`` = il2_j mean_p vc_p, ``variance`` = ``spread`` + ``gp_variance``, ``residual`` =
    z_j - ``mean``_j, ``zscore`` = residual / sqrt(variance), ``log_density`` = log mean_p N(z_j;
    mu_pj, vc_p il2_j); the last three are NaN where ``observed`` is False."""
    mean: torch.Tensor                                  # (D,)
    spread: torch.Tensor                                # (D,)
    gp_variance: torch.Tensor                           # (D,)
    variance: torch.Tensor                              # (D,)
    residual: torch.Tensor                              # (D,)
    zscore: torch.Tensor                                # (D,)
    log_density: torch.Tensor                           # (D,)
    n_valid: torch.Tensor                               # () int64
    observed: torch.Tensor                              # (D,) bool
    states: Optional[torch.Tensor] = None               # (P, d)
    variance_common: Optional[torch.Tensor] = None      # (P,)


def _innovation_call(owner, entry, filters, particles):
    """``innovation`` of a filter (``filters`` = ()) or a bank ((F_local,)): the library's
    ``entry`` (its name; None for a bank without local filters) into host arrays with the leading
    shape ``filters``, returned as an ``Innovation``."""
    P, d, D = owner._num_particles, owner.latent_dim, owner.observation_dim
    f7 = [np.full(filters + (D,), np.nan) for _ in range(7)]
    nv = np.zeros(filters, dtype=np.int64)
    ob = np.zeros(filters + (D,), dtype=np.uint8)
    st = np.zeros(filters + (P, d)) if particles else None
    vc = np.zeros(filters + (P,)) if particles else None
    if entry is not None:
        owner._sync_model()
        out = _lib.InnovationOut(*[_lib.dptr(a) for a in f7], _lib.i64ptr(nv), ctypes.c_void_p(ob.ctypes.data),
                                 _lib.dptr(st), _lib.dptr(vc))
        _lib.check(getattr(_lib.load(), entry)(owner._h, ctypes.byref(out), owner._stream()), "innovation")
    t = lambda a: None if a is None else torch.from_numpy(a)   # noqa: E731
    return Innovation(*map(t, f7), torch.from_numpy(nv), torch.from_numpy(ob.astype(bool)), t(st), t(vc))


class GateReport(NamedTuple):
    """``GPMDM_PF.gate_report``'s result (CPU tensors and Python scalars): what the gate decided
    for the frame the last ``update`` weighed.  ``zscore`` is bitwise ``innovation().zscore`` of
    that frame (NaN where unobserved); ``exceeded`` = observed and |zscore| > ``threshold``;
    ``gated`` = ``exceeded`` when between 1 and floor(limit D_obs) joints exceeded, else empty
    (``overflow``: more did, and the frame was weighed as observed); ``used`` = observed and not
    ``gated``, the joints the frame's weights rest on."""
    threshold: float
    zscore: torch.Tensor                                # (D,)
    exceeded: torch.Tensor                              # (D,) bool
    gated: torch.Tensor                                 # (D,) bool
    used: torch.Tensor                                  # (D,) bool
    n_gated: int
    n_valid: int
    overflow: bool


def _check_gate(k, limit):
    """``gate`` (None: off) and ``gate_limit`` as floats; raised here, before the library is touched."""
    real = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))   # noqa: E731
    if not real(limit) or not 0.0 < float(limit) <= 1.0:
        raise ValueError(f"gate_limit must be a real number in (0, 1], got {limit!r}")
    if k is None:
        return None, float(limit)
    if not real(k) or not 0.0 < float(k) < float("inf"):
        raise ValueError(f"gate must be None or a finite real number > 0, got {k!r}")
    return float(k), float(limit)


class BankGateReport(NamedTuple):
    """``GPMDM_PF_Bank.gate_report``'s result (CPU tensors): ``GateReport`` with a leading axis over
    this rank's filters.  Row f is bitwise the single filter's report on filter f's frame;
    ``threshold`` is ``inf`` for a filter that never rejects, and a blacked-out filter's row is a
    blackout frame's (``zscore`` NaN, no flag set, ``n_valid`` 0)."""
    threshold: torch.Tensor                             # (F,)
    zscore: torch.Tensor                                # (F, D)
    exceeded: torch.Tensor                              # (F, D) bool
    gated: torch.Tensor                                 # (F, D) bool
    used: torch.Tensor                                  # (F, D) bool
    n_gated: torch.Tensor                               # (F,) int64
    n_valid: torch.Tensor                               # (F,) int64
    overflow: torch.Tensor                              # (F,) bool


def _check_bank_gate(gate, limit, F, f_lo, f_hi):
    """A bank's ``gate`` as a tuple over the filters [f_lo, f_hi) of F (entries: a float > 0, or
    None: that filter never rejects), or None (off), and ``gate_limit`` as a float; raised here,
    before the library is touched.  ``gate``: None, one real number > 0 for every filter, or a
    sequence of F (each rank takes its rows) or f_hi - f_lo (local) entries."""
    _, lim = _check_gate(None, limit)
    if gate is None:
        return None, lim
    Fl = f_hi - f_lo
    if isinstance(gate, (list, tuple)) or (isinstance(gate, np.ndarray) and gate.ndim == 1):
        ks = list(gate)
        if len(ks) == F and Fl != F:
            ks = ks[f_lo:f_hi]
        elif len(ks) != Fl:
            raise ValueError(f"gate must be None, one real number > 0 or a sequence of {F} (or {Fl} local) "
                             f"entries, got {len(ks)}")
        return tuple(None if k is None else _check_gate(k, lim)[0] for k in ks), lim
    return (_check_gate(gate, lim)[0],) * Fl, lim


def _check_smoothing_lag(L) -> int:
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)):
        raise ValueError(f"smoothing lag must be an integer, got {L!r}")
    if not 0 <= int(L) <= _lib.GPMDM_SMOOTH_MAX_LAG:
        raise ValueError(f"smoothing lag must be in [0, {_lib.GPMDM_SMOOTH_MAX_LAG}], got {L}")
    return int(L)


def _check_lag_range(lag):
    """``smoothed``'s ``lag`` as (first, last), last None for "up to the depth"."""
    def one(x):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) <= _lib.GPMDM_SMOOTH_MAX_LAG:
            raise ValueError(f"lag must be an integer in [0, {_lib.GPMDM_SMOOTH_MAX_LAG}], got {x!r}")
        return int(x)
    if lag is None:
        return 0, None
    if isinstance(lag, (tuple, list)):
        if len(lag) != 2:
            raise ValueError(f"lag must be None, an integer or a pair (first, last), got {lag!r}")
        a, b = one(lag[0]), one(lag[1])
        if a > b:
            raise ValueError(f"lag range must have first <= last, got {lag!r}")
        return a, b
    return one(lag), one(lag)


def _forecast_call(owner, entry, filters, horizon, mode, observation, particles, seed):
    """``forecast`` of a filter (``filters`` = ()) or a bank ((F_local,)): the argument checks, then
    the library's ``entry`` (its name; None for a bank without local filters) into host arrays
    with the library's leading shape (H, *filters).  Returns the six arrays in ``Forecast``'s
    order, None for those not asked for."""
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)):
        raise ValueError(f"horizon must be an integer, got {horizon!r}")
    H = int(horizon)
    if not 1 <= H <= _lib.GPMDM_FORECAST_MAX_HORIZON:
        raise ValueError(f"horizon must be in [1, {_lib.GPMDM_FORECAST_MAX_HORIZON}], got {H}")
    if mode not in _lib.FORECAST_MODES:
        raise ValueError(f"mode must be one of {sorted(_lib.FORECAST_MODES)}, got {mode!r}")
    P, C, d, D = owner._num_particles, owner.num_classes, owner.latent_dim, owner.observation_dim
    lead = (H, *filters)
    cp, sm = np.zeros(lead + (C,)), np.zeros(lead + (d,))
    om = np.zeros(lead + (D,)) if observation else None
    osp = np.zeros(lead + (D,)) if observation else None
    st = np.zeros(lead + (P, d)) if particles else None
    cl = np.zeros(lead + (P,), dtype=np.int64) if particles else None
    if entry is not None:
        owner._sync_model()
        out = _lib.ForecastOut(_lib.dptr(cp), _lib.dptr(sm), _lib.dptr(om), _lib.dptr(osp), _lib.dptr(st),
                               _lib.i64ptr(cl))
        sd = None if seed is None else ctypes.byref(ctypes.c_uint64(int(seed) & (2 ** 64 - 1)))
        _lib.check(getattr(_lib.load(), entry)(owner._h, H, _lib.FORECAST_MODES[mode], sd, ctypes.byref(out),
                                               owner._stream()), "forecast")
    return cp, sm, om, osp, st, cl


def _smoothed_call(owner, what, entry, filters, lag, observation, particles):
    """``smoothed`` of a filter (``filters`` = ()) or a bank ((F_local,)), ``what`` its name in the
    messages: the argument checks, then the library's ``entry`` (its name; None for a bank without
    local filters) into host arrays with the library's leading shape (n, *filters).  Returns the
    lags and the eight arrays that follow ``frames`` in ``Smoothed``, None for those not asked for."""
    first, last = _check_lag_range(lag)
    if not owner._smoothing_lag:
        raise ValueError(f"smoothing is off: build the {what} with smoothing_lag=L or call set_smoothing(L)")
    depth = owner.smoothing_depth
    if last is None:
        last = depth
    if last > depth:
        raise ValueError(f"lag {last} is above the recorded depth {depth} (smoothing lag {owner._smoothing_lag})")
    P, C, d, D = owner._num_particles, owner.num_classes, owner.latent_dim, owner.observation_dim
    lead = (last - first + 1, *filters)
    cp, sm, da = np.zeros(lead + (C,)), np.zeros(lead + (d,)), np.zeros(lead, dtype=np.int64)
    om = np.zeros(lead + (D,)) if observation else None
    osp = np.zeros(lead + (D,)) if observation else None
    an = np.zeros(lead + (P,), dtype=np.int64) if particles else None
    st = np.zeros(lead + (P, d)) if particles else None
    cl = np.zeros(lead + (P,), dtype=np.int64) if particles else None
    if entry is not None:
        out = _lib.SmoothedOut(_lib.dptr(cp), _lib.dptr(sm), _lib.i64ptr(da), _lib.dptr(om), _lib.dptr(osp),
                               _lib.i64ptr(an), _lib.dptr(st), _lib.i64ptr(cl))
        _lib.check(getattr(_lib.load(), entry)(owner._h, first, last, ctypes.byref(out), owner._stream()), "smoothed")
    return np.arange(first, last + 1, dtype=np.int64), (cp, sm, da, om, osp, an, st, cl)


def _as_f64_vector(z) -> np.ndarray:
    """The observation as a contiguous float64 vector (the reference casts it with
    torch.tensor(z, dtype=float64), gpmdm_pf.py:123; float32 -> float64 is exact)."""
    if isinstance(z, np.ndarray):
        return np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    return np.ascontiguousarray(torch.as_tensor(z, dtype=torch.float64).cpu().numpy().reshape(-1))


class GPMDM_PF:
    def __init__(self, gpmdm: GPMDM, markov_switching_model, num_particles: int, *,
                 rng: str = "torch", seed=None, resample: str = "multinomial", process_group=None,
                 shard=None, exchange=None, dedup: bool = True, shard_order: bool = True,
                 dyn_tiles: str = "auto", devices=None, obs_cutoff: bool = False, transport: str = "rccl",
                 smoothing_lag: int = 0, predictive: bool = False, gate=None, gate_limit: float = 0.5,
                 map_path: bool = False):
        self._smoothing_lag = _check_smoothing_lag(smoothing_lag)
        self._map_path = bool(map_path)
        if self._map_path and not self._smoothing_lag:
            raise ValueError("map_path=True needs smoothing_lag=L > 0 (the history it decodes)")
        if self._map_path and (process_group is not None or shard is not None or devices is not None):
            raise ValueError("map_path= serves single filters on one rank: no process_group, shard or devices")
        self._gate, self._gate_limit = _check_gate(gate, gate_limit)
        if self._gate is not None and (process_group is not None or shard is not None):
            raise ValueError("gate= serves single filters on one rank: no process_group or shard")
        self._predictive = bool(predictive) or self._gate is not None   # (the gate reads the frame's vc)
        self._gpmdm = gpmdm
        self._gpmdm.set_evaluation_mode()
        self._markov_switching_model = torch.as_tensor(markov_switching_model).type(self.dtype)
        self._num_particles = int(num_particles)
        if self._gpmdm.n_classes != self._markov_switching_model.size(0):
            raise ValueError("Number of classes in the GPMDM model and the Markov model do not match")
        if rng not in ("torch", "philox"):
            raise ValueError("rng must be 'torch' or 'philox'")
        if resample not in ("multinomial", "systematic"):
            raise ValueError("resample must be 'multinomial' or 'systematic'")
        self._rng = rng
        self._draws = None                      # replay.FrameDraws (rng='torch'), made on first use
        self._pre_sw = False                    # a replay pre-switch with the draws made ahead is pending
        self._n_staged = False                  # ... and the normals drawn ahead are on the device
        self._resample_mode = resample
        self._group = process_group
        self._exchange_fn = exchange
        self._devices = None
        if devices is not None:                 # one process, one handle per device (device_shard_plan)
            if process_group is not None or shard is not None or exchange is not None:
                raise ValueError("devices= drives every rank itself: no process_group, shard or exchange")
            if transport not in ("rccl", "loopback"):
                raise ValueError("transport must be 'rccl' or 'loopback'")
            self._devices = [p[0] for p in device_shard_plan(self._num_particles, devices,
                                                             repeat=transport == "loopback")]
            self._world, self._rank = len(self._devices), 0
        elif process_group is not None:
            import torch.distributed as dist
            self._world, self._rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        elif shard is not None:                 # (world, rank) with a caller-driven exchange
            self._world, self._rank = int(shard[0]), int(shard[1])
            if self._world > 1 and rng == "philox" and seed is None:
                raise ValueError("shard= with rng='philox' needs an explicit seed (identical on every rank)")
        else:
            self._world, self._rank = 1, 0
        if self._gate is not None and self._world > 1:
            raise ValueError("gate= serves single filters on one rank, not sharded filters")
        self._collective =process_group is not None and self._world > 1
        if self._collective and rng == "torch":
            from .distributed import identical_on_all_ranks
            if not identical_on_all_ranks(torch.get_rng_state().numpy().tobytes(), process_group, self.device):
                raise ValueError("rng='torch' on several ranks needs identical torch RNG states "
                                 "(torch.manual_seed with the same seed on every rank)")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if rng == "philox" else 0
        if self._collective and rng == "philox":
            from .distributed import broadcast_array
            seed = int(broadcast_array(np.array([seed], dtype=np.int64), process_group, self.device)[0])
        self._seed = int(seed)
        lib = _lib.load()
        T = np.ascontiguousarray(self._markov_switching_model.numpy(), dtype=np.float64)
        if dyn_tiles not in _lib.DYN_TILES:
            raise ValueError("dyn_tiles must be 'auto', 'narrow' or 'wide'")

        if isinstance(obs_cutoff, str) and obs_cutoff != "auto":
            raise ValueError("obs_cutoff: True, False or 'auto'")
        self._obs_cutoff = 3 if obs_cutoff == "auto" else (1 if obs_cutoff else 0)
        if obs_cutoff:
            gpmdm.enable_obs_cutoff(True)       # the model's cutoff image (built once)
        self._obs_skip = True                   # set_obs_skip

        def create(model_handle, rank):
            h = ctypes.c_void_p()
            _lib.check(lib.gpmdm_pf_create(
                model_handle, _lib.dptr(T), self._num_particles,
                _lib.GPMDM_RNG_REPLAY if rng == "torch" else _lib.GPMDM_RNG_PHILOX,
                ctypes.c_uint64(self._seed & (2 ** 64 - 1)),
                _lib.GPMDM_RESAMPLE_MULTINOMIAL if resample == "multinomial" else _lib.GPMDM_RESAMPLE_SYSTEMATIC,
                self._world, rank, ctypes.byref(h)), "GPMDM_PF")
            _lib.check(lib.gpmdm_pf_set_dedup(h, 1 if dedup else 0), "dedup")
            _lib.check(lib.gpmdm_pf_set_shard_order(h, 1 if shard_order else 0), "shard_order")
            _lib.check(lib.gpmdm_pf_set_dyn_tiles(h, _lib.DYN_TILES[dyn_tiles]), "dyn_tiles")
            if self._obs_cutoff:
                _lib.check(lib.gpmdm_pf_set_obs_cutoff(h, self._obs_cutoff), "obs_cutoff")
            if not self._obs_skip:
                _lib.check(lib.gpmdm_pf_set_obs_skip(h, 0), "obs_skip")
            if self._smoothing_lag:
                try:
                    _lib.check(lib.gpmdm_pf_set_smoothing(h, self._smoothing_lag), "smoothing_lag")
                except Exception:
                    lib.gpmdm_pf_destroy(h)     # (a history above the memory limit: no handle is left behind)
                    raise
            if self._map_path:
                try:
                    _lib.check(lib.gpmdm_pf_set_map(h, 1), "map_path")
                except Exception:
                    lib.gpmdm_pf_destroy(h)
                    raise
            if self._predictive:
                _lib.check(lib.gpmdm_pf_set_predictive(h, 1), "predictive")
            if self._gate is not None:
                _lib.check(lib.gpmdm_pf_set_gate(h, self._gate, self._gate_limit), "gate")
            return h

        self._peers = []                        # devices=: ranks 1.. as (handle, device index)
        self._comms = []
        if self._devices is None:
            self._h = create(gpmdm.handle, self._rank)
            self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        else:
            hs = [create(gpmdm.handle_on(dev), r) for r, dev in enumerate(self._devices)]
            self._h, self._dev_index = hs[0], self._devices[0]
            self._peers = list(zip(hs[1:], self._devices[1:]))
            # one communicator per device, made together (ncclCommInitAll); rank r on devices[r]
            # (transport='loopback': the library's in-process test transport, several ranks
            # per device allowed -- gpmdm_comm_init_loopback)
            n = len(self._devices)
            comms = (ctypes.c_void_p * n)()
            init = lib.gpmdm_comm_init_loopback if transport == "loopback" else lib.gpmdm_comm_init_all
            _lib.check(init(n, (ctypes.c_int * n)(*self._devices), comms), "gpmdm_comm_init")
            self._comms = [ctypes.c_void_p(c) for c in comms]
            for h, c in zip(hs, self._comms):
                _lib.check(lib.gpmdm_pf_set_comm(h, c, 0), "set_comm")
        self._model_gen = gpmdm.generation
        self._readout = None
        self._comm = self._comms[0] if self._comms else None
        # read-out landing buffers and their pointers, made once (read per frame)
        C, d = self.num_classes, self.latent_dim
        self._ro = (np.zeros(C), np.zeros(d), np.zeros(1))
        self._ro_ptr = tuple(_lib.dptr(a) for a in self._ro)
        if self._world > 1 and self._devices is None:
            h = self._h
            w, lo, hi = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            lib.gpmdm_pf_exchange_width(h, ctypes.byref(w), ctypes.byref(lo), ctypes.byref(hi))
            dev = self.device
            n_loc, P = hi.value - lo.value, self._num_particles
            self._send = torch.empty((n_loc, w.value), dtype=torch.float64, device=dev)
            self._recv = torch.empty((P, w.value), dtype=torch.float64, device=dev)
            # the split exchange: {class, state} during the observation GP, then {ll}
            self._send_s = torch.empty((n_loc, w.value - 1), dtype=torch.float64, device=dev)
            self._recv_s = torch.empty((P, w.value - 1), dtype=torch.float64, device=dev)
            self._send_l = torch.empty((n_loc, 1), dtype=torch.float64, device=dev)
            self._recv_l = torch.empty((P, 1), dtype=torch.float64, device=dev)
        self._init_particles()

    def __del__(self):
        try:
            dr = getattr(self, "_draws", None)
            if dr is not None and hasattr(dr, "close"):
                dr.close()                      # draws ahead write into the handle's buffers: join them
            for h, _ in getattr(self, "_peers", []):
                _lib.load().gpmdm_pf_destroy(h)
            self._peers = []
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.load().gpmdm_pf_destroy(self._h)
                self._h = None
            for c in getattr(self, "_comms", []):   # after the filters using them
                _lib.load().gpmdm_comm_destroy(c)
            self._comms = []
        except Exception:
            pass

    # ---- helpers --------------------------------------------------------------
    def _stream(self):
        # the raw handle of the device's current stream (torch.cuda.current_stream builds a
        # Stream object per call: ~5 us, a visible share of a 0.12 ms notebook frame)
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(self._dev_index))

    def _sync_model(self):
        """The reference filter reads its GPMDM's current state on every call
        (gpmdm_pf.py:164, 183): after the model was rebuilt (set_latents, train_adam,
        a reload into the same object) rebind the device filter to the new image."""
        self._gpmdm._refresh()                  # parameters changed in place (an optimiser step)?
        if self._gpmdm.generation != self._model_gen:
            lib = _lib.load()
            if self._devices is None:
                _lib.check(lib.gpmdm_pf_set_model(self._h, self._gpmdm.handle), "rebind to the rebuilt model")
            else:
                for h, dev in [(self._h, self._devices[0])] + self._peers:
                    _lib.check(lib.gpmdm_pf_set_model(h, self._gpmdm.handle_on(dev)), "rebind to the rebuilt model")
            self._model_gen = self._gpmdm.generation

    def _all(self):
        """(handle, raw stream) of every rank this process drives (devices=: all of them)."""
        out = [(self._h, self._stream())]
        for h, dev in self._peers:
            out.append((h, ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(dev))))
        return out

    def _each(self, fn_name, *args, what=""):
        """The same library call (handle, *args, stream) on every rank this process drives."""
        lib = _lib.load()
        for h, s in self._all():
            _lib.check(getattr(lib, fn_name)(h, *args, s), what or fn_name)

    def _divide_into_n_parts(self, x: int, n: int) -> list:
        """gpmdm_pf.py:287-292."""
        g, r = divmod(x, n)
        return [g + (1 if i < r else 0) for i in range(n)]

    # ---- reference API ----------------------------------------------------------
    def _init_particles(self):
        """gpmdm_pf.py:87-115: P_c particles per class drawn from that class's latents."""
        counts = self._divide_into_n_parts(self._num_particles, self.num_classes)
        sizes = [self._gpmdm.get_X_for_class(c).shape[0] for c in range(self.num_classes)]
        idx = replay.init_draws(sizes, counts)
        states = np.concatenate([self._gpmdm.get_X_for_class(c).detach().cpu().numpy()[idx[c]] for c in range(self.num_classes)], 0)
        classes = np.concatenate([np.full(counts[c], c, dtype=np.int64) for c in range(self.num_classes)])
        states = np.ascontiguousarray(states, dtype=np.float64)
        if self._collective:                    # one replicated filter: rank 0's particles
            from .distributed import broadcast_array
            states = np.ascontiguousarray(broadcast_array(states, self._group, self.device))
            classes = np.ascontiguousarray(broadcast_array(classes, self._group, self.device))
        self._sync_model()
        for h in [self._h] + [p[0] for p in self._peers]:
            _lib.check(_lib.load().gpmdm_pf_init(h, _lib.dptr(states), _lib.i64ptr(classes)), "init")
        self._readout = None

    def reset(self):
        self._init_particles()

    def _check_mask(self, observed):
        """``observed`` as D uint8 flags (None: every dimension observed); shape errors are
        raised here, before the library is touched."""
        if observed is None:
            return None
        m = np.asarray(observed, dtype=bool).reshape(-1)
        if m.shape[0] != self.observation_dim:
            raise ValueError(f"observed must have {self.observation_dim} flags, got {m.shape[0]}")
        return np.ascontiguousarray(m, dtype=np.uint8)

    def _set_mask(self, mask):
        """Put the mask (``_check_mask``'s result) in force on every handle this process
        drives, if it differs from the one in force (gpmdm_pf_set_obs_mask)."""
        key = None if mask is None else mask.tobytes()
        if key == getattr(self, "_mask_key", None):
            return
        lib = _lib.load()
        ptr = None if mask is None else ctypes.c_void_p(mask.ctypes.data)
        for h in [self._h] + [p[0] for p in self._peers]:
            _lib.check(lib.gpmdm_pf_set_obs_mask(h, ptr), "observed")
        self._mask_key = key

    def update(self, z, observed=None):
        """gpmdm_pf.py:117-135: switch classes, propagate dynamics, weight, resample.

        ``observed`` (anything ``np.asarray(..., bool)`` turns into D flags; default: all):
        the dimensions of ``z`` that were seen this frame.  The particles are weighted by the
        reference's likelihood on the model restricted to those dimensions; ``z`` at the
        others is ignored (it may be NaN).  For a capture stream that marks a dropped marker
        with NaN the idiom is ``pf.update(z, observed=np.isfinite(z))``.  With no dimension
        observed the frame is a pure prediction step (``w`` exactly 1/P).  ``update(z)``
        without the argument is the reference's update, NaN propagation included.
        ``current_observation()`` then reads the pose back, missing joints imputed."""
        z = _as_f64_vector(z)
        if z.shape[0] != self.observation_dim:
            raise ValueError(f"observation must have {self.observation_dim} values, got {z.shape[0]}")
        mask = self._check_mask(observed)
        self._sync_model()
        self._set_mask(mask)
        lib, h, s = _lib.load(), self._h, self._stream()
        P, C, d = self._num_particles, self.num_classes, self.latent_dim
        if self._rng == "torch":
            if self._draws is None:
                nu = P if self._resample_mode == "multinomial" else 1
                if P >= PARALLEL_REPLAY_P and replay.host_threads() > 1:
                    # torch's own samplers in parallel chunks, bit for bit the serial streams,
                    # drawn straight into the library's pinned staging buffers (no copy)
                    pe, pn, pu = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
                    _lib.check(lib.gpmdm_pf_draw_buffers(h, ctypes.byref(pe), ctypes.byref(pn), ctypes.byref(pu)),
                               "draw buffers")
                    bufs = (np.ctypeslib.as_array(ctypes.cast(pe, ctypes.POINTER(ctypes.c_double)), (P, C)),
                            np.ctypeslib.as_array(ctypes.cast(pn, ctypes.POINTER(ctypes.c_double)), (P, d)),
                            np.ctypeslib.as_array(ctypes.cast(pu, ctypes.POINTER(ctypes.c_double)), (nu,)))
                    hh = self._h
                    self._draws = replay.ParallelFrameDraws(
                        P, C, d, nu, buffers=bufs,
                        wait_free=lambda k: _lib.check(_lib.load().gpmdm_pf_draws_free(hh, k), "draw buffer"))
                else:
                    self._draws = replay.FrameDraws(P, C, d, nu)
                self._counts = np.zeros(C, dtype=np.int64)
                dr = self._draws           # the draws land in place: their pointers are fixed
                self._draw_ptr = (_lib.dptr(dr.E), _lib.i64ptr(self._counts), _lib.dptr(dr.N), _lib.dptr(dr.U))
            dr, counts = self._draws, self._counts
            pE, pC, pN, pU = self._draw_ptr
            dr.switch()
            if self._pre_sw and not dr.last_hit:
                # the caller drew from the generator since the pre-switch: its E is stale
                _lib.check(lib.gpmdm_pf_preswitch(h, pE, s), "preswitch")
            self._pre_sw = False
            _lib.check(lib.gpmdm_pf_switch(h, pE, pC, s), "switch")
            for hp, sp in self._all()[1:]:      # devices=: every rank switches all P (replay)
                _lib.check(lib.gpmdm_pf_switch(hp, pE, None, sp), "switch")
            dr.dynamics(counts)
            if self._n_staged:
                # the first class's normals drawn ahead went to the device behind the last
                # read-out; copy what dynamics() drew (everything if the ahead draw was stale)
                v = dr.ahead_valid if dr.last_hit else 0
                _lib.check(lib.gpmdm_pf_stage_normals(h, pN, v, P * d, s), "stage normals")
                self._n_staged = False
            self._propagate(z, dr.N, s, pN)
            dr.resample()
            self._each("gpmdm_pf_resample", pU, what="resample")
            if self._replay_preswitch() and dr.ahead_ready():
                # the next frame's E and first-class normals are drawn ahead (they need no
                # device result): its switch and dynamics tiles go behind this read-out
                # (gpmdm_pf_preswitch), and the normals to the device (gpmdm_pf_stage_normals)
                _lib.check(lib.gpmdm_pf_preswitch(h, pE, s), "preswitch")
                _lib.check(lib.gpmdm_pf_stage_normals(h, pN, 0, P * d, s), "stage normals")
                self._pre_sw = self._n_staged = True
        else:
            self._each("gpmdm_pf_switch", None, None, what="switch")
            self._propagate(z, None, s)
            self._each("gpmdm_pf_resample", None, what="resample")
        self._readout = None

    step = update    # north-star name (BASELINE.json): one filter step

    def _replay_preswitch(self) -> bool:
        """Replay filters whose draws are made ahead (ParallelFrameDraws), on one handle and
        one rank, launch the next switch between frames (GPMDM_NO_PRESWITCH=1: not, A/B)."""
        return (isinstance(self._draws, replay.ParallelFrameDraws) and not self._peers and self._world == 1
                and not os.environ.get("GPMDM_NO_PRESWITCH"))

    def update_with_draws(self, z, exp_draws, normals, uniforms, observed=None):
        """One update with explicit random draws in the reference's order (replay: see
        gpmdm_amd.replay): exp_draws P x C, normals (sum_c P_c) x d grouped by class,
        uniforms P (multinomial) or 1 (systematic).  Requires rng='torch'.  ``observed``:
        as in ``update``."""
        if self._rng != "torch":
            raise ValueError("explicit draws need rng='torch' (replay mode)")
        z = _as_f64_vector(z)
        if z.shape[0] != self.observation_dim:
            raise ValueError(f"observation must have {self.observation_dim} values, got {z.shape[0]}")
        mask = self._check_mask(observed)
        self._sync_model()
        self._set_mask(mask)
        lib, h, s = _lib.load(), self._h, self._stream()
        P, C, d = self._num_particles, self.num_classes, self.latent_dim
        E = np.ascontiguousarray(exp_draws, dtype=np.float64).reshape(P, C)
        self._each("gpmdm_pf_switch", _lib.dptr(E), None, what="switch")
        nrm = np.ascontiguousarray(normals, dtype=np.float64).reshape(P, d)
        self._propagate(z, nrm, s)
        U = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
        self._each("gpmdm_pf_resample", _lib.dptr(U), what="resample")
        self._readout = None

    def set_comm(self, comm, pad_rows: bool = False):
        """Let the library run the per-frame exchange over an RCCL communicator
        (``gpmdm_pf_set_comm``; ``comm``: an ``RcclComm`` or a raw ncclComm_t address of
        this filter's (world, rank), on the model's device; ``None`` detaches).
        ``pad_rows`` forces the uneven-shard gather path (tests).  The communicator must
        outlive the filter's use of it."""
        if self._devices is not None:
            raise ValueError("a devices= filter holds its own communicators")
        ptr = getattr(comm, "ptr", comm)
        _lib.check(_lib.load().gpmdm_pf_set_comm(self._h, ctypes.c_void_p(ptr) if ptr else None,
                                                 _lib.GPMDM_COMM_PAD_ROWS if pad_rows else 0), "set_comm")
        self._comm = comm

    def _propagate(self, z, normals, s, normals_ptr=None):
        """gpmdm_pf.py:153-192 for this rank's particles, and on several ranks the exchange:
        the new {class, state} rows are all-gathered while the observation GP runs (they are
        final once the dynamics GP is done), the likelihoods after it -- by the library over
        its communicator (set_comm), or here over the process group / exchange callback."""
        lib, h = _lib.load(), self._h
        nrm = normals_ptr if normals_ptr is not None else (None if normals is None else _lib.dptr(normals))
        if self._devices is not None:
            # one thread drives every rank: the library stages them and groups the collectives
            hs = self._all()
            n = len(hs)
            _lib.check(lib.gpmdm_pf_propagate_multi((ctypes.c_void_p * n)(*[x[0] for x in hs]), n, _lib.dptr(z), nrm,
                                                    (ctypes.c_void_p * n)(*[x[1] for x in hs])), "propagate")
            return
        if self._world == 1 or self._comm is not None:
            _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), nrm, s), "propagate")
            return
        _lib.check(lib.gpmdm_pf_propagate_dynamics(h, nrm, s), "propagate_dynamics")
        _lib.check(lib.gpmdm_pf_pack_part(h, self._send_s.data_ptr(), _lib.GPMDM_PACK_STATES, s), "pack")
        states_done = self._gather(self._recv_s, self._send_s)
        _lib.check(lib.gpmdm_pf_weigh(h, _lib.dptr(z), s), "weigh")
        _lib.check(lib.gpmdm_pf_pack_part(h, self._send_l.data_ptr(), _lib.GPMDM_PACK_LL, s), "pack")
        self._gather(self._recv_l, self._send_l)()
        states_done()
        _lib.check(lib.gpmdm_pf_unpack_part(h, self._recv_s.data_ptr(), _lib.GPMDM_PACK_STATES, s), "unpack")
        _lib.check(lib.gpmdm_pf_unpack_part(h, self._recv_l.data_ptr(), _lib.GPMDM_PACK_LL, s), "unpack")

    def _gather(self, recv, send):
        """Start the all-gather of recv <- send; returns the function that completes it."""
        if self._exchange_fn is not None:
            self._exchange_fn(recv, send)
            return lambda: None
        from .distributed import allgather_rows_start
        return allgather_rows_start(recv, send, self._group)

    # staged update for callers that drive the exchange themselves (tests, schedulers)
    def _stage_propagate(self, z):
        z = np.ascontiguousarray(torch.as_tensor(z, dtype=torch.float64).cpu().numpy().reshape(-1))
        self._sync_model()
        lib, h, s = _lib.load(), self._h, self._stream()
        _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
        _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(z), None, s), "propagate")
        _lib.check(lib.gpmdm_pf_pack(h, self._send.data_ptr(), s), "pack")
        return self._send

    def _stage_resample(self):
        lib, h, s = _lib.load(), self._h, self._stream()
        _lib.check(lib.gpmdm_pf_unpack(h, self._recv.data_ptr(), s), "unpack")
        _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")
        self._readout = None

    def _read(self):
        if self._readout is None:
            post, mean, lik = self._ro           # reused buffers: callers get copies
            _lib.check(_lib.load().gpmdm_pf_read(self._h, *self._ro_ptr, self._stream()), "read")
            self._readout = (post, mean, float(lik[0]))
        return self._readout

    def log_likelihood(self) -> float:
        """gpmdm_pf.py:215-222 (as in the reference: sum exp(ll + log_w - max), not a log)."""
        return self._read()[2]

    def class_probabilities(self) -> torch.Tensor:
        """gpmdm_pf.py:224-248."""
        return torch.from_numpy(self._read()[0].copy())

    def get_most_likely_class(self) -> int:
        """gpmdm_pf.py:250-254 (argmax, first maximum as torch.argmax; numpy on the cached
        read-out: no tensor round trip in the per-frame loop)."""
        return int(np.argmax(self._read()[0]))

    def current_state_mean(self) -> torch.Tensor:
        """gpmdm_pf.py:256-262."""
        return torch.from_numpy(self._read()[1].copy())

    def predict(self) -> torch.Tensor:
        """Dynamics-only one-step prediction of the latent mean: the average over the
        current particles of each particle's class dynamics-GP mean (gpmdm.py:1032-1068),
        computed on the device (gpmdm_pf_predict: class grouping, the dynamics GP tiles,
        a fixed-order mean).  Does not change the filter state and draws no random numbers."""
        self._sync_model()
        out = np.zeros(self.latent_dim)
        _lib.check(_lib.load().gpmdm_pf_predict(self._h, _lib.dptr(out), self._stream()), "predict")
        return torch.from_numpy(out)

    def set_predictive(self, on: bool = True):
        """Keep, from the next update on, each particle's GP predictive-variance factor
        vc = 1 - k^T K_y^-1 k as the likelihood forms it (one 8-byte store per particle), for
        ``innovation`` and ``current_observation(gp_variance=True)`` (gpmdm_pf_set_predictive; the
        constructor's ``predictive``).  Off, an update issues exactly the work it issued without
        the feature.  Either way the filter's results are bitwise the same.  Between updates only;
        ValueError for ``set_predictive(False)`` while the gate is on."""
        if not on and getattr(self, "_gate", None) is not None:
            raise ValueError("set_predictive(False) while the gate is on: call set_gate(None) first")
        self._sync_model()
        lib = _lib.load()
        for h in [self._h] + [p[0] for p in self._peers]:
            _lib.check(lib.gpmdm_pf_set_predictive(h, 1 if on else 0), "set_predictive")
        self._predictive = bool(on)

    @property
    def predictive(self) -> bool:
        return self._predictive

    def innovation(self, particles: bool = False) -> Innovation:
        """Per-joint innovations of the frame the last ``update`` weighed (gpmdm_pf_innovation):
        ``pf.update(z); inn = pf.innovation(); suspicious = inn.zscore.abs() > k``.  Evaluated on the
        device from what the frame left there -- the propagated cloud, each particle's vc and the
        staged ``z`` -- by the pose read-out's tile with a log-sum-exp epilogue; no state change,
        no draw, the same frame gives bitwise the same result.  ``particles``: also the propagated
        states and their vc (``states``, ``variance_common``).  Needs ``predictive``; ValueError
        when it is off or the filter is sharded, RuntimeError before the first update after
        ``reset`` / ``load_state`` / ``set_predictive``."""
        if not self._predictive:
            raise ValueError("innovation: build the filter with predictive=True or call set_predictive(True)")
        return _innovation_call(self, "gpmdm_pf_innovation", (), particles)

    def set_gate(self, gate=None, limit: float = 0.5):
        """Reject outlier joints inside ``update``, from the next update on (gpmdm_pf_set_gate; the
        constructor's ``gate`` / ``gate_limit``): ``pf = GPMDM_PF(m, T, P, gate=6.0); pf.update(z);
        pf.gate_report().gated``.  With the frame's own innovation z-scores (``innovation``'s, on
        the propagated cloud), joints that are observed and have |zscore| > ``gate`` are dropped
        from the frame's likelihood before the particles are normalised and resampled, provided at
        most floor(``limit`` x observed joints) exceed; if more do, nothing is dropped (a surprise
        shared by most of the body is a lost track, not a marker fault).  Everything runs on the
        device behind the likelihood finish, without a host wait: the innovation tile
        (k_obs_innov), the decision (k_gate_decide) and, effective only where something is
        rejected, a mean-only re-weigh (k_obs_reweigh, k_gate_finish) with each particle's stored
        vc -- no second N x N pass.  No draw from any generator; a frame that rejects nothing is
        bitwise the frame of the same filter with ``predictive=True`` and no gate; the same frame
        gives the same bits.  ``innovation()`` keeps reporting against the caller's mask, and
        ``current_observation()`` imputes rejected joints as it imputes unobserved ones.
        ``gate=None`` turns it off: an update then issues exactly the work it issued without the
        feature.  Needs ``predictive`` (ValueError otherwise); single filters on one rank; between
        updates only.  Invalidates the last report."""
        k, lim = _check_gate(gate, limit)
        if k is not None and self._world > 1:
            raise ValueError("gate serves single filters on one rank, not sharded filters")
        if k is not None and not self._predictive:
            raise ValueError("gate: build the filter with predictive=True or call set_predictive(True)")
        self._sync_model()
        _lib.check(_lib.load().gpmdm_pf_set_gate(self._h, 0.0 if k is None else k, lim), "set_gate")
        self._gate, self._gate_limit = k, lim

    @property
    def gate(self):
        """The gate's z-score threshold, or None when it is off."""
        return self._gate

    @property
    def gate_limit(self) -> float:
        return self._gate_limit

    def gate_report(self) -> GateReport:
        """What the gate decided for the frame the last ``update`` weighed (gpmdm_pf_gate_report:
        one copy of k_gate_decide's device table and one wait): ``gated`` are the joints the frame
        rejected, ``used`` the ones its weights rest on, ``zscore`` bitwise ``innovation().zscore``.
        No state change, no draw.  ValueError with the gate off, RuntimeError before the first
        update after ``reset`` / ``load_state`` / ``set_predictive`` / ``set_gate``."""
        if getattr(self, "_gate", None) is None:
            raise ValueError("gate_report: build the filter with gate=k or call set_gate(k)")
        D = self.observation_dim
        zs = np.full(D, np.nan)
        ex, ga, us = (np.zeros(D, dtype=np.uint8) for _ in range(3))
        ng, nv, ov = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), ctypes.c_int32(0)
        self._sync_model()
        out = _lib.GateOut(_lib.dptr(zs), *[ctypes.c_void_p(a.ctypes.data) for a in (ex, ga, us)],
                           _lib.i64ptr(ng), _lib.i64ptr(nv), ctypes.pointer(ov))
        _lib.check(_lib.load().gpmdm_pf_gate_report(self._h, ctypes.byref(out), self._stream()), "gate_report")
        b = lambda a: torch.from_numpy(a.astype(bool))   # noqa: E731
        return GateReport(self._gate, torch.from_numpy(zs), b(ex), b(ga), b(us), int(ng[0]), int(nv[0]),
                          bool(ov.value))

    def current_observation(self, spread: bool = True, gp_variance: bool = False):
        """The filtered pose: the observation GP's mean (gpmdm.py:955-957) averaged over the
        particles the filter holds now, ``mean[j] = (1/P) sum_p mu_j(x_p)`` -- the denoised
        joint angles, and after masked updates the imputed values of the joints that were not
        seen -- and with ``spread`` the cloud's variance of each, ``(1/P) sum_p (mu_j(x_p) -
        mean[j])^2`` (the particles' disagreement, not the GP's own noise variance).  With
        ``gp_variance`` (a ``predictive`` filter, after an update) a last tensor is appended: the
        GP's own predictive variance ``il2_j mean_s vc[ancestor(s)]`` of the resampled cloud
        (gpmdm_pf_observation_gp; gathered from the values the frame's likelihood formed), so that
        ``spread + gp_variance`` is the calibrated posterior pose variance.  Computed
        on the device by a mean-only GP tile (gpmdm_pf_observation); does not change the
        filter state and draws no random numbers; the same cloud gives bitwise the same
        values.  A sharded filter evaluates its replicated cloud on rank 0."""
        self._sync_model()
        D = self.observation_dim
        mean = np.zeros(D)
        var = np.zeros(D) if spread else None
        _lib.check(_lib.load().gpmdm_pf_observation(self._h, _lib.dptr(mean), _lib.dptr(var), self._stream()),
                   "current_observation")
        res = (torch.from_numpy(mean), torch.from_numpy(var)) if spread else (torch.from_numpy(mean),)
        if gp_variance:
            if not self._predictive:
                raise ValueError("gp_variance: build the filter with predictive=True or call set_predictive(True)")
            gpv = np.zeros(D)
            _lib.check(_lib.load().gpmdm_pf_observation_gp(self._h, _lib.dptr(gpv), self._stream()),
                       "current_observation")
            res = res + (torch.from_numpy(gpv),)
        return res if len(res) > 1 else res[0]

    def current_observation_mean(self) -> torch.Tensor:
        """``current_observation``'s mean alone: the observation-space counterpart of
        ``current_state_mean``."""
        return self.current_observation(spread=False)

    def forecast(self, horizon: int, *, mode: str = "sample", observation: bool = True,
                 particles: bool = False, seed=None) -> Forecast:
        """Where the pose, the latent state and the activity will be 1..``horizon`` frames from
        now: the filter's own proposal (Markov switch, then the new class's dynamics GP with its
        noise; gpmdm_pf.py:137-168) rolled out ``horizon`` times on a scratch copy of the
        particles it holds now, without weighting or resampling, all on the device
        (gpmdm_pf_forecast).  Row h - 1 of each result is h frames ahead: the class fractions
        and mean state of the roll-out cloud, with ``observation`` the pose read-out of
        ``current_observation`` on it (mean and cloud spread), with ``particles`` the cloud
        itself.  ``mode="mean"`` is the deterministic variant (classes frozen, no noise; its
        first ``state_mean`` is ``predict()``'s).

        The draws are the device's Philox streams whatever the filter's ``rng``, keyed by
        ``seed`` (default: the filter's) and the current ``frame``: the same cloud, frame and
        seed give bitwise the same forecast, and a shorter horizon gives the first rows of a
        longer one.  The filter is not changed: no state change, no draw from torch's
        generator, and later updates are bitwise those without the call.  A sharded filter
        forecasts its replicated cloud on rank 0."""
        t = lambda a: None if a is None else torch.from_numpy(a)   # noqa: E731
        return Forecast(*map(t, _forecast_call(self, "gpmdm_pf_forecast", (), horizon, mode, observation,
                                               particles, seed)))

    def set_smoothing(self, lag: int):
        """Keep the last ``lag`` + 1 frames' resampling ancestors, classes and states on the
        device for ``smoothed`` (gpmdm_pf_set_smoothing; the constructor's ``smoothing_lag``).
        Each update then records its frame with one more short launch.  ``lag=0`` turns
        smoothing off and releases the history.  Every call, also one that repeats the lag in
        force, clears the history: the depth is 0 and the current cloud its root; so do
        ``reset``, ``load_state`` / ``import_state`` and a rebind to a rebuilt model
        (``export_state`` does not carry the history).  Between updates only."""
        L = _check_smoothing_lag(lag)
        self._sync_model()
        lib = _lib.load()
        for h in [self._h] + [p[0] for p in self._peers]:
            _lib.check(lib.gpmdm_pf_set_smoothing(h, L), "set_smoothing")
        self._smoothing_lag = L

    @property
    def smoothing_lag(self) -> int:
        return self._smoothing_lag

    def set_map_path(self, on: bool = True):
        """Record, with every frame of the history, the observation log-likelihood each recorded
        particle was resampled with, for ``map_path`` (gpmdm_pf_set_map; the constructor's
        ``map_path=True``): one more short launch per update and ``smoothing_lag`` + 1 rows of P
        doubles.  Needs smoothing on; single filters on one rank; between updates only.  Turning it
        on clears the history as ``set_smoothing`` does; a later ``set_smoothing`` keeps it."""
        on = bool(on)
        if on and not self._smoothing_lag:
            raise ValueError("smoothing is off: build the filter with smoothing_lag=L or call set_smoothing(L)")
        if self._peers or getattr(self, "_world", 1) > 1:
            raise ValueError("map_path serves filters on one rank, not sharded filters")
        self._sync_model()
        _lib.check(_lib.load().gpmdm_pf_set_map(self._h, 1 if on else 0), "set_map_path")
        self._map_path = on

    @property
    def map_recording(self) -> bool:
        """Whether the history keeps what ``map_path`` needs (``map_path=True`` / ``set_map_path``)."""
        return bool(getattr(self, "_map_path", False))

    @property
    def smoothing_depth(self) -> int:
        """min(smoothing lag, frames recorded since the history was last cleared): the largest
        lag ``smoothed`` serves now."""
        if not self._smoothing_lag:
            return 0
        self._sync_model()                      # (a rebuilt model clears the history)
        lag, depth = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().gpmdm_pf_smoothing_depth(self._h, ctypes.byref(lag), ctypes.byref(depth)),
                   "smoothing_depth")
        return depth.value

    def smoothed(self, lag=None, *, observation: bool = False, particles: bool = False) -> Smoothed:
        """What was happening ``lag`` frames ago, given what has been seen since: fixed-lag
        smoothing from the particles' ancestry (the genealogy smoother, Kitagawa 1996;
        gpmdm_pf_smoothed).  Each current particle p is traced back through the recorded
        resampling indices, j_0 = p, j_{l+1} = a_{t-l}[j_l]; row l holds the class fractions
        and the mean state of the traced cloud {X_{t-l}[j_l(p)]} (equal weights), the number
        of distinct ancestors it rests on, with ``observation`` the pose read-out of
        ``current_observation`` on it, and with ``particles`` the ancestors, states and
        classes themselves.  ``lag``: None for every lag 0..``smoothing_depth``, an integer for
        one, ``(first, last)`` for an inclusive range.

        Lag 0 is the resampled cloud itself with equal weights -- not ``class_probabilities()``,
        which pairs pre-resample weights with post-resample classes as the reference does.
        The filter resamples every frame, so far lags hang on few ancestors (path degeneracy):
        ``distinct_ancestors`` says how much each row is worth.  The filter is not changed: no
        draw, no state change, and later updates are bitwise those without the call; the same
        history gives bitwise the same result.  A sharded filter reads rank 0's history (every
        rank records the replicated cloud).  Needs ``smoothing_lag`` / ``set_smoothing``."""
        lags, rest = _smoothed_call(self, "filter", "gpmdm_pf_smoothed", (), lag, observation, particles)
        t = lambda a: None if a is None else torch.from_numpy(a)   # noqa: E731
        return Smoothed(t(lags), t(self.frame - lags), *map(t, rest))

    def smoothed_marginal(self, lag=None, *, particles: bool = False) -> MarginalSmoothed:
        """What was happening ``lag`` frames ago, given what has been seen since, as a distribution
        over that frame's whole recorded cloud: the forward-filter backward marginal smoother
        (gpmdm_pf_smoothed_marginal).  With w_0 = 1/P on the current cloud, each lag's weights come
        from the previous lag's by one ``backward_step`` against the filter's own proposal (class
        switch, then the new class's dynamics GP); row l holds sum_i w_l,i [c_i = c], sum_i w_l,i X_i,
        the mass sum_i w_l,i (1 to rounding, never renormalised), ``ess`` = mass^2 / sum w^2,
        ``ess_distinct`` = mass^2 / sum m_i w_i^2 with m_i the copies of particle i's resampling
        ancestor in its frame, and with ``particles`` the weights themselves.  ``lag`` as in
        ``smoothed``.  ``ess`` counts copies as support; read ``ess_distinct`` beside
        ``smoothed().distinct_ancestors``.

        Prefer ``smoothed`` for whole trajectories, poses and near lags (its cost is O(P) per lag);
        prefer this one wherever ``distinct_ancestors`` has collapsed (its cost is O(P^2) per lag).
        No draw, no state change: later updates are bitwise those without the call, and the same
        history gives the same bits.  Single filters on one rank, up to 262144 particles."""
        first, last = _check_lag_range(lag)
        if self._peers or getattr(self, "_world", 1) > 1:
            raise ValueError("smoothed_marginal serves filters on one rank, not sharded filters")
        P = self._num_particles
        if P * P > _lib.GPMDM_BACKSMOOTH_MAX_PAIRS:
            raise ValueError(f"smoothed_marginal serves up to 262144 particles (2^36 pairs per step), got {P}")
        if not self._smoothing_lag:
            raise ValueError("smoothing is off: build the filter with smoothing_lag=L or call set_smoothing(L)")
        depth = self.smoothing_depth
        if last is None:
            last = depth
        if last > depth:
            raise ValueError(f"lag {last} is above the recorded depth {depth} (smoothing lag {self._smoothing_lag})")
        C, d, n = self.num_classes, self.latent_dim, last - first + 1
        cp, sm = np.zeros((n, C)), np.zeros((n, d))
        ms, es, ed = np.zeros(n), np.zeros(n), np.zeros(n)
        w = np.zeros((n, P)) if particles else None
        out = _lib.MarginalOut(*map(_lib.dptr, (cp, sm, ms, es, ed, w)))
        _lib.check(_lib.load().gpmdm_pf_smoothed_marginal(self._h, first, last, ctypes.byref(out), self._stream()),
                   "smoothed_marginal")
        lags = np.arange(first, last + 1, dtype=np.int64)
        t = lambda x: None if x is None else torch.from_numpy(x)   # noqa: E731
        return MarginalSmoothed(t(lags), t(self.frame - lags), *map(t, (cp, sm, ms, es, ed, w)))

    def map_path(self, lag=None, *, observation: bool = False, particles: bool = False) -> MapPath:
        """The most probable class-and-state sequence over the last ``lag`` frames' recorded clouds
        (None: the whole recorded depth), given what was seen in them: the MAP sequence estimate on
        the particle grid, a Viterbi recursion with the filter's own proposal as transition density
        (gpmdm_pf_map_path; Godsill, Doucet & West 2001).  With delta = 0 on the cloud ``lag`` frames
        ago, each nearer frame's delta_l(j) = ll_l[j] + max_k [delta_{l+1}(k) + log f(k -> j)]
        (``map_step``; ll_l[j] the log-likelihood particle j was resampled with), the path ends in
        the lowest-index argmax of delta_0 and follows the back-pointers.  Where per-frame argmaxes
        of ``smoothed`` / ``smoothed_marginal`` may switch class along transitions ``T`` forbids,
        this is one trajectory that the model supports.  ``observation``: ``model.map_x_to_y`` of the
        path's states; ``particles``: delta and the back-pointers of every recorded particle.

        Ties go to the lowest index, no draw is taken and nothing in the filter changes: later
        updates are bitwise those without the call, and the same history gives the same bits.  The
        recursion runs on each frame's distinct resampling ancestors (``distinct``), so far lags
        cost little.  Needs ``smoothing_lag`` and ``map_path=True`` / ``set_map_path``; single
        filters on one rank, up to 262144 particles."""
        if lag is not None and (isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or
                                not 1 <= int(lag) <= _lib.GPMDM_SMOOTH_MAX_LAG):
            raise ValueError(f"lag must be None or an integer in [1, {_lib.GPMDM_SMOOTH_MAX_LAG}], got {lag!r}")
        if self._peers or getattr(self, "_world", 1) > 1:
            raise ValueError("map_path serves filters on one rank, not sharded filters")
        P = self._num_particles
        if P * P > _lib.GPMDM_BACKSMOOTH_MAX_PAIRS:
            raise ValueError(f"map_path serves up to 262144 particles (2^36 pairs per step), got {P}")
        if not self._smoothing_lag:
            raise ValueError("smoothing is off: build the filter with smoothing_lag=L or call set_smoothing(L)")
        if not getattr(self, "_map_path", False):
            raise ValueError("map recording is off: build the filter with map_path=True or call set_map_path()")
        depth = self.smoothing_depth
        n_lag = depth if lag is None else int(lag)
        if n_lag > depth or n_lag < 1:
            raise ValueError(f"lag {n_lag} is outside [1, the recorded depth {depth}] (smoothing lag {self._smoothing_lag})")
        d, n = self.latent_dim, n_lag + 1
        ix, cl, ds = (np.zeros(n, dtype=np.int64) for _ in range(3))
        st, sc, lj = np.zeros((n, d)), np.zeros(n), np.zeros(1)
        de = np.zeros((n, P)) if particles else None
        bp = np.zeros((n_lag, P), dtype=np.int64) if particles else None
        out = _lib.MapOut(_lib.i64ptr(ix), _lib.i64ptr(cl), _lib.dptr(st), _lib.dptr(sc), _lib.dptr(lj),
                          _lib.i64ptr(ds), _lib.dptr(de), _lib.i64ptr(bp))
        _lib.check(_lib.load().gpmdm_pf_map_path(self._h, n_lag, ctypes.byref(out), self._stream()), "map_path")
        lags = np.arange(n, dtype=np.int64)
        t = lambda x: None if x is None else torch.from_numpy(x)   # noqa: E731
        om = None
        if observation:
            ok = np.isfinite(st).all(axis=1)
            om = torch.full((n, self.observation_dim), float("nan"), dtype=torch.float64)
            if ok.any():
                y = self._gpmdm.map_x_to_y(torch.from_numpy(st[ok]))
                y = y[0] if isinstance(y, (tuple, list)) else y
                om[torch.from_numpy(ok)] = y.detach().cpu().to(torch.float64)
        return MapPath(t(lags), t(self.frame - lags), t(ix), t(cl), t(st), t(sc), float(lj[0]), t(ds), t(de), t(bp), om)

    def sample_trajectories(self, n, lag=None, *, seed=None, observation: bool = False) -> SampledTrajectories:
        """``n`` draws from the joint smoothing distribution over the last ``lag`` frames' recorded
        clouds (None: the whole recorded depth): backward simulation (FFBSi;
        gpmdm_pf_sample_trajectories).  Trajectory m starts at a uniformly drawn particle of the
        current cloud and steps back frame by frame, each time drawing a particle of the older
        cloud with probability proportional to its transition density towards the one it holds
        (``backward_sample_step`` against the filter's own proposal).  Where ``smoothed`` hangs on a
        few ancestors, ``smoothed_marginal`` loses what ties one frame to the next and ``map_path``
        is one sequence with no spread, these are whole class-and-state sequences that the model
        supports -- the thing to compute the distribution of any statistic of a sequence from.
        Cost: O(n P) per lag.  ``observation``: the pose read-out of ``current_observation`` on each
        lag's sampled states.

        The uniforms are Philox draws keyed by ``seed`` (None: the filter's own) on a stream of
        their own, counted by (trajectory, frame, lag): trajectory m does not depend on ``n``, a
        shorter window is a prefix of a longer one, and the same call gives the same bits.  No
        draw is taken from the filter's streams or torch's generator and nothing in the filter
        changes: later updates are bitwise those without the call.  Needs ``smoothing_lag`` /
        ``set_smoothing``; single filters on one rank, ``n * P`` up to 2^36."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) < 2 ** 31:
            raise ValueError(f"n must be an integer in [1, 2^31), got {n!r}")
        if lag is not None and (isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or
                                not 1 <= int(lag) <= _lib.GPMDM_SMOOTH_MAX_LAG):
            raise ValueError(f"lag must be None or an integer in [1, {_lib.GPMDM_SMOOTH_MAX_LAG}], got {lag!r}")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or
                                 not 0 <= int(seed) < 2 ** 64):
            raise ValueError(f"seed must be None or an integer in [0, 2^64), got {seed!r}")
        if self._peers or getattr(self, "_world", 1) > 1:
            raise ValueError("sample_trajectories serves filters on one rank, not sharded filters")
        n, P = int(n), self._num_particles
        if n * P > _lib.GPMDM_BACKSMOOTH_MAX_PAIRS:
            raise ValueError(f"sample_trajectories serves up to 2^36 trajectory-particle pairs per step, got {n} x {P}")
        if not self._smoothing_lag:
            raise ValueError("smoothing is off: build the filter with smoothing_lag=L or call set_smoothing(L)")
        depth = self.smoothing_depth
        n_lag = depth if lag is None else int(lag)
        if n_lag > depth or n_lag < 1:
            raise ValueError(f"lag {n_lag} is outside [1, the recorded depth {depth}] (smoothing lag {self._smoothing_lag})")
        C, d, D, L1 = self.num_classes, self.latent_dim, self.observation_dim, n_lag + 1
        ix, cl = np.zeros((L1, n), dtype=np.int64), np.zeros((L1, n), dtype=np.int64)
        st, cp, sm = np.zeros((L1, n, d)), np.zeros((L1, C)), np.zeros((L1, d))
        al, ds = np.zeros(L1, dtype=np.int64), np.zeros(L1, dtype=np.int64)
        om, os_ = (np.zeros((L1, D)), np.zeros((L1, D))) if observation else (None, None)
        out = _lib.SampleOut(_lib.i64ptr(ix), _lib.i64ptr(cl), _lib.dptr(st), _lib.dptr(cp), _lib.dptr(sm),
                             _lib.i64ptr(al), _lib.i64ptr(ds), _lib.dptr(om), _lib.dptr(os_))
        key = None if seed is None else ctypes.byref(ctypes.c_uint64(int(seed)))
        _lib.check(_lib.load().gpmdm_pf_sample_trajectories(self._h, n, n_lag, key, ctypes.byref(out), self._stream()),
                   "sample_trajectories")
        lags = np.arange(L1, dtype=np.int64)
        t = lambda x: None if x is None else torch.from_numpy(x)   # noqa: E731
        return SampledTrajectories(t(lags), t(self.frame - lags), *map(t, (ix, cl, st, cp, sm, al, ds, om, os_)))

    @property
    def frame(self) -> int:
        """Resamples done so far: the Philox counter of the next step's draws."""
        f = np.zeros(1, dtype=np.int64)
        _lib.check(_lib.load().gpmdm_pf_frame(self._h, _lib.i64ptr(f)), "frame")
        return int(f[0])

    def health(self, reset: bool = False) -> dict:
        """Failure counters since creation (or the last reset), per particle and step
        (SURVEY.md §5): non-positive observation / dynamics variances and non-finite
        log-likelihoods / states.  The arithmetic is the reference's (NaN propagates);
        these counts say when it happened."""
        n = np.zeros(len(_lib.HEALTH), dtype=np.int64)
        for h, s in self._all():                # devices=: each rank counts its own slice's events
            m = np.zeros(len(_lib.HEALTH), dtype=np.int64)
            _lib.check(_lib.load().gpmdm_pf_health(h, _lib.i64ptr(m), 1 if reset else 0, s), "health")
            n += m
        return {k: int(v) for k, v in zip(_lib.HEALTH, n)}

    # ---- introspection (tests, checkpoint of the filter state) --------------------
    def export_state(self) -> dict:
        P, d = self._num_particles, self.latent_dim
        out = dict(states=np.zeros((P, d)), classes=np.zeros(P, dtype=np.int64), ll=np.zeros(P),
                   log_w=np.zeros(P), w=np.zeros(P), resample_idx=np.zeros(P, dtype=np.int64))
        _lib.check(_lib.load().gpmdm_pf_export(
            self._h, _lib.dptr(out["states"]), _lib.i64ptr(out["classes"]), _lib.dptr(out["ll"]),
            _lib.dptr(out["log_w"]), _lib.dptr(out["w"]), _lib.i64ptr(out["resample_idx"]), self._stream()),
            "export")
        out["frame"] = self.frame
        out["seed"] = self._seed
        return out

    def load_state(self, states, classes, *, ll=None, log_w=None, w=None, resample_idx=None, frame=None):
        """Set the particle state.  With ``states``/``classes`` only: those particles with the
        reference's initial weights (ll = log_w = 0, w = 1/P; gpmdm_pf.py:100-104), e.g. a
        reference pre-step state.  With ``ll``, ``log_w`` and ``w`` as well (all three): the
        full filter state of ``export_state`` (gpmdm_pf.py:78-82) -- the read-outs right
        after are the exporter's, and the next updates continue its trajectory bit for bit
        (``resample_idx``: the ancestors of the last resample, optional; ``frame``: the
        Philox counter, optional; a replay filter's torch RNG state is the caller's to
        restore).  ``gpmdm_pf_import``."""
        self._sync_model()
        P = self._num_particles
        states = np.ascontiguousarray(states, dtype=np.float64).reshape(P, self.latent_dim)
        classes = np.ascontiguousarray(classes, dtype=np.int64).reshape(P)
        full = (ll, log_w, w)
        if all(x is None for x in full) and resample_idx is None and frame is None:
            for h in [self._h] + [p[0] for p in self._peers]:
                _lib.check(_lib.load().gpmdm_pf_init(h, _lib.dptr(states), _lib.i64ptr(classes)), "load_state")
        else:
            if any(x is None for x in full):
                raise ValueError("a full state import needs ll, log_w and w together")
            ll, log_w, w = (np.ascontiguousarray(x, dtype=np.float64).reshape(P) for x in full)
            ridx = None if resample_idx is None else np.ascontiguousarray(resample_idx, dtype=np.int64).reshape(P)
            for h in [self._h] + [p[0] for p in self._peers]:
                _lib.check(_lib.load().gpmdm_pf_import(
                    h, _lib.dptr(states), _lib.i64ptr(classes), _lib.dptr(ll), _lib.dptr(log_w), _lib.dptr(w),
                    _lib.i64ptr(ridx), -1 if frame is None else int(frame)), "load_state")
        self._readout = None

    def import_state(self, st: dict):
        """Restore an ``export_state()`` dict (a checkpoint of this filter or of one with
        the same configuration): ``load_state`` with every field it holds.  A Philox filter
        must have been built with the exporter's seed (checked)."""
        if self._rng == "philox" and "seed" in st and int(st["seed"]) != self._seed:
            raise ValueError("the state was exported by a filter with another Philox seed")
        self.load_state(st["states"], st["classes"], ll=st["ll"], log_w=st["log_w"], w=st["w"],
                        resample_idx=st.get("resample_idx"), frame=st.get("frame"))

    _CUT_SPLIT = {"auto": 0, "none": 1, "all": 2, "tail": 3, "chunks": 4}

    def set_obs_cutoff(self, on=True, stats: bool = False, split: str | None = None):
        """Run the observation GP with the model's kernel-value cutoff (GPMDM.enable_obs_cutoff,
        built here if needed) or the dense kernel; ``on="auto"``: per frame, the cutoff while
        the reach it measured on its last frame is below its break-even against the dense
        kernel, else the dense kernel (re-measured at least every 8 frames; one-rank filters,
        gpmdm_pf_set_obs_cutoff mode 3); ``stats`` also counts the MFMA groups run
        (obs_cutoff_stats; not with "auto"); ``split`` ("auto" default, "none", "all", "tail", "chunks")
        schedules the particle tiles run as two workgroups each (gpmdm_pf_set_obs_cutoff_split;
        the same results under every policy).  Between frames only."""
        if split is not None and split not in self._CUT_SPLIT:
            raise ValueError(f"split: one of {sorted(self._CUT_SPLIT)}")
        if isinstance(on, str) and on != "auto":
            raise ValueError("on: True, False or 'auto'")
        if on == "auto" and stats:
            raise ValueError("stats count the cutoff's work of every frame: not with on='auto'")
        if on:
            self._gpmdm.enable_obs_cutoff(True)
            self._sync_model()
        mode = 3 if on == "auto" else ((2 if stats else 1) if on else 0)
        lib = _lib.load()
        for h in [self._h] + [p[0] for p in self._peers]:
            _lib.check(lib.gpmdm_pf_set_obs_cutoff(h, mode), "set_obs_cutoff")
            if split is not None:
                _lib.check(lib.gpmdm_pf_set_obs_cutoff_split(h, self._CUT_SPLIT[split]), "set_obs_cutoff")
        self._obs_cutoff = mode

    def set_obs_skip(self, on: bool = True):
        """The dense observation tile branches around the MFMAs of all-zero 16 x 4 blocks of
        kernel values (default) or runs every block (gpmdm_pf_set_obs_skip).  The results are
        bitwise the same either way; off exists to show that.  Between frames only."""
        lib = _lib.load()
        for h in [self._h] + [p[0] for p in self._peers]:
            _lib.check(lib.gpmdm_pf_set_obs_skip(h, 1 if on else 0), "set_obs_skip")
        self._obs_skip = bool(on)

    def obs_cutoff_auto(self) -> dict:
        """AUTO cutoff state: whether the last frame ran the cutoff kernel, and the fraction of
        the dense MFMA work it ran on its last cutoff frame (None: not measured yet)."""
        last, frac = ctypes.c_int(), ctypes.c_double()
        _lib.check(_lib.load().gpmdm_pf_obs_cutoff_auto(self._h, ctypes.byref(last), ctypes.byref(frac)),
                   "obs_cutoff_auto")
        return {"last_frame_cutoff": bool(last.value), "fraction_run": frac.value if frac.value >= 0 else None}

    def obs_cutoff_stats(self, reset: bool = True) -> dict:
        """MFMA groups (16-particle x 16-column tile x 16-row K-step) the cutoff kernel ran since
        the last reset, against the dense kernel's count for the same launches."""
        lib = _lib.load()
        run, dense = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(lib.gpmdm_pf_obs_cutoff_stats(self._h, ctypes.byref(run), ctypes.byref(dense), 1 if reset else 0,
                                                 self._stream()), "obs_cutoff_stats")
        return {"run": run.value, "dense": dense.value,
                "fraction_run": run.value / dense.value if dense.value else None}

    def dynamics_rows(self) -> int:
        """Rows the last dynamics-GP pass evaluated (distinct ancestor/class keys when
        de-duplicating; this rank's particle count otherwise)."""
        r = np.zeros(1, dtype=np.int64)
        _lib.check(_lib.load().gpmdm_pf_dyn_rows(self._h, _lib.i64ptr(r), self._stream()), "dyn_rows")
        return int(r[0])

    def enable_timing(self, on: bool = True, stages=None):
        """Record per-stage HIP events (``stages``: names from ``_lib.STAGES``; default all).
        Each recorded stage adds two event records to the stream."""
        lib = _lib.load()
        names = _lib.STAGES if stages is None else tuple(stages)
        mask = 0
        for n in names:
            mask |= 1 << _lib.STAGES.index(n)
        _lib.check(lib.gpmdm_pf_timing_stages(self._h, mask))
        _lib.check(lib.gpmdm_pf_enable_timing(self._h, 1 if on else 0))

    def stage_times(self) -> dict:
        ms = np.zeros(len(_lib.STAGES))
        n = np.zeros(len(_lib.STAGES), dtype=np.int64)
        _lib.check(_lib.load().gpmdm_pf_stage_times(self._h, _lib.dptr(ms), _lib.i64ptr(n)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.STAGES)}

    # ---- properties (gpmdm_pf.py:267-285) ------------------------------------------
    @property
    def latent_dim(self):
        return self._gpmdm.d

    @property
    def observation_dim(self):
        return self._gpmdm.D

    @property
    def num_classes(self):
        return self._gpmdm.n_classes

    @property
    def dtype(self):
        return self._gpmdm.dtype

    @property
    def device(self):
        return self._gpmdm.device
