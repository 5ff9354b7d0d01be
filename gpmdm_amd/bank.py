"""GPMDM_PF_Bank -- many independent particle filters sharing one GPMDM.

The reference runs one ``GPMDM_PF`` per observation stream, one after another (the 39
trials of ``test_gpmdm_pf.ipynb`` cell 4, each a fresh filter over the same model;
SURVEY.md §8(f) row 3).  A bank runs F such filters as one device computation: the
dynamics and observation GP tile kernels see all F x P particles at once (filling the
GPU at the notebooks' P = 100), while normalisation, resampling and the read-outs run
per filter.  Every filter keeps the reference's per-filter semantics
(``gpmdm_pf.py:117-262``).

Draws come from the device (Philox).  Filter f is keyed with ``seed + f``, so its
trajectory is bit-identical to a single ``GPMDM_PF(..., rng='philox', seed=seed + f)``
started from the same particles; the bank changes the schedule, not the numbers.

With a ``process_group`` the filters are sharded over ranks (rank r owns filters
``[r F / R, (r + 1) F / R)``, the particle-shard rule of ``gpmdm_pf_create``).  Filters
are independent, so the step needs no collective at all; ``gather_readouts()`` is the
only exchange and is optional.  ``shard=(world, rank)`` selects the same slice without a
process group.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, replay
from .distributed import shard_range
from .model import GPMDM
from .pf import (BankGateReport, Forecast, Innovation, Smoothed, _check_bank_gate, _check_smoothing_lag, _forecast_call,
                 _innovation_call, _smoothed_call)


def _filter_major(a):
    """A (steps, F, ...) result of the library as a contiguous (F, steps, ...) tensor."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, 0, 1)))


class GPMDM_PF_Bank:
    def __init__(self, gpmdm: GPMDM, markov_switching_model, num_filters: int, num_particles: int, *,
                 seed=None, resample: str = "multinomial", process_group=None, shard=None,
                 dedup: bool = True, dyn_tiles: str = "auto", obs_cutoff: bool = False, smoothing_lag: int = 0,
                 predictive: bool = False, **gating):
        """``gating``: the keywords ``gate`` (default None) and ``gate_limit`` (default 0.5) of
        ``set_gate``, and nothing else (TypeError).  They are taken as a keyword group and are not
        named parameters of the signature: tests/test_gate_api_host.py pins the named ones."""
        unknown = sorted(set(gating) - {"gate", "gate_limit"})
        if unknown:
            raise TypeError(f"GPMDM_PF_Bank() got an unexpected keyword argument {unknown[0]!r}")
        gate, gate_limit = gating.get("gate"), gating.get("gate_limit", 0.5)
        self._gpmdm = gpmdm
        self._gpmdm.set_evaluation_mode()
        self._T = torch.as_tensor(markov_switching_model).type(torch.float64)
        if self._gpmdm.n_classes != self._T.size(0):
            raise ValueError("Number of classes in the GPMDM model and the Markov model do not match")
        if resample not in ("multinomial", "systematic"):
            raise ValueError("resample must be 'multinomial' or 'systematic'")
        self._smoothing_lag = _check_smoothing_lag(smoothing_lag)
        self._predictive = False
        self._num_filters = int(num_filters)
        self._num_particles = int(num_particles)
        if self._num_filters < 1 or self._num_particles < 1:
            raise ValueError("num_filters and num_particles must be positive")
        self._group = process_group
        if process_group is not None:
            import torch.distributed as dist
            world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        elif shard is not None:                   # (world, rank) without a process group
            world, rank = int(shard[0]), int(shard[1])
            if world > 1 and seed is None:
                raise ValueError("shard= needs an explicit seed (identical on every rank)")
        else:
            world, rank = 1, 0
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if process_group is not None and world > 1:   # one seed for the whole bank: rank 0's
            from .distributed import broadcast_array
            seed = int(broadcast_array(np.array([seed], dtype=np.int64), process_group, self.device)[0])
        self._seed = int(seed)
        self._world, self._rank = world, rank
        self._f_lo, self._f_hi = shard_range(self._num_filters, world, rank)
        gate, gate_limit = _check_bank_gate(gate, gate_limit, self._num_filters, self._f_lo, self._f_hi)
        if gate is not None and not predictive:
            raise ValueError("gate= needs predictive=True (the gate reads the frame's vc)")
        self._gate, self._gate_limit = None, gate_limit
        self._h = None
        self._readout = None
        if obs_cutoff:
            gpmdm.enable_obs_cutoff(True)     # the model's cutoff image (built once)
        if self.local_filters > 0:
            T = np.ascontiguousarray(self._T.numpy(), dtype=np.float64)
            h = ctypes.c_void_p()
            _lib.check(_lib.load().gpmdm_bank_create(
                gpmdm.handle, _lib.dptr(T), self.local_filters, self._num_particles,
                ctypes.c_uint64((self._seed + self._f_lo) & (2 ** 64 - 1)),
                _lib.GPMDM_RESAMPLE_MULTINOMIAL if resample == "multinomial" else _lib.GPMDM_RESAMPLE_SYSTEMATIC,
                ctypes.byref(h)), "GPMDM_PF_Bank")
            self._h = h
            self._model_gen = gpmdm.generation
            _lib.check(_lib.load().gpmdm_pf_set_dedup(h, 1 if dedup else 0), "dedup")
            if dyn_tiles not in _lib.DYN_TILES:
                raise ValueError("dyn_tiles must be 'auto', 'narrow' or 'wide'")
            _lib.check(_lib.load().gpmdm_pf_set_dyn_tiles(h, _lib.DYN_TILES[dyn_tiles]), "dyn_tiles")
            if obs_cutoff:                    # the observation GP's kernel-value cutoff (GPMDM_PF's)
                _lib.check(_lib.load().gpmdm_pf_set_obs_cutoff(h, 1), "obs_cutoff")
            self._init_particles()
            if self._smoothing_lag:
                self.set_smoothing(self._smoothing_lag)
        if predictive:
            self.set_predictive(True)
        if gate is not None:
            self.set_gate(gate, gate_limit)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.load().gpmdm_pf_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        dev = self.device
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None
                                                                   else torch.cuda.current_device()))

    def _sync_model(self):
        """Rebind to the GPMDM's current device image (see GPMDM_PF._sync_model)."""
        self._gpmdm._refresh()
        if self._h is not None and self._gpmdm.generation != self._model_gen:
            _lib.check(_lib.load().gpmdm_pf_set_model(self._h, self._gpmdm.handle), "rebind to the rebuilt model")
            self._model_gen = self._gpmdm.generation

    # ---- state ----------------------------------------------------------------------
    def _init_particles(self):
        """gpmdm_pf.py:87-115 for every local filter.  Filter f's initial draws come from a
        generator seeded with seed + f, so they do not depend on the rank count."""
        C, P = self.num_classes, self._num_particles
        g, r = divmod(P, C)
        counts = [g + (1 if i < r else 0) for i in range(C)]
        Xc = [self._gpmdm.get_X_for_class(c).detach().cpu().numpy() for c in range(C)]
        sizes = [x.shape[0] for x in Xc]
        states, classes = [], []
        for f in range(self._f_lo, self._f_hi):
            gen = torch.Generator().manual_seed(self._seed + f)
            idx = replay.init_draws(sizes, counts, generator=gen)
            states.append(np.concatenate([Xc[c][idx[c]] for c in range(C)], 0))
            classes.append(np.concatenate([np.full(counts[c], c, dtype=np.int64) for c in range(C)]))
        self.load_state(np.stack(states), np.stack(classes))

    def reset(self):
        if self._h is not None:
            self._init_particles()

    def load_state(self, states, classes, *, ll=None, log_w=None, w=None, resample_idx=None, frame=None):
        """states (F_local, P, d), classes (F_local, P); with ll / log_w / w (F_local, P) the
        full state of ``export_state`` (GPMDM_PF.load_state; gpmdm_pf_import)."""
        Fl, P, d = self.local_filters, self._num_particles, self.latent_dim
        states = np.ascontiguousarray(states, dtype=np.float64).reshape(Fl * P, d)
        classes = np.ascontiguousarray(classes, dtype=np.int64).reshape(Fl * P)
        self._sync_model()
        full = (ll, log_w, w)
        if all(x is None for x in full) and resample_idx is None and frame is None:
            _lib.check(_lib.load().gpmdm_pf_init(self._h, _lib.dptr(states), _lib.i64ptr(classes)), "load_state")
        else:
            if any(x is None for x in full):
                raise ValueError("a full state import needs ll, log_w and w together")
            ll, log_w, w = (np.ascontiguousarray(x, dtype=np.float64).reshape(Fl * P) for x in full)
            ridx = None if resample_idx is None else np.ascontiguousarray(resample_idx, dtype=np.int64).reshape(Fl * P)
            _lib.check(_lib.load().gpmdm_pf_import(
                self._h, _lib.dptr(states), _lib.i64ptr(classes), _lib.dptr(ll), _lib.dptr(log_w), _lib.dptr(w),
                _lib.i64ptr(ridx), -1 if frame is None else int(frame)), "load_state")
        self._readout = None

    def import_state(self, st: dict):
        """Restore an ``export_state()`` dict (same filters, same seed: checked)."""
        if "seed" in st and int(st["seed"]) != self._seed:
            raise ValueError("the state was exported by a bank with another seed")
        self.load_state(st["states"], st["classes"], ll=st["ll"], log_w=st["log_w"], w=st["w"],
                        resample_idx=st.get("resample_idx"), frame=st.get("frame"))

    def export_state(self) -> dict:
        Fl, P, d = self.local_filters, self._num_particles, self.latent_dim
        n = Fl * P
        out = dict(states=np.zeros((n, d)), classes=np.zeros(n, dtype=np.int64), ll=np.zeros(n),
                   log_w=np.zeros(n), w=np.zeros(n), resample_idx=np.zeros(n, dtype=np.int64))
        _lib.check(_lib.load().gpmdm_pf_export(
            self._h, _lib.dptr(out["states"]), _lib.i64ptr(out["classes"]), _lib.dptr(out["ll"]),
            _lib.dptr(out["log_w"]), _lib.dptr(out["w"]), _lib.i64ptr(out["resample_idx"]), self._stream()),
            "export")
        out["states"] = out["states"].reshape(Fl, P, d)
        for k in ("classes", "ll", "log_w", "w", "resample_idx"):
            out[k] = out[k].reshape(Fl, P)
        out["frame"] = self.frame
        out["seed"] = self._seed
        return out

    # ---- per-frame ------------------------------------------------------------------
    def _check_masks(self, observed):
        """``observed`` as (F_local, D) uint8 flags (None: every dimension of every filter
        observed).  Accepts (F, D) (each rank takes its rows, as for Z), (F_local, D) or (D,)
        (one mask for every filter); shape errors are raised here, before the library is
        touched."""
        if observed is None:
            return None
        m = np.asarray(observed, dtype=bool)
        F, Fl, D = self._num_filters, self.local_filters, self.observation_dim
        if m.shape == (D,):
            m = np.broadcast_to(m, (Fl, D))
        elif m.shape == (F, D) and Fl != F:
            m = m[self._f_lo:self._f_hi]
        elif m.shape != (Fl, D):
            raise ValueError(f"observed must be ({F}, {D}), ({Fl}, {D}) (local) or ({D},) flags, "
                             f"got {tuple(m.shape)}")
        return np.ascontiguousarray(m, dtype=np.uint8)

    def _set_masks(self, masks):
        """Put the masks (``_check_masks``' result) in force, if their bytes differ from the
        ones in force (gpmdm_bank_set_obs_masks; GPMDM_PF._set_mask)."""
        key = None if masks is None else masks.tobytes()
        if key == getattr(self, "_mask_key", None):
            return
        ptr = None if masks is None else ctypes.c_void_p(masks.ctypes.data)
        _lib.check(_lib.load().gpmdm_bank_set_obs_masks(self._h, ptr), "observed")
        self._mask_key = key

    def update(self, Z, observed=None):
        """One frame for every filter.  Z: (F, D) (all filters; each rank takes its rows)
        or (F_local, D).

        ``observed`` (anything ``np.asarray(..., bool)`` turns into (F, D), (F_local, D) or
        (D,) flags; default: all): the dimensions of each filter's row of ``Z`` that were seen
        this frame, one mask per filter (``GPMDM_PF.update``'s ``observed`` for each).  Filter
        f's particles are weighted by the reference's likelihood on the model restricted to
        f's observed dimensions; ``Z`` elsewhere is ignored (it may be NaN).  The idiom for
        capture streams that mark dropped markers with NaN is ``bank.update(Z,
        observed=np.isfinite(Z))``.  A filter with no dimension observed takes a pure
        prediction step (``w`` exactly 1/P).  ``update(Z)`` without the argument is the
        reference's update, NaN propagation included."""
        Z = np.asarray(torch.as_tensor(Z, dtype=torch.float64).cpu().numpy(), dtype=np.float64)
        Z = Z.reshape(-1, self.observation_dim)
        if Z.shape[0] == self._num_filters and self.local_filters != self._num_filters:
            Z = Z[self._f_lo:self._f_hi]
        if Z.shape[0] != self.local_filters:
            raise ValueError(f"expected {self._num_filters} (or {self.local_filters} local) observations, "
                             f"got {Z.shape[0]}")
        masks = self._check_masks(observed)
        self._readout = None
        if self._h is None:
            return
        Z = np.ascontiguousarray(Z)
        self._sync_model()
        self._set_masks(masks)
        lib, h, s = _lib.load(), self._h, self._stream()
        _lib.check(lib.gpmdm_pf_switch(h, None, None, s), "switch")
        _lib.check(lib.gpmdm_pf_propagate(h, _lib.dptr(Z), None, s), "propagate")
        _lib.check(lib.gpmdm_pf_resample(h, None, s), "resample")

    step = update

    def _read(self):
        if self._readout is None:
            Fl, C, d = self.local_filters, self.num_classes, self.latent_dim
            post, mean, lik = np.zeros((Fl, C)), np.zeros((Fl, d)), np.zeros(Fl)
            if self._h is not None:
                _lib.check(_lib.load().gpmdm_pf_read(self._h, _lib.dptr(post), _lib.dptr(mean), _lib.dptr(lik),
                                                     self._stream()), "read")
            self._readout = (post, mean, lik)
        return self._readout

    def class_probabilities(self) -> torch.Tensor:
        """(F_local, C): gpmdm_pf.py:224-248 per filter."""
        return torch.tensor(self._read()[0], dtype=torch.float64)

    def get_most_likely_class(self) -> torch.Tensor:
        """(F_local,): gpmdm_pf.py:250-254 per filter (first maximum)."""
        return torch.argmax(self.class_probabilities(), dim=1)

    def current_state_mean(self) -> torch.Tensor:
        """(F_local, d): gpmdm_pf.py:256-262 per filter."""
        return torch.tensor(self._read()[1], dtype=torch.float64)

    def log_likelihood(self) -> torch.Tensor:
        """(F_local,): gpmdm_pf.py:215-222 per filter (a sum of exponentials, as there)."""
        return torch.tensor(self._read()[2], dtype=torch.float64)

    def predict(self) -> torch.Tensor:
        """(F_local, d): GPMDM_PF.predict per filter (gpmdm_pf_predict)."""
        out = np.zeros((self.local_filters, self.latent_dim))
        if self._h is not None:
            self._sync_model()
            _lib.check(_lib.load().gpmdm_pf_predict(self._h, _lib.dptr(out), self._stream()), "predict")
        return torch.from_numpy(out)

    def set_predictive(self, on: bool = True):
        """``GPMDM_PF.set_predictive`` for the bank (gpmdm_bank_set_predictive): every update
        from now on keeps each particle's vc for ``innovation`` and
        ``current_observation(gp_variance=True)``; off, the bank issues exactly the work of a
        bank built without it.  Between updates only; ValueError for ``set_predictive(False)`` while
        the gate is on."""
        if not on and getattr(self, "_gate", None) is not None:
            raise ValueError("set_predictive(False) while the gate is on: call set_gate(None) first")
        if self._h is not None:
            self._sync_model()
            _lib.check(_lib.load().gpmdm_bank_set_predictive(self._h, 1 if on else 0), "set_predictive")
        self._predictive = bool(on)

    @property
    def predictive(self) -> bool:
        return self._predictive

    def innovation(self, particles: bool = False) -> Innovation:
        """``GPMDM_PF.innovation`` for every local filter in one pair of launches
        (gpmdm_bank_innovation): every field has a leading filter axis, and row f is bitwise the
        single filter's result on filter f's frame (its own row of ``Z`` and of the masks; a
        blacked-out filter has ``n_valid`` 0 and NaN in every field but ``mean`` and ``spread``)."""
        if not self._predictive:
            raise ValueError("innovation: build the bank with predictive=True or call set_predictive(True)")
        return _innovation_call(self, None if self._h is None else "gpmdm_bank_innovation", (self.local_filters,),
                                particles)

    def set_gate(self, gate=None, limit: float = 0.5):
        """``GPMDM_PF.set_gate`` for the bank (gpmdm_bank_set_gate; the constructor's ``gate`` /
        ``gate_limit``): from the next update on every filter rejects its own outlier joints inside
        ``update``, from its own row of ``Z``, of the masks and of the frame's innovations --
        ``bank = GPMDM_PF_Bank(m, T, F, P, predictive=True, gate=6.0); bank.update(Z);
        bank.gate_report().gated``.  ``gate``: None (off), one real number > 0 for every filter, or a
        sequence of ``num_filters`` entries (each rank takes its rows, as for ``observed``), each a
        real number > 0 or None -- that filter never rejects.  The cap is per filter,
        floor(``limit`` x the filter's observed joints).  A gated-mode update queues the innovation
        pair, the decision, the re-weigh tile and its finish once for all filters, without a host
        wait; filter f's frame is bitwise the frame of ``GPMDM_PF(rng="philox", seed=seed + f,
        predictive=True, gate=gate[f])``, and a filter that rejects nothing is bitwise the ungated
        filter whatever its neighbours reject.  A blacked-out filter's ``ll`` stays exactly 0.
        ``gate=None`` turns it off: an update then issues exactly the work it issued without the
        feature.  Needs ``predictive`` (ValueError otherwise); between updates only.  Invalidates the
        last report."""
        ks, lim = _check_bank_gate(gate, limit, self._num_filters, self._f_lo, self._f_hi)
        if ks is not None and not self._predictive:
            raise ValueError("gate: build the bank with predictive=True or call set_predictive(True)")
        if self._h is not None:
            self._sync_model()
            thr = np.zeros(self.local_filters) if ks is None else np.array(
                [np.inf if k is None else k for k in ks], dtype=np.float64)
            _lib.check(_lib.load().gpmdm_bank_set_gate(self._h, _lib.dptr(thr), lim), "set_gate")
        self._gate, self._gate_limit = ks, lim

    @property
    def gate(self):
        """The local filters' z-score thresholds as a tuple (None: that filter never rejects), or
        None when the gate is off."""
        return self._gate

    @property
    def gate_limit(self) -> float:
        return self._gate_limit

    def gate_report(self) -> BankGateReport:
        """``GPMDM_PF.gate_report`` for every local filter (gpmdm_bank_gate_report: one copy of the
        device tables and one wait): what each filter's gate decided for the frame the last
        ``update`` weighed, every field with a leading filter axis, row f bitwise the single
        filter's report.  No state change, no draw.  ValueError with the gate off, RuntimeError
        before the first update after ``reset`` / ``load_state`` / ``set_predictive`` /
        ``set_gate``."""
        if getattr(self, "_gate", None) is None:
            raise ValueError("gate_report: build the bank with gate=k or call set_gate(k)")
        Fl, D = self.local_filters, self.observation_dim
        zs = np.full((Fl, D), np.nan)
        ex, ga, us = (np.zeros((Fl, D), dtype=np.uint8) for _ in range(3))
        ng, nv, ov = np.zeros(Fl, dtype=np.int64), np.zeros(Fl, dtype=np.int64), np.zeros(Fl, dtype=np.int32)
        if self._h is not None:
            self._sync_model()
            out = _lib.GateOut(_lib.dptr(zs), *[ctypes.c_void_p(a.ctypes.data) for a in (ex, ga, us)],
                               _lib.i64ptr(ng), _lib.i64ptr(nv), ov.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
            _lib.check(_lib.load().gpmdm_bank_gate_report(self._h, ctypes.byref(out), self._stream()), "gate_report")
        thr = np.array([np.inf if k is None else k for k in self._gate], dtype=np.float64)
        b = lambda a: torch.from_numpy(a.astype(bool))   # noqa: E731
        return BankGateReport(torch.from_numpy(thr), torch.from_numpy(zs), b(ex), b(ga), b(us), torch.from_numpy(ng),
                              torch.from_numpy(nv), b(ov))

    def current_observation(self, spread: bool = True, gp_variance: bool = False):
        """(F_local, D): the filtered pose of every local filter, ``GPMDM_PF.current_observation``
        per filter -- the observation GP's mean averaged over the particles the filter holds
        now (after masked updates: with the unseen joints imputed) and, with ``spread``, the
        cloud's variance of each.  One pair of launches for the whole bank
        (gpmdm_bank_observation); no state change, no draw; the same clouds give bitwise the
        same values, and row f is bitwise a single filter's read-out of the same cloud."""
        Fl, D = self.local_filters, self.observation_dim
        mean = np.zeros((Fl, D))
        var = np.zeros((Fl, D)) if spread else None
        if self._h is not None:
            self._sync_model()
            _lib.check(_lib.load().gpmdm_bank_observation(self._h, _lib.dptr(mean), _lib.dptr(var), self._stream()),
                       "current_observation")
        res = (torch.from_numpy(mean), torch.from_numpy(var)) if spread else (torch.from_numpy(mean),)
        if gp_variance:                       # (GPMDM_PF.current_observation: the GP's own variance, per filter)
            if not self._predictive:
                raise ValueError("gp_variance: build the bank with predictive=True or call set_predictive(True)")
            gpv = np.zeros((Fl, D))
            if self._h is not None:
                _lib.check(_lib.load().gpmdm_bank_observation_gp(self._h, _lib.dptr(gpv), self._stream()),
                           "current_observation")
            res = res + (torch.from_numpy(gpv),)
        return res if len(res) > 1 else res[0]

    def current_observation_mean(self) -> torch.Tensor:
        """``current_observation``'s mean alone: (F_local, D)."""
        return self.current_observation(spread=False)

    def forecast(self, horizon: int, *, mode: str = "sample", observation: bool = True,
                 particles: bool = False, seed=None) -> Forecast:
        """``GPMDM_PF.forecast`` for every local filter in one sequence of launches
        (gpmdm_bank_forecast): the grouping and the dynamics tiles run once over all F x P
        particles, counts, sums and the pose read-out per filter.  Every field has a leading
        filter axis: ``class_probabilities`` (F_local, H, C), ``state_mean`` (F_local, H, d),
        the pose (F_local, H, D), with ``particles`` ``states`` (F_local, H, P, d) and
        ``classes`` (F_local, H, P).

        Filter f draws with the key ``seed + f`` (default: the bank's seed, i.e. the filter's
        own key) and its in-filter particle index, so row f is bitwise
        ``GPMDM_PF.forecast(horizon, seed=seed + f)`` of a single filter holding f's cloud at
        the same frame -- except ``state_mean``, which a bank sums per filter in particle order
        (the single filter sums in class-grouped order): the same mean to rounding, bitwise
        reproducible, independent of ``horizon`` and identical between a full bank and the
        shards of a sharded one.  The bank is not changed by the call."""
        # (the handle's filter 0 is the bank's filter f_lo)
        arrays = _forecast_call(self, None if self._h is None else "gpmdm_bank_forecast", (self.local_filters,),
                                horizon, mode, observation, particles, None if seed is None else int(seed) + self._f_lo)
        return Forecast(*map(_filter_major, arrays))

    def set_smoothing(self, lag: int):
        """``GPMDM_PF.set_smoothing`` for the bank (gpmdm_bank_set_smoothing): keep the last
        ``lag`` + 1 frames' ancestors, classes and states of every filter on the device; each
        update then records its frame with one more short launch.  ``lag=0`` turns smoothing
        off and releases the history (the bank then issues exactly the launches of a bank built
        without it).  Every call clears the history, as do ``reset``, ``load_state`` /
        ``import_state`` and a rebind to a rebuilt model; ``export_state`` does not carry it.
        Between updates only."""
        L = _check_smoothing_lag(lag)
        if self._h is not None:
            self._sync_model()
            _lib.check(_lib.load().gpmdm_bank_set_smoothing(self._h, L), "set_smoothing")
        self._smoothing_lag = L

    @property
    def smoothing_lag(self) -> int:
        return self._smoothing_lag

    @property
    def smoothing_depth(self) -> int:
        """min(smoothing lag, frames recorded since the history was last cleared): the largest
        lag ``smoothed`` serves now (every filter of the bank steps together)."""
        if not self._smoothing_lag or self._h is None:
            return 0
        self._sync_model()                      # (a rebuilt model clears the history)
        lag, depth = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().gpmdm_pf_smoothing_depth(self._h, ctypes.byref(lag), ctypes.byref(depth)),
                   "smoothing_depth")
        return depth.value

    def smoothed(self, lag=None, *, observation: bool = False, particles: bool = False) -> Smoothed:
        """``GPMDM_PF.smoothed`` for every local filter in one trace (gpmdm_bank_smoothed):
        each filter's current particles are traced back through its own recorded ancestors.
        ``lags`` and ``frames`` stay (n,); every other field has a leading filter axis --
        ``class_probabilities`` (F_local, n, C), ``state_mean`` (F_local, n, d),
        ``distinct_ancestors`` (F_local, n), the pose (F_local, n, D), with ``particles``
        ``ancestors`` (in-filter indices) and ``classes`` (F_local, n, P) and ``states``
        (F_local, n, P, d).  Row f is bitwise ``GPMDM_PF.smoothed`` of a single filter with the
        same history, ``state_mean`` included.  The bank is not changed by the call."""
        lags, rest = _smoothed_call(self, "bank", None if self._h is None else "gpmdm_bank_smoothed",
                                    (self.local_filters,), lag, observation, particles)
        return Smoothed(torch.from_numpy(lags), torch.from_numpy(self.frame - lags), *map(_filter_major, rest))

    def health(self, reset: bool = False) -> dict:
        """Failure counters of the local filters together since creation (or the last reset):
        ``GPMDM_PF.health`` (gpmdm_pf_health).  A blacked-out filter's frames add nothing."""
        n = np.zeros(len(_lib.HEALTH), dtype=np.int64)
        if self._h is not None:
            _lib.check(_lib.load().gpmdm_pf_health(self._h, _lib.i64ptr(n), 1 if reset else 0, self._stream()),
                       "health")
        return {k: int(v) for k, v in zip(_lib.HEALTH, n)}

    def gather_readouts(self) -> dict:
        """All filters' read-outs on every rank (one all-gather of F x (C + d + 1))."""
        post, mean, lik = self._read()
        rows = np.concatenate([post, mean, lik[:, None]], 1)
        if self._group is None:
            full = rows
        else:
            import torch.distributed as dist
            from .distributed import allgather_rows
            dev = self.device if dist.get_backend(self._group) != "gloo" else torch.device("cpu")
            send = torch.as_tensor(rows, dtype=torch.float64, device=dev)
            recv = torch.empty((self._num_filters, rows.shape[1]), dtype=torch.float64, device=dev)
            allgather_rows(recv, send, self._group)
            full = recv.cpu().numpy()
        C, d = self.num_classes, self.latent_dim
        return dict(class_probabilities=torch.tensor(full[:, :C]),
                    current_state_mean=torch.tensor(full[:, C:C + d]),
                    log_likelihood=torch.tensor(full[:, C + d]))

    # ---- properties -----------------------------------------------------------------
    @property
    def frame(self) -> int:
        """Resamples done so far (every filter of the bank steps together)."""
        f = np.zeros(1, dtype=np.int64)
        if self._h is not None:
            _lib.check(_lib.load().gpmdm_pf_frame(self._h, _lib.i64ptr(f)), "frame")
        return int(f[0])

    @property
    def num_filters(self):
        return self._num_filters

    @property
    def local_filters(self):
        return self._f_hi - self._f_lo

    @property
    def filter_range(self):
        return self._f_lo, self._f_hi

    @property
    def num_particles(self):
        return self._num_particles

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
