"""CPU restatement of the forecast roll-out's draws and of one roll-out step (test helper).

``GPMDM_PF.forecast`` (gpmdm_pf_forecast, csrc/forecast.h) draws with Philox4x32-10 under the
filter's key and the counter

    (particle index, frame, stream, (h << 8) | pair),   h = 1..H the roll-out step,

stream 4 for the switch's Exp(1) draws and 5 for the dynamics normals, ``pair = j >> 1`` of
class / dimension j, through the transforms of the filter's own draws (``oracle.philox``):
``E = -log u`` with u in (0, 1); Box-Muller from a (0, 1) and a [0, 1) uniform, the second
normal of a pair unused at odd d.  One step is the oracle's ``switch_classes`` followed by
``propagate_dynamics`` with those draws regrouped by class, as a filter step's proposal is.
"""
from __future__ import annotations

import numpy as np

from oracle import gpmdm_oracle as O
from oracle import philox as ph

STREAM_FORECAST_SWITCH, STREAM_FORECAST_DYN = 4, 5


def _sub(h: int, n_pairs: int) -> np.ndarray:
    return (np.uint32(h << 8) | np.arange(n_pairs, dtype=np.uint32))[None, :]


def switch_draws(seed: int, frame: int, h: int, P: int, C: int) -> np.ndarray:
    """P x C Exp(1) draws of roll-out step h."""
    k0, k1 = ph.filter_key(seed)
    p = np.arange(P, dtype=np.uint32)[:, None]
    x, y, z, w = ph.philox4x32_10(p, np.uint32(frame), np.uint32(STREAM_FORECAST_SWITCH), _sub(h, (C + 1) // 2),
                                  k0, k1)
    E = np.empty((P, 2 * ((C + 1) // 2)))
    E[:, 0::2] = -np.log(ph.u01_oo(x, y))
    E[:, 1::2] = -np.log(ph.u01_oo(z, w))
    return E[:, :C]


def dynamics_normals(seed: int, frame: int, h: int, P: int, d: int) -> np.ndarray:
    """P x d standard normals of roll-out step h, by particle index."""
    k0, k1 = ph.filter_key(seed)
    p = np.arange(P, dtype=np.uint32)[:, None]
    x, y, z, w = ph.philox4x32_10(p, np.uint32(frame), np.uint32(STREAM_FORECAST_DYN), _sub(h, (d + 1) // 2),
                                  k0, k1)
    u1, u2 = ph.u01_oo(x, y), ph.u01_co(z, w)
    rr = np.sqrt(-2.0 * np.log(u1))
    t = 6.283185307179586476925 * u2
    out = np.empty((P, 2 * ((d + 1) // 2)))
    out[:, 0::2] = rr * np.cos(t)
    out[:, 1::2] = rr * np.sin(t)
    return out[:, :d]


def switch_step(classes, T, seed: int, frame: int, h: int) -> np.ndarray:
    """The classes after roll-out step h's switch."""
    T = np.asarray(T, dtype=np.float64)
    return O.switch_classes(np.asarray(classes), T, switch_draws(seed, frame, h, len(classes), T.shape[0]))


def sample_step(om, T, states, classes, seed: int, frame: int, h: int):
    """(classes, states) after roll-out step h from the cloud before it."""
    C = np.asarray(T).shape[0]
    cls = switch_step(classes, T, seed, frame, h)
    eps = ph.grouped_normals(dynamics_normals(seed, frame, h, states.shape[0], states.shape[1]), cls, C)
    return cls, O.propagate_dynamics(om, states, cls, eps)


def mean_step(om, states, classes) -> np.ndarray:
    """mode="mean": each particle's class dynamics-GP mean."""
    out = np.empty_like(states)
    for c in range(om.n_classes):
        idx = np.nonzero(classes == c)[0]
        if idx.shape[0]:
            out[idx] = om.map_x_dynamics_for_class(states[idx], c)[0]
    return out
