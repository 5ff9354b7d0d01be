"""tests/smooth_ref.py (the numpy restatement the GPU smoothing tests compare with) on a
genealogy written out by hand: P = 4 particles, three frames (a root and two resamples).

    frame 0 (root)   states (0,10) (1,11) (2,12) (3,13)      classes 0 1 1 0
    frame 1          ancestors 2 2 2 0                       classes 1 1 1 0
    frame 2          ancestors 1 1 0 2                       classes 0 0 1 1

From frame 2: lag 1 reaches particles 1 1 0 2 of frame 1 (three distinct), and through frame
1's ancestors 2 2 2 0 every one of them reaches particle 2 of the root: at lag 2 all four
current particles share one ancestor."""
import numpy as np
import pytest

import smooth_ref as R


def _history():
    f0 = dict(states=np.array([[0., 10.], [1., 11.], [2., 12.], [3., 13.]]), classes=np.array([0, 1, 1, 0]),
              resample_idx=np.array([3, 3, 3, 3]))            # the root's own indices are never read
    f1 = dict(states=np.array([[.5, 1.], [1.5, 2.], [2.5, 3.], [3.5, 4.]]), classes=np.array([1, 1, 1, 0]),
              resample_idx=np.array([2, 2, 2, 0]))
    f2 = dict(states=np.array([[-1., 0.], [-2., .25], [-3., .5], [-4., .75]]), classes=np.array([0, 0, 1, 1]),
              resample_idx=np.array([1, 1, 0, 2]))
    return [f0, f1, f2]


def test_hand_genealogy():
    s = R.smoothed(_history())
    assert np.array_equal(s["lags"], [0, 1, 2])
    assert np.array_equal(s["ancestors"], [[0, 1, 2, 3], [1, 1, 0, 2], [2, 2, 2, 2]])
    assert np.array_equal(s["classes"], [[0, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]])
    assert np.array_equal(s["class_counts"], [[2, 2], [0, 4], [0, 4]])
    assert np.array_equal(s["distinct_ancestors"], [4, 3, 1])
    assert np.array_equal(s["state_mean"], [[-2.5, .375], [1.5, 2.], [2., 12.]])
    assert np.array_equal(s["states"][1], [[1.5, 2.], [1.5, 2.], [.5, 1.], [2.5, 3.]])
    assert np.array_equal(s["states"][2], np.tile([2., 12.], (4, 1)))
    assert np.array_equal(R.class_probabilities(s, 3), [[.5, .5, 0.], [0., 1., 0.], [0., 1., 0.]])


def test_ranges_and_depth():
    h = _history()
    full = R.smoothed(h)
    one = R.smoothed(h, 2, 2)
    assert np.array_equal(one["lags"], [2]) and np.array_equal(one["ancestors"], full["ancestors"][2:])
    assert np.array_equal(one["state_mean"], full["state_mean"][2:])
    part = R.smoothed(h, 1, 2)
    assert np.array_equal(part["states"], full["states"][1:])
    # a shorter history: frame 1 is the latest, the root one step behind it
    s = R.smoothed(h[:2])
    assert np.array_equal(s["ancestors"], [[0, 1, 2, 3], [2, 2, 2, 0]])
    assert np.array_equal(s["distinct_ancestors"], [4, 2])
    assert np.array_equal(s["state_mean"][1], [(2 + 2 + 2 + 0) / 4, (12 + 12 + 12 + 10) / 4])
    # the root alone: lag 0 only
    assert np.array_equal(R.smoothed(h[:1])["ancestors"], [[0, 1, 2, 3]])
    for bad in ((0, 3), (2, 1), (-1, 0)):
        with pytest.raises(ValueError):
            R.smoothed(h, *bad)


def test_mean_is_the_correctly_rounded_sum():
    """fsum, not a running sum: 1e16 + 1 + 1 - 1e16 = 2 exactly."""
    f = dict(states=np.array([[1e16], [1.], [1.], [-1e16]]), classes=np.zeros(4, dtype=np.int64),
             resample_idx=np.arange(4))
    assert R.smoothed([f])["state_mean"][0, 0] == 0.5
