"""GPU: outlier gating inside a bank's ``update`` (``GPMDM_PF_Bank(gate=...)``, gpmdm_bank_set_gate /
gpmdm_bank_gate_report; csrc/obs_gate.h with the filter as a grid dimension).

The reference for every case is the set of F independent single filters
``GPMDM_PF(rng="philox", seed=seed + f, predictive=True, gate=k_f)`` loaded from the bank's
exported initial cloud.  tests/test_gpu_gate.py ties the single gated filter to gate_ref.py and the
masked twin; the bank only has to equal it bit for bit, so no tolerance appears here.  Before the
equalities every decision of the mixed frame is checked to be decisive against tests/innov_ref.py on
the ungated predictive twin's cloud: a z-score meant to be rejected clears the threshold by more
than 1, one meant to be kept stays more than 1 below (the device's z-score error is of order 1e-8,
tests/test_gpu_innovation.py).

Shapes: Pf = 100 is two 64-particle tiles per filter, the second partial, and takes the deferred
likelihood finish; Pf = 257 (systematic) is two blocks of 256 per filter with one particle in the
second; Pf = 1500 on config 2 runs k_obs_ll (several blocks per filter).
"""
import math

import numpy as np
import pytest
import torch

import innov_ref as R
from conftest import oracle_model, product_model

pytestmark = pytest.mark.gpu

KEYS = ("states", "classes", "ll", "log_w", "w", "resample_idx", "frame")
REPORT = ("zscore", "exceeded", "gated", "used", "n_gated", "n_valid", "overflow")
SEED = 500
K = 6.0
ROW0 = 200                       # the first frame's row of Y (filter f: ROW0 + frame + 7 f)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def il2_of(m):
    return (torch.exp(m._host("y_log_lambdas")) ** -2).numpy().astype(np.float64).reshape(-1)


@pytest.fixture(scope="module")
def c1(fx_config1):
    return product_model(fx_config1), oracle_model(fx_config1), fx_config1


@pytest.fixture(scope="module")
def c2(fx_config2):
    return product_model(fx_config2), oracle_model(fx_config2), fx_config2


def make_bank(m, fx, F, P, resample="multinomial", **kw):
    from gpmdm_amd import GPMDM_PF_Bank
    return GPMDM_PF_Bank(m, torch.tensor(fx["T"]), F, P, seed=SEED, resample=resample, **kw)


def make_singles(m, fx, bank, ks, resample="multinomial", lo=0):
    """One single filter per local filter of ``bank`` (a fresh bank), loaded from its exported
    cloud; ks[f] None: the predictive filter with no gate."""
    from gpmdm_amd import GPMDM_PF
    st0 = bank.export_state()
    out = []
    for f, k in enumerate(ks):
        kw = dict(predictive=True) if k is None else dict(gate=k)
        pf = GPMDM_PF(m, torch.tensor(fx["T"]), bank.num_particles, rng="philox", seed=SEED + lo + f, resample=resample,
                      **kw)
        pf.load_state(st0["states"][f], st0["classes"][f])
        out.append(pf)
    return out


def frames(m, F, n, row0=ROW0):
    Y = f64(m.get_Y())
    return [np.stack([Y[(row0 + k + 7 * f) % Y.shape[0]] for f in range(F)]) for k in range(n)]


def clean_reference(m, om, fx, F, P, resample, warm, Zc):
    """The ungated predictive bank stepped on ``warm`` and then the clean frame: per filter the
    oracle's means of the propagated cloud, the device's vc and innov_ref on the clean frame."""
    il2 = il2_of(m)
    tw = make_bank(m, fx, F, P, resample, predictive=True)
    for Z in warm:
        tw.update(Z)
    tw.update(Zc)
    inn = tw.innovation(particles=True)
    mu = [f64(om.map_x_to_y(inn.states[f].numpy())[0]) for f in range(F)]
    vc = [inn.variance_common[f].numpy() for f in range(F)]
    return mu, vc, [R.innovation(mu[f], vc[f], Zc[f], None, il2) for f in range(F)]


def shifted(z, ref, want, sigmas=10.0):
    """z with the joints in ``want`` moved ``sigmas`` standard deviations away from the cloud's
    mean, on the side the clean residual is on (so |zscore| >= sigmas there)."""
    side = np.where(f64(ref.residual) < 0, -1.0, 1.0)
    return z + np.where(want, sigmas * side * np.sqrt(f64(ref.variance)), 0.0)


def check_decisive(ref, obs, want, k, what):
    zs = np.abs(f64(ref.zscore))
    keep = obs & ~want
    print(f"{what}: k {k}, kept max |z| {float(np.max(zs[keep], initial=0.0)):.3f}, "
          f"rejected min |z| {float(np.min(zs[want], initial=np.inf)):.3f}")
    assert np.all(zs[keep] < k - 1), (what, float(np.max(zs[keep])))
    assert np.all(zs[want] > k + 1), (what, float(np.min(zs[want])))


def readouts(x):
    lik = x.log_likelihood()
    return [x.class_probabilities().numpy(), x.current_state_mean().numpy(), f64(lik),
            *(t.numpy() for t in x.current_observation())]


def assert_rows_equal(bank, singles, what, reports=True, gates=None):
    """Every key of export_state(), the read-outs and (gated singles) every field of the report
    row: the bank's row f is the single filter f, bit for bit."""
    b = bank.export_state()
    rb = readouts(bank)
    rep = bank.gate_report() if reports else None
    for f, pf in enumerate(singles):
        s = pf.export_state()
        for key in KEYS:
            assert same(b[key][f] if key != "frame" else b[key], s[key]), (what, f, key)
        for x, y in zip(rb, readouts(pf)):
            assert same(x[f], y), (what, f)
        if reports and pf.gate is not None:
            rs = pf.gate_report()
            assert float(rep.threshold[f]) == rs.threshold, (what, f)
            for name in REPORT:
                assert same(getattr(rep, name)[f].numpy(), np.asarray(getattr(rs, name))), (what, f, name)
    return b, rep


def mixed_frame(m, om, fx, F, P, resample):
    """Two warm frames and the third, on which filter 0 has one corrupted joint, filter 1 is clean,
    filter 2 has more corrupted joints than the cap allows and (F = 5) filter 3 a caller's mask
    with a corrupted observed joint and filter 4 a blackout.  Returns warm, Z, observed (None when
    F = 3), and per filter the joints meant to exceed."""
    D = m.get_Y().shape[1]
    il2 = il2_of(m)
    warm = frames(m, F, 2)
    Zc = frames(m, F, 3)[2]
    mu, vc, clean = clean_reference(m, om, fx, F, P, resample, warm, Zc)
    j0 = min(17, D - 1)
    cap = math.floor(0.5 * D)
    obs = np.ones((F, D), bool)
    want = np.zeros((F, D), bool)
    want[0, j0] = True
    want[2, :cap + 1] = True
    if F == 5:
        obs[3, D // 3:2 * D // 3] = False
        assert obs[3, j0]
        want[3, j0] = True
        obs[4] = False
    Z = np.stack([shifted(Zc[f], clean[f], want[f]) for f in range(F)])
    Z[~obs] = np.nan
    if F == 5:
        Z[3, D // 3 + 1] = 1e30                      # unobserved: never looked at
    for f in range(F):
        if obs[f].any():
            ref = R.innovation(mu[f], vc[f], np.where(obs[f], Z[f], 0.0), obs[f], il2)
            check_decisive(ref, obs[f], want[f], K, f"mixed F={F} P={P} filter {f}")
    return warm, Z, (obs if F == 5 else None), want, cap


def run_mixed(m, om, fx, F, P, resample):
    warm, Z, obs, want, cap = mixed_frame(m, om, fx, F, P, resample)
    D = Z.shape[1]
    bank = make_bank(m, fx, F, P, resample, predictive=True, gate=K)
    assert bank.gate == (K,) * F and bank.gate_limit == 0.5 and bank.predictive is True
    ks = [K] * F
    ks[1] = None                                     # filter 1's single: predictive, no gate at all
    singles = make_singles(m, fx, bank, ks, resample)
    gated1 = make_singles(m, fx, bank, [K, K], resample)[1]   # ... and the gated one, for its report row
    for Zw in warm:
        bank.update(Zw)
        for f, pf in enumerate(singles):
            pf.update(Zw[f])
        gated1.update(Zw[1])
        rep = bank.gate_report()
        assert not rep.n_gated.any() and not rep.overflow.any() and rep.used.all()
    if obs is None:
        bank.update(Z)
    else:
        bank.update(Z, observed=obs)
    for f, pf in list(enumerate(singles)) + [(1, gated1)]:
        if obs is None:
            pf.update(Z[f])
        else:
            pf.update(Z[f], observed=obs[f])
    what = f"mixed F={F} P={P}"
    b, rep = assert_rows_equal(bank, singles, what)
    singles[1] = gated1
    assert_rows_equal(bank, singles, what + " (gated single 1)")
    # the fates
    o = np.ones((F, D), bool) if obs is None else obs
    assert same(rep.exceeded.numpy(), want), what
    assert rep.n_gated.tolist()[:3] == [1, 0, 0] and rep.overflow.tolist()[:3] == [False, False, True], what
    assert same(rep.gated[0].numpy(), want[0]) and not rep.gated[1].any() and not rep.gated[2].any(), what
    assert int(want[2].sum()) == cap + 1 and rep.used[2].all(), what
    assert same(rep.used[0].numpy(), ~want[0]) and rep.used[1].all(), what
    if F == 5:
        assert int(rep.n_gated[3]) == 1 and same(rep.used[3].numpy(), o[3] & ~want[3]), what
        assert same(np.isnan(rep.zscore[3].numpy()), ~o[3]), what
        assert int(rep.n_gated[4]) == 0 and int(rep.n_valid[4]) == 0 and not bool(rep.overflow[4]), what
        assert np.all(np.isnan(rep.zscore[4].numpy())), what
        assert not rep.used[4].any() and not rep.exceeded[4].any() and not rep.gated[4].any(), what
        assert np.all(b["ll"][4] == 0.0) and np.all(b["w"][4] == 1.0 / P), what
    assert bank.health() == {key: 0 for key in bank.health()}, what


# ---- 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,P,resample", [(5, 100, "multinomial"), (3, 257, "systematic")])
def test_mixed_bank(c1, F, P, resample):
    run_mixed(*c1, F, P, resample)


# ---- 2 ---------------------------------------------------------------------------------------
def test_block_maxima(c2):
    """Config 2, Pf = 1500: the singles' k_obs_ll writes block maxima and their k_gate_finish
    rewrites them; the bank's normaliser takes each filter's maximum from ll -- the same bits."""
    m, om, fx = c2
    F, P = 2, 1500
    D = m.get_Y().shape[1]
    warm = frames(m, F, 2)
    Zc = frames(m, F, 3)[2]
    mu, vc, clean = clean_reference(m, om, fx, F, P, "multinomial", warm, Zc)
    want = np.zeros((F, D), bool)
    want[0, 17] = True
    Z = np.stack([shifted(Zc[f], clean[f], want[f]) for f in range(F)])
    for f in range(F):
        check_decisive(R.innovation(mu[f], vc[f], Z[f], None, il2_of(m)), np.ones(D, bool), want[f], K,
                       f"block maxima filter {f}")
    bank = make_bank(m, fx, F, P, predictive=True, gate=K)
    singles = make_singles(m, fx, bank, [K, None])
    for Zf in warm + [Z]:
        bank.update(Zf)
        for f, pf in enumerate(singles):
            pf.update(Zf[f])
    _, rep = assert_rows_equal(bank, singles, "block maxima")
    assert rep.n_gated.tolist() == [1, 0] and same(rep.gated.numpy(), want) and not rep.overflow.any()


# ---- 3 ---------------------------------------------------------------------------------------
def test_per_filter_thresholds(c1):
    m, om, fx = c1
    F, P = 3, 100
    D = m.get_Y().shape[1]
    ks = [6.0, None, 3.0]
    warm = frames(m, F, 2)
    Zc = frames(m, F, 3)[2]
    _, _, clean = clean_reference(m, om, fx, F, P, "multinomial", warm, Zc)
    want = np.zeros((F, D), bool)
    want[1, min(17, D - 1)] = True
    Z = np.stack([shifted(Zc[f], clean[f], want[f]) for f in range(F)])
    bank = make_bank(m, fx, F, P, predictive=True, gate=ks)
    assert bank.gate == (6.0, None, 3.0)
    singles = make_singles(m, fx, bank, ks)
    for Zf in warm + [Z]:
        bank.update(Zf)
        for f, pf in enumerate(singles):
            pf.update(Zf[f])
    _, rep = assert_rows_equal(bank, singles, "per-filter thresholds")
    assert rep.threshold.tolist() == [6.0, math.inf, 3.0]
    assert abs(float(rep.zscore[1, min(17, D - 1)])) > 9.0          # the 10 sigma joint, seen and kept
    assert not rep.exceeded[1].any() and not rep.gated[1].any() and rep.used[1].all()
    assert int(rep.n_gated[1]) == 0 and not bool(rep.overflow[1]) and int(rep.n_valid[1]) == P


# ---- 4 ---------------------------------------------------------------------------------------
def test_clean_streams_are_the_ungated_bank(c1):
    m, om, fx = c1
    F, P, n = 5, 100, 8
    Zs = frames(m, F, n, row0=300)
    off = make_bank(m, fx, F, P, predictive=True)
    out_off, zmax = [], 0.0
    for Z in Zs:
        off.update(Z)
        zmax = max(zmax, float(np.max(np.abs(off.innovation().zscore.numpy()))))
        out_off.append(readouts(off))
    thr = 1 + math.ceil(zmax)
    print(f"clean bank stream: max |z| {zmax:.3f}, threshold {thr}")
    on = make_bank(m, fx, F, P, predictive=True, gate=thr)
    for k, Z in enumerate(Zs):
        on.update(Z)
        rep = on.gate_report()
        assert not rep.n_gated.any() and not rep.overflow.any() and not rep.gated.any() and rep.used.all(), k
        assert all(same(x, y) for x, y in zip(readouts(on), out_off[k])), k
    sa, sb = on.export_state(), off.export_state()
    for key in KEYS:
        assert same(sa[key], sb[key]), key
    assert on.health() == off.health() and on.frame == off.frame


# ---- 5 ---------------------------------------------------------------------------------------
def test_shards(c1):
    m, om, fx = c1
    F, P = 4, 100
    D = m.get_Y().shape[1]
    ks = [6.0, 5.0, None, 6.0]
    warm = frames(m, F, 2)
    Zc = frames(m, F, 3)[2]
    _, _, clean = clean_reference(m, om, fx, F, P, "multinomial", warm, Zc)
    want = np.zeros((F, D), bool)
    want[1, 3] = want[2, 5] = want[3, 7] = True
    Z = np.stack([shifted(Zc[f], clean[f], want[f]) for f in range(F)])
    full = make_bank(m, fx, F, P, predictive=True, gate=ks)
    shards = [make_bank(m, fx, F, P, predictive=True, gate=ks, shard=(2, r)) for r in range(2)]
    assert shards[0].gate == (6.0, 5.0) and shards[1].gate == (None, 6.0)
    for Zf in warm + [Z]:
        for bnk in [full] + shards:
            bnk.update(Zf)
    sf, rf, of = full.export_state(), full.gate_report(), readouts(full)
    assert rf.n_gated.tolist() == [0, 1, 0, 1]
    for r, sh in enumerate(shards):
        lo, hi = sh.filter_range
        assert (lo, hi) == (2 * r, 2 * r + 2)
        ss, rs = sh.export_state(), sh.gate_report()
        for key in KEYS[:-1]:
            assert same(ss[key], sf[key][lo:hi]), (r, key)
        for x, y in zip(readouts(sh), of):
            assert same(x, y[lo:hi]), r
        for name in ("threshold",) + REPORT:
            assert same(getattr(rs, name).numpy(), getattr(rf, name)[lo:hi].numpy()), (r, name)


# ---- 6 ---------------------------------------------------------------------------------------
def test_repeatability_and_switches(c1):
    from gpmdm_amd import GPMDM_PF_Bank, _lib
    lib = _lib.load()
    m, om, fx = c1
    F, P = 3, 100
    T = torch.tensor(fx["T"])
    warm, Z, _, want, _ = mixed_frame(m, om, fx, F, P, "multinomial")
    runs = []
    for _ in range(2):
        bank = make_bank(m, fx, F, P, predictive=True, gate=K)
        with pytest.raises(RuntimeError):               # before the first update
            bank.gate_report()
        for Zf in warm + [Z]:
            bank.update(Zf)
        runs.append((bank.export_state(), bank.gate_report(), readouts(bank)))
    (sa, ra, oa), (sb, rb, ob) = runs
    for key in KEYS:
        assert same(sa[key], sb[key]), key
    assert all(same(getattr(ra, n).numpy(), getattr(rb, n).numpy()) for n in ("threshold",) + REPORT)
    assert all(same(x, y) for x, y in zip(oa, ob))
    assert int(ra.n_gated[0]) == 1
    # set_gate(None): the ungated frame, bit for bit
    off = make_bank(m, fx, F, P, predictive=True)
    off.import_state(sa)
    bank.set_gate(None)
    assert bank.gate is None and bank.predictive is True
    with pytest.raises(ValueError):
        bank.gate_report()
    s = bank._stream()
    assert lib.gpmdm_bank_gate_report(bank._h, _lib.GateOut(), s) == _lib.GPMDM_E_INVALID
    Z4 = frames(m, F, 4)[3]
    Z4[0, 5] += 1e3                                      # (an outlier nobody rejects now)
    bank.update(Z4)
    off.update(Z4)
    sa, sb = bank.export_state(), off.export_state()
    for key in KEYS:
        assert same(sa[key], sb[key]), key
    # a new gate invalidates the report; set_predictive(False) is refused while gated
    bank.set_gate([6.0, None, 4.0], 0.25)
    assert bank.gate == (6.0, None, 4.0) and bank.gate_limit == 0.25
    with pytest.raises(RuntimeError):
        bank.gate_report()
    with pytest.raises(ValueError):
        bank.set_predictive(False)
    assert lib.gpmdm_bank_set_predictive(bank._h, 0) == _lib.GPMDM_E_STATE
    # the library's own checks
    thr = np.array([6.0, 0.0, 6.0])
    assert lib.gpmdm_bank_set_gate(bank._h, _lib.dptr(thr), 0.5) == _lib.GPMDM_E_INVALID     # on and off mixed
    thr = np.array([6.0, np.nan, 6.0])
    assert lib.gpmdm_bank_set_gate(bank._h, _lib.dptr(thr), 0.5) == _lib.GPMDM_E_INVALID
    thr = np.array([6.0, 6.0, 6.0])
    assert lib.gpmdm_bank_set_gate(bank._h, _lib.dptr(thr), 1.5) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_bank_set_gate(bank._h, None, 0.5) == _lib.GPMDM_E_INVALID
    # a bank handle is not a single filter's
    assert lib.gpmdm_pf_set_gate(bank._h, 6.0, 0.5) == _lib.GPMDM_E_INVALID
    assert lib.gpmdm_pf_gate_report(bank._h, _lib.GateOut(), s) == _lib.GPMDM_E_INVALID
    bank.update(frames(m, F, 5)[4])
    assert bank.gate_report().threshold.tolist() == [6.0, math.inf, 4.0]   # (the refused calls changed nothing)
    # gate without predictive, a wrong-length sequence
    with pytest.raises(ValueError, match="predictive"):
        GPMDM_PF_Bank(m, T, F, P, seed=SEED, gate=6.0)
    plain = GPMDM_PF_Bank(m, T, F, P, seed=SEED)
    with pytest.raises(ValueError, match="predictive"):
        plain.set_gate(6.0)
    assert lib.gpmdm_bank_set_gate(plain._h, _lib.dptr(thr), 0.5) == _lib.GPMDM_E_STATE
    with pytest.raises(ValueError, match="gate"):
        GPMDM_PF_Bank(m, T, F, P, seed=SEED, predictive=True, gate=[6.0, 6.0])
    with pytest.raises(ValueError, match="gate"):
        bank.set_gate([6.0] * 4)
