"""Benchmark: GPMDM particle-filter step on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
                    [--config {1,2,3,4,5}] [--rng {auto,philox,torch}]
                    [--stream {mocap,predictive}] [--y-lambda L]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run does only what the headline needs: it builds the model and the filter, runs W
warm-up frames, times K frames and prints the line (the contract fields, ``ms_per_step``,
``config``, ``roofline``, ``posterior_last``).  ``--full`` adds, after the timed frames,
every other measurement and check listed below (``stages_ms_per_step``, ``nodedup``, ``ess_*``,
``dyn_rows_last``, ``replay``, ``bank``, ``spread``, ``cutoff``, ``library_exchange``,
``cpu_baseline``) with their own options; without ``--full`` those options are accepted and
do nothing.  The timed loop, and so ``value`` and ``ms_per_step``, is the same either way.

``--dump-outputs DIR`` writes what the caller of the timed step received in the last timed
frame as float64 ``DIR/<name>.npy``: ``most_likely_class`` (1,), ``class_probabilities`` (C,)
and ``current_state_mean`` (d,).  Model, observation stream and seeds are fixed, so the same
arguments give the same inputs in every run and two builds can be compared array for array.

``--gpus N`` (N > 1) without a launcher around it starts N worker processes itself (one per
GPU, RANK / LOCAL_RANK / WORLD_SIZE in their environment, before anything touches the GPU)
and forwards rank 0's line; fewer visible GPUs than N is an error (exit 2) unless
``--rehearse-gloo`` asks for a time-shared gloo rehearsal.  The line reports the world size
the backend saw (``world_size_backend``), the backend, the launcher and the exchange; RCCL
runs add ``library_exchange``: the same filter over the library's own communicator
(gpmdm_pf_set_comm), timed and checked bit for bit against the process-group filter.

Workload (BASELINE.json configs[1]): N=2000 training latents, D=62, d=3, C=2 classes, 500 frames,
P=100,000 particles per GPU (weak scaling: P_total = 100k x GPUs), synthetic model and
observation stream.  One step = ``update(z)`` + ``class_probabilities()``
+ ``current_state_mean()``, the notebook's per-frame loop (test_gpmdm_pf.ipynb:197-201),
with device-side Philox draws and the reference's multinomial resampling.
``--config 3|4|5`` runs the other BASELINE.json configurations (per-GPU share of P for
the 8-GPU ones); they are not the headline line.

``--config 1`` is the notebook's own filter (N=500, P=100) in the drop-in's default mode:
``rng='torch'`` (host draws from torch's generator in the reference's order, uploaded per
frame) and multinomial resampling; the line adds ``ms_per_frame`` beside the reference's
published 78.2 ms/frame (test_gpmdm_pf.ipynb:259-260) and its 16.3 ms measured in the
build container, and ``bank``: the 39-trial loop of test_gpmdm_pf.ipynb
cell 4 as one GPMDM_PF_Bank of 39 filters x 100 particles stepped per frame.

``--stream predictive`` replaces the mocap-surrogate observation stream by one drawn from
the filter's own predictive distribution: a first, untimed pass of the same filter (same
seed) takes at each frame a random particle x_r of the current cloud and observes
z = mu(x_r) + sqrt(var(x_r)) eps (map_x_to_y); the timed pass replays those z on a fresh
filter, which follows the same trajectory bit for bit (checked).  ``--y-lambda`` sets the
observation GP's output scales (exp(y_log_lambdas)); below 1 the likelihood is less peaked.
Together they keep the cloud spread out (ESS well above the mocap stream's ~0.3%), so the
resample path and the dynamics tiles are timed on many distinct ancestors.

Prints ONE JSON line (rank 0) with the contract fields plus (every field after ``roofline``
only with ``--full``):
  roofline      dominant kernel (observation-GP tile kernel) vs the FP64 MFMA peak;
                achieved = algorithmic FLOPs per launch (triangular form N(N+1) + 2N + 2ND
                per particle; SURVEY §8(d)'s dense 2N^2 + 2ND is reported beside it) / mean
                launch time from HIP events on the launch stream; traffic = HBM bytes per
                launch of the same kernel from the committed rocprofv3 PMC passes of this
                bench command (profiles/r06_pmc_summary.json; its "commit" field names the
                build it measured -- the driver's bench run has no profiler attached), or null
  cpu_baseline  the CPU oracle (numpy fp64) on this configuration's own particle count
                for N <= 2000 (a bounded sample of frames), a 1000-particle sample above;
                cores = BLAS threads it ran on, with nproc and torch's thread count beside
  stages_ms_per_step  per-stage device time from a separate 10-step pass after the timed
                region (inside it only the roofline kernel records events: 2 per step)
  nodedup       the same step with ancestor de-duplication off (every particle's dynamics
                GP evaluated, as the reference does): ms/step, throughput and stages -- the
                headline's dynamics stage is cheap partly because resampling collapses the
                cloud onto few ancestors; this line does not depend on that
  ess_last      effective sample size 1 / sum w^2 of the last timed step's weights
  spread        (config 2, one GPU) the same step on a cloud that stays spread out
                (spread_line: less peaked observation GP + predictive stream), with its
                ESS, dynamics rows per frame, stage times and dynamics-tile TF/s
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

METRIC = "particle-steps/sec (P×timesteps) + achieved HBM GB/s, N=2000 D=62 d=3"
FP64_MFMA_PEAK_TFLOPS = 78.6          # MI355X spec (dense FP64 matrix); measured 77.1 (profiles/)
# The reference's only published throughput for this path: P = 100 particles
# at 12.78 frames/s on the author's laptop CPU (test_gpmdm_pf.ipynb:79, 259-260).  It is the
# notebook's own configuration, not configs[1]'s N/P, so it is NOT this metric's baseline:
# vs_baseline stays null and the figure is reported beside the line (published_reference);
# cpu_baseline is the same-box, same-configuration comparison.
PUBLISHED_PARTICLE_STEPS = 100 * 12.78
PUBLISHED_BASIS = ("the reference's published frame rate, 12.78 FPS x P=100 = 1.278e3 particle-steps/s "
                   "(author's laptop CPU, test_gpmdm_pf.ipynb:259-260; BASELINE.md §1), quoted at the "
                   "notebook's own model (N=500) and P=100, not configs[1]'s: a different workload, so no "
                   "vs_baseline; cpu_baseline is the same-box comparison on this configuration")
# per-GPU particles: configs 4 and 5 are quoted on 8 GPUs
P_PER_GPU = {1: 100, 2: 100_000, 3: 100_000, 4: 125_000, 5: 125_000}
WORKLOAD = None


def workload(cfg):
    from gpmdm_amd import synthetic
    c = synthetic.CONFIGS[cfg]
    # y_lambda: the observation GP's exp(y_log_lambdas) (1.0: the headline's mocap model;
    # --y-lambda for the spread stream); tools that import bench get the default
    return dict(cfg=cfg, C=c["C"], S=c["S"], L=c["L"], D=c["D"], d=c["d"], P_per_gpu=P_PER_GPU[cfg], y_lambda=1.0)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_model(device):
    from gpmdm_amd import GPMDM, synthetic
    w = WORKLOAD
    data = synthetic.make_sequences(w["C"], w["S"], w["L"], w["D"], w["d"], seed=0)
    hp = synthetic.default_hyperparameters(w["D"], w["d"], 0.1)
    hp["y_lambdas_init"] = hp["y_lambdas_init"] * w["y_lambda"]
    m = GPMDM(D=w["D"], d=w["d"], n_classes=w["C"], dyn_target="full", dyn_back_step=1, device=device, **hp)
    for c in range(w["C"]):
        for y in data.sequences[c]:
            m.add_data(y, c)
    m.init_X()
    return m, data


def obs_kernel_flops(N, D, bk=16):
    """FLOPs per particle of the observation-GP tile kernel.

    algorithmic: the implemented algorithm's useful work -- R^T k with R upper
        triangular (column j has j+1 non-zeros: N(N+1)), the sum of squares (2N) and the
        mean k^T beta (2ND).  This is what roofline.achieved counts.
    dense_form: SURVEY §8(d)'s 2N^2 + 2ND (the reference's dense K^-1 quadratic form);
        it is twice the work actually required, so it is reported, not used as achieved.
    executed: what the MFMAs issue: each 16-column tile runs K-steps of 16 rows up to its
        diagonal (mean tiles: all rows).
    """
    algorithmic = N * (N + 1.0) + 2.0 * N + 2.0 * N * D
    dense_form = 2.0 * N * N + 2.0 * N * D
    rows = 0
    for tc in range(-(-(N + D) // 16)):
        kmax = min(tc * 16 + 16, N)
        rows += -(-kmax // bk) * bk
    executed = 2.0 * 16 * rows
    return algorithmic, dense_form, executed


def dyn_row_flops(model):
    """Algorithmic FLOPs of one dynamics-GP row (triangular R_c^T k plus the mean weights),
    averaged over the classes."""
    rows = model._class_dynamics_rows()
    return sum(n * (n + 1.0) + 2.0 * n * model.d for n in rows) / len(rows)


def obs_model_bytes(N, D):
    """Algorithmic model bytes of the observation GP: the non-zeros of triu(R) and K^-1 Y."""
    return 8.0 * (N * (N + 1) / 2 + N * D)


def pmc_traffic(cfg):
    """(HBM bytes per launch of the obs tile kernel, source note) from the committed
    rocprofv3 PMC summary of this bench command (tools/pmc_passes.sh + tools/pmc_summary.py)."""
    for name in ("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json", "pmc_summary.json"):
        p = ROOT / "profiles" / name
        if not p.exists():
            continue
        try:
            j = json.loads(p.read_text())
        except Exception:
            continue
        key = "obs_gemm_hbm_bytes_per_launch" if cfg == 2 else f"config{cfg}_obs_gemm_hbm_bytes_per_launch"
        if j.get(key) is not None:
            sub = j if cfg == 2 else j.get(f"config{cfg}", {})   # each configuration's passes name their build
            commit = sub.get("commit") or j.get("commit") or "unrecorded"
            return j[key], (f"profiles/{name}: rocprofv3 --pmc passes (FETCH_SIZE x2 + WRITE_SIZE, gfx950 "
                            f"correction) of bench.py --config {cfg} at commit {commit}")
    return None, None


def host_cores():
    """(threads the environment caps BLAS at, cores this process may run on, nproc)."""
    nproc = os.cpu_count() or 1
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = nproc
    quota = cgroup_cpu_quota()          # a CFS quota caps the CPUs this process really gets
    if quota:
        usable = max(1, min(usable, int(np.ceil(quota))))
    capped = None
    for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        v = os.environ.get(k)
        if v and v.isdigit():
            capped = int(v)
            break
    return capped, usable, nproc


def cgroup_cpu_quota():
    """CPUs the cgroup's CFS quota allows (cgroup v2 cpu.max), or None."""
    try:
        q, per = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        return None if q == "max" else int(q) / int(per)
    except Exception:
        return None


def cpu_baseline(data, budget_s=12.0):
    """The numpy oracle on the same workload: this configuration's own particle count when
    N <= 2000 (configs 1, 2, 4: a few frames of P = 100k / 125k), a 1000-particle sample
    above.  Runs once on every core this process may use (threadpoolctl sets the BLAS pool;
    ``cores``) and, when the environment caps the BLAS threads (OMP_NUM_THREADS on the GPU
    box), once more at that cap (``capped``)."""
    from oracle import gpmdm_oracle as O
    from gpmdm_amd import synthetic
    import contextlib
    import torch
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                 # the BLAS pool stays as the environment set it
        threadpool_limits = None
    capped, usable, nproc = host_cores()
    w = WORKLOAD
    from sklearn.decomposition import PCA
    Y = np.concatenate([y for c in data.sequences for y in c]).astype(np.float64)
    X = PCA(n_components=w["d"]).fit_transform(Y)
    hp = synthetic.default_hyperparameters(w["D"], w["d"], 0.1)
    hp["y_lambdas_init"] = hp["y_lambdas_init"] * w["y_lambda"]
    N = Y.shape[0]
    m = O.OracleModel(X=X, Y=Y, seq_lengths=[[w["L"]] * w["S"]] * w["C"],
                      y_log_lengthscales=np.log(hp["y_lengthscales_init"]), y_log_lambdas=np.log(hp["y_lambdas_init"]),
                      y_log_sigma_n=np.log(0.1), x_log_lengthscales=np.log(hp["x_lengthscales_init"]),
                      x_log_lambdas=np.log(hp["x_lambdas_init"]), x_log_sigma_n=np.log(0.1),
                      x_log_lin_coeff=np.log(hp["x_lin_coeff_init"])).precompute(
                          "cholesky" if N > 4096 else "inverse")   # N >= 10^4: solves, not the O(N^3) inverse
    T = synthetic.markov_matrix(w["C"])
    Ps = w["P_per_gpu"] if N <= 2000 else 1000
    Ps -= Ps % w["C"]
    z = data.observation_stream(64, seed=1)

    def run(threads):
        rng = np.random.RandomState(0)
        parts = [rng.randint(0, m.X_for_class(c).shape[0], Ps // w["C"]) for c in range(w["C"])]
        s, c = O.init_particles(m, Ps, parts)
        with threadpool_limits(threads) if threadpool_limits else contextlib.nullcontext():
            steps, t0 = 0, time.perf_counter()
            while True:
                r = O.step(m, T, s, c, z[steps % 64], rng.exponential(size=(Ps, w["C"])), rng.randn(Ps, w["d"]),
                           rng.rand(Ps))
                s, c = r.states, r.classes
                steps += 1
                el = time.perf_counter() - t0
                if el > budget_s or steps >= (3 if Ps >= 100_000 else 50):
                    break
        return Ps * steps / el, steps, el

    v, steps, el = run(usable)
    if threadpool_limits is None:       # the pool was not set: report what the environment gave it
        usable = capped or int(torch.get_num_threads())
    rec = {"value": v, "unit": "particle-steps/s", "cores": int(usable), "kind": "port",
           "blas_pool": "threadpoolctl" if threadpool_limits else "not set (threadpoolctl missing): environment default",
           "nproc": nproc, "sched_affinity_cores": usable, "cgroup_cpu_quota": cgroup_cpu_quota(), "torch_threads": int(torch.get_num_threads()),
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "sample": f"oracle (numpy fp64 restatement of gpmdm_pf.py's step, BLAS pool set to all {usable} usable "
                     f"cores: CPU affinity capped by the cgroup CPU quota) N={N} D={w['D']} d={w['d']} C={w['C']}, P={Ps} particles x {steps} frames in "
                     f"{el:.1f} s (model precompute excluded)",
           "calibration": "port vs the unmodified reference on 8 threads of the build container: "
                          "profiles/r03/cpu_calibration.txt, BASELINE.md §2"}
    if capped and capped != usable and threadpool_limits is not None:
        vc, sc, ec = run(capped)
        rec["capped"] = {"value": vc, "cores": capped, "frames": sc, "seconds": ec,
                         "note": "BLAS pool at the environment's OMP_NUM_THREADS cap"}
    return rec


def predictive_stream(pf, model, frames, seed=5):
    """Observations drawn from the filter's own predictive distribution (see the module
    docstring): frame f observes z = mu(x_r) + sqrt(var(x_r)) eps for a uniformly chosen
    particle r of the cloud after frame f - 1.  Returns the stream and the last frame's
    posterior (the timed replay must reproduce it bit for bit)."""
    import torch
    rng = np.random.RandomState(seed)
    zs = np.zeros((frames + 64, model.D))
    ess = []
    for f in range(frames):
        st = pf.export_state()
        x = torch.tensor(st["states"][rng.randint(len(st["states"]))][None, :])
        mu, var = model.map_x_to_y(x)
        zs[f] = mu.numpy()[0] + np.sqrt(np.maximum(var.numpy()[0], 0.0)) * rng.randn(model.D)
        pf.update(zs[f])
        if f >= frames - 10:
            w = pf.export_state()["w"]
            ess.append(float(1.0 / np.sum(w * w)))
    zs[frames:] = zs[:64]
    return zs, {"posterior": pf.class_probabilities().numpy(), "generator_ess_last10_mean": float(np.mean(ess)),
                "note": "z_f = mu(x_r) + sqrt(var(x_r)) eps, r a uniform particle of the cloud after frame "
                        "f-1, from an untimed pass of the same filter (same seed); the timed pass replays "
                        "the stream"}


SPREAD_LAMBDA = 0.05   # observation-GP output scale of the spread-cloud line (see spread_line)


def spread_line(device, steps, warmup=5, y_lambda=SPREAD_LAMBDA, dyn_tiles="auto"):
    """The headline step on a cloud that stays spread out: the same configuration with the
    observation GP's output scales exp(y_log_lambdas) = y_lambda (a less peaked likelihood)
    and the predictive observation stream (predictive_stream), so resampling keeps many
    distinct ancestors and the dynamics GP evaluates tens of thousands of rows per frame.
    Times `steps` frames after `warmup`; per-stage times, ESS and dynamics rows come from the
    same frames (every stage's events on: two event records per stage)."""
    import torch
    from gpmdm_amd import GPMDM_PF, synthetic
    saved = WORKLOAD["y_lambda"]
    WORKLOAD["y_lambda"] = y_lambda
    try:
        model, _ = build_model(device)
    finally:
        WORKLOAD["y_lambda"] = saved
    T = torch.from_numpy(synthetic.markov_matrix(WORKLOAD["C"]))
    P = WORKLOAD["P_per_gpu"]

    def new_filter():
        torch.manual_seed(11)
        return GPMDM_PF(model, T, P, rng="philox", seed=11, dyn_tiles=dyn_tiles)

    zs, check = predictive_stream(new_filter(), model, warmup + steps)
    pf = new_filter()
    for k in range(warmup):
        pf.update(zs[k])
        pf.class_probabilities()
    torch.cuda.synchronize()
    pf.stage_times()
    pf.enable_timing(True)
    ess, rows = [], []
    t0 = time.perf_counter()
    for k in range(steps):
        pf.update(zs[warmup + k])
        pf.get_most_likely_class()
        pf.class_probabilities()
        pf.current_state_mean()
        rows.append(pf.dynamics_rows())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    pf.enable_timing(False)
    st = pf.stage_times()
    w = pf.export_state()["w"]
    ess_last = float(1.0 / np.sum(w * w))
    dyn_ms = st["dyn_gemm"][0] / max(st["dyn_gemm"][1], 1)
    mean_rows = float(np.mean(rows))
    return {"y_lambda": y_lambda, "stream": "predictive", "steps": steps, "ms_per_step": el / steps * 1e3,
            "value": P * steps / el, "ess_frac_last": ess_last / P,
            "generator_ess_last10_mean": check["generator_ess_last10_mean"],
            "replay_matches": bool(np.array_equal(pf.class_probabilities().numpy(), check["posterior"])),
            "dyn_rows_mean": mean_rows, "dyn_rows_frac": mean_rows / P,
            "stages_ms_per_step": {k: v[0] / max(v[1], 1) for k, v in st.items()},
            "dyn_gemm_tflops": dyn_row_flops(model) * mean_rows / max(dyn_ms, 1e-9) / 1e9,
            "note": "same N/D/d/C/P as the headline; exp(y_log_lambdas) = y_lambda and the predictive "
                    "observation stream keep the cloud spread out; timed with every stage's events on "
                    "(ms_per_step includes them)"}


def cutoff_line(model, T, P, zs, warmup, steps, headline_ms=None, headline_obs_ms=None, split=None):
    """The same step with the observation GP's opt-in kernel-value cutoff
    (GPMDM_PF(obs_cutoff=True)): kernel values below the model's tau flushed to
    0 and the unreachable 16-row K-steps skipped.  A timed pass (the roofline kernel's events
    on every 4th frame), then the same frames replayed from the same state, untimed, counting
    the MFMA groups the kernel ran on the event-timed frames against the dense kernel's
    (executed FLOP = groups x 16 x 16 x 16 x 2).  Results equal the
    dense filter's to rounding (tests/test_gpu_obs_cutoff.py); beside the headline, never it."""
    import torch
    from gpmdm_amd import GPMDM_PF, _lib
    t0 = time.perf_counter()
    model.enable_obs_cutoff(True)
    setup_s = time.perf_counter() - t0
    torch.manual_seed(11)
    pf = GPMDM_PF(model, T, P, rng="philox", seed=11, obs_cutoff=True)
    if split is not None:
        pf.set_obs_cutoff(True, split=split)

    def frame(k):
        pf.update(zs[k])
        pf.get_most_likely_class()
        pf.class_probabilities()
        pf.current_state_mean()

    for k in range(warmup):
        frame(k)
    torch.cuda.synchronize()
    pf.stage_times()
    pf.enable_timing(True, stages=("obs_gemm",))
    pf.enable_timing(False)
    lib_, h_ = _lib.load(), pf._h
    snap = pf.export_state()             # (the stats pass replays the timed frames from here)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for k in range(steps):
        if k % 4 == 0:
            lib_.gpmdm_pf_enable_timing(h_, 1)
        frame(warmup + k)
        if k % 4 == 0:
            lib_.gpmdm_pf_enable_timing(h_, 0)
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    pf.enable_timing(False)
    obs_ms, obs_n = pf.stage_times()["obs_gemm"]
    obs_launch_ms = obs_ms / max(obs_n, 1)
    # stats pass: the timed frames again from the same state (Philox: the same clouds), the
    # MFMA groups counted by the kernel on the frames whose launches were timed
    pf.load_state(snap["states"], snap["classes"], ll=snap["ll"], log_w=snap["log_w"], w=snap["w"],
                  resample_idx=snap["resample_idx"], frame=snap.get("frame"))
    pf.obs_cutoff_stats(reset=True)
    n_st = 0
    for k in range(steps):
        if k % 4 == 0:
            _lib.check(lib_.gpmdm_pf_set_obs_cutoff(h_, 2), "stats")
        frame(warmup + k)
        if k % 4 == 0:
            _lib.check(lib_.gpmdm_pf_set_obs_cutoff(h_, 1), "stats")
            n_st += 1
    st = pf.obs_cutoff_stats()
    tau = model.obs_cutoff_tau
    ms = el / steps * 1e3
    groups_per_launch = st["run"] / max(n_st, 1)
    exec_flop = groups_per_launch * 16 * 16 * 16 * 2
    out = {"ms_per_step": ms, "value": P * steps / el, "steps": steps,
           "vs_dense_headline": (headline_ms / ms) if headline_ms else None,
           "obs_launch_ms": obs_launch_ms,
           "obs_speedup_vs_dense": (headline_obs_ms / obs_launch_ms) if headline_obs_ms else None,
           "tau": tau, "mfma_groups_run_fraction": st["fraction_run"],
           "skipped_fraction": (1.0 - st["fraction_run"]) if st["fraction_run"] is not None else None,
           "executed_tflops": exec_flop / (obs_launch_ms * 1e-3) / 1e12,
           "executed_frac_of_peak": exec_flop / (obs_launch_ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS,
           "setup_s": setup_s,
           "note": "GPMDM_PF(obs_cutoff=True): kernel values below tau flushed to 0 (tau bounds the change "
                   "of 1 - k^T K^-1 k below half an ulp, DESIGN.md §3) and the MFMAs of unreachable 16-row "
                   "K-steps skipped; mfma_groups_run_fraction = groups the kernel ran / the dense kernel's, "
                   "counted on the event-timed frames replayed from the same state; executed_tflops = those "
                   "groups x 8192 FLOP / the observation launch time; results equal the dense filter's to "
                   "rounding "
                   "(tests/test_gpu_obs_cutoff.py)"}
    return out


def cutoff_spread_line(model, T, P, zs, spreads=(0.05, 0.2, 0.5), n_anc=2000, reps=4, split=None):
    """The cutoff on clouds that are NOT one ancestor: n_anc distinct training
    latents as ancestors (each with its class), P / n_anc particles around each, offset by
    spread x the observation GP's lengthscale x N(0, 1) per coordinate, contiguous per ancestor
    (a resampled cloud's order).  Per spread: the dense filter and the cutoff filter load the
    same cloud (load_state) and run the same Philox step (same frame: same draws) ``reps``
    times, each from the loaded cloud again; the observation launch is event-timed, then one
    more step from the same cloud counts the cutoff's MFMA groups (gpmdm.py:923-963 either
    way; the cutoff's results equal the dense kernel's to rounding)."""
    import torch
    from gpmdm_amd import GPMDM_PF
    model.enable_obs_cutoff(True)
    X = model.X.detach().cpu().numpy()
    N, d = X.shape
    ell = np.exp(model.y_log_lengthscales.detach().cpu().numpy())
    cls_of = np.concatenate([np.full(model.get_X_for_class(c).shape[0], c) for c in range(model.n_classes)])
    g = np.random.RandomState(23)
    anc = np.sort(g.choice(N, min(n_anc, N), replace=False))
    g.shuffle(anc)                               # ancestors in no spatial order
    owner = anc[(np.arange(P) * anc.size) // P]  # contiguous runs per ancestor
    base = X[owner]
    classes = cls_of[owner].astype(np.int64)
    filt = {cut: GPMDM_PF(model, T, P, rng="philox", seed=11, obs_cutoff=cut) for cut in (False, True)}
    if split is not None:
        filt[True].set_obs_cutoff(True, split=split)
    zero, unif = np.zeros(P), np.full(P, 1.0 / P)   # the reference's initial weights (gpmdm_pf.py:100-104)
    rows = []
    for sp in spreads:
        states = np.ascontiguousarray(base + sp * ell[None, :] * g.randn(P, d))
        r = {"spread_ell": sp, "distinct_ancestors": int(anc.size), "P": P}
        for cut, pf in filt.items():
            pf.stage_times()
            ms = []
            for k in range(reps + 1):
                pf.load_state(states, classes, ll=zero, log_w=zero, w=unif, frame=7)
                torch.cuda.synchronize()
                if k > 0:                        # (the first step is a warm-up)
                    pf.enable_timing(True, stages=("obs_gemm",))
                pf.update(zs[7])
                torch.cuda.synchronize()
                if k > 0:
                    pf.enable_timing(False)
                    t, n = pf.stage_times()["obs_gemm"]
                    ms.append(t / max(n, 1))
            key = "cutoff" if cut else "dense"
            r[f"{key}_obs_launch_ms"] = float(np.median(ms))
            r[f"{key}_obs_launch_ms_all"] = [round(x, 4) for x in ms]
            if not cut:
                w = pf.export_state()["w"]
                r["ess_fraction"] = float(1.0 / np.sum(w * w) / P)
            else:
                pf.load_state(states, classes, ll=zero, log_w=zero, w=unif, frame=7)
                pf.set_obs_cutoff(True, stats=True)
                pf.obs_cutoff_stats(reset=True)
                pf.update(zs[7])
                st = pf.obs_cutoff_stats()
                pf.set_obs_cutoff(True, stats=False)
                r["mfma_groups_run_fraction"] = st["fraction_run"]
                flop = st["run"] * 16 * 16 * 16 * 2
                r["executed_tflops"] = flop / (r["cutoff_obs_launch_ms"] * 1e-3) / 1e12
                r["executed_frac_of_peak"] = r["executed_tflops"] / FP64_MFMA_PEAK_TFLOPS
        r["obs_speedup"] = r["dense_obs_launch_ms"] / r["cutoff_obs_launch_ms"]
        rows.append(r)
        log(f"[bench] cutoff spread {sp}: {json.dumps(r)}")
    return {"rows": rows,
            "note": "clouds of distinct_ancestors training latents (their classes) with P/n particles each, "
                    "offset by spread_ell x l_y x N(0,1); dense and cutoff filters run the same Philox step "
                    "from the same loaded cloud; obs launch = median over the timed repeats (HIP events on the "
                    "launch stream); mfma_groups_run_fraction counted by the cutoff kernel on one more step "
                    "from the same cloud; executed_tflops = groups x 8192 FLOP / the cutoff launch time"}


def nodedup_line(model, T, P_total, group, dist, device, zs, steps, rng, dyn_tiles="auto"):
    """The same step with ancestor de-duplication off (every particle's dynamics GP)."""
    import torch
    from gpmdm_amd import GPMDM_PF
    n_nd = min(steps, 20)
    torch.manual_seed(11)
    pf_nd = GPMDM_PF(model, T, P_total, rng=rng, seed=11 if rng == "philox" else None, process_group=group,
                     dedup=False, dyn_tiles=dyn_tiles)
    for k in range(3):
        pf_nd.update(zs[k])
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t_nd = time.perf_counter()
    for k in range(n_nd):
        pf_nd.update(zs[3 + k])
        pf_nd.get_most_likely_class()
        pf_nd.class_probabilities()
        pf_nd.current_state_mean()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    el_nd = time.perf_counter() - t_nd
    if dist is not None:
        t = torch.tensor([el_nd], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el_nd = float(t.item())
    pf_nd.enable_timing(True)
    for k in range(min(n_nd, 10)):
        pf_nd.update(zs[3 + n_nd + k])
    torch.cuda.synchronize()
    pf_nd.enable_timing(False)
    nd_stages = pf_nd.stage_times()
    P_local = P_total // (dist.get_world_size() if dist is not None else 1)
    return {"ms_per_step": el_nd / n_nd * 1e3, "value": P_total * n_nd / el_nd, "steps": n_nd,
            "stages_ms_per_step": {k: v[0] / max(v[1], 1) for k, v in nd_stages.items()},
            "dyn_gemm_tflops": dyn_row_flops(model) * P_local / max(nd_stages["dyn_gemm"][0] / max(nd_stages["dyn_gemm"][1], 1), 1e-9) / 1e9,
            "note": "dedup=False: the dynamics GP runs on every particle (the reference's work) on "
                    "the wide dynamics tiles; the same filter as the headline's up to summation order; "
                    "dyn_gemm_tflops = algorithmic N_c(N_c+1) + 2 N_c d FLOP per row (class mean) / "
                    "launch time"}


def replay_line(model, T, P, zs, warmup, steps, headline_ms=None):
    """The drop-in default at this size: rng='torch', the reference's draws from torch's
    global generator in its order (gpmdm_pf.py:137-213), drawn on the host as parallel chunks
    of torch's own samplers (replay.ParallelFrameDraws, bit for bit the serial draws) while
    the GPU runs, and uploaded per frame.  Beside the headline, never the headline."""
    import torch
    from gpmdm_amd import GPMDM_PF, replay
    torch.manual_seed(11)
    pf = GPMDM_PF(model, T, P)                 # the reference's signature: rng='torch' by default

    def frame(k):
        pf.update(zs[k])
        pf.get_most_likely_class()
        pf.class_probabilities()
        pf.current_state_mean()

    for k in range(warmup):
        frame(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        frame(warmup + k)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    dr = pf._draws
    # the same frame's draws with torch's serial samplers (what the reference itself does)
    ser = replay.FrameDraws(P, model.n_classes, model.d, P)
    g = torch.Generator().manual_seed(1)
    ser._gen = g
    t1 = time.perf_counter()
    for _ in range(3):
        ser.switch()
        ser.dynamics([P // 2, P - P // 2])
        ser.resample()
    serial_ms = (time.perf_counter() - t1) / 3 * 1e3
    ms = el / steps * 1e3
    return {"rng": "torch (host draws, the reference's order; GPMDM_PF's default)", "steps": steps,
            "ms_per_step": ms, "value": P * steps / el,
            "vs_headline": (headline_ms / ms) if headline_ms else None,
            "draws": type(dr).__name__, "host_threads": getattr(dr, "threads", 1),
            "prefetch_hits": getattr(dr, "prefetch_hits", None), "prefetch_misses": getattr(dr, "prefetch_misses", None),
            "serial_draws_ms_per_frame": serial_ms,
            "note": "update + get_most_likely_class + class_probabilities + current_state_mean per frame; "
                    "serial_draws_ms_per_frame = torch's serial samplers for one frame's E, normals and U on "
                    "this host (the cost the parallel, ahead-of-time draws take off the frame)"}


def bank_line(model, T, F, P, zs, warmup, steps):
    """test_gpmdm_pf.ipynb cell 4's trial loop as one bank: F filters of P particles, each
    frame one bank update plus the read-outs (every filter sees its own observation; here
    the stream shifted by the filter index)."""
    import torch
    from gpmdm_amd import GPMDM_PF_Bank
    bank = GPMDM_PF_Bank(model, T, F, P, seed=11)
    n = len(zs) - F

    def frame(k):
        Z = np.stack([zs[(k + f) % n] for f in range(F)])
        bank.update(Z)
        bank.get_most_likely_class()
        bank.class_probabilities()
        bank.current_state_mean()

    for k in range(warmup):
        frame(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        frame(warmup + k)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"filters": F, "particles_per_filter": P, "frames": steps, "ms_per_frame": el / steps * 1e3,
            "ms_per_filter_frame": el / steps / F * 1e3, "value": F * P * steps / el,
            "unit": "particle-steps/s", "rng": "philox (a bank draws on the device)",
            "note": "one GPMDM_PF_Bank update + get_most_likely_class + class_probabilities + "
                    "current_state_mean per frame for all filters; the notebook runs its 39 trials one "
                    "after another with one filter"}


def library_comm(world, rank, local, group, device):
    """An RCCL communicator made by the library (gpmdm_comm_init), rank 0's unique id
    broadcast over the process group."""
    from gpmdm_amd import _lib
    from gpmdm_amd.distributed import RcclComm, broadcast_array
    uid = bytes(_lib.GPMDM_COMM_ID_BYTES)
    err = None
    if rank == 0:
        try:
            uid = RcclComm.unique_id()
        except Exception as e:  # noqa: BLE001  (the others still get the broadcast: all zeros)
            err = e
    uid = broadcast_array(np.frombuffer(uid, dtype=np.uint8).copy(), group, device).tobytes()
    if err is not None:
        raise err
    if not any(uid):
        raise RuntimeError("rank 0 could not make an RCCL unique id")
    return RcclComm(world, rank, uid, local)


def library_exchange_line(new_filter, zs, steps, dist, device, P_total, warmup=3):
    """Multi-rank runs over RCCL: the same filter with the library's own exchange
    (gpmdm_pf_set_comm, both all-gathers on a library stream) timed for ``steps`` frames,
    then a torch.distributed filter stepped over the same frames; their read-outs and
    exported states must be bitwise equal (the library path and the process-group path
    are one filter)."""
    import torch
    pf = new_filter(exchange="library")
    for k in range(warmup):
        pf.update(zs[k])
        pf.class_probabilities()
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for k in range(steps):
        pf.update(zs[warmup + k])
        pf.get_most_likely_class()
        pf.class_probabilities()
        pf.current_state_mean()
    torch.cuda.synchronize()
    dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    el = float(el.item())
    ref = new_filter(exchange="torch")
    for k in range(warmup + steps):
        ref.update(zs[k])
    a, b = pf.export_state(), ref.export_state()
    same = (np.array_equal(pf.class_probabilities().numpy(), ref.class_probabilities().numpy())
            and np.array_equal(pf.current_state_mean().numpy(), ref.current_state_mean().numpy())
            and all(np.array_equal(a[k], b[k]) for k in ("states", "classes", "ll", "resample_idx")))
    ok = torch.tensor([1 if same else 0], dtype=torch.int64, device=device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    return {"exchange": "gpmdm_pf_set_comm (library-owned RCCL communicator and stream)", "steps": steps,
            "ms_per_step": el / steps * 1e3, "value": P_total * steps / el,
            "bitwise_equal_to_process_group_filter": bool(ok.item()),
            "note": "the headline filter with the library's exchange instead of torch.distributed; read-outs and "
                    "exported states compared bit for bit with a process-group filter after the same frames, on "
                    "every rank"}


def dump_outputs(path, arrays):
    """``--dump-outputs DIR``: each array as DIR/<name>.npy (float64; a few hundred bytes in all)."""
    out = Path(path)
    out.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(out / f"{name}.npy", np.ascontiguousarray(a, dtype=np.float64))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_devices():
    """GPUs this process could use, counted without initialising the GPU runtime
    (torch.cuda.device_count() does not initialise HIP on this image)."""
    import torch
    return torch.cuda.device_count()


def launch(args, argv):
    """``bench.py --gpus N`` without a launcher around it: start N worker processes of this
    script (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment; one process per
    GPU, as torch.distributed.run would), forward rank 0's JSON line and return the exit
    status.  The parent never touches the GPU (it only counts devices) and never execs; a
    worker that fails, or a run past ``--launch-timeout``, ends every worker (by PID) and
    the launch with a non-zero status.

    Fewer visible GPUs than N is an error (exit 2): nothing would be measured on N GPUs.
    ``--rehearse-gloo`` is the explicit opt-in to time-share the visible GPU(s) over the gloo
    backend (RCCL refuses two ranks on one device); ``--plumbing-check`` runs the launcher
    and the distributed timing harness with no GPU work at all (CPU tests)."""
    import subprocess
    N = args.gpus
    if args.plumbing_check:
        backend = "gloo"
    else:
        ndev = visible_devices()
        if ndev < N and not args.rehearse_gloo:
            log(f"[bench] --gpus {N} but {ndev} GPU(s) visible: refusing to report an {N}-GPU number "
                f"(--rehearse-gloo time-shares the visible GPU(s) over gloo, explicitly)")
            return 2
        if ndev == 0:
            log("[bench] no GPU visible")
            return 2
        backend = "gloo" if args.rehearse_gloo else "nccl"
    import tempfile
    import threading
    port = _free_port()
    logdir = Path(os.environ.get("GPMDM_BENCH_LOGDIR") or tempfile.mkdtemp(prefix="gpmdm_bench_"))
    logdir.mkdir(parents=True, exist_ok=True)
    procs, pumps = [], []
    out_chunks = []                     # rank 0's stdout, drained while the workers run

    def pump_stdout(pipe, path):
        # Every rank's stdout is read as it is written (a pipe holds 64 KiB: a rank that
        # writes more -- RCCL's own messages go to stdout -- would block until the launcher
        # read it, i.e. forever).  Rank 0's is kept for its JSON line; every rank's also goes
        # to its own log file.
        with open(path, "wb") as f:
            for chunk in iter(lambda: pipe.read1(65536), b""):
                f.write(chunk)
                if path.name == "rank0.stdout":
                    out_chunks.append(chunk)

    def pump_stderr(pipe, path, r):
        # each rank's stderr to its own file, and forwarded line by line with a rank prefix
        with open(path, "wb") as f:
            for line in iter(pipe.readline, b""):
                f.write(line)
                f.flush()
                try:
                    sys.stderr.write(f"[rank {r}] " + line.decode(errors="replace"))
                    sys.stderr.flush()
                except Exception:   # noqa: BLE001  (a closed parent stderr must not stop the drain)
                    pass

    for r in range(N):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(N), LOCAL_WORLD_SIZE=str(N),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   GPMDM_BENCH_BACKEND=backend, GPMDM_BENCH_LAUNCHER="bench.py")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC (RCCL between processes)
        p = subprocess.Popen([sys.executable, "-u", str(Path(__file__).resolve()), *argv], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        procs.append(p)
        for target, a in ((pump_stdout, (p.stdout, logdir / f"rank{r}.stdout")),
                          (pump_stderr, (p.stderr, logdir / f"rank{r}.stderr", r))):
            t = threading.Thread(target=target, args=a, daemon=True)
            t.start()
            pumps.append(t)
    log(f"[bench] {N} workers, per-rank logs in {logdir}")
    t0 = time.time()
    rc = 0
    failed = []
    try:
        live = set(range(N))
        while live:
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0:
                    failed.append(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 128 - code
                    log(f"[bench] worker rank {r} exited with status {code}: stopping the launch")
            if rc:
                break
            if time.time() - t0 > args.launch_timeout:
                log(f"[bench] launch exceeded {args.launch_timeout} s: stopping the workers")
                rc = 124
                failed.extend(r for r in range(N) if procs[r].poll() is None)
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            try:
                p.wait(timeout=30)
            except Exception:
                pass
        for t in pumps:                 # the pipes close with their processes
            t.join(timeout=30)
    if rc != 0:
        for r in sorted(set(failed)):
            path = logdir / f"rank{r}.stderr"
            try:
                tail = path.read_bytes()[-4000:].decode(errors="replace")
            except OSError:
                tail = "(no log)"
            log(f"[bench] ---- rank {r} stderr tail ({path}) ----\n{tail}")
    if rc == 0:
        out = b"".join(out_chunks)
        lines = [ln for ln in out.decode(errors="replace").splitlines() if ln.startswith("{")]
        if len(lines) != 1:
            log(f"[bench] rank 0 printed {len(lines)} JSON lines, expected 1")
            return 1
        print(lines[0], flush=True)
    return rc


def plumbing_worker(args):
    """The distributed timing harness with no GPU work (``--plumbing-check``): process
    group over gloo, barrier-bracketed timed region of K tiny CPU steps, max over ranks,
    one JSON line from rank 0 -- the launcher's and the harness's plumbing, testable on a
    machine without a GPU."""
    import datetime
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=args.collective_timeout))
    if os.environ.get("GPMDM_PLUMBING_FAIL_RANK") == str(rank):   # tests: a worker that dies mid-run
        os._exit(3)
    # tests: a worker that writes more than a pipe buffer to stdout / stderr before its line
    # (RCCL's debug and warning output goes to stdout)
    spam = int(os.environ.get("GPMDM_PLUMBING_SPAM_BYTES", "0"))
    if spam:
        row = f"NCCL INFO rank {rank}: " + "x" * 100 + "\n"
        for _ in range(spam // len(row) + 1):
            sys.stdout.write(row)
            sys.stderr.write(row)
        sys.stdout.flush()
        sys.stderr.flush()
    try:
        x = np.arange(4096, dtype=np.float64)
        for _ in range(args.warmup):
            x = np.sqrt(x * x + 1.0)
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            x = np.sqrt(x * x + 1.0)
        dist.barrier()
        el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": None, "unit": "particle-steps/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": float(el.item()) / max(args.steps, 1) * 1e3,
                              "world_size_backend": dist.get_world_size(), "backend": dist.get_backend(),
                              "launcher": os.environ.get("GPMDM_BENCH_LAUNCHER", "external"),
                              "data": "none: --plumbing-check (launcher and timing harness only, no GPU work)"}),
                  flush=True)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="GPUs (one worker process each).  Without WORLD_SIZE in the environment and N > 1, "
                         "bench.py starts the N workers itself; under torch.distributed.run it must equal WORLD_SIZE")
    ap.add_argument("--rehearse-gloo", action="store_true",
                    help="explicit opt-in: run N ranks over gloo on fewer GPUs than N (time-shared; a rehearsal "
                         "of the multi-rank path, not an N-GPU measurement)")
    ap.add_argument("--plumbing-check", action="store_true",
                    help="launcher + distributed timing harness only, no GPU work (CPU tests)")
    ap.add_argument("--launch-timeout", type=float, default=3000.0,
                    help="seconds before the self-launch stops its workers")
    ap.add_argument("--collective-timeout", type=float, default=600.0,
                    help="seconds a collective may stall before its worker fails")
    ap.add_argument("--exchange", default="torch", choices=("torch", "library"),
                    help="multi-rank exchange: torch.distributed (process_group=) or the library's own RCCL "
                         "communicator (gpmdm_pf_set_comm)")
    ap.add_argument("--replay-steps", type=int, default=None,
                    help="frames of the rng='torch' (drop-in default) line beside a Philox headline "
                         "(default 30 at config 2 on one GPU, 0 = off)")
    ap.add_argument("--library-steps", type=int, default=20,
                    help="multi-rank RCCL runs: frames of the library-exchange line (0 = off)")
    ap.add_argument("--steps", type=int, default=None,
                    help="timed frames (default: 500, configs[1]'s 500 frames; 20 for configs 3 and 5)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other measurement and check (stage breakdown, "
                         "nodedup, replay, bank, spread, cutoff, library exchange, CPU baseline); without it "
                         "the run sets up, warms up, times --steps frames and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the read-outs of the last timed step (what the caller of the step receives) "
                         "as DIR/<name>.npy, float64")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--config", type=int, default=2, choices=(1, 2, 3, 4, 5))
    ap.add_argument("--rng", default="auto", choices=("auto", "philox", "torch"),
                    help="auto: 'torch' (the drop-in default, host draws) for config 1, else 'philox'")
    ap.add_argument("--stream", default="mocap", choices=("mocap", "predictive"))
    ap.add_argument("--y-lambda", type=float, default=1.0)
    ap.add_argument("--bank", type=int, default=None,
                    help="filters of the bank line (config 1: 39, the notebook's test trials)")
    ap.add_argument("--no-nodedup", action="store_true")
    ap.add_argument("--spread-lambda", type=float, default=SPREAD_LAMBDA,
                    help="observation-GP output scale of the spread line (configurations with more "
                         "observation dimensions need a smaller one to keep the cloud spread)")
    ap.add_argument("--spread-steps", type=int, default=None,
                    help="frames of the spread-cloud line (config 2, one GPU; default 30, 0 = off)")
    ap.add_argument("--cutoff-steps", type=int, default=None,
                    help="frames of the observation-GP cutoff line (obs_cutoff=True; configs 2, 3, 5 on one GPU: "
                         "default 20, 0 = off)")
    ap.add_argument("--cutoff-spread", action="store_true",
                    help="only the cutoff-vs-dense observation launch on spread clouds of >= 1000 ancestors "
                         "(cutoff_spread_line; one GPU), one JSON line with its rows; not a headline run")
    ap.add_argument("--cutoff-spread-at", type=float, nargs="+", default=[0.05, 0.2, 0.5],
                    help="the spreads (x the observation lengthscale) of --cutoff-spread")
    ap.add_argument("--cutoff-split", default=None, choices=("auto", "none", "all", "tail", "chunks"),
                    help="the cutoff filters' tile scheduling (gpmdm_pf_set_obs_cutoff_split; default auto)")
    ap.add_argument("--cutoff-spread-reps", type=int, default=4,
                    help="timed launches per spread and kernel of --cutoff-spread (after one warm-up)")
    ap.add_argument("--dyn-tiles", default="auto", choices=("auto", "narrow", "wide"),
                    help="dynamics tile shape of the headline filter (gpmdm_pf_set_dyn_tiles)")
    argv = sys.argv[1:]
    args = ap.parse_args(argv)
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch(args, argv))
    if env_world is not None and int(env_world) != args.gpus:
        log(f"[bench] --gpus {args.gpus} but WORLD_SIZE={env_world}: the launcher and the flag disagree")
        sys.exit(2)
    if args.plumbing_check:
        plumbing_worker(args)
        return
    global WORKLOAD
    WORKLOAD = workload(args.config)
    WORKLOAD["y_lambda"] = args.y_lambda
    if args.steps is None:
        args.steps = 20 if args.config in (3, 5) else (200 if args.config == 1 else 500)
    rng = args.rng if args.rng != "auto" else ("torch" if args.config == 1 else "philox")
    if args.bank is None:
        args.bank = 39 if args.config == 1 else 0

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    backend = os.environ.get("GPMDM_BENCH_BACKEND", "nccl")
    if world > ndev:
        if backend != "gloo":
            log(f"[bench] WORLD_SIZE={world} but {ndev} GPU(s) visible: refusing to time-share GPUs over "
                f"{backend} (GPMDM_BENCH_BACKEND=gloo / --rehearse-gloo is the explicit rehearsal)")
            sys.exit(2)
        local %= max(ndev, 1)           # rehearsal: ranks time-share the visible GPU(s)
    dist = None
    group = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        torch.cuda.set_device(local)
        tmo = datetime.timedelta(seconds=args.collective_timeout)   # a stalled collective fails the worker
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local), timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)
        group = dist.group.WORLD
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)

    from gpmdm_amd import GPMDM_PF, build
    from gpmdm_amd import _lib
    # one builder per node (a no-op when the in-tree library is current); the other ranks
    # wait, so concurrent ranks never write the same objects
    if int(os.environ.get("LOCAL_RANK", "0")) == 0:
        build.build()
    if dist is not None:
        dist.barrier()
    _lib.load()
    t_setup = time.perf_counter()
    model, data = build_model(device)
    P_total = WORKLOAD["P_per_gpu"] * world
    from gpmdm_amd import synthetic
    T = torch.from_numpy(synthetic.markov_matrix(WORKLOAD["C"]))
    full = args.full
    n_breakdown = min(args.steps, 10) if full else 0
    n_frames = args.warmup + args.steps + n_breakdown + 64
    if args.config == 1 and full:
        n_frames += args.steps          # the event-free pass of the notebook line
    comm = None
    if world > 1 and args.exchange == "library":
        if backend != "nccl":
            log("[bench] --exchange library needs RCCL (one GPU per rank), not a gloo rehearsal")
            sys.exit(2)
        comm = library_comm(world, rank, local, group, device)

    def new_filter(exchange=args.exchange, **kw):
        torch.manual_seed(11)
        seed = 11 if rng == "philox" else None
        if world > 1 and exchange == "library":
            # the library's own exchange: shard=(world, rank) + gpmdm_pf_set_comm
            pf_ = GPMDM_PF(model, T, P_total, rng=rng, seed=seed, shard=(world, rank), dyn_tiles=args.dyn_tiles, **kw)
            pf_.set_comm(comm)
            return pf_
        return GPMDM_PF(model, T, P_total, rng=rng, seed=seed, process_group=group, dyn_tiles=args.dyn_tiles, **kw)

    stream_check = None
    if args.stream == "predictive":
        zs, stream_check = predictive_stream(new_filter(), model, args.warmup + args.steps + n_breakdown)
    else:
        zs = data.observation_stream(n_frames, seed=1)
    if args.cutoff_spread:
        if world > 1:
            log("[bench] --cutoff-spread runs on one GPU")
            sys.exit(2)
        res = cutoff_spread_line(model, T, P_total, zs, spreads=tuple(args.cutoff_spread_at),
                                 reps=args.cutoff_spread_reps, split=args.cutoff_split)
        print(json.dumps({"metric": "observation launch ms, dense vs cutoff, spread clouds",
                          "config": {"workload": f"configs[{WORKLOAD['cfg'] - 1}]", "N": int(model.X.shape[0]),
                                     "D": WORKLOAD["D"], "d": WORKLOAD["d"], "C": WORKLOAD["C"], "P": P_total},
                          "cutoff_spread": res}), flush=True)
        return
    pf = new_filter()
    log(f"[bench] rank {rank}/{world} setup {time.perf_counter() - t_setup:.1f}s, P_total={P_total}")

    def one(k):
        pf.update(zs[k])
        pf.get_most_likely_class()
        pf.class_probabilities()
        pf.current_state_mean()

    for k in range(args.warmup):
        one(k)
    torch.cuda.synchronize()
    pf.stage_times()                # drop warm-up records
    # The roofline kernel's launches are timed live with HIP events (two per timed launch)
    # on every `sample`-th frame of the timed region: each record is a host API call on the
    # frame's critical path (~11 us; measured at the notebook's 0.13 ms frames) and idles the
    # GPU between the kernels around it (a sampled headline frame runs ~40 us longer:
    # profiles/r04/events_ab/), so the sample keeps that cost out of ms_per_step while the
    # average launch time still comes from launches inside the timed loop (>= 31 of 500 at
    # configs 2 / 4; configs 3 / 5 time 20 frames of 0.15-0.8 s launches, every 4th).
    sample = {1: 8, 3: 4, 5: 4}.get(args.config, 16)
    pf.enable_timing(True, stages=("obs_gemm",))   # the roofline kernel only
    pf.enable_timing(False)
    lib_, h_ = _lib.load(), pf._h
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        if k % sample == 0:
            lib_.gpmdm_pf_enable_timing(h_, 1)
        one(args.warmup + k)
        if k % sample == 0:
            lib_.gpmdm_pf_enable_timing(h_, 0)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    pf.enable_timing(False)
    stages = pf.stage_times()
    # what the caller of the timed step received in its last frame (the read-outs are cached
    # on the host by the step's own calls: nothing runs on the GPU here)
    outputs = {"most_likely_class": np.array([pf.get_most_likely_class()], dtype=np.float64),
               "class_probabilities": pf.class_probabilities().numpy().astype(np.float64),
               "current_state_mean": pf.current_state_mean().numpy().astype(np.float64)}
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outputs)
    # per-stage breakdown from a separate, untimed pass (every stage's events on)
    bd_rows = 0
    breakdown = None
    if full:
        pf.enable_timing(True)
        for k in range(n_breakdown):            # the stream's next frames (no jump back in time)
            one(args.warmup + args.steps + k)
            bd_rows += pf.dynamics_rows()       # rows the dynamics GP evaluated this frame
        torch.cuda.synchronize()
        pf.enable_timing(False)
        breakdown = pf.stage_times()
    untimed_ms = None
    if full and args.config == 1 and world == 1:
        # the same loop once more without the roofline's two timing events per frame (at
        # 0.1 ms per frame their records are a visible part of the frame)
        k0 = args.warmup + args.steps + n_breakdown
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for k in range(args.steps):
            one(k0 + k)
        torch.cuda.synchronize()
        untimed_ms = (time.perf_counter() - t1) / args.steps * 1e3
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    post = pf.class_probabilities().numpy()
    if stream_check is not None:     # the timed filter followed the stream's own trajectory
        stream_check["replay_matches"] = bool(np.array_equal(post, stream_check.pop("posterior")))
    dyn_rows = ess = None
    if full:
        dyn_rows = pf.dynamics_rows()
        w_last = pf.export_state()["w"]
        ess = float(1.0 / np.sum(w_last * w_last))
    bank = (bank_line(model, T, args.bank, P_total, zs, args.warmup, args.steps)
            if full and args.bank and world == 1 else None)
    nodedup = None if (args.no_nodedup or not full) else nodedup_line(model, T, P_total, group, dist, device, zs, args.steps, rng,
                                                                args.dyn_tiles)
    rep = None
    if args.replay_steps is None:
        args.replay_steps = 30 if (args.config == 2 and rng == "philox" and args.stream == "mocap") else 0
    if full and args.replay_steps and world == 1:
        rep = replay_line(model, T, P_total, zs, 3, args.replay_steps, elapsed / args.steps * 1e3)
    libx = None
    if full and world > 1 and backend == "nccl" and args.library_steps > 0:
        if comm is None:
            try:
                comm = library_comm(world, rank, local, group, device)
            except Exception as e:  # noqa: BLE001
                libx = {"exchange": "gpmdm_pf_set_comm", "error": repr(e)[:400]}
        # every rank must hold a communicator before any enters the library's collectives (a
        # rank that failed alone would leave the others waiting in RCCL, which has no timeout)
        ok = torch.tensor([1 if comm is not None else 0], dtype=torch.int32, device=device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
        if int(ok.item()) == 0 and comm is not None:
            libx = {"exchange": "gpmdm_pf_set_comm", "error": "another rank could not make its communicator"}
            comm = None
        if comm is not None:
            try:    # an error here is reported in the line, not in place of the headline
                libx = library_exchange_line(new_filter, zs, min(args.steps, args.library_steps), dist, device,
                                             P_total)
            except Exception as e:  # noqa: BLE001
                libx = {"exchange": "gpmdm_pf_set_comm", "error": repr(e)[:400]}
    if args.spread_steps is None:
        args.spread_steps = 30 if (args.config == 2 and args.stream == "mocap" and args.y_lambda == 1.0) else 0
    spread = (spread_line(device, args.spread_steps, y_lambda=args.spread_lambda, dyn_tiles=args.dyn_tiles)
              if full and args.spread_steps and world == 1 else None)
    N, D, d = model.X.shape[0], model.D, model.d
    P_local = P_total // world
    alg, dense, executed = obs_kernel_flops(N, D)
    obs_ms, obs_n = stages["obs_gemm"]
    obs_launch_s = obs_ms / max(obs_n, 1) / 1e3
    if args.cutoff_steps is None:
        args.cutoff_steps = 20 if (args.config in (2, 3, 5) and rng == "philox" and args.stream == "mocap") else 0
    cut = None
    if full and args.cutoff_steps and world == 1 and len(zs) >= args.warmup + args.cutoff_steps + 10:
        try:   # reported beside the headline, never in place of it
            cut = cutoff_line(model, T, P_total, zs, args.warmup, args.cutoff_steps, elapsed / args.steps * 1e3,
                              obs_launch_s * 1e3, split=args.cutoff_split)
        except Exception as e:  # noqa: BLE001
            cut = {"error": repr(e)[:400]}
    achieved = alg * P_local / obs_launch_s / 1e12
    traffic, traffic_src = pmc_traffic(WORKLOAD["cfg"])
    b_image = obs_model_bytes(N, D)
    rec = {
        "metric": METRIC,
        "value": P_total * args.steps / elapsed,
        "unit": "particle-steps/s",
        "n_gpus": world,
        "world_size_backend": dist.get_world_size() if dist is not None else 1,
        "backend": backend if dist is not None else None,
        "launcher": os.environ.get("GPMDM_BENCH_LAUNCHER",
                                   "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ
                                   else ("external" if world > 1 else "single process")),
        "exchange": ("none (one rank)" if world == 1 else
                     "gpmdm_pf_set_comm (library RCCL communicator)" if args.exchange == "library" else
                     f"torch.distributed ({backend}) all-gathers over the process group"),
        "rehearsal": bool(world > ndev),
        "steps": args.steps,
        "warmup": args.warmup,
        "full": full,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "published_reference": {"value": PUBLISHED_PARTICLE_STEPS, "unit": "particle-steps/s",
                                "basis": PUBLISHED_BASIS},
        "dtype": "f64",
        "data": "synthetic (SURVEY §8(d) generator; random-phase sinusoid mocap surrogate, PCA latents)",
        "config": {"workload": f"configs[{WORKLOAD['cfg'] - 1}]: N={N} D={D} d={d} C={model.n_classes}, "
                               f"P={P_local} particles per GPU, "
                               f"{'philox (device) draws' if rng == 'philox' else 'torch (host) draws'}, "
                               f"multinomial resampling"
                               + (f", predictive observation stream" if args.stream == "predictive" else "")
                               + (f", y_lambda={args.y_lambda}" if args.y_lambda != 1.0 else ""),
                   "rng": rng, "stream": args.stream, "y_lambda": args.y_lambda,
                   "N": N, "D": D, "d": d, "C": model.n_classes, "P_per_gpu": P_local, "P_total": P_total,
                   "frames": args.warmup + args.steps,
                   "parallelism": f"particles sharded over {world} GPU(s), one all-gather per step"},
        "roofline": {"bound": "mfma", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": achieved / FP64_MFMA_PEAK_TFLOPS,
                     "traffic": traffic,
                     "traffic_GBps": traffic / obs_launch_s / 1e9 if traffic else None,
                     "traffic_source": traffic_src,
                     "traffic_note": ("HBM/MALL bytes per launch; the algorithmic bytes are triu(R) and K^-1 Y "
                                      f"({b_image / 1e6:.1f} MB) plus the particles; each XCD re-streams B panels "
                                      "once per round of concurrently resident tiles, which costs nothing "
                                      "measurable: the kernel is FP64-MFMA bound at a few % of HBM "
                                      "bandwidth (DESIGN.md §3)") if traffic else None,
                     "kernel": f"k_gp_tile<{d},false> (observation GP)",
                     "flops_per_particle_algorithmic": alg, "flops_per_particle_executed": executed,
                     "flops_per_particle_dense_form": dense,
                     "executed_tflops": executed * P_local / obs_launch_s / 1e12,
                     "dense_form_equivalent_tflops": dense * P_local / obs_launch_s / 1e12,
                     "launch_ms": obs_launch_s * 1e3,
                     "timed_launches": obs_n, "events_every_nth_frame": sample},
        "stream_check": stream_check,
        "posterior_last": [float(x) for x in post],
    }
    if args.dump_outputs:
        rec["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": {k: list(v.shape) for k, v in outputs.items()}}
    if full:
        rec.update({
            "stages_ms_per_step": {k: v[0] / max(v[1], 1) for k, v in breakdown.items()},
            "nodedup": nodedup,
            "ess_last": ess,
            "ess_frac_last": ess / P_total,
            "dyn_rows_last": {"evaluated": dyn_rows, "particles": P_local,
                              "breakdown_mean": bd_rows / max(n_breakdown, 1),
                              "dyn_gemm_tflops": dyn_row_flops(model) * bd_rows
                              / max(breakdown["dyn_gemm"][0], 1e-9) / 1e9,
                              "note": "dynamics GP rows: one per distinct (ancestor, class) key (bitwise-"
                                      "identical ancestor de-duplication, DESIGN.md §3); breakdown_mean and "
                                      "dyn_gemm_tflops over the stage-breakdown pass"}})
    if libx is not None:
        rec["library_exchange"] = libx
    if rep is not None:
        rec["replay"] = rep
    if bank is not None:
        rec["bank"] = bank
    if spread is not None:
        rec["spread"] = spread
    if cut is not None:
        rec["cutoff"] = cut
    if args.config == 1:
        ms = elapsed / args.steps * 1e3
        rec["ms_per_frame"] = ms
        rec["reference_ms_per_frame"] = {
            "published": 78.2, "published_source": "test_gpmdm_pf.ipynb:259-260 (12.78 FPS, author's laptop CPU)",
            "container": 16.3, "container_source": "BASELINE.md §2 (unmodified reference, 8 cores, N=500, P=100)",
            "speedup_vs_published": 78.2 / ms, "speedup_vs_container": 16.3 / ms}
        if full:
            rec["ms_per_frame_without_timing_events"] = {
                "value": untimed_ms, "note": "the next frames of the stream, same loop, no stage events "
                                             "(ms_per_step keeps the roofline kernel's two events per frame)"}
    if full and rank == 0 and not args.no_cpu_baseline:
        # after every timed pass (the other ranks wait at the barrier below); at N > 1 the
        # same per-GPU workload, so the N-GPU line carries the CPU baseline beside its value
        try:
            rec["cpu_baseline"] = cpu_baseline(data)
            if world > 1:
                rec["cpu_baseline"]["note"] = (f"rank 0's host, after the {world}-rank timed passes; the CPU "
                                               f"sample is one GPU's share (P={P_local})")
        except Exception as e:  # the baseline is reported, never the target
            log(f"[bench] cpu baseline failed: {e!r}")
            rec["cpu_baseline"] = None
    if dist is not None:
        dist.barrier()
    if rank == 0:
        print(json.dumps(rec), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
