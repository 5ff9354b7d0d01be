// C ABI, backward simulation (gpmdm_backward_sample_step, gpmdm_pf_sample_trajectories): one
// implementation of the step (the sources' records by the backward step's bs_records; then, per
// chunk of targets, their grouping, the range sums, the pick and the select, all queued on the
// caller's stream), applied to the caller's arrays by the first entry point and lag after lag to
// the slots of the ancestry ring (capi_smooth.hip) by the second, which ends with one copy-out and
// one wait -- and, when the pose is asked for, the read-outs over the alive states of each lag
// behind a second one (their sizes are the alive counts).  Kernels: backsample.h.
#include "capi_internal.h"
#include "backsample.h"

static_assert(gpmdm::kFsRange == GPMDM_BACKSAMPLE_RANGE, "the header exports the kernels' range length");

namespace gpmdm::capi {

constexpr long long kFsMaxPairs = 1ll << 36;
constexpr size_t kFsPartBytes = (size_t)64 << 20;   // the ranges' partial sums of one chunk of targets

// Targets per chunk: a target's result does not depend on the others, so the call's targets go
// through in chunks whose partial sums stay near kFsPartBytes (whole blocks; at least one).
static long long fs_chunk(long long n_s, long long n_t) {
  long long c = (long long)(kFsPartBytes / (2 * sizeof(double))) / fs_ranges(n_s) / kBsB * kBsB;
  if (c < kBsB) c = kBsB;
  return c < n_t ? c : n_t;
}
static size_t fs_part_bytes(long long n_s, long long n_t) {
  return 2 * sizeof(double) * (size_t)fs_ranges(n_s) * (size_t)fs_chunk(n_s, n_t);
}

static int fs_check(const gpmdm_model* m, long long n_s, long long n_t) {
  TRY(bs_check(m, n_s, n_t));
  CHECK(fs_ranges(n_s) <= 65535, "backward sample step: more than 65535 source ranges");
  return GPMDM_OK;
}

// The targets' part of one step on device arrays, queued on s: the records of the n_s sources are
// in sc.rec (bs_records).  idx: n_t source rows (-1: none); log_den: nullptr if not wanted.
static int fs_targets(const gpmdm_model* m, FsScratch& sc, long long n_s, long long n_t, const double* Xt,
                      const int* ct, const double* u, int* idx, double* log_den, hipStream_t s) {
  const int C = m->C, d = m->d;
  const long long chunk = fs_chunk(n_s, n_t);
  const int nr = (int)fs_ranges(n_s);
  TRY(sc.perm.grow((size_t)chunk, s));
  TRY(sc.tab.grow((size_t)2 * kMaxClasses + 2, s));
  TRY(sc.part.grow((size_t)2 * nr * chunk, s));
  TRY(sc.range.grow((size_t)chunk, s));
  TRY(sc.res.grow((size_t)chunk, s));
  TRY(sc.scale.grow((size_t)chunk, s));
  for (long long j0 = 0; j0 < n_t; j0 += chunk) {
    const long long nc = std::min(chunk, n_t - j0);
    BsGroupArgs ga{};
    ga.n = nc;
    ga.C = C;
    ga.cls = ct + j0;
    ga.perm = sc.perm;
    ga.tab = sc.tab;
    launch_bs_group(ga, s);
    FsPassArgs pa{};
    pa.n_s = n_s;
    pa.n_t = nc;
    pa.C = C;
    pa.d = d;
    pa.n_ranges = nr;
    pa.rec = sc.rec;
    pa.Xt = Xt + j0 * d;
    pa.perm = sc.perm;
    pa.tab = sc.tab;
    pa.part = sc.part;
    pa.range = sc.range;
    pa.res = sc.res;
    pa.scale = sc.scale;
    pa.u = u + j0;
    pa.idx = idx + j0;
    pa.log_den = log_den ? log_den + j0 : nullptr;
    launch_fs_sum(pa, s);
    launch_fs_pick(pa, s);
    launch_fs_select(pa, s);
  }
  HIPCHK(hipGetLastError());
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_backward_sample_step(gpmdm_model_t m, const double* T, int64_t n_s, const double* Xs, const int64_t* cs,
                               const double* a, int64_t n_t, const double* Xt, const int64_t* ct, const double* u,
                               int64_t* idx_out, double* log_den_out, void* stream) {
  CHECK(m, "null model");
  CHECK(T && Xs && cs && Xt && ct && u, "null argument");
  TRY(fs_check(m, n_s, n_t));
  const int C = m->C, d = m->d;
  std::vector<int> cs32, ct32, idx32;
  TRY(bs_to_classes(cs, n_s, C, cs32, "sources"));
  TRY(bs_to_classes(ct, n_t, C, ct32, "targets"));
  for (int64_t j = 0; j < n_t; ++j) CHECK(u[j] >= 0.0 && u[j] < 1.0, "backward sample step: a uniform is outside [0, 1)");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  // the call's own buffers and scratch, released when it has waited for its launches
  FsScratch sc;
  DevBuf<double> dT, dXs, dXt, da, du, dld;
  DevBuf<int> dcs, dct, didx;
  TRY(dT.alloc((size_t)C * C));
  TRY(dXs.alloc((size_t)n_s * d));
  TRY(dXt.alloc((size_t)n_t * d));
  TRY(du.alloc((size_t)n_t));
  TRY(dld.alloc((size_t)n_t));
  TRY(didx.alloc((size_t)n_t));
  TRY(dcs.alloc((size_t)n_s));
  TRY(dct.alloc((size_t)n_t));
  if (a) TRY(da.alloc((size_t)n_s));
  if (idx_out) idx32.resize((size_t)n_t);
  auto launches = [&]() -> int {
    HIPCHK(hipMemcpyAsync(dT, T, sizeof(double) * C * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dXs, Xs, sizeof(double) * n_s * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dXt, Xt, sizeof(double) * n_t * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(du, u, sizeof(double) * n_t, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcs, cs32.data(), sizeof(int) * n_s, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dct, ct32.data(), sizeof(int) * n_t, hipMemcpyHostToDevice, s));
    if (a) HIPCHK(hipMemcpyAsync(da, a, sizeof(double) * n_s, hipMemcpyHostToDevice, s));
    TRY(bs_records(m, sc.rec, sc.mu, sc.var, sc.q, dT, n_s, dXs, dcs, da, s));
    TRY(fs_targets(m, sc, n_s, n_t, dXt, dct, du, didx, dld, s));
    if (idx_out) HIPCHK(hipMemcpyAsync(idx32.data(), didx, sizeof(int) * n_t, hipMemcpyDeviceToHost, s));
    if (log_den_out) HIPCHK(hipMemcpyAsync(log_den_out, dld, sizeof(double) * n_t, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  const int rc = launches();
  const hipError_t waited = hipStreamSynchronize(s);   // (also after a failure: the buffers go with the call)
  TRY(rc);
  HIPCHK(waited);
  HIPCHK(m->note_use(s));
  for (size_t j = 0; j < idx32.size(); ++j) idx_out[j] = idx32[j];
  return GPMDM_OK;
}

int gpmdm_pf_sample_trajectories(gpmdm_pf_t pf, int64_t n, int lag, const uint64_t* seed, const gpmdm_sample_out* out,
                                 void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "trajectory sampling serves single filters, not banks");
  CHECK(pf->n_ranks == 1, "trajectory sampling serves filters on one rank");
  CHECK(pf->sm_L > 0, "smoothing is off (gpmdm_pf_set_smoothing)");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the sampler's)
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "sample_trajectories between switch and resample");
  gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d, D = m->D;
  const long long P = pf->P;
  CHECK(n >= 1 && n < (1ll << 31), "n must be in [1, 2^31)");
  CHECK(n <= kFsMaxPairs / P, "more than 2^36 trajectory-particle pairs per step (n x P)");
  CHECK(lag >= 1 && lag <= pf->sm_depth, "lag must be in [1, the recorded depth] (gpmdm_pf_smoothing_depth)");
  TRY(fs_check(m, P, n));
  static const gpmdm_sample_out none{};
  const gpmdm_sample_out& o = out ? *out : none;
  const bool obs = o.obs_mean || o.obs_spread;
  const int L1 = lag + 1;
  const int W = 2 + C + 2 * d;   // {alive, distinct, counts[C], sum hi[d], sum lo[d]}
  // the uniforms and the rows {index, class, state} of every lag, the records, one chunk's sums
  const size_t rows = (size_t)L1 * (size_t)n;
  CHECK(rows <= kSmoothBytes / (sizeof(double) * (d + 1) + 2 * sizeof(int)) &&
            rows * (sizeof(double) * (d + 1) + 2 * sizeof(int)) + bs_record_bytes(C, d, P) + fs_part_bytes(P, n) <=
                kSmoothBytes,
        "this window needs more than 1 GiB of device staging (rows of n uniforms, indices, classes and states per "
        "lag): ask for fewer trajectories or a shorter window");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  FsScratch& sc = pf->fs;
  const size_t n_out = (size_t)L1 * W + (size_t)L1 * 2 * D;   // the rows, then {mean[D], spread[D]} of every lag
  TRY(pf->fs_out.reserve(n_out, s));
  TRY(sc.u.grow(rows, s));
  TRY(sc.X.grow(rows * d, s));
  TRY(sc.idx.grow(rows, s));
  TRY(sc.cls.grow(rows, s));
  TRY(sc.mark.grow((size_t)P, s));
  if (obs) TRY(sc.ro_part.grow(readout_part_doubles(n, D, 1), s));
  const unsigned long long sd = seed ? *seed : (((unsigned long long)pf->seed_hi << 32) | pf->seed_lo);
  const int ns = pf->sm_L + 1;
  auto slot_of = [&](int l) { return (size_t)((pf->sm_slot() - l % ns + ns) % ns) * (size_t)P; };
  std::vector<int> i32, c32;
  auto launches = [&]() -> int {
    // the record of the latest frame, if it ran on another stream
    if (pf->sm_pending && pf->sm_stream != s) HIPCHK(pf->sm_ev.block(s));
    HIPCHK(hipMemsetAsync(sc.mark, 0, sizeof(int) * (size_t)P, s));
    FsDrawArgs da{};
    da.n = n;
    da.P = P;
    da.lag = lag;
    da.frame = pf->frame;
    da.seed_lo = (unsigned)(sd & 0xffffffffu);
    da.seed_hi = (unsigned)(sd >> 32);
    da.u = sc.u;
    da.idx0 = sc.idx;
    launch_fs_draw(da, s);
    for (int l = 0; l <= lag; ++l) {
      const size_t k = slot_of(l), r = (size_t)l * n;
      FsGatherArgs ga{};
      ga.n = n;
      ga.d = d;
      ga.idx = sc.idx + r;
      ga.X = pf->sm_X + k * d;
      ga.cls = pf->sm_cls + k;
      ga.X_out = sc.X + r * d;
      ga.cls_out = sc.cls + r;
      launch_fs_gather(ga, s);
      FsReduceArgs ra{};
      ra.n = n;
      ra.C = C;
      ra.d = d;
      ra.idx = sc.idx + r;
      ra.cls = sc.cls + r;
      ra.X = sc.X + r * d;
      ra.mark = sc.mark;
      ra.out = pf->fs_out.dev + (size_t)l * W;
      launch_fs_reduce(ra, s);
      if (l < lag) {   // j_{l+1}: the slot clouds are post-resample, every a_k = 1 / P
        const size_t ks = slot_of(l + 1);
        TRY(bs_records(m, sc.rec, sc.mu, sc.var, sc.q, pf->T, P, pf->sm_X + ks * d, pf->sm_cls + ks, nullptr, s));
        TRY(fs_targets(m, sc, P, n, sc.X + r * d, sc.cls + r, sc.u + r + n, sc.idx + r + n, nullptr, s));
      }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->fs_out.pin, pf->fs_out.dev, sizeof(double) * L1 * W, hipMemcpyDeviceToHost, s));
    if (o.states) HIPCHK(hipMemcpyAsync(o.states, sc.X, sizeof(double) * rows * d, hipMemcpyDeviceToHost, s));
    if (o.index) {
      i32.resize(rows);
      HIPCHK(hipMemcpyAsync(i32.data(), sc.idx, sizeof(int) * rows, hipMemcpyDeviceToHost, s));
    }
    if (o.classes) {
      c32.resize(rows);
      HIPCHK(hipMemcpyAsync(c32.data(), sc.cls, sizeof(int) * rows, hipMemcpyDeviceToHost, s));
    }
    return GPMDM_OK;
  };
  const int rc = launches();
  TRY(pf->fs_out.finish(rc, s));          // (quiesce waits for the launches if the wait fails)
  if (pf->sm_pending && pf->sm_stream == s) pf->sm_pending = false;   // (the record preceded the launches on s)
  const double* pin = pf->fs_out.pin;
  const double nan = std::nan("");
  for (int l = 0; l < L1; ++l) {
    const double* row = pin + (size_t)l * W;
    const double alive = row[0];
    if (o.alive) o.alive[l] = (int64_t)alive;
    if (o.distinct) o.distinct[l] = (int64_t)row[1];
    for (int c = 0; o.class_prob && c < C; ++c) o.class_prob[(size_t)l * C + c] = alive > 0 ? row[2 + c] / alive : nan;
    for (int q = 0; o.state_mean && q < d; ++q)   // the two-term sum's quotient, rounded once
      o.state_mean[(size_t)l * d + q] =
          alive > 0 ? (double)(((long double)row[2 + C + q] + (long double)row[2 + C + d + q]) / (long double)alive) : nan;
  }
  for (size_t i = 0; i < i32.size(); ++i) o.index[i] = i32[i];
  for (size_t i = 0; i < c32.size(); ++i) o.classes[i] = c32[i];
  if (!obs) return GPMDM_OK;
  // The pose of each lag: the read-out gpmdm_pf_smoothed runs on a traced cloud, here on the
  // lag's alive states -- the rows themselves, or with dead trajectories their stable compaction
  // (k_bs_group on the alive flags: the alive rows follow the dead ones).
  double* out_ro = pf->fs_out.dev + (size_t)L1 * W;
  auto poses = [&]() -> int {
    for (int l = 0; l < L1; ++l) {
      const long long alive = (long long)pin[(size_t)l * W];
      if (alive == 0) continue;
      const size_t r = (size_t)l * n;
      const double* X = sc.X + r * d;
      if (alive < n) {
        TRY(sc.ro_flag.grow((size_t)n, s));
        TRY(sc.ro_perm.grow((size_t)n, s));
        TRY(sc.ro_tab.grow((size_t)2 * kMaxClasses + 2, s));
        TRY(sc.ro_X.grow((size_t)n * d, s));
        launch_fs_flag(sc.idx + r, n, sc.ro_flag, s);
        BsGroupArgs ga{};
        ga.n = n;
        ga.C = 2;
        ga.cls = sc.ro_flag;
        ga.perm = sc.ro_perm;
        ga.tab = sc.ro_tab;
        launch_bs_group(ga, s);
        FsGatherArgs fa{};
        fa.n = alive;
        fa.d = d;
        fa.idx = sc.ro_perm + (n - alive);
        fa.X = X;
        fa.X_out = sc.ro_X;               // (the states alone: no class row)
        launch_fs_gather(fa, s);
        X = sc.ro_X;
      }
      ReadoutParams rp = pose_readout(pf, X, sc.ro_part, out_ro + (size_t)l * 2 * D);
      rp.P = alive;
      rp.F = 1;
      launch_obs_readout(rp, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->fs_out.pin + (size_t)L1 * W, out_ro, sizeof(double) * L1 * 2 * D, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  TRY(pf->fs_out.finish(poses(), s));
  for (int l = 0; l < L1; ++l) {
    const bool any = pin[(size_t)l * W] > 0;
    const double* ro = pin + (size_t)L1 * W + (size_t)l * 2 * D;
    for (int j = 0; j < D; ++j) {
      if (o.obs_mean) o.obs_mean[(size_t)l * D + j] = any ? ro[j] : nan;
      if (o.obs_spread) o.obs_spread[(size_t)l * D + j] = any ? ro[D + j] : nan;
    }
  }
  return GPMDM_OK;
}

}  // extern "C"
