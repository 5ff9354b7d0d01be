// C ABI, the forecast roll-out (gpmdm_pf_forecast, gpmdm_bank_forecast): H steps of the filter's
// proposal on a scratch copy of the cloud, all queued on the caller's stream -- per step the
// roll-out switch, the filter's grouping passes on the forecast's own tables, the dynamics-GP
// tiles as predict() launches them, the roll-out finish, (the bank entry's) per-filter sum and
// the reduce, and the pose read-out pointed at the scratch cloud -- then one copy-back and one
// wait.  Grouping and tiles run over all F x Pf particles; sums, counts and the pose per filter.
// The two entry points differ in their handle checks and in who sums the mean state
// (forecast.h); every device result is step-major, then filter-major.  Kernels: forecast.h.
#include "capi_internal.h"
#include "forecast.h"

namespace gpmdm::capi {

// Scratch of both entry points, and H x F result rows: {class_prob[C], state_mean[d]} of every
// (step, filter), then {mean[D], spread[D]} of every (step, filter) -- the read-out writes the
// F filters of a step as one contiguous block.
static int ensure_scratch(gpmdm_pf* pf, int H, bool obs, bool per_filter_sums, hipStream_t s) {
  const gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d, D = m->D, F = pf->F;
  const long long P = pf->P;
  const long long nb = cdiv(P, 256), nbf = cdiv(pf->Pf, 256);
#define NEED(buf, n) TRY(pf->buf.grow((size_t)(n), s))
  for (int k = 0; k < 2; ++k) {
    NEED(fc_X[k], P * d);
    NEED(fc_cls[k], P);
  }
  NEED(fc_perm, P);
  NEED(fc_blockcounts, nb * C);
  NEED(fc_blockoff, nb * C);
  NEED(fc_mu, P * d);
  NEED(fc_part, F * nbf * d);
  if (per_filter_sums) NEED(fc_bcounts, F * nbf * C);
  NEED(fc_tab, 256);
  NEED(fc_q, (size_t)pf->nparts_dyn_max * P);
  if (obs) NEED(fc_ro_part, readout_part_doubles(pf->Pf, D, F));
#undef NEED
  return pf->fc_out.reserve((size_t)H * F * (C + d + 2 * D), s);
}

// The filter's grouping passes on the forecast's own tables: classes `cls` (all pf->P particles,
// a bank's F x Pf among them), whose per-block counts are in fc_blockcounts.
static void fc_group(gpmdm_pf* pf, const int* cls, hipStream_t s) {
  const gpmdm_model* m = pf->m;
  ScanArgs sc{};
  GroupArgs ga{};
  fill_grouping(sc, ga, ClassTables{pf->fc_tab}, pf->fc_blockcounts, pf->fc_blockoff, pf->fc_perm, cls, pf->P, m->C,
                m->dyn_set(true)[0].geo.pt());
  launch_scan_counts(sc, s);
  launch_group(ga, s);
}

// Every launch of the roll-out.  per_filter_sums: k_fc_sum sums the new cloud and counts its
// classes per filter (gpmdm_bank_forecast, whatever F); else the finish sums its own blocks and
// the class counts are the grouping's (gpmdm_pf_forecast, F = 1).  stage_X / stage_cls (or
// nullptr): H x P x d / H x P device rows that take each step's cloud instead of the ping-pong
// halves (the next step reads its input there: no copy).
static int launch_rollout(gpmdm_pf* pf, int H, bool mean_only, bool obs, bool per_filter_sums, unsigned seed_lo,
                          unsigned seed_hi, double* stage_X, int* stage_cls, hipStream_t s) {
  gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d, D = m->D, F = pf->F;
  const long long P = pf->P, Pf = pf->Pf;
  const int nbf = (int)cdiv(Pf, 256);
  const std::vector<GpImage>& dset = m->dyn_set(true);   // every particle is evaluated: predict()'s images
  const ClassTables tb{pf->fc_tab};
  double* out_ro = pf->fc_out.dev + (size_t)H * F * (C + d);
  const double* Xcur = pf->X;
  const int* ccur = pf->cls;
  for (int h = 0; h < H; ++h) {
    double* Xnext = stage_X ? stage_X + (size_t)h * P * d : pf->fc_X[h & 1];
    const bool regroup = !mean_only || h == 0;   // (mean mode: classes frozen, one grouping and one count)
    if (regroup) {
      if (mean_only) {
        launch_class_hist(ccur, P, C, pf->fc_blockcounts, s);
      } else {
        int* cnext = stage_cls ? stage_cls + (size_t)h * P : pf->fc_cls[h & 1];
        FcSwitchArgs sa{};
        sa.P = P;
        sa.Pf = Pf;
        sa.C = C;
        sa.h = (unsigned)(h + 1);
        sa.frame = pf->frame;
        sa.seed_lo = seed_lo;
        sa.seed_hi = seed_hi;
        sa.cls = ccur;
        sa.cls_new = cnext;
        sa.T = pf->T;
        sa.blockcounts = pf->fc_blockcounts;
        launch_fc_switch(sa, s);
        ccur = cnext;
      }
      fc_group(pf, ccur, s);
    }
    // each class's dynamics GP on the scratch cloud, rows in the grouped order of fc_group
    // (gpmdm_pf_predict's launches: every particle is evaluated)
    launch_dyn_tiles(m, dset, dset[0].geo, tb.seg(), pf->fc_perm, Xcur, P, pf->fc_q, P, pf->fc_mu, s);
    FcFinishArgs fa{};
    fa.P = P;
    fa.Pf = Pf;
    fa.C = C;
    fa.d = d;
    fa.mean_only = mean_only ? 1 : 0;
    fa.h = (unsigned)(h + 1);
    fa.frame = pf->frame;
    fa.seed_lo = seed_lo;
    fa.seed_hi = seed_hi;
    fa.seg_out_base = tb.seg().out();
    fa.seg_pos_begin = tb.seg().begin();
    fa.perm = pf->fc_perm;
    for (int c = 0; c < C; ++c) fa.n_parts[c] = dset[c].n_parts();
    fa.qpart = pf->fc_q;
    fa.ld_q = P;
    fa.mu = pf->fc_mu;
    fa.X = Xcur;
    for (int j = 0; j <= d; ++j) fa.lin_c2[j] = m->x_lin_c2[j];
    for (int j = 0; j < d; ++j) fa.il2[j] = m->x_il2[j];
    fa.X_out = Xnext;
    fa.partials = per_filter_sums ? nullptr : pf->fc_part;
    launch_fc_finish(fa, s);
    if (per_filter_sums) {               // the new cloud's sums in particle order, and the step's class counts
      FcSumArgs ua{};
      ua.Pf = Pf;
      ua.C = C;
      ua.d = d;
      ua.X = Xnext;
      ua.cls = regroup ? ccur : nullptr;
      ua.bcounts = pf->fc_bcounts;
      ua.partials = pf->fc_part;
      launch_fc_sum(ua, F, s);
    }
    FcReduceArgs ra{};
    ra.Pf = Pf;
    ra.C = C;
    ra.d = d;
    ra.nbf = nbf;
    ra.n_count_rows = per_filter_sums ? nbf : 1;
    ra.counts = per_filter_sums ? pf->fc_bcounts : tb.counts();
    ra.partials = pf->fc_part;
    ra.out = pf->fc_out.dev + (size_t)h * F * (C + d);
    launch_fc_reduce(ra, F, s);
    if (obs)                             // the step's pose: one read-out over the F clouds
      launch_obs_readout(pose_readout(pf, Xnext, pf->fc_ro_part, out_ro + (size_t)h * F * 2 * D), s);
    Xcur = Xnext;
    HIPCHK(hipGetLastError());
  }
  return GPMDM_OK;
}

// The body of both entry points on a checked handle.  stage_refusal: the entry point's wording
// of the 1 GiB staging limit.
static int forecast(gpmdm_pf* pf, int horizon, int mode, const uint64_t* seed, const gpmdm_forecast_out* out,
                    void* stream, bool per_filter_sums, const char* stage_refusal) {
  CHECK(horizon >= 1 && horizon <= GPMDM_FORECAST_MAX_HORIZON, "horizon must be in [1, GPMDM_FORECAST_MAX_HORIZON]");
  CHECK(mode == GPMDM_FORECAST_SAMPLE || mode == GPMDM_FORECAST_MEAN, "mode: GPMDM_FORECAST_SAMPLE or GPMDM_FORECAST_MEAN");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the forecast's)
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "forecast between switch and resample");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int C = m->C, d = m->d, D = m->D, H = horizon, F = pf->F;
  const long long P = pf->P;
  const bool mean_only = mode == GPMDM_FORECAST_MEAN;
  static const gpmdm_forecast_out none{};
  const gpmdm_forecast_out& o = out ? *out : none;
  const bool obs = o.obs_mean || o.obs_spread;
  if (o.states || o.classes)
    CHECK((size_t)H * (size_t)P * (size_t)(d + 1) <= kForecastStageBytes / sizeof(double), stage_refusal);
  const unsigned long long sd = seed ? *seed : (((unsigned long long)pf->seed_hi << 32) | pf->seed_lo);
  TRY(ensure_scratch(pf, H, obs, per_filter_sums, s));
  // per-call staging of the clouds, released in the stream's order on every exit
  DevBuf<double> stage_X;
  DevBuf<int> stage_cls;
  if (o.states) TRY(stage_X.alloc((size_t)H * P * d));
  if (o.classes && !mean_only && stage_cls.alloc((size_t)H * P) != GPMDM_OK) return GPMDM_E_NOMEM;
  int rc = launch_rollout(pf, H, mean_only, obs, per_filter_sums, (unsigned)(sd & 0xffffffffu), (unsigned)(sd >> 32),
                          stage_X, stage_cls, s);
  const size_t n_rows = (size_t)H * F;
  const size_t n_out = n_rows * (C + d) + (obs ? n_rows * 2 * D : 0);
  std::vector<int> c32;
  auto copies = [&]() -> int {
    HIPCHK(hipMemcpyAsync(pf->fc_out.pin, pf->fc_out.dev, sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    if (o.states) HIPCHK(hipMemcpyAsync(o.states, stage_X, sizeof(double) * H * P * d, hipMemcpyDeviceToHost, s));
    if (o.classes) {
      c32.resize((size_t)(mean_only ? 1 : H) * P);   // (mean mode: the filters' classes, every step)
      HIPCHK(hipMemcpyAsync(c32.data(), mean_only ? pf->cls.p : stage_cls.p, sizeof(int) * c32.size(),
                            hipMemcpyDeviceToHost, s));
    }
    return GPMDM_OK;
  };
  if (rc == GPMDM_OK) rc = copies();
  stage_X.release_after(s);
  stage_cls.release_after(s);
  TRY(pf->fc_out.finish(rc, s));         // (quiesce waits for the launches if the wait fails)
  const double* ro = pf->fc_out.pin + n_rows * (C + d);
  for (size_t q = 0; q < n_rows; ++q) {  // q = h * F + f
    const double* row = pf->fc_out.pin + q * (C + d);
    if (o.class_prob) std::memcpy(o.class_prob + q * C, row, sizeof(double) * C);
    if (o.state_mean) std::memcpy(o.state_mean + q * d, row + C, sizeof(double) * d);
    if (o.obs_mean) std::memcpy(o.obs_mean + q * D, ro + q * 2 * D, sizeof(double) * D);
    if (o.obs_spread) std::memcpy(o.obs_spread + q * D, ro + q * 2 * D + D, sizeof(double) * D);
  }
  if (o.classes)
    for (size_t i = 0; i < (size_t)H * P; ++i) o.classes[i] = c32[mean_only ? i % (size_t)P : i];
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_pf_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed, const gpmdm_forecast_out* out,
                      void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "the forecast serves single filters, not banks (gpmdm_bank_forecast)");
  return forecast(pf, horizon, mode, seed, out, stream, false,
                  "states / classes of this forecast need more than 1 GiB of device staging (H x P x (d + 1) doubles)");
}

int gpmdm_bank_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed, const gpmdm_forecast_out* out,
                        void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F <= 65535, "the bank forecast serves up to 65535 filters");
  return forecast(pf, horizon, mode, seed, out, stream, true,
                  "states / classes of this forecast need more than 1 GiB of device staging (H x F x P x (d + 1) "
                  "doubles)");
}

}  // extern "C"
