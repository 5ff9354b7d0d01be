// C ABI, forecasts and fixed-lag smoothing for filter banks (gpmdm_bank_forecast,
// gpmdm_bank_set_smoothing, gpmdm_bank_smoothed): the launch sequences of capi_forecast.hip and
// capi_smooth.hip with the filter dimension of bank_rollout.h.  The grouping passes and the
// dynamics tiles run bank-wide over all F x Pf particles; sums, counts and the pose read-out run
// per filter.  Every device result is step-major, then filter-major.  The ring's record
// (sm_record, behind every resample of an enabled handle) and its clears serve banks as they are.
#include "capi_internal.h"
#include "bank_rollout.h"

namespace gpmdm::capi {

// gpmdm_pf_forecast's scratch (shared: at F = 1 every size is that call's), the per-filter
// blocks' sums and counts, and H x F result rows: {class_prob[C], state_mean[d]} of every
// (step, filter), then {mean[D], spread[D]} of every (step, filter) -- the read-out writes the
// F filters of a step as one contiguous block.
static int ensure_scratch(gpmdm_pf* pf, int H, bool obs) {
  const gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d, D = m->D, F = pf->F;
  const long long P = pf->P;
  const long long nb = cdiv(P, 256), nbf = cdiv(pf->Pf, 256);
#define NEED(ptr, n) do { if (!(ptr)) TRY(dalloc(&(ptr), (size_t)(n))); } while (0)
  for (int k = 0; k < 2; ++k) {
    NEED(pf->fc_X[k], P * d);
    NEED(pf->fc_cls[k], P);
  }
  NEED(pf->fc_perm, P);
  NEED(pf->fc_blockcounts, nb * C);
  NEED(pf->fc_blockoff, nb * C);
  NEED(pf->fc_mu, P * d);
  NEED(pf->fc_part, F * nbf * d);
  NEED(pf->fc_bcounts, F * nbf * C);
  NEED(pf->fc_tab, 256);
#undef NEED
  const size_t qn = (size_t)pf->nparts_dyn_max * P;
  if (pf->fc_q_cap < qn) {
    dfree(pf->fc_q);
    pf->fc_q_cap = 0;
    TRY(dalloc(&pf->fc_q, qn));
    pf->fc_q_cap = qn;
  }
  if (obs && !pf->fc_ro_part) TRY(dalloc(&pf->fc_ro_part, readout_part_doubles(pf->Pf, D, F)));
  const size_t on = (size_t)H * F * (C + d + 2 * D);
  if (pf->fc_out_cap < on) {
    dfree(pf->fc_out);
    hfree(pf->fc_pin);
    pf->fc_out_cap = 0;
    TRY(dalloc(&pf->fc_out, on));
    TRY(halloc(&pf->fc_pin, on, 0));
    pf->fc_out_cap = on;
  }
  if (!pf->fc_ev) HIPCHK(hipEventCreateWithFlags(&pf->fc_ev, hipEventDisableTiming));
  return GPMDM_OK;
}

static ReadoutParams bank_readout(const gpmdm_pf* pf, const double* X, double* part, double* out) {
  const gpmdm_model* m = pf->m;
  ReadoutParams rp{};
  rp.X = X;
  rp.P = pf->Pf;
  rp.F = pf->F;
  rp.d = m->d;
  rp.D = m->D;
  rp.ls = m->y_ls_dev;
  rp.Xrec = m->obs.Xrec;
  rp.nks = ksteps((int)m->N);
  rp.Bro = m->ro_beta;
  rp.n_groups = readout_groups(m->D);
  rp.part = part;
  rp.out = out;                          // F x {mean[D], spread[D]}
  return rp;
}

// Every launch of the bank's roll-out (launch_rollout of capi_forecast.hip, with the filter
// dimension).  stage_X / stage_cls (or nullptr): H x P x d / H x P device rows that take each
// step's cloud instead of the ping-pong halves.
static int launch_rollout(gpmdm_pf* pf, int H, bool mean_only, bool obs, unsigned seed_lo, unsigned seed_hi,
                          double* stage_X, int* stage_cls, hipStream_t s) {
  gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d, D = m->D, F = pf->F;
  const long long P = pf->P, Pf = pf->Pf;
  const int nbf = (int)cdiv(Pf, 256);
  const std::vector<GpImage>& dset = m->dyn_set(true);   // every particle is evaluated: predict()'s images
  const FcTables tb{pf->fc_tab};
  double* out_ro = pf->fc_out + (size_t)H * F * (C + d);
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
        FcbSwitchArgs sa{};
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
        launch_fcb_switch(sa, s);
        ccur = cnext;
      }
      fc_group(pf, ccur, s);
    }
    fc_tiles(pf, Xcur, s);
    FcbFinishArgs fa{};
    fa.P = P;
    fa.Pf = Pf;
    fa.C = C;
    fa.d = d;
    fa.mean_only = mean_only ? 1 : 0;
    fa.h = (unsigned)(h + 1);
    fa.frame = pf->frame;
    fa.seed_lo = seed_lo;
    fa.seed_hi = seed_hi;
    fa.seg_out_base = tb.seg_out();
    fa.seg_pos_begin = tb.seg_begin();
    fa.perm = pf->fc_perm;
    for (int c = 0; c < C; ++c) fa.n_parts[c] = dset[c].n_parts();
    fa.qpart = pf->fc_q;
    fa.ld_q = P;
    fa.mu = pf->fc_mu;
    fa.X = Xcur;
    for (int j = 0; j <= d; ++j) fa.lin_c2[j] = m->x_lin_c2[j];
    for (int j = 0; j < d; ++j) fa.il2[j] = m->x_il2[j];
    fa.X_out = Xnext;
    launch_fcb_finish(fa, s);
    // per filter: the new cloud's sums in particle order, and the class counts of the step
    FcbSumArgs ua{};
    ua.Pf = Pf;
    ua.C = C;
    ua.d = d;
    ua.X = Xnext;
    ua.cls = regroup ? ccur : nullptr;
    ua.bcounts = pf->fc_bcounts;
    ua.partials = pf->fc_part;
    launch_fcb_sum(ua, F, s);
    FcbReduceArgs ra{};
    ra.Pf = Pf;
    ra.C = C;
    ra.d = d;
    ra.nbf = nbf;
    ra.bcounts = pf->fc_bcounts;
    ra.partials = pf->fc_part;
    ra.out = pf->fc_out + (size_t)h * F * (C + d);
    launch_fcb_reduce(ra, F, s);
    if (obs)                             // the step's pose: one read-out over the F clouds
      launch_obs_readout(bank_readout(pf, Xnext, pf->fc_ro_part, out_ro + (size_t)h * F * 2 * D), s);
    Xcur = Xnext;
    HIPCHK(hipGetLastError());
  }
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_bank_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed, const gpmdm_forecast_out* out,
                        void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F <= 65535, "the bank forecast serves up to 65535 filters");
  CHECK(horizon >= 1 && horizon <= GPMDM_FORECAST_MAX_HORIZON, "horizon must be in [1, GPMDM_FORECAST_MAX_HORIZON]");
  CHECK(mode == GPMDM_FORECAST_SAMPLE || mode == GPMDM_FORECAST_MEAN, "mode: GPMDM_FORECAST_SAMPLE or GPMDM_FORECAST_MEAN");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the forecast's)
  if ((pf->switched && !pf->preswitched) || pf->dyn_done || pf->propagated)
    return fail(GPMDM_E_STATE, "forecast between switch and resample");
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
    CHECK((size_t)H * (size_t)P * (size_t)(d + 1) <= kForecastStageBytes / sizeof(double),
          "states / classes of this forecast need more than 1 GiB of device staging (H x F x P x (d + 1) doubles)");
  const unsigned long long sd = seed ? *seed : (((unsigned long long)pf->seed_hi << 32) | pf->seed_lo);
  TRY(ensure_scratch(pf, H, obs));
  // per-call staging of the clouds, released in the stream's order on every exit
  double* stage_X = nullptr;
  int* stage_cls = nullptr;
  if (o.states) TRY(dalloc(&stage_X, (size_t)H * P * d));
  if (o.classes && !mean_only && dalloc(&stage_cls, (size_t)H * P) != GPMDM_OK) {
    dfree(stage_X);
    return GPMDM_E_NOMEM;
  }
  int rc = launch_rollout(pf, H, mean_only, obs, (unsigned)(sd & 0xffffffffu), (unsigned)(sd >> 32), stage_X,
                          stage_cls, s);
  const size_t n_rows = (size_t)H * F;
  const size_t n_out = n_rows * (C + d) + (obs ? n_rows * 2 * D : 0);
  std::vector<int> c32;
  auto copies = [&]() -> int {
    HIPCHK(hipMemcpyAsync(pf->fc_pin, pf->fc_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    if (o.states) HIPCHK(hipMemcpyAsync(o.states, stage_X, sizeof(double) * H * P * d, hipMemcpyDeviceToHost, s));
    if (o.classes) {
      c32.resize((size_t)(mean_only ? 1 : H) * P);   // (mean mode: the filters' classes, every step)
      HIPCHK(hipMemcpyAsync(c32.data(), mean_only ? pf->cls : stage_cls, sizeof(int) * c32.size(),
                            hipMemcpyDeviceToHost, s));
    }
    return GPMDM_OK;
  };
  if (rc == GPMDM_OK) rc = copies();
  const bool marked = hipEventRecord(pf->fc_ev, s) == hipSuccess;
  pf->fc_pending = marked;               // (quiesce waits for the launches if the wait below fails)
  if (stage_X) dfree_after(stage_X, s);
  if (stage_cls) dfree_after(stage_cls, s);
  if (rc != GPMDM_OK) return rc;
  HIPCHK(hipStreamSynchronize(s));
  pf->fc_pending = false;
  const double* ro = pf->fc_pin + n_rows * (C + d);
  for (size_t q = 0; q < n_rows; ++q) {  // q = h * F + f
    const double* row = pf->fc_pin + q * (C + d);
    if (o.class_prob) std::memcpy(o.class_prob + q * C, row, sizeof(double) * C);
    if (o.state_mean) std::memcpy(o.state_mean + q * d, row + C, sizeof(double) * d);
    if (o.obs_mean) std::memcpy(o.obs_mean + q * D, ro + q * 2 * D, sizeof(double) * D);
    if (o.obs_spread) std::memcpy(o.obs_spread + q * D, ro + q * 2 * D + D, sizeof(double) * D);
  }
  if (o.classes)
    for (size_t i = 0; i < (size_t)H * P; ++i) o.classes[i] = c32[mean_only ? i % (size_t)P : i];
  return GPMDM_OK;
}

int gpmdm_bank_set_smoothing(gpmdm_pf_t pf, int lag) {
  CHECK(pf, "null handle");
  return sm_set(pf, lag);
}

int gpmdm_bank_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F <= 65535, "bank smoothing serves up to 65535 filters");
  CHECK(pf->sm_L > 0, "smoothing is off (gpmdm_bank_set_smoothing)");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the smoother's)
  if ((pf->switched && !pf->preswitched) || pf->dyn_done || pf->propagated)
    return fail(GPMDM_E_STATE, "smoothed between switch and resample");
  CHECK(lag_first >= 0 && lag_first <= lag_last, "lags: 0 <= lag_first <= lag_last");
  CHECK(lag_last <= pf->sm_depth, "lag_last is above the recorded depth (gpmdm_pf_smoothing_depth)");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int C = m->C, d = m->d, D = m->D, F = pf->F;
  const long long P = pf->P, Pf = pf->Pf;
  const int n = lag_last - lag_first + 1;
  const size_t n_rows = (size_t)n * F;   // row q = (l - lag_first) * F + f
  const int W = C + d + 1;
  const long long nbf = sm_blocks(Pf), ldm = sm_ld_marks(Pf);
  static const gpmdm_smoothed_out none{};
  const gpmdm_smoothed_out& o = out ? *out : none;
  const bool obs = o.obs_mean || o.obs_spread;
  const bool want_X = obs || o.states;
  const size_t cnt_bytes = (n_rows * C * sizeof(int) + 15) & ~(size_t)15;   // counts, then the marks
  const size_t stage = n_rows * (size_t)ldm + (size_t)n * P * ((want_X ? sizeof(double) * d : 0) +
                                                               (o.ancestors ? sizeof(int) : 0) +
                                                               (o.classes ? sizeof(int) : 0));
  CHECK(stage <= kSmoothBytes, "these lags need more than 1 GiB of device staging (rows of F x P states, ancestors, "
                               "classes and marks per lag): ask for fewer lags per call");
  TRY(grow(pf->sm_marks, pf->sm_marks_cap, cnt_bytes + n_rows * ldm, s));
  TRY(grow(pf->sm_part, pf->sm_part_cap, n_rows * nbf * d, s));
  const size_t n_out = n_rows * W + n_rows * 2 * D;   // the rows, then {mean[D], spread[D]} of every row
  if (pf->sm_out_cap < n_out) {
    hfree(pf->sm_pin);
    TRY(grow(pf->sm_out, pf->sm_out_cap, n_out, s));
    TRY(halloc(&pf->sm_pin, n_out, 0));
  }
  if (obs && !pf->sm_ro_part) TRY(dalloc(&pf->sm_ro_part, readout_part_doubles(Pf, D, F)));
  // per-call staging of the particle rows, released in the stream's order on every exit
  double* stage_X = nullptr;
  int *stage_anc = nullptr, *stage_cls = nullptr;
  int rc = GPMDM_OK;
  if (want_X) rc = dalloc(&stage_X, (size_t)n * P * d);
  if (rc == GPMDM_OK && o.ancestors) rc = dalloc(&stage_anc, (size_t)n * P);
  if (rc == GPMDM_OK && o.classes) rc = dalloc(&stage_cls, (size_t)n * P);
  std::vector<int> a32, c32;
  double* out_ro = pf->sm_out + n_rows * W;
  auto launches = [&]() -> int {
    // the record of the latest frame, if it ran on another stream
    if (pf->sm_pending && pf->sm_stream != s) HIPCHK(hipStreamWaitEvent(s, pf->sm_ev, 0));
    int* counts = reinterpret_cast<int*>(pf->sm_marks);
    unsigned char* marks = pf->sm_marks + cnt_bytes;
    HIPCHK(hipMemsetAsync(pf->sm_marks, 0, cnt_bytes + n_rows * ldm, s));
    SmbTraceArgs ta{};
    ta.Pf = Pf;
    ta.F = F;
    ta.C = C;
    ta.d = d;
    ta.lag_first = lag_first;
    ta.lag_last = lag_last;
    ta.ring = SmRing{pf->sm_anc, pf->sm_cls, pf->sm_X, pf->sm_L + 1, pf->sm_slot()};
    ta.counts = counts;
    ta.partials = pf->sm_part;
    ta.marks = marks;
    ta.ld_marks = ldm;
    ta.anc_out = stage_anc;
    ta.cls_out = stage_cls;
    ta.X_out = stage_X;
    launch_smb_trace(ta, s);
    SmbReduceArgs ra{};
    ra.Pf = Pf;
    ra.C = C;
    ra.d = d;
    ra.nbf = (int)nbf;
    ra.counts = counts;
    ra.partials = pf->sm_part;
    ra.marks = marks;
    ra.ld_marks = ldm;
    ra.out = pf->sm_out;
    ra.ld_out = W;
    launch_smb_reduce(ra, n, F, s);
    for (int r = 0; obs && r < n; ++r)   // each lag's pose: one read-out over the F traced clouds
      launch_obs_readout(bank_readout(pf, stage_X + (size_t)r * P * d, pf->sm_ro_part, out_ro + (size_t)r * F * 2 * D), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->sm_pin, pf->sm_out, sizeof(double) * (obs ? n_out : n_rows * W), hipMemcpyDeviceToHost, s));
    if (o.states) HIPCHK(hipMemcpyAsync(o.states, stage_X, sizeof(double) * n * P * d, hipMemcpyDeviceToHost, s));
    if (o.ancestors) {
      a32.resize((size_t)n * P);
      HIPCHK(hipMemcpyAsync(a32.data(), stage_anc, sizeof(int) * a32.size(), hipMemcpyDeviceToHost, s));
    }
    if (o.classes) {
      c32.resize((size_t)n * P);
      HIPCHK(hipMemcpyAsync(c32.data(), stage_cls, sizeof(int) * c32.size(), hipMemcpyDeviceToHost, s));
    }
    return GPMDM_OK;
  };
  if (rc == GPMDM_OK) rc = launches();
  pf->sm_tr_pending = hipEventRecord(pf->sm_tr_ev, s) == hipSuccess;   // (quiesce waits if the wait below fails)
  if (stage_X) dfree_after(stage_X, s);
  if (stage_anc) dfree_after(stage_anc, s);
  if (stage_cls) dfree_after(stage_cls, s);
  if (rc != GPMDM_OK) return rc;
  HIPCHK(hipStreamSynchronize(s));
  pf->sm_tr_pending = false;
  if (pf->sm_pending && pf->sm_stream == s) pf->sm_pending = false;   // (the record preceded the trace on s)
  const double* ro = pf->sm_pin + n_rows * W;
  for (size_t q = 0; q < n_rows; ++q) {
    const double* row = pf->sm_pin + q * W;
    if (o.class_prob) std::memcpy(o.class_prob + q * C, row, sizeof(double) * C);
    if (o.state_mean) std::memcpy(o.state_mean + q * d, row + C, sizeof(double) * d);
    if (o.distinct) o.distinct[q] = (int64_t)row[C + d];
    if (o.obs_mean) std::memcpy(o.obs_mean + q * D, ro + q * 2 * D, sizeof(double) * D);
    if (o.obs_spread) std::memcpy(o.obs_spread + q * D, ro + q * 2 * D + D, sizeof(double) * D);
  }
  for (size_t i = 0; i < a32.size(); ++i) o.ancestors[i] = a32[i];
  for (size_t i = 0; i < c32.size(); ++i) o.classes[i] = c32[i];
  return GPMDM_OK;
}

}  // extern "C"
