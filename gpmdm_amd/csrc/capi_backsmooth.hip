// C ABI, marginal backward smoothing (gpmdm_backward_step, gpmdm_pf_smoothed_marginal): one
// implementation of the backward step (bs_step: the sources' moments from gpmdm_predict_dyn's
// launch builder for every class, the targets' grouping, the two passes and their finishes, all
// queued on the caller's stream), applied to the caller's arrays by the first entry point and to
// the slots of the ancestry ring (capi_smooth.hip) by the second.  Kernels: backsmooth.h.
#include "capi_internal.h"
#include "backsmooth.h"

namespace gpmdm::capi {

constexpr long long kBsMaxPairs = 1ll << 36;

size_t bs_record_bytes(int C, int d, long long n_s) {
  return sizeof(double) * (size_t)C * (size_t)n_s * (size_t)(2 * d + 1);
}

// The step's refusals, decided before any launch.
int bs_check(const gpmdm_model* m, long long n_s, long long n_t) {
  CHECK(n_s >= 1 && n_t >= 1 && n_s < (1ll << 31) && n_t < (1ll << 31), "backward step: n_s and n_t must be in [1, 2^31)");
  CHECK(n_s <= kBsMaxPairs / n_t, "backward step: more than 2^36 source-target pairs (P > 262144)");
  CHECK(bs_record_bytes(m->C, m->d, n_s) <= kSmoothBytes,
        "backward step: the sources' moments need more than 1 GiB of device staging (C x n_s x (2 d + 1) doubles)");
  return GPMDM_OK;
}

// The sources' records of every class (k_bs_moments behind gpmdm_predict_dyn's launches), queued
// on s; the buffers are grown as needed.
int bs_records(const gpmdm_model* m, DevBuf<double>& rec, DevBuf<double>& mu, DevBuf<double>& var, DevBuf<double>& q,
               const double* T, long long n_s, const double* Xs, const int* cs, const double* a, hipStream_t s) {
  const int C = m->C, d = m->d;
  size_t nq = 0;
  for (int c = 0; c < C; ++c) nq = std::max(nq, predict_dyn_scratch(m, c, n_s));
  TRY(rec.grow((size_t)C * n_s * (2 * d + 1), s));
  TRY(mu.grow((size_t)n_s * d, s));
  TRY(var.grow((size_t)n_s * d, s));
  TRY(q.grow(nq, s));
  for (int c = 0; c < C; ++c) {
    launch_predict_dyn(m, c, Xs, n_s, mu, var, q, s);
    BsMomentArgs ma{};
    ma.n = n_s;
    ma.C = C;
    ma.d = d;
    ma.c = c;
    ma.mu = mu;
    ma.var = var;
    ma.cls = cs;
    ma.a = a;
    ma.T = T;
    ma.rec = rec;
    launch_bs_moments(ma, s);
  }
  return GPMDM_OK;
}

// One backward step on device arrays (a: nullptr for equal weights; log_den: nullptr if not
// wanted), queued on s.  Sizes checked by the caller (bs_check).
static int bs_step(const gpmdm_model* m, BsScratch& sc, const double* T, long long n_s, const double* Xs,
                   const int* cs, const double* a, long long n_t, const double* Xt, const int* ct, const double* wt,
                   double* ws, double* log_den, hipStream_t s) {
  const int C = m->C, d = m->d;
  const int split_d = bs_split(n_t, n_s), split_w = bs_split(n_s, n_t);
  TRY(bs_records(m, sc.rec, sc.mu, sc.var, sc.q, T, n_s, Xs, cs, a, s));
  TRY(sc.perm.grow((size_t)n_t, s));
  TRY(sc.tab.grow((size_t)2 * kMaxClasses + 2, s));
  TRY(sc.lw.grow((size_t)n_t, s));
  TRY(sc.part.grow(2 * std::max((size_t)split_d * n_t, (size_t)split_w * n_s), s));
  BsGroupArgs ga{};
  ga.n = n_t;
  ga.C = C;
  ga.cls = ct;
  ga.perm = sc.perm;
  ga.tab = sc.tab;
  launch_bs_group(ga, s);
  BsPassArgs pa{};
  pa.n_s = n_s;
  pa.n_t = n_t;
  pa.C = C;
  pa.d = d;
  pa.rec = sc.rec;
  pa.Xt = Xt;
  pa.perm = sc.perm;
  pa.tab = sc.tab;
  pa.lw = sc.lw;
  pa.part = sc.part;
  pa.split = split_d;
  launch_bs_den(pa, s);
  BsDenFinArgs df{};
  df.n_t = n_t;
  df.split = split_d;
  df.part = sc.part;
  df.perm = sc.perm;
  df.wt = wt;
  df.log_den = log_den;
  df.lw = sc.lw;
  launch_bs_den_fin(df, s);
  pa.split = split_w;
  launch_bs_wgt(pa, s);
  BsWgtFinArgs wf{};
  wf.n_s = n_s;
  wf.split = split_w;
  wf.part = sc.part;
  wf.ws = ws;
  launch_bs_wgt_fin(wf, s);
  HIPCHK(hipGetLastError());
  return GPMDM_OK;
}

int bs_to_classes(const int64_t* src, long long n, int C, std::vector<int>& dst, const char* what) {
  dst.resize((size_t)n);
  for (long long i = 0; i < n; ++i) {
    CHECK(src[i] >= 0 && src[i] < C, std::string("backward step: a class of the ") + what + " is outside [0, C)");
    dst[(size_t)i] = (int)src[i];
  }
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_backward_step(gpmdm_model_t m, const double* T, int64_t n_s, const double* Xs, const int64_t* cs,
                        const double* a, int64_t n_t, const double* Xt, const int64_t* ct, const double* wt,
                        double* ws_out, double* log_den_out, void* stream) {
  CHECK(m, "null model");
  CHECK(T && Xs && cs && Xt && ct && wt, "null argument");
  TRY(bs_check(m, n_s, n_t));
  const int C = m->C, d = m->d;
  std::vector<int> cs32, ct32;
  TRY(bs_to_classes(cs, n_s, C, cs32, "sources"));
  TRY(bs_to_classes(ct, n_t, C, ct32, "targets"));
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  // the call's own buffers and scratch, released when it has waited for its launches
  BsScratch sc;
  DevBuf<double> dT, dXs, dXt, da, dwt, dws, dld;
  DevBuf<int> dcs, dct;
  TRY(dT.alloc((size_t)C * C));
  TRY(dXs.alloc((size_t)n_s * d));
  TRY(dXt.alloc((size_t)n_t * d));
  TRY(dwt.alloc((size_t)n_t));
  TRY(dws.alloc((size_t)n_s));
  TRY(dld.alloc((size_t)n_t));
  TRY(dcs.alloc((size_t)n_s));
  TRY(dct.alloc((size_t)n_t));
  if (a) TRY(da.alloc((size_t)n_s));
  auto launches = [&]() -> int {
    HIPCHK(hipMemcpyAsync(dT, T, sizeof(double) * C * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dXs, Xs, sizeof(double) * n_s * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dXt, Xt, sizeof(double) * n_t * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dwt, wt, sizeof(double) * n_t, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcs, cs32.data(), sizeof(int) * n_s, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dct, ct32.data(), sizeof(int) * n_t, hipMemcpyHostToDevice, s));
    if (a) HIPCHK(hipMemcpyAsync(da, a, sizeof(double) * n_s, hipMemcpyHostToDevice, s));
    TRY(bs_step(m, sc, dT, n_s, dXs, dcs, da, n_t, dXt, dct, dwt, dws, dld, s));
    if (ws_out) HIPCHK(hipMemcpyAsync(ws_out, dws, sizeof(double) * n_s, hipMemcpyDeviceToHost, s));
    if (log_den_out) HIPCHK(hipMemcpyAsync(log_den_out, dld, sizeof(double) * n_t, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  const int rc = launches();
  const hipError_t waited = hipStreamSynchronize(s);   // (also after a failure: the buffers go with the call)
  TRY(rc);
  HIPCHK(waited);
  HIPCHK(m->note_use(s));
  return GPMDM_OK;
}

int gpmdm_pf_smoothed_marginal(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_marginal_out* out,
                               void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "marginal smoothing serves single filters, not banks");
  CHECK(pf->n_ranks == 1, "marginal smoothing serves filters on one rank");
  CHECK(pf->sm_L > 0, "smoothing is off (gpmdm_pf_set_smoothing)");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the smoother's)
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "smoothed_marginal between switch and resample");
  CHECK(lag_first >= 0 && lag_first <= lag_last, "lags: 0 <= lag_first <= lag_last");
  CHECK(lag_last <= pf->sm_depth, "lag_last is above the recorded depth (gpmdm_pf_smoothing_depth)");
  gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d;
  const long long P = pf->P;
  TRY(bs_check(m, P, P));
  static const gpmdm_marginal_out none{};
  const gpmdm_marginal_out& o = out ? *out : none;
  const int n = lag_last - lag_first + 1;
  const int W = C + d + 3;
  const size_t stage = o.weights ? sizeof(double) * (size_t)n * P : 0;
  CHECK(stage + bs_record_bytes(C, d, P) <= kSmoothBytes,
        "these lags need more than 1 GiB of device staging (rows of P weights per lag): ask for fewer lags per call");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  TRY(pf->bs_out.reserve((size_t)n * W, s));
  TRY(pf->bs_w[0].grow((size_t)P, s));
  TRY(pf->bs_w[1].grow((size_t)P, s));
  if (o.weights) TRY(pf->bs_stage.grow((size_t)n * P, s));
  TRY(pf->bs.hist.grow((size_t)P, s));
  TRY(pf->bs.mult.grow((size_t)P, s));
  const int ns = pf->sm_L + 1;
  auto slot_of = [&](int lag) { return (size_t)((pf->sm_slot() - lag % ns + ns) % ns) * (size_t)P; };
  // the weights of lag l: its row of the staging when the caller wants it, else a ping-pong half
  auto w_of = [&](int lag) -> double* {
    return o.weights && lag >= lag_first ? pf->bs_stage + (size_t)(lag - lag_first) * P : pf->bs_w[lag & 1].p;
  };
  auto launches = [&]() -> int {
    // the record of the latest frame, if it ran on another stream
    if (pf->sm_pending && pf->sm_stream != s) HIPCHK(pf->sm_ev.block(s));
    launch_bs_fill(w_of(0), P, 1.0 / (double)P, s);
    for (int l = 0; l <= lag_last; ++l) {
      const size_t k = slot_of(l);
      if (l >= lag_first) {
        const bool anc = l < pf->sm_depth || pf->sm_root_anc;
        if (anc) launch_bs_mult(pf->sm_anc + k, P, pf->bs.hist, pf->bs.mult, s);
        BsReduceArgs ra{};
        ra.P = P;
        ra.C = C;
        ra.d = d;
        ra.w = w_of(l);
        ra.X = pf->sm_X + k * d;
        ra.cls = pf->sm_cls + k;
        ra.mult = anc ? pf->bs.mult.p : nullptr;
        ra.out = pf->bs_out.dev + (size_t)(l - lag_first) * W;
        launch_bs_reduce(ra, s);
      }
      if (l < lag_last) {
        const size_t ks = slot_of(l + 1);
        TRY(bs_step(m, pf->bs, pf->T, P, pf->sm_X + ks * d, pf->sm_cls + ks, nullptr, P, pf->sm_X + k * d,
                    pf->sm_cls + k, w_of(l), w_of(l + 1), nullptr, s));
      }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->bs_out.pin, pf->bs_out.dev, sizeof(double) * n * W, hipMemcpyDeviceToHost, s));
    if (o.weights) HIPCHK(hipMemcpyAsync(o.weights, pf->bs_stage, sizeof(double) * n * P, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  const int rc = launches();
  TRY(pf->bs_out.finish(rc, s));          // (quiesce waits for the launches if the wait fails)
  if (pf->sm_pending && pf->sm_stream == s) pf->sm_pending = false;   // (the record preceded the launches on s)
  for (int r = 0; r < n; ++r) {
    const double* row = pf->bs_out.pin + (size_t)r * W;
    if (o.class_prob) std::memcpy(o.class_prob + (size_t)r * C, row, sizeof(double) * C);
    if (o.state_mean) std::memcpy(o.state_mean + (size_t)r * d, row + C, sizeof(double) * d);
    if (o.mass) o.mass[r] = row[C + d];
    if (o.ess) o.ess[r] = row[C + d + 1];
    if (o.ess_distinct) o.ess_distinct[r] = row[C + d + 2];
  }
  return GPMDM_OK;
}

}  // extern "C"
