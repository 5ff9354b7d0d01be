// C ABI, fixed-lag smoothing (gpmdm_pf_set_smoothing, gpmdm_pf_smoothing_depth,
// gpmdm_pf_smoothed and the banks' gpmdm_bank_set_smoothing, gpmdm_bank_smoothed): the ring of
// per-frame {ancestors, classes, states} that every resample of an enabled filter or bank records
// into, and the read-out that walks it -- a clear, the trace, the per-(lag, filter) reduce and
// per lag with a pose one read-out of obs_readout.h over the F traced clouds, all queued on the
// caller's stream, then one copy-back and one wait.  Every device result is lag-major, then
// filter-major.  Kernels: smooth.h.
#include "capi_internal.h"
#include "smooth.h"
#include "mappath.h"

namespace gpmdm::capi {

// (map: the log-likelihood plane of gpmdm_pf_set_map is counted too)
static size_t ring_bytes(long long P, int d, int L, bool map) {
  return (size_t)(L + 1) * (size_t)P * (sizeof(double) * (d + (map ? 1 : 0)) + 2 * sizeof(int));
}

int sm_wait(gpmdm_pf* pf) {
  if (pf->sm_pending) {
    HIPCHK(pf->sm_ev.sync());
    pf->sm_pending = false;
  }
  TRY(pf->bs_out.wait());
  TRY(pf->mp_out.wait());
  TRY(pf->fs_out.wait());
  return pf->sm_out.wait();
}

// root: a cleared ring's root (no resample behind it: its log-likelihoods are zeros)
static void launch_record(gpmdm_pf* pf, hipStream_t s, bool root = false) {
  const size_t k = (size_t)pf->sm_slot() * pf->P;
  // (ll is final here: the resample's launches finished it, gpmdm_pf_resample)
  if (pf->sm_map) launch_mp_ll_record(pf->ll, root ? nullptr : pf->ridx.p, pf->P, pf->sm_ll + k, s);
  SmRecordArgs a{};
  a.P = pf->P;
  a.d = pf->m->d;
  a.ridx = pf->ridx;
  a.cls = pf->cls;
  a.X = pf->X;
  a.anc_dst = pf->sm_anc + k;
  a.cls_dst = pf->sm_cls + k;
  a.X_dst = pf->sm_X + k * pf->m->d;
  launch_sm_record(a, s);
}

// The frame the resample on s has just completed (pf->frame counts it already).
int sm_record(gpmdm_pf* pf, hipStream_t s) {
  launch_record(pf, s);
  HIPCHK(hipGetLastError());
  // (a frame counter that wrapped starts a new history: slots follow the counter)
  if (pf->frame == 0 || pf->sm_depth == pf->sm_L) pf->sm_root_anc = true;   // the oldest slot in reach is a resample's
  pf->sm_depth = pf->frame == 0 ? 0 : std::min(pf->sm_L, pf->sm_depth + 1);
  HIPCHK(pf->sm_ev.record(s));
  pf->sm_pending = true;
  pf->sm_stream = s;
  return GPMDM_OK;
}

// Forget the history; the cloud the filter holds now is its root (no ancestors).  The caller
// has waited for the filter's launches (quiesce, or sm_wait and the last read-out); s: the
// lifecycle stream, synchronised here.
int sm_clear(gpmdm_pf* pf, hipStream_t s) {
  pf->sm_depth = 0;
  pf->sm_root_anc = false;
  if (pf->sm_L == 0 || !pf->initialised) return GPMDM_OK;
  launch_record(pf, s, true);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  return GPMDM_OK;
}

// gpmdm_pf_set_smoothing / gpmdm_bank_set_smoothing on a checked handle (P: all F x Pf particles)
int sm_set(gpmdm_pf* pf, int lag) {
  CHECK(lag >= 0 && lag <= GPMDM_SMOOTH_MAX_LAG, "lag must be in [0, GPMDM_SMOOTH_MAX_LAG]");
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_smoothing between switch and resample");
  gpmdm_model* m = pf->m;
  CHECK(lag == 0 || ring_bytes(pf->P, m->d, lag, pf->sm_map) <= kSmoothBytes,
        "the history of this lag needs more than 1 GiB of device memory ((lag + 1) x P x (d + 1) doubles; one more "
        "per particle with map recording on)");
  HIPCHK(hipSetDevice(m->device));
  // a record or a read-out in flight, and the last frame's resample (it precedes the frame's
  // read-out; a pending pre-switch reads the cloud only, and stays pending)
  TRY(sm_wait(pf));
  HIPCHK(pf->zslot_free());
  auto drop_ring = [&] {
    pf->sm_anc.release();
    pf->sm_cls.release();
    pf->sm_X.release();
    pf->sm_ll.release();
  };
  drop_ring();
  pf->sm_L = pf->sm_depth = 0;
  if (lag == 0) return GPMDM_OK;
  const size_t n = (size_t)(lag + 1) * pf->P;
  if (pf->sm_anc.alloc(n) || pf->sm_cls.alloc(n) || pf->sm_X.alloc(n * m->d) || (pf->sm_map && pf->sm_ll.alloc(n))) {
    drop_ring();
    return GPMDM_E_NOMEM;
  }
  pf->sm_L = lag;
  hipStream_t ls = life_stream(m->device);
  CHECK(ls, "the library's lifecycle stream");
  return sm_clear(pf, ls);
}

// gpmdm_pf_smoothed / gpmdm_bank_smoothed on a checked handle with smoothing on.  stage_refusal:
// the entry point's wording of the 1 GiB staging limit.
static int smoothed(gpmdm_pf* pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out, void* stream,
                    const char* stage_refusal) {
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the smoother's)
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "smoothed between switch and resample");
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
  CHECK(stage <= kSmoothBytes, stage_refusal);
  TRY(pf->sm_marks.grow(cnt_bytes + n_rows * ldm, s));
  TRY(pf->sm_part.grow(n_rows * nbf * d, s));
  const size_t n_out = n_rows * W + n_rows * 2 * D;   // the rows, then {mean[D], spread[D]} of every row
  TRY(pf->sm_out.reserve(n_out, s));
  if (obs) TRY(pf->sm_ro_part.grow(readout_part_doubles(Pf, D, F), s));
  // per-call staging of the particle rows, released in the stream's order on every exit
  DevBuf<double> stage_X;
  DevBuf<int> stage_anc, stage_cls;
  int rc = GPMDM_OK;
  if (want_X) rc = stage_X.alloc((size_t)n * P * d);
  if (rc == GPMDM_OK && o.ancestors) rc = stage_anc.alloc((size_t)n * P);
  if (rc == GPMDM_OK && o.classes) rc = stage_cls.alloc((size_t)n * P);
  std::vector<int> a32, c32;
  double* out_ro = pf->sm_out.dev + n_rows * W;
  auto launches = [&]() -> int {
    // the record of the latest frame, if it ran on another stream
    if (pf->sm_pending && pf->sm_stream != s) HIPCHK(pf->sm_ev.block(s));
    int* counts = reinterpret_cast<int*>(pf->sm_marks.p);
    unsigned char* marks = pf->sm_marks + cnt_bytes;
    HIPCHK(hipMemsetAsync(pf->sm_marks, 0, cnt_bytes + n_rows * ldm, s));
    SmTraceArgs ta{};
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
    launch_sm_trace(ta, s);
    SmReduceArgs ra{};
    ra.Pf = Pf;
    ra.C = C;
    ra.d = d;
    ra.nbf = (int)nbf;
    ra.counts = counts;
    ra.partials = pf->sm_part;
    ra.marks = marks;
    ra.ld_marks = ldm;
    ra.out = pf->sm_out.dev;
    ra.ld_out = W;
    launch_sm_reduce(ra, n, F, s);
    for (int r = 0; obs && r < n; ++r)   // each lag's pose: one read-out over the F traced clouds
      launch_obs_readout(pose_readout(pf, stage_X + (size_t)r * P * d, pf->sm_ro_part, out_ro + (size_t)r * F * 2 * D), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->sm_out.pin, pf->sm_out.dev, sizeof(double) * (obs ? n_out : n_rows * W), hipMemcpyDeviceToHost, s));
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
  stage_X.release_after(s);
  stage_anc.release_after(s);
  stage_cls.release_after(s);
  TRY(pf->sm_out.finish(rc, s));         // (quiesce waits for the launches if the wait fails)
  if (pf->sm_pending && pf->sm_stream == s) pf->sm_pending = false;   // (the record preceded the trace on s)
  const double* ro = pf->sm_out.pin + n_rows * W;
  for (size_t q = 0; q < n_rows; ++q) {
    const double* row = pf->sm_out.pin + q * W;
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

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_pf_set_smoothing(gpmdm_pf_t pf, int lag) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "smoothing serves single filters, not banks (gpmdm_bank_set_smoothing)");
  return sm_set(pf, lag);
}

int gpmdm_bank_set_smoothing(gpmdm_pf_t pf, int lag) {
  CHECK(pf, "null handle");
  return sm_set(pf, lag);
}

int gpmdm_pf_set_map(gpmdm_pf_t pf, int on) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "map recording serves single filters, not banks");
  CHECK(pf->n_ranks == 1, "map recording serves filters on one rank");
  CHECK(!on || pf->sm_L > 0, "map recording needs smoothing on (gpmdm_pf_set_smoothing)");
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_map between switch and resample");
  gpmdm_model* m = pf->m;
  CHECK(!on || ring_bytes(pf->P, m->d, pf->sm_L, true) <= kSmoothBytes,
        "the history with the log-likelihood plane needs more than 1 GiB of device memory ((lag + 1) x P x (d + 2) "
        "doubles)");
  HIPCHK(hipSetDevice(m->device));
  TRY(sm_wait(pf));                    // (as sm_set: a record or a read-out in flight, the last frame)
  HIPCHK(pf->zslot_free());
  pf->sm_ll.release();
  pf->sm_map = false;
  if (!on) return GPMDM_OK;            // (the rest of the history stays)
  if (pf->sm_ll.alloc((size_t)(pf->sm_L + 1) * pf->P)) return GPMDM_E_NOMEM;
  pf->sm_map = true;
  hipStream_t ls = life_stream(m->device);
  CHECK(ls, "the library's lifecycle stream");
  return sm_clear(pf, ls);
}

int gpmdm_pf_map_recording(gpmdm_pf_t pf, int* on) {
  CHECK(pf, "null handle");
  if (on) *on = pf->sm_map ? 1 : 0;
  return GPMDM_OK;
}

int gpmdm_pf_smoothing_depth(gpmdm_pf_t pf, int* lag, int* depth) {
  CHECK(pf, "null handle");
  if (lag) *lag = pf->sm_L;
  if (depth) *depth = pf->sm_depth;
  return GPMDM_OK;
}

int gpmdm_pf_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "smoothing serves single filters, not banks (gpmdm_bank_smoothed)");
  CHECK(pf->sm_L > 0, "smoothing is off (gpmdm_pf_set_smoothing)");
  return smoothed(pf, lag_first, lag_last, out, stream,
                  "these lags need more than 1 GiB of device staging (rows of P states, ancestors, classes and "
                  "marks per lag): ask for fewer lags per call");
}

int gpmdm_bank_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F <= 65535, "bank smoothing serves up to 65535 filters");
  CHECK(pf->sm_L > 0, "smoothing is off (gpmdm_bank_set_smoothing)");
  return smoothed(pf, lag_first, lag_last, out, stream,
                  "these lags need more than 1 GiB of device staging (rows of F x P states, ancestors, classes and "
                  "marks per lag): ask for fewer lags per call");
}

}  // extern "C"
