// C ABI, MAP trajectory decoding (gpmdm_map_step, gpmdm_pf_map_path): one implementation of the
// step (mp_step: the sources' records from gpmdm_predict_dyn's launch builder for every class
// with the scores as log-domain addend, the targets' grouping, the max pass and its finish, all
// queued on the caller's stream), applied to the caller's arrays as they are by the first entry
// point and to the leaders of the ancestry ring's slots (capi_smooth.hip; the plane sm_ll of
// gpmdm_pf_set_map) by the second, which ends with the backtrack, one copy-out and one wait.
// Kernels: mappath.h.
#include "capi_internal.h"
#include "mappath.h"

namespace gpmdm::capi {

constexpr long long kMpMaxPairs = 1ll << 36;

static size_t mp_record_bytes(int C, int d, long long n_s) {
  return sizeof(double) * (size_t)C * (size_t)n_s * (size_t)(2 * d + 1);
}

// The step's refusals, decided before any launch (gpmdm_backward_step's).
static int mp_check(const gpmdm_model* m, long long n_s, long long n_t) {
  CHECK(n_s >= 1 && n_t >= 1 && n_s < (1ll << 31) && n_t < (1ll << 31), "map step: n_s and n_t must be in [1, 2^31)");
  CHECK(n_s <= kMpMaxPairs / n_t, "map step: more than 2^36 source-target pairs (P > 262144)");
  CHECK(mp_record_bytes(m->C, m->d, n_s) <= kSmoothBytes,
        "map step: the sources' moments need more than 1 GiB of device staging (C x n_s x (2 d + 1) doubles)");
  return GPMDM_OK;
}

// One step on device arrays, queued on s: n_s sources (rows of Xs, cs; delta: nullptr for zeros)
// and n_t targets (ll: nullptr for zeros) at most, the real counts at ns_dev / nt_dev when set;
// shape_n: the row count that picks the dynamics image (the whole slot's).  src_rows: what psi
// names for source row r (nullptr: r).  Sizes checked by the caller (mp_check).
static int mp_step(const gpmdm_model* m, MpScratch& sc, const double* T, long long n_s, const int* ns_dev,
                   const double* Xs, const int* cs, const double* delta, const int* src_rows, long long n_t,
                   const int* nt_dev, const double* Xt, const int* ct, const double* ll, long long shape_n,
                   double* delta_out, int* psi_out, hipStream_t s) {
  const int C = m->C, d = m->d;
  const int split = bs_split(n_t, n_s);
  size_t nq = 0;
  for (int c = 0; c < C; ++c) nq = std::max(nq, predict_dyn_scratch(m, c, n_s, shape_n));
  TRY(sc.rec.grow((size_t)C * n_s * (2 * d + 1), s));
  TRY(sc.mu.grow((size_t)n_s * d, s));
  TRY(sc.var.grow((size_t)n_s * d, s));
  TRY(sc.q.grow(nq, s));
  TRY(sc.perm.grow((size_t)n_t, s));
  TRY(sc.tab.grow((size_t)2 * kMaxClasses + 2, s));
  TRY(sc.val.grow((size_t)split * n_t, s));
  TRY(sc.idx.grow((size_t)split * n_t, s));
  for (int c = 0; c < C; ++c) {
    launch_predict_dyn(m, c, Xs, n_s, sc.mu, sc.var, sc.q, s, shape_n, ns_dev);
    MpMomentArgs ma{};
    ma.n = n_s;
    ma.n_dev = ns_dev;
    ma.C = C;
    ma.d = d;
    ma.c = c;
    ma.mu = sc.mu;
    ma.var = sc.var;
    ma.cls = cs;
    ma.delta = delta;
    ma.T = T;
    ma.rec = sc.rec;
    launch_mp_moments(ma, s);
  }
  BsGroupArgs ga{};
  ga.n = n_t;
  ga.n_dev = nt_dev;
  ga.C = C;
  ga.cls = ct;
  ga.perm = sc.perm;
  ga.tab = sc.tab;
  launch_bs_group(ga, s);
  MpMaxArgs xa{};
  xa.n_s = n_s;
  xa.n_t = n_t;
  xa.ns_dev = ns_dev;
  xa.C = C;
  xa.d = d;
  xa.split = split;
  xa.rec = sc.rec;
  xa.Xt = Xt;
  xa.perm = sc.perm;
  xa.tab = sc.tab;
  xa.val = sc.val;
  xa.idx = sc.idx;
  launch_mp_max(xa, s);
  MpFinArgs fa{};
  fa.n_t = n_t;
  fa.nt_dev = nt_dev;
  fa.split = split;
  fa.val = sc.val;
  fa.idx = sc.idx;
  fa.perm = sc.perm;
  fa.ll = ll;
  fa.src_rows = src_rows;
  fa.delta = delta_out;
  fa.psi = psi_out;
  launch_mp_fin(fa, s);
  HIPCHK(hipGetLastError());
  return GPMDM_OK;
}

static int mp_classes(const int64_t* src, long long n, int C, std::vector<int>& dst, const char* what) {
  dst.resize((size_t)n);
  for (long long i = 0; i < n; ++i) {
    CHECK(src[i] >= 0 && src[i] < C, std::string("map step: a class of the ") + what + " is outside [0, C)");
    dst[(size_t)i] = (int)src[i];
  }
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_map_step(gpmdm_model_t m, const double* T, int64_t n_s, const double* Xs, const int64_t* cs,
                   const double* delta_s, int64_t n_t, const double* Xt, const int64_t* ct, const double* ll_t,
                   double* delta_out, int64_t* psi_out, void* stream) {
  CHECK(m, "null model");
  CHECK(T && Xs && cs && Xt && ct, "null argument");
  TRY(mp_check(m, n_s, n_t));
  const int C = m->C, d = m->d;
  std::vector<int> cs32, ct32, psi32;
  TRY(mp_classes(cs, n_s, C, cs32, "sources"));
  TRY(mp_classes(ct, n_t, C, ct32, "targets"));
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  // the call's own buffers and scratch, released when it has waited for its launches
  MpScratch sc;
  DevBuf<double> dT, dXs, dXt, dds, dll, dout;
  DevBuf<int> dcs, dct, dpsi;
  TRY(dT.alloc((size_t)C * C));
  TRY(dXs.alloc((size_t)n_s * d));
  TRY(dXt.alloc((size_t)n_t * d));
  TRY(dout.alloc((size_t)n_t));
  TRY(dpsi.alloc((size_t)n_t));
  TRY(dcs.alloc((size_t)n_s));
  TRY(dct.alloc((size_t)n_t));
  if (delta_s) TRY(dds.alloc((size_t)n_s));
  if (ll_t) TRY(dll.alloc((size_t)n_t));
  if (psi_out) psi32.resize((size_t)n_t);
  auto launches = [&]() -> int {
    HIPCHK(hipMemcpyAsync(dT, T, sizeof(double) * C * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dXs, Xs, sizeof(double) * n_s * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dXt, Xt, sizeof(double) * n_t * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcs, cs32.data(), sizeof(int) * n_s, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dct, ct32.data(), sizeof(int) * n_t, hipMemcpyHostToDevice, s));
    if (delta_s) HIPCHK(hipMemcpyAsync(dds, delta_s, sizeof(double) * n_s, hipMemcpyHostToDevice, s));
    if (ll_t) HIPCHK(hipMemcpyAsync(dll, ll_t, sizeof(double) * n_t, hipMemcpyHostToDevice, s));
    TRY(mp_step(m, sc, dT, n_s, nullptr, dXs, dcs, delta_s ? dds.p : nullptr, nullptr, n_t, nullptr, dXt, dct,
                ll_t ? dll.p : nullptr, n_s, dout, dpsi, s));
    if (delta_out) HIPCHK(hipMemcpyAsync(delta_out, dout, sizeof(double) * n_t, hipMemcpyDeviceToHost, s));
    if (psi_out) HIPCHK(hipMemcpyAsync(psi32.data(), dpsi, sizeof(int) * n_t, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  const int rc = launches();
  const hipError_t waited = hipStreamSynchronize(s);   // (also after a failure: the buffers go with the call)
  TRY(rc);
  HIPCHK(waited);
  HIPCHK(m->note_use(s));
  for (size_t j = 0; j < psi32.size(); ++j) psi_out[j] = psi32[j];
  return GPMDM_OK;
}

int gpmdm_pf_map_path(gpmdm_pf_t pf, int lag, const gpmdm_map_out* out, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "MAP decoding serves single filters, not banks");
  CHECK(pf->n_ranks == 1, "MAP decoding serves filters on one rank");
  CHECK(pf->sm_L > 0, "smoothing is off (gpmdm_pf_set_smoothing)");
  CHECK(pf->sm_map, "map recording is off (gpmdm_pf_set_map)");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  // (a pending pre-switch reads the cloud and writes the step's tables: neither is the decoder's)
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "map_path between switch and resample");
  CHECK(lag >= 1 && lag <= pf->sm_depth, "lag must be in [1, the recorded depth] (gpmdm_pf_smoothing_depth)");
  gpmdm_model* m = pf->m;
  const int C = m->C, d = m->d;
  const long long P = pf->P;
  TRY(mp_check(m, P, P));
  static const gpmdm_map_out none{};
  const gpmdm_map_out& o = out ? *out : none;
  const int n = lag + 1;
  const int W = d + 4;
  // the scores and back-pointers of every lag by particle, and the records
  const size_t stage = sizeof(double) * (size_t)n * P + sizeof(int) * (size_t)lag * P;
  CHECK(stage + mp_record_bytes(C, d, P) <= kSmoothBytes,
        "this window needs more than 1 GiB of device staging (rows of P scores and back-pointers per lag): ask "
        "for a shorter window");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  MpScratch& sc = pf->mp;
  TRY(pf->mp_out.reserve((size_t)n * W + 1, s));
  TRY(sc.delta.grow((size_t)n * P, s));
  TRY(sc.psi.grow((size_t)lag * P, s));
  TRY(sc.count.grow((size_t)n, s));
  TRY(sc.owner.grow((size_t)P, s));
  TRY(sc.rank.grow((size_t)P, s));
  TRY(sc.psi_c.grow((size_t)P, s));
  TRY(sc.Xs.grow((size_t)P * d, s));
  TRY(sc.Xt.grow((size_t)P * d, s));
  TRY(sc.llt.grow((size_t)P, s));
  TRY(sc.cs.grow((size_t)P, s));
  TRY(sc.ct.grow((size_t)P, s));
  for (int h = 0; h < 2; ++h) {
    TRY(sc.rows[h].grow((size_t)P, s));
    TRY(sc.lead[h].grow((size_t)P, s));
    TRY(sc.dc[h].grow((size_t)P, s));
  }
  const int ns = pf->sm_L + 1;
  auto slot_of = [&](int l) { return (size_t)((pf->sm_slot() - l % ns + ns) % ns) * (size_t)P; };
  std::vector<int> psi32, cnt32;
  // slot l's leaders into half l & 1
  auto leaders = [&](int l) {
    MpLeadArgs la{};
    la.P = P;
    la.anc = pf->sm_anc + slot_of(l);
    la.owner = sc.owner;
    la.rank = sc.rank;
    la.rows = sc.rows[l & 1];
    la.lead = sc.lead[l & 1];
    la.count = sc.count + l;
    launch_mp_leaders(la, l < pf->sm_depth || pf->sm_root_anc, s);
  };
  auto gather = [&](int l, double* X, int* cls, double* ll) {
    const size_t k = slot_of(l);
    MpGatherArgs ga{};
    ga.n = P;
    ga.d = d;
    ga.n_dev = sc.count + l;
    ga.rows = sc.rows[l & 1];
    ga.X = pf->sm_X + k * d;
    ga.cls = pf->sm_cls + k;
    ga.ll = ll ? pf->sm_ll + k : nullptr;
    ga.X_out = X;
    ga.cls_out = cls;
    ga.ll_out = ll;
    launch_mp_gather(ga, s);
  };
  auto expand = [&](int l) {
    MpExpandArgs ea{};
    ea.P = P;
    ea.lead = sc.lead[l & 1];
    ea.delta_c = sc.dc[l & 1];
    ea.psi_c = l < lag ? sc.psi_c.p : nullptr;
    ea.delta = sc.delta + (size_t)l * P;
    ea.psi = l < lag ? sc.psi + (size_t)l * P : nullptr;
    launch_mp_expand(ea, s);
  };
  auto launches = [&]() -> int {
    // the record of the latest frame, if it ran on another stream
    if (pf->sm_pending && pf->sm_stream != s) HIPCHK(pf->sm_ev.block(s));
    leaders(lag);
    launch_bs_fill(sc.dc[lag & 1], P, 0.0, s);          // the root cloud: flat over its support
    expand(lag);
    for (int l = lag - 1; l >= 0; --l) {
      leaders(l);
      gather(l + 1, sc.Xs, sc.cs, nullptr);
      gather(l, sc.Xt, sc.ct, sc.llt);
      TRY(mp_step(m, sc, pf->T, P, sc.count + l + 1, sc.Xs, sc.cs, sc.dc[(l + 1) & 1], sc.rows[(l + 1) & 1], P,
                  sc.count + l, sc.Xt, sc.ct, sc.llt, P, sc.dc[l & 1], sc.psi_c, s));
      expand(l);
    }
    MpBackArgs ba{};
    ba.P = P;
    ba.d = d;
    ba.lag = lag;
    ba.n_slots = ns;
    ba.slot = pf->sm_slot();
    ba.ring_X = pf->sm_X;
    ba.ring_cls = pf->sm_cls;
    ba.delta = sc.delta;
    ba.psi = sc.psi;
    ba.count = sc.count;
    ba.out = pf->mp_out.dev;
    launch_mp_back(ba, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->mp_out.pin, pf->mp_out.dev, sizeof(double) * ((size_t)n * W + 1), hipMemcpyDeviceToHost, s));
    if (o.delta) HIPCHK(hipMemcpyAsync(o.delta, sc.delta, sizeof(double) * n * P, hipMemcpyDeviceToHost, s));
    if (o.backpointer) {
      psi32.resize((size_t)lag * P);
      HIPCHK(hipMemcpyAsync(psi32.data(), sc.psi, sizeof(int) * psi32.size(), hipMemcpyDeviceToHost, s));
    }
    return GPMDM_OK;
  };
  const int rc = launches();
  TRY(pf->mp_out.finish(rc, s));          // (quiesce waits for the launches if the wait fails)
  if (pf->sm_pending && pf->sm_stream == s) pf->sm_pending = false;   // (the record preceded the launches on s)
  const double* pin = pf->mp_out.pin;
  for (int l = 0; l < n; ++l) {
    const double* row = pin + (size_t)l * W;
    if (o.index) o.index[l] = (int64_t)row[0];
    if (o.classes) o.classes[l] = (int64_t)row[1];
    if (o.score) o.score[l] = row[2];
    if (o.distinct) o.distinct[l] = (int64_t)row[3];
    if (o.states) std::memcpy(o.states + (size_t)l * d, row + 4, sizeof(double) * d);
  }
  if (o.log_joint) *o.log_joint = pin[(size_t)n * W];
  for (size_t i = 0; i < psi32.size(); ++i) o.backpointer[i] = psi32[i];
  return GPMDM_OK;
}

}  // extern "C"
