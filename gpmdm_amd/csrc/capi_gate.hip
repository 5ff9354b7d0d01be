// C ABI, outlier gating inside the frame (gpmdm_pf_set_gate, gpmdm_pf_gate_report): the switch,
// the launches a gated-mode weigh ends with (gate_frame: the innovation tile and its finish over
// X_prop, vc_prop, the staged z and the mask snapshot, then the decision, the re-weigh tile and
// its finish -- all on the frame's stream, none waited for), and the report's copy of the device
// table.  Kernels: obs_gate.h.
#include "capi_internal.h"
#include "obs_gate.h"

namespace gpmdm::capi {

int gate_rebind(gpmdm_pf* pf) {
  if (!(pf->gate_k > 0.0)) return GPMDM_OK;
  const gpmdm_model* m = pf->m;
  const int D = m->D;
  // the last frame's finish may still read the table: it precedes the frame's read-out
  HIPCHK(pf->zslot_free());
  if (!pf->gt_lil) TRY(pf->gt_lil.alloc((size_t)D));
  std::vector<double> lil((size_t)D);
  for (int j = 0; j < D; ++j) lil[(size_t)j] = std::log(m->y_il2[(size_t)j]);   // capi_pf.hip install_obs_mask's terms
  return h2d(pf->gt_lil, lil.data(), sizeof(double) * D);
}

static int set_gate(gpmdm_pf* pf, double threshold, double limit) {
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_gate between switch and resample");
  CHECK(std::isfinite(threshold), "set_gate: the threshold must be finite");
  if (!(threshold > 0.0)) {
    pf->gate_k = 0.0;
    pf->gt_ready = false;
    return GPMDM_OK;
  }
  CHECK(limit > 0.0 && limit <= 1.0, "set_gate: the limit must be in (0, 1]");   // (false for NaN)
  CHECK(pf->n_ranks == 1, "gating does not serve sharded filters (only ll is exchanged between ranks)");
  if (!pf->predictive) return fail(GPMDM_E_STATE, "set_gate: the predictive switch is off (gpmdm_pf_set_predictive)");
  HIPCHK(hipSetDevice(pf->m->device));
  pf->gt_ready = false;
  const int D = pf->m->D;
  const size_t n_tab = gate_tab_doubles(D);
  if (!pf->gt_tab) TRY(pf->gt_tab.alloc(n_tab));
  if (!pf->gt_out) TRY(pf->gt_out.alloc(innov_out_doubles(D, 1)));
  if (!pf->gt_pin) TRY(pf->gt_pin.alloc(n_tab));
  const double was = pf->gate_k;
  pf->gate_k = threshold;
  const int rc = gate_rebind(pf);
  if (rc != GPMDM_OK) {
    pf->gate_k = was;
    return rc;
  }
  pf->gate_limit = limit;
  return GPMDM_OK;
}

int gate_frame(gpmdm_pf* pf, hipStream_t s) {
  gpmdm_model* m = pf->m;
  const int D = m->D;
  const long long P = pf->P;
  pf->gt_host = !pf->pv_has_vc;        // a blackout frame: nothing exceeded, ll stays exactly 0
  pf->gt_ready = true;
  if (pf->gt_host) return GPMDM_OK;
  TRY(flush_ll(pf, s));                // a deferred finish has produced neither ll nor vc yet
  TRY(pf->gt_part.grow(innov_part_doubles(P, D, 1), s));
  TRY(pf->gt_sp.grow((size_t)readout_groups(D) * (size_t)P, s));
  InnovParams ip{};
  ip.ro = pose_readout(pf, pf->X_prop, nullptr, nullptr);
  ip.vc = pf->vc_prop;
  ip.z = pf->pv_z;
  ip.mask = pf->pv_masked ? pf->pv_mask.dev : nullptr;
  ip.il2 = m->y_il2_dev;
  ip.lam2 = m->y_lam2_dev;
  ip.part = pf->gt_part;
  ip.vpart = pf->gt_part + (size_t)readout_tiles(P) * readout_groups(D) * kRoGC * kInnovPlanes;
  ip.out = pf->gt_out;
  launch_obs_innov(ip, s);
  GateParams gp{};
  gp.ro = ip.ro;
  gp.innov = pf->gt_out;
  gp.mask = ip.mask;
  gp.z = ip.z;
  gp.lam2 = m->y_lam2_dev;
  gp.log_il2 = pf->gt_lil;
  gp.vc = pf->vc_prop;
  gp.threshold = pf->gate_k;
  // the cap on the host, in fp64, from the frame's observed dimensions
  gp.cap = (int)std::floor(pf->gate_limit * (double)(pf->masked() ? pf->D_obs : D));
  gp.tab = pf->gt_tab;
  gp.Sp = pf->gt_sp;
  gp.ll = pf->ll;
  gp.bmax = pf->bmax_ready ? pf->bmax.p : nullptr;   // (else the normaliser takes the maximum from ll itself)
  launch_gate(gp, s);
  HIPCHK(hipGetLastError());
  return GPMDM_OK;
}

static int gate_report(gpmdm_pf* pf, const gpmdm_gate_out* out, void* stream) {
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  CHECK(pf->gate_k > 0.0, "gate_report: the gate is off (gpmdm_pf_set_gate)");
  if (!pf->gt_ready) return fail(GPMDM_E_STATE, "gate_report: no frame weighed with the gate on");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D;
  const gpmdm_gate_out& o = *out;
  if (pf->gt_host) {
    for (int j = 0; j < D; ++j) {
      if (o.zscore) o.zscore[j] = std::nan("");
      if (o.exceeded) o.exceeded[j] = 0;
      if (o.gated) o.gated[j] = 0;
      if (o.used) o.used[j] = 0;
    }
    if (o.n_gated) *o.n_gated = 0;
    if (o.n_valid) *o.n_valid = 0;
    if (o.overflow) *o.overflow = 0;
    return GPMDM_OK;
  }
  if (!pf->propagated) HIPCHK(pf->zslot_free());   // the frame's launches, whatever stream they ran on
  HIPCHK(hipMemcpyAsync(pf->gt_pin, pf->gt_tab, sizeof(double) * gate_tab_doubles(D), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const double* t = pf->gt_pin;
  const double* rows = t + kGateHead;
  if (o.zscore) std::memcpy(o.zscore, rows, sizeof(double) * D);
  for (int j = 0; j < D; ++j) {
    if (o.exceeded) o.exceeded[j] = rows[(size_t)D + j] != 0.0;
    if (o.gated) o.gated[j] = rows[2 * (size_t)D + j] != 0.0;
    if (o.used) o.used[j] = rows[3 * (size_t)D + j] != 0.0;
  }
  if (o.n_gated) *o.n_gated = (int64_t)t[kGateNGated];
  if (o.n_valid) *o.n_valid = (int64_t)t[kGateNValid];
  if (o.overflow) *o.overflow = t[kGateOverflow] != 0.0;
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_pf_set_gate(gpmdm_pf_t pf, double threshold, double limit) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "gpmdm_pf_set_gate serves single filters, not banks");
  return set_gate(pf, threshold, limit);
}

int gpmdm_pf_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream) {
  CHECK(pf && out, "null argument");
  CHECK(pf->F == 1, "gpmdm_pf_gate_report serves single filters, not banks");
  return gate_report(pf, out, stream);
}

}  // extern "C"
