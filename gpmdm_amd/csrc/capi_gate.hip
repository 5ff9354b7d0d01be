// C ABI, outlier gating inside the frame (gpmdm_pf_set_gate, gpmdm_pf_gate_report and the banks'
// gpmdm_bank_set_gate, gpmdm_bank_gate_report): the switch, the launches a gated-mode weigh ends
// with (gate_frame: the innovation tile and its finish over X_prop, vc_prop, the staged z and the
// mask snapshot, then the decision, the re-weigh tile and its finish -- each once for all the
// handle's filters, all on the frame's stream, none waited for), and the report's copy of the
// device tables.  A single filter is the bank of F = 1.  Kernels: obs_gate.h.
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

// thresholds: F (the caller has refused NaN)
static int set_gate(gpmdm_pf* pf, const double* thresholds, double limit) {
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_gate between switch and resample");
  const int F = pf->F;
  int n_on = 0;
  for (int f = 0; f < F; ++f) n_on += thresholds[f] > 0.0 ? 1 : 0;
  if (n_on == 0) {
    pf->gate_k = 0.0;
    pf->gate_ks.clear();
    pf->gt_ready = false;
    return GPMDM_OK;
  }
  CHECK(n_on == F, "set_gate: the thresholds must be all > 0 (+inf: that filter never rejects) or all <= 0 (off)");
  CHECK(limit > 0.0 && limit <= 1.0, "set_gate: the limit must be in (0, 1]");   // (false for NaN)
  CHECK(pf->n_ranks == 1, "gating does not serve sharded filters (only ll is exchanged between ranks)");
  if (!pf->predictive) return fail(GPMDM_E_STATE, "set_gate: the predictive switch is off (gpmdm_pf_set_predictive)");
  HIPCHK(hipSetDevice(pf->m->device));
  pf->gt_ready = false;
  const int D = pf->m->D;
  const size_t n_tab = (size_t)F * gate_tab_doubles(D);
  if (!pf->gt_tab) TRY(pf->gt_tab.alloc(n_tab));
  if (!pf->gt_out) TRY(pf->gt_out.alloc(innov_out_doubles(D, F)));
  if (!pf->gt_cfg) TRY(pf->gt_cfg.alloc((size_t)F * kGateCfg));
  if (!pf->gt_pin) TRY(pf->gt_pin.alloc(n_tab));
  const double was = pf->gate_k;
  pf->gate_k = thresholds[0];
  const int rc = gate_rebind(pf);
  if (rc != GPMDM_OK) {
    pf->gate_k = was;
    return rc;
  }
  pf->gate_ks.assign(thresholds, thresholds + F);
  pf->gate_limit = limit;
  return GPMDM_OK;
}

// The decision's {threshold, cap} rows for this frame; uploaded only when they differ from what
// the device holds.
static int gate_config(gpmdm_pf* pf) {
  const int D = pf->m->D, F = pf->F;
  std::vector<double> cfg((size_t)F * kGateCfg);
  pf->gt_black.assign((size_t)F, 0);
  for (int f = 0; f < F; ++f) {
    int n_obs = D;
    if (pf->masked()) {
      const unsigned char* mf = pf->obs_mask.data() + (size_t)f * D;
      n_obs = 0;
      for (int j = 0; j < D; ++j) n_obs += mf[j] ? 1 : 0;
    }
    pf->gt_black[(size_t)f] = n_obs == 0;
    cfg[(size_t)f * kGateCfg] = pf->gate_ks[(size_t)f];
    // the cap on the host, in fp64, from the frame's observed dimensions
    cfg[(size_t)f * kGateCfg + 1] = std::floor(pf->gate_limit * (double)n_obs);
  }
  if (cfg == pf->gt_cfg_host) return GPMDM_OK;
  // the last frame's decision may still read the table: it precedes the frame's read-out
  HIPCHK(pf->zslot_free());
  pf->gt_cfg_host.clear();
  TRY(h2d(pf->gt_cfg, cfg.data(), sizeof(double) * cfg.size()));
  pf->gt_cfg_host.swap(cfg);
  return GPMDM_OK;
}

int gate_frame(gpmdm_pf* pf, hipStream_t s) {
  gpmdm_model* m = pf->m;
  const int D = m->D, F = pf->F;
  const long long Pf = pf->Pf;
  pf->gt_host = !pf->pv_has_vc;        // a blackout frame (of every filter): nothing exceeded, ll stays exactly 0
  pf->gt_ready = true;
  if (pf->gt_host) return GPMDM_OK;
  TRY(gate_config(pf));                // (a blacked-out filter of a bank: cap 0, nothing observed, its ll stays 0)
  TRY(flush_ll(pf, s));                // a deferred finish has produced neither ll nor vc yet
  TRY(pf->gt_part.grow(innov_part_doubles(Pf, D, F), s));
  TRY(pf->gt_sp.grow((size_t)F * readout_groups(D) * (size_t)Pf, s));
  InnovParams ip{};
  ip.ro = pose_readout(pf, pf->X_prop, nullptr, nullptr);
  ip.vc = pf->vc_prop;
  ip.z = pf->pv_z;
  ip.mask = pf->pv_masked ? pf->pv_mask.dev : nullptr;
  ip.il2 = m->y_il2_dev;
  ip.lam2 = m->y_lam2_dev;
  ip.part = pf->gt_part;
  ip.vpart = pf->gt_part + (size_t)F * readout_tiles(Pf) * readout_groups(D) * kRoGC * kInnovPlanes;
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
  gp.cfg = pf->gt_cfg;
  gp.tab = pf->gt_tab;
  gp.Sp = pf->gt_sp;
  gp.ll = pf->ll;
  // (else -- and in every bank, whose finish writes no block maxima -- the normaliser takes the
  // maximum from ll itself)
  gp.bmax = pf->bmax_ready ? pf->bmax.p : nullptr;
  launch_gate(gp, s);
  HIPCHK(hipGetLastError());
  return GPMDM_OK;
}

// a frame (or a filter of it) with nothing observed: nothing exceeded, nothing used, n_valid = 0
static void blackout_row(const gpmdm_gate_out& o, int f, int D) {
  for (int j = 0; j < D; ++j) {
    const size_t k = (size_t)f * D + j;
    if (o.zscore) o.zscore[k] = std::nan("");
    if (o.exceeded) o.exceeded[k] = 0;
    if (o.gated) o.gated[k] = 0;
    if (o.used) o.used[k] = 0;
  }
  if (o.n_gated) o.n_gated[f] = 0;
  if (o.n_valid) o.n_valid[f] = 0;
  if (o.overflow) o.overflow[f] = 0;
}

static int gate_report(gpmdm_pf* pf, const gpmdm_gate_out* out, void* stream) {
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  CHECK(pf->gate_k > 0.0, "gate_report: the gate is off (gpmdm_pf_set_gate)");
  if (!pf->gt_ready) return fail(GPMDM_E_STATE, "gate_report: no frame weighed with the gate on");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D, F = pf->F;
  const gpmdm_gate_out& o = *out;
  if (pf->gt_host) {
    for (int f = 0; f < F; ++f) blackout_row(o, f, D);
    return GPMDM_OK;
  }
  if (!pf->propagated) HIPCHK(pf->zslot_free());   // the frame's launches, whatever stream they ran on
  const size_t n_row = gate_tab_doubles(D);
  HIPCHK(hipMemcpyAsync(pf->gt_pin, pf->gt_tab, sizeof(double) * F * n_row, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int f = 0; f < F; ++f) {
    if (pf->gt_black[(size_t)f]) {
      blackout_row(o, f, D);
      continue;
    }
    const double* t = pf->gt_pin + (size_t)f * n_row;
    const double* rows = t + kGateHead;
    const size_t r0 = (size_t)f * D;
    if (o.zscore) std::memcpy(o.zscore + r0, rows, sizeof(double) * D);
    for (int j = 0; j < D; ++j) {
      if (o.exceeded) o.exceeded[r0 + j] = rows[(size_t)D + j] != 0.0;
      if (o.gated) o.gated[r0 + j] = rows[2 * (size_t)D + j] != 0.0;
      if (o.used) o.used[r0 + j] = rows[3 * (size_t)D + j] != 0.0;
    }
    if (o.n_gated) o.n_gated[f] = (int64_t)t[kGateNGated];
    if (o.n_valid) o.n_valid[f] = (int64_t)t[kGateNValid];
    if (o.overflow) o.overflow[f] = t[kGateOverflow] != 0.0;
  }
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_pf_set_gate(gpmdm_pf_t pf, double threshold, double limit) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "gpmdm_pf_set_gate serves single filters, not banks");
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_gate between switch and resample");
  CHECK(std::isfinite(threshold), "set_gate: the threshold must be finite");
  return set_gate(pf, &threshold, limit);
}

int gpmdm_pf_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream) {
  CHECK(pf && out, "null argument");
  CHECK(pf->F == 1, "gpmdm_pf_gate_report serves single filters, not banks");
  return gate_report(pf, out, stream);
}

int gpmdm_bank_set_gate(gpmdm_pf_t pf, const double* thresholds, double limit) {
  CHECK(pf && thresholds, "null argument");
  CHECK(pf->F <= 65535, "bank gating serves up to 65535 filters");
  for (int f = 0; f < pf->F; ++f) CHECK(!std::isnan(thresholds[f]), "set_gate: a threshold is NaN");
  return set_gate(pf, thresholds, limit);
}

int gpmdm_bank_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream) {
  CHECK(pf && out, "null argument");
  CHECK(pf->F <= 65535, "bank gating serves up to 65535 filters");
  return gate_report(pf, out, stream);
}

}  // extern "C"
