// C ABI, innovations and the GP's predictive variance (gpmdm_pf_set_predictive,
// gpmdm_pf_innovation, gpmdm_pf_observation_gp and the banks'): the switch that makes every weigh
// keep vc (capi_frame.hip weigh: ObsFinishArgs::vc_out), and the two read-outs over what the
// frame left on the device -- the innovation tile and its finish over X_prop, vc_prop and the
// staged z, or the gather of vc_prop through the resample's ancestors -- queued on the caller's
// stream, then one pinned copy and one wait.  Kernels: obs_innov.h.
#include "capi_internal.h"
#include "obs_innov.h"

namespace gpmdm::capi {

int iv_wait(gpmdm_pf* pf) {
  return pf->iv_out.wait();
}

static int set_predictive(gpmdm_pf* pf, int on) {
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_predictive between switch and resample");
  if (!on && pf->gate_k > 0.0) return fail(GPMDM_E_STATE, "set_predictive(0) while the gate is on (gpmdm_pf_set_gate)");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  // the last frame's finish may still write vc_prop: it precedes the frame's read-out (a
  // pending pre-switch touches none of this, and stays pending)
  TRY(iv_wait(pf));
  HIPCHK(pf->zslot_free());
  pf->pv_clear();
  pf->predictive = false;
  if (!on) {
    pf->vc_prop.release();
    return GPMDM_OK;
  }
  if (!pf->vc_prop) TRY(pf->vc_prop.alloc((size_t)pf->P));
  if (!pf->pv_mask) TRY(pf->pv_mask.alloc_mapped((size_t)pf->F * m->D));
  pf->predictive = true;
  return GPMDM_OK;
}

// the checks both read-outs share; s: the caller's stream
static int readable(gpmdm_pf* pf, const char* what) {
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  CHECK(pf->predictive, std::string(what) + ": the predictive switch is off (gpmdm_pf_set_predictive)");
  CHECK(pf->n_ranks == 1, std::string(what) + " does not serve sharded filters (only ll is exchanged between ranks)");
  return GPMDM_OK;
}

static int innovation(gpmdm_pf* pf, const gpmdm_innovation_out* out, void* stream) {
  TRY(readable(pf, "innovation"));
  if (!pf->pv_weighed) return fail(GPMDM_E_STATE, "innovation: no frame weighed with the predictive switch on");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int d = m->d, D = m->D, F = pf->F;
  const long long P = pf->P, Pf = pf->Pf;
  static const gpmdm_innovation_out none{};
  const gpmdm_innovation_out& o = out ? *out : none;
  if (pf->propagated)
    TRY(flush_ll(pf, s));              // a deferred finish has not produced vc yet
  else
    HIPCHK(pf->zslot_free());          // the frame's launches, whatever stream they ran on
  const size_t n_out = innov_out_doubles(D, F);
  TRY(pf->iv_part.grow(innov_part_doubles(Pf, D, F), s));
  TRY(pf->iv_out.reserve(n_out, s));
  const size_t n_tile_part = (size_t)F * readout_tiles(Pf) * readout_groups(D) * kRoGC * kInnovPlanes;
  InnovParams ip{};
  ip.ro = pose_readout(pf, pf->X_prop, nullptr, nullptr);
  ip.vc = pf->pv_has_vc ? pf->vc_prop : nullptr;
  ip.z = pf->pv_z;
  ip.mask = pf->pv_masked ? pf->pv_mask.dev : nullptr;
  ip.il2 = m->y_il2_dev;
  ip.lam2 = m->y_lam2_dev;
  ip.part = pf->iv_part;
  ip.vpart = pf->iv_part + n_tile_part;
  ip.out = pf->iv_out.dev;
  launch_obs_innov(ip, s);
  if (!out) {                          // launched only (timing): the handle's lifecycle waits for it
    HIPCHK(hipGetLastError());
    return pf->iv_out.leave_pending(s);
  }
  auto copies = [&]() -> int {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->iv_out.pin, pf->iv_out.dev, sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    if (o.states) HIPCHK(hipMemcpyAsync(o.states, pf->X_prop, sizeof(double) * P * d, hipMemcpyDeviceToHost, s));
    if (o.variance_common && pf->pv_has_vc)
      HIPCHK(hipMemcpyAsync(o.variance_common, pf->vc_prop, sizeof(double) * P, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  TRY(pf->iv_out.finish(copies(), s));   // (quiesce waits for the launches if the wait fails)
  double* const fields[kInnovFields] = {o.mean, o.spread, o.gp_variance, o.variance, o.residual, o.zscore, o.log_density};
  for (int f = 0; f < F; ++f) {
    const double* row = pf->iv_out.pin + (size_t)f * (kInnovFields * D + 1);
    for (int k = 0; k < kInnovFields; ++k)
      if (fields[k]) std::memcpy(fields[k] + (size_t)f * D, row + (size_t)k * D, sizeof(double) * D);
    if (o.n_valid) o.n_valid[f] = (int64_t)row[(size_t)kInnovFields * D];
  }
  if (o.observed) {
    if (pf->pv_masked)
      std::memcpy(o.observed, pf->pv_mask, (size_t)F * D);
    else
      std::memset(o.observed, 1, (size_t)F * D);
  }
  if (o.variance_common && !pf->pv_has_vc)
    for (long long i = 0; i < P; ++i) o.variance_common[i] = std::nan("");
  return GPMDM_OK;
}

static int observation_gp(gpmdm_pf* pf, double* gp_var, void* stream) {
  TRY(readable(pf, "observation_gp"));
  if (pf->mid_step() || !pf->pv_resampled)
    return fail(GPMDM_E_STATE, "observation_gp needs a completed resample of a frame weighed with the predictive switch on");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D, F = pf->F;
  const size_t n_out = (size_t)F * D, nbf = (size_t)cdiv(pf->Pf, 256);
  HIPCHK(pf->zslot_free());            // the frame's resample, whatever stream it ran on
  TRY(pf->iv_part.grow((size_t)F * nbf * 2, s));
  TRY(pf->iv_out.reserve(n_out, s));
  VcGatherArgs ga{};
  ga.Pf = pf->Pf;
  ga.D = D;
  ga.vc = pf->pv_has_vc ? pf->vc_prop : nullptr;
  ga.ridx = pf->ridx;
  ga.il2 = m->y_il2_dev;
  ga.partials = pf->iv_part;
  ga.out = pf->iv_out.dev;
  launch_vc_gather(ga, F, s);
  if (!gp_var) {                       // launched only (timing)
    HIPCHK(hipGetLastError());
    return pf->iv_out.leave_pending(s);
  }
  auto copy = [&]() -> int {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pf->iv_out.pin, pf->iv_out.dev, sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  TRY(pf->iv_out.finish(copy(), s));
  std::memcpy(gp_var, pf->iv_out.pin, sizeof(double) * n_out);
  return GPMDM_OK;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_pf_set_predictive(gpmdm_pf_t pf, int on) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "gpmdm_pf_set_predictive serves single filters, not banks (gpmdm_bank_set_predictive)");
  return set_predictive(pf, on);
}

int gpmdm_bank_set_predictive(gpmdm_pf_t pf, int on) {
  CHECK(pf, "null handle");
  return set_predictive(pf, on);
}

int gpmdm_pf_innovation(gpmdm_pf_t pf, const gpmdm_innovation_out* out, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "gpmdm_pf_innovation serves single filters, not banks (gpmdm_bank_innovation)");
  return innovation(pf, out, stream);
}

int gpmdm_bank_innovation(gpmdm_pf_t pf, const gpmdm_innovation_out* out, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F <= 65535, "bank innovations serve up to 65535 filters");
  return innovation(pf, out, stream);
}

int gpmdm_pf_observation_gp(gpmdm_pf_t pf, double* gp_var, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "gpmdm_pf_observation_gp serves single filters, not banks (gpmdm_bank_observation_gp)");
  return observation_gp(pf, gp_var, stream);
}

int gpmdm_bank_observation_gp(gpmdm_pf_t pf, double* gp_var, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F <= 65535, "bank innovations serve up to 65535 filters");
  return observation_gp(pf, gp_var, stream);
}

}  // extern "C"
