// Outlier gating inside the frame (gpmdm_pf_set_gate, gpmdm_pf_gate_report): joints whose
// innovation z-score exceeds a threshold are dropped from the frame's likelihood before the
// normaliser runs, decided on the device from what the likelihood finish left there.
//
// With obs the caller's mask, zscore_j the frame's innovation z-score (obs_innov.h: against the
// propagated, equally weighted cloud), threshold k and cap = floor(limit D_obs) (host, fp64):
//   exceeded_j = obs_j and |zscore_j| > k            (false for NaN)
//   gated      = exceeded if 1 <= n_exceeded <= cap, else empty (overflow if n_exceeded > cap)
//   used       = obs and not gated,  D' = |used|
// and, when something is gated, for every particle (vc_p: the stored vc_prop)
//   S'_p  = sum_{j in used} (z_j - mu_pj)^2 lam2_j
//   ll'_p = -1/2 S'_p / vc_p - D' log vc_p - sum_{j in used} log il2_j - (D'/2 ln 2 pi)_f32
// -- obs_ll_value's expression (pf_kernels.hip) on the kept joints; D' = 0 gives exactly 0, as a
// blackout frame.  vc_p is independent of z and of the mask, so no N x N pass runs again.
//
// Launches, all on the frame's stream behind the likelihood finish, none waited for:
//   launch_obs_innov  (obs_innov.h, unchanged) into the gate's own scratch: zscore, n_valid
//   k_gate_decide     one workgroup: the rule above into the table GateTab (the joint sums in
//                     ascending joint order by one thread; the float32 constant by IEEE fp32
//                     multiplication, as capi_pf.hip install_obs_mask forms it); every store is
//                     one 8-byte value per lane
//   k_obs_reweigh     k_obs_readout's sibling: the same workgroup (64 particles x 64 columns),
//                     the same K loop (obs_readout_tile.h ro_tile_means).  Epilogue: per element
//                     used_j ? (z_j - mu_pj)^2 lam2_j : 0 (a lane holds one column and 16 particle
//                     rows); per particle row the 16 columns of the lane group (xor 1, 2, 4, 8),
//                     then the four waves through LDS in wave order; one 8-byte partial per
//                     particle and column group, Sp[G][p].  Padding columns and rows past the
//                     tile's count add exact zeros.
//   k_gate_finish     one thread per particle, blocks of 256 as k_obs_ll: the column groups in
//                     order, ll'_p stored where ll lives, and the block's maximum key
//                     (ord_enc(fmax(-inf, ll'))) where the frame's normaliser reads block maxima.
// The host does not know the decision when it queues the resample: k_obs_reweigh and
// k_gate_finish are launched on every gated-mode frame and return at once, uniformly per
// workgroup, when the table's n_gated is 0 -- ll, the maxima and everything after them are then
// untouched.  Every order is fixed and there are no floating-point atomics: the same frame gives
// the same bits.
#pragma once
#include "obs_innov.h"

namespace gpmdm {

// GateTab: doubles.  [0, 8): n_gated, n_valid, overflow, D', sum_{used} log il2, the float32
// constant, n_exceeded, unused; then four rows of D: zscore, exceeded, gated, used (0 / 1).
constexpr int kGateHead = 8;
enum GateSlot : int { kGateNGated = 0, kGateNValid, kGateOverflow, kGateDUsed, kGateSumLog, kGateConst, kGateNExceeded };
inline size_t gate_tab_doubles(int D) { return (size_t)kGateHead + 4 * (size_t)D; }

struct GateParams {
  ReadoutParams ro;                  // the cloud x~ (X = X_prop); part / out unused
  const double* innov;               // launch_obs_innov's table (7 D + 1)
  const unsigned char* mask;         // D (1: observed), or nullptr: every joint observed
  const double* z;                   // D staged observation
  const double* lam2;                // D: the model's lambda_j^2
  const double* log_il2;             // D: log il2_j as the host forms it
  const double* vc;                  // P: vc_prop
  double threshold;
  int cap;
  double* tab;                       // GateTab
  double* Sp;                        // n_groups x P partial sums
  double* ll;                        // P
  unsigned long long* bmax;          // ceil(P / 256) block maxima, or nullptr
};

void launch_gate(const GateParams& p, hipStream_t s);

}  // namespace gpmdm
