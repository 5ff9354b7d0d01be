// Outlier gating inside the frame (gpmdm_pf_set_gate, gpmdm_pf_gate_report and the banks'
// gpmdm_bank_set_gate, gpmdm_bank_gate_report): joints whose innovation z-score exceeds a
// threshold are dropped from the frame's likelihood before the normaliser runs, decided on the
// device from what the likelihood finish left there.
//
// Per filter (a single filter is the bank of F = 1: one definition of each kernel), with obs the
// filter's mask, zscore_j the frame's innovation z-score (obs_innov.h: against the
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
//   k_gate_decide     one workgroup per filter (grid F): the rule above from filter f's row of
//                     the innovation table, of the mask and of the host's {threshold, cap} table
//                     into f's GateTab (the joint sums in ascending joint order by one thread;
//                     the float32 constant by IEEE fp32 multiplication, as capi_pf.hip
//                     install_obs_mask forms it); every store is one 8-byte value per lane
//   k_obs_reweigh     k_obs_readout's sibling: the same workgroup (64 particles x 64 columns),
//                     the same K loop (obs_readout_tile.h ro_tile_means).  Epilogue: per element
//                     used_j ? (z_j - mu_pj)^2 lam2_j : 0 (a lane holds one column and 16 particle
//                     rows); per particle row the 16 columns of the lane group (xor 1, 2, 4, 8),
//                     then the four waves through LDS in wave order; one 8-byte partial per
//                     particle and column group, Sp[f][G][p].  Padding columns and rows past the
//                     tile's count add exact zeros.  The filter is grid.z, as in k_obs_readout
//                     and k_obs_innov: tiles are cut within the filter (a padded row evaluates
//                     the tile's first particle, never the next filter's), and the workgroup
//                     reads filter f's rows of z and of `used`.
//   k_gate_finish     one thread per particle, blocks of 256 cut within the filter (grid
//                     ceil(P / 256) x F) as k_obs_ll: the column groups in order, ll'_p stored
//                     where ll lives (f P + p), and -- single filters, whose finish produces them
//                     -- the block's maximum key (ord_enc(fmax(-inf, ll'))) where the frame's
//                     normaliser reads block maxima (a bank's normaliser takes each filter's
//                     maximum from ll itself: nullptr).
// The host does not know the decision when it queues the resample: k_obs_reweigh and
// k_gate_finish are launched on every gated-mode frame, once for all filters, and a workgroup
// returns at once, uniformly and before any barrier, when its filter's n_gated is 0 -- that
// filter's ll, the maxima and everything after them are then untouched, whatever its neighbours
// decide.  Every order is fixed and there are no floating-point atomics: the same frame gives
// the same bits, and row f is bitwise the single filter's on filter f's frame.
#pragma once
#include "obs_innov.h"

namespace gpmdm {

// GateTab, one per filter: doubles.  [0, 8): n_gated, n_valid, overflow, D', sum_{used} log il2, the float32
// constant, n_exceeded, unused; then four rows of D: zscore, exceeded, gated, used (0 / 1).
constexpr int kGateHead = 8;
enum GateSlot : int { kGateNGated = 0, kGateNValid, kGateOverflow, kGateDUsed, kGateSumLog, kGateConst, kGateNExceeded };
inline size_t gate_tab_doubles(int D) { return (size_t)kGateHead + 4 * (size_t)D; }

// the host's table, per filter: the threshold k (+inf: never rejects) and the cap
constexpr int kGateCfg = 2;

struct GateParams {
  ReadoutParams ro;                  // the cloud x~ (X = X_prop; P per filter, F filters); part / out unused
  const double* innov;               // launch_obs_innov's table, F x (7 D + 1)
  const unsigned char* mask;         // F x D (1: observed), or nullptr: every joint observed
  const double* z;                   // F x D staged observation
  const double* lam2;                // D: the model's lambda_j^2
  const double* log_il2;             // D: log il2_j as the host forms it
  const double* vc;                  // F x P: vc_prop
  const double* cfg;                 // F x {threshold, cap}
  double* tab;                       // F x GateTab
  double* Sp;                        // F x n_groups x P partial sums
  double* ll;                        // F x P
  unsigned long long* bmax;          // ceil(P / 256) block maxima (F = 1), or nullptr
};

void launch_gate(const GateParams& p, hipStream_t s);

}  // namespace gpmdm
