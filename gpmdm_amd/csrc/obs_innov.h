// Per-joint innovations of the frame just weighed (gpmdm_pf_innovation) and the GP's predictive
// variance of the resampled cloud (gpmdm_pf_observation_gp).
//
// With x~_p the propagated particles (pre-resample, equally weighted), mu_pj the observation
// GP's mean, vc_p = 1 - k^T K_y^-1 k as the likelihood finish formed it (ObsFinishArgs::vc_out),
// il2_j = lambda_j^-2, V = {p : vc_p > 0}, n_valid = |V|, z the frame's staged observation:
//   mean_j, spread_j   (1/P) sum_p mu_pj, (1/P) sum_p (mu_pj - mean_j)^2 -- the pose read-out's
//   gp_variance_j      il2_j (1/n_valid) sum_{p in V} vc_p
//   variance_j         spread_j + gp_variance_j
//   residual_j         z_j - mean_j
//   zscore_j           residual_j / sqrt(variance_j)
//   log_density_j      log (1/n_valid) sum_{p in V} N(z_j; mu_pj, vc_p il2_j)
// residual, zscore and log_density are NaN at unobserved joints; every vc-dependent field is NaN
// when n_valid = 0.
//
// k_obs_innov is k_obs_readout's sibling: the same workgroup (64 particles x 64 columns), the same
// K loop and (mean, M2) epilogue (obs_readout_tile.h: one definition, so mean and spread are
// bitwise the read-out's on the same cloud).  Before the epilogue wave 0 stages, per particle of
// the tile, -1/2 / vc and -1/2 log vc in LDS (one division and one log per particle, none per
// element).  A second pass over the accumulators forms per element
//   a = -1/2 (t^2 lam2_j / vc_p) - 1/2 (log vc_p + log il2_j + ln 2 pi),  t = z_j - mu_pj
// (as one fma on the staged values) and per column the tile's log-sum-exp pair (M = max a,
// s = sum exp(a - M), the exponentials by the generation's exp2_64) over the valid rows
// (inside the tile, vc_p > 0): the lane's 16 elements (maximum, then the sum as a fixed pairwise
// tree), then the four lane groups (xor 16, xor 32) by
//   (M, s) + (M', s') = (max, s exp(M - max) + s' exp(M' - max)).
// Partials per tile: four planes {mean, M2, M, s} x (64 n_groups), and from the workgroups of
// column group 0 the tile's sum of valid vc and their count (wave 0's butterfly) -- all 8-byte
// stores.  k_obs_innov_finish merges the tiles in the read-out's order (16 runs of contiguous
// tiles, then the runs in order): Chan's update for (n, mean, M2), the rule above for (M, s),
// plain sums for (sum vc, count); then it forms the table.  No floating-point atomics, every
// order fixed: the same frame gives the same bits on every call.  The filter is grid.z / grid.y
// as in the read-out; a masked bank reads filter f's row of z and of the mask.
//
// k_vc_gather: sum_s vc[ridx[s]] over the valid entries and their count per filter -- blocks of
// 256 cut within the filter, wave butterfly, the four waves in order (k_fc_sum's order);
// k_vc_gather_finish adds the blocks in order and writes il2_j sum / count.
#pragma once
#include "obs_readout.h"

namespace gpmdm {

constexpr int kInnovPlanes = 4;      // {mean, M2, M, s} per tile and column
constexpr int kInnovFields = 7;      // mean, spread, gp_variance, variance, residual, zscore, log_density

struct InnovParams {
  ReadoutParams ro;                  // the cloud x~ (X = X_prop); part / out unused
  const double* vc;                  // F x P, or nullptr: no observation kernel ran (every vc invalid)
  const double* z;                   // F x D staged observation
  const unsigned char* mask;         // F x D (1: observed), or nullptr: every joint observed
  const double* il2;                 // D
  const double* lam2;                // D: 1 / il2
  double* part;                      // F x n_tiles x 4 x (64 n_groups)
  double* vpart;                     // F x {sum vc, count} x n_tiles
  double* out;                       // F x (7 D + 1): the seven fields, then n_valid
};

inline size_t innov_part_doubles(long long P, int D, int F) {
  return (size_t)F * readout_tiles(P) * (readout_groups(D) * kRoGC * kInnovPlanes + 2);
}
inline size_t innov_out_doubles(int D, int F) { return (size_t)F * (kInnovFields * D + 1); }

struct VcGatherArgs {
  long long Pf;
  int D;
  const double* vc;                  // F x Pf (the propagated cloud's, or nullptr: all invalid)
  const int* ridx;                   // F x Pf ancestors, within the filter
  const double* il2;                 // D
  double* partials;                  // F x ceil(Pf / 256) x {sum, count}
  double* out;                       // F x D
};

void launch_obs_innov(const InnovParams& p, hipStream_t s);
void launch_vc_gather(const VcGatherArgs& a, int F, hipStream_t s);

}  // namespace gpmdm
