// Filtered-pose read-out (gpmdm_pf_observation): the observation GP's mean only, averaged
// over the particle cloud.
//
//   mu_j(x_p) = sum_i k(x_p, X_i) beta_ij,  beta = K_y^-1 Y  (gpmdm.py:955-957)
//   mean_j = (1/P) sum_p mu_j(x_p),  spread_j = (1/P) sum_p (mu_j(x_p) - mean_j)^2
//
// The filter's observation tile (gp_tile.h) produces mu only inside its fused likelihood
// epilogue, behind the N x N triangle of the variance's quadratic form.  This kernel touches
// the mean part alone: 2 N 16 ceil(D/16) FLOPs per particle plus N generated kernel values.
//
// k_obs_readout: one workgroup (4 waves) = 64 particles x one group of 64 columns, looping
// over all training rows in K-steps of 16.  Per K-step the 64 x 16 K* tile is generated once
// per workgroup -- the same expansion-form exponent and exp2_64 as gp_tile.h, from the
// observation image's row records (SegDesc::Xrec), thread (particle m = lane, rows w + 4s) --
// into a double-buffered LDS tile, one barrier per K-step; wave w contracts it with its own
// 16-column tile of beta by v_mfma_f64_16x16x4_f64 (4 particle tiles x 4 sub-steps).  beta is
// a fragment-ordered copy of its own (pack_readout_beta), zero-padded to whole K-steps and
// whole column groups: lane l of wave w reads the four sub-steps' B operands
//   B[row = 16 ks + 4 kk + (l >> 4)][col = 64 G + 16 w + (l & 15)],  kk = 0..3
// as 32 contiguous bytes at (((G nks + ks) 4 + w) 64 + l) 4.  A model with D > 64 has several
// column groups (grid.y); each re-generates K*.
// Rows past the last particle evaluate the tile's first particle (no per-lane mask in the K
// loop) and carry count 0 in the epilogue's reduction.
// Epilogue: per column, the tile's sum (pairwise in the lane, then across the four lane
// groups), its mean, and in a second pass over the accumulators the sum of squares centred
// on that mean; (mean, M2) go to part[tile][column].  k_obs_readout_finish merges the tiles'
// partials in tile order with the pairwise update of Chan et al. (16 contiguous runs of
// tiles per column, then the 16 runs in order), so the spread is never formed as
// E[mu^2] - mean^2 and every reduction has a fixed order: the same cloud gives bitwise the
// same read-out on every call.
// A bank (gpmdm_bank_observation) adds a filter dimension to both grids: ceil(P / 64) tiles per
// filter, cut within the filter, partials and finish per filter -- the partition within a filter
// is the single filter's, so row f is bitwise the read-out of a single filter holding f's cloud.
// The K loop, the (mean, M2) epilogue and the pairwise update are device functions of
// obs_readout_tile.h, which the innovation tile (obs_innov.h) calls too.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "geometry.h"

namespace gpmdm {

constexpr int kRoPT = 64;        // particles per workgroup
constexpr int kRoGC = 64;        // columns per group (4 waves x one 16-column tile)

struct ReadoutParams {
  const double* X;               // F x P x d particle states
  long long P;                   // particles per filter
  int F;                         // filters (a bank: one pair of launches for all; 0 or 1: one cloud)
  int d, D;
  const double* ls;              // d observation-kernel lengthscales (device)
  const double* Xrec;            // the observation image's row records
  int nks;                       // K-steps: ksteps(N)
  const double* Bro;             // fragment-ordered beta (pack_readout_beta)
  int n_groups;                  // column groups: ceil(D / 64)
  double* part;                  // F x n_tiles x {mean, M2} x (64 n_groups)
  double* out;                   // F x {mean[D], spread[D]}
};

inline int readout_tiles(long long P) { return (int)((P + kRoPT - 1) / kRoPT); }
inline int readout_groups(int D) { return (D + kRoGC - 1) / kRoGC; }
inline size_t readout_part_doubles(long long P, int D, int F = 1) {
  return (size_t)F * readout_tiles(P) * readout_groups(D) * kRoGC * 2;
}

// beta (N x D row-major) in the kernel's fragment order: readout_groups(D) * ksteps(N) * 1024 doubles
void pack_readout_beta(const double* beta, long long N, int D, std::vector<double>& out);
void launch_obs_readout(const ReadoutParams& p, hipStream_t s);

}  // namespace gpmdm
