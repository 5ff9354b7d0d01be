// Multi-step forecast roll-out (gpmdm_pf_forecast): the filter's own proposal -- Markov switch,
// then x <- mu_c(x) + sqrt(var_c(x)) eps (gpmdm_pf.py:137-168) -- chained h = 1..H on a scratch
// copy of the particle cloud, with no weighting and no resampling, and per horizon the class
// fractions and the mean state (the pose read-out of each step is obs_readout.h's).
//
// The dynamics-GP tiles (gp_tile.h) and the grouping passes (k_scan_counts, k_group) are the
// filter's; the three kernels here are the O(P (C + d)) passes around them:
//   k_fc_switch   k_switch's argmax_j T[c, j] / E_j on the scratch classes, with the forecast
//                 draws, and the per-block class counts the grouping scans
//   k_fc_finish   k_dyn_finish's variance and sample from the tiles' partials, written to the
//                 next scratch cloud, and per-block partial sums of the new states
//   k_fc_reduce   class fractions and mean state of one horizon step, fixed summation order
//
// Draws: Philox4x32-10 with the filter's key and the counter
//   (particle index, frame, kStreamForecastSwitch | kStreamForecastDyn, (h << 8) | pair),
// h = 1..H the roll-out step and pair = j >> 1 as in k_switch / k_dyn_finish: a forecast is a
// function of (cloud, frame, seed) alone, its first rows do not depend on H, and it shares no
// counter with the filter's own streams.  No floating-point atomics: every sum has a fixed
// order, so the same cloud gives bitwise the same forecast.
#pragma once
#include "common.h"
#include "pf_kernels.h"

namespace gpmdm {

struct FcSwitchArgs {
  long long P;
  int C;
  unsigned h, frame, seed_lo, seed_hi;
  const int* cls;                 // P   classes before the step
  int* cls_new;                   // P   switched classes
  const double* T;                // C x C Markov matrix (device)
  int* blockcounts;               // ceil(P / 256) x C
};

struct FcFinishArgs {
  long long P;
  int C, d, mean_only;            // mean_only: x <- mu_c(x), no draw
  unsigned h, frame, seed_lo, seed_hi;
  const int* seg_out_base;        // [C] first tile row of each class (the grouping's table)
  const int* seg_pos_begin;       // [C] first grouped position of each class
  const int* perm;                // grouped position -> particle
  int n_parts[kMaxClasses];       // q partials per class
  const double* qpart;            // [part][P]
  long long ld_q;
  const double* mu;               // P x d, tile rows
  const double* X;                // P x d cloud before the step
  double lin_c2[kMaxD + 1];
  double il2[kMaxD];
  double* X_out;                  // P x d cloud after the step (particle order)
  double* partials;               // ceil(P / 256) x d block sums of X_out
};

struct FcReduceArgs {
  long long P;
  int C, d, nb;
  const int* counts;              // [C] class counts of the step (k_scan_counts)
  const double* partials;         // nb x d
  double* out;                    // {class_prob[C], state_mean[d]}
};

void launch_fc_switch(const FcSwitchArgs& a, hipStream_t s);
void launch_fc_finish(const FcFinishArgs& a, hipStream_t s);
void launch_fc_reduce(const FcReduceArgs& a, hipStream_t s);

}  // namespace gpmdm
