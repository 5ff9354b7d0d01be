// Multi-step forecast roll-out (gpmdm_pf_forecast, gpmdm_bank_forecast): the filter's own
// proposal -- Markov switch, then x <- mu_c(x) + sqrt(var_c(x)) eps (gpmdm_pf.py:137-168) --
// chained h = 1..H on a scratch copy of the particle cloud, with no weighting and no resampling,
// and per horizon and filter the class fractions and the mean state (the pose read-out of each
// step is obs_readout.h's).
//
// One set of kernels serves single filters and banks: a single filter is a bank of F = 1.
// Particles are filter-major (g = f * Pf + p).  The dynamics-GP tiles (gp_tile.h) and the
// grouping passes (k_scan_counts, k_group) are the filter's and run over all F * Pf particles, as
// the step and predict() run them; the kernels here are the O(P (C + d)) passes around them:
//   k_fc_switch   k_switch's argmax_j T[c, j] / E_j on the scratch classes, with the forecast
//                 draws, and the per-block class counts the grouping scans (blocks span the
//                 whole bank and may mix filters)
//   k_fc_finish   k_dyn_finish's variance and sample from the tiles' partials, written to the
//                 next scratch cloud; with `partials` set, also the per-block sums of the new
//                 states, in the grouped order of its blocks (F = 1 only: grouped blocks mix
//                 filters)
//   k_fc_sum      grid (ceil(Pf / 256), F), blocks cut within the filter, particle order: the
//                 block's class histogram (integers, plain stores: one row per block) and its
//                 sum of the new states
//   k_fc_reduce   one workgroup per filter: class fractions from the integer counts, the mean
//                 state from the blocks' sums, fixed summation order, each divided once by Pf
// The mean state has two summation orders, chosen by the entry point and never by F:
// gpmdm_pf_forecast sums inside the finish (grouped order, no k_fc_sum launch, class counts from
// the grouping's table); gpmdm_bank_forecast runs k_fc_sum, so a filter's mean state depends on
// its own cloud alone -- not on the other filters of the bank, not on how a bank is sharded.
//
// Draws: Philox4x32-10 with filter f's key (seed + f) and the counter
//   (in-filter index p, frame, kStreamForecastSwitch | kStreamForecastDyn, (h << 8) | pair),
// h = 1..H the roll-out step and pair = j >> 1 as in k_switch / k_dyn_finish: a forecast is a
// function of (cloud, frame, seed) alone, its first rows do not depend on H, it shares no
// counter with the filter's own streams, and row f of a bank's result is the single filter's
// result on f's cloud.  No floating-point atomics: every sum has a fixed order, so the same
// cloud gives bitwise the same forecast.
#pragma once
#include "common.h"
#include "pf_kernels.h"

namespace gpmdm {

struct FcSwitchArgs {
  long long P, Pf;                // all particles (F * Pf), particles per filter
  int C;
  unsigned h, frame, seed_lo, seed_hi;
  const int* cls;                 // P   classes before the step
  int* cls_new;                   // P   switched classes
  const double* T;                // C x C Markov matrix (device)
  int* blockcounts;               // ceil(P / 256) x C, bank-wide blocks (the grouping's)
};

struct FcFinishArgs {
  long long P, Pf;
  int C, d, mean_only;            // mean_only: x <- mu_c(x), no draw
  unsigned h, frame, seed_lo, seed_hi;
  const int* seg_out_base;        // [C] first tile row of each class (the grouping's table)
  const int* seg_pos_begin;       // [C] first grouped position of each class
  const int* perm;                // grouped position -> particle (bank-wide index g)
  int n_parts[kMaxClasses];       // q partials per class
  const double* qpart;            // [part][P]
  long long ld_q;
  const double* mu;               // P x d, tile rows
  const double* X;                // P x d cloud before the step
  double lin_c2[kMaxD + 1];
  double il2[kMaxD];
  double* X_out;                  // P x d cloud after the step (particle order)
  double* partials;               // ceil(P / 256) x d block sums of X_out, or nullptr: k_fc_sum's
};

struct FcSumArgs {
  long long Pf;
  int C, d;
  const double* X;                // F x Pf x d   the step's cloud
  const int* cls;                 // F x Pf       its classes, or nullptr: counts are kept
  int* bcounts;                   // F x nbf x C  per-block class counts
  double* partials;               // F x nbf x d  per-block state sums
};

struct FcReduceArgs {
  long long Pf;
  int C, d, nbf;
  int n_count_rows;               // rows of C counts per filter: nbf (k_fc_sum's), or 1 (the grouping's table)
  const int* counts;
  const double* partials;         // F x nbf x d
  double* out;                    // F rows of {class_prob[C], state_mean[d]}
};

void launch_fc_switch(const FcSwitchArgs& a, hipStream_t s);
void launch_fc_finish(const FcFinishArgs& a, hipStream_t s);
void launch_fc_sum(const FcSumArgs& a, int F, hipStream_t s);
void launch_fc_reduce(const FcReduceArgs& a, int F, hipStream_t s);

}  // namespace gpmdm
