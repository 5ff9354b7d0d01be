// Forecasts and fixed-lag smoothing for filter banks (gpmdm_bank_forecast, gpmdm_bank_smoothed):
// the O(P) kernels of forecast.h and smooth.h with a filter dimension.  Particles are
// filter-major (g = f * Pf + p), ancestors are in-filter indices, and filter f's Philox key is
// seed + f with the in-filter index p in the counter, so row f of every result is the single
// filter's result on f's cloud.
//
// The roll-out's grouping (k_scan_counts, k_group) and dynamics tiles run bank-wide over all
// F * Pf particles, as the bank's step and predict() run them; around them
//   k_fcb_switch  k_fc_switch with f = g / Pf: key filter_key(seed, f), counter word p, and the
//                 per-block class counts the bank-wide grouping scans
//   k_fcb_finish  k_fc_finish's variance and sample with the same key and counter; writes the
//                 next cloud only (its blocks are in grouped order and mix filters)
//   k_fcb_sum     grid (ceil(Pf / 256), F), blocks cut within the filter, particle order: the
//                 block's class histogram (integers, plain stores: one row per block) and its
//                 sum of the new states (wave butterfly, then the four waves in order)
//   k_fcb_reduce  one workgroup per filter: class fractions from the blocks' integer counts,
//                 the mean state from the blocks' sums (k_sm_reduce's order), divided by Pf
// so a filter's mean state depends on its own cloud alone: not on the horizon, not on the other
// filters of the bank, not on how a bank is sharded.
//
// The smoother's record (k_sm_record) is a plain copy and serves F * Pf rows as it is; the
// read-out's trace and reduce take the filter as a grid dimension:
//   k_smb_trace   grid (ceil(Pf / 256), F): k_sm_trace inside filter f's rows of each slot
//                 (gathers clamped to [0, Pf)); counts per (lag, filter, class), marks one row
//                 per (lag, filter), partials per (lag, filter, block)
//   k_smb_reduce  grid (lags, F): k_sm_reduce per (lag, filter), divided by Pf
// Blocks cut within a filter are the single filter's blocks, so every smoothed value is bitwise
// the single filter's.  No floating-point atomics anywhere.
#pragma once
#include "forecast.h"
#include "smooth.h"

namespace gpmdm {

struct FcbSwitchArgs {
  long long P, Pf;                // all particles (F * Pf), particles per filter
  int C;
  unsigned h, frame, seed_lo, seed_hi;
  const int* cls;                 // P   classes before the step
  int* cls_new;                   // P   switched classes
  const double* T;                // C x C Markov matrix (device)
  int* blockcounts;               // ceil(P / 256) x C, bank-wide blocks (the grouping's)
};

struct FcbFinishArgs {
  long long P, Pf;
  int C, d, mean_only;
  unsigned h, frame, seed_lo, seed_hi;
  const int* seg_out_base;        // [C] first tile row of each class (the grouping's table)
  const int* seg_pos_begin;       // [C] first grouped position of each class
  const int* perm;                // grouped position -> particle (bank-wide index g)
  int n_parts[kMaxClasses];
  const double* qpart;            // [part][P]
  long long ld_q;
  const double* mu;               // P x d, tile rows
  const double* X;                // P x d cloud before the step
  double lin_c2[kMaxD + 1];
  double il2[kMaxD];
  double* X_out;                  // P x d cloud after the step (particle order)
};

struct FcbSumArgs {
  long long Pf;
  int C, d;
  const double* X;                // F x Pf x d   the step's cloud
  const int* cls;                 // F x Pf       its classes, or nullptr: counts are kept
  int* bcounts;                   // F x nbf x C  per-block class counts
  double* partials;               // F x nbf x d  per-block state sums
};

struct FcbReduceArgs {
  long long Pf;
  int C, d, nbf;
  const int* bcounts;
  const double* partials;
  double* out;                    // F rows of {class_prob[C], state_mean[d]}
};

// rows q = (l - lag_first) * F + f of every output
struct SmbTraceArgs {
  long long Pf;
  int F, C, d;
  int lag_first, lag_last;
  SmRing ring;                    // slots of F * Pf rows
  int* counts;                    // n x F x C        (zeroed before the launch)
  double* partials;               // n x F x nbf x d
  unsigned char* marks;           // n x F x ld_marks (zeroed before)
  long long ld_marks;             // sm_ld_marks(Pf)
  int* anc_out;                   // n x F x Pf       in-filter indices, or nullptr
  int* cls_out;                   // n x F x Pf       or nullptr
  double* X_out;                  // n x F x Pf x d   or nullptr
};

struct SmbReduceArgs {
  long long Pf;
  int C, d, nbf;
  const int* counts;
  const double* partials;
  const unsigned char* marks;
  long long ld_marks;
  double* out;                    // n x F rows of ld_out: {class_prob[C], state_mean[d], distinct}
  int ld_out;
};

void launch_fcb_switch(const FcbSwitchArgs& a, hipStream_t s);
void launch_fcb_finish(const FcbFinishArgs& a, hipStream_t s);
void launch_fcb_sum(const FcbSumArgs& a, int F, hipStream_t s);
void launch_fcb_reduce(const FcbReduceArgs& a, int F, hipStream_t s);
void launch_smb_trace(const SmbTraceArgs& a, hipStream_t s);
void launch_smb_reduce(const SmbReduceArgs& a, int n_lags, int F, hipStream_t s);

}  // namespace gpmdm
