// Backward simulation (gpmdm_backward_sample_step, gpmdm_pf_sample_trajectories): draws from the
// joint smoothing distribution over the clouds the ancestry ring of smooth.h holds (FFBSi;
// Godsill, Doucet & West 2004).  One step takes backsmooth.h's sources {x_k, c_k, a_k}, targets
// {x'_j, c'_j} and one uniform u_j per target, and with that header's transition density f_kj gives
//   D_j = sum_k a_k f_kj,   idx_j = the lowest k with sum_{i <= k} a_i f_ij > u_j D_j
// (sources in index order; -1 when no source reaches j).  The sums are backsmooth.h's (m, s)
// pairs, by the same code (bs_den_range): the sources are cut into ranges of kFsRange rows -- a
// function of n_s alone, so a target's result does not depend on the other targets -- and
//   k_fs_sum     k_bs_den's layout (targets across threads in the class-grouped blocks, a class's
//                records through LDS 64 at a time), gridDim.y the ranges: each (target, range)
//                leaves its (m, s)
//   k_fs_pick    per target: the ranges merged in range order into D = S 2^M and log_den; the
//                threshold t = u S in the scale 2^M; the merge once more, stopping at the first
//                range whose prefix exceeds t (scaled to 2^M: exact), and the residual t - prefix
//                before it; no crossing by rounding: the last range of positive sum, residual +inf
//   k_fs_select  k_fs_sum's grid; a thread takes part in its target's chosen range only and runs
//                that range's sum again -- the same code in the same order, so the partial sums are
//                bitwise pass 1's -- up to the first source behind which the sum, scaled to 2^M,
//                exceeds the residual; it carries the last source of positive term as fallback
// Only sources with a finite exponent are ever candidates, so a source of term zero is never
// returned, and whenever D_j > 0 one is.  The ring's glue:
//   k_fs_draw    the uniforms u_{m,l} = u01_co of Philox (m, frame, kStreamBackSample, l) and
//                j_0 = min(P - 1, floor(u_{m,0} P))
//   k_fs_gather  row l of the result from slot l by j_l: {state, class}, NaN and -1 for a dead
//                trajectory (j_l = -1) -- also the next step's targets: a NaN state has no finite
//                exponent, so a dead trajectory stays dead
//   k_fs_reduce  one workgroup per lag: alive count, class counts, the state sums (thread-strided,
//                wave butterfly, the waves in order: k_bs_reduce's order, on two-term sums so that
//                the mean is the rounded exact one) and the distinct particles by an integer
//                mark-and-count
// No floating-point atomics; every order is fixed: the same inputs give the same bits.
#pragma once
#include "backsmooth.h"

namespace gpmdm {

constexpr int kFsRange = 1024;   // sources per range (GPMDM_BACKSAMPLE_RANGE)
static_assert(kFsRange % kBsTile == 0, "ranges are whole tiles");

inline long long fs_ranges(long long n_s) { return (n_s + kFsRange - 1) / kFsRange; }

struct FsPassArgs {
  long long n_s, n_t;             // n_t: the targets of this launch (a chunk of the call's)
  int C, d, n_ranges;
  const double* rec;              // C x n_s x (2 d + 1)
  const double* Xt;               // n_t x d
  const int* perm;                // n_t
  const int* tab;
  double* part;                   // 2 x n_ranges x n_t: the ranges' m, then their s, by grouped position
  // k_fs_pick's results, by grouped position (k_fs_select reads them)
  int* range;                     // the chosen range, -1: no source reaches the target
  double* res;                    // the residual threshold in the scale 2^M
  double* scale;                  // M
  const double* u;                // n_t
  int* idx;                       // n_t
  double* log_den;                // n_t natural logarithm, or nullptr
};

struct FsDrawArgs {
  long long n, P;
  int lag;
  unsigned frame, seed_lo, seed_hi;
  double* u;                      // (lag + 1) x n
  int* idx0;                      // n
};

struct FsGatherArgs {
  long long n;
  int d;
  const int* idx;                 // n: rows of the slot, -1: dead
  const double* X;                // the slot's P x d
  const int* cls;                 // the slot's P
  double* X_out;                  // n x d
  int* cls_out;                   // n, or nullptr: the states alone
};

struct FsReduceArgs {
  long long n;
  int C, d;
  const int* idx;                 // n
  const int* cls;                 // n (-1: dead)
  const double* X;                // n x d
  int* mark;                      // P zeros, left zeroed
  double* out;                    // {alive, distinct, counts[C], sum hi[d], sum lo[d]}
};

void launch_fs_sum(const FsPassArgs& a, hipStream_t s);
void launch_fs_pick(const FsPassArgs& a, hipStream_t s);
void launch_fs_select(const FsPassArgs& a, hipStream_t s);
void launch_fs_draw(const FsDrawArgs& a, hipStream_t s);
void launch_fs_gather(const FsGatherArgs& a, hipStream_t s);
void launch_fs_reduce(const FsReduceArgs& a, hipStream_t s);
void launch_fs_flag(const int* idx, long long n, int* flag, hipStream_t s);   // flag[m] = idx[m] >= 0

}  // namespace gpmdm
