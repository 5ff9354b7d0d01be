// Marginal backward smoothing (gpmdm_backward_step, gpmdm_pf_smoothed_marginal): the
// forward-filter backward marginal smoother (FFBSm; Doucet, Godsill & Andrieu 2000 §2.3) over
// the clouds the ancestry ring of smooth.h already holds.  One backward step takes sources
// {x_k, c_k} with filter weights a_k and targets {x'_j, c'_j} with smoothing weights w_j and, with
// the filter's proposal as transition density (the class switches, then the state moves under
// the new class's dynamics GP),
//   log f_kj = log T[c_k, c'_j] - 1/2 sum_q [(x'_jq - mu_q)^2 / v_q + log v_q] - d/2 log 2 pi,
//   mu, v = the class-c'_j dynamics GP's mean and variance at x_k,
// computes
//   D_j = sum_k a_k f_kj,   ws_k = a_k sum_j w_j f_kj / D_j   (targets with D_j = 0 contribute 0).
// Everything runs on base-2 logarithms.  A running sum is a pair (m, s) = s 2^m with m an
// integer: a new exponent l adds 2^(l - m) after m has been raised to ceil(l) if l exceeds it,
// which rescales s by a power of two -- exactly -- so the value of a sum depends on the order
// of its terms through the rounding of the additions only.
//   k_bs_moments  thread (k, c): the source record {mu[d], 1/v[d], g} of class c at source k from
//                 the dynamics tiles' mean and variance; g = log2 of a_k T[c_k, c] (2 pi)^(-d/2)
//                 prod_q v_q^(-1/2), -inf when v is non-positive or non-finite
//   k_bs_group    one workgroup: the stable grouping of the targets by class (counts, starts,
//                 the permutation) -- every lane of a block of the passes shares c'
//   k_bs_den      targets across threads (grouped order, blocks cut within a class), the class's
//                 source records streamed through LDS in index order (every lane reads the same
//                 address: a broadcast); gridDim.y splits the sources into equal ranges
//   k_bs_den_fin  the ranges' (m, s) combined in range order: log_den_j, and the target's
//                 exponent lw_j = log2 w_j - log2 D_j for the weight pass
//   k_bs_wgt      sources across threads, the targets {x', lw} streamed through LDS in grouped
//                 order, the thread holding one class's record in registers at a time;
//                 gridDim.y splits the grouped targets into equal ranges
//   k_bs_wgt_fin  the ranges combined in range order: ws_k = s 2^m
//   k_bs_hist / k_bs_mult   the integer histogram of a slot's ancestors and m_i = hist[anc_i]
//   k_bs_reduce   one workgroup per row: class masses, mean state, mass, sum w^2, sum m w^2
//                 (thread-strided, wave butterfly, the waves in order: k_sm_reduce's order)
// No floating-point atomics; the ranges are a function of (n_s, n_t) alone: the same inputs give
// the same bits, and two sources with the same (x, c, a) get the same weight.
#pragma once
#include "common.h"
#include "pf_kernels.h"

namespace gpmdm {

constexpr int kBsB = 256;       // threads per block of the passes
constexpr int kBsTile = 64;     // streamed rows per LDS tile
constexpr int kBsMaxSplit = 64; // ranges of the streamed side

// ranges of a streamed side of n rows when the other side has n_other rows: enough blocks to
// fill the machine at small sizes, never shorter than a tile
inline int bs_split(long long n_other, long long n) {
  const long long bx = (n_other + kBsB - 1) / kBsB;
  long long s = (2048 + bx - 1) / bx;
  const long long tiles = (n + kBsTile - 1) / kBsTile;
  if (s > tiles) s = tiles;
  if (s > kBsMaxSplit) s = kBsMaxSplit;
  return (int)(s < 1 ? 1 : s);
}

struct BsMomentArgs {
  long long n;                    // sources
  int C, d, c;                    // c: the class whose records are written
  const double* mu;               // n x d   dynamics mean of class c at source k
  const double* var;              // n x d   ... variance
  const int* cls;                 // n
  const double* a;                // n filter weights, or nullptr: 1 / n each
  const double* T;                // C x C
  double* rec;                    // C x n x (2 d + 1)
};

struct BsGroupArgs {
  long long n;
  const int* n_dev;               // the row count on the device (mappath.h's compacted slots), or nullptr: n
  int C;
  const int* cls;                 // n
  int* perm;                      // n      grouped position -> target
  int* tab;                       // [0, C]: class starts (tab[C] = n); [C + 1, 2 C + 1]: block starts
};

struct BsPassArgs {
  long long n_s, n_t;
  int C, d, split;
  const double* rec;              // C x n_s x (2 d + 1)
  const double* Xt;               // n_t x d
  const int* perm;                // n_t
  const int* tab;
  const double* lw;               // n_t: the targets' exponents (weight pass)
  double* part;                   // 2 x split x n: the ranges' m, then their s
};

struct BsDenFinArgs {
  long long n_t;
  int split;
  const double* part;             // by grouped position
  const int* perm;
  const double* wt;               // n_t
  double* log_den;                // n_t natural logarithm, or nullptr
  double* lw;                     // n_t, by grouped position
};

struct BsWgtFinArgs {
  long long n_s;
  int split;
  const double* part;
  double* ws;                     // n_s
};

struct BsReduceArgs {
  long long P;
  int C, d;
  const double* w;                // P
  const double* X;                // P x d
  const int* cls;                 // P
  const int* mult;                // P, or nullptr: 1
  double* out;                    // {class mass[C], mean state[d], mass, ess, ess_distinct}
};

void launch_bs_moments(const BsMomentArgs& a, hipStream_t s);
void launch_bs_group(const BsGroupArgs& a, hipStream_t s);
void launch_bs_den(const BsPassArgs& a, hipStream_t s);
void launch_bs_den_fin(const BsDenFinArgs& a, hipStream_t s);
void launch_bs_wgt(const BsPassArgs& a, hipStream_t s);
void launch_bs_wgt_fin(const BsWgtFinArgs& a, hipStream_t s);
void launch_bs_fill(double* w, long long n, double v, hipStream_t s);
void launch_bs_mult(const int* anc, long long P, int* hist, int* mult, hipStream_t s);   // hist: P, zeroed here
void launch_bs_reduce(const BsReduceArgs& a, hipStream_t s);

}  // namespace gpmdm
