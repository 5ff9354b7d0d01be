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

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------
// Device code the denominator pass shares with backward simulation (backsample.h): one
// definition of the running sums, of a pair's exponent and of a range's loop.
constexpr double kHalfLog2e = 0.72134752044448170368;   // 1/2 log2 e
constexpr double kLn2 = 0.69314718055994530942;

// Running sums s 2^m, m an integer (or -inf with s = 0).
__device__ __forceinline__ int bs_shift(double from, double to) {   // from - to <= 0, clamped (2^-4096 = 0)
  return (int)fmax(from - to, -4096.0);
}
__device__ __forceinline__ void bs_add(double& m, double& s, double l) {
  if (!(l > -INFINITY)) return;          // a term of weight zero
  if (l > m) {
    const double mn = ceil(l);
    s = ldexp(s, bs_shift(m, mn));       // exact (m = -inf: s = 0)
    m = mn;
  }
  s += exp2(l - m);
}
__device__ __forceinline__ void bs_merge(double& m, double& s, double m2, double s2) {
  if (!(s2 > 0.0)) return;
  if (m2 > m) {
    s = ldexp(s, bs_shift(m, m2)) + s2;
    m = m2;
  } else {
    s += ldexp(s2, bs_shift(m2, m));
  }
}

__device__ __forceinline__ int bs_class(int c, int C) { return c < 0 ? 0 : (c >= C ? C - 1 : c); }

// Block b of a pass over the grouped targets (k_bs_group's block starts): its class, false past
// the last block; and thread tid's grouped position in it.
__device__ __forceinline__ bool bs_block_class(const int* tab, int C, int b, int& c) {
  const int* bstart = tab + C + 1;
  if (b >= bstart[C]) return false;
  c = 0;
  while (c + 1 < C && b >= bstart[c + 1]) ++c;
  return true;
}
__device__ __forceinline__ long long bs_block_pos(const int* tab, int C, int b, int c, int tid) {
  return (long long)tab[c] + (long long)(b - tab[C + 1 + c]) * kBsB + tid;
}
template <int D>
__device__ __forceinline__ void bs_load_target(const double* Xt, const int* perm, long long pos, bool live, double (&x)[D]) {
  const long long j = live ? perm[pos] : 0;
#pragma unroll
  for (int q = 0; q < D; ++q) x[q] = live ? Xt[j * D + q] : 0.0;
}

// log2 of a_k f_kj: target x against the source record row = {mu[D], 1/v[D], g}
template <int D>
__device__ __forceinline__ double bs_pair_exponent(const double (&x)[D], const double* row) {
  double qd = 0.0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const double df = x[q] - row[q];
    qd = fma(df, df * row[D + q], qd);
  }
  return fma(qd, -kHalfLog2e, row[2 * D]);
}

// Sources [k0, k1) of one class's records through LDS, kBsTile at a time (every lane reads the
// same address: a broadcast), added to the thread's running sum in index order.  after(k, l, m, s)
// sees the sum behind source k, whose exponent was l; returning true ends the thread's part (it
// keeps the barriers).  Called by every thread of the block.
template <int D, class After>
__device__ __forceinline__ void bs_den_range(const double* rec, long long k0, long long k1, bool live,
                                             const double (&x)[D], double* tile, double& m, double& s, After after) {
  constexpr int R = 2 * D + 1;
  const int tid = threadIdx.x;
  for (long long kt = k0; kt < k1; kt += kBsTile) {
    const int rows = (int)(k1 - kt < kBsTile ? k1 - kt : kBsTile);
    for (int e = tid; e < rows * R; e += kBsB) tile[e] = rec[kt * R + e];
    __syncthreads();
    if (live) {
      for (int r = 0; r < rows; ++r) {
        const double l = bs_pair_exponent<D>(x, tile + r * R);
        bs_add(m, s, l);
        if (after(kt + r, l, m, s)) {
          live = false;
          break;
        }
      }
    }
    __syncthreads();
  }
}
#endif  // __HIPCC__

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
