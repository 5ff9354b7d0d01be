// Fixed-lag smoothing from particle ancestry (gpmdm_pf_smoothed, gpmdm_bank_smoothed): the
// genealogy smoother of Kitagawa (1996).  Every resample of a filter with smoothing on records its ancestors
// (ridx), classes and states into a ring of L + 1 frames; a read-out walks the ancestry of
// the particles the filter holds now back through the ring,
//   j_0 = p,  j_{l+1} = a_{t-l}[j_l],
// and reads the class fractions, the mean state and the number of distinct ancestors of the
// traced cloud {X_{t-l}[j_l(p)]} at every requested lag l (the pose of a lag is
// obs_readout.h's read-out pointed at that cloud).
//
// One set of kernels serves single filters and banks: a single filter is a bank of F = 1.
// Particles are filter-major (g = f * Pf + p) and ancestors are in-filter indices.
//   k_sm_record   one frame's {ridx, cls, X} into its slot of the ring (a plain copy of all
//                 F * Pf rows)
//   k_sm_trace    grid (ceil(Pf / 256), F), one thread per current particle: the dependent
//                 gathers l = 0..lag_last inside filter f's rows of each slot (clamped to
//                 [0, Pf)), and from lag_first on the class counts (integer atomics), per-block
//                 partial sums of the traced states (wave butterfly, then the waves in order),
//                 a mark per visited ancestor (plain byte store), and on request the rows
//   k_sm_reduce   grid (lags, F), one workgroup per (lag, filter): class fractions, the mean
//                 state from the blocks' partials in block order, the count of the marks
// Blocks are cut within a filter, so row f of a bank's result is bitwise the single filter's
// on f's history.  No floating-point atomics and no draws: the same ring gives bitwise the same
// read-out.
#pragma once
#include "common.h"
#include "pf_kernels.h"

namespace gpmdm {

// the ring: slot k holds the frame f with f mod n_slots = k
struct SmRing {
  const int* anc;                 // n_slots x P   ancestors (ridx) of the frame's resample (P = F * Pf)
  const int* cls;                 // n_slots x P   post-resample classes
  const double* X;                // n_slots x P x d post-resample states
  int n_slots;                    // L + 1
  int head;                       // the latest frame's slot
};

struct SmRecordArgs {
  long long P;                    // all F * Pf particles
  int d;
  const int* ridx;                // P
  const int* cls;                 // P
  const double* X;                // P x d
  int* anc_dst;                   // the slot's rows
  int* cls_dst;
  double* X_dst;
};

// rows q = (l - lag_first) * F + f of every output; mark rows are ld_marks bytes apart (a
// multiple of 16)
struct SmTraceArgs {
  long long Pf;
  int F, C, d;
  int lag_first, lag_last;        // 0 <= lag_first <= lag_last <= depth < n_slots
  SmRing ring;
  int* counts;                    // n x F x C         class counts (zeroed before the launch)
  double* partials;               // n x F x nbf x d   block sums of the traced states
  unsigned char* marks;           // n x F x ld_marks  1 at every visited ancestor (zeroed before)
  long long ld_marks;             // sm_ld_marks(Pf)
  int* anc_out;                   // n x F x Pf        j_l(p), in-filter, or nullptr
  int* cls_out;                   // n x F x Pf        or nullptr
  double* X_out;                  // n x F x Pf x d    the traced clouds, or nullptr
};

struct SmReduceArgs {
  long long Pf;
  int C, d, nbf;
  const int* counts;
  const double* partials;
  const unsigned char* marks;
  long long ld_marks;
  double* out;                    // n x F rows of ld_out: {class_prob[C], state_mean[d], distinct}
  int ld_out;
};

inline long long sm_blocks(long long P) { return (P + 255) / 256; }
inline long long sm_ld_marks(long long P) { return (P + 15) & ~15ll; }

void launch_sm_record(const SmRecordArgs& a, hipStream_t s);
void launch_sm_trace(const SmTraceArgs& a, hipStream_t s);
void launch_sm_reduce(const SmReduceArgs& a, int n_lags, int F, hipStream_t s);

}  // namespace gpmdm
