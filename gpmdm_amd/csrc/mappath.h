// MAP trajectory decoding (gpmdm_map_step, gpmdm_pf_map_path): the particle Viterbi recursion
// (Godsill, Doucet & West 2001) over the clouds the ancestry ring of smooth.h holds, with the
// filter's proposal as transition density -- backsmooth.h's log f_kj, the pair exponent of
// k_bs_den.  One step takes sources {x_k, c_k} with scores delta_k and targets {x'_j, c'_j} with
// observation log-likelihoods l_j and computes
//   delta'_j = l_j + max_k [delta_k + log f_kj],   psi_j = the lowest k attaining the maximum
// (psi_j = -1 and delta'_j = -inf when no source reaches j or l_j is not finite; a NaN candidate
// never wins).  The pair exponents are base-2 logarithms, as backsmooth's; delta and l are natural
// logarithms and enter the source record through one multiplication by log2 e.
// A maximum has no summation order, and copies of a resampled particle are bitwise-equal
// candidates: over a slot of the ring the recursion runs on the slot's leaders -- per distinct
// resampling ancestor the copy of lowest index, in increasing index -- and gives the bits and the
// back-pointers of the recursion over all P rows.  The leaders' count is known on the device
// only: every kernel below takes a host row count and, when n_dev is set, reads the real one
// there (its grid is sized by the host's upper bound; the surplus blocks leave at once).
//   k_mp_owner    owner[a_i] = min i: an integer atomicMin, order-free (owner preset to INT_MAX)
//   k_mp_compact  one workgroup: leader flags (owner[a_i] == i) and their stable compaction in
//                 index order -- rows[r] -> particle, rank[i] = r of a leader, the count
//   k_mp_lead     lead[i] = rank[owner[a_i]]: every particle's compact row
//   k_mp_iota     a slot without recorded ancestors: the identity
//   k_mp_gather   the compacted {x, c} (and l) of a slot; rows past the count are zeroed
//   k_mp_seg_table  the dynamics tiles' segment table from the device count: launch_predict_dyn
//                 then runs the tiles of the real rows only
//   k_mp_moments  k_bs_moments with a log-domain addend: the record's g = log2 T[c_k, c] -
//                 d/2 log2 2 pi - 1/2 sum_q log2 v_q + delta_k log2 e, -inf when unusable
//   k_mp_max      k_bs_den's layout (targets across threads in k_bs_group's order, the class's
//                 source records through LDS 64 at a time, gridDim.y ranges of the sources): per
//                 pair the same quadratic form and exponent fma, compared with a strict > in
//                 increasing source index, so the lowest index of a range wins; value and index
//                 go to separate planes
//   k_mp_fin      the ranges in range order with a strict >; + l; delta' by compact row, psi as
//                 the source leader's particle index
//   k_mp_expand   delta' and psi to all P particles: a copy reads its leader's row
//   k_mp_back     one workgroup: argmax of delta_0 with the lowest index (thread-strided, wave
//                 butterfly on (value, index), the waves in order), one thread walks psi, then
//                 the path's index, class, score, compact size and state per lag
// No floating-point atomics; ties go to the lowest index everywhere: the same inputs give the
// same bits.
#pragma once
#include "backsmooth.h"

namespace gpmdm {

struct MpLeadArgs {
  long long P;
  const int* anc;                 // P resampling ancestors of the slot
  int* owner;                     // P
  int* rank;                      // P
  int* rows;                      // P   compact row -> particle
  int* lead;                      // P   particle -> compact row
  int* count;                     // 1   the compact size
};

struct MpGatherArgs {
  long long n;                    // rows of the output (upper bound)
  int d;
  const int* n_dev;               // the real row count, or nullptr: n
  const int* rows;                // compact row -> particle, or nullptr: the identity
  const double* X;                // the slot's states
  const int* cls;
  const double* ll;               // the slot's log-likelihoods, or nullptr
  double* X_out;                  // n x d
  int* cls_out;                   // n
  double* ll_out;                 // n, or nullptr
};

struct MpMomentArgs {
  long long n;                    // sources (upper bound; the records' leading dimension)
  const int* n_dev;
  int C, d, c;                    // c: the class whose records are written
  const double* mu;               // n x d   dynamics mean of class c at source k
  const double* var;              // n x d   ... variance
  const int* cls;                 // n
  const double* delta;            // n natural logarithms, or nullptr: zeros
  const double* T;                // C x C
  double* rec;                    // C x n x (2 d + 1)
};

struct MpMaxArgs {
  long long n_s, n_t;             // upper bounds (n_s: the records' leading dimension)
  const int* ns_dev;              // the real source count, or nullptr
  int C, d, split;
  const double* rec;              // C x n_s x (2 d + 1)
  const double* Xt;               // n_t x d
  const int* perm;                // n_t   grouped position -> target
  const int* tab;                 // k_bs_group's tables
  double* val;                    // split x n_t: the ranges' maxima, by grouped position
  int* idx;                       // split x n_t: their source rows (-1: none)
};

struct MpFinArgs {
  long long n_t;                  // upper bound, the planes' leading dimension
  const int* nt_dev;
  int split;
  const double* val;
  const int* idx;
  const int* perm;
  const double* ll;               // n_t by target row, or nullptr: zeros
  const int* src_rows;            // source row -> particle, or nullptr: the identity
  double* delta;                  // n_t by target row (natural logarithm)
  int* psi;                       // n_t by target row
};

struct MpExpandArgs {
  long long P;
  const int* lead;                // particle -> compact row, or nullptr: the identity
  const double* delta_c;
  const int* psi_c;               // or nullptr (the root)
  double* delta;                  // P
  int* psi;                       // P, or nullptr
};

struct MpBackArgs {
  long long P;
  int d, lag;                     // the window: lags 0..lag
  int n_slots, slot;              // the ring: slot of lag l = (slot - l) mod n_slots
  const double* ring_X;
  const int* ring_cls;
  const double* delta;            // (lag + 1) x P
  const int* psi;                 // lag x P
  const int* count;               // lag + 1 compact sizes
  double* out;                    // (lag + 1) x (d + 4) {index, class, score, distinct, state[d]}, then log_joint
};

constexpr int kMpMaxLag = 4096;   // (GPMDM_SMOOTH_MAX_LAG: the walk's path lives in LDS)

void launch_mp_leaders(const MpLeadArgs& a, bool has_anc, hipStream_t s);
void launch_mp_gather(const MpGatherArgs& a, hipStream_t s);
void launch_mp_moments(const MpMomentArgs& a, hipStream_t s);
void launch_mp_max(const MpMaxArgs& a, hipStream_t s);
void launch_mp_fin(const MpFinArgs& a, hipStream_t s);
void launch_mp_expand(const MpExpandArgs& a, hipStream_t s);
void launch_mp_back(const MpBackArgs& a, hipStream_t s);
void launch_mp_seg_table(int* t, const int* n_dev, int n_max, int pt, hipStream_t s);
void launch_mp_ll_record(const double* ll, const int* ridx, long long P, double* dst, hipStream_t s);

}  // namespace gpmdm
