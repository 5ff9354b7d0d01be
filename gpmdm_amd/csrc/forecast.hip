// The forecast roll-out's O(P) kernels (forecast.h): switch, finish, per-filter sum and reduce.
#include "forecast.h"

namespace gpmdm {

constexpr int kB = 256;   // threads per block, as the filter's O(P) kernels

// The filter of bank-wide particle g.  A single filter (uniform: P == Pf) skips the 64-bit
// division: about 0.2 us of the launch-bound notebook-size roll-out step (DESIGN_APPENDIX.md,
// "One set of roll-out kernels").
__device__ __forceinline__ long long filter_of(long long g, long long P, long long Pf) {
  return P == Pf ? 0 : g / Pf;
}

// ---------------------------------------------------------------------------------
// k_switch (pf_kernels.hip) on the roll-out's classes: the same transform and first-maximum
// rule, the forecast stream's counters, no ownership order and no leader election.  Particle
// g = f * Pf + p draws with filter f's key and p in the counter.  Blocks span the whole bank
// (they may mix filters): their counts feed the bank-wide grouping only.
__global__ __launch_bounds__(kB) void k_fc_switch(FcSwitchArgs a) {
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < a.C) hist[tid] = 0;
  __syncthreads();
  const long long g = (long long)blockIdx.x * kB + tid;
  if (g < a.P) {
    const long long f = filter_of(g, a.P, a.Pf), p = g - f * a.Pf;
    const int best = switch_draw(a.T, a.C, a.cls[g], nullptr, 0, (unsigned)p, a.frame, kStreamForecastSwitch, a.h << 8,
                                 filter_key(a.seed_lo, a.seed_hi, f));
    a.cls_new[g] = best;
    atomicAdd(&hist[best], 1);
  }
  __syncthreads();
  if (tid < a.C) a.blockcounts[(long long)blockIdx.x * a.C + tid] = hist[tid];
}

// ---------------------------------------------------------------------------------
// k_dyn_finish's arithmetic on tile row o (= grouped position: every particle is evaluated):
// q from the column blocks' partials, vc = k(x, x) - q, x' = eps sqrt(vc il2) + mu, with the
// draws of the particle's own filter.  The new state goes to the particle's row of the next
// cloud; with a.partials (uniform: every thread reaches the wave sums) its block sum (wave
// butterflies, then the four waves in order) to partials[block], else the sums are k_fc_sum's.
__global__ __launch_bounds__(kB) void k_fc_finish(FcFinishArgs a) {
  __shared__ double red[kB / 64][kMaxD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long o = (long long)blockIdx.x * kB + tid;
  const bool live = o < a.P;
  const int d = a.d;
  long long g = 0, f = 0, p = 0;
  double vc = 0.0;
  if (live) {
    const int c = seg_of(a.seg_out_base, a.C, o);
    const long long pos = a.seg_pos_begin[c] + (o - a.seg_out_base[c]);
    g = a.perm[pos];
    f = filter_of(g, a.P, a.Pf);
    p = g - f * a.Pf;
    if (!a.mean_only) vc = dyn_vc(a.qpart, a.ld_q, a.n_parts[c], o, a.X + g * d, a.lin_c2, d);
  }
  for (int j = 0; j < d; j += 2) {
    double x0 = 0.0, x1 = 0.0;
    if (live) {
      double e0 = 0.0, e1 = 0.0;
      if (!a.mean_only) {
        // k_dyn_finish's Box-Muller pair, written out in both kernels: through a shared device
        // function this kernel took 98 VGPRs instead of 96 (occupancy 4 instead of 5)
        const uint4 r = philox4x32_10(
            make_uint4((unsigned)p, a.frame, kStreamForecastDyn, (a.h << 8) | (unsigned)(j >> 1)),
            filter_key(a.seed_lo, a.seed_hi, f));
        const double u1 = u01_oo(r.x, r.y), u2 = u01_co(r.z, r.w);
        const double rr = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincos(6.283185307179586476925 * u2, &sn, &cs);
        e0 = rr * cs;
        e1 = rr * sn;
      }
      const double m0 = a.mu[o * d + j];
      x0 = a.mean_only ? m0 : e0 * sqrt(vc * a.il2[j]) + m0;
      a.X_out[g * d + j] = x0;
      if (j + 1 < d) {
        const double m1 = a.mu[o * d + j + 1];
        x1 = a.mean_only ? m1 : e1 * sqrt(vc * a.il2[j + 1]) + m1;
        a.X_out[g * d + j + 1] = x1;
      }
    }
    if (a.partials) {
      const double s0 = wave_sum(x0), s1 = wave_sum(x1);
      if (lane == 0) {
        red[w][j] = s0;
        if (j + 1 < d) red[w][j + 1] = s1;
      }
    }
  }
  if (!a.partials) return;
  __syncthreads();
  if (tid < d) {
    double t = red[0][tid];
    for (int v = 1; v < kB / 64; ++v) t += red[v][tid];
    a.partials[(long long)blockIdx.x * d + tid] = t;
  }
}

// ---------------------------------------------------------------------------------
// Block (b, f): particles [256 b, 256 b + 256) of filter f, in particle order.  The class
// histogram goes through LDS to the block's own row (plain stores); the state sums through the
// wave butterflies and then the four waves in order.  Dead threads add zeros.
__global__ __launch_bounds__(kB) void k_fc_sum(FcSumArgs a) {
  __shared__ double red[kB / 64][kMaxD];
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long f = blockIdx.y, nbf = gridDim.x;
  const long long p = (long long)blockIdx.x * kB + tid;
  const bool live = p < a.Pf;
  const long long g = f * a.Pf + (live ? p : 0);
  const long long blk = f * nbf + blockIdx.x;
  if (a.cls) {
    if (tid < a.C) hist[tid] = 0;
    __syncthreads();
    if (live) {
      int c = a.cls[g];
      c = c < 0 ? 0 : (c >= a.C ? a.C - 1 : c);
      atomicAdd(&hist[c], 1);
    }
  }
  for (int k = 0; k < a.d; ++k) {
    const double s = wave_sum(live ? a.X[g * a.d + k] : 0.0);
    if (lane == 0) red[w][k] = s;
  }
  __syncthreads();
  if (tid < a.d) {
    double t = red[0][tid];
    for (int v = 1; v < kB / 64; ++v) t += red[v][tid];
    a.partials[blk * a.d + tid] = t;
  }
  if (a.cls && tid < a.C) a.bcounts[blk * a.C + tid] = hist[tid];
}

// ---------------------------------------------------------------------------------
// One workgroup per filter: class fractions from the filter's n_count_rows rows of integer
// counts (any order gives the same integer) and the mean state from the blocks' sums
// (thread-strided, wave butterfly, waves in order: k_sm_reduce's order), each divided once by Pf.
__global__ __launch_bounds__(kB) void k_fc_reduce(FcReduceArgs a) {
  __shared__ double red[kB / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long f = blockIdx.x;
  double* out = a.out + f * (a.C + a.d);
  if (tid < a.C) {
    long long n = 0;
    for (int b = 0; b < a.n_count_rows; ++b) n += a.counts[(f * a.n_count_rows + b) * a.C + tid];
    out[tid] = (double)n / (double)a.Pf;
  }
  const double* part = a.partials + f * a.nbf * a.d;
  for (int j = 0; j < a.d; ++j) {
    double s = 0.0;
    for (int b = tid; b < a.nbf; b += kB) s += part[(long long)b * a.d + j];
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (tid == 0) {
      double t = red[0];
      for (int v = 1; v < kB / 64; ++v) t += red[v];
      out[a.C + j] = t / (double)a.Pf;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------
static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_fc_switch(const FcSwitchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_switch, dim3(nblk(a.P, kB)), dim3(kB), 0, s, a);
}
void launch_fc_finish(const FcFinishArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_finish, dim3(nblk(a.P, kB)), dim3(kB), 0, s, a);
}
void launch_fc_sum(const FcSumArgs& a, int F, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_sum, dim3(nblk(a.Pf, kB), (unsigned)F), dim3(kB), 0, s, a);
}
void launch_fc_reduce(const FcReduceArgs& a, int F, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_reduce, dim3((unsigned)F), dim3(kB), 0, s, a);
}

}  // namespace gpmdm
