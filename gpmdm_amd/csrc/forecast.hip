// The forecast roll-out's O(P) kernels (forecast.h): switch, finish, per-horizon reduce.
#include "forecast.h"

namespace gpmdm {

constexpr int kB = 256;   // threads per block, as the filter's O(P) kernels

// ---------------------------------------------------------------------------------
// k_switch (pf_kernels.hip) on the roll-out's classes: the same transform and first-maximum
// rule, the forecast stream's counters, no ownership order and no leader election.
__global__ __launch_bounds__(kB) void k_fc_switch(FcSwitchArgs a) {
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < a.C) hist[tid] = 0;
  __syncthreads();
  const long long p = (long long)blockIdx.x * kB + tid;
  if (p < a.P) {
    const int c0 = a.cls[p];
    const uint2 key = filter_key(a.seed_lo, a.seed_hi, 0);
    int best = 0;
    double bestv = -INFINITY;
    for (int j = 0; j < a.C; j += 2) {
      const uint4 r = philox4x32_10(
          make_uint4((unsigned)p, a.frame, kStreamForecastSwitch, (a.h << 8) | (unsigned)(j >> 1)), key);
      const double e0 = -log(u01_oo(r.x, r.y));
      const double e1 = -log(u01_oo(r.z, r.w));
      const double v0 = a.T[c0 * a.C + j] / e0;
      if (v0 > bestv) { bestv = v0; best = j; }
      if (j + 1 < a.C) {
        const double v1 = a.T[c0 * a.C + j + 1] / e1;
        if (v1 > bestv) { bestv = v1; best = j + 1; }
      }
    }
    a.cls_new[p] = best;
    atomicAdd(&hist[best], 1);
  }
  __syncthreads();
  if (tid < a.C) a.blockcounts[(long long)blockIdx.x * a.C + tid] = hist[tid];
}

// ---------------------------------------------------------------------------------
// k_dyn_finish's arithmetic on tile row o (= grouped position: every particle is evaluated):
// q from the column blocks' partials, vc = k(x, x) - q, x' = eps sqrt(vc il2) + mu.  The new
// state goes to the particle's row of the next cloud; its block sum (wave butterflies, then
// the four waves in order) to partials[block].
__global__ __launch_bounds__(kB) void k_fc_finish(FcFinishArgs a) {
  __shared__ double red[kB / 64][kMaxD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long o = (long long)blockIdx.x * kB + tid;
  const bool live = o < a.P;
  const int d = a.d;
  long long p = 0;
  double vc = 0.0;
  if (live) {
    int c = 0;
    for (int s = 1; s < a.C; ++s)
      if (o >= a.seg_out_base[s]) c = s;
    const long long pos = a.seg_pos_begin[c] + (o - a.seg_out_base[c]);
    p = a.perm[pos];
    if (!a.mean_only) {
      double q = 0.0;
      const int np = a.n_parts[c];
      for (int k = 0; k < np; ++k) q += a.qpart[(long long)k * a.ld_q + o];
      double kd = 0.0;
      for (int j = 0; j < d; ++j) {
        const double x = a.X[p * d + j];
        kd = fma(a.lin_c2[j] * x, x, kd);
      }
      kd = 1.0 + (kd + a.lin_c2[d]);
      vc = kd - q;
    }
  }
  for (int j = 0; j < d; j += 2) {
    double x0 = 0.0, x1 = 0.0;
    if (live) {
      double e0 = 0.0, e1 = 0.0;
      if (!a.mean_only) {
        const uint4 r = philox4x32_10(
            make_uint4((unsigned)p, a.frame, kStreamForecastDyn, (a.h << 8) | (unsigned)(j >> 1)),
            filter_key(a.seed_lo, a.seed_hi, 0));
        const double u1 = u01_oo(r.x, r.y), u2 = u01_co(r.z, r.w);
        const double rr = sqrt(-2.0 * log(u1));
        double sn, cs;
        sincos(6.283185307179586476925 * u2, &sn, &cs);
        e0 = rr * cs;
        e1 = rr * sn;
      }
      const double m0 = a.mu[o * d + j];
      x0 = a.mean_only ? m0 : e0 * sqrt(vc * a.il2[j]) + m0;
      a.X_out[p * d + j] = x0;
      if (j + 1 < d) {
        const double m1 = a.mu[o * d + j + 1];
        x1 = a.mean_only ? m1 : e1 * sqrt(vc * a.il2[j + 1]) + m1;
        a.X_out[p * d + j + 1] = x1;
      }
    }
    const double s0 = wave_sum(x0), s1 = wave_sum(x1);
    if (lane == 0) {
      red[w][j] = s0;
      if (j + 1 < d) red[w][j + 1] = s1;
    }
  }
  __syncthreads();
  if (tid < d) {
    double t = red[0][tid];
    for (int v = 1; v < kB / 64; ++v) t += red[v][tid];
    a.partials[(long long)blockIdx.x * d + tid] = t;
  }
}

// ---------------------------------------------------------------------------------
// One workgroup per horizon step: class fractions from the grouping's counts, and the mean
// state from the blocks' sums (thread-strided, wave butterfly, waves in order).
__global__ __launch_bounds__(kB) void k_fc_reduce(FcReduceArgs a) {
  __shared__ double red[kB / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < a.C) a.out[tid] = (double)a.counts[tid] / (double)a.P;
  for (int j = 0; j < a.d; ++j) {
    double s = 0.0;
    for (int b = tid; b < a.nb; b += kB) s += a.partials[(long long)b * a.d + j];
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (tid == 0) {
      double t = red[0];
      for (int v = 1; v < kB / 64; ++v) t += red[v];
      a.out[a.C + j] = t / (double)a.P;
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
void launch_fc_reduce(const FcReduceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_reduce, dim3(1), dim3(kB), 0, s, a);
}

}  // namespace gpmdm
