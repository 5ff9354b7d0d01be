// The bank variants of the roll-out's and the smoother's O(P) kernels (bank_rollout.h).
#include "bank_rollout.h"

namespace gpmdm {

constexpr int kB = 256;   // threads per block (four wave64s), as the filter's O(P) kernels

// ---------------------------------------------------------------------------------
// k_fc_switch over the bank's particles g = f * Pf + p: filter f's key, p in the counter.
// Blocks are bank-wide (they may mix filters): their counts feed the bank-wide grouping only.
__global__ __launch_bounds__(kB) void k_fcb_switch(FcbSwitchArgs a) {
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < a.C) hist[tid] = 0;
  __syncthreads();
  const long long g = (long long)blockIdx.x * kB + tid;
  if (g < a.P) {
    const long long f = g / a.Pf, p = g - f * a.Pf;
    const int c0 = a.cls[g];
    const uint2 key = filter_key(a.seed_lo, a.seed_hi, f);
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
    a.cls_new[g] = best;
    atomicAdd(&hist[best], 1);
  }
  __syncthreads();
  if (tid < a.C) a.blockcounts[(long long)blockIdx.x * a.C + tid] = hist[tid];
}

// ---------------------------------------------------------------------------------
// k_fc_finish's arithmetic on tile row o (grouped order over the whole bank), with the draws of
// the particle's own filter.  The sums of the new cloud are k_fcb_sum's: a block here mixes
// filters.
__global__ __launch_bounds__(kB) void k_fcb_finish(FcbFinishArgs a) {
  const long long o = (long long)blockIdx.x * kB + threadIdx.x;
  if (o >= a.P) return;
  const int d = a.d;
  int c = 0;
  for (int s = 1; s < a.C; ++s)
    if (o >= a.seg_out_base[s]) c = s;
  const long long pos = a.seg_pos_begin[c] + (o - a.seg_out_base[c]);
  const long long g = a.perm[pos];
  const long long f = g / a.Pf, p = g - f * a.Pf;
  double vc = 0.0;
  if (!a.mean_only) {
    double q = 0.0;
    const int np = a.n_parts[c];
    for (int k = 0; k < np; ++k) q += a.qpart[(long long)k * a.ld_q + o];
    double kd = 0.0;
    for (int j = 0; j < d; ++j) {
      const double x = a.X[g * d + j];
      kd = fma(a.lin_c2[j] * x, x, kd);
    }
    kd = 1.0 + (kd + a.lin_c2[d]);
    vc = kd - q;
  }
  const uint2 key = filter_key(a.seed_lo, a.seed_hi, f);
  for (int j = 0; j < d; j += 2) {
    double e0 = 0.0, e1 = 0.0;
    if (!a.mean_only) {
      const uint4 r = philox4x32_10(
          make_uint4((unsigned)p, a.frame, kStreamForecastDyn, (a.h << 8) | (unsigned)(j >> 1)), key);
      const double u1 = u01_oo(r.x, r.y), u2 = u01_co(r.z, r.w);
      const double rr = sqrt(-2.0 * log(u1));
      double sn, cs;
      sincos(6.283185307179586476925 * u2, &sn, &cs);
      e0 = rr * cs;
      e1 = rr * sn;
    }
    const double m0 = a.mu[o * d + j];
    a.X_out[g * d + j] = a.mean_only ? m0 : e0 * sqrt(vc * a.il2[j]) + m0;
    if (j + 1 < d) {
      const double m1 = a.mu[o * d + j + 1];
      a.X_out[g * d + j + 1] = a.mean_only ? m1 : e1 * sqrt(vc * a.il2[j + 1]) + m1;
    }
  }
}

// ---------------------------------------------------------------------------------
// Block (b, f): particles [256 b, 256 b + 256) of filter f, in particle order.  The class
// histogram goes through LDS to the block's own row (plain stores); the state sums through the
// wave butterflies and then the four waves in order.  Dead threads add zeros.
__global__ __launch_bounds__(kB) void k_fcb_sum(FcbSumArgs a) {
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
// One workgroup per filter: class fractions from the blocks' integer counts (any order gives
// the same integer) and the mean state from the blocks' sums (thread-strided, wave butterfly,
// waves in order: k_sm_reduce's order), each divided once by Pf.
__global__ __launch_bounds__(kB) void k_fcb_reduce(FcbReduceArgs a) {
  __shared__ double red[kB / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long f = blockIdx.x;
  double* out = a.out + f * (a.C + a.d);
  if (tid < a.C) {
    long long n = 0;
    for (int b = 0; b < a.nbf; ++b) n += a.bcounts[(f * a.nbf + b) * a.C + tid];
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
// k_sm_trace inside filter f = blockIdx.y: thread p walks its ancestry through filter f's rows
// of each slot; every index is in-filter and clamped to [0, Pf), so no gather leaves them.
__global__ __launch_bounds__(kB) void k_smb_trace(SmbTraceArgs a) {
  __shared__ double red[kB / 64][kMaxD];
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long f = blockIdx.y, nbf = gridDim.x;
  const long long p = (long long)blockIdx.x * kB + tid;
  const bool live = p < a.Pf;
  const int d = a.d, ns = a.ring.n_slots;
  const long long P = a.Pf * a.F;
  long long j = live ? p : 0;
  int slot = a.ring.head;
  for (int l = 0; l <= a.lag_last; ++l) {
    const long long row = (long long)slot * P + f * a.Pf;
    if (l >= a.lag_first) {
      const long long q = (long long)(l - a.lag_first) * a.F + f;
      if (tid < a.C) hist[tid] = 0;
      __syncthreads();
      if (live) {
        int c = a.ring.cls[row + j];
        c = c < 0 ? 0 : (c >= a.C ? a.C - 1 : c);
        atomicAdd(&hist[c], 1);
        a.marks[q * a.ld_marks + j] = 1;
        if (a.anc_out) a.anc_out[q * a.Pf + p] = (int)j;
        if (a.cls_out) a.cls_out[q * a.Pf + p] = c;
      }
      for (int k = 0; k < d; ++k) {
        const double x = live ? a.ring.X[(row + j) * d + k] : 0.0;
        if (live && a.X_out) a.X_out[(q * a.Pf + p) * d + k] = x;
        const double s = wave_sum(x);
        if (lane == 0) red[w][k] = s;
      }
      __syncthreads();
      if (tid < d) {
        double t = red[0][tid];
        for (int v = 1; v < kB / 64; ++v) t += red[v][tid];
        a.partials[(q * nbf + blockIdx.x) * d + tid] = t;
      }
      if (tid < a.C && hist[tid]) atomicAdd(&a.counts[q * a.C + tid], hist[tid]);
      __syncthreads();
    }
    if (l < a.lag_last) {
      if (live) {
        const long long n = a.ring.anc[row + j];
        j = n < 0 ? 0 : (n >= a.Pf ? a.Pf - 1 : n);
      }
      slot = slot == 0 ? ns - 1 : slot - 1;
    }
  }
}

// ---------------------------------------------------------------------------------
// k_sm_reduce per (lag, filter): row q = lag row * F + f.
__global__ __launch_bounds__(kB) void k_smb_reduce(SmbReduceArgs a) {
  __shared__ double red[kB / 64];
  __shared__ unsigned long long cnt[kB / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long q = (long long)blockIdx.x * gridDim.y + blockIdx.y;
  double* out = a.out + q * a.ld_out;
  if (tid < a.C) out[tid] = (double)a.counts[q * a.C + tid] / (double)a.Pf;
  const double* part = a.partials + q * a.nbf * a.d;
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
  const uint4* m = reinterpret_cast<const uint4*>(a.marks + q * a.ld_marks);   // rows are 16-byte multiples
  unsigned long long n = 0;
  for (long long i = tid; i < a.ld_marks / 16; i += kB) {
    const uint4 v = m[i];
    n += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
  if (lane == 0) cnt[w] = n;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (int v = 0; v < kB / 64; ++v) t += cnt[v];
    out[a.C + a.d] = (double)t;
  }
}

// ---------------------------------------------------------------------------------
static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_fcb_switch(const FcbSwitchArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fcb_switch, dim3(nblk(a.P, kB)), dim3(kB), 0, s, a);
}
void launch_fcb_finish(const FcbFinishArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fcb_finish, dim3(nblk(a.P, kB)), dim3(kB), 0, s, a);
}
void launch_fcb_sum(const FcbSumArgs& a, int F, hipStream_t s) {
  hipLaunchKernelGGL(k_fcb_sum, dim3(nblk(a.Pf, kB), (unsigned)F), dim3(kB), 0, s, a);
}
void launch_fcb_reduce(const FcbReduceArgs& a, int F, hipStream_t s) {
  hipLaunchKernelGGL(k_fcb_reduce, dim3((unsigned)F), dim3(kB), 0, s, a);
}
void launch_smb_trace(const SmbTraceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_smb_trace, dim3(nblk(a.Pf, kB), (unsigned)a.F), dim3(kB), 0, s, a);
}
void launch_smb_reduce(const SmbReduceArgs& a, int n_lags, int F, hipStream_t s) {
  hipLaunchKernelGGL(k_smb_reduce, dim3((unsigned)n_lags, (unsigned)F), dim3(kB), 0, s, a);
}

}  // namespace gpmdm
