// The fixed-lag smoother's kernels (smooth.h): record, trace, per-lag reduce.
#include "smooth.h"

namespace gpmdm {

constexpr int kB = 256;   // threads per block (four wave64s), as the filter's O(P) kernels

// ---------------------------------------------------------------------------------
// One frame into its slot: thread i copies state value i, and ancestor / class i while i < P.
__global__ __launch_bounds__(kB) void k_sm_record(SmRecordArgs a) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i < a.P * a.d) a.X_dst[i] = a.X[i];
  if (i < a.P) {
    a.anc_dst[i] = a.ridx[i];
    a.cls_dst[i] = a.cls[i];
  }
}

// ---------------------------------------------------------------------------------
// Thread p of filter f = blockIdx.y walks its ancestry through filter f's rows of each slot
// (every index in-filter); the block moves through the lags together (the same trip count
// for every thread, dead threads included: they add zeros), so each lag's class counts go
// through a block histogram in LDS to one integer atomic per class and block, and its state
// sums through the wave butterflies and then the four waves in order to partials[row][block].
__global__ __launch_bounds__(kB) void k_sm_trace(SmTraceArgs a) {
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
        j = n < 0 ? 0 : (n >= a.Pf ? a.Pf - 1 : n);   // (ridx is in [0, Pf): never a wild gather)
      }
      slot = slot == 0 ? ns - 1 : slot - 1;
    }
  }
}

// ---------------------------------------------------------------------------------
// One workgroup per (lag, filter), row q = lag row * F + f: class fractions (the count divided
// once by Pf), the mean state from the blocks' sums (thread-strided, wave butterfly, waves in order: k_fc_reduce's order), and
// the number of marks (bytes of 0 / 1, four to a word: their sum is the word's popcount).
__global__ __launch_bounds__(kB) void k_sm_reduce(SmReduceArgs a) {
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

void launch_sm_record(const SmRecordArgs& a, hipStream_t s) {
  const long long n = a.P * (a.d > 1 ? a.d : 1);
  hipLaunchKernelGGL(k_sm_record, dim3(nblk(n, kB)), dim3(kB), 0, s, a);
}
void launch_sm_trace(const SmTraceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_sm_trace, dim3(nblk(a.Pf, kB), (unsigned)a.F), dim3(kB), 0, s, a);
}
void launch_sm_reduce(const SmReduceArgs& a, int n_lags, int F, hipStream_t s) {
  hipLaunchKernelGGL(k_sm_reduce, dim3((unsigned)n_lags, (unsigned)F), dim3(kB), 0, s, a);
}

}  // namespace gpmdm
