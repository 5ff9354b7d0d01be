// Backward simulation's kernels (backsample.h).
#include "backsample.h"

namespace gpmdm {

// ---------------------------------------------------------------------------------
// Pass 1.  k_bs_den with ranges of kFsRange sources: block b serves 256 grouped targets of one
// class, range blockIdx.y of that class's records goes through LDS.
template <int D>
__global__ __launch_bounds__(kBsB) void k_fs_sum(FsPassArgs a) {
  __shared__ double tile[kBsTile * (2 * D + 1)];
  int c;
  if (!bs_block_class(a.tab, a.C, blockIdx.x, c)) return;   // (uniform over the block)
  const long long pos = bs_block_pos(a.tab, a.C, blockIdx.x, c, threadIdx.x);
  const bool live = pos < a.tab[c + 1];
  double x[D];
  bs_load_target<D>(a.Xt, a.perm, pos, live, x);
  const long long k0 = (long long)blockIdx.y * kFsRange;
  const long long k1 = k0 + kFsRange < a.n_s ? k0 + kFsRange : a.n_s;
  double m = -INFINITY, s = 0.0;
  bs_den_range<D>(a.rec + (long long)c * a.n_s * (2 * D + 1), k0, k1, live, x, tile, m, s,
                  [](long long, double, double, double) { return false; });
  if (live) {
    double* out = a.part + (long long)blockIdx.y * a.n_t + pos;    // the m plane, then the s plane
    out[0] = m;
    out[(long long)a.n_ranges * a.n_t] = s;
  }
}

// ---------------------------------------------------------------------------------
// Per target: D and log_den, the threshold, the range it falls in and what is left of it there.
__global__ __launch_bounds__(kBsB) void k_fs_pick(FsPassArgs a) {
  const long long pos = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (pos >= a.n_t) return;
  const long long plane = (long long)a.n_ranges * a.n_t;
  double M = -INFINITY, S = 0.0;
  for (int r = 0; r < a.n_ranges; ++r) {
    const double* p = a.part + (long long)r * a.n_t + pos;
    bs_merge(M, S, p[0], p[plane]);
  }
  const long long j = a.perm[pos];
  const bool reached = S > 0.0;
  if (a.log_den) a.log_den[j] = reached ? (M + log2(S)) * kLn2 : -INFINITY;
  if (!reached) {
    a.range[pos] = -1;
    a.idx[j] = -1;
    return;
  }
  const double t = __dmul_rn(a.u[j], S);           // the threshold in the scale 2^M
  double Mp = -INFINITY, Sp = 0.0, res = INFINITY;
  int chosen = -1, last = -1;
  for (int r = 0; r < a.n_ranges; ++r) {
    const double* p = a.part + (long long)r * a.n_t + pos;
    const double m2 = p[0], s2 = p[plane];
    if (!(s2 > 0.0)) continue;                     // (bs_merge skips it)
    last = r;
    const double M0 = Mp, S0 = Sp;
    bs_merge(Mp, Sp, m2, s2);
    // Mp <= M: the prefix in the scale 2^M is exact
    if (t == 0.0 || ldexp(Sp, bs_shift(Mp, M)) > t) {
      chosen = r;
      res = t - ldexp(S0, bs_shift(M0, M));
      break;
    }
  }
  a.range[pos] = chosen >= 0 ? chosen : last;      // (no crossing by rounding: the last source of positive term)
  a.res[pos] = res;
  a.scale[pos] = M;
}

// ---------------------------------------------------------------------------------
// Pass 2.  The chosen range's running sum once more, up to the crossing.
template <int D>
__global__ __launch_bounds__(kBsB) void k_fs_select(FsPassArgs a) {
  __shared__ double tile[kBsTile * (2 * D + 1)];
  int c;
  if (!bs_block_class(a.tab, a.C, blockIdx.x, c)) return;   // (uniform over the block)
  const long long pos = bs_block_pos(a.tab, a.C, blockIdx.x, c, threadIdx.x);
  const bool live = pos < a.tab[c + 1] && a.range[pos] == (int)blockIdx.y;
  if (!__syncthreads_or(live)) return;             // none of the block's targets chose this range
  double x[D];
  bs_load_target<D>(a.Xt, a.perm, pos, live, x);
  const double res = live ? a.res[pos] : 0.0, M = live ? a.scale[pos] : 0.0;
  const long long k0 = (long long)blockIdx.y * kFsRange;
  const long long k1 = k0 + kFsRange < a.n_s ? k0 + kFsRange : a.n_s;
  double m = -INFINITY, s = 0.0;
  long long found = -1, last = -1;
  bs_den_range<D>(a.rec + (long long)c * a.n_s * (2 * D + 1), k0, k1, live, x, tile, m, s,
                  [&](long long k, double l, double mk, double sk) {
                    if (!(l > -INFINITY)) return false;      // a term of weight zero is no candidate
                    last = k;
                    if (sk > 0.0 && (res <= 0.0 || ldexp(sk, bs_shift(mk, M)) > res)) {
                      found = k;
                      return true;
                    }
                    return false;
                  });
  if (live) a.idx[a.perm[pos]] = (int)(found >= 0 ? found : last);
}

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBsB) void k_fs_draw(FsDrawArgs a) {
  const long long e = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (e >= (long long)(a.lag + 1) * a.n) return;
  const long long l = e / a.n, m = e - l * a.n;
  const uint4 r = philox4x32_10(make_uint4((unsigned)m, a.frame, kStreamBackSample, (unsigned)l),
                                filter_key(a.seed_lo, a.seed_hi, 0));
  const double u = u01_co(r.x, r.y);
  a.u[e] = u;
  if (l == 0) {
    const long long j = (long long)(u * (double)a.P);
    a.idx0[m] = (int)(j < a.P - 1 ? j : a.P - 1);
  }
}

// thread (m, q): q < d a coordinate of the state, q = d the class
__global__ __launch_bounds__(kBsB) void k_fs_gather(FsGatherArgs a) {
  const long long e = (long long)blockIdx.x * kBsB + threadIdx.x;
  const int w = a.d + 1;
  if (e >= a.n * w) return;
  const long long m = e / w;
  const int q = (int)(e - m * w);
  const long long j = a.idx[m];
  if (q < a.d) a.X_out[m * a.d + q] = j >= 0 ? a.X[j * a.d + q] : NAN;
  else if (a.cls_out) a.cls_out[m] = j >= 0 ? a.cls[j] : -1;
}

__global__ __launch_bounds__(kBsB) void k_fs_flag(const int* idx, long long n, int* flag) {
  const long long m = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (m < n) flag[m] = idx[m] >= 0;
}

// ---------------------------------------------------------------------------------
// Two-term sums (Knuth's two-sum; hi + lo carries the sum to about 2^-106).
__device__ __forceinline__ void fs_dd_merge(double& hi, double& lo, double h2, double l2) {
  const double s = hi + h2;
  const double bb = s - hi;
  const double e = (hi - (s - bb)) + (h2 - bb);
  hi = s;
  lo = (lo + l2) + e;
}

// One workgroup: quantity after quantity, thread-strided sums, wave butterfly, the waves in order.
__global__ __launch_bounds__(kBsB) void k_fs_reduce(FsReduceArgs a) {
  __shared__ double red[2][kBsB / 64];
  __shared__ int redi[kBsB / 64];
  __shared__ double row[2 + kMaxClasses + 64];     // (d <= 32: host_image.h)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int C = a.C, d = a.d;
  // integers: alive, distinct, the class counts
  for (int qn = 0; qn < C + 2; ++qn) {
    int cnt = 0;
    for (long long i = tid; i < a.n; i += kBsB) {
      const int j = a.idx[i];
      if (j < 0) continue;
      if (qn == 0) cnt += 1;
      else if (qn == 1) cnt += atomicOr(&a.mark[j], 1) == 0;
      else cnt += bs_class(a.cls[i], C) == qn - 2;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) redi[w] = cnt;
    __syncthreads();
    if (tid == 0) {
      int t = redi[0];
      for (int v = 1; v < kBsB / 64; ++v) t += redi[v];
      row[qn] = (double)t;
    }
    __syncthreads();
    if (qn == 1)                                    // (every mark was set before the barrier)
      for (long long i = tid; i < a.n; i += kBsB) {
        const int j = a.idx[i];
        if (j >= 0) a.mark[j] = 0;
      }
  }
  for (int q = 0; q < d; ++q) {
    double hi = 0.0, lo = 0.0;
    for (long long i = tid; i < a.n; i += kBsB)
      if (a.idx[i] >= 0) fs_dd_merge(hi, lo, a.X[i * d + q], 0.0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double h2 = __shfl_xor(hi, off), l2 = __shfl_xor(lo, off);
      fs_dd_merge(hi, lo, h2, l2);
    }
    if (lane == 0) {
      red[0][w] = hi;
      red[1][w] = lo;
    }
    __syncthreads();
    if (tid == 0) {
      double th = red[0][0], tl = red[1][0];
      for (int v = 1; v < kBsB / 64; ++v) fs_dd_merge(th, tl, red[0][v], red[1][v]);
      row[2 + C + q] = th;
      row[2 + C + d + q] = tl;
    }
    __syncthreads();
  }
  // (one 8-byte store per thread: no wide store, tests/test_isa_guard.py)
  if (tid < 2 + C + 2 * d) a.out[tid] = row[tid];
}

// ---------------------------------------------------------------------------------
static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

template <int D>
static void launch_passes(const FsPassArgs& a, bool select, hipStream_t s) {
  const dim3 grid(nblk(a.n_t, kBsB) + a.C, (unsigned)a.n_ranges);
  if (select) hipLaunchKernelGGL(k_fs_select<D>, grid, dim3(kBsB), 0, s, a);
  else hipLaunchKernelGGL(k_fs_sum<D>, grid, dim3(kBsB), 0, s, a);
}
static void launch_pass(const FsPassArgs& a, bool select, hipStream_t s) {
  switch (a.d) {
#define GPMDM_D(n) case n: launch_passes<n>(a, select, s); break;
    GPMDM_D(1) GPMDM_D(2) GPMDM_D(3) GPMDM_D(4) GPMDM_D(5) GPMDM_D(6) GPMDM_D(7) GPMDM_D(8)
    GPMDM_D(9) GPMDM_D(10) GPMDM_D(11) GPMDM_D(12) GPMDM_D(13) GPMDM_D(14) GPMDM_D(15) GPMDM_D(16)
    GPMDM_D(24) GPMDM_D(32)
#undef GPMDM_D
    default: break;   // (a model's d is one of these: host_image.h)
  }
}
void launch_fs_sum(const FsPassArgs& a, hipStream_t s) { launch_pass(a, false, s); }
void launch_fs_select(const FsPassArgs& a, hipStream_t s) { launch_pass(a, true, s); }
void launch_fs_pick(const FsPassArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fs_pick, dim3(nblk(a.n_t, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_fs_draw(const FsDrawArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fs_draw, dim3(nblk((long long)(a.lag + 1) * a.n, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_fs_gather(const FsGatherArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fs_gather, dim3(nblk(a.n * (a.d + 1), kBsB)), dim3(kBsB), 0, s, a);
}
void launch_fs_flag(const int* idx, long long n, int* flag, hipStream_t s) {
  hipLaunchKernelGGL(k_fs_flag, dim3(nblk(n, kBsB)), dim3(kBsB), 0, s, idx, n, flag);
}
void launch_fs_reduce(const FsReduceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_fs_reduce, dim3(1), dim3(kBsB), 0, s, a);
}

}  // namespace gpmdm
