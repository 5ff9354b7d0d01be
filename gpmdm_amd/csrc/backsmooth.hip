// The marginal backward smoother's kernels (backsmooth.h).
#include "backsmooth.h"

namespace gpmdm {

constexpr double kLog2TwoPi = 2.6514961294723187980;    // log2 (2 pi)
constexpr int kGroupB = 1024;

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBsB) void k_bs_moments(BsMomentArgs a) {
  const long long k = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (k >= a.n) return;
  const int d = a.d, c = a.c;
  const double* mu = a.mu + k * d;
  const double* var = a.var + k * d;
  double* rec = a.rec + ((long long)c * a.n + k) * (2 * d + 1);
  bool ok = true;
  double lv = 0.0;
  for (int q = 0; q < d; ++q) {
    const double v = var[q];
    ok = ok && v > 0.0 && v < INFINITY;
    rec[q] = mu[q];
    rec[d + q] = 1.0 / v;
    lv += log2(v);
  }
  const double w = a.a ? a.a[k] : 1.0 / (double)a.n;
  const double t = a.T[bs_class(a.cls[k], a.C) * a.C + c];
  const double g = log2(w) + log2(t) - 0.5 * lv - 0.5 * (double)d * kLog2TwoPi;
  rec[2 * d] = ok && w > 0.0 && t > 0.0 && g > -INFINITY && g < INFINITY ? g : -INFINITY;
}

// ---------------------------------------------------------------------------------
// Stable grouping by class in one workgroup: thread t owns the contiguous chunk t of the rows;
// per class, the chunks' counts are scanned (Hillis-Steele in LDS) and each thread writes its
// rows of the class behind the rows of the chunks before it.
__global__ __launch_bounds__(kGroupB) void k_bs_group(BsGroupArgs a) {
  __shared__ int scan[2][kGroupB];
  __shared__ int base;
  const int t = threadIdx.x;
  const long long n = a.n_dev ? (long long)*a.n_dev : a.n;
  const long long len = (n + kGroupB - 1) / kGroupB;
  const long long i0 = (long long)t * len < n ? (long long)t * len : n;
  const long long i1 = i0 + len < n ? i0 + len : n;
  if (t == 0) base = 0;
  __syncthreads();
  int blocks = 0;
  for (int c = 0; c < a.C; ++c) {
    int cnt = 0;
    for (long long i = i0; i < i1; ++i) cnt += bs_class(a.cls[i], a.C) == c;
    int cur = 0;
    scan[0][t] = cnt;
    __syncthreads();
    for (int off = 1; off < kGroupB; off <<= 1) {
      const int v = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0);
      scan[cur ^ 1][t] = v;
      cur ^= 1;
      __syncthreads();
    }
    const int start = base;
    int pos = start + scan[cur][t] - cnt;
    const int total = scan[cur][kGroupB - 1];
    for (long long i = i0; i < i1; ++i)
      if (bs_class(a.cls[i], a.C) == c) a.perm[pos++] = (int)i;
    if (t == 0) {
      a.tab[c] = start;
      a.tab[a.C + 1 + c] = blocks;
    }
    blocks += (total + kBsB - 1) / kBsB;
    __syncthreads();
    if (t == 0) base = start + total;
    __syncthreads();
  }
  if (t == 0) {
    a.tab[a.C] = base;
    a.tab[2 * a.C + 1] = blocks;
  }
}

// ---------------------------------------------------------------------------------
// Denominators.  Block b serves 256 grouped targets of one class c (the block starts of
// k_bs_group); range blockIdx.y of the sources goes through LDS 64 records of class c at a time.
template <int D>
__global__ __launch_bounds__(kBsB) void k_bs_den(BsPassArgs a) {
  __shared__ double tile[kBsTile * (2 * D + 1)];
  int c;
  if (!bs_block_class(a.tab, a.C, blockIdx.x, c)) return;   // (uniform over the block)
  const long long pos = bs_block_pos(a.tab, a.C, blockIdx.x, c, threadIdx.x);
  bool live = pos < a.tab[c + 1];
  double x[D];
  bs_load_target<D>(a.Xt, a.perm, pos, live, x);
  const long long len = (a.n_s + a.split - 1) / a.split;
  const long long k0 = (long long)blockIdx.y * len;
  const long long k1 = k0 + len < a.n_s ? k0 + len : a.n_s;
  double m = -INFINITY, s = 0.0;
  bs_den_range<D>(a.rec + (long long)c * a.n_s * (2 * D + 1), k0, k1, live, x, tile, m, s,
                  [](long long, double, double, double) { return false; });
  if (live) {
    double* out = a.part + (long long)blockIdx.y * a.n_t + pos;    // the m plane, then the s plane
    out[0] = m;
    out[(long long)a.split * a.n_t] = s;
  }
}

__global__ __launch_bounds__(kBsB) void k_bs_den_fin(BsDenFinArgs a) {
  const long long pos = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (pos >= a.n_t) return;
  double m = -INFINITY, s = 0.0;
  for (int r = 0; r < a.split; ++r) {
    const double* p = a.part + (long long)r * a.n_t + pos;
    bs_merge(m, s, p[0], p[(long long)a.split * a.n_t]);
  }
  const long long j = a.perm[pos];
  const bool reached = s > 0.0;
  const double l2 = reached ? m + log2(s) : -INFINITY;
  if (a.log_den) a.log_den[j] = reached ? l2 * kLn2 : -INFINITY;
  const double w = a.wt[j];
  a.lw[pos] = reached && w > 0.0 ? log2(w) - l2 : -INFINITY;
}

// ---------------------------------------------------------------------------------
// Weights.  Thread k is source k; range blockIdx.y of the grouped targets goes through LDS 64
// rows {x', lw} at a time, class segment by class segment, the thread holding its record of the
// segment's class in registers.
template <int D>
__global__ __launch_bounds__(kBsB) void k_bs_wgt(BsPassArgs a) {
  constexpr int R = 2 * D + 1, RT = D + 1;
  __shared__ double tile[kBsTile * RT];
  const int tid = threadIdx.x, C = a.C;
  const long long k = (long long)blockIdx.x * kBsB + tid;
  const bool live = k < a.n_s;
  const long long len = (a.n_t + a.split - 1) / a.split;
  const long long r0 = (long long)blockIdx.y * len;
  const long long r1 = r0 + len < a.n_t ? r0 + len : a.n_t;
  double m = -INFINITY, s = 0.0;
  for (int c = 0; c < C; ++c) {
    const long long p0 = r0 > a.tab[c] ? r0 : a.tab[c];
    const long long p1 = r1 < a.tab[c + 1] ? r1 : a.tab[c + 1];
    if (p0 >= p1) continue;              // (uniform over the block)
    double mu[D], iv[D], g = -INFINITY;
    {
      const double* rec = a.rec + ((long long)c * a.n_s + (live ? k : 0)) * R;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        mu[q] = rec[q];
        iv[q] = rec[D + q];
      }
      if (live) g = rec[2 * D];
    }
    for (long long pt = p0; pt < p1; pt += kBsTile) {
      const int rows = (int)(p1 - pt < kBsTile ? p1 - pt : kBsTile);
      for (int e = tid; e < rows * RT; e += kBsB) {
        const int r = e / RT, q = e - r * RT;
        tile[e] = q < D ? a.Xt[(long long)a.perm[pt + r] * D + q] : a.lw[pt + r];
      }
      __syncthreads();
      if (g > -INFINITY) {
        for (int r = 0; r < rows; ++r) {
          const double* row = tile + r * RT;
          double qd = 0.0;
#pragma unroll
          for (int q = 0; q < D; ++q) {
            const double df = row[q] - mu[q];
            qd = fma(df, df * iv[q], qd);
          }
          bs_add(m, s, fma(qd, -kHalfLog2e, g) + row[D]);
        }
      }
      __syncthreads();
    }
  }
  if (live) {
    double* out = a.part + (long long)blockIdx.y * a.n_s + k;
    out[0] = m;
    out[(long long)a.split * a.n_s] = s;
  }
}

__global__ __launch_bounds__(kBsB) void k_bs_wgt_fin(BsWgtFinArgs a) {
  const long long k = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (k >= a.n_s) return;
  double m = -INFINITY, s = 0.0;
  for (int r = 0; r < a.split; ++r) {
    const double* p = a.part + (long long)r * a.n_s + k;
    bs_merge(m, s, p[0], p[(long long)a.split * a.n_s]);
  }
  a.ws[k] = s > 0.0 ? ldexp(s, (int)fmax(fmin(m, 4096.0), -4096.0)) : 0.0;
}

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBsB) void k_bs_fill(double* w, long long n, double v) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < n) w[i] = v;
}

__device__ __forceinline__ long long bs_anc(int a, long long P) { return a < 0 ? 0 : (a >= P ? P - 1 : a); }

__global__ __launch_bounds__(kBsB) void k_bs_hist(const int* anc, long long P, int* hist) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < P) atomicAdd(&hist[bs_anc(anc[i], P)], 1);
}
__global__ __launch_bounds__(kBsB) void k_bs_mult(const int* anc, long long P, const int* hist, int* mult) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < P) mult[i] = hist[bs_anc(anc[i], P)];
}

// ---------------------------------------------------------------------------------
// One workgroup: quantity after quantity, thread-strided sums, wave butterfly, the waves in order.
__global__ __launch_bounds__(kBsB) void k_bs_reduce(BsReduceArgs a) {
  __shared__ double red[kBsB / 64];
  __shared__ double tot[3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int C = a.C, d = a.d, nq = C + d + 3;
  for (int qn = 0; qn < nq; ++qn) {
    double s = 0.0;
    for (long long i = tid; i < a.P; i += kBsB) {
      const double wi = a.w[i];
      double t;
      if (qn < C) t = bs_class(a.cls[i], C) == qn ? wi : 0.0;
      else if (qn < C + d) t = wi * a.X[i * d + (qn - C)];
      else if (qn == C + d) t = wi;
      else if (qn == C + d + 1) t = wi * wi;
      else t = (a.mult ? (double)a.mult[i] : 1.0) * (wi * wi);
      s += t;
    }
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (tid == 0) {
      double t = red[0];
      for (int v = 1; v < kBsB / 64; ++v) t += red[v];
      if (qn < C + d) a.out[qn] = t;
      else tot[qn - C - d] = t;
    }
    __syncthreads();
  }
  // (one 8-byte store per thread: no wide store, tests/test_isa_guard.py)
  if (tid < 3) a.out[C + d + tid] = tid == 0 ? tot[0] : tot[0] * tot[0] / tot[tid];
}

// ---------------------------------------------------------------------------------
static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_bs_moments(const BsMomentArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_moments, dim3(nblk(a.n, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_bs_group(const BsGroupArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_group, dim3(1), dim3(kGroupB), 0, s, a);
}

template <int D>
static void launch_passes(const BsPassArgs& a, bool den, hipStream_t s) {
  if (den)
    hipLaunchKernelGGL(k_bs_den<D>, dim3(nblk(a.n_t, kBsB) + a.C, (unsigned)a.split), dim3(kBsB), 0, s, a);
  else
    hipLaunchKernelGGL(k_bs_wgt<D>, dim3(nblk(a.n_s, kBsB), (unsigned)a.split), dim3(kBsB), 0, s, a);
}
static void launch_pass(const BsPassArgs& a, bool den, hipStream_t s) {
  switch (a.d) {
#define GPMDM_D(n) case n: launch_passes<n>(a, den, s); break;
    GPMDM_D(1) GPMDM_D(2) GPMDM_D(3) GPMDM_D(4) GPMDM_D(5) GPMDM_D(6) GPMDM_D(7) GPMDM_D(8)
    GPMDM_D(9) GPMDM_D(10) GPMDM_D(11) GPMDM_D(12) GPMDM_D(13) GPMDM_D(14) GPMDM_D(15) GPMDM_D(16)
    GPMDM_D(24) GPMDM_D(32)
#undef GPMDM_D
    default: break;   // (a model's d is one of these: host_image.h)
  }
}
void launch_bs_den(const BsPassArgs& a, hipStream_t s) { launch_pass(a, true, s); }
void launch_bs_wgt(const BsPassArgs& a, hipStream_t s) { launch_pass(a, false, s); }

void launch_bs_den_fin(const BsDenFinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_den_fin, dim3(nblk(a.n_t, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_bs_wgt_fin(const BsWgtFinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_wgt_fin, dim3(nblk(a.n_s, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_bs_fill(double* w, long long n, double v, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_fill, dim3(nblk(n, kBsB)), dim3(kBsB), 0, s, w, n, v);
}
void launch_bs_mult(const int* anc, long long P, int* hist, int* mult, hipStream_t s) {
  (void)hipMemsetAsync(hist, 0, sizeof(int) * (size_t)P, s);
  hipLaunchKernelGGL(k_bs_hist, dim3(nblk(P, kBsB)), dim3(kBsB), 0, s, anc, P, hist);
  hipLaunchKernelGGL(k_bs_mult, dim3(nblk(P, kBsB)), dim3(kBsB), 0, s, anc, P, (const int*)hist, mult);
}
void launch_bs_reduce(const BsReduceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_reduce, dim3(1), dim3(kBsB), 0, s, a);
}

}  // namespace gpmdm
