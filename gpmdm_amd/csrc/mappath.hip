// The MAP trajectory decoder's kernels (mappath.h).
#include "mappath.h"

namespace gpmdm {

// (backsmooth.hip's constants: the pair exponent below is k_bs_den's)
constexpr double kMpHalfLog2e = 0.72134752044448170368;   // 1/2 log2 e
constexpr double kMpLog2e = 1.4426950408889634074;
constexpr double kMpLog2TwoPi = 2.6514961294723187980;    // log2 (2 pi)
constexpr double kMpLn2 = 0.69314718055994530942;
constexpr int kMpGroupB = 1024;

__device__ __forceinline__ int mp_class(int c, int C) { return c < 0 ? 0 : (c >= C ? C - 1 : c); }
__device__ __forceinline__ long long mp_anc(int a, long long P) { return a < 0 ? 0 : (a >= P ? P - 1 : a); }
__device__ __forceinline__ long long mp_count(const int* n_dev, long long n) {
  if (!n_dev) return n;
  const long long v = *n_dev;
  return v < 0 ? 0 : (v > n ? n : v);
}

// ---------------------------------------------------------------------------------
// Leaders of a slot.
__global__ __launch_bounds__(kBsB) void k_mp_owner(MpLeadArgs a) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < a.P) atomicMin(&a.owner[mp_anc(a.anc[i], a.P)], (int)i);
}

// One workgroup, k_bs_group's scan: thread t owns the contiguous chunk t of the particles, the
// chunks' leader counts are scanned (Hillis-Steele in LDS) and each thread writes its leaders
// behind those of the chunks before it -- increasing particle index.
__global__ __launch_bounds__(kMpGroupB) void k_mp_compact(MpLeadArgs a) {
  __shared__ int scan[2][kMpGroupB];
  const int t = threadIdx.x;
  const long long len = (a.P + kMpGroupB - 1) / kMpGroupB;
  const long long i0 = (long long)t * len < a.P ? (long long)t * len : a.P;
  const long long i1 = i0 + len < a.P ? i0 + len : a.P;
  int cnt = 0;
  for (long long i = i0; i < i1; ++i) cnt += a.owner[mp_anc(a.anc[i], a.P)] == (int)i;
  int cur = 0;
  scan[0][t] = cnt;
  __syncthreads();
  for (int off = 1; off < kMpGroupB; off <<= 1) {
    const int v = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0);
    scan[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  int pos = scan[cur][t] - cnt;
  for (long long i = i0; i < i1; ++i)
    if (a.owner[mp_anc(a.anc[i], a.P)] == (int)i) {
      a.rank[i] = pos;
      a.rows[pos++] = (int)i;
    }
  if (t == 0) a.count[0] = scan[cur][kMpGroupB - 1];
}

__global__ __launch_bounds__(kBsB) void k_mp_lead(MpLeadArgs a) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < a.P) a.lead[i] = a.rank[a.owner[mp_anc(a.anc[i], a.P)]];
}

__global__ __launch_bounds__(kBsB) void k_mp_iota(MpLeadArgs a) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < a.P) {
    a.rows[i] = (int)i;
    a.lead[i] = (int)i;
  }
  if (i == 0) a.count[0] = (int)a.P;
}

// ---------------------------------------------------------------------------------
// Thread e copies state value e, and class / log-likelihood e while e < n; zeros past the count
// (the dynamics tiles of a partly filled last tile read finite rows).
__global__ __launch_bounds__(kBsB) void k_mp_gather(MpGatherArgs a) {
  const long long e = (long long)blockIdx.x * kBsB + threadIdx.x;
  const long long n = mp_count(a.n_dev, a.n);
  if (e < a.n * a.d) {
    const long long r = e / a.d;
    const int q = (int)(e - r * a.d);
    const long long i = r < n ? (a.rows ? (long long)a.rows[r] : r) : 0;
    a.X_out[e] = r < n ? a.X[i * a.d + q] : 0.0;
  }
  if (e < a.n) {
    const long long i = e < n ? (a.rows ? (long long)a.rows[e] : e) : 0;
    a.cls_out[e] = e < n ? a.cls[i] : 0;
    if (a.ll_out) a.ll_out[e] = e < n ? (a.ll ? a.ll[i] : 0.0) : 0.0;
  }
}

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBsB) void k_mp_moments(MpMomentArgs a) {
  const long long k = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (k >= mp_count(a.n_dev, a.n)) return;
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
  const double t = a.T[mp_class(a.cls[k], a.C) * a.C + c];
  const double dl = a.delta ? a.delta[k] : 0.0;
  const double g = fma(dl, kMpLog2e, log2(t) - 0.5 * lv - 0.5 * (double)d * kMpLog2TwoPi);
  rec[2 * d] = ok && t > 0.0 && g > -INFINITY && g < INFINITY ? g : -INFINITY;
}

// ---------------------------------------------------------------------------------
// The max pass.  Block b serves 256 grouped targets of one class c (the block starts of
// k_bs_group); range blockIdx.y of the sources goes through LDS 64 records of class c at a time.
template <int D>
__global__ __launch_bounds__(kBsB) void k_mp_max(MpMaxArgs a) {
  constexpr int R = 2 * D + 1;
  __shared__ double tile[kBsTile * R];
  const int tid = threadIdx.x, C = a.C;
  const int b = blockIdx.x;
  const int* bstart = a.tab + C + 1;
  if (b >= bstart[C]) return;            // (uniform over the block)
  int c = 0;
  while (c + 1 < C && b >= bstart[c + 1]) ++c;
  const long long pos = (long long)a.tab[c] + (long long)(b - bstart[c]) * kBsB + tid;
  const bool live = pos < a.tab[c + 1];
  double x[D];
  {
    const long long j = live ? a.perm[pos] : 0;
#pragma unroll
    for (int q = 0; q < D; ++q) x[q] = live ? a.Xt[j * D + q] : 0.0;
  }
  const long long n_s = mp_count(a.ns_dev, a.n_s);
  const long long len = (n_s + a.split - 1) / a.split;
  const long long k0 = (long long)blockIdx.y * len;
  const long long k1 = k0 + len < n_s ? k0 + len : n_s;
  const double* rec = a.rec + (long long)c * a.n_s * R;
  double best = -INFINITY;
  int arg = -1;
  for (long long kt = k0; kt < k1; kt += kBsTile) {
    const int rows = (int)(k1 - kt < kBsTile ? k1 - kt : kBsTile);
    for (int e = tid; e < rows * R; e += kBsB) tile[e] = rec[kt * R + e];
    __syncthreads();
    if (live) {
      for (int r = 0; r < rows; ++r) {
        const double* row = tile + r * R;
        double qd = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
          const double df = x[q] - row[q];
          qd = fma(df, df * row[D + q], qd);
        }
        const double v = fma(qd, -kMpHalfLog2e, row[2 * D]);
        if (v > best) {                  // (strict: the lowest index of the range; NaN never wins)
          best = v;
          arg = (int)(kt + r);
        }
      }
    }
    __syncthreads();
  }
  if (live) {
    a.val[(long long)blockIdx.y * a.n_t + pos] = best;
    a.idx[(long long)blockIdx.y * a.n_t + pos] = arg;
  }
}

__global__ __launch_bounds__(kBsB) void k_mp_fin(MpFinArgs a) {
  const long long pos = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (pos >= mp_count(a.nt_dev, a.n_t)) return;
  double best = -INFINITY;
  int arg = -1;
  for (int r = 0; r < a.split; ++r) {
    const double v = a.val[(long long)r * a.n_t + pos];
    if (v > best) {                      // (the ranges rise with the source index)
      best = v;
      arg = a.idx[(long long)r * a.n_t + pos];
    }
  }
  const long long j = a.perm[pos];
  const double l = a.ll ? a.ll[j] : 0.0;
  const bool ok = arg >= 0 && l > -INFINITY && l < INFINITY;
  a.delta[j] = ok ? fma(best, kMpLn2, l) : -INFINITY;
  a.psi[j] = ok ? (a.src_rows ? a.src_rows[arg] : arg) : -1;
}

__global__ __launch_bounds__(kBsB) void k_mp_expand(MpExpandArgs a) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i >= a.P) return;
  const long long r = a.lead ? (long long)a.lead[i] : i;
  a.delta[i] = a.delta_c[r];
  if (a.psi) a.psi[i] = a.psi_c[r];
}

// ---------------------------------------------------------------------------------
// (value, index) pairs: the larger value, then the lower index (index < 0: no candidate yet).
__device__ __forceinline__ void mp_better(double& v, int& i, double v2, int i2) {
  if (i2 >= 0 && (v2 > v || (v2 == v && (i < 0 || i2 < i)))) {
    v = v2;
    i = i2;
  }
}

__global__ __launch_bounds__(kBsB) void k_mp_back(MpBackArgs a) {
  __shared__ double red_v[kBsB / 64];
  __shared__ int red_i[kBsB / 64];
  __shared__ int path[kMpMaxLag + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double v = -INFINITY;
  int arg = -1;
  for (long long i = tid; i < a.P; i += kBsB) {
    const double x = a.delta[i];
    if (x > v) {
      v = x;
      arg = (int)i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double v2 = __shfl_xor(v, off);
    const int i2 = __shfl_xor(arg, off);
    mp_better(v, arg, v2, i2);
  }
  if (lane == 0) {
    red_v[w] = v;
    red_i[w] = arg;
  }
  __syncthreads();
  if (tid == 0) {
    double bv = red_v[0];
    int j = red_i[0];
    for (int u = 1; u < kBsB / 64; ++u) mp_better(bv, j, red_v[u], red_i[u]);
    for (int l = 0; l <= a.lag; ++l) {
      path[l] = j;
      if (j >= 0 && l < a.lag) j = a.psi[(long long)l * a.P + j];
    }
  }
  __syncthreads();
  // (one 8-byte store per thread and turn: no wide store, tests/test_isa_guard.py)
  const int W = a.d + 4;
  for (int e = tid; e < (a.lag + 1) * W; e += kBsB) {
    const int l = e / W, q = e - l * W;
    const int j = path[l];
    const long long k = (long long)((a.slot - l % a.n_slots + a.n_slots) % a.n_slots) * a.P + (j < 0 ? 0 : j);
    double o;
    if (q == 0) o = (double)j;
    else if (q == 1) o = j < 0 ? -1.0 : (double)a.ring_cls[k];
    else if (q == 2) o = j < 0 ? -INFINITY : a.delta[(long long)l * a.P + j];
    else if (q == 3) o = (double)a.count[l];
    else o = j < 0 ? NAN : a.ring_X[k * a.d + (q - 4)];
    a.out[e] = o;
  }
  if (tid == 0) a.out[(long long)(a.lag + 1) * W] = path[0] < 0 ? -INFINITY : a.delta[path[0]];
}

// ---------------------------------------------------------------------------------
// The ring's log-likelihood plane: the proposal each slot particle copies (ridx nullptr: a
// cleared ring's root, zeros).
__global__ __launch_bounds__(kBsB) void k_mp_ll_record(const double* ll, const int* ridx, long long P, double* dst) {
  const long long i = (long long)blockIdx.x * kBsB + threadIdx.x;
  if (i < P) dst[i] = ridx ? ll[mp_anc(ridx[i], P)] : 0.0;
}

// The dynamics tiles' one-segment table (pf_kernels.hip k_seg_table) for a device row count.
__global__ void k_mp_seg_table(int* t, const int* n_dev, int n_max, int pt) {
  const int i = threadIdx.x;
  const int n = (int)mp_count(n_dev, n_max);
  if (i < 5) t[i] = i == 1 ? n : (i == 4 ? (n + pt - 1) / pt : 0);
}

// ---------------------------------------------------------------------------------
static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_mp_leaders(const MpLeadArgs& a, bool has_anc, hipStream_t s) {
  if (!has_anc) {
    hipLaunchKernelGGL(k_mp_iota, dim3(nblk(a.P, kBsB)), dim3(kBsB), 0, s, a);
    return;
  }
  (void)hipMemsetAsync(a.owner, 0x7f, sizeof(int) * (size_t)a.P, s);   // 0x7f7f7f7f: above every index
  hipLaunchKernelGGL(k_mp_owner, dim3(nblk(a.P, kBsB)), dim3(kBsB), 0, s, a);
  hipLaunchKernelGGL(k_mp_compact, dim3(1), dim3(kMpGroupB), 0, s, a);
  hipLaunchKernelGGL(k_mp_lead, dim3(nblk(a.P, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_mp_gather(const MpGatherArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_gather, dim3(nblk(a.n * a.d, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_mp_moments(const MpMomentArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_moments, dim3(nblk(a.n, kBsB)), dim3(kBsB), 0, s, a);
}

template <int D>
static void launch_max(const MpMaxArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_max<D>, dim3(nblk(a.n_t, kBsB) + a.C, (unsigned)a.split), dim3(kBsB), 0, s, a);
}
void launch_mp_max(const MpMaxArgs& a, hipStream_t s) {
  switch (a.d) {
#define GPMDM_D(n) case n: launch_max<n>(a, s); break;
    GPMDM_D(1) GPMDM_D(2) GPMDM_D(3) GPMDM_D(4) GPMDM_D(5) GPMDM_D(6) GPMDM_D(7) GPMDM_D(8)
    GPMDM_D(9) GPMDM_D(10) GPMDM_D(11) GPMDM_D(12) GPMDM_D(13) GPMDM_D(14) GPMDM_D(15) GPMDM_D(16)
    GPMDM_D(24) GPMDM_D(32)
#undef GPMDM_D
    default: break;   // (a model's d is one of these: host_image.h)
  }
}
void launch_mp_fin(const MpFinArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_fin, dim3(nblk(a.n_t, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_mp_expand(const MpExpandArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_expand, dim3(nblk(a.P, kBsB)), dim3(kBsB), 0, s, a);
}
void launch_mp_back(const MpBackArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_back, dim3(1), dim3(kBsB), 0, s, a);
}
void launch_mp_seg_table(int* t, const int* n_dev, int n_max, int pt, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_seg_table, dim3(1), dim3(64), 0, s, t, n_dev, n_max, pt);
}
void launch_mp_ll_record(const double* ll, const int* ridx, long long P, double* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_mp_ll_record, dim3(nblk(P, kBsB)), dim3(kBsB), 0, s, ll, ridx, P, dst);
}

}  // namespace gpmdm
