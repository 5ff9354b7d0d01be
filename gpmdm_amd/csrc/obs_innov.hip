// The innovation tile and its finish, and the ancestors' gather of vc (obs_innov.h):
// gpmdm_pf_innovation, gpmdm_pf_observation_gp.
#include "obs_innov.h"

#include "common.h"
#include "obs_readout_tile.h"

namespace gpmdm {

constexpr double kLn2Pi = 1.8378770664093453;   // float64 ln 2 pi

__device__ __forceinline__ double innov_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// (M, s) <- (M, s) + (Mb, sb): log-sum-exp pairs, s = sum exp(a - M); the empty pair is (-inf, 0).
// One exponential per merge -- the larger side's factor is exp(0) = 1 exactly -- by the
// generation's exp2_64 (gp_tile.h; tab: kExp2Tab in LDS).  NaN never wins a max.
__device__ __forceinline__ void lse_merge(double& M, double& s, double Mb, double sb, const double* tab) {
  if (!(Mb > -INFINITY)) return;
  if (M >= Mb) {
    s = fma(sb, exp2_64((Mb - M) * kLog2eX64, tab), s);
  } else {
    // (M = -inf: s = 0, and the factor's NaN from inf - inf must not reach it)
    s = M > -INFINITY ? fma(s, exp2_64((M - Mb) * kLog2eX64, tab), sb) : sb;
    M = Mb;
  }
}

__global__ __launch_bounds__(256) void k_obs_innov(const InnovParams prm) {
  __shared__ RoTileLds sh;
  // per particle of the tile: -1/2 / vc (0: invalid) and -1/2 log vc -- one division and one log
  // per particle, none per element
  __shared__ double hvs[kRoPT], lvs[kRoPT];
  const ReadoutParams& ro = prm.ro;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x, G = blockIdx.y;
  const long long fil = blockIdx.z;
  const int li = lane & 15, lk = lane >> 4;
  d4 acc[4];
  ro_tile_means(ro, sh, tile, G, fil, acc);                  // the read-out's K loop (obs_readout_tile.h)

  const long long pos0 = (long long)tile * kRoPT;
  const long long left = ro.P - pos0;
  const int n = left < kRoPT ? (int)left : kRoPT;            // the tile's count
  if (w == 0) {
    // particle m = lane: one log per particle; rows past the tile's count are invalid
    double v = innov_nan();
    if (lane < n && prm.vc) v = prm.vc[fil * ro.P + pos0 + lane];
    const bool ok = v > 0.0;                                 // (false for NaN)
    hvs[lane] = ok ? -0.5 / v : 0.0;
    lvs[lane] = ok ? -0.5 * log(v) : 0.0;
    if (G == 0) {
      const double sv = wave_sum(ok ? v : 0.0), cnt = wave_sum(ok ? 1.0 : 0.0);
      if (lane == 0) {
        // two planes per filter, so each value is an 8-byte store of its own
        double* vp = prm.vpart + (size_t)fil * gridDim.x * 2 + tile;
        vp[0] = sv;
        vp[gridDim.x] = cnt;
      }
    }
  }
  __syncthreads();

  // ---- epilogue 1: the read-out's (mean, M2)
  double mean, m2;
  ro_tile_moments(acc, n, lk, mean, m2);

  // ---- epilogue 2: the column's log-sum-exp pair over the tile's valid rows
  const int col = kRoGC * G + 16 * w + li;
  const bool live = col < ro.D;                              // (padding columns: mu = 0, finite dummies)
  const double zj = live ? prm.z[fil * ro.D + col] : 0.0;
  const double l2 = live ? prm.lam2[col] : 1.0;
  const double c0 = live ? -0.5 * (log(prm.il2[col]) + kLn2Pi) : 0.0;
  double a[16];
  double M = -INFINITY;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = mt * 16 + lk + 4 * r;
      const double hv = hvs[row];
      double av = -INFINITY;
      if (hv < 0.0) {
        const double t = zj - acc[mt][r];
        av = fma(t * t * l2, hv, lvs[row] + c0);
      }
      a[mt * 4 + r] = av;
      M = fmax(M, av);
    }
#pragma unroll
  for (int i = 0; i < 16; ++i)                               // exp(a - M) by the generation's exp2_64 (gp_tile.h)
    a[i] = a[i] > -INFINITY ? exp2_64((a[i] - M) * kLog2eX64, sh.tab) : 0.0;
  double s = ro_tree16(a);
  lse_merge(M, s, __shfl_xor(M, 16), __shfl_xor(s, 16), sh.tab);
  lse_merge(M, s, __shfl_xor(M, 32), __shfl_xor(s, 32), sh.tab);

  if (lk == 0) {
    const int Dpad = ro.n_groups * kRoGC;
    double* o = prm.part + ((size_t)fil * gridDim.x + tile) * kInnovPlanes * Dpad + col;   // 8-byte stores
    o[0] = mean;
    o[Dpad] = m2;
    o[2 * (size_t)Dpad] = M;
    o[3 * (size_t)Dpad] = s;
  }
}

// 16 columns x 16 runs of tiles per workgroup, as k_obs_readout_finish: run r merges its contiguous
// tiles in order, then the runs are merged in order.  blockIdx.y: the filter.
__global__ __launch_bounds__(256) void k_obs_innov_finish(const InnovParams prm, int n_tiles) {
  __shared__ double sn[16][16], sm[16][16], sq[16][16], sM[16][16], ss[16][16], sv[16][16], sc[16][16];
  __shared__ double tab[64];
  if (threadIdx.x < 64) tab[threadIdx.x] = kExp2Tab[threadIdx.x];
  __syncthreads();
  const ReadoutParams& ro = prm.ro;
  const int cl = threadIdx.x & 15, run = threadIdx.x >> 4;
  const int Dpad = ro.n_groups * kRoGC, D = ro.D;
  const int col = blockIdx.x * 16 + cl;                      // < Dpad (a multiple of 16)
  const long long fil = blockIdx.y;
  const int chunk = (n_tiles + 15) / 16;
  const int t0 = run * chunk, t1 = min(n_tiles, t0 + chunk);
  double n = 0.0, mean = 0.0, M2 = 0.0, M = -INFINITY, s = 0.0, vsum = 0.0, cnt = 0.0;
  for (int t = t0; t < t1; t += 4) {             // four tiles' loads in flight, then the merges in tile order
    double v[4][6];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int tt = min(t + k, t1 - 1);
      const double* p = prm.part + ((size_t)fil * n_tiles + tt) * kInnovPlanes * Dpad + col;
      const double* vp = prm.vpart + (size_t)fil * n_tiles * 2 + tt;
      v[k][0] = p[0];
      v[k][1] = p[Dpad];
      v[k][2] = p[2 * (size_t)Dpad];
      v[k][3] = p[3 * (size_t)Dpad];
      v[k][4] = vp[0];
      v[k][5] = vp[n_tiles];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t + k < t1) {
        const long long left = ro.P - (long long)(t + k) * kRoPT;
        const double nb = left < kRoPT ? (double)left : (double)kRoPT;
        chan_merge(n, mean, M2, nb, v[k][0], v[k][1]);
        lse_merge(M, s, v[k][2], v[k][3], tab);
        vsum += v[k][4];
        cnt += v[k][5];
      }
  }
  sn[run][cl] = n;
  sm[run][cl] = mean;
  sq[run][cl] = M2;
  sM[run][cl] = M;
  ss[run][cl] = s;
  sv[run][cl] = vsum;
  sc[run][cl] = cnt;
  __syncthreads();
  if (run == 0 && col < D) {
    for (int r = 1; r < 16; ++r) {
      chan_merge(n, mean, M2, sn[r][cl], sm[r][cl], sq[r][cl]);
      lse_merge(M, s, sM[r][cl], ss[r][cl], tab);
      vsum += sv[r][cl];
      cnt += sc[r][cl];
    }
    const double nan = innov_nan();
    const bool some = cnt > 0.0;
    const bool obs = !prm.mask || prm.mask[fil * D + col] != 0;
    const double spread = M2 / n;
    const double gpv = some ? prm.il2[col] * (vsum / cnt) : nan;
    const double var = spread + gpv;
    const double res = obs ? prm.z[fil * D + col] - mean : nan;
    double* out = prm.out + fil * (kInnovFields * D + 1);
    out[col] = mean;
    out[D + col] = spread;
    out[2 * D + col] = gpv;
    out[3 * D + col] = var;
    out[4 * D + col] = res;
    out[5 * D + col] = res / sqrt(var);
    out[6 * D + col] = obs && some ? M + log(s) - log(cnt) : nan;
    if (col == 0) out[kInnovFields * D] = cnt;
  }
}

// Block (b, f): resampled slots [256 b, 256 b + 256) of filter f.  Dead threads and invalid
// entries add zeros.
__global__ __launch_bounds__(256) void k_vc_gather(VcGatherArgs a) {
  __shared__ double red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long f = blockIdx.y, nbf = gridDim.x;
  const long long p = (long long)blockIdx.x * 256 + tid;
  double v = 0.0, c = 0.0;
  if (p < a.Pf && a.vc) {
    const double x = a.vc[f * a.Pf + a.ridx[f * a.Pf + p]];
    if (x > 0.0) {
      v = x;
      c = 1.0;
    }
  }
  v = wave_sum(v);
  c = wave_sum(c);
  if (lane == 0) {
    red[w][0] = v;
    red[w][1] = c;
  }
  __syncthreads();
  if (tid < 2) {
    double t = red[0][tid];
    for (int k = 1; k < 4; ++k) t += red[k][tid];
    a.partials[(f * nbf + blockIdx.x) * 2 + tid] = t;
  }
}

// One workgroup per filter: the blocks in order, then il2_j sum / count (NaN with no valid entry)
__global__ __launch_bounds__(256) void k_vc_gather_finish(VcGatherArgs a, int nbf) {
  constexpr int kChunk = 1024;                   // blocks staged in LDS at a time (all threads load)
  __shared__ double stage[2 * kChunk];
  __shared__ double tot[2];
  const long long f = blockIdx.x;
  double t = 0.0;
  for (int b0 = 0; b0 < nbf; b0 += kChunk) {
    const int nb = min(kChunk, nbf - b0);
    for (int i = threadIdx.x; i < 2 * nb; i += 256) stage[i] = a.partials[(f * nbf + b0) * 2 + i];
    __syncthreads();
    if (threadIdx.x < 2)
      for (int b = 0; b < nb; ++b) t += stage[2 * b + threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x < 2) tot[threadIdx.x] = t;
  __syncthreads();
  const double vbar = tot[1] > 0.0 ? tot[0] / tot[1] : innov_nan();
  for (int j = threadIdx.x; j < a.D; j += 256) a.out[f * a.D + j] = a.il2[j] * vbar;
}

void launch_obs_innov(const InnovParams& p, hipStream_t s) {
  const int tiles = readout_tiles(p.ro.P);
  const int F = p.ro.F > 0 ? p.ro.F : 1;
  hipLaunchKernelGGL(k_obs_innov, dim3(tiles, p.ro.n_groups, F), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_obs_innov_finish, dim3(p.ro.n_groups * kRoGC / 16, F), dim3(256), 0, s, p, tiles);
}

void launch_vc_gather(const VcGatherArgs& a, int F, hipStream_t s) {
  const int nbf = (int)((a.Pf + 255) / 256);
  hipLaunchKernelGGL(k_vc_gather, dim3(nbf, F), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_vc_gather_finish, dim3(F), dim3(256), 0, s, a, nbf);
}

}  // namespace gpmdm
