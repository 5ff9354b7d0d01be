// The device code k_obs_readout (obs_readout.hip) and k_obs_innov (obs_innov.hip) share: the
// K loop of the mean-only observation tile, the (mean, M2) epilogue over its accumulators and
// the pairwise update the finishes merge the tiles with.  One definition, so that both kernels
// give bitwise the same mean and spread on the same cloud.  Layout and orders: obs_readout.h.
#pragma once
#include "obs_readout.h"

#include "gp_tile.h"   // kExp2Tab, exp2_64

namespace gpmdm {

struct RoTileLds {
  double As[2][kBK][kRoPT + 16];     // rows k, k+1 land 32 banks apart (gp_tile.h)
  double PA[kMaxD][kRoPT];           // 2 (x / l) (64 / ln 2), coordinate-major
  double tab[64];
};

// acc[mt][r] <- mu of particle row mt 16 + (lane >> 4) + 4 r, column 64 G + 16 w + (lane & 15)
// of tile `tile` of filter `fil` (256 threads, all of them; ends behind a barrier)
__device__ __forceinline__ void ro_tile_means(const ReadoutParams& prm, RoTileLds& sh, int tile, int G, long long fil,
                                              d4 (&acc)[4]) {
  constexpr double kScale = kLog2eX64;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long pos0 = (long long)tile * kRoPT;
  const int d = prm.d, RW = d + 1, nks = prm.nks;

  for (int i = tid; i < 64; i += 256) sh.tab[i] = kExp2Tab[i];

  // generation role: particle m = lane, rows w + 4 s of each K-step (gp_tile.h's split)
  const int m = lane;
  long long pos = pos0 + m;
  if (pos >= prm.P) pos = pos0;                              // padded row: count 0 in the epilogue
  double asq = 0.0;
  for (int j = 0; j < d; ++j) {
    const double xs = prm.X[(fil * prm.P + pos) * d + j] / prm.ls[j];
    asq = fma(xs, xs, asq);
    if ((j & 3) == w) sh.PA[j][m] = (2.0 * kScale) * xs;
  }
  asq *= kScale;
  __syncthreads();

  const double* __restrict__ Xrec = prm.Xrec;
  auto gen = [&](int ks, int buf) {
    const double* r0 = Xrec + ((long long)ks * kBK + w) * RW;   // wave-uniform: rows w, w+4, w+8, w+12
    double x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = -(asq + r0[s * 4 * RW + d]);
    for (int j = 0; j < d; ++j) {
      const double a = sh.PA[j][m];
#pragma unroll
      for (int s = 0; s < 4; ++s) x[s] = fma(a, r0[s * 4 * RW + j], x[s]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) sh.As[buf][w + 4 * s][m] = exp2_64(x[s], sh.tab);   // padding rows: exactly 0
  };

  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = (d4){0.0, 0.0, 0.0, 0.0};
  const d4* __restrict__ Bw = reinterpret_cast<const d4*>(prm.Bro) + ((size_t)G * nks * 4 + w) * 64 + lane;

  gen(0, 0);
  __syncthreads();
  for (int ks = 0; ks < nks; ++ks) {
    const d4 bv = Bw[(size_t)ks * 256];
    if (ks + 1 < nks) gen(ks + 1, (ks + 1) & 1);
    const int buf = ks & 1;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(sh.As[buf][kk * 4 + lk][mt * 16 + li], bv[kk], acc[mt], 0, 0, 0);
    __syncthreads();
  }
}

__device__ __forceinline__ double ro_lane_groups(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

__device__ __forceinline__ double ro_tree16(const double (&a)[16]) {
  double b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) b[i] = a[2 * i] + a[2 * i + 1];
  return ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));
}

// the tile's mean and centred sum of squares of this lane's column over the first n particle
// rows (C/D layout lane l, reg r -> particle row mt 16 + (l >> 4) + 4 r, column l & 15)
__device__ __forceinline__ void ro_tile_moments(const d4 (&acc)[4], int n, int lk, double& mean, double& m2) {
  double v[16];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[mt * 4 + r] = mt * 16 + lk + 4 * r < n ? acc[mt][r] : 0.0;
  mean = ro_lane_groups(ro_tree16(v)) / (double)n;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double t = acc[mt][r] - mean;
      v[mt * 4 + r] = mt * 16 + lk + 4 * r < n ? t * t : 0.0;
    }
  m2 = ro_lane_groups(ro_tree16(v));
}

// (n, mean, M2) <- (n, mean, M2) + (nb, mb, Mb): Chan, Golub & LeVeque's pairwise update
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& M2, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (n == 0.0) {
    n = nb;
    mean = mb;
    M2 = Mb;
    return;
  }
  const double nt = n + nb, delta = mb - mean;
  mean = fma(delta, nb / nt, mean);
  M2 = (M2 + Mb) + delta * delta * (n * nb / nt);
  n = nt;
}

}  // namespace gpmdm
