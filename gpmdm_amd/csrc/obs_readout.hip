// The mean-only observation tile and its finish (obs_readout.h): gpmdm_pf_observation.
#include "obs_readout.h"

#include "gp_tile.h"   // kExp2Tab, exp2_64

namespace gpmdm {

void pack_readout_beta(const double* beta, long long N, int D, std::vector<double>& out) {
  const int nks = ksteps((int)N), ng = readout_groups(D);
  out.assign((size_t)ng * nks * 1024, 0.0);
  for (int G = 0; G < ng; ++G)
    for (int ks = 0; ks < nks; ++ks)
      for (int w = 0; w < 4; ++w)
        for (int l = 0; l < 64; ++l)
          for (int kk = 0; kk < 4; ++kk) {
            const long long row = (long long)ks * kBK + 4 * kk + (l >> 4);
            const int col = kRoGC * G + 16 * w + (l & 15);
            if (row < N && col < D)
              out[((((size_t)G * nks + ks) * 4 + w) * 64 + l) * 4 + kk] = beta[row * D + col];
          }
}

__global__ __launch_bounds__(256) void k_obs_readout(const ReadoutParams prm) {
  constexpr int LDA = kRoPT + 16;                            // rows k, k+1 land 32 banks apart (gp_tile.h)
  __shared__ double As[2][kBK][LDA];
  __shared__ double PA[kMaxD][kRoPT];                        // 2 (x / l) (64 / ln 2), coordinate-major
  __shared__ double tab[64];
  constexpr double kScale = kLog2eX64;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, G = blockIdx.y;
  const long long fil = blockIdx.z;                          // the filter (a bank: tiles are cut within it)
  const long long pos0 = (long long)tile * kRoPT;
  const int d = prm.d, RW = d + 1, nks = prm.nks;

  for (int i = tid; i < 64; i += 256) tab[i] = kExp2Tab[i];

  // generation role: particle m = lane, rows w + 4 s of each K-step (gp_tile.h's split)
  const int m = lane;
  long long pos = pos0 + m;
  if (pos >= prm.P) pos = pos0;                              // padded row: count 0 in the epilogue
  double asq = 0.0;
  for (int j = 0; j < d; ++j) {
    const double xs = prm.X[(fil * prm.P + pos) * d + j] / prm.ls[j];
    asq = fma(xs, xs, asq);
    if ((j & 3) == w) PA[j][m] = (2.0 * kScale) * xs;
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
      const double a = PA[j][m];
#pragma unroll
      for (int s = 0; s < 4; ++s) x[s] = fma(a, r0[s * 4 * RW + j], x[s]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) As[buf][w + 4 * s][m] = exp2_64(x[s], tab);   // padding rows: exactly 0
  };

  const int li = lane & 15, lk = lane >> 4;
  d4 acc[4];
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
        acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[buf][kk * 4 + lk][mt * 16 + li], bv[kk], acc[mt], 0, 0, 0);
    __syncthreads();
  }

  // ---- epilogue: C/D layout lane l, reg r -> particle row mt 16 + (l >> 4) + 4 r, column l & 15
  const long long left = prm.P - pos0;
  const int n = left < kRoPT ? (int)left : kRoPT;            // the tile's count
  auto lane_groups = [](double v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
  };
  double v[16];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[mt * 4 + r] = mt * 16 + lk + 4 * r < n ? acc[mt][r] : 0.0;
  auto tree16 = [](const double (&a)[16]) {
    double b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = a[2 * i] + a[2 * i + 1];
    return ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));
  };
  const double mean = lane_groups(tree16(v)) / (double)n;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double t = acc[mt][r] - mean;
      v[mt * 4 + r] = mt * 16 + lk + 4 * r < n ? t * t : 0.0;
    }
  const double m2 = lane_groups(tree16(v));
  if (lk == 0) {
    const int Dpad = prm.n_groups * kRoGC;
    // two planes per tile, so each value is an 8-byte store of its own (no 16-byte VGPR
    // stores in this code base: tests/test_isa_guard.py)
    double* o = prm.part + ((size_t)fil * gridDim.x + tile) * 2 * Dpad + kRoGC * G + 16 * w + li;
    o[0] = mean;
    o[Dpad] = m2;
  }
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

// 16 columns x 16 runs of tiles per workgroup: run r merges its contiguous tiles in order,
// then the runs are merged in order.  blockIdx.y: the filter, over its own n_tiles partials.
__global__ __launch_bounds__(256) void k_obs_readout_finish(const ReadoutParams prm, int n_tiles) {
  __shared__ double sn[16][16], sm[16][16], sq[16][16];
  const int cl = threadIdx.x & 15, run = threadIdx.x >> 4;
  const int Dpad = prm.n_groups * kRoGC;
  const int col = blockIdx.x * 16 + cl;                      // < Dpad (a multiple of 16)
  const long long fil = blockIdx.y;
  const int chunk = (n_tiles + 15) / 16;
  const int t0 = run * chunk, t1 = min(n_tiles, t0 + chunk);
  double n = 0.0, mean = 0.0, M2 = 0.0;
  for (int t = t0; t < t1; ++t) {
    const long long left = prm.P - (long long)t * kRoPT;
    const double nb = left < kRoPT ? (double)left : (double)kRoPT;
    const double* p = prm.part + ((size_t)fil * n_tiles + t) * 2 * Dpad + col;
    chan_merge(n, mean, M2, nb, p[0], p[Dpad]);
  }
  sn[run][cl] = n;
  sm[run][cl] = mean;
  sq[run][cl] = M2;
  __syncthreads();
  if (run == 0 && col < prm.D) {
    for (int r = 1; r < 16; ++r) chan_merge(n, mean, M2, sn[r][cl], sm[r][cl], sq[r][cl]);
    double* out = prm.out + fil * 2 * prm.D;
    out[col] = mean;
    out[prm.D + col] = M2 / n;
  }
}

void launch_obs_readout(const ReadoutParams& p, hipStream_t s) {
  const int tiles = readout_tiles(p.P);
  const int F = p.F > 0 ? p.F : 1;                           // (a zero-initialised F: one cloud)
  hipLaunchKernelGGL(k_obs_readout, dim3(tiles, p.n_groups, F), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_obs_readout_finish, dim3(p.n_groups * kRoGC / 16, F), dim3(256), 0, s, p, tiles);
}

}  // namespace gpmdm
