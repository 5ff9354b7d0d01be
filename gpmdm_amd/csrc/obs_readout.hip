// The mean-only observation tile and its finish (obs_readout.h): gpmdm_pf_observation.
#include "obs_readout_tile.h"

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
  __shared__ RoTileLds sh;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x, G = blockIdx.y;
  const long long fil = blockIdx.z;                          // the filter (a bank: tiles are cut within it)
  const int li = lane & 15, lk = lane >> 4;
  d4 acc[4];
  ro_tile_means(prm, sh, tile, G, fil, acc);                 // the K loop (obs_readout_tile.h)

  // ---- epilogue: C/D layout lane l, reg r -> particle row mt 16 + (l >> 4) + 4 r, column l & 15
  const long long left = prm.P - (long long)tile * kRoPT;
  const int n = left < kRoPT ? (int)left : kRoPT;            // the tile's count
  double mean, m2;
  ro_tile_moments(acc, n, lk, mean, m2);
  if (lk == 0) {
    const int Dpad = prm.n_groups * kRoGC;
    // two planes per tile, so each value is an 8-byte store of its own (no 16-byte VGPR
    // stores in this code base: tests/test_isa_guard.py)
    double* o = prm.part + ((size_t)fil * gridDim.x + tile) * 2 * Dpad + kRoGC * G + 16 * w + li;
    o[0] = mean;
    o[Dpad] = m2;
  }
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
