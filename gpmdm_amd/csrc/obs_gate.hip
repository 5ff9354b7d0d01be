// The gate's decision, the re-weigh tile and its finish (obs_gate.h): gpmdm_pf_set_gate,
// gpmdm_bank_set_gate.
#include "obs_gate.h"

#include "common.h"
#include "obs_readout_tile.h"

namespace gpmdm {

constexpr int kB = 256;   // threads per block, as the filter's O(P) kernels

// one filter's rows of the decision's inputs
struct GateRow {
  const double* innov;               // 7 D + 1
  const unsigned char* mask;         // D, or nullptr
  double threshold;
  int D;
};

__device__ __forceinline__ bool gate_exceeded(const GateRow& r, int j) {
  const bool obs = !r.mask || r.mask[j] != 0;
  return obs && fabs(r.innov[5 * (size_t)r.D + j]) > r.threshold;   // (false for NaN, and for k = +inf)
}

// One workgroup per filter.  The count over all joints first, then each joint's row entries (one
// 8-byte value per lane and store), then thread 0 alone: the kept joints' sums in ascending joint
// order.
__global__ __launch_bounds__(kB) void k_gate_decide(const GateParams p) {
  __shared__ int wc[kB / 64];
  __shared__ double head[kGateHead];
  const int D = p.ro.D, tid = threadIdx.x;
  const size_t fil = blockIdx.x;
  GateRow r;
  r.innov = p.innov + fil * (kInnovFields * (size_t)D + 1);
  r.mask = p.mask ? p.mask + fil * D : nullptr;
  r.threshold = p.cfg[fil * kGateCfg];
  r.D = D;
  const int cap = (int)p.cfg[fil * kGateCfg + 1];
  double* tab = p.tab + fil * (kGateHead + 4 * (size_t)D);
  int c = 0;
  for (int j = tid; j < D; j += kB) c += gate_exceeded(r, j) ? 1 : 0;
  c = wave_sum(c);
  if ((tid & 63) == 0) wc[tid >> 6] = c;
  __syncthreads();
  int n_ex = 0;
  for (int v = 0; v < kB / 64; ++v) n_ex += wc[v];
  const bool gate = n_ex >= 1 && n_ex <= cap;
  double* rows = tab + kGateHead;
  for (int j = tid; j < D; j += kB) {
    const bool obs = !r.mask || r.mask[j] != 0;
    const bool ex = gate_exceeded(r, j);
    rows[j] = r.innov[5 * (size_t)D + j];
    rows[(size_t)D + j] = ex ? 1.0 : 0.0;
    rows[2 * (size_t)D + j] = ex && gate ? 1.0 : 0.0;
    rows[3 * (size_t)D + j] = obs && !(ex && gate) ? 1.0 : 0.0;
  }
  if (tid == 0) {
    int Dp = 0;
    double sl = 0.0;
    for (int j = 0; j < D; ++j) {
      const bool obs = !r.mask || r.mask[j] != 0;
      if (obs && !(gate && gate_exceeded(r, j))) {
        sl += p.log_il2[j];
        ++Dp;
      }
    }
    head[kGateNGated] = gate ? (double)n_ex : 0.0;
    head[kGateNValid] = r.innov[kInnovFields * (size_t)D];
    head[kGateOverflow] = n_ex > cap ? 1.0 : 0.0;
    head[kGateDUsed] = (double)Dp;
    head[kGateSumLog] = sl;
    // D'/2 ln(2 pi) in float32: one IEEE fp32 multiplication (capi_pf.hip install_obs_mask)
    head[kGateConst] = (double)__fmul_rn((float)(0.5 * Dp), (float)1.8378770351409912);
    head[kGateNExceeded] = (double)n_ex;
    head[kGateHead - 1] = 0.0;
  }
  __syncthreads();
  if (tid < kGateHead) tab[tid] = head[tid];                 // one 8-byte value per lane
}

__global__ __launch_bounds__(256) void k_obs_reweigh(const GateParams p) {
  const ReadoutParams& ro = p.ro;
  const long long fil = blockIdx.z;                          // the filter (tiles are cut within it)
  const double* tab = p.tab + fil * (kGateHead + 4 * (long long)ro.D);
  if (tab[kGateNGated] == 0.0) return;                       // nothing gated in this filter: its ll stays (uniform, before any barrier)
  __shared__ RoTileLds sh;
  __shared__ double red[4][kRoPT];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x, G = blockIdx.y;
  const int li = lane & 15, lk = lane >> 4;
  d4 acc[4];
  ro_tile_means(ro, sh, tile, G, fil, acc);                  // the read-out's K loop (obs_readout_tile.h)

  const long long pos0 = (long long)tile * kRoPT;
  const long long left = ro.P - pos0;
  const int n = left < kRoPT ? (int)left : kRoPT;            // the tile's count, within the filter
  const int col = kRoGC * G + 16 * w + li;
  const bool live = col < ro.D && tab[kGateHead + 3 * (size_t)ro.D + col] != 0.0;   // a kept joint
  const double zj = live ? p.z[fil * ro.D + col] : 0.0;
  const double l2 = live ? p.lam2[col] : 0.0;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = mt * 16 + lk + 4 * r;
      const double t = zj - acc[mt][r];
      double v = live && row < n ? t * t * l2 : 0.0;        // (padding and dropped columns: exact zeros)
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 8);
      if (li == 0) red[w][row] = v;
    }
  __syncthreads();
  if (threadIdx.x < n) {
    const int row = threadIdx.x;
    const double s = ((red[0][row] + red[1][row]) + red[2][row]) + red[3][row];
    p.Sp[((size_t)fil * ro.n_groups + G) * ro.P + pos0 + row] = s;
  }
}

// Block (b, f): particles [256 b, 256 b + 256) of filter f.
__global__ __launch_bounds__(kB) void k_gate_finish(const GateParams p) {
  const long long fil = blockIdx.y;
  const double* tab = p.tab + fil * (kGateHead + 4 * (long long)p.ro.D);
  if (tab[kGateNGated] == 0.0) return;                       // (uniform, before any barrier)
  const long long P = p.ro.P;
  const long long o = (long long)blockIdx.x * kB + threadIdx.x;
  unsigned long long key = 0;            // below ord_enc of any double
  if (o < P) {
    const double Dn = tab[kGateDUsed];
    double llv = 0.0;                    // no joint kept: exactly 0, as a blackout frame
    if (Dn != 0.0) {
      const double* Sp = p.Sp + (size_t)fil * p.ro.n_groups * P;
      double S = 0.0;
      for (int g = 0; g < p.ro.n_groups; ++g) S += Sp[(size_t)g * P + o];
      const double vc = p.vc[fil * P + o];
      llv = -0.5 * S / vc - Dn * log(vc) - tab[kGateSumLog] - tab[kGateConst];   // obs_ll_value's expression
    }
    p.ll[fil * P + o] = llv;
    key = ord_enc(fmax(-INFINITY, llv));  // k_norm_max's value set: NaN ignored
  }
  if (p.bmax) block_max_key_store<kB / 64>(key, p.bmax);   // (single filters: grid.y = 1)
}

void launch_gate(const GateParams& p, hipStream_t s) {
  const int tiles = readout_tiles(p.ro.P);
  const unsigned F = p.ro.F > 0 ? (unsigned)p.ro.F : 1u;
  hipLaunchKernelGGL(k_gate_decide, dim3(F), dim3(kB), 0, s, p);
  hipLaunchKernelGGL(k_obs_reweigh, dim3(tiles, p.ro.n_groups, F), dim3(256), 0, s, p);
  hipLaunchKernelGGL(k_gate_finish, dim3((unsigned)((p.ro.P + kB - 1) / kB), F), dim3(kB), 0, s, p);
}

}  // namespace gpmdm
