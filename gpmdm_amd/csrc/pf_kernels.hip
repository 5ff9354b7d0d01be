// Particle-filter kernels around the fused GP tiles (gfx950).
//
//   k_switch        _propogate_markov_switching   gpmdm_pf.py:137-151
//   k_scan_counts   class counts, per-block offsets, this rank's class segments
//   k_group         stable class grouping (the order of gpmdm_pf.py:158-161)
//   k_lead_*        ancestor de-duplication: leader flags, leader rows, their segment tables
//   k_dyn_finish    variance + sample mu + sqrt(var) eps   gpmdm.py:1062-1067, gpmdm_pf.py:167-168
//   k_obs_finish    variance + Gaussian log-likelihood      gpmdm.py:958-961, gpmdm_pf.py:188-192
//   k_obs_ll        the same from the tile kernel's fused partial sums (filter path)
//   k_norm_*        log_w = ll - max, w = exp / sum          gpmdm_pf.py:200-204
//   k_guide/k_resample  torch.multinomial(w, P, True) inverse CDF + gathers  gpmdm_pf.py:206-213
//                   and the read-out partial sums            gpmdm_pf.py:224-262, 302-312
//   k_readout       read-out totals
//   k_small_switch, k_small_resample   the two chains in one workgroup each (P <= 1024)
// Each step of a chain is one device function, called by its kernel of the multi-kernel path and
// by the one-workgroup kernel with another BlockGeo and with LDS mirrors where the multi-kernel
// path reads a buffer back; the wave and workgroup scans and maxima are common.h's, the draws
// pf_kernels.h's (shared with forecast.hip).
// All arithmetic is fp64; every reduction has a fixed order (bitwise run-to-run repeatable).
#include <cstdlib>

#include "common.h"
#include "pf_kernels.h"

namespace gpmdm {

constexpr int kB = 256;   // threads per block of the O(P) kernels
constexpr unsigned kMaxNormBlocks = 128;   // blocks per filter of k_norm_max

// The 256-thread block of the O(P) kernels a thread stands for: a workgroup of the multi-kernel
// path, or a quarter of a one-workgroup kernel's 1024 threads (block b = waves 4b .. 4b+3, so
// every wave-level scan and sum sees the same lanes on either path).
struct BlockGeo {
  int b;    // the block
  int t;    // the thread's index in it
  int wq;   // its wave of the block
};
__device__ __forceinline__ BlockGeo grid_block() {
  return BlockGeo{(int)blockIdx.x, (int)threadIdx.x, (int)threadIdx.x >> 6};
}
__device__ __forceinline__ BlockGeo quarter_block() {
  return BlockGeo{(int)threadIdx.x >> 8, (int)threadIdx.x & 255, ((int)threadIdx.x >> 6) & 3};
}

// The de-duplication key of particle p with new class c and in-filter ancestor anc.
__device__ __forceinline__ long long dedup_key(long long P, long long Pf, int c, long long p, int anc) {
  return (long long)c * P + (p / Pf) * Pf + anc;
}

// ---------------------------------------------------------------------------------
// The switch of particle p: its new class, stored.
__device__ __forceinline__ int switch_particle(const SwitchArgs& a, long long p) {
  const long long f = p / a.Pf;
  const int best = switch_draw(a.T, a.C, a.cls[p], a.E, p, (unsigned)(p - f * a.Pf), a.frame,
                               kStreamSwitch, 0u, filter_key(a.seed_lo, a.seed_hi, f));
  a.cls_new[p] = best;
  return best;
}

// OWN: ancestor-ordered shards (thread i handles particle own[i]); the identity
// instantiation keeps p == i visible to the compiler (one-rank path unchanged).
template <bool OWN>
__global__ __launch_bounds__(kB) void k_switch(SwitchArgs a) {
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < a.C) hist[tid] = 0;
  const long long t = (long long)blockIdx.x * kB + tid;
  const long long i = a.base + t;                   // position in the ownership order
  long long dkey = -1;                              // de-duplication key (owner index)
  unsigned pid = 0;                                 // this thread's particle
  if (a.gmax_reset && t < a.F) a.gmax_reset[t] = ord_enc(-INFINITY);
  __syncthreads();
  if (t < a.n) {
    const long long p = OWN ? (long long)a.own[i] : i;
    pid = (unsigned)p;
    const int best = switch_particle(a, p);
    atomicAdd(&hist[best], 1);
    if (a.owner && i >= a.lo && i < a.hi) dkey = dedup_key(a.P, a.Pf, best, p, a.anc[p]);
  }
  if (a.owner) {
    // Leader election: one atomicMin per distinct key per wave (its lowest lane), so a
    // collapsed cloud (every particle one ancestor) does not serialise P atomics on one
    // address.  The leader is deterministic; which particle leads does not change any value.
    // (k_small_switch, at most 1024 particles, issues one atomicMin per particle instead.)
    const int lane = tid & 63;
    unsigned long long pending = __ballot(dkey >= 0);
    while (pending) {
      const int l0 = __ffsll((long long)pending) - 1;
      const unsigned lo32 = __shfl((unsigned)(dkey & 0xffffffffll), l0);
      const int hi32 = __shfl((int)(dkey >> 32), l0);
      const long long k0 = ((long long)hi32 << 32) | lo32;
      const unsigned long long same = __ballot(dkey == k0);
      if (lane == l0) atomicMin(&a.owner[k0], pid);
      pending &= ~same;
    }
  }
  __syncthreads();
  if (tid < a.C) a.blockcounts[(long long)blockIdx.x * a.C + tid] = hist[tid];
}

// ---------------------------------------------------------------------------------
// One thread: the class table pass.  tot / lo_cnt / hi_cnt: per class its particles, and those
// among positions [0, lo) and [0, hi) of the ownership order.  class_start and seg_t: C + 1.
__device__ __forceinline__ void class_seg_tables(int C, int pt, const int* tot, const int* lo_cnt, const int* hi_cnt,
                                                 int* class_start, int* seg_b, int* seg_e, int* seg_o, int* seg_t,
                                                 int* counts, int* counts_host) {
  int cs = 0, ob = 0, ts = 0;
  for (int c = 0; c < C; ++c) {
    class_start[c] = cs;
    if (counts) counts[c] = tot[c];
    if (counts_host) counts_host[c] = tot[c];
    const int b0 = cs + lo_cnt[c], e0 = cs + hi_cnt[c];
    seg_b[c] = b0;
    seg_e[c] = e0;
    seg_o[c] = ob;
    seg_t[c] = ts;
    ob += e0 - b0;
    ts += (e0 - b0 + pt - 1) / pt;
    cs += tot[c];
  }
  class_start[C] = cs;
  seg_t[C] = ts;
}

// One workgroup: exclusive scans of the per-block class counts, class starts, and the
// segments (grouped position ranges) of this rank's particle slice [lo, hi).
__global__ __launch_bounds__(1024) void k_scan_counts(ScanArgs a) {
  __shared__ int tot[kMaxClasses];
  __shared__ int lo_cnt[kMaxClasses], hi_cnt[kMaxClasses];
  const int tid = threadIdx.x;
  const int nb = a.nb;
  for (int c = 0; c < a.C; ++c) {
    const int total = chunked1024_exclusive_scan(a.blockcounts + c, a.blockoff + c, a.C, nb, 0, OpSum(),
                                                 [](int x, int* t) { return block1024_exclusive_sum(x, t); });
    if (tid == 0) tot[c] = total;
  }
  __syncthreads();
  // counts of each class among particles [0, lo) and [0, hi)
  if (tid < a.C) { lo_cnt[tid] = 0; hi_cnt[tid] = 0; }
  __syncthreads();
  for (int which = 0; which < 2; ++which) {
    const long long bound = which ? a.hi : a.lo;
    const long long bb = bound / kB;
    const long long start = bb * kB;
    if (tid < kB && start + tid < bound) {
      const long long q = a.base + start + tid;
      const int cc = a.cls_new[a.own ? a.own[q] : q];
      atomicAdd(which ? &hi_cnt[cc] : &lo_cnt[cc], 1);
    }
    __syncthreads();
    if (tid < a.C) {
      const int base = bb < nb ? a.blockoff[bb * a.C + tid] : tot[tid];
      if (which) hi_cnt[tid] += base; else lo_cnt[tid] += base;
    }
    __syncthreads();
  }
  if (tid == 0) {
    class_seg_tables(a.C, a.pt, tot, lo_cnt, hi_cnt, a.class_start, a.seg_pos_begin, a.seg_pos_end, a.seg_out_base,
                     a.seg_tile_start, a.counts, a.counts_host);
    if (a.counts_seq_host)              // the host waits on this number, not on an event
      publish_seq(a.counts_seq_host, a.counts_seq);   // (this thread wrote counts_host above)
  }
}

// ---------------------------------------------------------------------------------
// The stable class grouping of one block: the grouped position of the thread's particle of
// class c (c < 0: no particle, returns -1).  wcount: the block's wave counts per class (LDS);
// blockoff: the block's row of class offsets.  Contains a barrier.
__device__ __forceinline__ int group_position(int c, int C, BlockGeo g, int (*wcount)[kMaxClasses],
                                              const int* class_start, const int* blockoff) {
  int rank = 0;
  for (int k = 0; k < C; ++k) {
    int n;
    const int r = ballot_rank(c == k, &n);
    if (c == k) rank = r;
    if ((g.t & 63) == 0) wcount[g.wq][k] = n;
  }
  __syncthreads();
  if (c < 0) return -1;
  int off = class_start[c] + blockoff[c];
  for (int v = 0; v < g.wq; ++v) off += wcount[v][c];
  return off + rank;
}

template <bool OWN>
__global__ __launch_bounds__(kB) void k_group(GroupArgs a) {
  __shared__ int wcount[kB / 64][kMaxClasses];
  const long long t = (long long)blockIdx.x * kB + threadIdx.x;
  const long long i = a.base + t;                         // position in the ownership order
  const long long p = t < a.n ? (OWN ? (long long)a.own[i] : i) : -1;
  const int c = p >= 0 ? a.cls_new[p] : -1;
  const int pos = group_position(c, a.C, grid_block(), wcount, a.class_start,
                                 a.blockoff + (long long)blockIdx.x * a.C);
  if (pos >= 0) a.perm[pos] = (int)p;
}

// ---------------------------------------------------------------------------------
// Ancestor de-duplication of the dynamics GP.  After a resample, every
// offspring of one ancestor holds a bit-identical copy of its state, and the dynamics GP
// of (state, class) does not depend on anything else, so the tile kernel only needs one
// row per distinct (ancestor, new class) key of this rank's slice: its leader (the
// smallest particle index, k_switch's atomicMin).  Leaders are compacted in class-grouped
// position order, so leader rows of class c are contiguous and the tile kernel's segment
// tables keep their meaning.  Per-particle arithmetic is independent of which rows share a
// tile, so the results are bitwise those of the undeduplicated path.
//
// The lflag_scan entry of a position with leader flag lf: flag | block-local exclusive count
// << 1.  wc: the block's wave counts (LDS), left for the caller's block total.  Contains a barrier.
__device__ __forceinline__ int lead_flag_scan(int lf, BlockGeo g, int* wc) {
  int n;
  const int excl = ballot_rank(lf, &n);
  if ((g.t & 63) == 0) wc[g.wq] = n;
  __syncthreads();
  int base = 0;
  for (int v = 0; v < g.wq; ++v) base += wc[v];
  return ((base + excl) << 1) | lf;
}

__global__ __launch_bounds__(kB) void k_lead_flags(LeadArgs a) {
  __shared__ int wc[kB / 64];
  const long long pos = (long long)blockIdx.x * kB + threadIdx.x;
  int lf = 0;
  if (pos < a.npos) {
    const long long p = a.perm[pos];
    // only this rank's slice registered owners, so owner == p also means "p is in the slice"
    lf = a.owner[dedup_key(a.P, a.Pf, a.cls_new[p], p, a.anc[p])] == (unsigned)p;
  }
  const int v = lead_flag_scan(lf, grid_block(), wc);
  if (pos < a.npos) a.lflag_scan[pos] = v;
  if (threadIdx.x == 0) {
    int t = 0;
    for (int u = 0; u < kB / 64; ++u) t += wc[u];
    a.lblock[blockIdx.x] = t;
  }
}

// One thread: the leader segment tables.  Leaders before position x: pre[x / kB] (its block's
// exclusive offset) + lflag[x] >> 1, and `total` from npos on.
__device__ __forceinline__ void lead_seg_tables(int C, int pt, long long npos, int total, const int* pre,
                                                const int* lflag, const int* seg_b, const int* seg_e, int* lseg_b,
                                                int* lseg_e, int* lseg_o, int* lseg_t) {
  auto row = [&](long long x) { return x >= npos ? total : pre[x / kB] + (lflag[x] >> 1); };
  int ts = 0;
  for (int c = 0; c < C; ++c) {
    const int b0 = row(seg_b[c]), e0 = row(seg_e[c]);
    lseg_b[c] = b0;
    lseg_e[c] = e0;
    lseg_o[c] = b0;
    lseg_t[c] = ts;
    ts += (e0 - b0 + pt - 1) / pt;
  }
  lseg_t[C] = ts;
}

// One workgroup: lblock -> exclusive offsets (in place), then the leader segment tables.
__global__ __launch_bounds__(1024) void k_lead_tables(LeadArgs a) {
  const int total = chunked1024_exclusive_scan(a.lblock, a.lblock, 1, a.nb, 0, OpSum(),
                                               [](int x, int* t) { return block1024_exclusive_sum(x, t); });
  __syncthreads();
  if (threadIdx.x == 0)
    lead_seg_tables(a.C, a.pt, a.npos, total, a.lblock, a.lflag_scan, a.seg_pos_begin, a.seg_pos_end,
                    a.lseg_pos_begin, a.lseg_pos_end, a.lseg_out_base, a.lseg_tile_start);
}

// The leader row of position pos, if it holds a leader: first (its block's first row) + the
// block-local count.
__device__ __forceinline__ void lead_compact_row(const LeadArgs& a, const int* lflag, const int* perm,
                                                 const int* cls_new, const int* anc, long long pos, int first) {
  if (pos >= a.npos) return;
  const int v = lflag[pos];
  if (!(v & 1)) return;
  const long long p = perm[pos];
  const int r = first + (v >> 1);
  a.lperm[r] = (int)p;
  const long long key = dedup_key(a.P, a.Pf, cls_new[p], p, anc[p]);
  a.slot[key] = r;
  if (a.owner_reset) a.owner_reset[key] = 0xffffffffu;   // the next election's preset
}
__global__ __launch_bounds__(kB) void k_lead_compact(LeadArgs a) {
  lead_compact_row(a, a.lflag_scan, a.perm, a.cls_new, a.anc, (long long)blockIdx.x * kB + threadIdx.x,
                   a.lblock[blockIdx.x]);
}

// k_lead_tables + k_lead_compact in one launch (nb <= kMaxLeadBlocks): block b's first leader
// row is the sum of the leader counts of blocks 0 .. b-1, which the block adds up itself
// (integers: any order gives k_lead_tables's prefix; a re-sum per block, where k_lead_tables
// scans once, is what saves the launch); block 0 also scans every block's count
// and writes the leader segment tables with k_lead_tables's row rule.  Same rows, same tables.
// Up to 1024 blocks (P <= 262,144 per launch): each block's prefix re-sum is O(nb) loads and
// block 0's table is 4 KB of static LDS in every block; above, the two launches (ADVICE r5:
// at nb = 8192 the re-sums were ~33M loads and a 32 KB table limited occupancy).
constexpr int kMaxLeadBlocks = 1024;
__global__ __launch_bounds__(kB) void k_lead_tables_compact(LeadArgs a) {
  __shared__ int red[kB / 64];
  __shared__ int pre[kMaxLeadBlocks];          // block 0: exclusive prefix of every block's count
  __shared__ int total_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, nb = a.nb;
  int s = 0;
  for (int bb = tid; bb < b; bb += kB) s += a.lblock[bb];
  s = wave_sum(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  int first = 0;
#pragma unroll
  for (int v = 0; v < kB / 64; ++v) first += red[v];
  if (b == 0) {
    // exclusive scan of the counts: per thread a chunk of consecutive blocks, then a
    // 256-wide scan of the chunk sums
    const int chunk = (nb + kB - 1) / kB;
    int cs = 0;
    for (int i = 0; i < chunk; ++i) {
      const int bb = tid * chunk + i;
      if (bb < nb) cs += a.lblock[bb];
    }
    __syncthreads();                           // (red is reused)
    int run = block_inclusive_scan(cs, 0, OpSum(), red, w) - cs;
    for (int i = 0; i < chunk; ++i) {
      const int bb = tid * chunk + i;
      if (bb < nb) {
        pre[bb] = run;
        run += a.lblock[bb];
      }
    }
    if (tid == kB - 1) total_s = run;
    __syncthreads();
    if (tid == 0)
      lead_seg_tables(a.C, a.pt, a.npos, total_s, pre, a.lflag_scan, a.seg_pos_begin, a.seg_pos_end,
                      a.lseg_pos_begin, a.lseg_pos_end, a.lseg_out_base, a.lseg_tile_start);
  }
  lead_compact_row(a, a.lflag_scan, a.perm, a.cls_new, a.anc, (long long)b * kB + tid, first);
}


// ---------------------------------------------------------------------------------
// Small single-shard filters (all P <= kSmallSwitchP particles switched by one rank, no
// ownership order): one 1024-thread workgroup runs the switch, the class scan, the grouping
// and the leader compaction in one launch instead of seven (with the owner preset).  The steps
// are the multi-kernel path's own device functions, called with the workgroup's quarters as the
// 256-thread blocks; what that path reads back from its buffers is kept in LDS and handed to
// the step functions in the buffers' place (the buffers are still written for the later
// stages), so every table is the multi-kernel path's exactly (tests/test_gpu_small_path.py).
// Three things are its own, each integer and deterministic (the leader of a key is its smallest
// particle index, whatever the order of the atomics; integer sums in any order are equal):
//  * one atomicMin per particle instead of k_switch's per-wave election: at most 1024 atomics;
//  * the scans over at most four blocks are serial, one thread per class (or one thread),
//    instead of 1024-wide passes;
//  * the owners were set by this launch's own atomics (at L2), so the leader flags read them
//    with an atomic load past the L1.
constexpr long long kSmallSwitchP = 1024;

__global__ __launch_bounds__(1024) void k_small_switch(SwitchArgs sa, ScanArgs sc, GroupArgs ga, LeadArgs la,
                                                       int dedup) {
  __shared__ int hist[4][kMaxClasses];        // block counts (blockcounts)
  __shared__ int boff[4][kMaxClasses];        // block offsets (blockoff)
  __shared__ int cstart[kMaxClasses + 1];     // class_start
  __shared__ int lo_cnt[kMaxClasses], hi_cnt[kMaxClasses];
  __shared__ int segb[kMaxClasses], sege[kMaxClasses], sego[kMaxClasses], segt[kMaxClasses + 1];
  __shared__ int ctot[kMaxClasses];           // counts
  __shared__ int lsegb[kMaxClasses], lsege[kMaxClasses], lsegt[kMaxClasses + 1];
  __shared__ int wcount[4][4][kMaxClasses];
  __shared__ int wc[4][4];
  __shared__ int lblk[4], ltot;               // lblock (exclusive offsets), all leaders
  __shared__ int cls_s[kSmallSwitchP];        // cls_new
  __shared__ int anc_s[kSmallSwitchP];        // anc
  __shared__ int perm_s[kSmallSwitchP];       // perm
  __shared__ int lflag_s[kSmallSwitchP];      // lflag_scan
  const int tid = threadIdx.x;
  const BlockGeo g = quarter_block();
  const long long P = sa.P;
  const int C = sa.C;
  const int nb = (int)((P + kB - 1) / kB);
  if (dedup)
    for (long long i = tid; i < (long long)C * P; i += 1024) sa.owner[i] = 0xffffffffu;
  if (tid < 4 * kMaxClasses) hist[tid / kMaxClasses][tid % kMaxClasses] = 0;
  if (tid < kMaxClasses) { lo_cnt[tid] = 0; hi_cnt[tid] = 0; }
  if (sa.gmax_reset && tid < sa.F) sa.gmax_reset[tid] = ord_enc(-INFINITY);
  __threadfence();                            // the owner preset lands before the atomics
  __syncthreads();
  // ---- k_switch ----
  const long long p = tid;
  int best = -1;
  if (p < P) {
    best = switch_particle(sa, p);
    cls_s[p] = best;
    atomicAdd(&hist[g.b][best], 1);
    if (dedup) {
      const int an = sa.anc[p];
      anc_s[p] = an;
      if (p >= sa.lo && p < sa.hi) atomicMin(&sa.owner[dedup_key(P, sa.Pf, best, p, an)], (unsigned)p);
    }
  }
  __syncthreads();
  // ---- k_scan_counts ----
  if (tid < nb * C) sa.blockcounts[tid] = hist[tid / C][tid % C];   // block bb, class c: bb * C + c
  if (tid < C) {
    int run = 0;
    for (int bb = 0; bb < nb; ++bb) {
      boff[bb][tid] = run;
      sc.blockoff[(long long)bb * C + tid] = run;
      run += hist[bb][tid];
    }
    ctot[tid] = run;
  }
  // class counts among positions [0, lo) and [0, hi): the partial block by atomics, then the
  // whole blocks before it
  for (int which = 0; which < 2; ++which) {
    const long long bound = which ? sc.hi : sc.lo;
    const long long start = (bound / kB) * kB;
    if (tid < kB && start + tid < bound) atomicAdd(which ? &hi_cnt[cls_s[start + tid]] : &lo_cnt[cls_s[start + tid]], 1);
  }
  __syncthreads();
  if (tid < C) {
    const long long blo = sc.lo / kB, bhi = sc.hi / kB;
    lo_cnt[tid] += blo < nb ? boff[blo][tid] : ctot[tid];
    hi_cnt[tid] += bhi < nb ? boff[bhi][tid] : ctot[tid];
  }
  __syncthreads();
  if (tid == 0) class_seg_tables(C, sc.pt, ctot, lo_cnt, hi_cnt, cstart, segb, sege, sego, segt, nullptr, nullptr);
  __syncthreads();
  // the tables, one entry per lane (a one-thread loop of stores is vectorised into wide
  // stores, which tests/test_isa_guard.py rejects)
  if (tid < C) {
    sc.class_start[tid] = cstart[tid];
    sc.counts[tid] = ctot[tid];
    if (sc.counts_host) sc.counts_host[tid] = ctot[tid];
    sc.seg_pos_begin[tid] = segb[tid];
    sc.seg_pos_end[tid] = sege[tid];
    sc.seg_out_base[tid] = sego[tid];
    sc.seg_tile_start[tid] = segt[tid];
  } else if (tid == C) {
    sc.class_start[C] = cstart[C];
    sc.seg_tile_start[C] = segt[C];
  }
  // ---- k_group ----
  const int gpos = group_position(best, C, g, wcount[g.b], cstart, boff[g.b]);
  if (gpos >= 0) {
    ga.perm[gpos] = (int)p;
    perm_s[gpos] = (int)p;
  }
  __syncthreads();
  if (!dedup) return;
  // ---- k_lead_flags ----
  int lf = 0;
  if (p < la.npos) {
    const long long q = perm_s[p];
    lf = __hip_atomic_load(&la.owner[dedup_key(la.P, la.Pf, cls_s[q], q, anc_s[q])], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT) == (unsigned)q;
  }
  const int lv = lead_flag_scan(lf, g, wc[g.b]);
  if (p < la.npos) {
    la.lflag_scan[p] = lv;
    lflag_s[p] = lv;
  }
  // ---- k_lead_tables ----
  if (tid == 0) {
    int run = 0;
    for (int bb = 0; bb < nb; ++bb) {
      lblk[bb] = run;
      for (int v = 0; v < kB / 64; ++v) run += wc[bb][v];
    }
    ltot = run;
  }
  __syncthreads();
  if (tid == 0) lead_seg_tables(C, la.pt, la.npos, ltot, lblk, lflag_s, segb, sege, lsegb, lsege, lsegb, lsegt);
  __syncthreads();
  if (tid < C) {
    la.lseg_pos_begin[tid] = lsegb[tid];
    la.lseg_pos_end[tid] = lsege[tid];
    la.lseg_out_base[tid] = lsegb[tid];
    la.lseg_tile_start[tid] = lsegt[tid];
  } else if (tid == C) {
    la.lseg_tile_start[C] = lsegt[C];
  }
  // ---- k_lead_compact (la.owner_reset is nullptr here: the preset above is this kernel's) ----
  if (tid < nb) la.lblock[tid] = lblk[tid];
  lead_compact_row(la, lflag_s, perm_s, cls_s, anc_s, p, lblk[g.b]);
}

// ---------------------------------------------------------------------------------
// Failure counters: one atomic per wave for the lanes that saw the event (events are rare;
// a collapsed or indefinite model can make every particle bad, hence the ballot).
__device__ __forceinline__ void count_event(unsigned* ctr, bool bad) {
  const unsigned long long b = __ballot(bad);
  if (b && (int)(threadIdx.x & 63) == __ffsll((long long)b) - 1) atomicAdd(ctr, (unsigned)__popcll(b));
}

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void k_dyn_finish(DynFinishArgs a) {
  const long long o = (long long)blockIdx.x * kB + threadIdx.x;
  if (a.gmax_reset && o < a.F) a.gmax_reset[o] = ord_enc(-INFINITY);
  if (o < a.z_n) a.z_dst[o] = a.z_src[o];
  if (a.rows_out && o == 0) {
    int r = 0;
    for (int c = 0; c < a.n_rows_seg; ++c) r += a.rows_e[c] - a.rows_b[c];
    a.rows_out[0] = r;
    if (a.rows_host) a.rows_host[0] = r;
  }
  if (o >= a.n_out) return;
  const int c = a.seg_out_base ? seg_of(a.seg_out_base, a.n_seg, o) : 0;
  const long long pos = (a.seg_pos_begin ? a.seg_pos_begin[c] : 0) + (o - (a.seg_out_base ? a.seg_out_base[c] : 0));
  const long long p = a.perm ? a.perm[pos] : pos;
  long long r = o;                      // tile row holding this particle's GP outputs
  if (a.slot) r = a.slot[dedup_key(a.P, a.Pf, c, p, a.anc[p])];
  const int d = a.d;
  const double vc = dyn_vc(a.qpart, a.ld_q, a.n_parts[c], r, a.X + p * d, a.lin_c2, d);
  if (a.var_out) {                      // predictive map (map_x_dynamics_for_class)
    for (int j = 0; j < d; ++j) a.var_out[o * d + j] = vc * a.il2[j];
    return;
  }
  bool bad_state = false;
  // torch.normal(mean, std) = eps * std + mean (gpmdm_pf.py:167-168)
  for (int j = 0; j < d; j += 2) {
    double e0, e1 = 0.0;
    if (a.normals) {
      e0 = a.normals[pos * d + j];
      if (j + 1 < d) e1 = a.normals[pos * d + j + 1];
    } else {
      const long long f = p / a.Pf;
      const uint4 r = philox4x32_10(make_uint4((unsigned)(p - f * a.Pf), a.frame, kStreamDyn, (unsigned)(j >> 1)),
                                    filter_key(a.seed_lo, a.seed_hi, f));
      const double u1 = u01_oo(r.x, r.y), u2 = u01_co(r.z, r.w);
      const double rr = sqrt(-2.0 * log(u1));
      double sn, cs;
      sincos(6.283185307179586476925 * u2, &sn, &cs);   // (Box-Muller; k_fc_finish has the same lines)
      e0 = rr * cs;
      e1 = rr * sn;
    }
    const double x0 = e0 * sqrt(vc * a.il2[j]) + a.mu[r * a.ld_mu + j];
    a.X_out[p * d + j] = x0;
    bad_state |= !isfinite(x0);
    if (j + 1 < d) {
      const double x1 = e1 * sqrt(vc * a.il2[j + 1]) + a.mu[r * a.ld_mu + j + 1];
      a.X_out[p * d + j + 1] = x1;
      bad_state |= !isfinite(x1);
    }
  }
  if (a.health) {
    count_event(a.health + kHealthDynVar, !(vc > 0.0));
    count_event(a.health + kHealthDynState, bad_state);
  }
}

// ---------------------------------------------------------------------------------
// One wave per particle: the D-term log-likelihood sum is spread over 64 lanes.
__global__ __launch_bounds__(kB) void k_obs_finish(ObsFinishArgs a) {
  const int lane = threadIdx.x & 63;
  const long long o = (long long)blockIdx.x * (kB / 64) + (threadIdx.x >> 6);
  double llv = -INFINITY;
  if (o < a.n_out) {
    double q = 0.0;
    for (int k = lane; k < a.n_parts; k += 64) q += a.qpart[(long long)k * a.ld_q + o];
    q = wave_sum(q);
    const double vc = 1.0 - q;                         // k(x*,x*) = 1 (gpmdm.py:991)
    const double* mu = a.mu + o * a.ld_mu;
    if (a.var_out) {
      for (int j = lane; j < a.D; j += 64) a.var_out[o * a.D + j] = vc * a.il2[j];
    } else {
      // ll = -1/2 sum[(z-mu)^2/var + log var] + sum(-log sqrt var) - D/2 ln(2pi)_f32
      const double* z = a.z + ((a.ll_offset + o) / a.Pf) * a.D;
      double s1 = 0.0, s2 = 0.0;
      for (int j = lane; j < a.D; j += 64) {
        const double var = vc * a.il2[j];
        const double t = z[j] - mu[j];
        s1 += t * t / var + log(var);
        s2 += -log(sqrt(var));
      }
      s1 = wave_sum(s1);
      s2 = wave_sum(s2);
      llv = -0.5 * s1 + s2 - a.ll_const;
      if (lane == 0) a.ll[a.ll_offset + o] = llv;
    }
  }
}

// Fused form of k_obs_finish for the filter (one thread per particle): the tile kernel
// left S = sum_j (z_j - mu_j)^2 lam2_j in spart, and with var_j = vc il2_j
//   ll = -1/2 sum_j[(z_j - mu_j)^2 / var_j + log var_j] + sum_j(-log sqrt var_j) - D/2 ln(2pi)_f32
//      = -1/2 S / vc - D log vc - sum_j log il2_j - D/2 ln(2pi)_f32
// (the reference's double count of log var kept, gpmdm_pf.py:188-192).
__device__ __forceinline__ double obs_ll_value(const ObsFinishArgs& a, long long o, double& vc) {
  double Dn = a.D, sum_log_il2 = a.sum_log_il2, ll_const = a.ll_const;
  if (a.ftab) {
    // a masked bank: the three scalars of the filter that owns this output's particle
    const long long pi = a.own ? a.own[a.ll_offset + o] : a.ll_offset + o;
    const double* row = a.ftab + 3 * (pi / a.Pf);
    Dn = row[0];
    sum_log_il2 = row[1];
    ll_const = row[2];
    if (Dn == 0.0) {
      // blackout: ll is exactly 0 whatever the tiles left (0 * log(vc) is NaN for vc <= 0),
      // and nothing for the health counters
      vc = 1.0;
      return 0.0;
    }
  }
  double q = 0.0;
  for (int k = 0; k < a.n_parts; ++k) q += a.qpart[(long long)k * a.ld_q + o];
  double S = 0.0;
  for (int k = a.jm0; k < a.n_j; ++k) S += a.spart[(long long)k * a.ld_q + o];
  if (a.cut_part && o >= a.cut_o0) {
    // a split tile: its first part left q and S over list entries [0, tpc c*); the second
    // part's entries follow in list order (R tiles into q, then mean tiles into S), the whole
    // tile's running sums exactly
    const long long r = o - a.cut_o0;
    const int2 sp = a.cut_split[r / a.cut_pt];
    const int nt = sp.x + a.cut_tm;
    const int r0 = cutoff_chunk_begin(1, nt, a.cut_tpc);
    const double* pp = a.cut_part + r;
    int i = cutoff_chunk_begin(sp.y, nt, a.cut_tpc);
    for (; i + 8 <= nt; i += 8) {              // eight loads in flight, then the adds in order
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = pp[(long long)(i + k - r0) * a.cut_ld];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (i + k < sp.x)
          q += v[k];
        else
          S += v[k];
      }
    }
    for (; i < nt; ++i) {
      const double v = pp[(long long)(i - r0) * a.cut_ld];
      if (i < sp.x)
        q += v;
      else
        S += v;
    }
  }
  vc = 1.0 - q;                                        // k(x*,x*) = 1 (gpmdm.py:991)
  return -0.5 * S / vc - Dn * log(vc) - sum_log_il2 - ll_const;
}

// The likelihood finish of output o (live: o < n_out; every thread of the wave calls it, for
// the counters' ballots): ll stored at the output's particle, the vc a predictive filter keeps
// (ObsFinishArgs::vc_out: the vc that obs_ll_value formed, or NaN where it returned early, a
// masked bank's blacked-out filter), the health counters.  Returns ll (0 for a dead thread).
__device__ __forceinline__ double obs_ll_step(const ObsFinishArgs& a, long long o, bool live) {
  double vc = 1.0, llv = 0.0;
  if (live) {
    llv = obs_ll_value(a, o, vc);
    const long long pi = a.own ? a.own[a.ll_offset + o] : a.ll_offset + o;
    a.ll[pi] = llv;
    if (a.vc_out)
      a.vc_out[pi] = a.ftab && a.ftab[3 * (pi / a.Pf)] == 0.0 ? __longlong_as_double(0x7ff8000000000000ll) : vc;
  }
  if (a.health) {
    count_event(a.health + kHealthObsVar, live && !(vc > 0.0));
    count_event(a.health + kHealthObsLL, live && !isfinite(llv));
  }
  return llv;
}

__global__ __launch_bounds__(kB) void k_obs_ll(ObsFinishArgs a) {
  const long long o = (long long)blockIdx.x * kB + threadIdx.x;
  const bool live = o < a.n_out;
  const double llv = obs_ll_step(a, o, live);
  // k_norm_max's value set: NaN ignored; a dead thread's key is below ord_enc of any double
  if (a.bmax) block_max_key_store<kB / 64>(live ? ord_enc(fmax(-INFINITY, llv)) : 0ull, a.bmax);
}

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void k_norm_max(NormArgs a) {
  __shared__ double s[kB / 64];
  const long long f = blockIdx.y;
  // grid-stride over the filter's particles: at most kMaxNormBlocks atomics per filter
  // address (one per block; thousands of same-address atomics serialise at the L2)
  double v = -INFINITY;
  for (long long p = (long long)blockIdx.x * kB + threadIdx.x; p < a.P; p += (long long)gridDim.x * kB)
    v = fmax(v, a.ll[f * a.P + p]);
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = s[0];
    for (int i = 1; i < kB / 64; ++i) m = fmax(m, s[i]);
    atomicMax(a.gmax + f, ord_enc(m));
  }
}

// e = exp(ll - max); block-local inclusive scan of e; block sums.
__global__ __launch_bounds__(kB) void k_norm_exp_scan(NormArgs a) {
  __shared__ double wsum[kB / 64];
  __shared__ unsigned long long wk[kB / 64];
  const int tid = threadIdx.x;
  const long long f = blockIdx.y;
  const long long p = (long long)blockIdx.x * kB + tid;
  double M;
  if (a.bmax) {
    // single filter: the maximum over k_obs_ll's block maxima (no k_norm_max launch); every
    // block computes it, block 0 publishes it for the resample and export
    unsigned long long key = 0;
    const int nk = a.nbmax ? a.nbmax : a.nb;
    for (int i = tid; i < nk; i += kB) key = a.bmax[i] > key ? a.bmax[i] : key;
    key = block_max_key<kB / 64>(key, wk);
    if (blockIdx.x == 0 && tid == 0) a.gmax[f] = key;
    M = ord_dec(key);
  } else {
    M = ord_dec(a.gmax[f]);
  }
  const double e = p < a.P ? exp(a.ll[f * a.P + p] - M) : 0.0;
  if (p < a.P) a.e[f * a.P + p] = e;
  const double x = block_inclusive_scan(e, 0.0, OpSum(), wsum, tid >> 6);
  if (p < a.P) a.local[f * a.P + p] = x;
  if (tid == kB - 1) a.blocksum[f * a.nb + blockIdx.x] = x;
}

// One workgroup per filter: exclusive scan of block sums, total S.  The Hillis-Steele form:
// k_small_resample reproduces its association.
__global__ __launch_bounds__(1024) void k_norm_total(NormArgs a) {
  const long long f = blockIdx.x;
  const double S =
      chunked1024_exclusive_scan(a.blocksum + f * a.nb, a.blockoff + f * a.nb, 1, a.nb, 0.0, OpSum(),
                                 [](double x, double* t) { return block1024_exclusive_scan_hs(x, 0.0, OpSum(), t); });
  if (threadIdx.x == 1023) a.total[f] = S;
}

// The normalised CDF of filter f at particle i: k_norm_exp_scan's block-local inclusive scan
// plus k_norm_total's block offset, over the total, the last bucket forced to 1 (torch:
// cumsum(w) / sum, gpmdm_pf.py:206-213).  Evaluated where the inverse-CDF searches read it
// (k_guide, k_sys_marks, k_resample) instead of stored by a CDF pass: the same expression on
// the same operands, so every value -- and every index -- is the stored CDF's, one dependent
// launch fewer per frame.
//
// Not monotone to the last ulp for general weights: boff[b] (a Hillis-Steele prefix) and
// boff[b-1] + local[last of b-1] are two associations of one sum, the lanes of a wave scan add
// in different orders, and a value before the last can exceed the forced 1.  The dips are a few
// ulps (a host model of this summation order: tests/resample_ref.py, device_association_cdf),
// far inside the (P + 8) 2^-53 band that any order of summing P non-negative terms has, so a
// search that meets one still returns an ancestor whose exact CDF interval holds u to rounding.
// tests/test_gpu_resample_edges.py holds every search form to that band, and to ancestors that
// do not decrease with u, with uniforms placed on the CDF's values at every block boundary;
// with weights in {0, 1} every sum is an integer, the CDF is monotone and the ancestors are
// np.searchsorted's exactly.
__device__ __forceinline__ double cdf_value(double boff, double local, double S, bool last) {
  return last ? 1.0 : (boff + local) / S;
}
struct CdfView {
  const double* boff;
  const double* local;
  double S;
  long long P;
  __device__ __forceinline__ double operator[](long long i) const {
    return cdf_value(boff[i / kB], local[i], S, i == P - 1);
  }
};
__device__ __forceinline__ CdfView cdf_view(const ResampleArgs& a, long long f) {
  return CdfView{a.blockoff + f * a.nb, a.local + f * a.P, a.total[f], a.P};
}
// First index of [lo, hi) with cum >= u, hi if none (torch's searchsorted); cum: a CdfView, or
// the CDF's values in LDS.
template <class Cdf>
__device__ __forceinline__ long long cdf_search(const Cdf& cum, double u, long long lo, long long hi) {
  while (hi - lo > 0) {
    const long long mid = lo + (hi - lo) / 2;
    if (cum[mid] < u) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One thread per output slot s: inverse-CDF search, gather, read-out partials.
// identity=1 computes the read-outs of the current state without resampling (after init).
// Guide table for the inverse-CDF search: guide[b] = first i with cum[i] >= b / GB (P if
// none), for b = 0 .. GB + 2.  The queries b / GB are sorted, so neighbouring threads walk
// nearly the same binary-search path (cache-friendly, unlike the random uniforms).
//
// A wave's 64 queries are consecutive, so their answers lie between those of its first and
// last query: lanes 0-31 and 32-63 find those two by 32-way searches (32 independent probes
// per step: four steps span 10^6 particles, against 20 dependent loads of a binary search),
// then each lane searches the usually short range between them -- in registers when it holds
// at most 64 particles (a collapsed cloud's range is often a single particle).  On a monotone
// CDF every form returns the binary search's answer.  The evaluated CDF can dip by a few ulps
// (see CdfView); across such a dip the forms may settle on different particles of the dip, each
// inside the band its uniform allows -- the guarantee is the band, not one index.
__global__ __launch_bounds__(kB) void k_guide(ResampleArgs a) {
  const long long f = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * kB + threadIdx.x;
  const long long nb = a.GB + 3;                       // queries b = 0 .. GB + 2
  const long long b0 = b - lane;                       // the wave's first query
  if (b0 >= nb) return;                                // (wave-uniform)
  const long long bl = b0 + 63 < nb - 1 ? b0 + 63 : nb - 1;   // its last query
  const CdfView cum = cdf_view(a, f);
  // two 32-way searches in lock step: half h finds the first index with cum >= t(h ? bl : b0)
  const int h = lane >> 5, k = lane & 31;
  const unsigned long long hm = h ? 0xffffffff00000000ull : 0x00000000ffffffffull;
  const double th = (double)(h ? bl : b0) / (double)a.GB;
  long long L = 0, H = a.P;
  while (__ballot(H - L > 32)) {
    const long long st = (H - L + 31) / 32;
    const bool live = H - L > 32;
    long long q = (L + (long long)(k + 1) * st < H ? L + (long long)(k + 1) * st : H) - 1;
    q = q > 0 ? q : 0;
    const long long c = __popcll(__ballot(live && cum[q] < th) & hm);
    if (live) {
      const long long nH = L + (c + 1) * st < H ? L + (c + 1) * st : H;
      L = L + c * st < H ? L + c * st : H;
      H = nH;
    }
  }
  {
    const long long q = L + k;
    L += __popcll(__ballot(q < H && cum[q] < th) & hm);
  }
  const long long A0 = __shfl(L, 0), A1 = __shfl(L, 32);
  const double t = (double)b / (double)a.GB;
  long long lo = A0;                                   // this lane's answer is in [A0, A1]
  if (A1 - A0 <= 64) {
    // the range's CDF values in registers, one per lane; per lane a binary search over them
    const double v = A0 + lane < A1 ? cum[A0 + lane] : 0.0;
    int l = 0, r = (int)(A1 - A0);
    while (__ballot(r > l)) {
      const int m = l + (r - l) / 2;
      const double vm = __shfl(v, m < 63 ? m : 63);
      if (r > l) {
        if (vm < t) l = m + 1; else r = m;
      }
    }
    lo = A0 + l;
  } else {
    lo = cdf_search(cum, t, A0, A1);
  }
  if (b < nb) a.guide[f * nb + b] = (int)lo;
}

// ---------------------------------------------------------------------------------
// Systematic resampling by scan (north_star's scan-based systematic resampler).  Slot s
// draws u_s = (s + u0) / P; the search form gives slot s the first i with cum_i >= u_s, so
// particle i owns slots [S_{i-1}, S_i) with S_i = #{s : u_s <= cum_i} (u_s is monotone in
// s).  S_i comes from the closed form floor(cum_i P - u0) + 1, corrected against the same
// fp64 expression for u_s the search compares, so the indices are exactly the search's.
// Each particle with offspring marks the start of its run; an inclusive max-scan over the
// slots then fills every run with its particle: O(P) work, no per-slot search, no load
// imbalance when one ancestor takes most slots.
__device__ __forceinline__ double sys_u(long long s, double u0, long long P) {
  return ((double)s + u0) / (double)P;                      // exactly k_resample's expression
}
__device__ __forceinline__ long long sys_count(double c, double u0, long long P) {
  long long k = (long long)floor(c * (double)P - u0) + 1;    // estimate of #{s : u_s <= c}
  k = k < 0 ? 0 : (k > P ? P : k);
  while (k > 0 && sys_u(k - 1, u0, P) > c) --k;
  while (k < P && sys_u(k, u0, P) <= c) ++k;
  return k;
}
__device__ __forceinline__ double sys_u0(const ResampleArgs& a, long long f) {
  if (a.U) return a.U[0];
  const uint4 r = philox4x32_10(make_uint4(0u, a.frame, kStreamSystematic, 0u), filter_key(a.seed_lo, a.seed_hi, f));
  return u01_co(r.x, r.y);
}

// marks[s] = i where particle i's offspring start (-1 elsewhere: memset before)
__global__ __launch_bounds__(kB) void k_sys_marks(ResampleArgs a) {
  const long long f = blockIdx.y;
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= a.P) return;
  const double u0 = sys_u0(a, f);
  const CdfView cum = cdf_view(a, f);
  const long long lo = i > 0 ? sys_count(cum[i - 1], u0, a.P) : 0;
  const long long hi = sys_count(cum[i], u0, a.P);
  if (hi > lo) a.sys_mark[f * a.P + lo] = (int)i;
}

// block-local inclusive max-scan of the marks (in place) and the block maxima
__global__ __launch_bounds__(kB) void k_sys_scan(ResampleArgs a) {
  __shared__ int wmax[kB / 64];
  const int tid = threadIdx.x;
  const long long f = blockIdx.y;
  const long long s = (long long)blockIdx.x * kB + tid;
  const int x = block_inclusive_scan(s < a.P ? a.sys_mark[f * a.P + s] : -1, -1, OpMax(), wmax, tid >> 6);
  if (s < a.P) a.sys_mark[f * a.P + s] = x;
  if (tid == kB - 1) a.sys_block[f * a.nb + blockIdx.x] = x;
}

// one workgroup per filter: exclusive max-scan of the block maxima (in place)
__global__ __launch_bounds__(1024) void k_sys_blocks(ResampleArgs a) {
  int* blk = a.sys_block + (long long)blockIdx.x * a.nb;
  chunked1024_exclusive_scan(blk, blk, 1, a.nb, -1, OpMax(),
                             [](int x, int* t) { return block1024_exclusive_scan_hs(x, -1, OpMax(), t); });
}

// The uniform of slot s of filter f; u_replay: the replay's uniform for the slot where a.U is
// set (U[0] for systematic resampling, else U[s]), loaded by the caller.
__device__ __forceinline__ double resample_uniform(const ResampleArgs& a, long long f, long long s, uint2 key,
                                                   double u_replay) {
  if (a.systematic) return sys_u(s, a.U ? u_replay : sys_u0(a, f), a.P);
  if (a.U) return u_replay;
  const uint4 r = philox4x32_10(make_uint4((unsigned)s, a.frame, kStreamResample, 0u), key);
  return u01_co(r.x, r.y);
}

// The read-out terms of slot s (pre-resample ll / e at slot s; M = max ll, S = sum e): e2 the
// unnormalised weight of the likelihood read-outs, wv the normalised weight of the state mean.
__device__ __forceinline__ void readout_terms(double llv, double M, double e, double S, double& e2, double& wv) {
  const double lw = llv - M;
  e2 = exp((llv + lw) - M);                  // ll + log_w - max(ll + log_w); that max is M
  wv = e / S;
}
// One block's sums of the nq = C + 1 + d read-out quantities of its slots (act: a live slot of
// post-resample class cnew and state xs): wave sums into red (the block's, LDS), then for thread
// t < nq of the block the four waves of quantity t in order (other threads: 0).  Contains a barrier.
__device__ __forceinline__ double readout_block_sum(bool act, int cnew, double e2, double wv, const double* xs, int C,
                                                    int nq, BlockGeo g, double (*red)[kMaxReadout]) {
  for (int k = 0; k < nq; ++k) {
    double v = 0.0;
    if (act) {
      if (k < C) v = (cnew == k) ? e2 : 0.0;
      else if (k == C) v = e2;
      else v = xs[k - C - 1] * wv;
    }
    v = wave_sum(v);
    if ((g.t & 63) == 0) red[g.wq][k] = v;
  }
  __syncthreads();
  double t = 0.0;
  if (g.t < nq)
    for (int v = 0; v < kB / 64; ++v) t += red[v][g.t];
  return t;
}

__global__ __launch_bounds__(kB) void k_resample(ResampleArgs a) {
  __shared__ double red[kB / 64][kMaxReadout];
  const int tid = threadIdx.x, lane = tid & 63;
  const long long f = blockIdx.y;
  const long long s = (long long)blockIdx.x * kB + tid;   // slot within filter f
  const long long g0 = f * a.P;                            // filter f's first particle
  const uint2 key = filter_key(a.seed_lo, a.seed_hi, f);
  const int C = a.C, d = a.d;
  const int nq = C + 1 + d;
  const bool act = s < a.P;
  long long idx = 0;                                       // source, within filter f
  int cnew = -1;
  const double* xs = nullptr;                              // the source particle's state
  double e2 = 0.0, wv = 0.0;
  if (act) {
    if (a.identity) {
      idx = s;
    } else if (a.sys_mark) {                                // systematic by scan
      idx = max(a.sys_mark[g0 + s], a.sys_block[f * a.nb + blockIdx.x]);
    } else {
      // (systematic: the search form; the filter resamples by scan)
      const double u = resample_uniform(a, f, s, key, a.U ? a.U[a.systematic ? 0 : s] : 0.0);
      // first index with cum >= u (torch's searchsorted), searched between two guide
      // entries that bracket it: t_lo = (q0 - 1) / GB <= u and t_hi = (q0 + 2) / GB > u for
      // q0 = floor(u GB) whatever its rounding, so the result is exactly that of a search
      // over [0, P]
      long long lo = 0, hi = a.P;
      if (a.GB > 0) {                           // guided (large P): bracket, then search
        const int* gd = a.guide + f * (a.GB + 3);
        const long long q0 = (long long)floor(u * (double)a.GB);
        lo = gd[q0 - 1 > 0 ? q0 - 1 : 0];
        hi = gd[q0 + 2 < a.GB + 2 ? q0 + 2 : a.GB + 2];
      }
      idx = cdf_search(cdf_view(a, f), u, lo, hi);
    }
    if (a.rows) {                 // the exchanged row of particle idx, read in place
      const double* row = a.rows + (a.rows_inv ? (long long)a.rows_inv[g0 + idx] : g0 + idx) * a.rows_w;
      cnew = (int)row[0];
      xs = row + 1;
    } else {
      cnew = a.cls_src[g0 + idx];
      xs = a.X_src + (g0 + idx) * d;
    }
    if (!a.identity) {
      a.ridx[g0 + s] = (int)idx;
      a.cls_dst[g0 + s] = cnew;
    }
    // read-outs: post-resample class/state at slot s, pre-resample ll/log_w at slot s
    readout_terms(a.ll[g0 + s], ord_dec(a.gmax[f]), a.e[g0 + s], a.total[f], e2, wv);
  }
  if (!a.identity) {
    // The wave's 64 new states are one contiguous run of X_dst: lane l stores its elements
    // l, l + 64, ... of that run (8-byte stores, each instruction one contiguous 512 bytes)
    // from the source rows it finds through the owning lanes' pointers -- rows this wave has
    // just read.  Per-lane stores of d doubles at stride 8 d bytes ran at ~1 TB/s.
    // (k_small_resample keeps the per-lane rows: at most 1024 of them, latency-bound.)
    const long long s0 = s - lane;                         // the wave's first slot
    const long long nv = a.P - s0 < 64 ? a.P - s0 : 64;   // its slots in range (wave-uniform)
    const long long n = nv * d;
    for (long long e = lane; e < 64LL * d; e += 64) {
      const int l2 = (int)(e / d), i2 = (int)(e - (long long)l2 * d);
      const double* src = (const double*)__shfl((long long)xs, l2);
      if (e < n) a.X_dst[(g0 + s0) * d + e] = src[i2];
    }
  }
  const double t = readout_block_sum(act, cnew, e2, wv, xs, C, nq, grid_block(), red);
  if (tid < nq) a.partials[(f * a.nb + blockIdx.x) * nq + tid] = t;
}

// The all-gathered {ll} column (rows in position order: row r holds particle own[r]) into
// particle order, with each kRowsLL-particle block's maximum as an ord_enc key: the
// normaliser's maximum (gpmdm_pf.py:200) without k_norm_max, as k_obs_ll gives it to a
// single rank.
constexpr int kRowsLLPer = 8;
constexpr long long kRowsLL = (long long)kRowsLLPer * kB;
__global__ __launch_bounds__(kB) void k_rows_ll(RowsLLArgs a) {
  unsigned long long key = 0;            // below ord_enc of any double
#pragma unroll
  for (int k = 0; k < kRowsLLPer; ++k) {
    const long long p = (long long)blockIdx.x * kRowsLL + (long long)k * kB + threadIdx.x;
    if (p < a.P) {
      const double v = a.rows[(a.inv ? (long long)a.inv[p] : p) * a.w];
      a.ll[p] = v;
      const unsigned long long kk = ord_enc(fmax(-INFINITY, v));   // k_norm_max's value set: NaN ignored
      key = kk > key ? kk : key;
    }
  }
  block_max_key_store<kB / 64>(key, a.bmax);
}

// The read-out is in mapped host memory: publish its sequence number after it, so the host
// that sees the number sees the values -- gpmdm_pf_read then waits on host memory, and no
// event record sits between the read-out and the next frame's switch.  The protocol
// (DESIGN.md §1 "Mapped-memory handshake"):
//  * every other thread that wrote host memory in this kernel issues a system-scope fence
//    before the workgroup barrier (its stores are performed at system scope first);
//  * thread 0, after the barrier, publishes the number with a system-scope RELEASE store
//    (publish_seq): it orders thread 0's own stores, and everything that happens-before it
//    -- the other threads' fenced stores through the barrier, and every earlier kernel of
//    the stream (k_dyn_finish's row count) -- before the number;
//  * the host polls with ACQUIRE loads (gpmdm_pf::min_mapped), so its later plain loads of
//    the guarded values cannot be hoisted above the number.
// `stored`: this thread wrote host memory in this kernel (only those need the system-scope
// fence, whose L2 write-back costs ~3 us a wave; thread 0's release store includes its own).
__device__ inline void publish_readout(const ResampleArgs& a, long long f, int tid, bool stored) {
  if (!a.seq_host) return;              // (uniform over the workgroup)
  if (stored && tid != 0) __threadfence_system();
  __syncthreads();
  if (tid == 0) publish_seq(a.seq_host + f, a.seq);
}

// One 1024-thread workgroup: filter f's read-out from its nb blocks' partial sums (row b at
// partials + b * ld: the buffer, or its LDS mirror), stored to readout and readout_host.
// Returns whether this thread stored a value.  Contains barriers.
__device__ __forceinline__ bool readout_values(const ResampleArgs& a, long long f, const double* partials, int ld,
                                               int nb) {
  __shared__ double red[8][16];
  __shared__ double tot[kMaxReadout];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nq = a.C + 1 + a.d;
  // eight read-out quantities per pass over the partials (every thread's loads in flight
  // together; per quantity the same thread-strided order as one quantity at a time)
  for (int k0 = 0; k0 < nq; k0 += 8) {
    double s[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) s[kk] = 0.0;
    for (long long b = tid; b < nb; b += 1024)
#pragma unroll
      for (int kk = 0; kk < 8; ++kk)
        if (k0 + kk < nq) s[kk] += partials[b * ld + k0 + kk];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const double v = wave_sum(s[kk]);
      if (lane == 0) red[kk][w] = v;
    }
    __syncthreads();
    if (tid < 8 && k0 + tid < nq) {
      double t = 0.0;
      for (int v = 0; v < 16; ++v) t += red[tid][v];
      tot[k0 + tid] = t;
    }
    __syncthreads();
  }
  // one value per lane, so every store is 8 bytes: a one-lane loop was vectorised into
  // 16-byte stores (the >8-byte store-data hazard; tests/test_isa_guard.py)
  const int nro = a.C + a.d + 1;
  if (tid < nro) {
    double v;
    if (tid < a.C) {                                     // class_probabilities
      double cl = 0.0;
      for (int c = 0; c < a.C; ++c) cl += tot[c];
      v = tot[tid] / cl;
    } else if (tid < a.C + a.d) {
      v = tot[tid + 1];                                  // current_state_mean
    } else {
      v = tot[a.C];                                      // log_likelihood()
    }
    a.readout[f * nro + tid] = v;
    if (a.readout_host) a.readout_host[f * nro + tid] = v;
  }
  return tid < nro;
}

__global__ __launch_bounds__(1024) void k_readout(ResampleArgs a) {
  const int tid = threadIdx.x;
  const long long f = blockIdx.x;
  const int nq = a.C + 1 + a.d;
  const bool ro = readout_values(a, f, a.partials + f * a.nb * nq, nq, a.nb);
  // the AUTO cutoff's counters of this frame, one per lane (8-byte stores: the ISA guard)
  const bool cst = a.cut_stats && f == 0 && tid < 2;
  if (cst) {
    a.cut_stats_host[tid] = a.cut_stats[tid];
    a.cut_stats[tid] = 0;
  }
  publish_readout(a, f, tid, ro || cst);
}


// ---------------------------------------------------------------------------------
// Small filters (P <= kSmallP per filter, no guide table): one 1024-thread workgroup per
// filter runs normalise + CDF + resample + read-out in one launch instead of six -- at the
// notebook's P = 100 each launch of the multi-kernel path costs more than its work.  The steps
// are the multi-kernel path's own device functions (obs_ll_step, block_inclusive_scan,
// cdf_value, resample_uniform, cdf_search, readout_terms, readout_block_sum, readout_values),
// called with the workgroup's quarters as the 256-thread blocks of k_norm_exp_scan /
// k_resample and cdf_view, and with LDS mirrors (M, block sums and offsets, S, the CDF, the
// read-out partials) where that path reads a buffer back; the buffers are still written for
// their other readers.  Its own: the maximum (exact in any order); k_norm_total's scan,
// emulated over four slots (below); the early load of the replay uniforms; per-lane X_dst rows
// (see k_resample).  Systematic resampling takes the search form, whose indices the scan form
// reproduces exactly (k_sys_marks).  Results are bitwise those of the multi-kernel path
// (tests/test_gpu_small_path.py).
constexpr long long kSmallP = 1024;

__global__ __launch_bounds__(1024) void k_small_resample(NormArgs na, ResampleArgs a) {
  __shared__ double mx[16];
  __shared__ double wsum[4][4];
  __shared__ double Msh, Ssh, bsum[4], boff[4];
  __shared__ double psh[4][kMaxReadout];              // partials
  __shared__ double cum_s[kSmallP];
  __shared__ double red[4][4][kMaxReadout];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const BlockGeo g = quarter_block();
  const long long f = blockIdx.x;
  const long long P = na.P;
  const int nb = na.nb;
  const long long p = tid;                            // = g.b * 256 + g.t
  const long long g0 = f * P;
  const bool act = p < P;
  // the replay uniforms (host-mapped for small filters: a PCIe round trip) are loaded
  // here, ahead of the phases before the search, so their latency overlaps them
  const double u_pre = (a.U && !a.identity && act) ? a.U[a.systematic ? 0 : p] : 0.0;
  // ---- k_obs_ll (deferred by the single-shard filter's weigh step): out index g0 + p ----
  const double llp = na.obs_pending ? obs_ll_step(na.obs, g0 + p, act) : (act ? na.ll[g0 + p] : 0.0);
  // ---- k_norm_max: the largest ll (NaN ignored, as fmax does) ----
  {
    double v = act ? llp : -INFINITY;
    v = fmax(-INFINITY, v);
    v = wave_max(v);
    if (lane == 0) mx[w] = v;
    __syncthreads();
    if (tid == 0) {
      double m = mx[0];
      for (int i = 1; i < 16; ++i) m = fmax(m, mx[i]);
      na.gmax[f] = ord_enc(m);
      Msh = ord_dec(ord_enc(m));
    }
    __syncthreads();
  }
  const double M = Msh;
  // ---- k_norm_exp_scan ----
  const double e = act ? exp(llp - M) : 0.0;
  if (act) na.e[g0 + p] = e;
  const double e_incl = block_inclusive_scan(e, 0.0, OpSum(), wsum[g.b], g.wq);
  if (act) na.local[g0 + p] = e_incl;
  if (g.t == kB - 1 && g.b < nb) {
    na.blocksum[f * nb + g.b] = e_incl;
    bsum[g.b] = e_incl;
  }
  __syncthreads();
  // ---- k_norm_total ----
  // k_norm_total's 1024-wide Hillis-Steele scan over the nb <= 4 block sums (zeros
  // beyond): every addition past the first four slots adds an exact +0, so its values are
  // those of the same scan over four slots, computed here by one thread with the same
  // operand order (part[i] = part[i] + part[i - off]).
  if (tid == 0) {
    double h[4];
    for (int i = 0; i < 4; ++i) h[i] = i < nb ? bsum[i] : 0.0;
    for (int off = 1; off < 4; off <<= 1)
      for (int i = 3; i >= off; --i) h[i] = h[i] + h[i - off];
    for (int bb = 0; bb < 4; ++bb) boff[bb] = bb ? h[bb - 1] : 0.0;
    Ssh = h[3];
  }
  __syncthreads();
  const double S = Ssh;
  if (tid < nb) na.blockoff[f * nb + tid] = boff[tid];      // one 8-byte store per lane
  if (tid == 0) na.total[f] = S;
  if (act) cum_s[p] = cdf_value(boff[g.b], e_incl, S, p == P - 1);
  __syncthreads();
  // ---- k_resample (slot s = p) ----
  const int C = a.C, d = a.d, nq = C + 1 + d;
  long long idx = 0;
  int cnew = -1;
  const double* xs = nullptr;
  double e2 = 0.0, wv = 0.0;
  if (act) {
    if (a.identity) {
      idx = p;
    } else {
      const double u = resample_uniform(a, f, p, filter_key(a.seed_lo, a.seed_hi, f), u_pre);
      idx = cdf_search(cum_s, u, 0, P);
    }
    cnew = a.cls_src[g0 + idx];
    xs = a.X_src + (g0 + idx) * d;
    if (!a.identity) {
      a.ridx[g0 + p] = (int)idx;
      a.cls_dst[g0 + p] = cnew;
      if (a.cls_host) a.cls_host[g0 + p] = cnew;
      for (int j = 0; j < d; ++j) a.X_dst[(g0 + p) * d + j] = xs[j];
    }
    readout_terms(llp, M, e, S, e2, wv);
  }
  const double t = readout_block_sum(act, cnew, e2, wv, xs, C, nq, g, red[g.b]);
  if (g.t < nq && g.b < nb) {
    a.partials[(f * nb + g.b) * nq + g.t] = t;
    psh[g.b][g.t] = t;
  }
  __syncthreads();
  // ---- k_readout ----
  readout_values(a, f, &psh[0][0], kMaxReadout, nb);
  publish_readout(a, f, tid, true);   // (cls_host: any slot's thread)
}

// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void k_pack(PackArgs a) {
  const long long r = (long long)blockIdx.x * kB + threadIdx.x;
  if (r >= a.n) return;
  const long long p = a.own ? a.own[a.lo + r] : a.lo + r;
  const int lo = a.part == GPMDM_PACK_STATES ? 1 : 0;            // first column present
  const int hi = a.part == GPMDM_PACK_LL ? 1 : a.d + 2;           // one past the last
  double* o = a.buf + r * (hi - lo);                              // o[k - lo]: column k
  if (lo == 0) o[0] = a.ll[p];
  if (hi > 1) {
    o[1 - lo] = (double)a.cls[p];
    for (int j = 0; j < a.d; ++j) o[2 - lo + j] = a.X[p * a.d + j];
  }
}

// one thread per particle p, reading its row inv[p] (a gather: the writes stay coalesced;
// scattering the rows to own[r] made every write a partial-line write, 57 us at P = 800k)
__global__ __launch_bounds__(kB) void k_unpack(PackArgs a) {
  const long long p = (long long)blockIdx.x * kB + threadIdx.x;
  if (p >= a.n) return;
  const long long r = a.inv ? a.inv[p] : p;
  const int lo = a.part == GPMDM_PACK_STATES ? 1 : 0;
  const int hi = a.part == GPMDM_PACK_LL ? 1 : a.d + 2;
  const double* i = a.buf + r * (hi - lo);
  if (lo == 0) a.ll[p] = i[0];
  if (hi > 1) {
    a.cls[p] = (int)i[1 - lo];
    for (int j = 0; j < a.d; ++j) a.X[p * a.d + j] = i[2 - lo + j];
  }
}

// ---------------------------------------------------------------------------------
// predict(): class histogram of the current classes (k_switch's histogram without a switch)
__global__ __launch_bounds__(kB) void k_class_hist(const int* cls, long long P, int C, int* blockcounts) {
  __shared__ int hist[kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < C) hist[tid] = 0;
  __syncthreads();
  const long long p = (long long)blockIdx.x * kB + tid;
  if (p < P) atomicAdd(&hist[cls[p]], 1);
  __syncthreads();
  if (tid < C) blockcounts[(long long)blockIdx.x * C + tid] = hist[tid];
}

__global__ __launch_bounds__(kB) void k_predict_scatter(const int* perm, const double* mu, double* mu_p,
                                                        long long P, int d) {
  const long long o = (long long)blockIdx.x * kB + threadIdx.x;
  if (o >= P) return;
  const long long p = perm[o];
  for (int j = 0; j < d; ++j) mu_p[p * d + j] = mu[o * d + j];
}

// One workgroup per filter: mean over the filter's particles, thread-strided partial sums
// combined in a fixed order.
__global__ __launch_bounds__(kB) void k_predict_mean(const double* mu_p, double* out, long long Pf, int d) {
  __shared__ double red[kB / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long f = blockIdx.x;
  for (int j = 0; j < d; ++j) {
    double s = 0.0;
    for (long long p = tid; p < Pf; p += kB) s += mu_p[(f * Pf + p) * d + j];
    s = wave_sum(s);
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int v = 0; v < kB / 64; ++v) t += red[v];
      out[f * d + j] = t / (double)Pf;
    }
    __syncthreads();
  }
}

// One-segment table of a predictive map, written in stream order (no host-to-device copy
// of a host array per call): {pos_begin, pos_end, out_base, tile_start[0], tile_start[1]}.
__global__ void k_seg_table(int* t, int n, int tiles) {
  const int i = threadIdx.x;
  if (i < 5) t[i] = i == 1 ? n : (i == 4 ? tiles : 0);
}

// ---------------------------------------------------------------------------------
static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

// GPMDM_NO_SMALL_PATH=1 forces the multi-kernel path (the reference of tests/test_gpu_small_path.py)
static bool small_path_enabled() {
  static const bool on = std::getenv("GPMDM_NO_SMALL_PATH") == nullptr;
  return on;
}

void launch_seg_table(int* t, int n, int tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_seg_table, dim3(1), dim3(64), 0, s, t, n, tiles);
}

void launch_class_hist(const int* cls, long long P, int C, int* blockcounts, hipStream_t s) {
  hipLaunchKernelGGL(k_class_hist, dim3(nblk(P, kB)), dim3(kB), 0, s, cls, P, C, blockcounts);
}
void launch_predict_mean(const int* perm, const double* mu, double* mu_p, double* out, long long P,
                         long long Pf, int F, int d, hipStream_t s) {
  hipLaunchKernelGGL(k_predict_scatter, dim3(nblk(P, kB)), dim3(kB), 0, s, perm, mu, mu_p, P, d);
  hipLaunchKernelGGL(k_predict_mean, dim3((unsigned)F), dim3(kB), 0, s, mu_p, out, Pf, d);
}

static void launch_switch(const SwitchArgs& a, hipStream_t s) {
  if (a.own)
    hipLaunchKernelGGL(k_switch<true>, dim3(nblk(a.n > 0 ? a.n : 1, kB)), dim3(kB), 0, s, a);
  else
    hipLaunchKernelGGL(k_switch<false>, dim3(nblk(a.n > 0 ? a.n : 1, kB)), dim3(kB), 0, s, a);
}
void launch_scan_counts(const ScanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, a);
}
void launch_group(const GroupArgs& a, hipStream_t s) {
  if (a.own)
    hipLaunchKernelGGL(k_group<true>, dim3(nblk(a.n > 0 ? a.n : 1, kB)), dim3(kB), 0, s, a);
  else
    hipLaunchKernelGGL(k_group<false>, dim3(nblk(a.n > 0 ? a.n : 1, kB)), dim3(kB), 0, s, a);
}
static void launch_lead(const LeadArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_lead_flags, dim3((unsigned)a.nb), dim3(kB), 0, s, a);
  if (a.nb <= kMaxLeadBlocks) {
    hipLaunchKernelGGL(k_lead_tables_compact, dim3((unsigned)a.nb), dim3(kB), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_lead_tables, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_lead_compact, dim3((unsigned)a.nb), dim3(kB), 0, s, a);
  }
}
// switch + class scan + grouping (+ leader compaction with `la`): one launch for a small
// single-shard filter (k_small_switch, the same tables), the multi-kernel path otherwise.
// The owner preset of the leader election is part of either path.
bool launch_switch_group(const SwitchArgs& sa, const ScanArgs& sc, const GroupArgs& ga, const LeadArgs* la,
                         bool owner_preset, hipStream_t s) {
  if (small_path_enabled() && sa.P <= kSmallSwitchP && sa.n == sa.P && sa.base == 0 && !sa.own && sa.n > 0 &&
      (la == nullptr) == (sa.owner == nullptr) && (la == nullptr || la->npos == sa.P)) {
    LeadArgs l = la ? *la : LeadArgs{};
    l.owner_reset = nullptr;             // the kernel presets the whole table itself
    hipLaunchKernelGGL(k_small_switch, dim3(1), dim3(1024), 0, s, sa, sc, ga, l, la ? 1 : 0);
    return true;
  }
  if (la && owner_preset) (void)hipMemsetAsync(sa.owner, 0xff, sizeof(unsigned) * (size_t)sa.C * sa.P, s);
  launch_switch(sa, s);
  launch_scan_counts(sc, s);
  launch_group(ga, s);
  if (la) launch_lead(*la, s);
  return false;
}
void launch_dyn_finish(const DynFinishArgs& a, hipStream_t s) {
  if (a.n_out > 0) hipLaunchKernelGGL(k_dyn_finish, dim3(nblk(a.n_out, kB)), dim3(kB), 0, s, a);
}
void launch_obs_finish(const ObsFinishArgs& a, hipStream_t s) {
  if (a.n_out <= 0) return;
  if (a.spart)
    hipLaunchKernelGGL(k_obs_ll, dim3(nblk(a.n_out, kB)), dim3(kB), 0, s, a);
  else
    hipLaunchKernelGGL(k_obs_finish, dim3(nblk(a.n_out, kB / 64)), dim3(kB), 0, s, a);
}
static void launch_normalise(const NormArgs& a, hipStream_t s) {
  const dim3 g(nblk(a.P, kB), (unsigned)a.F);
  const unsigned nbm = nblk(a.P, kB) < kMaxNormBlocks ? nblk(a.P, kB) : kMaxNormBlocks;
  if (!a.bmax) hipLaunchKernelGGL(k_norm_max, dim3(nbm, (unsigned)a.F), dim3(kB), 0, s, a);
  hipLaunchKernelGGL(k_norm_exp_scan, g, dim3(kB), 0, s, a);
  hipLaunchKernelGGL(k_norm_total, dim3((unsigned)a.F), dim3(1024), 0, s, a);
}
void launch_resample(const ResampleArgs& a, hipStream_t s) {
  if (!a.identity && a.sys_mark) {
    (void)hipMemsetAsync(a.sys_mark, 0xff, sizeof(int) * (size_t)a.P * a.F, s);   // -1: no run starts
    hipLaunchKernelGGL(k_sys_marks, dim3(nblk(a.P, kB), (unsigned)a.F), dim3(kB), 0, s, a);
    hipLaunchKernelGGL(k_sys_scan, dim3(nblk(a.P, kB), (unsigned)a.F), dim3(kB), 0, s, a);
    hipLaunchKernelGGL(k_sys_blocks, dim3((unsigned)a.F), dim3(1024), 0, s, a);
  } else if (!a.identity && a.GB > 0)
    hipLaunchKernelGGL(k_guide, dim3(nblk(a.GB + 3, kB), (unsigned)a.F), dim3(kB), 0, s, a);
  hipLaunchKernelGGL(k_resample, dim3(nblk(a.P, kB), (unsigned)a.F), dim3(kB), 0, s, a);
  hipLaunchKernelGGL(k_readout, dim3((unsigned)a.F), dim3(1024), 0, s, a);
}
// normalise + resample + read-out: one launch for small filters (k_small_resample, bitwise
// the multi-kernel path), the multi-kernel path otherwise
bool small_resample_ok(const NormArgs& na, const ResampleArgs& ra) {
  return small_path_enabled() && na.P <= kSmallP && ra.GB == 0;
}

void launch_normalise_resample(const NormArgs& na, const ResampleArgs& ra, hipStream_t s) {
  if (small_resample_ok(na, ra)) {
    hipLaunchKernelGGL(k_small_resample, dim3((unsigned)na.F), dim3(1024), 0, s, na, ra);
    return;
  }
  if (na.obs_pending) launch_obs_finish(na.obs, s);
  launch_normalise(na, s);
  launch_resample(ra, s);
}
int rows_ll_blocks(long long P) { return (int)nblk(P, kRowsLL); }
void launch_rows_ll(const RowsLLArgs& a, hipStream_t s) {
  if (a.P > 0) hipLaunchKernelGGL(k_rows_ll, dim3(nblk(a.P, kRowsLL)), dim3(kB), 0, s, a);
}
void launch_pack(const PackArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_pack, dim3(nblk(a.n, kB)), dim3(kB), 0, s, a);
}
void launch_unpack(const PackArgs& a, hipStream_t s) {
  if (a.n > 0) hipLaunchKernelGGL(k_unpack, dim3(nblk(a.n, kB)), dim3(kB), 0, s, a);
}

}  // namespace gpmdm
