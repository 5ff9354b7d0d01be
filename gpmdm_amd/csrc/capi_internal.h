// Internal interface of the C-ABI translation units (capi_*.hip): the model and filter
// handles (device layout, per-frame bookkeeping) and the helpers the units share.  Not part of
// the public ABI (include/gpmdm_hip.h).
// Ownership: both handles hold their device buffers, pinned buffers and events in status.h's
// owning types (DevBuf, PinBuf, Event), released by the members' destructors; the handles'
// own destructors keep only what has an order (side streams drained first).  The read-outs
// whose results land in a pinned buffer are status.h Landing objects, which also carry the
// pending event the lifecycle waits (quiesce) go through.  What several units fill the same
// way has one builder here: the class-table layout (ClassTables / SegTables), fill_grouping,
// launch_dyn_tiles, pose_readout, ll_const, host_ord_enc / host_ord_dec.
//   capi_model.hip     models, predictive maps (gpmdm_model_*, gpmdm_predict_*), images
//   capi_pf.hip        filter and bank lifecycle, state import / export, settings, predict,
//                      the pose read-out (gpmdm_pf_observation) and the grouping arguments
//   capi_frame.hip     the per-frame launch sequence: switch, propagate, weigh, resample, read;
//                      the dynamics tile launches
//   capi_exchange.hip  the multi-rank exchange (pack / unpack, RCCL communicator, gathers)
//   capi_replay.hip    replay-draw staging (pinned buffers, staged normals, pre-switch)
//   capi_forecast.hip  the multi-step forecast roll-out (gpmdm_pf_forecast, gpmdm_bank_forecast)
//   capi_smooth.hip    fixed-lag smoothing: the ancestry ring and its read-out (gpmdm_pf_smoothed,
//                      gpmdm_bank_smoothed)
//   capi_backsmooth.hip  marginal backward smoothing over that ring (gpmdm_backward_step,
//                      gpmdm_pf_smoothed_marginal)
//   capi_backsample.hip  backward simulation over that ring (gpmdm_backward_sample_step,
//                      gpmdm_pf_sample_trajectories)
//   capi_innov.hip     per-joint innovations and the GP's predictive variance (gpmdm_pf_set_predictive,
//                      gpmdm_pf_innovation, gpmdm_pf_observation_gp and the banks')
//   capi_gate.hip      outlier gating inside the frame (gpmdm_pf_set_gate, gpmdm_pf_gate_report)
#pragma once
#include <algorithm>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <functional>
#include <mutex>
#include <type_traits>

#include <rccl/rccl.h>   // types only: the entry points are resolved at run time (rccl())

#include "../../include/gpmdm_hip.h"
#include "common.h"
#include "host_image.h"
#include "obs_readout.h"
#include "pf_kernels.h"
#include "status.h"

static_assert(gpmdm::kMaxClassesDesc == gpmdm::kMaxClasses, "descriptor check and kernels agree on the class limit");

namespace gpmdm::capi {

// Rows from which a dynamics-GP predictive map uses the wide tile image (a throughput
// problem; below, the narrow tiles' shorter K loops win)
constexpr long long kWideRows = 4096;

// Single replay filters up to this size count their switched classes on the host
// (gpmdm_pf::cls_pin; the one-workgroup resampling kernel k_small_resample provides the
// classes).  The host loop is P x C fp64 divisions: ~1 us at the notebook's P = 100.
constexpr long long kHostCountsMaxP = 1024;

// The class-table layout (one definition: the step's tables small + 0, predict()'s
// small + kPredictTables, the forecast's fc_tab; the leaders' ltab holds the segment part
// only): arrays of kTabStride ints -- class_start, counts, then the four segment arrays the
// dynamics tiles read.
constexpr int kTabStride = 40;
struct SegTables {
  int* t;
  int* begin() const { return t; }
  int* end() const { return t + kTabStride; }
  int* out() const { return t + 2 * kTabStride; }
  int* tiles() const { return t + 3 * kTabStride; }
};
struct ClassTables {
  int* t;
  int* class_start() const { return t; }
  int* counts() const { return t + kTabStride; }
  SegTables seg() const { return SegTables{t + 2 * kTabStride}; }
};

// The host's side of common.h's order-preserving uint64 image of a double (ord_enc / ord_dec
// there are device functions)
inline unsigned long long host_ord_enc(double x) {
  unsigned long long u;
  std::memcpy(&u, &x, sizeof(u));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double host_ord_dec(unsigned long long u) {
  const unsigned long long v = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
  double x;
  std::memcpy(&x, &v, sizeof(x));
  return x;
}

// The likelihood's constant 0.5 n log(2 pi) of n observed dimensions, rounded as the reference
// rounds it (fp32 factors); the finish takes it as an argument
inline double ll_const(int n_observed) { return (double)((float)(0.5 * n_observed) * (float)1.8378770351409912); }

// One GP's device image: scaled inputs (+ squared norms) and B = [R | M] (+ H for the
// dynamics GPs) in MFMA-fragment order -- layout and packing in host_image.h.
struct GpImage {
  int n_rows = 0, n_m = 0, n_j = 0, coff = 0;
  bool dyn = false;       // a dynamics GP's image (linear-kernel rows H)
  TileGeo geo = kGeo64x256;
  DevBuf<double> Xrec;    // row_cap(n_rows) x (d + 1) row records (host_image.h)
  DevBuf<double> Hf;      // dynamics only
  DevBuf<double> Bf;

  SegDesc seg() const {
    SegDesc s{};
    s.Xrec = Xrec;
    s.Hf = Hf;
    s.Bf = Bf;
    s.n_rows = n_rows;
    s.n_m = n_m;
    s.n_j = n_j;
    s.coff = coff;
    return s;
  }
  // Read-out partials (gp_tile.h epilogue): one per column block, or for the dynamics GP's
  // wide shape (4 waves x 8 column tiles: 32 x 512) one per 256-column part, indexed as the
  // 16 x 256 image's blocks (front padding col_offset(n_cols, 256)) -- so the narrow and wide
  // dynamics images' partials are the same numbers in the same slots.
  bool split() const { return dyn && geo.nw == 4 && geo.ntw == 8; }
  int pnb() const { return split() ? geo.nb() / 2 : geo.nb(); }
  int pcoff() const { return split() ? col_offset(n_rows + n_m, pnb()) : coff; }
  int n_parts() const { return (int)cdiv(n_rows + pcoff(), pnb()); }              // parts holding R columns
  int n_pblocks() const { return (int)cdiv(n_rows + n_m + pcoff(), pnb()); }      // all parts
  int jm0() const { return (n_rows + pcoff()) / pnb(); }                          // first part with mean columns
  int tiles(long long n) const { return (int)cdiv(n, geo.pt()); }
};

int build_image(GpImage& g, int n_rows, int d, int n_m, const double* X, const double* ls,
                const double* lin_c2, const double* R, const double* M, TileGeo geo);

// One backward step's device scratch (capi_backsmooth.hip bs_step): the sources' records, one
// class's dynamics moments and tile partials, the targets' grouping, the ranges' partial sums,
// the targets' exponents, and the multiplicity histogram of a slot
struct BsScratch {
  DevBuf<double> rec, mu, var, q, part, lw;
  DevBuf<int> perm, tab, hist, mult;
};

// One MAP step's device scratch (capi_mappath.hip mp_step): the sources' records, one class's
// dynamics moments and tile partials, the targets' grouping and the ranges' maxima with their
// source rows; and a decoded window's: the two slots' leaders (rows, lead; owner and rank while
// they are elected), the compacted sources and targets, the scores by compact row (two halves),
// the back-pointers by compact row, the compact sizes, and the scores and back-pointers of every
// lag by particle
struct MpScratch {
  DevBuf<double> rec, mu, var, q, val;
  DevBuf<int> idx, perm, tab;
  DevBuf<double> Xs, Xt, llt, dc[2], delta;
  DevBuf<int> owner, rank, rows[2], lead[2], cs, ct, psi_c, psi, count;
};

// One backward-simulation step's device scratch (capi_backsample.hip fs_moments / fs_targets): the
// sources' records, one class's dynamics moments and tile partials, a chunk of targets' grouping,
// the ranges' partial sums and what k_fs_pick leaves per target; and a sampled window's: the
// uniforms, the result rows {index, class, state} of every lag, the distinct count's marks, and
// for the pose of a lag with dead trajectories the alive rows' flags, grouping and states
struct FsScratch {
  DevBuf<double> rec, mu, var, q, part, res, scale;
  DevBuf<int> perm, tab, range;
  DevBuf<double> u, X, ro_part, ro_X;
  DevBuf<int> idx, cls, mark, ro_flag, ro_perm, ro_tab;
};

}  // namespace gpmdm::capi

using namespace gpmdm;
using namespace gpmdm::capi;

// =====================================================================================
struct gpmdm_model {
  // Reference count: the caller's handle plus one per filter built on the model, so a
  // filter keeps the device image it was built on alive until it is destroyed or rebound
  // (gpmdm_pf_set_model) even after the caller rebuilt the model (GPMDM.set_latents).
  std::atomic<int> refs{1};
  int device = 0;
  long long N = 0;
  int D = 0, d = 0, C = 0;
  std::vector<double> X;              // host copy, N x d
  std::vector<double> y_ls, x_ls, x_lin_c2, x_il2, y_il2;
  GpImage obs;
  // the observation GP in 16 x 256 tiles for small models and filters (obs_pick): at the
  // notebook's N = 500 and P = 100 the 512-column blocks leave a 32-K-step chain of wide
  // MFMA steps on a handful of CUs; 256-column blocks halve each chain (empty: not built)
  GpImage obs_small;
  std::vector<GpImage> dyn;           // narrow tiles (16x256): de-duplicated rows, small maps
  std::vector<GpImage> dynw;          // wide tiles (the observation GP's shape): every particle
                                      // (dedup off, predict), large maps; empty = same as dyn
  const std::vector<GpImage>& dyn_set(bool wide) const { return wide && !dynw.empty() ? dynw : dyn; }
  int dyn_parts_max() const {
    int mx = 0;
    for (auto& g : dyn) mx = std::max(mx, g.n_parts());
    for (auto& g : dynw) mx = std::max(mx, g.n_parts());
    return mx;
  }
  DevBuf<double> y_il2_dev;
  DevBuf<double> y_lam2_dev;      // 1 / il2 = exp(y_log_lambdas)^2
  double sum_log_il2 = 0.0;
  // the filtered-pose read-out (obs_readout.h): beta = K_y^-1 Y in its own fragment order,
  // and the observation kernel's lengthscales on the device
  DevBuf<double> ro_beta, y_ls_dev;
  // Observation-GP cutoff image (gpmdm_model_set_obs_cutoff; empty: not set): K^-1's block
  // upper triangle and M over the training rows in a spatial order, tile-major
  // (host_image.h CutoffPacker, obs_cutoff.h), the K-step spheres, and the cutoff (tau; cut2 =
  // the squared scaled distance past which a value is below tau, with a margin; t_cut = ln tau
  // in the generation's exponent units)
  struct CutImage {
    int n_rows = 0, n_m = 0, T_R = 0, T_M = 0;
    DevBuf<double> Xrec, Bt, sph;
    DevBuf<long long> toff;
  } obs_cut;
  bool has_cutoff() const { return obs_cut.Bt != nullptr; }
  double cut_tau = 0.0, cut2 = 0.0, t_cut = 0.0;
  void release_cutoff() { obs_cut = CutImage{}; }
  // The dense filter's flush (gpmdm_model_set_obs_flush): tau from the column sums of K_y^-1 Y
  // kept at creation, and t_flush = ln tau in the generation's exponent units (as t_cut; negative);
  // 0: nothing is flushed
  std::vector<double> obs_m1;
  double flush_tau = 0.0, t_flush = 0.0;

  // Lifecycle (DESIGN.md §1 "Lifecycle waits"): the filters built on the model --
  // gpmdm_model_set_obs_cutoff waits for each one's own last frame (quiesce) before it
  // replaces the cutoff image -- and one event per stream the predictive maps ran on, so the
  // images' release at the last reference is ordered after those launches on the lifecycle
  // stream (no device-wide wait either way).
  std::mutex life_mu;
  std::vector<gpmdm_pf*> users;
  std::vector<std::pair<hipStream_t, hipEvent_t>> uses;
  void add_user(gpmdm_pf* pf) {
    std::lock_guard<std::mutex> lk(life_mu);
    users.push_back(pf);
  }
  void remove_user(gpmdm_pf* pf) {
    std::lock_guard<std::mutex> lk(life_mu);
    users.erase(std::remove(users.begin(), users.end(), pf), users.end());
  }
  hipError_t note_use(hipStream_t s) {   // after a predictive map's launches on s
    std::lock_guard<std::mutex> lk(life_mu);
    for (auto& u : uses)
      if (u.first == s) return hipEventRecord(u.second, s);
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    uses.emplace_back(s, ev);
    return hipEventRecord(ev, s);
  }

  ~gpmdm_model() {
    (void)hipSetDevice(device);
    if (hipStream_t life = life_stream(device)) {
      for (auto& u : uses) (void)hipStreamWaitEvent(life, u.second, 0);
    }
    for (auto& u : uses) (void)hipEventDestroy(u.second);
    // (the images and tables are released by their members' destructors, after these waits)
  }
};

inline void model_release(gpmdm_model* m) {
  if (m && m->refs.fetch_sub(1) == 1) delete m;
}

// The observation launch's image and shape for filters of P particles each (all ranks;
// a bank: per filter) whose shard holds n rows.
// * Small models (N <= kSmallObsN, d <= 12) and filters (P <= kSmallObsP): the 16 x 256
//   image (model.obs_small).  Its column blocks differ from the default image's, so the
//   per-block partial sums combine in another order: results agree to rounding, not bit
//   for bit, and the choice depends on the per-filter P only (every rank of a sharded
//   filter, and a bank and its filters run alone, make the same one).  (Splitting the
//   default image's partials as the dynamics images do would make them bitwise, at 0.5% of
//   the d = 3 observation launch: gp_tile.h.)
//   GPMDM_OBS_IMAGE16=0 does not build the image.
// * Otherwise, with fewer 32-row tiles than one per CU per column block, 16-row tiles over
//   the same 32 x 512 image (the image's fragment layout depends on the waves and column
//   tiles only): each workgroup's MFMA chain halves and twice the CUs work; every output is
//   accumulated and reduced in the same order whatever the tile height, so results are
//   bitwise those of the default shape (tests/test_gpu_small_path.py).
//   GPMDM_OBS_SMALL_TILES=0 / 1 forces these 16-row tiles off / on (A/B).
constexpr long long kSmallObsN = 1024, kSmallObsP = 1024;

inline int obs_parts_max(const gpmdm_model* m) {
  return std::max(m->obs.n_parts(), m->obs_small.Bf ? m->obs_small.n_parts() : 0);
}
inline int obs_blocks_max(const gpmdm_model* m) {
  return std::max(m->obs.n_pblocks(), m->obs_small.Bf ? m->obs_small.n_pblocks() : 0);
}

struct gpmdm_pf {
  gpmdm_model* m = nullptr;
  // P = all particles = F filters x Pf (a single filter: F = 1, Pf = P)
  long long P = 0, Pf = 0, lo = 0, hi = 0, nloc = 0;
  int F = 1;
  int n_ranks = 1, rank = 0, rng_mode = 0, resample_mode = 0, nb = 0, nbf = 0;
  unsigned seed_lo = 0, seed_hi = 0, frame = 0;
  bool initialised = false, switched = false, propagated = false;
  bool dyn_done = false;             // gpmdm_pf_propagate_dynamics ran, gpmdm_pf_weigh not yet
  // replay filters whose caller draws the normals after the switch's class counts: the
  // switch launches the dynamics-GP tiles (they need no normals) before it waits for the
  // counts, so they run while the host draws; propagate then launches the finish only
  bool gemm_ahead = false;
  Event cnt_done;                     // after the switch's class counts (replay, large filters)
  bool dedup = true;                  // ancestor de-duplication of the dynamics GP
  int dyn_tiles = GPMDM_DYN_TILES_AUTO;   // gpmdm_pf_set_dyn_tiles
  bool wide_dyn() const { return dyn_tiles == GPMDM_DYN_TILES_WIDE || (dyn_tiles == GPMDM_DYN_TILES_AUTO && !dedup); }
  bool dyn_wide_frame = false;        // this frame's dynamics image (set by the switch: dyn_frame_wide)
  // device state
  DevBuf<double> T, X, X_prop, ll;
  DevBuf<int> cls, cls_new, perm, ridx;
  DevBuf<int> blockcounts, blockoff, small;   // small: class tables
  DevBuf<int> obs_tab;               // [0, 5): the observation launch's segment table; [8, 13): the cutoff image's
  // the observation GP's kernel-value cutoff (gpmdm_pf_set_obs_cutoff): on, and the skip
  // statistics of the cutoff kernel (device: MFMA groups run, the dense kernel's count)
  bool obs_cutoff = false;
  // the dense tile branches around all-zero 16 x 4 blocks of kernel values (gpmdm_pf_set_obs_skip;
  // off: the same kernel runs every block)
  bool obs_skip = true;
  DevBuf<unsigned long long> sp_stats;
  bool sp_stats_on = false;
  // AUTO (gpmdm_pf_set_obs_cutoff mode 3; single-rank filters and banks with mapped
  // read-outs): the cutoff kernel while the reach it measured is low, the dense kernel
  // otherwise -- decided per frame from the last cutoff frame's MFMA-group fraction, with a
  // cutoff frame (a probe) at least every kCutAutoProbe frames.  The counters travel with the
  // read-out (k_readout -> cut_auto_host), so the decision is a function of the filter's own
  // trajectory: deterministic, but not rank-count invariant (multi-rank filters run mode 1).
  static constexpr int kCutAutoProbe = 8;
  static constexpr double kCutAutoMaxRun = 0.75;   // break-even: cutoff 0.65 vs dense 0.865 of peak
  bool cut_auto = false;
  DevBuf<unsigned long long> cut_auto_dev;         // device counters {run, dense}
  PinBuf<unsigned long long> cut_auto_host;        // mapped: the last cutoff frame's counters
  bool cut_auto_pending = false;                   // a cutoff frame's counters are on their way
  long long cut_auto_seq = 0;                      // ... published with this read-out number
  double cut_auto_frac = -1.0;                     // the last measured fraction (< 0: none)
  long long cut_auto_probe = -(1LL << 40);         // the frame of the last cutoff frame
  bool cut_frame = false;                          // this frame's observation GP is the cutoff's
  bool cut_frame_auto = false;                     // ... an AUTO filter's (its counters go with the read-out)
  // the counters run on every cutoff frame of a one-rank filter with mapped read-outs (modes 1
  // and 3): AUTO's choice of kernel, and the split policy's choice of the chunk grid
  bool cut_measure_active() const {
    return obs_cutoff && !sp_stats_on && n_ranks == 1 && seq_pin != nullptr && cut_auto_dev != nullptr;
  }
  bool cut_auto_active() const { return cut_auto && cut_measure_active(); }
  // the last cutoff frame's counters, published with its read-out (as the next frame reads them)
  hipError_t cut_auto_collect() {
    if (!cut_auto_pending) return hipSuccess;
    const hipError_t e = wait_readout(cut_auto_seq);
    if (e != hipSuccess) return e;
    const unsigned long long run = __atomic_load_n(cut_auto_host + 0, __ATOMIC_ACQUIRE);
    const unsigned long long dense = __atomic_load_n(cut_auto_host + 1, __ATOMIC_ACQUIRE);
    cut_auto_frac = dense ? (double)run / (double)dense : 0.0;
    cut_auto_pending = false;
    return hipSuccess;
  }
  static constexpr double kCutChunksMin = 0.5;     // GPMDM_CUT_SPLIT_AUTO: the chunk grid from this reach
  // the cutoff kernel's split tiles (capi_frame.hip): second parts' partials, (n_act, c*) per
  // split tile; grown on demand
  int cut_split_policy = GPMDM_CUT_SPLIT_AUTO;
  DevBuf<double> cut_part;
  DevBuf<int2> cut_split;
  // (grown inside a frame: the old buffers are released after the frame stream's earlier work)
  int ensure_cut_split(size_t n_part, int n_split, hipStream_t s) {
    if (cut_part.grow(n_part, s)) return fail(GPMDM_E_NOMEM, "cutoff split partials");
    if (cut_split.grow((size_t)n_split, s)) return fail(GPMDM_E_NOMEM, "cutoff split table");
    return GPMDM_OK;
  }
  // Masked observations (gpmdm_pf_set_obs_mask; obs_mask empty: every dimension observed).
  // The observation kernels reduce S = sum_j (z_j - mu_j)^2 lam2_j against a lam2 pointer and
  // the finish takes D, sum_j log il2_j and the constant as arguments, so a masked frame is
  // the same launches with lam2_obs (lam2_j where observed, exactly 0 elsewhere) and the three
  // scalars of the observed dimensions -- the likelihood of the model restricted to them.
  // z is zeroed at the unobserved positions in the staging copies (stage_z), so a NaN there
  // never reaches a kernel.
  // A bank (gpmdm_bank_set_obs_masks) holds one mask per filter: obs_mask and lam2_obs are
  // F x D, filter-major, the tiles read the row of each particle's filter, and the finish takes
  // the three scalars from an F-row table {D_obs, sum_log_il2_obs, ll_const_obs} that follows
  // lam2_obs in the same allocation (obs_ftab; one upload installs both).  D_obs is then the
  // sum over the filters (0: every filter blacked out) and the two scalars are unused.
  std::vector<unsigned char> obs_mask;
  DevBuf<double> lam2_obs;
  int D_obs = 0;
  double sum_log_il2_obs = 0.0, ll_const_obs = 0.0;
  bool masked() const { return !obs_mask.empty(); }
  const double* obs_ftab() const { return lam2_obs + (size_t)F * m->D; }
  void stage_z(double* dst, const double* zh) const {
    const size_t n = (size_t)m->D * F;
    if (!masked()) {
      std::memcpy(dst, zh, sizeof(double) * n);
      return;
    }
    for (size_t j = 0; j < n; ++j) dst[j] = obs_mask[j] ? zh[j] : 0.0;
  }
  // The filtered-pose read-out (gpmdm_pf_observation, obs_readout.h): the tiles' partials,
  // the device result {mean, spread} and its pinned landing buffer, allocated on first use;
  // ro_obs.ev follows the last read-out's launches (quiesce waits for it).
  DevBuf<double> ro_part;
  Landing ro_obs;
  // The forecast roll-out (gpmdm_pf_forecast / gpmdm_bank_forecast, forecast.h;
  // capi_forecast.hip): scratch of its own, allocated on first use -- the two halves of the
  // ping-pong cloud, the grouping's tables (the layout of `small`'s, base 0), block counts /
  // offsets and permutation, the dynamics tiles' outputs, the per-filter blocks' state sums
  // (F x ceil(Pf / 256) x d) and class counts (x C: gpmdm_bank_forecast's, on its first call),
  // the pose read-out's partials, and the H x F x (C + d + 2 D) result rows with their pinned
  // landing buffer (grown on demand).  None
  // of it is shared with the step, the pre-switch, predict() or the read-out, so a forecast
  // leaves a pending pre-switch pending.  fc_out.ev follows a forecast's launches (quiesce waits
  // for it while pending: the call itself synchronises, so only after a failed one).
  DevBuf<double> fc_X[2];
  DevBuf<int> fc_cls[2];
  DevBuf<int> fc_perm, fc_blockcounts, fc_blockoff, fc_tab, fc_bcounts;
  DevBuf<double> fc_q, fc_mu, fc_part, fc_ro_part;
  Landing fc_out;
  // Fixed-lag smoothing (gpmdm_pf_set_smoothing / gpmdm_pf_smoothed and the banks', smooth.h;
  // capi_smooth.hip).  sm_L > 0: every resample records {ridx, cls, X} into slot
  // frame mod (sm_L + 1) of the ring (sm_anc / sm_cls / sm_X, sm_L + 1 frames each); sm_depth =
  // min(sm_L, frames recorded since the ring was last cleared), the root of a cleared ring
  // being the cloud the filter held then (sm_clear records it).  The record launch follows the
  // frame's read-out number, which quiesce takes for the frame's last work: sm_ev is recorded
  // behind every record launch (smoothing on only) and quiesce waits for it while sm_pending.
  // The read-out's scratch -- marks with the class counts at their head, block sums, result rows with their pinned
  // landing buffer, the pose read-out's partials -- is its own, allocated on first use and grown
  // on demand; sm_out.ev follows a read-out's launches (waited for while pending: the call
  // itself synchronises, so only after a failed one).
  int sm_L = 0, sm_depth = 0;
  DevBuf<int> sm_anc, sm_cls;
  DevBuf<double> sm_X;
  Event sm_ev;
  hipStream_t sm_stream = nullptr;    // the stream of the last record launch
  bool sm_pending = false;
  DevBuf<double> sm_part, sm_ro_part;
  Landing sm_out;
  DevBuf<unsigned char> sm_marks;
  int sm_slot() const { return (int)(frame % (unsigned)(sm_L + 1)); }   // the latest frame's
  // Marginal backward smoothing over the same ring (gpmdm_pf_smoothed_marginal, backsmooth.h;
  // capi_backsmooth.hip): scratch of its own, grown on demand, and the result rows with their
  // pinned landing buffer (sm_wait covers bs_out).  sm_root_anc: the oldest slot in reach (lag
  // sm_depth) was recorded by a resample, so its ancestors are real (a cleared ring's root has none).
  bool sm_root_anc = false;
  BsScratch bs;
  DevBuf<double> bs_w[2], bs_stage;
  Landing bs_out;
  // MAP trajectory decoding over the same ring (gpmdm_pf_set_map, gpmdm_pf_map_path, mappath.h;
  // capi_mappath.hip).  sm_map: every record also keeps the log-likelihood of the proposal each
  // slot particle copies, ll[ridx[i]], in the plane sm_ll (sm_L + 1 frames; a cleared ring's root
  // holds zeros) -- one more short launch per frame, none with the flag off.  The call's scratch
  // is its own, grown on demand; mp_out: the path's rows and their pinned landing buffer (sm_wait
  // covers it).
  bool sm_map = false;
  DevBuf<double> sm_ll;
  MpScratch mp;
  Landing mp_out;
  // Backward simulation over the same ring (gpmdm_pf_sample_trajectories, backsample.h;
  // capi_backsample.hip): scratch of its own, grown on demand, and the per-lag rows and poses with
  // their pinned landing buffer (sm_wait covers fs_out).
  FsScratch fs;
  Landing fs_out;
  // Innovations and the GP's predictive variance (gpmdm_pf_set_predictive, gpmdm_pf_innovation,
  // gpmdm_pf_observation_gp and the banks'; obs_innov.h, capi_innov.hip).  predictive: every
  // weigh keeps vc = 1 - k^T K_y^-1 k of its particles in vc_prop (F x Pf, the order of X_prop
  // and ll), remembers where the frame's staged z lies (pv_z: pf->z or the frame's mapped
  // staging slot -- either is next written by the staging of a later frame, which follows that
  // frame's propagate) and the mask it was weighed with (pv_mask: mapped, F x D bytes;
  // pv_masked).  pv_weighed: a frame has been weighed with the feature on since the last
  // propagate, init, import, rebind or set_predictive (pv_has_vc: an observation kernel ran
  // for it, i.e. no single-filter blackout); pv_resampled: that frame's resample has completed,
  // so vc_prop[ridx] is the resampled cloud's.  The calls' scratch is their own, grown on
  // demand; iv_out.ev follows their launches (quiesce waits for it while pending).
  bool predictive = false, pv_weighed = false, pv_has_vc = false, pv_resampled = false, pv_masked = false;
  DevBuf<double> vc_prop;
  const double* pv_z = nullptr;
  PinBuf<unsigned char> pv_mask;
  DevBuf<double> iv_part;
  Landing iv_out;
  void pv_clear() { pv_weighed = pv_has_vc = pv_resampled = gt_ready = false; }
  // Outlier gating inside the frame (gpmdm_pf_set_gate, gpmdm_pf_gate_report and the banks'
  // gpmdm_bank_set_gate, gpmdm_bank_gate_report; obs_gate.h, capi_gate.hip).  gate_k > 0: on
  // (one rank, predictive on; gate_ks: the F filters' thresholds, +inf: that filter never
  // rejects; gate_k: the first of them): weigh ends with gate_frame -- the innovation launches
  // into scratch of the gate's own (gt_part, gt_out), then the decision, the re-weigh tile and
  // its finish, each once for all F filters -- on the frame's stream, so the frame's read-out
  // follows them and the lifecycle waits cover them.  gt_tab: the device tables (F x GateTab),
  // gt_sp the re-weigh partials, gt_lil the host's log il2_j of the filter's model (uploaded by
  // set_gate and again by a rebind), gt_pin the report's pinned landing buffer.
  // gt_cfg: the decision's F x {threshold, cap} table, the cap floor(limit D_obs_f) formed on
  // the host in fp64 from the frame's per-filter observed counts; gt_cfg_host is what the device
  // holds, and gate_frame uploads a frame's table only when it differs (a new threshold, limit or
  // mask), after the wait that guards gt_lil (zslot_free: the last frame's decision has read it).
  // gt_ready: a frame has been weighed in gated mode since the last propagate, init, import,
  // rebind, set_predictive or set_gate (gt_host: a blackout frame of every filter, no launch;
  // gt_black: the filters blacked out in that frame -- their report rows are the host's).
  double gate_k = 0.0, gate_limit = 0.5;
  std::vector<double> gate_ks, gt_cfg_host;
  std::vector<unsigned char> gt_black;
  bool gt_ready = false, gt_host = false;
  DevBuf<double> gt_part, gt_out, gt_tab, gt_sp, gt_lil, gt_cfg;
  PinBuf<double> gt_pin;
  // likelihood finish deferred into the resampling launch (single-shard small filters:
  // k_small_resample computes ll first, one launch less per frame); flush_ll runs it for
  // any reader of ll that comes first
  bool ll_pending = false;
  ObsFinishArgs oa_pending{};
  const GpImage* obs_img = nullptr;   // the observation launch's image and shape (obs_pick)
  TileGeo obs_geo{};
  DevBuf<int> guide;                // F x (GB + 3) inverse-CDF guide table
  DevBuf<int> sys_mark, sys_block;  // systematic resampling by scan (pf_kernels.hip)
  // ancestor de-duplication: owner/slot are C x P keyed by (class, ancestor)
  DevBuf<unsigned> owner;
  DevBuf<int> slot, lflag, lblock, ltab, lperm;
  // ancestor-ordered shards (multi-rank philox filters, shard_order.hip): own = particles
  // in order of their resampling uniform's bucket; this rank evaluates positions [lo, hi)
  DevBuf<int> own;
  DevBuf<int> own_inv;               // own_inv[own[r]] = r
  DevBuf<unsigned char> own_tmp;
  size_t own_tmp_bytes = 0;
  bool own_valid = false;
  bool shard_order = true;            // gpmdm_pf_set_shard_order
  // The order a resample installs depends only on (seed, frame), so the pre-switch computes
  // the next resample's order into own_next / inv_next behind the read-out (the GPU's gap
  // while the host takes the outputs); that resample swaps it in instead of computing it.
  DevBuf<int> own_next, inv_next;
  long long own_next_frame = -1;     // the frame own_next was computed for (-1: none)
  // (single-rank filters keep it only with the observation-GP cutoff: particles of one
  // resampling-ancestor range form compact tiles, which skip more of the cutoff's K-steps)
  bool order_wanted() const {
    return own && (n_ranks > 1 || obs_cutoff) && dedup && shard_order && resample_mode != GPMDM_RESAMPLE_SYSTEMATIC &&
           uniform_order_supported(P);
  }
  // Exchanged rows read in place (gpmdm_pf_unpack_part): the all-gathered {class, state} rows
  // are read by the resample's gathers through the ownership order (only the ancestors' rows
  // are ever touched) and the {ll} column by a launch inside the resample that also writes
  // the normaliser's block maxima, instead of two unpack passes over every particle.  Rows
  // are in position order (row r = particle own[r]); *_w = doubles per row.  flush_rows
  // writes them out for a reader that needs X_prop / cls_new / ll first (export).
  const double* rows_st = nullptr;   // column 0 = class, 1..d = state
  int rows_st_w = 0;
  const double* rows_ll = nullptr;   // column 0 = ll
  int rows_ll_w = 0;
  const int* rows_inv = nullptr;     // the ownership order the rows were gathered in (nullptr: identity)
  // observation upload through two pinned slots (a pageable hipMemcpyAsync is staged by the
  // runtime and stalls the launching thread); each slot's event guards its reuse
  PinBuf<double> zpin[2];             // mapped (small z read in place)
  PinBuf<double> rpin;                // pinned read-out landing buffer (F x (C + d + 1))
  // replay-mode draws (E, normals, U) staged through pinned buffers: the caller's arrays are
  // free for reuse when the call returns, whatever the runtime does with pageable copies;
  // each buffer's event guards its reuse
  // Small draws (<= kZeroCopyBytes: the notebook's P = 100) are not copied at all: the
  // kernels read them from the mapped pinned buffer (a copy is a launch of its own, ~4 us
  // on the frame's critical path).  rep_src[k] is what the kernels read this frame; the
  // event, recorded after the consuming launches (draws_used), guards the buffer's reuse.
  PinBuf<double> rep_pin[3];          // mapped
  const double* rep_src[3] = {nullptr, nullptr, nullptr};
  Event rep_ev[3];
  static constexpr size_t kZeroCopyBytes = 32768;
  hipError_t upload_draws(int k, double* dst, const double* src, size_t n, hipStream_t s) {
    // the buffer's previous readers have run (kernels that read it in place: guarded by the
    // read-out number of the frame that read it, see draws_used)
    const bool in_place = sizeof(double) * n <= kZeroCopyBytes && rep_pin[k].dev;
    hipError_t e = in_place && seq_pin ? wait_readout(ro_seq) : rep_ev[k].sync();
    if (e != hipSuccess) return e;
    // draws written straight into the staging buffer (gpmdm_pf_draw_buffers): no copy
    if (src != rep_pin[k]) std::memcpy(rep_pin[k], src, sizeof(double) * n);
    if (in_place) {
      rep_src[k] = rep_pin[k].dev;
      return hipSuccess;
    }
    rep_src[k] = dst;
    return hipMemcpyAsync(dst, rep_pin[k], sizeof(double) * n, hipMemcpyHostToDevice, s);
  }
  // after the launches that read buffer k: an event, unless they read it in place and the
  // frame's read-out number follows them (each event record between kernels idles the GPU
  // ~6 us; at the notebook's 0.11 ms frames that is 5%)
  hipError_t draws_used(int k, hipStream_t s) {
    if (seq_pin && rep_pin[k].dev && rep_src[k] == rep_pin[k].dev) return hipSuccess;
    return rep_ev[k].record(s);
  }
  PinBuf<int> cnt_pin;                // class counts landing buffer (mapped; replay mode)
  // Host-side class counts (single small replay filters).  The per-class normals are drawn
  // on the host with shapes P_c x d after the switch, so the switch's class counts used to
  // cost a mid-frame stream synchronisation.  The switch is argmax_j T[c_p, j] / E[p, j]
  // (k_switch), and every input is on the host once the previous resample's classes are:
  // k_small_resample also writes them into mapped memory (cls_pin), so the host computes the
  // same counts with the same fp64 divisions and comparisons while the kernels run.  The
  // device's own counts still land in cnt_pin and are compared at the next synchronisation
  // (a mismatch is an error, never a silent divergence).
  PinBuf<int> cls_pin;                // mapped: the current classes (valid when cls_host_ok)
  bool cls_host_ok = false;           // cls_pin holds the classes the next switch reads
  bool cls_ev_pending = false;        // ... once cls_ev (after the resample that wrote them) is done
  Event cls_ev;
  Event cnt_ev;                       // after the switch whose device counts cnt_expect awaits
  std::vector<double> T_host;         // C x C
  int cnt_expect[kMaxClasses] = {0};
  bool cnt_check = false;             // compare cnt_pin with cnt_expect at the next sync
  // read-outs written by the resampling kernels straight into mapped host memory as well
  // (small read-out tables): gpmdm_pf_read then needs no copy launch, only the stream sync
  PinBuf<double> ro_pin;
  // A z slot is written again two frames after its frame used it; its readers (k_dyn_finish,
  // the observation tiles, the likelihood finish) precede that frame's read-out, and the
  // resample of the frame in between has recorded ro_ev by then (the call order is enforced),
  // so ro_ev guards both slots -- no event record of its own between two kernels.
  hipError_t zslot_free() {
    if (seq_pin) return wait_readout(ro_seq);
    return ro_ev_ok ? ro_ev.sync() : hipSuccess;
  }
  // Filters whose read-outs land in mapped memory (one number per filter of a bank) also get
  // their sequence numbers there (the read-out kernels publish them after the values:
  // publish_readout), and the host waits on them instead of on an event recorded behind the
  // read-out -- such a record idles the GPU ~6 us before the next frame's switch.
  PinBuf<long long> seq_pin;
  // the last read-out's number (0: none launched); atomic because gpmdm_pf_draws_free may
  // run on a drawing thread while the frame's thread launches the next read-out
  std::atomic<long long> ro_seq{0};
  long long seq_min() const { return min_mapped(seq_pin, F); }   // (one number per filter)
  // The numbers are read with ACQUIRE loads: the device publishes each with a system-scope
  // release store after the values it guards (publish_seq, pf_kernels.hip), so a caller that
  // has seen a number >= its target may then read those values with plain loads -- the
  // acquire keeps the compiler (and the CPU) from moving them above the number's load.
  static long long min_mapped(const long long* p, long long n) {
    long long v = __atomic_load_n(p, __ATOMIC_ACQUIRE);
    for (long long f = 1; f < n; ++f) {
      const long long x = __atomic_load_n(p + f, __ATOMIC_ACQUIRE);
      v = x < v ? x : v;
    }
    return v;
  }
  // until every one of the n numbers at p is >= target (a number the device publishes after
  // the data it guards).  `s`: the stream the publishing kernel was launched on -- if the
  // number has not appeared after 60 s, that stream is drained and the number looked at once
  // more (an error, not a hang, if it is still missing).
  static hipError_t wait_mapped(const long long* p, long long n, long long target, hipStream_t s) {
    if (min_mapped(p, n) >= target) return hipSuccess;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1;; ++it) {
      if (min_mapped(p, n) >= target) return hipSuccess;
      if ((it & 255) == 0) {
        std::this_thread::yield();
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
          const hipError_t e = hipStreamSynchronize(s);
          if (e != hipSuccess) return e;
          return min_mapped(p, n) >= target ? hipSuccess : hipErrorUnknown;
        }
      } else {
        __builtin_ia32_pause();
      }
    }
  }
  hipStream_t ro_stream = nullptr;    // the stream of the last read-out (its number's publisher)
  hipStream_t cnt_stream = nullptr;   // the stream of the switch whose counts cseq guards
  hipError_t wait_readout(long long target) const { return wait_mapped(seq_pin, F, target, ro_stream); }
  hipError_t wait_counts() const { return wait_mapped(cseq_pin, 1, cseq, cnt_stream); }
  // the switch's class counts (replay filters): k_scan_counts publishes cseq after writing
  // them to cnt_pin, so the host's wait for them needs no event record behind the switch
  PinBuf<long long> cseq_pin;
  long long cseq = 0;
  bool pre_counts_seq = false;        // the pending pre-switch's counts come with cseq
  int zslot = 0;
  bool z_staged = false;              // zpin[zslot] holds the frame's z, k_dyn_finish copies it
  DevBuf<double> qdyn, mudyn, qobs, sobs;
  int nparts_dyn_max = 0;
  // failure detection: kHealth* counters, device, zeroed at create
  DevBuf<unsigned> health;
  // predict(): per-particle dynamics-GP means, lazily allocated
  DevBuf<double> pred_q, pred_mu, pred_mu_p, pred_out;
  DevBuf<double> z, E, normals, U;
  DevBuf<unsigned long long> gmax;
  // single filters: k_obs_ll's per-block maxima of ll, read by the normaliser in place of
  // k_norm_max (bmax_ready: produced by this frame's weigh, not yet consumed)
  DevBuf<unsigned long long> bmax;
  bool bmax_ready = false;
  DevBuf<unsigned long long> bmax_rows;      // multi-rank filters: k_rows_ll's block maxima
  // the leader election's owner table is all 0xffffffff (the last compaction restored it)
  bool owner_clean = false;
  DevBuf<double> e, local, blocksum, blockoffw, total, partials, readout;
  // library-driven exchange (gpmdm_pf_set_comm): an RCCL communicator of n_ranks ranks, a
  // library-owned stream for the collectives, and the packed rows.  pad = rows per rank in
  // the collective (the largest shard; ranks' shards differ by at most one row).  When the
  // shards are uneven (or GPMDM_COMM_PAD_ROWS asks for it) the gather lands in *_stage and
  // each rank's rows are copied down to their shard offset.
  ncclComm_t comm = nullptr;
  bool comm_loop = false;            // comm is an in-process loopback communicator (tests)
  hipStream_t cstream = nullptr;
  Event cev[3];
  long long pad = 0;
  bool padded = false;
  DevBuf<double> xs_send, xs_recv, xs_stage, xl_send, xl_recv, xl_stage;
  void release_comm() {
    if (cstream) (void)hipStreamSynchronize(cstream);
    for (DevBuf<double>* b : {&xs_send, &xs_recv, &xs_stage, &xl_send, &xl_recv, &xl_stage}) b->release();
    if (cstream) (void)hipStreamDestroy(cstream);
    cstream = nullptr;
    comm = nullptr;                    // the caller owns the communicator
    comm_loop = false;
  }
  // Pre-switch (Philox filters): the next frame's class switch needs no host input (its
  // draws are keyed by the frame counter), so the resample launches it right behind the
  // read-out; it runs while the host takes the frame's outputs, and gpmdm_pf_switch then
  // only consumes it.  Every later call that reads or rewrites the switch's tables, or must
  // see the filter between frames (predict, set_*, init), drops it first, and the next
  // gpmdm_pf_switch launches it again -- the same draws, bitwise the same tables.  The
  // normaliser-maximum reset and the dynamics row count moved out of the switch into
  // k_dyn_finish, so nothing a between-frames reader sees changes.  GPMDM_NO_PRESWITCH=1
  // turns it off (A/B).
  bool preswitch = true;
  bool preswitched = false;           // launched, not yet consumed by gpmdm_pf_switch
  // between switch and resample: a step is under way (a pending pre-switch is not one)
  bool mid_step() const { return (switched && !preswitched) || dyn_done || propagated; }
  // after the pre-switch: recorded on sw_stream only when another stream or the host must
  // wait for it (an event record between two kernels idles the GPU ~6 us; on the stream
  // itself the order already holds), so it covers whatever followed the pre-switch there too
  Event sw_ev;
  hipStream_t sw_stream = nullptr;
  // Replay filters pre-switch on the caller's request (gpmdm_pf_preswitch: the next frame's
  // Exp(1) draws are the caller's, drawn ahead on the host): the switch, its class counts into
  // mapped memory (cnt_pin, cnt_done after them) and the dynamics-GP tiles, all behind the
  // read-out.  gpmdm_pf_switch consumes it when handed the same E pointer.
  const double* pre_E = nullptr;
  bool pre_counts = false;            // the pre-switch's counts land in cnt_pin (cnt_done)
  hipStream_t up_stream = nullptr;    // its Exp(1) draws go up on this stream, beside the frame
  Event up_ev;                        // still running on the caller's (the switch waits on it)
  Event ndev_ev;                      // after the last dynamics finish (the device normals' reader)
  hipError_t make_up_stream() {
    return up_stream ? hipSuccess : hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking);
  }
  // Replay normals copied to the device ahead of the propagate that reads them
  // (gpmdm_pf_stage_normals): the value ranges staged from nstage_ptr since the last propagate
  const double* nstage_ptr = nullptr;
  bool n_staged_frame = false;        // this frame's normals came fully staged
  std::vector<std::pair<long long, long long>> nstaged;
  bool normals_staged(const double* p, long long n) const {   // does the union cover [0, n)?
    if (p != nstage_ptr) return false;
    long long reach = 0;
    for (const auto& r : nstaged) {     // sorted by start
      if (r.first > reach) return false;
      reach = std::max(reach, r.second);
    }
    return reach >= n;
  }
  Event ro_ev;                        // after the last read-out (gpmdm_pf_read waits on it)
  bool ro_ev_ok = false;
  int* rows_last() const { return small + 504; }   // rows of the last dynamics pass
  // Tile height of the dynamics pass on the 16 x 256 image: 16, 32 or 64 particle rows per
  // workgroup give bitwise the same results (same column blocks, same per-row association),
  // so the height is a pure schedule choice: short grids of few rows want 16-row tiles, long
  // grids 64-row ones (a B fragment feeds 4 row groups).  Chosen per frame from the row count
  // of the dynamics pass the last gpmdm_pf_read saw (k_dyn_finish writes it to rows_pin).
  PinBuf<int> rows_pin;
  int rows_hint = 0;
  TileGeo dyn_geo_frame{};            // this frame's dynamics launch shape (set by the switch)
  // timing
  bool timing = false;
  std::vector<hipEvent_t> pool;
  struct Rec { int stage; hipEvent_t a, b; };
  std::vector<Rec> recs;

  // class tables of the step's grouping (small[0, 240)); predict() groups into its own
  // copy (small[256, 496), base 256) so the step's tables -- which gpmdm_pf_dyn_rows
  // reads -- survive a predict between steps
  static constexpr int kPredictTables = 256;
  ClassTables tables(int base = 0) const { return ClassTables{small + base}; }
  SegTables ltables() const { return SegTables{ltab}; }   // the leaders' segment tables
  const int* own_order() const { return own_valid ? own.p : nullptr; }

  // Only what has an order to respect: the side streams are drained (and destroyed) before
  // the members' destructors, which run after this body, hand the buffers those streams used
  // back to the pool and destroy the events; the model goes when its last user has gone.
  ~gpmdm_pf() {
    // (gpmdm_pf_destroy has waited for the filter's own work: quiesce, capi_pf.hip; a handle
    // deleted by a failed create has launched nothing)
    if (m) (void)hipSetDevice(m->device);
    if (up_stream) (void)hipStreamSynchronize(up_stream);
    release_comm();
    if (up_stream) (void)hipStreamDestroy(up_stream);
    for (auto& r : recs) { pool.push_back(r.a); pool.push_back(r.b); }
    for (auto ev : pool) (void)hipEventDestroy(ev);
    if (m) m->remove_user(this);
    model_release(m);
  }

  hipEvent_t ev() {
    if (!pool.empty()) { hipEvent_t x = pool.back(); pool.pop_back(); return x; }
    hipEvent_t x = nullptr;
    // timing-only events: no system-scope fence at record time (a fenced record left a
    // ~10 us bubble between the stages it separates)
    (void)hipEventCreateWithFlags(&x, hipEventDisableSystemFence);
    return x;
  }
  unsigned timing_mask = (1u << GPMDM_N_STAGES) - 1;   // gpmdm_pf_timing_stages
  void mark_begin(hipStream_t s, int stage, hipEvent_t& a) {
    a = nullptr;
    if (timing && (timing_mask >> stage & 1u)) { a = ev(); (void)hipEventRecord(a, s); }
  }
  void mark_end(hipStream_t s, int stage, hipEvent_t a) {
    if (!timing || !a) return;
    hipEvent_t b = ev();
    (void)hipEventRecord(b, s);
    recs.push_back({stage, a, b});
  }
};

namespace gpmdm::capi {
// shared helpers (defined in the unit named beside each)
void fill_tile_common(TileParams& tp, const gpmdm_model* m, bool dyn);
ResampleArgs resample_args(gpmdm_pf* pf);
NormArgs norm_args(gpmdm_pf* pf);
int flush_ll(gpmdm_pf* pf, hipStream_t s);
int drop_preswitch(gpmdm_pf* pf, hipStream_t s, bool host_wait);
int quiesce(gpmdm_pf* pf);
int quiesce_users(gpmdm_model* m);
// smoothing (capi_smooth.hip): wait for the record / read-out launches in flight; record the
// frame just resampled on s; forget the history and record the current cloud as its root on s
int sm_wait(gpmdm_pf* pf);
int sm_record(gpmdm_pf* pf, hipStream_t s);
int sm_clear(gpmdm_pf* pf, hipStream_t s);
// the pose read-out over the F clouds at X (F x Pf x d) into out (F x {mean[D], spread[D]});
// capi_pf.hip
ReadoutParams pose_readout(const gpmdm_pf* pf, const double* X, double* part, double* out);
// The common part of the class grouping's two launches (launch_scan_counts, launch_group) over
// all P particles with classes `cls`, whose per-block counts are in blockcounts: tables, block
// offsets and the permutation it writes; pt: the tile unit of the dynamics pass.  capi_pf.hip
void fill_grouping(ScanArgs& sc, GroupArgs& ga, ClassTables tb, const int* blockcounts, int* blockoff, int* perm,
                   const int* cls, long long P, int C, int pt);
// The dynamics-GP tile launches of image set dset in shape geo (per class, segments of at most
// kMaxSeg classes per launch) over the rows of X that tb and perm name, at most rows_ub of
// them, into q (leading dimension ld_q) and mu.  capi_frame.hip
void launch_dyn_tiles(const gpmdm_model* m, const std::vector<GpImage>& dset, TileGeo geo, SegTables tb,
                      const int* perm, const double* X, long long rows_ub, double* q, long long ld_q, double* mu,
                      hipStream_t s);
int sm_set(gpmdm_pf* pf, int lag);     // (set_smoothing of a checked handle, single or bank)
// gpmdm_predict_dyn's launches for class c over n device rows, q: predict_dyn_scratch doubles
// (capi_model.hip)
size_t predict_dyn_scratch(const gpmdm_model* m, int c, long long n, long long shape_n = -1);
void launch_predict_dyn(const gpmdm_model* m, int c, const double* Xs, long long n, double* mu, double* var,
                        double* q, hipStream_t s, long long shape_n = -1, const int* n_dev = nullptr);
// the backward step's parts that backward simulation shares (capi_backsmooth.hip): the refusals
// decided before any launch, the classes as the kernels take them, and the sources' records
size_t bs_record_bytes(int C, int d, long long n_s);
int bs_check(const gpmdm_model* m, long long n_s, long long n_t);
int bs_to_classes(const int64_t* src, long long n, int C, std::vector<int>& dst, const char* what);
int bs_records(const gpmdm_model* m, DevBuf<double>& rec, DevBuf<double>& mu, DevBuf<double>& var, DevBuf<double>& q,
               const double* T, long long n_s, const double* Xs, const int* cs, const double* a, hipStream_t s);
int iv_wait(gpmdm_pf* pf);             // an innovation call's launches in flight (capi_innov.hip)
// gating (capi_gate.hip): the end of a gated-mode weigh on s; the log il2 table of the filter's
// (new) model
int gate_frame(gpmdm_pf* pf, hipStream_t s);
int gate_rebind(gpmdm_pf* pf);
// staging of a forecast's per-step clouds may take this much device memory (H x P x (d + 1)
// doubles); so may the smoothing ring, and a smoothed read-out's staging of the particle rows
constexpr size_t kForecastStageBytes = (size_t)1 << 30;
constexpr size_t kSmoothBytes = (size_t)1 << 30;
int h2d(void* dst, const void* src, size_t bytes);
// the observation-GP cutoff image (capi_model.hip; packed on the host or the device)
struct CutoffPlan {
  std::vector<long long> perm, toff;
  std::vector<double> sph, rec;
  double tau = 0.0;
  int T_R = 0, T_M = 0;
};
int cutoff_plan(gpmdm_model* m, double sigma2, const double* M, const double* y_absmax, CutoffPlan& pl);
int cutoff_install(gpmdm_model* m, const CutoffPlan& pl, const std::function<int(double*, const long long*)>& fill);
int do_switch(gpmdm_pf* pf, const double* E, int64_t* class_counts, hipStream_t s, bool order_ahead = false, bool counts_ahead = false, bool e_uploaded = false);
int propagate_dynamics(gpmdm_pf* pf, const double* normals, hipStream_t s, bool zstage = false);
int weigh(gpmdm_pf* pf, const double* zh, hipStream_t s);
int propagate_exchange(gpmdm_pf* pf, const double* zh, const double* normals, hipStream_t s);
int flush_rows(gpmdm_pf* pf, hipStream_t s);
const GpImage& obs_pick(const gpmdm_model* m, long long P, long long n, TileGeo& geo);
}  // namespace gpmdm::capi

