// C ABI, filter and bank lifecycle: create / destroy, init / import / export of the
// particle state (gpmdm_pf.py:78-115), settings (de-duplication, tile images, shard order,
// model rebind, timing), health counters and predict().  The banks are filters with F > 1
// (gpmdm_bank_create): every entry point here serves both.
#include <memory>

#include "capi_internal.h"

namespace gpmdm::capi {

// The ownership order's buffers (shard_order.hip): multi-rank Philox filters at create,
// single-rank ones with the observation-GP cutoff.  All or none.
static int alloc_order(gpmdm_pf* pf) {
  const size_t P = (size_t)pf->P;
  pf->own_tmp_bytes = std::max<size_t>(uniform_order_temp_bytes(pf->P), 1);
  if (pf->own.alloc(P) || pf->own_inv.alloc(P) || pf->own_next.alloc(P) || pf->inv_next.alloc(P) ||
      pf->own_tmp.alloc(pf->own_tmp_bytes)) {
    for (DevBuf<int>* b : {&pf->own, &pf->own_inv, &pf->own_next, &pf->inv_next}) b->release();
    pf->own_tmp.release();
    return fail(GPMDM_E_NOMEM, "ownership order buffers");
  }
  return GPMDM_OK;
}

// ------------------------------------------------------------------------------------
static int pf_create(gpmdm_model_t m, const double* T, int64_t F, int64_t Pf, int rng_mode, uint64_t seed,
                     int resample_mode, int n_ranks, int rank, gpmdm_pf_t* out) {
  CHECK(m && T && out, "null argument");
  *out = nullptr;
  CHECK(Pf >= 1 && F >= 1 && F <= 65535 && F * Pf < (1ll << 31) - 256, "num_particles out of range");
  CHECK(F == 1 || (rng_mode == GPMDM_RNG_PHILOX && n_ranks == 1),
        "filter banks use device (philox) draws on one rank; shard filters, not particles");
  const long long P = F * Pf;
  CHECK(rng_mode == GPMDM_RNG_REPLAY || rng_mode == GPMDM_RNG_PHILOX, "bad rng mode");
  CHECK(resample_mode == GPMDM_RESAMPLE_MULTINOMIAL || resample_mode == GPMDM_RESAMPLE_SYSTEMATIC,
        "bad resample mode");
  CHECK(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bad rank");
  HIPCHK(hipSetDevice(m->device));
  std::unique_ptr<gpmdm_pf> holder(new gpmdm_pf());   // released on every failure below
  gpmdm_pf* pf = holder.get();
  pf->m = m;
  m->refs.fetch_add(1);   // released by ~gpmdm_pf
  pf->P = P;
  pf->Pf = Pf;
  pf->F = (int)F;
  pf->n_ranks = n_ranks;
  pf->rank = rank;
  pf->lo = P * rank / n_ranks;
  pf->hi = P * (rank + 1) / n_ranks;
  pf->nloc = pf->hi - pf->lo;
  pf->rng_mode = rng_mode;
  pf->resample_mode = resample_mode;
  pf->seed_lo = (unsigned)(seed & 0xffffffffu);
  pf->seed_hi = (unsigned)(seed >> 32);
  pf->nb = (int)cdiv(P, 256);
  pf->nbf = (int)cdiv(Pf, 256);
  const int C = m->C, d = m->d, D = m->D;
  const int maxparts = m->dyn_parts_max();
  pf->nparts_dyn_max = maxparts;
  const long long nl = std::max(pf->nloc, 1ll);
#define ALLOC(buf, n) TRY(pf->buf.alloc((size_t)(n)))
  ALLOC(T, C * C);
  ALLOC(X, P * d);
  ALLOC(X_prop, P * d);
  ALLOC(ll, P);
  ALLOC(cls, P);
  ALLOC(cls_new, P);
  ALLOC(perm, P);
  ALLOC(ridx, P);
  ALLOC(blockcounts, (long long)pf->nb * C);
  ALLOC(blockoff, (long long)pf->nb * C);
  ALLOC(small, 512);
  ALLOC(obs_tab, 16);
  ALLOC(owner, (long long)C * P);
  ALLOC(slot, (long long)C * P);
  ALLOC(lflag, P);
  ALLOC(lblock, pf->nb);
  ALLOC(ltab, 200);
  ALLOC(lperm, P);
  ALLOC(qdyn, (long long)maxparts * nl);
  ALLOC(mudyn, nl * d);
  ALLOC(qobs, (long long)obs_parts_max(m) * nl);
  ALLOC(sobs, (long long)obs_blocks_max(m) * nl);   // fused likelihood partials (no mean stored)
  ALLOC(z, F * D);
  if (rng_mode == GPMDM_RNG_REPLAY) {
    ALLOC(E, P * C);
    ALLOC(normals, P * d);
    ALLOC(U, P);
  }
  ALLOC(gmax, F);
  if (F == 1 && n_ranks == 1) ALLOC(bmax, pf->nb);
  if (F == 1 && n_ranks > 1) ALLOC(bmax_rows, rows_ll_blocks(P));
  ALLOC(e, P);
  ALLOC(local, P);
  ALLOC(blocksum, F * pf->nbf);
  ALLOC(blockoffw, F * pf->nbf);
  ALLOC(total, F);
  ALLOC(guide, guide_buckets_used(Pf) > 0 ? F * (guide_buckets(Pf) + 3) : 1);
  ALLOC(partials, F * pf->nbf * (C + 1 + d));
  ALLOC(readout, F * (C + d + 1));
  ALLOC(health, kHealthN);
  if (resample_mode == GPMDM_RESAMPLE_SYSTEMATIC) {
    ALLOC(sys_mark, P);
    ALLOC(sys_block, F * pf->nbf);
  }
  if (n_ranks > 1 && rng_mode == GPMDM_RNG_PHILOX) TRY(alloc_order(pf));
#undef ALLOC
  for (int k = 0; k < 2; ++k)
    if (pf->zpin[k].alloc_mapped((size_t)(F * D))) return fail(GPMDM_E_NOMEM, "pinned observation buffer");
  if (pf->rpin.alloc((size_t)(F * (C + d + 1)))) return fail(GPMDM_E_NOMEM, "pinned read-out buffer");
  if (sizeof(double) * F * (C + d + 1) <= 32768) {
    if (pf->ro_pin.alloc_mapped((size_t)(F * (C + d + 1)))) return fail(GPMDM_E_NOMEM, "mapped read-out buffer");
    if (pf->seq_pin.alloc_mapped((size_t)F)) return fail(GPMDM_E_NOMEM, "mapped read-out number");
    for (long long f = 0; f < F; ++f) pf->seq_pin[f] = 0;
  }
  if (pf->rows_pin.alloc_mapped(1)) return fail(GPMDM_E_NOMEM, "mapped row-count buffer");
  *pf->rows_pin = 0;
  if (rng_mode == GPMDM_RNG_REPLAY) {
    const long long n[3] = {P * C, P * d, P};      // E, normals, U
    // mapped, coherent (fine-grained): kernels may read the small draws in place
    for (int k = 0; k < 3; ++k)
      if (pf->rep_pin[k].alloc_mapped((size_t)(n[k]))) return fail(GPMDM_E_NOMEM, "pinned replay-draw buffer");
    if (pf->cnt_pin.alloc_mapped((size_t)(kMaxClasses))) return fail(GPMDM_E_NOMEM, "pinned class-count buffer");
    if (pf->cseq_pin.alloc_mapped(1)) return fail(GPMDM_E_NOMEM, "mapped class-count number");
    *pf->cseq_pin = 0;
    if (F == 1 && n_ranks == 1 && P <= kHostCountsMaxP) {
      if (pf->cls_pin.alloc_mapped((size_t)(P))) return fail(GPMDM_E_NOMEM, "pinned class buffer");
      pf->T_host.assign(T, T + (size_t)C * C);
    }
  }
  pf->preswitch = rng_mode == GPMDM_RNG_PHILOX && std::getenv("GPMDM_NO_PRESWITCH") == nullptr;
  pf->obs_img = &obs_pick(m, pf->Pf, pf->nloc, pf->obs_geo);
  const int tab[5] = {(int)pf->lo, (int)pf->hi, 0, 0, (int)cdiv(pf->nloc, pf->obs_geo.pt())};
  hipStream_t life = life_stream(m->device);   // (the lifecycle stream: no null-stream ordering)
  if (!life || hipMemcpyAsync(pf->obs_tab, tab, sizeof(tab), hipMemcpyHostToDevice, life) != hipSuccess ||
      hipMemcpyAsync(pf->T, T, sizeof(double) * C * C, hipMemcpyHostToDevice, life) != hipSuccess ||
      hipMemsetAsync(pf->health, 0, sizeof(unsigned) * kHealthN, life) != hipSuccess ||
      hipMemsetAsync(pf->small, 0, sizeof(int) * 512, life) != hipSuccess || hipStreamSynchronize(life) != hipSuccess)
    return fail(GPMDM_E_HIP, "upload of particle-filter tables failed");
  m->add_user(pf);
  *out = holder.release();
  return GPMDM_OK;
}

ResampleArgs resample_args(gpmdm_pf* pf) {
  const gpmdm_model* m = pf->m;
  ResampleArgs ra{};
  ra.P = pf->Pf;
  ra.nb = pf->nbf;
  ra.F = pf->F;
  ra.C = m->C;
  ra.d = m->d;
  ra.systematic = pf->resample_mode == GPMDM_RESAMPLE_SYSTEMATIC;
  ra.frame = pf->frame;
  ra.seed_lo = pf->seed_lo;
  ra.seed_hi = pf->seed_hi;
  ra.local = pf->local;
  ra.blockoff = pf->blockoffw;
  ra.ll = pf->ll;
  ra.e = pf->e;
  ra.total = pf->total;
  ra.gmax = pf->gmax;
  ra.cls_src = pf->cls_new;
  ra.X_src = pf->X_prop;
  ra.cls_dst = pf->cls;
  ra.X_dst = pf->X;
  ra.ridx = pf->ridx;
  ra.partials = pf->partials;
  ra.readout = pf->readout;
  ra.readout_host = pf->ro_pin.dev;
  ra.guide = pf->guide;
  ra.GB = guide_buckets_used(pf->Pf);   // 0: plain search
  ra.sys_mark = pf->sys_mark;           // systematic: by scan, no search
  ra.sys_block = pf->sys_block;
  return ra;
}

NormArgs norm_args(gpmdm_pf* pf) {
  NormArgs na{};
  na.P = pf->Pf;
  na.nb = pf->nbf;
  na.F = pf->F;
  na.ll = pf->ll;
  na.gmax = pf->gmax;
  na.e = pf->e;
  na.local = pf->local;
  na.blocksum = pf->blocksum;
  na.blockoff = pf->blockoffw;
  na.total = pf->total;
  if (pf->ll_pending) {
    na.obs = pf->oa_pending;
    na.obs_pending = 1;
  }
  if (pf->bmax_ready) na.bmax = pf->bmax;
  return na;
}

int flush_ll(gpmdm_pf* pf, hipStream_t s) {
  if (!pf->ll_pending) return GPMDM_OK;
  launch_obs_finish(pf->oa_pending, s);
  pf->ll_pending = false;
  HIPCHK(hipGetLastError());
  return GPMDM_OK;
}

// Undo a pre-switch before a call that reads or rewrites the switch's tables or needs the
// filter between frames: the caller's stream (or, with none, the host) waits for it, and
// the next gpmdm_pf_switch launches the switch again (same draws: the same tables).
int drop_preswitch(gpmdm_pf* pf, hipStream_t s, bool host_wait) {
  if (!pf->preswitched) return GPMDM_OK;
  if (host_wait || s != pf->sw_stream) HIPCHK(pf->sw_ev.record(pf->sw_stream));   // (see sw_ev)
  if (host_wait)
    HIPCHK(pf->sw_ev.sync());
  else if (s != pf->sw_stream)
    HIPCHK(pf->sw_ev.block(s));
  pf->preswitched = false;
  pf->switched = false;
  pf->gemm_ahead = pf->pre_counts = false;   // (a replay pre-switch's tiles are redone too)
  return GPMDM_OK;
}

// Wait for everything this filter has launched, and nothing else (DESIGN.md §1 "Lifecycle
// waits"): its pending pre-switch, its last read-out -- every stage of a frame precedes the
// read-out on the frame's stream, which publishes a sequence number in mapped memory (or
// records ro_ev) -- and its own side streams (replay uploads, the exchange's collectives).
// Calls between frames that launch work (export, health, predict, dyn_rows) wait for it
// themselves.  A filter stopped inside a frame (switched or propagated, not yet resampled)
// has no such marker: then, and only then, the device is synchronised.
int quiesce(gpmdm_pf* pf) {
  HIPCHK(hipSetDevice(pf->m->device));
  TRY(drop_preswitch(pf, nullptr, true));
  if (pf->switched || pf->propagated || pf->dyn_done) {
    HIPCHK(hipDeviceSynchronize());
  } else if (pf->seq_pin && pf->ro_seq.load() > 0) {
    HIPCHK(pf->wait_readout(pf->ro_seq.load()));
  } else if (pf->ro_ev_ok) {
    HIPCHK(pf->ro_ev.sync());
  }
  if (pf->up_stream) HIPCHK(hipStreamSynchronize(pf->up_stream));
  if (pf->cstream) HIPCHK(hipStreamSynchronize(pf->cstream));
  // read-outs launched without a copy, or that failed before their own wait (Landing::wait);
  // a smoothing record follows the frame's read-out number on the frame's stream
  TRY(pf->ro_obs.wait());
  TRY(pf->fc_out.wait());
  TRY(sm_wait(pf));
  return iv_wait(pf);
}

// The mask's device array and scalars from the filter's current model (gpmdm_pf_set_obs_mask,
// and again when the filter is rebound to a rebuilt model).  Between frames.
static int install_obs_mask(gpmdm_pf* pf, const std::vector<unsigned char>& mask) {
  const gpmdm_model* m = pf->m;
  const int D = m->D;
  // the last frame's observation kernels may still read lam2_obs: they precede its read-out
  // (a pending pre-switch reads neither, and stays pending)
  HIPCHK(pf->zslot_free());
  // F rows of lam2 (a bank: one mask per filter), then the finish's F-row table of scalars
  const int F = pf->F;
  const size_t n_lam = (size_t)F * D, n_all = n_lam + 3 * (size_t)F;
  if (!pf->lam2_obs) TRY(pf->lam2_obs.alloc(n_all));
  std::vector<double> lam2(n_all, 0.0);
  int n_tot = 0;
  double sl = 0.0, lc = 0.0;
  for (int f = 0; f < F; ++f) {
    const unsigned char* mf = mask.data() + (size_t)f * D;
    int n_obs = 0;
    sl = 0.0;
    for (int j = 0; j < D; ++j)
      if (mf[j]) {
        lam2[(size_t)f * D + j] = 1.0 / m->y_il2[(size_t)j];   // the model's y_lam2_dev value
        sl += std::log(m->y_il2[(size_t)j]);
        ++n_obs;
      }
    lc = ll_const(n_obs);
    double* row = lam2.data() + n_lam + 3 * (size_t)f;
    row[0] = (double)n_obs;
    row[1] = sl;
    row[2] = lc;
    n_tot += n_obs;
  }
  TRY(h2d(pf->lam2_obs, lam2.data(), sizeof(double) * n_all));
  pf->obs_mask = mask;
  pf->D_obs = n_tot;
  pf->sum_log_il2_obs = sl;            // (single filters: the finish's arguments)
  pf->ll_const_obs = lc;
  return GPMDM_OK;
}

ReadoutParams pose_readout(const gpmdm_pf* pf, const double* X, double* part, double* out) {
  const gpmdm_model* m = pf->m;
  ReadoutParams rp{};
  rp.X = X;
  rp.P = pf->Pf;
  rp.F = pf->F;
  rp.d = m->d;
  rp.D = m->D;
  rp.ls = m->y_ls_dev;
  rp.Xrec = m->obs.Xrec;
  rp.nks = ksteps((int)m->N);
  rp.Bro = m->ro_beta;
  rp.n_groups = readout_groups(m->D);
  rp.part = part;
  rp.out = out;
  return rp;
}

void fill_grouping(ScanArgs& sc, GroupArgs& ga, ClassTables tb, const int* blockcounts, int* blockoff, int* perm,
                   const int* cls, long long P, int C, int pt) {
  const SegTables sg = tb.seg();
  sc.nb = (int)cdiv(P, 256);
  sc.C = C;
  sc.pt = pt;
  sc.lo = 0;
  sc.hi = P;
  sc.blockcounts = blockcounts;
  sc.cls_new = cls;
  sc.blockoff = blockoff;
  sc.class_start = tb.class_start();
  sc.counts = tb.counts();
  sc.seg_pos_begin = sg.begin();
  sc.seg_pos_end = sg.end();
  sc.seg_out_base = sg.out();
  sc.seg_tile_start = sg.tiles();
  ga.P = P;
  ga.n = P;
  ga.C = C;
  ga.cls_new = cls;
  ga.class_start = tb.class_start();
  ga.blockoff = blockoff;
  ga.perm = perm;
}

}  // namespace gpmdm::capi

extern "C" {

int gpmdm_pf_create(gpmdm_model_t m, const double* T, int64_t P, int rng_mode, uint64_t seed,
                    int resample_mode, int n_ranks, int rank, gpmdm_pf_t* out) {
  return pf_create(m, T, 1, P, rng_mode, seed, resample_mode, n_ranks, rank, out);
}

int gpmdm_bank_create(gpmdm_model_t m, const double* T, int64_t n_filters, int64_t P, uint64_t seed,
                      int resample_mode, gpmdm_pf_t* out) {
  return pf_create(m, T, n_filters, P, GPMDM_RNG_PHILOX, seed, resample_mode, 1, 0, out);
}

int gpmdm_pf_shape(gpmdm_pf_t pf, int64_t* n_filters, int64_t* P) {
  CHECK(pf, "null handle");
  if (n_filters) *n_filters = pf->F;
  if (P) *P = pf->Pf;
  return GPMDM_OK;
}

int gpmdm_pf_destroy(gpmdm_pf_t pf) {
  if (!pf) return GPMDM_OK;
  const int rc = quiesce(pf);   // the filter's own launches only: its buffers are then released
  delete pf;                    // in the lifecycle stream's order (memory.hip)
  return rc;
}

int gpmdm_pf_init(gpmdm_pf_t pf, const double* states, const int64_t* classes) {
  CHECK(pf && states && classes, "null argument");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  const long long P = pf->P;
  std::vector<int> c32(P);
  for (long long i = 0; i < P; ++i) {
    CHECK(classes[i] >= 0 && classes[i] < m->C, "class id out of range");
    c32[i] = (int)classes[i];
  }
  TRY(quiesce(pf));                    // the filter's own frames, not the device
  pf->bmax_ready = false;
  // the uploads and the read-out of the initial state on the lifecycle stream (memory.hip)
  hipStream_t ls = life_stream(m->device);
  CHECK(ls, "the library's lifecycle stream");
  std::vector<int> r32(P);
  for (long long i = 0; i < P; ++i) r32[i] = (int)(i % pf->Pf);   // no shared ancestors yet
  const std::vector<unsigned long long> neg(pf->F, host_ord_enc(-INFINITY));
  HIPCHK(hipMemcpyAsync(pf->X, states, sizeof(double) * P * m->d, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->cls, c32.data(), sizeof(int) * P, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->ridx, r32.data(), sizeof(int) * P, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemsetAsync(pf->ll, 0, sizeof(double) * P, ls));
  HIPCHK(hipMemcpyAsync(pf->gmax, neg.data(), sizeof(unsigned long long) * pf->F, hipMemcpyHostToDevice, ls));
  if (pf->cls_pin) {
    std::memcpy(pf->cls_pin, c32.data(), sizeof(int) * P);
    pf->cls_host_ok = true;
    pf->cls_ev_pending = false;
  }
  // read-outs of the initial state: ll = log_w = 0, w = 1/P (gpmdm_pf.py:102-104)
  ResampleArgs ra = resample_args(pf);
  ra.identity = 1;
  ra.cls_src = pf->cls;
  ra.X_src = pf->X;
  launch_normalise_resample(norm_args(pf), ra, ls);
  HIPCHK(hipGetLastError());
  HIPCHK(pf->ro_ev.record(ls));
  HIPCHK(hipStreamSynchronize(ls));
  pf->ro_ev_ok = true;
  if (pf->seq_pin) pf->ro_seq = pf->seq_min();   // (synchronised: nothing to wait for)
  pf->initialised = true;
  pf->own_valid = false;               // no ancestors yet: identity ownership
  pf->rows_st = pf->rows_ll = nullptr;
  pf->switched = pf->propagated = pf->dyn_done = pf->ll_pending = pf->gemm_ahead = false;
  pf->pv_clear();                      // no frame weighed on this cloud yet
  return sm_clear(pf, ls);             // smoothing: this cloud is the history's root
}

// Restore an exported state (gpmdm_pf.py:78-82, 100-104): particles, ancestors, ll and the
// weights, then the read-outs of that state from the restored values themselves -- the
// identity resampling pass reads ll, max(ll) and e / total, so with e = w and total = 1 it
// reads w as the exporter's read-out read e / S (export's w is that same division), and
// the read-outs equal the exporter's bit for bit.  The next frame's normalisation
// recomputes e and the total from its own ll (weights are not recursive, gpmdm_pf.py:198).
int gpmdm_pf_import(gpmdm_pf_t pf, const double* states, const int64_t* classes, const double* ll,
                    const double* log_w, const double* w, const int64_t* ridx, int64_t frame) {
  CHECK(pf && states && classes && ll && log_w && w, "null argument");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  TRY(drop_preswitch(pf, nullptr, true));
  if (pf->switched || pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "import between switch and resample");
  TRY(quiesce(pf));                    // the filter's own frames, not the device
  CHECK(frame < (1ll << 32), "frame out of range");
  const long long P = pf->P, Pf = pf->Pf;
  const int F = pf->F;
  std::vector<int> c32(P), r32(P);
  for (long long i = 0; i < P; ++i) {
    CHECK(classes[i] >= 0 && classes[i] < m->C, "class id out of range");
    c32[i] = (int)classes[i];
    if (ridx) CHECK(ridx[i] >= 0 && ridx[i] < Pf, "resample index out of range");
    r32[i] = ridx ? (int)ridx[i] : (int)(i % Pf);
  }
  // max(ll) per filter as k_norm_max takes it (fmax: NaN ignored), and log_w = ll - max
  std::vector<unsigned long long> gm(F);
  for (int f = 0; f < F; ++f) {
    double M = -INFINITY;
    for (long long i = f * Pf; i < (f + 1) * Pf; ++i) M = std::fmax(M, ll[i]);
    for (long long i = f * Pf; i < (f + 1) * Pf; ++i) {
      const double lw = ll[i] - M;
      CHECK(std::memcmp(&lw, &log_w[i], sizeof(double)) == 0 || (std::isnan(lw) && std::isnan(log_w[i])),
            "log_w is not ll - max(ll) of its filter");
    }
    gm[f] = host_ord_enc(M);
  }
  const std::vector<double> ones(F, 1.0);
  hipStream_t ls = life_stream(m->device);   // uploads and read-outs on the lifecycle stream
  CHECK(ls, "the library's lifecycle stream");
  HIPCHK(hipMemcpyAsync(pf->X, states, sizeof(double) * P * m->d, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->cls, c32.data(), sizeof(int) * P, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->ridx, r32.data(), sizeof(int) * P, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->ll, ll, sizeof(double) * P, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->e, w, sizeof(double) * P, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->total, ones.data(), sizeof(double) * F, hipMemcpyHostToDevice, ls));
  HIPCHK(hipMemcpyAsync(pf->gmax, gm.data(), sizeof(unsigned long long) * F, hipMemcpyHostToDevice, ls));
  if (pf->cls_pin) {
    std::memcpy(pf->cls_pin, c32.data(), sizeof(int) * P);
    pf->cls_host_ok = true;
    pf->cls_ev_pending = false;
  }
  pf->bmax_ready = false;
  pf->ll_pending = false;
  pf->cnt_check = false;
  if (frame >= 0) pf->frame = (unsigned)frame;
  ResampleArgs ra = resample_args(pf);
  ra.identity = 1;
  ra.cls_src = pf->cls;
  ra.X_src = pf->X;
  launch_resample(ra, ls);
  HIPCHK(hipGetLastError());
  // the next frame's shards: the identity order (the exporter's uniforms are not part of the
  // state; the ownership order changes which rank evaluates a particle, never its values)
  pf->own_valid = false;
  pf->rows_st = pf->rows_ll = nullptr;
  HIPCHK(pf->ro_ev.record(ls));
  HIPCHK(hipStreamSynchronize(ls));
  pf->ro_ev_ok = true;
  if (pf->seq_pin) pf->ro_seq = pf->seq_min();   // (synchronised: nothing to wait for)
  pf->initialised = true;
  pf->switched = pf->propagated = pf->dyn_done = pf->gemm_ahead = false;
  pf->pv_clear();                      // the exporter's vc is not part of the state
  return sm_clear(pf, ls);             // smoothing: the imported cloud is the history's root
}

int gpmdm_pf_export(gpmdm_pf_t pf, double* states, int64_t* classes, double* ll, double* log_w,
                    double* w, int64_t* ridx, void* stream) {
  CHECK(pf, "null handle");
  const gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  TRY(flush_ll(pf, s));
  TRY(flush_rows(pf, s));
  // the copies in the caller's stream order, one wait at the end (not the null stream's)
  const long long P = pf->P;
  std::vector<int> tc(classes ? P : 0), tr(ridx ? P : 0);
  std::vector<double> l(P);
  std::vector<unsigned long long> gm(pf->F);
  std::vector<double> S(pf->F);
  if (states) HIPCHK(hipMemcpyAsync(states, pf->X, sizeof(double) * P * m->d, hipMemcpyDeviceToHost, s));
  if (classes) HIPCHK(hipMemcpyAsync(tc.data(), pf->cls, sizeof(int) * P, hipMemcpyDeviceToHost, s));
  if (ridx) HIPCHK(hipMemcpyAsync(tr.data(), pf->ridx, sizeof(int) * P, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(l.data(), pf->ll, sizeof(double) * P, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(gm.data(), pf->gmax, sizeof(unsigned long long) * pf->F, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(S.data(), pf->total, sizeof(double) * pf->F, hipMemcpyDeviceToHost, s));
  if (w) HIPCHK(hipMemcpyAsync(w, pf->e, sizeof(double) * P, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (long long i = 0; i < (classes ? P : 0); ++i) classes[i] = tc[i];
  for (long long i = 0; i < (ridx ? P : 0); ++i) ridx[i] = tr[i];
  if (ll) std::memcpy(ll, l.data(), sizeof(double) * P);
  for (int f = 0; f < pf->F; ++f) {
    const double M = host_ord_dec(gm[f]);
    for (long long i = f * pf->Pf; i < (f + 1) * pf->Pf; ++i) {
      if (log_w) log_w[i] = l[i] - M;
      if (w) w[i] /= S[f];
    }
  }
  return GPMDM_OK;
}

int gpmdm_pf_set_dedup(gpmdm_pf_t pf, int enable) {
  CHECK(pf, "null handle");
  TRY(drop_preswitch(pf, nullptr, true));
  if (pf->switched || pf->dyn_done) return fail(GPMDM_E_STATE, "set_dedup between switch and propagate");
  pf->dedup = enable != 0;
  return GPMDM_OK;
}

int gpmdm_pf_set_dyn_tiles(gpmdm_pf_t pf, int mode) {
  CHECK(pf, "null handle");
  CHECK(mode == GPMDM_DYN_TILES_AUTO || mode == GPMDM_DYN_TILES_NARROW || mode == GPMDM_DYN_TILES_WIDE,
        "mode must be GPMDM_DYN_TILES_*");
  TRY(drop_preswitch(pf, nullptr, true));
  if (pf->switched || pf->dyn_done) return fail(GPMDM_E_STATE, "set_dyn_tiles between switch and propagate");
  pf->dyn_tiles = mode;
  return GPMDM_OK;
}

int gpmdm_pf_set_shard_order(gpmdm_pf_t pf, int enable) {
  CHECK(pf, "null handle");
  TRY(drop_preswitch(pf, nullptr, true));
  if (pf->switched || pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "set_shard_order inside a step");
  pf->shard_order = enable != 0;
  if (!pf->shard_order) pf->own_valid = false;
  return GPMDM_OK;
}

int gpmdm_pf_dyn_rows(gpmdm_pf_t pf, int64_t* rows, void* stream) {
  CHECK(pf && rows, "null argument");
  HIPCHK(hipSetDevice(pf->m->device));
  hipStream_t s = (hipStream_t)stream;
  int r = 0;                           // k_dyn_finish's count of the last pass's rows
  HIPCHK(hipMemcpyAsync(&r, pf->rows_last(), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *rows = r;
  return GPMDM_OK;
}

int gpmdm_pf_enable_timing(gpmdm_pf_t pf, int enable) {
  CHECK(pf, "null handle");
  pf->timing = enable != 0;
  return GPMDM_OK;
}

int gpmdm_pf_timing_stages(gpmdm_pf_t pf, unsigned mask) {
  CHECK(pf, "null handle");
  pf->timing_mask = mask & ((1u << GPMDM_N_STAGES) - 1);
  return GPMDM_OK;
}

int gpmdm_pf_stage_times(gpmdm_pf_t pf, double* ms, int64_t* launches) {
  CHECK(pf, "null handle");
  HIPCHK(hipSetDevice(pf->m->device));
  double acc[GPMDM_N_STAGES] = {0};
  int64_t n[GPMDM_N_STAGES] = {0};
  for (auto& r : pf->recs) {
    HIPCHK(hipEventSynchronize(r.b));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, r.a, r.b));
    acc[r.stage] += t;
    n[r.stage] += 1;
    pf->pool.push_back(r.a);
    pf->pool.push_back(r.b);
  }
  pf->recs.clear();
  if (ms) std::memcpy(ms, acc, sizeof(acc));
  if (launches) std::memcpy(launches, n, sizeof(n));
  return GPMDM_OK;
}

int gpmdm_pf_frame(gpmdm_pf_t pf, int64_t* frame) {
  CHECK(pf && frame, "null argument");
  *frame = pf->frame;
  return GPMDM_OK;
}

int gpmdm_pf_set_model(gpmdm_pf_t pf, gpmdm_model_t m) {
  CHECK(pf && m, "null argument");
  TRY(drop_preswitch(pf, nullptr, true));
  if (pf->switched || pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "set_model inside a step");
  gpmdm_model* old = pf->m;
  if (m == old) return GPMDM_OK;
  CHECK(m->C == old->C && m->d == old->d && m->D == old->D,
        "the new model's (C, d, D) differ from the filter's");
  CHECK(m->device == old->device, "the new model lives on another device");
  HIPCHK(hipSetDevice(m->device));
  // buffers shaped by the model's column blocks
  const int maxparts = m->dyn_parts_max();
  const long long nl = std::max(pf->nloc, 1ll);
  DevBuf<double> qdyn, qobs, sobs;     // (released on every failure below)
  TRY(qdyn.alloc((size_t)maxparts * nl));
  TRY(qobs.alloc((size_t)obs_parts_max(m) * nl));
  TRY(sobs.alloc((size_t)obs_blocks_max(m) * nl));
  TileGeo og{};
  const GpImage* oimg = &obs_pick(m, pf->Pf, pf->nloc, og);
  // the filter's own launches in flight may still read the old buffers and obs_tab: wait for
  // them (not for the device), then release the old buffers in the lifecycle stream's order
  TRY(quiesce(pf));
  const int tab[5] = {(int)pf->lo, (int)pf->hi, 0, 0, (int)cdiv(pf->nloc, og.pt())};
  hipStream_t ls = life_stream(m->device);
  if (!ls || hipMemcpyAsync(pf->obs_tab, tab, sizeof(tab), hipMemcpyHostToDevice, ls) != hipSuccess ||
      hipStreamSynchronize(ls) != hipSuccess)
    return fail(GPMDM_E_HIP, "upload of the observation tile table");
  pf->qdyn = std::move(qdyn);
  pf->qobs = std::move(qobs);
  pf->sobs = std::move(sobs);
  pf->pred_q.release();
  pf->fc_q.release();                  // (the forecast's tile partials: as predict's)
  pf->nparts_dyn_max = maxparts;
  pf->obs_geo = og;
  pf->obs_img = oimg;
  m->refs.fetch_add(1);
  old->remove_user(pf);
  m->add_user(pf);
  pf->m = m;
  model_release(old);
  if (pf->masked()) {                  // the mask's lambda^2 and scalars are the new model's
    const std::vector<unsigned char> mask = pf->obs_mask;
    TRY(install_obs_mask(pf, mask));
  }
  pf->pv_clear();                      // the kept vc was the old model's
  TRY(gate_rebind(pf));                // the gate's log il2 table is the new model's
  return sm_clear(pf, ls);             // smoothing: older frames were the old model's
}

int gpmdm_pf_set_obs_cutoff(gpmdm_pf_t pf, int mode) {
  CHECK(pf, "null handle");
  CHECK(mode >= 0 && mode <= 3, "mode: 0 off, 1 on, 2 on with skip statistics, 3 auto");
  if (pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "set_obs_cutoff between propagate and resample");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  if (mode && !m->has_cutoff()) return fail(GPMDM_E_STATE, "the model has no cutoff image (gpmdm_model_set_obs_cutoff)");
  if (mode && !pf->own && pf->rng_mode == GPMDM_RNG_PHILOX && pf->F == 1 && uniform_order_supported(pf->P)) {
    // the ownership order for single-rank filters (order_wanted): resampling-ancestor ranges
    // of particles evaluated together, so the cutoff's particle tiles are compact
    TRY(alloc_order(pf));
  }
  if (!mode && pf->n_ranks == 1) pf->own_valid = false;   // (the order is the cutoff's only)
  if (mode == 2 && !pf->sp_stats) {
    TRY(pf->sp_stats.alloc(2));
    HIPCHK(hipMemset(pf->sp_stats, 0, 2 * sizeof(unsigned long long)));
  }
  if ((mode == 1 || mode == 3) && !pf->cut_auto_dev) {
    TRY(pf->cut_auto_dev.alloc(2));
    HIPCHK(hipMemset(pf->cut_auto_dev, 0, 2 * sizeof(unsigned long long)));
    TRY(pf->cut_auto_host.alloc_mapped(2));
  }
  pf->obs_cutoff = mode != 0;
  pf->sp_stats_on = mode == 2;
  pf->cut_auto = mode == 3;
  pf->cut_auto_pending = false;        // (a fresh measurement: the next frame probes)
  pf->cut_auto_frac = -1.0;
  return GPMDM_OK;
}

int gpmdm_pf_set_obs_mask(gpmdm_pf_t pf, const uint8_t* observed) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "a filter bank takes one mask per filter, F x D flags (gpmdm_bank_set_obs_masks)");
  return gpmdm_bank_set_obs_masks(pf, observed);
}

int gpmdm_bank_set_obs_masks(gpmdm_pf_t pf, const uint8_t* observed) {
  CHECK(pf, "null handle");
  if (pf->mid_step()) return fail(GPMDM_E_STATE, "set_obs_mask between switch and resample");
  gpmdm_model* m = pf->m;
  const size_t n = (size_t)m->D * pf->F;
  if (!observed) {
    pf->obs_mask.clear();              // (lam2_obs is kept for the next mask)
    return GPMDM_OK;
  }
  HIPCHK(hipSetDevice(m->device));
  std::vector<unsigned char> mask(n);
  for (size_t j = 0; j < n; ++j) mask[j] = observed[j] ? 1 : 0;
  return install_obs_mask(pf, mask);
}

int gpmdm_pf_observation(gpmdm_pf_t pf, double* mean, double* spread, void* stream) {
  CHECK(pf, "null handle");
  CHECK(pf->F == 1, "the filtered-pose read-out serves single filters, not banks (gpmdm_bank_observation)");
  return gpmdm_bank_observation(pf, mean, spread, stream);
}

int gpmdm_bank_observation(gpmdm_pf_t pf, double* mean, double* spread, void* stream) {
  CHECK(pf, "null handle");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D, F = pf->F;
  TRY(pf->ro_part.grow(readout_part_doubles(pf->Pf, D, F), s));
  TRY(pf->ro_obs.reserve((size_t)2 * D * F, s));
  // the particles the filter holds now (X: written by the resample only; a pending pre-switch
  // reads it too and stays pending)
  launch_obs_readout(pose_readout(pf, pf->X, pf->ro_part, pf->ro_obs.dev), s);
  HIPCHK(hipGetLastError());
  if (!mean && !spread) return pf->ro_obs.leave_pending(s);   // launched only (timing)
  auto copy = [&]() -> int {
    HIPCHK(hipMemcpyAsync(pf->ro_obs.pin, pf->ro_obs.dev, sizeof(double) * 2 * D * F, hipMemcpyDeviceToHost, s));
    return GPMDM_OK;
  };
  TRY(pf->ro_obs.finish(copy(), s));
  for (int f = 0; f < F; ++f) {        // device rows are {mean[D], spread[D]} per filter
    const double* row = pf->ro_obs.pin + (size_t)f * 2 * D;
    if (mean) std::memcpy(mean + (size_t)f * D, row, sizeof(double) * D);
    if (spread) std::memcpy(spread + (size_t)f * D, row + D, sizeof(double) * D);
  }
  return GPMDM_OK;
}

int gpmdm_pf_set_obs_skip(gpmdm_pf_t pf, int on) {
  CHECK(pf, "null handle");
  if (pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "set_obs_skip between propagate and resample");
  pf->obs_skip = on != 0;
  return GPMDM_OK;
}

int gpmdm_pf_obs_cutoff_auto(gpmdm_pf_t pf, int* last_cut, double* fraction) {
  CHECK(pf, "null handle");
  HIPCHK(pf->cut_auto_collect());
  if (last_cut) *last_cut = pf->cut_frame ? 1 : 0;
  if (fraction) *fraction = pf->cut_auto_frac;
  return GPMDM_OK;
}

int gpmdm_pf_set_obs_cutoff_split(gpmdm_pf_t pf, int policy) {
  CHECK(pf, "null handle");
  CHECK(policy == GPMDM_CUT_SPLIT_AUTO || policy == GPMDM_CUT_SPLIT_NONE || policy == GPMDM_CUT_SPLIT_ALL ||
            policy == GPMDM_CUT_SPLIT_TAIL || policy == GPMDM_CUT_SPLIT_CHUNKS,
        "policy: GPMDM_CUT_SPLIT_AUTO, _NONE, _ALL, _TAIL or _CHUNKS");
  if (pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "set_obs_cutoff_split between propagate and resample");
  pf->cut_split_policy = policy;
  return GPMDM_OK;
}

int gpmdm_pf_obs_cutoff_stats(gpmdm_pf_t pf, int64_t* run, int64_t* dense, int reset, void* stream) {
  CHECK(pf && run && dense, "null argument");
  *run = *dense = 0;
  if (!pf->sp_stats) return GPMDM_OK;
  HIPCHK(hipSetDevice(pf->m->device));
  hipStream_t s = (hipStream_t)stream;
  unsigned long long h[2];
  HIPCHK(hipMemcpyAsync(h, pf->sp_stats, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *run = (int64_t)h[0];
  *dense = (int64_t)h[1];
  if (reset) HIPCHK(hipMemsetAsync(pf->sp_stats, 0, sizeof(h), s));
  return GPMDM_OK;
}

int gpmdm_pf_health(gpmdm_pf_t pf, int64_t* counts, int reset, void* stream) {
  CHECK(pf, "null handle");
  HIPCHK(hipSetDevice(pf->m->device));
  hipStream_t s = (hipStream_t)stream;
  TRY(flush_ll(pf, s));
  unsigned h[kHealthN];
  HIPCHK(hipMemcpyAsync(h, pf->health, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (counts)
    for (int k = 0; k < kHealthN; ++k) counts[k] = h[k];
  if (reset) HIPCHK(hipMemsetAsync(pf->health, 0, sizeof(h), s));
  return GPMDM_OK;
}

int gpmdm_pf_predict(gpmdm_pf_t pf, double* mean, void* stream) {
  CHECK(pf && mean, "null argument");
  if (!pf->initialised) return fail(GPMDM_E_STATE, "particle filter not initialised");
  HIPCHK(hipSetDevice(pf->m->device));
  TRY(drop_preswitch(pf, (hipStream_t)stream, false));   // predict rewrites the grouping scratch
  if (pf->switched || pf->dyn_done || pf->propagated) return fail(GPMDM_E_STATE, "predict inside a step");
  gpmdm_model* m = pf->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  const int C = m->C, d = m->d;
  const long long P = pf->P;
  TRY(pf->pred_q.grow((size_t)pf->nparts_dyn_max * P, s));
  TRY(pf->pred_mu.grow((size_t)P * d, s));
  TRY(pf->pred_mu_p.grow((size_t)P * d, s));
  TRY(pf->pred_out.grow((size_t)pf->F * d, s));
  // group the current particles by their current class (perm / block tables are the
  // switch's scratch, rebuilt by the next switch; the class tables are predict's own)
  const ClassTables tb = pf->tables(gpmdm_pf::kPredictTables);
  const std::vector<GpImage>& dset = m->dyn_set(true);
  launch_class_hist(pf->cls, P, C, pf->blockcounts, s);
  ScanArgs sc{};
  GroupArgs ga{};
  fill_grouping(sc, ga, tb, pf->blockcounts, pf->blockoff, pf->perm, pf->cls, P, C, dset[0].geo.pt());
  launch_scan_counts(sc, s);
  launch_group(ga, s);
  // each class's dynamics-GP mean (gpmdm.py:1032-1068), rows in grouped order
  launch_dyn_tiles(m, dset, dset[0].geo, tb.seg(), pf->perm, pf->X, P, pf->pred_q, P, pf->pred_mu, s);
  launch_predict_mean(pf->perm, pf->pred_mu, pf->pred_mu_p, pf->pred_out, P, pf->Pf, pf->F, d, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(pf->rpin, pf->pred_out, sizeof(double) * pf->F * d, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(mean, pf->rpin, sizeof(double) * pf->F * d);
  return GPMDM_OK;
}

}  // extern "C"
