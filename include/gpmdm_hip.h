/*
 * gpmdm_hip.h -- C ABI of libgpmdm_hip.so, the MI355X (gfx950) engine for the GPMDM
 * particle-filter inference step.
 *
 * The reference (Priyanshu4/gpmdm) is pure Python: its "boundary" is the class API of
 * gpmdm/gpmdm_pf.py (GPMDM_PF) and the two predictive maps of gpmdm/gpmdm.py it calls.
 * There is no FFI in the reference; each entry point below names the reference call it
 * replaces (file:line under /root/reference).  The Python mirror of the reference API
 * (gpmdm_amd.GPMDM / gpmdm_amd.GPMDM_PF) binds these through ctypes; INTEGRATION.md
 * shows the binding.
 *
 * Conventions
 *   - every function returns int: 0 = ok, < 0 = error (see GPMDM_E_*); the message of
 *     the last error on the calling thread is gpmdm_last_error();
 *   - all floating point is IEEE fp64, row-major, contiguous; class ids are int64 at the
 *     boundary (int32 on the device);
 *   - "host" pointers are ordinary CPU memory; "device" pointers are HIP device memory
 *     owned by the caller (e.g. torch tensors' data_ptr());
 *   - host input arrays are read before the call returns (the library stages them in its
 *     own pinned buffers), so the caller may reuse or free them at once; host output
 *     arrays are complete when the call returns (the call synchronises the stream);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  A handle keeps
 *     no stream of its own: launches go to the stream given to each call;
 *   - a handle is not thread-safe; distinct handles are independent.
 */
#ifndef GPMDM_HIP_H
#define GPMDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMDM_OK 0
#define GPMDM_E_INVALID (-1)   /* bad argument / shape (reference raises ValueError) */
#define GPMDM_E_HIP (-2)       /* HIP runtime failure */
#define GPMDM_E_NOMEM (-3)     /* device allocation failed */
#define GPMDM_E_STATE (-4)     /* call out of order (e.g. step before init) */

#define GPMDM_RNG_REPLAY 0     /* draws supplied by the caller (torch-order replay) */
#define GPMDM_RNG_PHILOX 1     /* draws generated on the device (Philox4x32-10) */

#define GPMDM_RESAMPLE_MULTINOMIAL 0  /* torch.multinomial(w, P, True): inverse CDF (reference) */
#define GPMDM_RESAMPLE_SYSTEMATIC 1   /* systematic resampling: one uniform per step, slot s takes
                                         the first i with cum_i >= (s + u0) / P; computed by a
                                         scan over the slots (run starts + max-scan), no search */

typedef struct gpmdm_model* gpmdm_model_t;
typedef struct gpmdm_pf* gpmdm_pf_t;

/*
 * Model descriptor: everything the per-frame path reads, precomputed on the host the
 * way gpmdm.py:1284-1305 (_precompute_kernel_inverses) does, restricted to class blocks.
 * The library copies every array to the device; the caller may free them on return.
 *
 *   obs_R      N x N   upper-triangular U_y^-1 with K_y = U_y^T U_y, so K_y^-1 = R R^T
 *                      (gpmdm.py:1286-1289)
 *   obs_beta   N x D   K_y^-1 Y  (the mean weights of map_x_to_y, gpmdm.py:957)
 *   dyn_R[c]   Nc x Nc upper-triangular U_c^-1 of the class-c block of K_x (gpmdm.py:1299-1305)
 *   dyn_alpha[c] Nc x d  A_c Xout_c  (mean weights of map_x_dynamics_for_class, gpmdm.py:1064)
 */
/* GP-tile workgroup shapes (particles x columns of K* B per workgroup).  The default runs
 * the observation GP as 32x512 (d <= 12) or 64x512 (d > 12) and the dynamics GPs as
 * 16x256; an explicit 64x256 or 64x512 applies to both. */
enum {
  GPMDM_TILE_DEFAULT = 0,
  GPMDM_TILE_64x256 = 1,
  GPMDM_TILE_64x512 = 2,
  GPMDM_TILE_32x512 = 3
};

typedef struct gpmdm_model_desc {
  int64_t N;                     /* training latents (rows of X, Y) */
  int32_t D;                     /* observation dimension */
  int32_t d;                     /* latent dimension (<= 32) */
  int32_t C;                     /* classes */
  int32_t tile_shape;            /* GPMDM_TILE_*: GP-tile workgroup shape (0 = default) */
  const double* X;               /* N x d latents (particle initialisation is host-side) */
  const double* obs_R;           /* N x N */
  const double* obs_beta;        /* N x D */
  const double* y_lengthscales;  /* d  : exp(y_log_lengthscales) */
  const double* y_inv_lambda2;   /* D  : exp(y_log_lambdas)^-2 */
  const int64_t* Nc;             /* C  : dynamics rows per class */
  const double* const* Xin;      /* C pointers, Nc x d : dynamics inputs of class c */
  const double* const* dyn_R;    /* C pointers, Nc x Nc */
  const double* const* dyn_alpha;/* C pointers, Nc x d */
  const double* x_lengthscales;  /* d   : exp(x_log_lengthscales) */
  const double* x_lin_coeff2;    /* d+1 : exp(x_log_lin_coeff)^2 (bias last) */
  const double* x_inv_lambda2;   /* d   : exp(x_log_lambdas)^-2 */
} gpmdm_model_desc;

/* Upload a model (replaces the device-side state GPMDM holds after GPMDM.load /
 * init_X + _precompute_kernel_inverses, gpmdm.py:762-777, 1349-1414). */
int gpmdm_model_create(const gpmdm_model_desc* desc, int device, gpmdm_model_t* out);
int gpmdm_model_destroy(gpmdm_model_t model);

/* GPMDM.map_x_to_y(Xstar, flg_noise=False)  (gpmdm.py:923-963).
 * Xs_dev: n x d; mu_dev, var_dev: n x D (device, caller-owned). */
int gpmdm_predict_obs(gpmdm_model_t model, const double* Xs_dev, int64_t n,
                      double* mu_dev, double* var_dev, void* stream);

/* GPMDM.map_x_dynamics_for_class(Xstar, c, flg_noise=False)  (gpmdm.py:1032-1068).
 * Xs_dev: n x d; mu_dev, var_dev: n x d (device, caller-owned). */
int gpmdm_predict_dyn(gpmdm_model_t model, int c, const double* Xs_dev, int64_t n,
                      double* mu_dev, double* var_dev, void* stream);

/* GPMDM_PF(gpmdm, markov_switching_model, num_particles)  (gpmdm_pf.py:47-85).
 * T: C x C host.  Ranks own the contiguous particle range
 * [rank*P/n_ranks, (rank+1)*P/n_ranks); particle state is replicated on every rank.
 * The per-frame exchange is done either by the library over an RCCL communicator
 * (gpmdm_pf_set_comm; then gpmdm_pf_propagate / gpmdm_pf_step exchange by themselves) or
 * by the caller with the staged calls (gpmdm_pf_pack / gpmdm_pf_unpack). */
int gpmdm_pf_create(gpmdm_model_t model, const double* T, int64_t P, int rng_mode,
                    uint64_t seed, int resample_mode, int n_ranks, int rank,
                    gpmdm_pf_t* out);
int gpmdm_pf_destroy(gpmdm_pf_t pf);

/* Filter bank: n_filters independent filters of P particles each sharing one model (the
 * 39 trials test_gpmdm_pf.ipynb runs one after another).  Device
 * (philox) draws, one rank.  Filter f draws exactly what a single filter created with
 * seed + f draws, so its results are bit-identical to that filter's.  The handle works
 * with every gpmdm_pf_* call below, with per-filter arrays stacked filter-major:
 * states/classes (F*P) in init/export, z (F x D) in propagate, F x C / F x d / F in read.
 * gpmdm_pf_shape reports (F, P) of any handle (F = 1 for gpmdm_pf_create). */
int gpmdm_bank_create(gpmdm_model_t model, const double* T, int64_t n_filters, int64_t P,
                      uint64_t seed, int resample_mode, gpmdm_pf_t* out);
int gpmdm_pf_shape(gpmdm_pf_t pf, int64_t* n_filters, int64_t* P);

/* _init_particles / reset()  (gpmdm_pf.py:87-115, 264-265): states P x d, classes P
 * (host).  Clears weights to 1/P and log-likelihoods to 0 as the reference does. */
int gpmdm_pf_init(gpmdm_pf_t pf, const double* states, const int64_t* classes);

/* Restore a filter state exported by gpmdm_pf_export (checkpoint / resume):
 * the reference filter's state _particle_states, _particle_classes, _log_likelihoods,
 * _log_weights, _weights (gpmdm_pf.py:78-82, 100-104), all host.  states P x d, classes P,
 * ll P, log_w P, w P (all required); ridx P (the last resample's ancestor indices within each
 * filter, or NULL: none shared); frame >= 0 sets the Philox frame counter (< 0 keeps it).
 * log_w must be ll - max(ll) per filter, computed as gpmdm_pf_export computes it (exact
 * comparison; GPMDM_E_INVALID otherwise).  The read-outs right after the import equal the
 * exporter's (posterior, mean, likelihood sum, bit for bit), and a filter of the same
 * configuration and seed continues the exporter's trajectory bit for bit.  A replay
 * filter's draws come from the caller's generator: saving its state is the caller's part.
 * Drops a pending pre-switch; not between switch and resample. */
int gpmdm_pf_import(gpmdm_pf_t pf, const double* states, const int64_t* classes, const double* ll,
                    const double* log_w, const double* w, const int64_t* ridx, int64_t frame);

/* Replay filters: the library's own pinned staging buffers of the three draw streams
 * (exp draws P x C, normals P x d, uniforms P), so a host can draw straight into them.
 * Passing these very pointers to gpmdm_pf_switch / gpmdm_pf_propagate / gpmdm_pf_resample
 * skips the copy into staging.  A buffer may be written only when gpmdm_pf_draws_free
 * (which = 0, 1, 2) has returned: it waits until the launches that read the buffer's last
 * contents have run (a pending replay pre-switch included).  It may be called from another
 * thread than the one stepping the filter (a host drawing ahead) when the buffer is copied
 * to the device (a buffer of more than 32 KB); for smaller, in-place buffers call it
 * from the stepping thread (it reads the pre-switch's bookkeeping). */
int gpmdm_pf_draw_buffers(gpmdm_pf_t pf, double** exp_draws, double** normals, double** uniforms);
int gpmdm_pf_draws_free(gpmdm_pf_t pf, int which);

/* _propogate_markov_switching  (gpmdm_pf.py:137-151).  exp_draws: P x C host (replay)
 * or NULL (philox).  class_counts: C host, or NULL; when given, the post-switch class
 * counts are returned (the replay caller needs them to draw the per-class normals of the
 * next stage): a single replay filter of <= 1024 particles counts them on the host from
 * exp_draws and the classes its last resample left in mapped memory (no stream wait; the
 * device's counts are checked at the next switch), others copy them back synchronously.
 * Philox filters: gpmdm_pf_resample already launched the next frame's switch behind its
 * read-out (its draws need no host input), and this call then only consumes it (the
 * caller's stream waits on it if it is another stream); the call order is still required.
 * A replay filter consumes a pending gpmdm_pf_preswitch when exp_draws is the pointer the
 * pre-switch was given (its counts come from mapped memory once the switch kernels are
 * done, not after the dynamics tiles behind them); another pointer drops it and switches. */
int gpmdm_pf_switch(gpmdm_pf_t pf, const double* exp_draws, int64_t* class_counts,
                    void* stream);

/* The next frame's switch launched now, between frames -- behind the last read-out, while
 * the host is still busy -- instead of in gpmdm_pf_switch.  Replay filters: exp_draws is the
 * next frame's P x C Exp(1) draws (a host draws them ahead: they depend on no device
 * result); the switch, its class counts (into mapped memory) and the dynamics-GP tiles are
 * launched on `stream`, and the next gpmdm_pf_switch with the same exp_draws pointer
 * consumes them.  The caller promises that the array's contents do not change in between;
 * if they do (its generator moved), it calls gpmdm_pf_preswitch again, which drops the
 * earlier pre-switch.  Philox filters: what gpmdm_pf_resample already does (no-op if
 * pending).  Any call that drops a pre-switch (import, predict, set_*) drops this one: the
 * next gpmdm_pf_switch then switches from scratch.  Not inside a step. */
int gpmdm_pf_preswitch(gpmdm_pf_t pf, const double* exp_draws, void* stream);

/* Replay filters: copy values [begin, end) of the next propagate's normals ((sum_c P_c) x d,
 * flattened) to the device now, on `stream` (the propagate must run on the same stream).
 * The next gpmdm_pf_propagate(_dynamics) handed the same `normals` pointer copies nothing if
 * the ranges staged since the last propagate cover every value, else all of them.  A host
 * that knows part of the normals early (the first class's, drawn ahead) stages that part
 * behind the read-out and the rest once drawn; values changed after staging must be staged
 * again.  Small filters (<= 32 KB of normals, read in place) ignore it. */
int gpmdm_pf_stage_normals(gpmdm_pf_t pf, const double* normals, int64_t begin, int64_t end, void* stream);

/* _propogate_dynamics + _update_weights' likelihoods for this rank's particles
 * (gpmdm_pf.py:153-192).  z: D host.  normals: (sum_c P_c) x d host in the reference's
 * per-class order (replay) or NULL (philox).  A single-shard filter of <= 1024 particles
 * per filter leaves the last step of the likelihoods (the per-particle finish) to the
 * next gpmdm_pf_resample launch; gpmdm_pf_export, gpmdm_pf_pack(_part) and
 * gpmdm_pf_health run it first if it is still pending, so every reader sees the same ll.
 * The host arrays (draws, z) are copied before the call returns; small ones are read by
 * the kernels from the library's mapped pinned buffers instead of a copy launch. */
int gpmdm_pf_propagate(gpmdm_pf_t pf, const double* z, const double* normals, void* stream);

/* gpmdm_pf_propagate in two halves, so a multi-rank caller can exchange the new states
 * while the observation GP runs: propagate_dynamics = _propogate_dynamics
 * (gpmdm_pf.py:153-168; normals as for gpmdm_pf_propagate), weigh = _update_weights'
 * likelihoods (gpmdm_pf.py:170-192).  switch -> propagate_dynamics -> weigh -> resample. */
int gpmdm_pf_propagate_dynamics(gpmdm_pf_t pf, const double* normals, void* stream);
int gpmdm_pf_weigh(gpmdm_pf_t pf, const double* z, void* stream);

/* Multi-rank exchange: pack this rank's rows [lo, hi) as (hi-lo) x (d+2) doubles
 * {ll, class, state[d]}; unpack all P rows after an all-gather.  The _part forms move
 * column subsets: GPMDM_PACK_STATES = {class, state[d]} (d+1 wide; valid after
 * propagate_dynamics), GPMDM_PACK_LL = {ll} (1 wide; valid after weigh).
 * Unpacking hands the gathered rows to the filter, which reads them in place during the
 * next gpmdm_pf_resample (its gathers touch only the resampled ancestors' rows; the ll
 * column is read once, with the normaliser's maximum): recv_dev must stay allocated and
 * unmodified until that resample's kernels have run -- stream order on the resample's stream
 * suffices (the next frame's all-gather into the same buffer, enqueued after it, is safe). */
enum { GPMDM_PACK_ALL = 0, GPMDM_PACK_STATES = 1, GPMDM_PACK_LL = 2 };
int gpmdm_pf_exchange_width(gpmdm_pf_t pf, int64_t* width, int64_t* lo, int64_t* hi);
int gpmdm_pf_pack(gpmdm_pf_t pf, double* send_dev, void* stream);
int gpmdm_pf_unpack(gpmdm_pf_t pf, const double* recv_dev, void* stream);
int gpmdm_pf_pack_part(gpmdm_pf_t pf, double* send_dev, int part, void* stream);
int gpmdm_pf_unpack_part(gpmdm_pf_t pf, const double* recv_dev, int part, void* stream);

/* Library-driven exchange over RCCL (SURVEY.md §8(b)'s rccl_comm; it replaces the
 * reference's single-process hand-over from _update_weights to _resample,
 * gpmdm_pf.py:194-213).  rccl_comm: an ncclComm_t of n_ranks ranks in which this process is
 * `rank`, on the model's device (from gpmdm_comm_init or the caller's own
 * ncclCommInitRank); the caller keeps ownership and destroys it after the filter.  While
 * set, gpmdm_pf_propagate (and gpmdm_pf_step) all-gather every rank's new {class, state}
 * rows on a library-owned stream while the observation GP runs on the caller's stream, then
 * the {ll} column; the caller's stream waits for both gathers (events, no host wait) and
 * every rank holds the full replicated filter before gpmdm_pf_resample.  NULL detaches.
 * Also valid with n_ranks = 1 (the exchange then moves this rank's rows only).
 * flags: 0, or GPMDM_COMM_PAD_ROWS -- gather one padding row per rank more than needed,
 * through the uneven-shard path (staging buffer + copy-down; diagnostics and tests).
 * Not between switch and resample; not for filter banks (they shard filters). */
#define GPMDM_COMM_PAD_ROWS 1
#define GPMDM_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */
int gpmdm_pf_set_comm(gpmdm_pf_t pf, void* rccl_comm, int flags);

/* RCCL communicator helpers for native hosts that do not link RCCL themselves: rank 0
 * creates a unique id (GPMDM_COMM_ID_BYTES bytes) and hands it to every rank out of band;
 * each rank calls gpmdm_comm_init on its device (ncclCommInitRank: collective over the
 * ranks); gpmdm_comm_destroy after the filters using it are destroyed. */
int gpmdm_comm_unique_id(void* id);
int gpmdm_comm_init(int n_ranks, int rank, const void* id, int device, void** comm);
int gpmdm_comm_destroy(void* comm);

/* One process driving several devices (GPMDM_PF(devices=[...])): gpmdm_comm_init_all makes
 * the n communicators of devices[0..n-1] at once (ncclCommInitAll), comms[i] for rank i.
 * gpmdm_pf_propagate_multi is gpmdm_pf_propagate for the n filters pfs[i] (rank i of n,
 * each with comms[i] set by gpmdm_pf_set_comm, each switched) on streams[i]: every stage
 * runs for every rank and each stage's all-gathers are grouped (ncclGroupStart/End), as a
 * single thread that drives several ranks must.  z and the replay normals are the same
 * host arrays for every rank (the filter is replicated).  RCCL is resolved at run time
 * (librccl.so.1) by these and the calls above; GPMDM_E_HIP when it is missing. */
int gpmdm_comm_init_all(int n, const int* devices, void** comms);

/* TEST ONLY: n in-process loopback communicators, comms[i] = rank i of n on devices[i]
 * (devices may repeat: R ranks on one GPU, which RCCL refuses).  They stand in for RCCL
 * communicators everywhere above (gpmdm_pf_set_comm, gpmdm_pf_propagate_multi,
 * gpmdm_comm_destroy): each all-gather is R x R stream-ordered device copies made when the
 * last rank joins, with RCCL's completion semantics (no rank's stream passes the collective
 * before every rank's rows have landed).  Ranks joined by one thread inside
 * gpmdm_pf_propagate_multi are grouped; ranks on threads of their own block on the host in
 * each collective until all have joined (an error after 120 s).  Not a transport for
 * production: every byte goes through this process's device copies. */
int gpmdm_comm_init_loopback(int n, const int* devices, void** comms);
int gpmdm_pf_propagate_multi(gpmdm_pf_t* pfs, int n, const double* z, const double* normals,
                             void* const* streams);

/* _update_weights' normalisation + _resample + the read-outs  (gpmdm_pf.py:194-262,
 * 302-312).  uniforms: P host (replay, multinomial), 1 host (replay, systematic) or NULL.
 * Philox filters then launch the next frame's switch on the same stream (see
 * gpmdm_pf_switch); gpmdm_pf_predict, gpmdm_pf_init and the gpmdm_pf_set_* calls drop it,
 * and the next gpmdm_pf_switch launches it again (the same draws, the same result).  The
 * stream must stay valid until that next switch or drop (a call that waits for the
 * pre-switch from another stream or the host records its event on this stream then). */
int gpmdm_pf_resample(gpmdm_pf_t pf, const double* uniforms, void* stream);

/* update(z) in one call  (gpmdm_pf.py:117-135): switch + propagate + resample.
 * One rank, or several with a communicator (gpmdm_pf_set_comm); replay draws must all be
 * given (use the staged calls when the per-class normal counts are not known in advance). */
int gpmdm_pf_step(gpmdm_pf_t pf, const double* z, const double* exp_draws,
                  const double* normals, const double* uniforms, void* stream);

/* class_probabilities() / current_state_mean() / log_likelihood()
 * (gpmdm_pf.py:224-262, 215-222).  Waits for the last read-out -- the read-out kernels write
 * it to mapped host memory and then publish a sequence number there, which this call waits
 * on (GPMDM_RO_EVENT=1: an event recorded after the read-out), so not for a pre-launched
 * switch behind it -- or synchronises `stream` when the read-outs need a copy (banks of more
 * than ~800 filters); any pointer may be NULL. */
int gpmdm_pf_read(gpmdm_pf_t pf, double* posterior, double* mean, double* lik, void* stream);

/* Export the full particle state to host (any pointer may be NULL): states P x d,
 * classes P, ll P, log_w P, w P, resample indices P (of the last resample). */
int gpmdm_pf_export(gpmdm_pf_t pf, double* states, int64_t* classes, double* ll,
                    double* log_w, double* w, int64_t* resample_idx, void* stream);

/* Per-stage device time (HIP events on the launch stream).  enable=1 starts recording,
 * 0 stops.  gpmdm_pf_stage_times synchronises and returns, per stage, the summed
 * milliseconds and the number of launches since the last call (then resets). */
#define GPMDM_STAGE_SWITCH 0
#define GPMDM_STAGE_DYN_GEMM 1
#define GPMDM_STAGE_DYN_FINISH 2
#define GPMDM_STAGE_OBS_GEMM 3
#define GPMDM_STAGE_OBS_FINISH 4
#define GPMDM_STAGE_RESAMPLE 5
#define GPMDM_N_STAGES 6
int gpmdm_pf_enable_timing(gpmdm_pf_t pf, int enable);
/* Which stages record events while timing is on: bit (1 << GPMDM_STAGE_*) per stage,
 * default all.  Each recorded stage adds two event records to the stream. */
int gpmdm_pf_timing_stages(gpmdm_pf_t pf, unsigned mask);
int gpmdm_pf_stage_times(gpmdm_pf_t pf, double* ms, int64_t* launches);

/* Ancestor de-duplication of the dynamics GP (default on).  After a resample, offspring of
 * one ancestor carry bit-identical states; the dynamics GP (gpmdm.py:1032-1068) of a
 * (state, class) pair is evaluated once per distinct (ancestor, new class) key of the
 * rank's slice and shared by its offspring.  Results are bitwise identical either way
 * (per-particle arithmetic does not depend on tile membership); enable=0 evaluates every
 * particle, as the reference does.  Must not be toggled between switch and propagate.
 * gpmdm_pf_dyn_rows synchronises `stream` and returns the rows the last dynamics pass
 * evaluated (distinct keys with de-duplication, the slice size without). */
int gpmdm_pf_set_dedup(gpmdm_pf_t pf, int enable);
int gpmdm_pf_dyn_rows(gpmdm_pf_t pf, int64_t* rows, void* stream);

/* Tile shape of the dynamics-GP pass.  AUTO (default): narrow 16x256 tiles for the few
 * de-duplicated rows (short K loops), the observation GP's wide shape when every particle
 * is evaluated (dedup off: a throughput problem).  NARROW / WIDE force one.  For d <= 12 the
 * two are bitwise identical (the 32x512 wide tile reduces each 256-column half in the 16x256
 * order), and AUTO may run a de-duplicated pass on the wide image when a rank's last read
 * frame had many rows; above d = 12 the 64x512 wide shape differs in floating-point
 * summation order (the de-duplication tests pin one shape).  Not between switch and
 * propagate. */
#define GPMDM_DYN_TILES_AUTO 0
#define GPMDM_DYN_TILES_NARROW 1
#define GPMDM_DYN_TILES_WIDE 2
int gpmdm_pf_set_dyn_tiles(gpmdm_pf_t pf, int mode);

/* Ancestor-ordered shards (multi-rank philox filters; default on).  After each resample the
 * particles are put in a stable order of their resampling uniform's bucket floor(256 u) (the
 * inverse-CDF search is monotone in u, so a bucket descends from a contiguous ancestor range;
 * identical on every rank; systematic resampling: the identity order, already ancestor-
 * ordered) and rank r evaluates positions [lo, hi) of that order instead of particles
 * [lo, hi), so its slice covers a contiguous ancestor range and de-duplication keeps ~1/R of
 * the distinct (ancestor, class) keys.  Pack/unpack rows follow the same order, so the all-gathered
 * filter is bitwise the same either way.  No effect on one rank, replay draws or without
 * de-duplication.  Every rank must make the same call, outside switch..resample. */
int gpmdm_pf_set_shard_order(gpmdm_pf_t pf, int enable);

/* Frames (resamples) this handle has done: the Philox counter of the next step's draws
 * (rng_mode GPMDM_RNG_PHILOX; oracle/philox.py restates the draws). */
int gpmdm_pf_frame(gpmdm_pf_t pf, int64_t* frame);

/* Rebind a filter to another model of the same (C, d, D) on the same device -- the
 * reference filter reads its GPMDM's current state on every call (gpmdm_pf.py:164, 183),
 * so a retrained / re-initialised model (GPMDM.set_latents, train_adam) must reach the
 * filter.  Models are reference counted: a filter keeps the model it was built on (or
 * last rebound to) alive, so gpmdm_model_destroy never leaves a filter dangling.  Not
 * between switch and resample. */
int gpmdm_pf_set_model(gpmdm_pf_t pf, gpmdm_model_t model);

/* Observation-GP kernel-value cutoff (opt-in; DESIGN.md §3 "Kernel-value cutoff").  The
 * observation GP of map_x_to_y / _update_weights (gpmdm.py:923-963, gpmdm_pf.py:170-192) with
 * every kernel value k_i = exp(-|x* - X_i|^2 / l^2) below tau replaced by exactly 0, tau the
 * largest cutoff whose effect provably stays below half an ulp of the smallest possible
 * 1 - k^T K_y^-1 k and below half an ulp of each output dimension's largest training
 * observation in the means; the kernel then skips the 16-row K-steps a particle tile cannot
 * reach.  gpmdm_model_set_obs_cutoff builds the model's cutoff image from
 *   K_inv     N x N row-major, K_y^-1 -- the reference's Ky_inv = U^-1 U^-T (gpmdm.py:1286-1290)
 *   beta      N x D row-major, K_y^-1 Y (the mean weights, gpmdm.py:955-957)
 *   sigma2    the noise variance on K_y's diagonal (exp(y_log_sigma_n)^2 + sigma_n_num_Y^2)
 *   y_absmax  D values, max_i |Y_ij|
 * (K_inv = NULL removes it); gpmdm_model_obs_cutoff returns tau (0: none).  The call waits
 * for the last frame of every filter built on the model, not for the device: none of them
 * may be inside a frame or stepping on another thread meanwhile.  A filter uses it
 * after gpmdm_pf_set_obs_cutoff(pf, 1) (2: also count the MFMA groups run against the dense
 * kernel's, read and optionally reset by gpmdm_pf_obs_cutoff_stats; 0: the dense kernel).
 * Results are the dense filter's to rounding (not bit for bit), and do not depend on the
 * tiling or the shard count.  Limits: d <= 16 and an image below 4 GiB (about 32k training
 * rows); GPMDM_E_INVALID otherwise. */
int gpmdm_model_set_obs_cutoff(gpmdm_model_t model, const double* K_inv, const double* beta, double sigma2,
                               const double* y_absmax);
/* The same image built on the model's device from the model's own observation factor: R and
 * K_y^-1 Y are read back out of the device image, K_y^-1 = R R^T is formed by rocBLAS dsyrk
 * and the image is packed by a device kernel (only tau, the spatial order and the K-step
 * spheres are computed on the host, from X and the column sums of K_y^-1 Y).  Byte-equal to
 * gpmdm_model_set_obs_cutoff's image for the same K_y^-1.  kinv_out (N x N) and m_out (N x D)
 * are optional host copies of the K_y^-1 and K_y^-1 Y it packed (tests).  Like
 * gpmdm_model_set_obs_cutoff: no filter on the model may be inside a frame or stepping on
 * another thread during the call (the filters' last frames are waited for, not the device). */
int gpmdm_model_build_obs_cutoff(gpmdm_model_t model, double sigma2, const double* y_absmax, double* kinv_out,
                                 double* m_out);
/* The cutoff image's doubles (*n = their count; out = NULL: the count only).  Tests. */
int gpmdm_model_obs_cutoff_image(gpmdm_model_t model, int64_t* n, double* out);
int gpmdm_model_obs_cutoff(gpmdm_model_t model, double* tau);
int gpmdm_pf_set_obs_cutoff(gpmdm_pf_t pf, int mode);
/* mode 3 = AUTO: per frame the cutoff kernel while the fraction of the dense MFMA work it ran
 * on its last frame is at most 0.75 (its break-even against the dense kernel), else the
 * dense kernel, with a cutoff frame at least every 8 frames to measure again.  The counts
 * travel with the frame's read-out, so the choice is a function of the filter's own
 * trajectory (deterministic).  Single-rank filters and banks whose read-outs are mapped (up
 * to ~800 filters) with more than 1024 particles per filter; others run mode 1 (a rank-local
 * choice would make a particle's result depend on its rank).  Mode 1 filters of that kind
 * count the same way (for the split policy below).  gpmdm_pf_obs_cutoff_auto: did the last
 * frame run the cutoff, and the last measured fraction (< 0: none yet). */
int gpmdm_pf_obs_cutoff_auto(gpmdm_pf_t pf, int* last_cut, double* fraction);
int gpmdm_pf_obs_cutoff_stats(gpmdm_pf_t pf, int64_t* run, int64_t* dense, int reset, void* stream);
/* Scheduling of the cutoff kernel's particle tiles (results are identical under every
 * policy): a split tile runs as two workgroups.  GPMDM_CUT_SPLIT_AUTO (default): the
 * _CHUNKS grid below when the filter's last measured fraction (modes 1 and 3, above) is at
 * least 0.5; otherwise every tile when the launch is at most two rounds of resident workgroups or its last round holds at
 * most an eighth of a round, none at whole rounds, otherwise the tiles of the last round
 * (measured, DESIGN.md §3 "The grid's tail"); _NONE, _ALL, _TAIL (the last round's tiles);
 * _CHUNKS: every 32-tile chunk of every tile's list its own workgroup, the chunks at the
 * lists' ends first (the dense kernel's heavy-first column blocks, for clouds that reach most
 * K-steps).  Between frames only. */
#define GPMDM_CUT_SPLIT_AUTO 0
#define GPMDM_CUT_SPLIT_NONE 1
#define GPMDM_CUT_SPLIT_ALL 2
#define GPMDM_CUT_SPLIT_TAIL 3
#define GPMDM_CUT_SPLIT_CHUNKS 4
int gpmdm_pf_set_obs_cutoff_split(gpmdm_pf_t pf, int policy);

/* The default (dense) filter's flush and block skip (DESIGN.md §3.4 "Flush and skip in the dense
 * tile").  gpmdm_model_set_obs_flush computes the same tau as the cutoff image's, from the
 * model's own K_y^-1 Y (sigma2, y_absmax: as gpmdm_model_set_obs_cutoff).  From then on the
 * filters' observation likelihood replaces every kernel value below tau by exactly 0, value by
 * value, so a particle's result depends on nothing but its own state; the predictive maps
 * (gpmdm_predict_obs, gpmdm_predict_dyn) never flush.  A model without the call flushes nothing.
 * gpmdm_model_obs_flush returns tau (0: none).  Between frames only.
 * gpmdm_pf_set_obs_skip (default 1): the dense tile branches around the MFMAs of every 16-particle
 * x 4-training-row block of kernel values that is exactly zero (flushed, underflowed or padding).
 * Skipping such a block is bitwise the same as multiplying it; 0 runs every block in the same
 * kernel with the same flush, so one process can hold the two against each other. */
int gpmdm_model_set_obs_flush(gpmdm_model_t model, double sigma2, const double* y_absmax);
int gpmdm_model_obs_flush(gpmdm_model_t model, double* tau);
int gpmdm_pf_set_obs_skip(gpmdm_pf_t pf, int on);

/* Failure detection.  The filter keeps the reference's arithmetic: a
 * non-positive predictive variance gives NaN log-likelihoods / states as it does in
 * gpmdm_pf.py:167-168, 188-192.  Each event is counted on the device (per particle and
 * step) and read here: counts[0] observation-GP variance <= 0, [1] non-finite
 * log-likelihood, [2] dynamics-GP variance <= 0, [3] non-finite propagated state.
 * Synchronises `stream`; reset != 0 zeroes the counters afterwards. */
#define GPMDM_HEALTH_N 4
int gpmdm_pf_health(gpmdm_pf_t pf, int64_t* counts, int reset, void* stream);

/* GPMDM_PF.predict() (BASELINE.json north_star): the one-step dynamics-GP prediction of
 * the latent mean, (1/P) sum_p mu_{c_p}(x_p) with mu_c = map_x_dynamics_for_class's mean
 * (gpmdm.py:1032-1068) over the current particles and classes.  No state change, no draws.
 * mean: F x d host (F = 1 for a single filter).  Synchronises `stream`. */
int gpmdm_pf_predict(gpmdm_pf_t pf, double* mean, void* stream);

/* Masked observations: missing joints.  observed: D bytes (non-zero = this dimension of z is
 * observed) or NULL (all observed, the default).  Holds until changed.  Between frames only
 * (GPMDM_E_STATE inside a step); a pending pre-switch stays pending.  A masked frame computes
 * the reference's likelihood (gpmdm_pf.py:170-192) on the model restricted to the observed
 * dimensions -- the same kernels, with lambda^2 = 0 at the unobserved ones and D, sum log
 * il2 and the float32 constant taken over the observed ones.  z at the unobserved positions
 * is replaced by 0 in the library's staging copy (the caller's array is not written), so a
 * NaN there reaches no kernel.  With no dimension observed the frame is a pure prediction
 * step: no observation kernel runs, ll is exactly 0 and w exactly 1/P.  gpmdm_pf_step,
 * gpmdm_pf_propagate and gpmdm_pf_weigh honour it; every rank of a sharded filter must hold
 * the same mask (gpmdm_pf_propagate_multi: GPMDM_E_INVALID otherwise).  Filter banks:
 * GPMDM_E_INVALID (one mask per filter: gpmdm_bank_set_obs_masks). */
int gpmdm_pf_set_obs_mask(gpmdm_pf_t pf, const uint8_t* observed);

/* One mask per filter of a bank, gpmdm_pf_set_obs_mask's semantics for each: the mask holds
 * until changed, is set between frames only (GPMDM_E_STATE inside a step), leaves a pending
 * pre-switch pending, is re-derived when the handle is rebound to a rebuilt model, and is not
 * carried by export / import.  Filter f's frame computes the reference's likelihood on the
 * model restricted to f's observed dimensions: the device holds lambda^2 as F x D (0 at f's
 * unobserved dimensions) and an F-row table of D_obs, sum log il2 and the float32 constant;
 * the observation tiles read the row of each particle's own filter (a tile may mix filters)
 * and the likelihood finish the table row of the filter that owns the output's particle.
 * Each filter's row of z is zeroed at that filter's unobserved positions in the staging copy.
 * A filter with no dimension observed gets ll exactly 0 and w exactly 1/P and adds nothing to
 * the health counters; when every filter is blacked out no observation kernel runs.  The
 * install waits for the handle's own previous frame only, never for the device.  Any handle:
 * on a single filter (F = 1) this is gpmdm_pf_set_obs_mask. */
int gpmdm_bank_set_obs_masks(gpmdm_pf_t pf, const uint8_t* observed);   /* F x D bytes, filter-major; NULL: all observed */

/* The filtered pose: the observation-space read-out of the particles the filter holds now
 * (post-resample, equal weights):
 *   mean[j]   = (1/P) sum_p mu_j(x_p),  mu = the observation GP's mean (gpmdm.py:955-957)
 *   spread[j] = (1/P) sum_p (mu_j(x_p) - mean[j])^2   (may be NULL)
 * Host outputs, D doubles each.  Reads the particle states only: no draw, no state change, a
 * pending pre-switch stays pending; a mask or the cutoff do not enter (every dimension is
 * read out: the unobserved ones are the filter's imputation).  Valid any time after init /
 * import.  A mean-only GP tile of its own (csrc/obs_readout.h); fixed-order reductions, so
 * the same cloud gives bitwise the same values on every call.  A sharded filter evaluates
 * its replicated cloud on the handle it is called on.  Synchronises `stream`; with mean and
 * spread both NULL the kernels are launched only (timing).  Banks: GPMDM_E_INVALID
 * (gpmdm_bank_observation). */
int gpmdm_pf_observation(gpmdm_pf_t pf, double* mean, double* spread, void* stream);

/* The filtered pose of every filter of a bank: row f of mean / spread is gpmdm_pf_observation
 * of filter f's cloud, bitwise (tiles are cut within a filter, ceil(P / 64) per filter, and
 * partials and finish run per filter), in one pair of launches for the whole bank.  Any
 * handle: on a single filter (F = 1) this is gpmdm_pf_observation. */
int gpmdm_bank_observation(gpmdm_pf_t pf, double* mean, double* spread, void* stream);   /* F x D each, filter-major; spread may be NULL */

/* Multi-step forecast: class, latent state and pose h = 1..horizon frames ahead.  Starting from
 * the particles the filter holds now (post-resample, equal weights), a scratch copy of the
 * cloud runs the filter's own proposal `horizon` times, with no weighting and no resampling:
 *   1. switch    c <- argmax_j T[c, j] / E_j, first maximum (gpmdm_pf.py:137-151)
 *   2. propagate x <- mu_c(x) + sqrt(var_c(x)) eps with the new class's dynamics GP
 *                (gpmdm.py:1032-1068, gpmdm_pf.py:153-168)
 *   3. read out, into row h - 1 of each output that is not NULL:
 *        class_prob[c] = (particles in class c) / P,  state_mean = (1/P) sum_p x_p,
 *        obs_mean / obs_spread = gpmdm_pf_observation's mean and cloud variance of that cloud
 *        (the observation GP's own predictive variance does not enter),
 *        states / classes = the roll-out cloud after the step.
 * GPMDM_FORECAST_MEAN is the deterministic variant: no switch and no noise (classes frozen,
 * x <- mu_c(x)); its first state_mean is gpmdm_pf_predict's mean up to summation order.
 * Draws: always the device's Philox4x32-10, whatever the filter's rng mode, with the key of
 * *seed (NULL: the handle's seed) and the counter
 *   (particle index, the handle's frame, stream, (h << 8) | pair),  stream 4 = the switch's
 *   Exp(1) draws, 5 = the dynamics normals, pair = j >> 1 of class / dimension j,
 * through the transforms of the filter's own draws (E = -log u, u in (0, 1); Box-Muller from a
 * (0, 1) and a [0, 1) uniform).  So a forecast is a function of (cloud, frame, seed) alone, and
 * rows [0, k) of a longer forecast equal the forecast of horizon k bitwise; every reduction has
 * a fixed order.
 * The live filter is untouched: no state change, no draw from the host generator, no frame
 * added to the Philox counter, no health counter; a pending pre-switch stays pending (the
 * roll-out has scratch and class tables of its own, allocated on first use and kept on the
 * handle).  All steps are queued on `stream` without a host wait in between; the call copies the
 * results back and synchronises `stream` once.  With obs_mean and obs_spread both NULL no
 * observation kernel is launched.  states / classes are staged on the device in H x P x (d + 1)
 * doubles for the call's duration: GPMDM_E_INVALID above 1 GiB.  horizon in
 * [1, GPMDM_FORECAST_MAX_HORIZON].  Between a switch and its resample: GPMDM_E_STATE.  A
 * sharded filter forecasts its replicated cloud on the handle it is called on.  Banks:
 * GPMDM_E_INVALID (gpmdm_bank_forecast). */
enum { GPMDM_FORECAST_SAMPLE = 0, GPMDM_FORECAST_MEAN = 1 };
#define GPMDM_FORECAST_MAX_HORIZON 4096
typedef struct gpmdm_forecast_out {   /* host arrays; any may be NULL */
  double*  class_prob;   /* H x C */
  double*  state_mean;   /* H x d */
  double*  obs_mean;     /* H x D */
  double*  obs_spread;   /* H x D */
  double*  states;       /* H x P x d : the roll-out cloud after each step */
  int64_t* classes;      /* H x P */
} gpmdm_forecast_out;
int gpmdm_pf_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed,
                      const gpmdm_forecast_out* out, void* stream);

/* Fixed-lag smoothing from particle ancestry: what was happening `lag` frames ago, given what has
 * been seen since (the genealogy smoother, Kitagawa 1996, J. Comput. Graph. Stat. 5(1) §4.1).
 * Let frame t be the last completed resample, X_t[p], c_t[p] the particles after it and
 * a_t[p] the ancestor of slot p in frame t - 1's cloud (the resample's index,
 * gpmdm_pf.py:206-213; gpmdm_pf_export's ridx).  With j_0(p) = p and j_{l+1}(p) =
 * a_{t-l}[j_l(p)], particle j_l(p) of frame t - l is the lag-l ancestor of the current particle
 * p, and row l - lag_first of each output that is not NULL holds
 *   class_prob[c] = #{p : c_{t-l}[j_l(p)] = c} / P   (an integer count, divided once),
 *   state_mean    = (1/P) sum_p X_{t-l}[j_l(p)]      (fixed summation order),
 *   distinct      = the number of distinct j_l(p): P at lag 0, non-increasing in l,
 *   obs_mean / obs_spread = gpmdm_pf_observation's mean and cloud variance of the traced cloud,
 *   ancestors / states / classes = j_l(p), X_{t-l}[j_l(p)], c_{t-l}[j_l(p)] per current particle.
 * Lag 0 is the resampled cloud itself with equal weights: not gpmdm_pf_read's posterior, which
 * pairs the pre-resample weights with the post-resample classes as the reference does
 * (gpmdm_pf.py:224-248).  Path degeneracy: the filter resamples every frame, so far lags hang on
 * few ancestors -- `distinct` says how many each row rests on.
 * gpmdm_pf_set_smoothing(pf, lag) keeps the last lag + 1 frames' {a, c, X} on the device (one
 * more short launch per resample; lag 0: off, the history is released and a frame issues exactly
 * the work it issues without smoothing); lag in [0, GPMDM_SMOOTH_MAX_LAG], GPMDM_E_INVALID when
 * the history would take more than 1 GiB ((lag + 1) x P x (d + 1) doubles).  Between frames only
 * (GPMDM_E_STATE inside a step); a pending pre-switch stays pending.  The history is cleared --
 * depth 0, the current cloud its root -- by gpmdm_pf_set_smoothing (also with the lag it already
 * has), gpmdm_pf_init, gpmdm_pf_import and gpmdm_pf_set_model; gpmdm_pf_export does not carry
 * it.  gpmdm_pf_smoothing_depth: the lag in force and min(lag, frames recorded since the last
 * clear), the largest lag gpmdm_pf_smoothed serves.
 * gpmdm_pf_smoothed reads lags lag_first..lag_last (0 <= lag_first <= lag_last <= depth,
 * GPMDM_E_INVALID otherwise or with smoothing off).  The live filter is untouched: no state
 * change, no draw, no frame or health counter; a pending pre-switch stays pending; later frames
 * are bitwise those without the call.  No floating-point atomics: the same history gives
 * bitwise the same rows.  All launches are queued on `stream` without a host wait in between;
 * the call copies the results back and synchronises `stream` once.  With obs_mean and
 * obs_spread both NULL no observation kernel is launched.  The particle rows (and the traced
 * clouds a pose reads) are staged on the device for the call's duration: GPMDM_E_INVALID above
 * 1 GiB.  Between a switch and its resample: GPMDM_E_STATE.  Every rank of a sharded filter
 * records its replicated cloud; the read-out serves the handle it is called on.  Banks:
 * GPMDM_E_INVALID (gpmdm_bank_set_smoothing, gpmdm_bank_smoothed; gpmdm_pf_smoothing_depth
 * serves any handle). */
#define GPMDM_SMOOTH_MAX_LAG 4096
typedef struct gpmdm_smoothed_out {   /* host arrays; any may be NULL; n = lag_last - lag_first + 1 */
  double*  class_prob;   /* n x C */
  double*  state_mean;   /* n x d */
  int64_t* distinct;     /* n */
  double*  obs_mean;     /* n x D */
  double*  obs_spread;   /* n x D */
  int64_t* ancestors;    /* n x P */
  double*  states;       /* n x P x d */
  int64_t* classes;      /* n x P */
} gpmdm_smoothed_out;
int gpmdm_pf_set_smoothing(gpmdm_pf_t pf, int lag);
int gpmdm_pf_smoothing_depth(gpmdm_pf_t pf, int* lag, int* depth);
int gpmdm_pf_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out,
                      void* stream);

/* Forecasts and fixed-lag smoothing for filter banks: gpmdm_pf_forecast, gpmdm_pf_set_smoothing
 * and gpmdm_pf_smoothed for every filter of a bank in one sequence of launches.  Any handle
 * (F = 1 included).  The same limits and the same call-order rule hold (GPMDM_FORECAST_MAX_HORIZON,
 * GPMDM_SMOOTH_MAX_LAG, GPMDM_E_STATE between a switch and its resample), and the 1 GiB caps of
 * the forecast's staging, the history and the smoothed read-out's staging count all F x P
 * particles.  The outputs are gpmdm_forecast_out / gpmdm_smoothed_out with one more axis,
 * step-major (lag-major), then filter-major -- the order the device holds them in:
 *   class_prob [H][F][C]   state_mean [H][F][d]   obs_mean / obs_spread [H][F][D]
 *   states [H][F][P][d]    classes / ancestors [H][F][P]    distinct [n][F]
 * with P the particles per filter; ancestors are in-filter indices in [0, P).
 * Row f is the single filter's result on filter f's cloud.  Forecast: filter f draws with the
 * key *seed + f (NULL: the handle's seed, so the filter's own key) and its in-filter particle
 * index in the counter, so class_prob, obs_mean, obs_spread, states and classes are bitwise
 * gpmdm_pf_forecast's with seed *seed + f on a filter holding f's cloud at the same frame.
 * state_mean differs from that call in summation order only: a bank sums each filter's new
 * cloud in particle order, in blocks of 256 cut within the filter (wave butterfly, the four
 * waves in order, then the blocks' sums as gpmdm_pf_smoothed reduces them), because the single
 * call's grouped-order blocks would mix filters; the value depends on the filter's own cloud
 * alone -- not on the horizon, the other filters or how a bank is split into handles.  The
 * grouping and the dynamics tiles run once over all F x P particles, the class counts are
 * integers per (filter, class), and each step's pose is one read-out launch over the F clouds.
 * Smoothing: gpmdm_bank_set_smoothing keeps (lag + 1) x F x P rows; every resample of the bank
 * (each of its resampling paths, the cutoff's included) records behind its read-out, and
 * gpmdm_pf_init, gpmdm_pf_import, gpmdm_pf_set_model and gpmdm_bank_set_smoothing clear the
 * history as for a single filter.  The trace walks each filter's rows only, in blocks of 256 cut
 * within the filter -- the single filter's blocks -- so every field, state_mean included, is
 * bitwise gpmdm_pf_smoothed's on a single filter with the same history.  A bank with smoothing
 * off issues exactly the work it issued before.  Both calls queue everything on `stream`, end
 * with one pinned copy and one wait, release their staging in stream order, and are covered by
 * the handle's lifecycle waits. */
int gpmdm_bank_forecast(gpmdm_pf_t pf, int horizon, int mode, const uint64_t* seed,
                        const gpmdm_forecast_out* out, void* stream);
int gpmdm_bank_set_smoothing(gpmdm_pf_t pf, int lag);
int gpmdm_bank_smoothed(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_smoothed_out* out,
                        void* stream);

/* Per-joint innovations of the frame just weighed, and the GP's own predictive variance.
 * gpmdm_pf_set_predictive(pf, 1): from then on every weigh keeps, per particle, the value
 * vc = 1 - k^T K_y^-1 k its likelihood formed (one 8-byte store per particle; a blacked-out filter
 * of a masked bank keeps NaN), and remembers the frame's staged observation and mask.  Off (the
 * default), a frame issues exactly the launches and results it issued without the feature.
 * Between frames only (GPMDM_E_STATE inside a step); a pending pre-switch stays pending.
 * gpmdm_pf_innovation: with x~_p the propagated particles of that frame (pre-resample, equally
 * weighted), mu_pj the observation GP's mean at x~_p, il2_j = lambda_j^-2, V = {p : vc_p > 0},
 * n_valid = |V|, z the frame's observation and o its mask:
 *   mean_j, spread_j   (1/P) sum_p mu_pj and (1/P) sum_p (mu_pj - mean_j)^2 -- bitwise what
 *                      gpmdm_pf_observation gives on the cloud x~
 *   gp_variance_j      il2_j (1/n_valid) sum_{p in V} vc_p
 *   variance_j         spread_j + gp_variance_j (law of total variance of the mixture)
 *   residual_j         z_j - mean_j                           (NaN where o_j is false)
 *   zscore_j           residual_j / sqrt(variance_j)           (NaN where o_j is false)
 *   log_density_j      log (1/n_valid) sum_{p in V} N(z_j; mu_pj, vc_p il2_j), a proper Gaussian
 *                      with the float64 ln 2 pi               (NaN where o_j is false)
 * Particles outside V are left out of every vc-dependent quantity; with n_valid = 0 -- also a
 * frame or a bank's filter with no observed dimension, where no vc exists -- gp_variance,
 * variance, zscore and log_density are NaN.  states / variance_common: x~_p and vc_p in particle
 * order.  Every reduction has a fixed order: the same frame gives the same bits on every call.
 * Allowed between frames and between gpmdm_pf_propagate / gpmdm_pf_weigh and gpmdm_pf_resample
 * (a deferred likelihood finish is run first; the frame's results do not change).
 * GPMDM_E_INVALID: the feature is off, or the filter is sharded (only ll is exchanged).
 * GPMDM_E_STATE: no frame weighed since the feature was switched on or since gpmdm_pf_propagate,
 * gpmdm_pf_init, gpmdm_pf_import or gpmdm_pf_set_model.
 * gpmdm_pf_observation_gp: the posterior counterpart, gp_var_j = il2_j (1/n_valid) sum_{s: vc > 0}
 * vc[ridx[s]] over the resampled cloud's ancestors (gathered, never recomputed): spread (of
 * gpmdm_pf_observation) + gp_var is the calibrated posterior pose variance.  Needs a completed
 * resample of a frame weighed with the feature on (GPMDM_E_STATE otherwise).
 * The gpmdm_pf_* calls refuse banks (GPMDM_E_INVALID); the gpmdm_bank_* calls serve any handle,
 * outputs filter-major.  Each call queues everything on `stream`, ends with one pinned copy and
 * one wait, and is covered by the handle's lifecycle waits.  With `out` (`gp_var`) NULL the
 * kernels are launched only (timing), as gpmdm_pf_observation does it. */
typedef struct gpmdm_innovation_out {   /* host arrays; any may be NULL; F = 1 for a single filter */
  double*  mean;              /* F x D */
  double*  spread;            /* F x D */
  double*  gp_variance;       /* F x D */
  double*  variance;          /* F x D */
  double*  residual;          /* F x D */
  double*  zscore;            /* F x D */
  double*  log_density;       /* F x D */
  int64_t* n_valid;           /* F */
  uint8_t* observed;          /* F x D: the mask the frame was weighed with */
  double*  states;            /* F x P x d */
  double*  variance_common;   /* F x P */
} gpmdm_innovation_out;
int gpmdm_pf_set_predictive(gpmdm_pf_t pf, int on);
int gpmdm_pf_innovation(gpmdm_pf_t pf, const gpmdm_innovation_out* out, void* stream);
int gpmdm_pf_observation_gp(gpmdm_pf_t pf, double* gp_var /* D */, void* stream);
int gpmdm_bank_set_predictive(gpmdm_pf_t pf, int on);
int gpmdm_bank_innovation(gpmdm_pf_t pf, const gpmdm_innovation_out* out, void* stream);
int gpmdm_bank_observation_gp(gpmdm_pf_t pf, double* gp_var /* F x D */, void* stream);

/* Outlier gating inside the frame: joints whose innovation z-score is too large are dropped from
 * the frame's likelihood before the particles are normalised and resampled.
 * gpmdm_pf_set_gate(pf, threshold, limit): threshold k > 0 switches it on (threshold <= 0: off),
 * 0 < limit <= 1.  From then on every weigh of a frame with an observed dimension ends, on the
 * frame's stream and without a host wait, with the innovation launches of gpmdm_pf_innovation
 * (into scratch of the gate's own) and, with o the frame's mask and zscore_j exactly what
 * gpmdm_pf_innovation reports for the frame,
 *   exceeded_j = o_j and |zscore_j| > k                  (false for NaN)
 *   cap        = floor(limit D_obs)                      (host, fp64)
 *   gated      = exceeded if 1 <= n_exceeded <= cap; empty, with overflow set, if n_exceeded > cap
 *                (a surprise shared by most of the body is no marker fault: weighed as observed)
 *   used       = o and not gated, D' = |used|.
 * When something is gated every particle's log-likelihood is replaced, before the normaliser, by
 * the masked frame's value on the kept joints,
 *   ll'_p = -1/2 S'_p / vc_p - D' log vc_p - sum_{j in used} log il2_j - (D'/2 ln 2 pi)_f32,
 *   S'_p = sum_{j in used} (z_j - mu_pj)^2 lambda_j^2,
 * with the stored vc_p (the N x N pass is not run again; vc_p <= 0 gives NaN as before; D' = 0
 * gives exactly 0).  When nothing is gated the frame is bitwise the frame without the gate.  The
 * health counters and the cutoff's counters are those of the first finish; gpmdm_pf_innovation
 * keeps reporting against the caller's mask.  Off (the default), a frame issues exactly the
 * launches it issued without the feature.
 * Between frames only (GPMDM_E_STATE inside a step), and only with the predictive switch on
 * (GPMDM_E_STATE; gpmdm_pf_set_predictive(pf, 0) is refused while the gate is on).
 * GPMDM_E_INVALID: a bank, a sharded filter, a threshold that is NaN or infinite, a limit outside
 * (0, 1].  The call invalidates the last report.
 * gpmdm_pf_gate_report: what the last gated-mode frame decided -- one copy and one wait on
 * `stream`.  Allowed between gpmdm_pf_propagate / gpmdm_pf_weigh and gpmdm_pf_resample and after
 * the resample.  A blackout frame reports nothing exceeded, nothing used and n_valid = 0.
 * GPMDM_E_INVALID: the gate is off.  GPMDM_E_STATE: no frame weighed in gated mode since
 * gpmdm_pf_init, gpmdm_pf_import, gpmdm_pf_set_model, gpmdm_pf_set_predictive or
 * gpmdm_pf_set_gate. */
typedef struct gpmdm_gate_out {   /* host arrays; any may be NULL */
  double*  zscore;     /* D: the frame's, NaN where unobserved */
  uint8_t* exceeded;   /* D */
  uint8_t* gated;      /* D */
  uint8_t* used;       /* D: the joints the frame's weights rest on */
  int64_t* n_gated;    /* 1 */
  int64_t* n_valid;    /* 1 */
  int32_t* overflow;   /* 1 */
} gpmdm_gate_out;
int gpmdm_pf_set_gate(gpmdm_pf_t pf, double threshold, double limit);   /* threshold <= 0: off */
int gpmdm_pf_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream);
/* Filter banks (gpmdm_bank_create; a single filter is the bank of one): every filter decides for
 * itself, from its own row of z, of the masks and of the innovations, inside the bank's frame.
 * A gated-mode frame queues the innovation pair, the decision, the re-weigh tile and its finish
 * once for all F filters, with the filter as a grid dimension -- never per filter, and without a
 * host wait.  Filter f's frame is bitwise the frame of a single filter (seed + f) with threshold
 * thresholds[f] on f's row; a filter that rejects nothing is bitwise the ungated filter, whatever
 * its neighbours reject.
 * gpmdm_bank_set_gate: thresholds[f] > 0 per filter, +inf: that filter never rejects; all
 * thresholds <= 0: off for the whole bank (GPMDM_E_INVALID: NaN, or some <= 0 and some not).
 * The cap is per filter, floor(limit D_obs_f) of the frame's masks (gpmdm_bank_set_obs_masks); a
 * blacked-out filter's ll stays exactly 0.  The other rules and errors are gpmdm_pf_set_gate's
 * (the predictive switch: gpmdm_bank_set_predictive).  A bank sharded by filter is one handle
 * per rank and is served as it is.
 * gpmdm_bank_gate_report: gpmdm_gate_out with a leading filter axis -- zscore, exceeded, gated,
 * used F x D filter-major, n_gated, n_valid, overflow F each; a blacked-out filter's row is a
 * blackout frame's.  Up to 65535 filters.  gpmdm_pf_set_gate / gpmdm_pf_gate_report refuse a
 * bank handle (GPMDM_E_INVALID). */
int gpmdm_bank_set_gate(gpmdm_pf_t pf, const double* thresholds, double limit);   /* F thresholds; all <= 0: off */
int gpmdm_bank_gate_report(gpmdm_pf_t pf, const gpmdm_gate_out* out, void* stream);   /* arrays F x D, counts F */

/* Device-side GP factor: the recipe of _precompute_kernel_inverses
 * (gpmdm.py:1284-1305) for one GP block -- the observation GP, or one class block of the
 * dynamics GP (the reference's full masked matrix has exact zeros off the class blocks):
 *   K = exp(-|x_i/l - x_j/l|^2) + diag_a I + diag_b I [+ [x_i,1] diag(lin_c2) [x_j,1]^T] + diag_c I
 *   U = chol_upper(K) (rocSOLVER potrf), R = U^-1 (trtri), M = R R^T B (two rocBLAS trmm).
 * X: n x d, lengthscales: d, lin_c2: d+1 (dynamics) or NULL (observations), B: n x k (k may
 * be 0); outputs R (n x n, strictly-lower part zero) and M (n x k).  All host, row-major.
 * The observation GP uses diag_a = sigma_n^2, diag_b = sigma_num^2, diag_c = 0
 * (gpmdm.py:381-406); a dynamics block adds the linear kernel and diag_c = 1e-6
 * (gpmdm.py:408-434, 1299-1305).  A K that is not positive definite is GPMDM_E_INVALID
 * (the reference ignores cholesky_ex's info and continues with garbage). */
int gpmdm_gp_factor(int device, const double* X, int64_t n, int32_t d, const double* lengthscales,
                    const double* lin_c2, double diag_a, double diag_b, double diag_c,
                    const double* B, int64_t k, double* R, double* M);

/* In-place inverse of a symmetric positive-definite n x n matrix on the device (the
 * training loss's K^-1 and log|K|, gpmdm.py:576-584 / 612-619; gpmdm_amd/training.py):
 * rocSOLVER potrf + potri on the caller's buffer A (device, row-major = column-major for a
 * symmetric matrix, leading dimension n), symmetrised; *logdet (host) = 2 sum log diag of
 * the Cholesky factor.  Runs on `stream` (NULL: default) and returns after it completes.
 * A matrix that is not positive definite is GPMDM_E_INVALID and *logdet is NaN. */
int gpmdm_spd_inverse(int device, double* A_dev, int64_t n, double* logdet, void* stream);

/* Replay-mode host helper (no GPU): positions along torch's CPU generator stream, so the
 * reference's per-frame draws (gpmdm_pf.py:137-213: exponential_, normal_, the multinomial's
 * uniforms, all from torch's global generator) can run as parallel chunks of torch's own
 * samplers, each on a private generator set to the state the serial draw would have reached
 * at that chunk -- bit for bit the serial streams.  `state` is torch.Generator.get_state()'s
 * byte image (CPUGeneratorImplState, GPMDM_TORCH_GEN_STATE_BYTES bytes; MT19937,
 * ATen/core/MT19937RNGEngine.h).  A walk covers n_draws random64 draws (two MT outputs each)
 * from `state`; gpmdm_rng_walk_state writes the state after `draws` of them, with the
 * normal-sample cache bytes of `cache_from` (NULL: the start state's). */
#define GPMDM_TORCH_GEN_STATE_BYTES 5056
typedef struct gpmdm_rng_walk* gpmdm_rng_walk_t;
int gpmdm_rng_walk_create(const uint8_t* state, int64_t n_draws, gpmdm_rng_walk_t* out);
/* restart a walk at another state (its buffer is reused when large enough) */
int gpmdm_rng_walk_reset(gpmdm_rng_walk_t walk, const uint8_t* state, int64_t n_draws);
int gpmdm_rng_walk_state(gpmdm_rng_walk_t walk, int64_t draws, const uint8_t* cache_from, uint8_t* out_state);
/* the states at n offsets draws[0..n), written one after the other (n x 5056 bytes) */
int gpmdm_rng_walk_states(gpmdm_rng_walk_t walk, int64_t n, const int64_t* draws, const uint8_t* cache_from,
                          uint8_t* out_states);
int gpmdm_rng_walk_destroy(gpmdm_rng_walk_t walk);

/* Marginal backward smoothing over the history ring: the forward-filter backward marginal
 * smoother (FFBSm).  Where gpmdm_pf_smoothed follows the few ancestors that survived every
 * resample since, this re-weights each past frame's whole cloud by what was seen since; it
 * takes no draw and keeps no second ring.  The transition density is the filter's proposal
 * (gpmdm_pf.py:137-168): the class switches, then the state moves under the new class's dynamics
 * GP.  For a source (x, c) and a target (x', c'),
 *   log f = log T[c, c'] - 1/2 sum_q [(x'_q - mu_q)^2 / v_q + log v_q] - (d/2) log 2 pi,
 * mu, v = gpmdm_predict_dyn(model, c', x)'s mean and variance -- the same launches on the source
 * rows in their given order, so the same bits.  log 0 = -inf gives f = 0, and a source whose v is
 * non-positive or non-finite for class c' has f = 0 towards class-c' targets.
 * gpmdm_backward_step (host arrays; a pure function of its inputs): sources Xs (n_s x d), cs with
 * filter weights a (NULL: 1 / n_s each), targets Xt (n_t x d), ct with smoothing weights wt;
 *   D_j = sum_k a_k f_kj,            log_den_out[j] = log D_j (-inf when no source reaches j),
 *   ws_out[i] = a_i sum_j wt_j f_ij / D_j   (targets with D_j = 0 contribute 0: their mass is lost).
 * Everything is summed on logarithms (a running power-of-two scale, rescaled exactly), in an order
 * that is a function of (n_s, n_t, C) alone and without floating-point atomics: the same inputs
 * give the same bits, and two sources with bitwise-equal (x, c, a) get bitwise-equal weights.
 * GPMDM_E_INVALID: a class outside [0, C), more than 2^36 pairs, or more than 1 GiB of staging
 * for the sources' moments (C x n_s x (2 d + 1) doubles).  ws_out and log_den_out may be NULL.
 * gpmdm_pf_smoothed_marginal: with t the last completed frame, w_0 = 1/P on its cloud, and for
 * l = 0 .. lag_last - 1 one backward step with targets = frame t - l's recorded cloud carrying w_l
 * and sources = frame t - l - 1's with equal weights.  Row l - lag_first of each output that is not
 * NULL holds
 *   class_prob[c] = sum_i w_l,i [c_i = c],   state_mean = sum_i w_l,i X_i,
 *   mass          = sum_i w_l,i   (1 to rounding on a real history; never renormalised),
 *   ess           = mass^2 / sum_i w_l,i^2           (counts copies, and is flattered by them),
 *   ess_distinct  = mass^2 / sum_i m_i w_l,i^2, m_i = the particles of the slot that share i's
 *                   resampling ancestor (an integer histogram; 1 for a cleared ring's root):
 *                   copies carry equal weights, so this is the effective number of distinct
 *                   support points -- the number to read beside gpmdm_pf_smoothed's `distinct`,
 *   weights       = w_l per particle of frame t - l, in the ring's (gpmdm_pf_export's) order.
 * Every sum has a fixed order.  The rules are gpmdm_pf_smoothed's: 0 <= lag_first <= lag_last <=
 * depth, GPMDM_E_INVALID otherwise or with smoothing off, GPMDM_E_STATE between a switch and its
 * resample; the live filter is untouched (no draw, no frame or health counter, a pending
 * pre-switch stays pending, later frames are bitwise those without the call); everything is
 * queued on `stream` and ends with one copy-out and one wait; the scratch is the call's own,
 * grown on demand.  GPMDM_E_INVALID, decided before any launch: banks, sharded filters
 * (n_ranks > 1), more than 2^36 pairs per step (P > 262144), more than 1 GiB of staging. */
typedef struct gpmdm_marginal_out {   /* host arrays; any may be NULL; n = lag_last - lag_first + 1 */
  double* class_prob;     /* n x C */
  double* state_mean;     /* n x d */
  double* mass;           /* n */
  double* ess;            /* n */
  double* ess_distinct;   /* n */
  double* weights;        /* n x P */
} gpmdm_marginal_out;
int gpmdm_backward_step(gpmdm_model_t model, const double* T, int64_t n_s, const double* Xs, const int64_t* cs,
                        const double* a, int64_t n_t, const double* Xt, const int64_t* ct, const double* wt,
                        double* ws_out, double* log_den_out, void* stream);
int gpmdm_pf_smoothed_marginal(gpmdm_pf_t pf, int lag_first, int lag_last, const gpmdm_marginal_out* out,
                               void* stream);

/* Backward simulation over the history ring (FFBSi; Godsill, Doucet & West 2004): draws from the
 * joint smoothing distribution -- whole class-and-state sequences that the model supports, many of
 * them -- where gpmdm_pf_smoothed gives the genealogy, gpmdm_pf_smoothed_marginal per-frame
 * marginals and gpmdm_pf_map_path one sequence.  The transition density f is gpmdm_backward_step's.
 * gpmdm_backward_sample_step (host arrays; a pure function of its inputs): sources Xs (n_s x d), cs
 * with filter weights a (NULL: 1 / n_s each), targets Xt (n_t x d), ct, one uniform u_j in [0, 1)
 * per target;
 *   D_j = sum_k a_k f_kj,            log_den_out[j] = log D_j,
 *   idx_out[j] = the lowest k with sum_{i <= k} a_i f_ij > u_j D_j, the sources in index order;
 * idx_out[j] = -1 and log_den_out[j] = -inf when no source reaches j (D_j = 0, or every term -inf).
 * A source whose term is zero (a_k = 0, T[c_k, c'_j] = 0, an unusable variance) is never returned;
 * whenever D_j > 0 a source is returned: if rounding finds no crossing, the last source of
 * positive term that was searched.  The sums are gpmdm_backward_step's running power-of-two sums,
 * cut into ranges of GPMDM_BACKSAMPLE_RANGE sources -- a function of n_s alone -- and combined in
 * range order, without floating-point atomics: the same inputs give the same bits, and the result
 * for target j depends neither on the other targets nor on n_t.  GPMDM_E_INVALID:
 * gpmdm_backward_step's refusals (a class outside [0, C), more than 2^36 pairs, more than 1 GiB of
 * records) or a u outside [0, 1).  idx_out and log_den_out may be NULL.
 * gpmdm_pf_sample_trajectories(pf, n, lag, seed, out, stream): n trajectories over the window of
 * `lag` lags behind the last completed frame t, P particles.  Trajectory m starts at
 * j_0 = min(P - 1, floor(u_{m,0} P)) in the current cloud and for l = 0 .. lag - 1 draws j_{l+1} in
 * frame t - l - 1's recorded cloud by one step with that cloud as sources (post-resample: every
 * a_k = 1 / P), target j_l and uniform u_{m,l+1}.  A trajectory whose step returns -1 stays -1 for
 * all older lags: its class is -1 and its states are NaN.  u_{m,l} = the [0, 1) uniform of the
 * first two words of Philox4x32-10 with key `seed` (NULL: the handle's own, as gpmdm_pf_forecast)
 * and counter (m, frame, stream 6, l): trajectory m is a function of (seed, frame, m, history)
 * alone -- not of n, and a shorter window is a prefix of a longer one.  The call takes no draw
 * from the filter's own streams and changes nothing in the filter (no frame or health counter, a
 * pending pre-switch stays pending, later frames are bitwise those without the call).  Row l of
 * each output that is not NULL is lag l, frame t - l; class_prob = class counts / alive and
 * state_mean = the sum over the alive trajectories / alive (both NaN when alive is 0; the sums
 * have a fixed order and are carried in two terms); distinct = the distinct particles of slot l
 * among the alive ones; obs_mean / obs_spread = the pose read-out gpmdm_pf_smoothed runs on a
 * traced cloud, here on the alive sampled states of lag l (NaN when alive is 0).  GPMDM_E_INVALID,
 * decided before any launch: banks, sharded filters, smoothing off, n outside [1, 2^31), n x P above
 * 2^36, lag outside [1, depth], more than 1 GiB of records or of staging (the uniforms, indices,
 * classes and states of every lag); GPMDM_E_STATE between a switch and its resample.  Everything
 * is queued on `stream` and ends with one copy-out and one wait (with a pose: the read-outs, whose
 * sizes are the alive counts, and a second wait); the scratch lives on the handle, grown on demand. */
#define GPMDM_BACKSAMPLE_RANGE 1024
typedef struct gpmdm_sample_out {   /* host arrays; any may be NULL; L = lag + 1 */
  int64_t* index;         /* L x n: j_l of every trajectory, a particle of slot l (-1: dead) */
  int64_t* classes;       /* L x n */
  double* states;         /* L x n x d */
  double* class_prob;     /* L x C */
  double* state_mean;     /* L x d */
  int64_t* alive;         /* L */
  int64_t* distinct;      /* L */
  double* obs_mean;       /* L x D */
  double* obs_spread;     /* L x D */
} gpmdm_sample_out;
int gpmdm_backward_sample_step(gpmdm_model_t model, const double* T, int64_t n_s, const double* Xs, const int64_t* cs,
                               const double* a, int64_t n_t, const double* Xt, const int64_t* ct, const double* u,
                               int64_t* idx_out, double* log_den_out, void* stream);
int gpmdm_pf_sample_trajectories(gpmdm_pf_t pf, int64_t n, int lag, const uint64_t* seed, const gpmdm_sample_out* out,
                                 void* stream);

/* MAP trajectory decoding over the history ring: the most probable class-and-state sequence on
 * the particle grid (particle Viterbi; Godsill, Doucet & West 2001) -- one consistent trajectory
 * where gpmdm_pf_smoothed and gpmdm_pf_smoothed_marginal give per-frame marginals.  It takes no
 * draw.  Let frame t be the last completed resample and slot l the ring's record of frame t - l:
 * X_l[i], c_l[i], a_l[i].  gpmdm_pf_set_map(pf, 1) adds a plane l_l[i] to the ring: the
 * log-likelihood of the proposal that slot particle i copies, gpmdm_pf_export's ll[resample_idx[i]]
 * of that frame -- the value the frame's normaliser read, masked and gated as the frame was.
 * log f(k -> j) is gpmdm_backward_step's transition density with source (X_{l+1}[k], c_{l+1}[k])
 * and target (X_l[j], c_l[j]).  For a window of n lags, 1 <= n <= depth:
 *   delta_n(k) = 0   (the root cloud is flat over its support; its l is never read: a cleared
 *                     ring's root has none),
 *   delta_l(j) = l_l[j] + max_k [delta_{l+1}(k) + log f(k -> j)]       for l = n - 1 .. 0,
 *   psi_l(j)   = the lowest k attaining the maximum; psi_l(j) = -1 and delta_l(j) = -inf when no
 *                source reaches j or l_l[j] is not finite; a NaN candidate never wins,
 *   j*_0 = the lowest index attaining max_j delta_0(j),  j*_{l+1} = psi_l(j*_l),
 *   log_joint = delta_0(j*_0).
 * If log_joint is -inf the call succeeds with index and classes -1, states NaN and score -inf from
 * the first unreachable lag on.  All values are natural logarithms.  There are no floating-point
 * atomics, ties go to the lowest index always, and the same inputs give the same bits.
 * Copies of a resampled particle are bitwise-equal candidates and a maximum has no order: the
 * recursion runs on each slot's leaders (per distinct resampling ancestor the copy of lowest
 * index, in increasing index) and gives the delta and psi of the recursion over all P rows.
 * gpmdm_pf_set_map(pf, on): needs smoothing on (gpmdm_pf_set_smoothing), between frames only
 * (GPMDM_E_STATE inside one), single filters on one rank; allocates the plane, (lag + 1) x P
 * doubles -- counted in the history's 1 GiB limit while the flag is on -- and clears the history
 * exactly as gpmdm_pf_set_smoothing does (a cleared ring's root records l = 0).  A later
 * gpmdm_pf_set_smoothing keeps the flag and resizes the plane.  With the flag on every resample
 * issues one more short launch (l_dst[i] = ll[ridx[i]]); with it off a frame issues exactly the
 * launches it issued before.  on = 0 releases the plane and keeps the rest of the history.
 * gpmdm_pf_map_recording: the flag.
 * gpmdm_map_step (host arrays; a pure function of its inputs; no de-duplication, the caller's rows
 * are used as given): sources Xs (n_s x d), cs with scores delta_s (NULL: zeros), targets Xt
 * (n_t x d), ct with log-likelihoods ll_t (NULL: zeros);
 *   delta_out[j] = ll_t[j] + max_k [delta_s[k] + log f(k -> j)],   psi_out[j] = the lowest such k
 * (-inf and -1 as above).  Refusals are gpmdm_backward_step's: sizes, more than 2^36 pairs, more
 * than 1 GiB of records, a class outside [0, C).  delta_out and psi_out may be NULL.
 * gpmdm_pf_map_path(pf, lag, out, stream): the window of `lag` lags behind the last completed
 * frame; row l of each output that is not NULL is lag l, frame t - l.  The rules are
 * gpmdm_pf_smoothed_marginal's: GPMDM_E_INVALID, decided before any launch, for banks, sharded
 * filters, smoothing or map recording off, lag outside [1, depth], more than 2^36 pairs per step,
 * more than 1 GiB of staging (delta and psi of every lag by particle, and the records);
 * GPMDM_E_STATE between a switch and its resample.  The live filter is untouched (no draw, no
 * frame or health counter, a pending pre-switch stays pending, later frames are bitwise those
 * without the call); everything is queued on `stream` and ends with one copy-out and one wait. */
typedef struct gpmdm_map_out {   /* host arrays; any may be NULL; n = lag + 1 */
  int64_t* index;         /* n: j*_l, the path's particle in slot l */
  int64_t* classes;       /* n */
  double* states;         /* n x d */
  double* score;          /* n: delta_l(j*_l) */
  double* log_joint;      /* 1 */
  int64_t* distinct;      /* n: the slots' leaders (distinct resampling ancestors; P for a cleared ring's root) */
  double* delta;          /* n x P: delta_l per particle of slot l */
  int64_t* backpointer;   /* lag x P: psi_l per particle of slot l, an index into slot l + 1 */
} gpmdm_map_out;
int gpmdm_pf_set_map(gpmdm_pf_t pf, int on);
int gpmdm_pf_map_recording(gpmdm_pf_t pf, int* on);
int gpmdm_map_step(gpmdm_model_t model, const double* T, int64_t n_s, const double* Xs, const int64_t* cs,
                   const double* delta_s, int64_t n_t, const double* Xt, const int64_t* ct, const double* ll_t,
                   double* delta_out, int64_t* psi_out, void* stream);
int gpmdm_pf_map_path(gpmdm_pf_t pf, int lag, const gpmdm_map_out* out, void* stream);

/* Message of the last failed call on this thread ("" if none). */
const char* gpmdm_last_error(void);

/* Library version string. */
const char* gpmdm_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GPMDM_HIP_H */
