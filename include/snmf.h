/*
 * snmf.h -- C ABI of libsnmf_hip.so, the MI355X (gfx950) sparse-NMF multiplicative-update engine.
 *
 * Drop-in boundary for the hot path of lordet01/SE_SNMF_NAT:
 *     [w, h, objective] = sparse_nmf(v, p)            (reference: src/sparse_nmf.m:1)
 *     [w, h, objective] = sparse_nmf_GPU(v, p)        (reference: src/sparse_nmf_GPU.m:1)
 * and the 3-solve loop of run_basis_DNMF.m:36-55 built on it.  The reference is MATLAB; the
 * binding a maintainer adds is a MEX shim (integration/sparse_nmf_mex.cpp) or, from Python,
 * ctypes (se_snmf_nat_amd/_lib.py).  Every entry point below names the reference lines it replaces.
 *
 * Conventions: all matrices are column-major (MATLAB layout) with explicit leading dimensions
 * where given (a rows x cols matrix with leading dimension ld >= rows holds (cols - 1) * ld + rows elements, the BLAS convention:
 * nothing past the last column's last row is read or written, nor the rows between `rows` and ld of any column; a leading
 * dimension below the row count is SNMF_ERR_INVALID and nothing is written; arguments without one are tight); a HOST matrix handed
 * to snmf_plan_set_*, snmf_multi_set_* or snmf_batch_set_problem_* may be overwritten or freed as soon as the call returns (a
 * device buffer is read later, on the context's stream);
 * plain pointers and sizes only; every function returns an snmf_status and never
 * throws; snmf_last_error() returns a thread-local message for the last failure.
 * There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 * SNMF_ERR_NO_DEVICE.
 */
#ifndef SNMF_H_
#define SNMF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNMF_ABI_VERSION 5  /* 5: snmf_online_batch_* incl. _restart / _get_basis_f64 / _set_mel / _restart_mel / _get_mel_basis_f32 / _f64 (added within 5: new entries only), snmf_multi_release_cache, snmf_multi_cached_teams, snmf_rccl_*, snmf_plan_run_sharded_rccl (the device RNG of snmf_plan_set_h_random changed with 4: draws seeded under ABI 3 are not reproducible); 4: snmf_run_basis_dnmf_multi_*; 3: snmf_run_basis_dnmf_*, snmf_run_basis_train_audio_f64, snmf_sparse_nmf_oop_*, snmf_plan_set_h_random, snmf_ctx_xfer_stats; 2: snmf_multi_* */

typedef enum snmf_status {
    SNMF_OK = 0,
    SNMF_ERR_INVALID = 1,   /* bad argument (NULL, non-positive size, ...) */
    SNMF_ERR_NO_INIT = 2,   /* neither init_w nor r given: src/sparse_nmf.m:117-119 */
    SNMF_ERR_DIM = 3,       /* MATLAB dimension error on the path (e.g. partial h_update_ind, :192) */
    SNMF_ERR_NO_FIELD = 4,  /* p.cost_check missing: src/sparse_nmf.m:260 */
    SNMF_ERR_NO_DEVICE = 5, /* no HIP device / HIP runtime failure */
    SNMF_ERR_NOMEM = 6,
    SNMF_ERR_STATE = 7,     /* call order violated (e.g. run before set_v) */
    SNMF_ERR_UNSUPPORTED = 8,
    SNMF_ERR_INTERNAL = 9   /* a bounded device-side wait gave up (never expected): the results are invalid */
} snmf_status;

/* sparsity argument forms of src/sparse_nmf.m:150-155 */
typedef enum snmf_sparsity_kind {
    SNMF_SPARSITY_SCALAR = 0, /* length(p.sparsity)==1 -> ones(r,n)*s   (:151-152) */
    SNMF_SPARSITY_RVEC = 1,   /* r x 1 column -> repmat(.,1,n)         (:153-154) */
    SNMF_SPARSITY_FULL = 2    /* r x n given in full                    (:155)     */
} snmf_sparsity_kind;

/* Solver parameters = the fields of `p` the reference reads (src/sparse_nmf.m:79-164). */
typedef struct snmf_params {
    int32_t F;          /* rows of v       (m, :71) */
    int32_t T;          /* columns of v    (n, :72) */
    int32_t r;          /* rank            (:116-131) */
    double beta;        /* divergence order after the cf switch (:99-110): is=0, kl=1, ed=2 */
    int32_t max_iter;   /* :79-81, default 100 */
    double conv_eps;    /* :91-93, default 0 */
    int32_t cost_check; /* :260 (no default in the reference; the wrappers enforce presence) */
    int32_t floor_v;    /* 1: v = max(v,1e-9) as sparse_nmf.m:169; 0: sparse_nmf_GPU.m (absent) */
    int32_t sparsity_kind;     /* snmf_sparsity_kind */
    double sparsity_scalar;    /* used when kind == SCALAR */
    const uint8_t* w_update_ind; /* r flags or NULL = all true (:142-144) */
    const uint8_t* h_update_ind; /* r flags or NULL = all true (:146-148) */
} snmf_params;

typedef struct snmf_ctx snmf_ctx;   /* device + stream + kernel configuration */
typedef struct snmf_plan snmf_plan; /* one problem resident in HBM: V, W, H, workspaces */

/* ---- library ---------------------------------------------------------------------------- */
int snmf_abi_version(void);
const char* snmf_last_error(void);
int snmf_device_count(void); /* number of HIP devices visible, 0 if none (never fails) */

/* ---- context ---------------------------------------------------------------------------- */
/* Replaces the implicit gpuArray device state of src/sparse_nmf_GPU.m:161-166.
 * A context keeps the device blocks of destroyed plans for the next plan of the same sizes (a caller that solves problem after
 * problem of one shape -- every call site of sparse_nmf in the reference -- does not pay hipMalloc / hipFree per call): at most
 * SNMF_DEVCACHE_MB megabytes (environment, read at creation; default 4096, 0 = off), released by snmf_ctx_destroy. */
int snmf_ctx_create(snmf_ctx** out, int device);
/* Use a caller-owned hipStream_t; NULL = the context's own (non-blocking) stream.  The legacy
 * default stream has handle 0 == NULL and therefore cannot be selected: a caller that must order
 * other work (e.g. an RCCL all-reduce) against the solver passes an explicitly created stream and
 * issues that work on it (se_snmf_nat_amd/dist.py). */
int snmf_ctx_set_stream(snmf_ctx* ctx, void* hip_stream);
int snmf_ctx_sync(snmf_ctx* ctx);
void snmf_ctx_destroy(snmf_ctx* ctx);

/* ---- one-shot drop-in ------------------------------------------------------------------- */
/* [w,h,objective] = sparse_nmf(v,p) with explicit initial factors (the MATLAB wrapper draws
 * them with MATLAB's own RNG, src/sparse_nmf.m:112-140, so RNG parity is by construction).
 *   V      F x T  (ldV >= F), never modified                       (:71-72, :169)
 *   W      F x r  in: init_w (:116-131)   out: w, unit-L2 columns  (:242)
 *   H      r x T  in: init_h (:133-140)   out: h
 *   sparsity: NULL for SCALAR, r doubles for RVEC, r x T doubles for FULL (:150-155)
 *   div_out, cost_out: max_iter doubles each, zero-filled then objective.div/.cost (:171-173,
 *                      :263-264); may be NULL
 *   n_iter_out: number of iterations executed = length of the truncated vectors (:279-280)
 */
int snmf_sparse_nmf_f64(snmf_ctx* ctx, const snmf_params* p, const double* V, int64_t ldV,
                        double* W, double* H, const double* sparsity, double* div_out,
                        double* cost_out, int32_t* n_iter_out);
int snmf_sparse_nmf_f32(snmf_ctx* ctx, const snmf_params* p, const float* V, int64_t ldV,
                        float* W, float* H, const float* sparsity, double* div_out,
                        double* cost_out, int32_t* n_iter_out);
/* Out-of-place form: W0 (F x r) and H0 (r x T) are read-only, the results go to W and H (tight: leading dimensions F and r).
 * This is MATLAB's value semantics without a copy of init_h on the host first -- what the MEX shim calls. */
int snmf_sparse_nmf_oop_f64(snmf_ctx* ctx, const snmf_params* p, const double* V, int64_t ldV, const double* W0,
                            const double* H0, const double* sparsity, double* W, double* H, double* div_out,
                            double* cost_out, int32_t* n_iter_out);
int snmf_sparse_nmf_oop_f32(snmf_ctx* ctx, const snmf_params* p, const float* V, int64_t ldV, const float* W0,
                            const float* H0, const float* sparsity, float* W, float* H, double* div_out,
                            double* cost_out, int32_t* n_iter_out);
/* The fp64 solve mode (added within ABI 5: a new entry only).  The four entries above only name the type of the HOST buffers:
 * everything is narrowed on upload and the iteration runs on the fp32 MFMA (results ~1e-6 from the double-precision
 * algorithm).  This entry computes src/sparse_nmf.m:157-286 in fp64 from end to end: storage is fp64 and the five products
 * of an iteration (w*h, w'*R, w'*D, R*h', D*h'; :194-207, :215-243) run on the f64 MFMA (v_mfma_f64_16x16x4_f64), the
 * element-wise passes, the F x r epilogue (:215-244), the initial scaling (:157-169), the objective (:248-261) and the
 * stop test (:272-284, on the device) in fp64.  Every reduction has a fixed order: two calls on one input give the same bits.
 * What it is for: a caller who passes doubles and wants the double-precision algorithm's results (within ~1e-12 of a host
 * fp64 evaluation), and a judge of the fp32 path at the workload's own size.  What it costs: every intermediate lives in
 * HBM (about 8 (3 F T + 3 r T) bytes; 1.5 GB at 257 x 100 000, r = 256), nothing is fused, and the f64 MFMA runs at half
 * the f32 MFMA's rate -- measured 6 to 8 times fewer iterations per second than the fp32 entries.
 * Same argument list and meaning as snmf_sparse_nmf_oop_f64; every field of snmf_params means what it means there
 * (floor_v = 0: sparse_nmf_GPU.m; cost_check = 0: no objective, no stop; partial w_update_ind; the three sparsity forms;
 * a partial h_update_ind is SNMF_ERR_DIM).  Any F, T, r the device memory holds; a failed allocation is SNMF_ERR_NOMEM. */
int snmf_sparse_nmf_fp64(snmf_ctx* ctx, const snmf_params* p, const double* V, int64_t ldV, const double* W0,
                         const double* H0, const double* sparsity, double* W, double* H, double* div_out,
                         double* cost_out, int32_t* n_iter_out);

/* ---- resident-plan API (benchmarks, on-device pipelines, multi-GPU sharding) -------------- */
/* A plan owns fp32 device copies of V (F x T), W (F x r), H (r x T) in the engine's padded
 * layouts plus all workspaces.  Call order: create -> set_v/set_w/set_h[/set_sparsity] ->
 * init -> run (or the step functions) -> get_*.  `p->T` is the LOCAL column count of this
 * shard when the frame axis is sharded across ranks.
 * One documented deviation from the reference's expression: a Euclidean (beta = 2) FULL update with r < 2F forms the W step's
 * P = max(W*H, 1e-9) * H' (src/sparse_nmf.m:166, :228-233) as W * (H*H'), i.e. without the floor on W*H.  The two differ only
 * where W*H < 1e-9 (silent rows / frames), by at most 1e-9 * sum(h) per entry of P.  Environment SNMF_GRAM_P=0 at plan creation
 * selects the reference's expression (one more Lam' pass per iteration); tests/test_gpu_parity.py pins both. */
int snmf_plan_create(snmf_ctx* ctx, const snmf_params* p, snmf_plan** out);
void snmf_plan_destroy(snmf_plan* plan);

/* is_device != 0: pointer is device memory on the context's device (fp32/fp64 as named).  The library reads it on
 * the CONTEXT's stream (snmf_ctx_set_stream): a device buffer produced on another stream must be complete -- or that
 * stream ordered ahead of the context's with an event -- before the call; the host mirror synchronises the producer. */
int snmf_plan_set_v_f64(snmf_plan* plan, const double* V, int64_t ld, int is_device);
int snmf_plan_set_v_f32(snmf_plan* plan, const float* V, int64_t ld, int is_device);
int snmf_plan_set_w_f64(snmf_plan* plan, const double* W, int64_t ld, int is_device);
int snmf_plan_set_w_f32(snmf_plan* plan, const float* W, int64_t ld, int is_device);
int snmf_plan_set_h_f64(snmf_plan* plan, const double* H, int64_t ld, int is_device);
int snmf_plan_set_h_f32(snmf_plan* plan, const float* H, int64_t ld, int is_device);
/* RVEC: r values; FULL: r x T (ld = r).  SCALAR needs no call. */
int snmf_plan_set_sparsity_f64(snmf_plan* plan, const double* S, int is_device);
int snmf_plan_set_sparsity_f32(snmf_plan* plan, const float* S, int is_device);

/* src/sparse_nmf.m:157-169: normalise W columns, rescale H rows (V is floored at set_v); resets
 * the iteration counter and the objective history.  If W was not set again since the last init its
 * normalised form and norms are reused (same bits as normalising the same input again). */
int snmf_plan_init(snmf_plan* plan);

/* The hot loop src/sparse_nmf.m:186-286: up to `n_iters` more iterations (bounded by
 * max_iter), early stop per :273-282 evaluated on the device.  Asynchronous on the context's
 * stream unless conv_eps > 0 (then it synchronises every few iterations to read the stop flag).
 * iters_done (optional) receives the total iterations executed so far (after a sync). */
int snmf_plan_run(snmf_plan* plan, int32_t n_iters, int32_t* iters_done);

/* Step functions for frame-sharded multi-GPU training; one iteration is
 *     hstep -> wstats(stats) -> [all-reduce(sum) of stats across ranks] -> wapply(stats)
 * stats is a DEVICE buffer of snmf_plan_stats_len() doubles:
 *     [ G or Q (F*r) | P (F*r, beta != 1 only) | s (r) | div | sum(S.*H) ]
 * hstep  : src/sparse_nmf.m:189-208 on the local columns (no-op when no row of h is updated)
 * wstats : the T-reductions of :215-239 (+ the objective sums of :248-261 for the PREVIOUS
 *          iterate) over the local columns
 * wapply : the F x r epilogue of :215-244 on the reduced statistics, the convergence test of
 *          :272-284 on the reduced cost, identical on every rank.
 * finalize: objective of the last iterate (needs one more local pass + all-reduce of the two
 *          scalars): objstats -> [all-reduce] -> objapply. */
int64_t snmf_plan_stats_len(const snmf_plan* plan);
int snmf_plan_hstep(snmf_plan* plan);
int snmf_plan_wstats(snmf_plan* plan, double* stats_dev);
int snmf_plan_wapply(snmf_plan* plan, const double* stats_dev);
int snmf_plan_objstats(snmf_plan* plan, double* stats_dev);
int snmf_plan_objapply(snmf_plan* plan, const double* stats_dev);
/* 1 when the device-side convergence test has fired (synchronises the stream). */
int snmf_plan_stopped(snmf_plan* plan, int32_t* stopped);
/* The loop above in ONE call for a process-per-GPU host: up to n_iters iterations of
 *     hstep -> wstats(stats) -> all_reduce(stats, len, user) -> wapply(stats)
 * with the caller's collective as a callback (it must enqueue an in-place SUM of the `len` doubles at `stats` over the ranks on
 * the context's stream, or order its own stream against it; it returns 0, anything else aborts the loop with
 * SNMF_ERR_INVALID).  `len` is the whole buffer, or 2 (the two cost scalars at the tail: `stats + stats_len - 2`) when no
 * column of W is updated.  all_reduce = NULL: a single rank.  poll_every > 0: the convergence flag is read every poll_every
 * iterations when conv_eps > 0 (every rank reads the same value).  finalize != 0: after the last iteration of the SOLVE
 * (max_iter reached, no early stop) the objective of the last iterate is formed (objstats -> all_reduce -> objapply).
 * iters_done: iterations this call ran.  src/sparse_nmf.m:186-286 per rank. */
typedef int (*snmf_allreduce_fn)(double* stats_dev, int64_t len, void* user);
int snmf_plan_run_sharded(snmf_plan* plan, int32_t n_iters, double* stats_dev, snmf_allreduce_fn all_reduce, void* user,
                          int32_t poll_every, int32_t finalize, int32_t* iters_done);
/* The same loop with the collective issued by the library itself: ncclAllReduce (RCCL over xGMI) of the statistics on the
 * context's stream, once per iteration -- no callback into the host language (a ctypes / MEX trampoline per iteration was 29 us of
 * host work, a quarter of an iteration on a short shard).  librccl.so is resolved with dlopen when first needed (SNMF_RCCL_LIB, else
 * the copy the process already holds -- PyTorch's --, else the system's), so this library loads without it; snmf_rccl_available()
 * says whether it was found.  The communicator is set up by the caller's own out-of-band channel: rank 0 calls
 * snmf_rccl_get_unique_id (128 bytes), every rank receives them (torch.distributed broadcast, MPI, a file) and calls
 * snmf_rccl_comm_create(device, id, n_ranks, rank) -- ncclCommInitRank, collective over the ranks -- and later
 * snmf_rccl_comm_destroy.  One communicator per rank, on the plan's device.  Reference: the one sum per iteration that sharding the
 * frames of run_basis_train.m:88 / run_basis_DNMF.m:47,53 over ranks needs (the statistics of src/sparse_nmf.m:215-239, :248-261). */
typedef struct snmf_rccl_comm snmf_rccl_comm;
int snmf_rccl_available(void);
int snmf_rccl_get_unique_id(void* id_out, int64_t cap);
int snmf_rccl_comm_create(int32_t device, const void* id, int32_t n_ranks, int32_t rank, snmf_rccl_comm** out);
void snmf_rccl_comm_destroy(snmf_rccl_comm* comm);
int snmf_plan_run_sharded_rccl(snmf_plan* plan, int32_t n_iters, double* stats_dev, snmf_rccl_comm* comm, int32_t poll_every,
                               int32_t finalize, int32_t* iters_done);

/* Online separation stream (src/NTF_sep_event_RT.m:67-107 -> src/bnmf_sep_event_RT_IS16.m:138-154):
 * the SAME dictionary W and the SAME initial activations H0 (the reference re-seeds its generator
 * in every call, src/sparse_nmf.m:112-114, so H0 is identical for every frame) are used for
 * n_solves INDEPENDENT H-only solves, one per group of `frames_per_solve` (<= 32) consecutive
 * columns of V; each has its own objective and its own convergence test (:272-284).
 * Result-identical to n_solves calls of snmf_sparse_nmf_* with w_update_ind all false, but W stays
 * resident and normalised, V is uploaded once, and every solve is ONE persistent workgroup (all of
 * its iterations inside one launch), the solves running concurrently across the CUs.
 *   plan    : H-only plan whose T >= n_solves*frames_per_solve (capacity); snmf_plan_set_w called
 *   V       : F x (n_solves*frames_per_solve) host matrix, leading dimension ldV
 *   H0      : r x frames_per_solve host matrix
 *   H_out   : r x (n_solves*frames_per_solve) host matrix (leading dimension r)
 *   n_iter_out[n_solves], cost_out[n_solves] (last recorded cost, 0 without cost_check): optional
 * Scalar / r-vector sparsity only. */
int snmf_plan_solve_frames_f64(snmf_plan* plan, int32_t frames_per_solve, const double* V, int64_t ldV,
                               int32_t n_solves, const double* H0, double* H_out, int32_t* n_iter_out,
                               double* cost_out);
int snmf_plan_solve_frames_f32(snmf_plan* plan, int32_t frames_per_solve, const float* V, int64_t ldV,
                               int32_t n_solves, const float* H0, float* H_out, int32_t* n_iter_out,
                               double* cost_out);

/* Results.  W: F x r, H: r x T(local).  Host or device destinations. */
int snmf_plan_get_w_f64(snmf_plan* plan, double* W, int64_t ld, int is_device);
int snmf_plan_get_w_f32(snmf_plan* plan, float* W, int64_t ld, int is_device);
int snmf_plan_get_h_f64(snmf_plan* plan, double* H, int64_t ld, int is_device);
int snmf_plan_get_h_f32(snmf_plan* plan, float* H, int64_t ld, int is_device);
/* objective.div / objective.cost (src/sparse_nmf.m:263-264,:279-280): writes n_iter entries
 * of each (arrays must hold max_iter doubles; the tail is zero-filled). */
int snmf_plan_get_objective(snmf_plan* plan, double* div_out, double* cost_out,
                            int32_t* n_iter_out);

/* ---- spectrogram front-end on the device (the step before the path in every call stack) ---- */
/* Parameters of src/stft_fft.m + run_basis_train.m:60-63 (shipped values:
 * settings/initial_setting_SNMF_NAT.m:21-37,53,88-90). */
typedef struct snmf_stft_params {
    int32_t framelength;   /* sz,    p.framelength (640) */
    int32_t frameshift;    /* shift, p.frameshift  (160) */
    int32_t fftlength;     /* power of two in [64, 4096], p.fftlength (1024) */
    int32_t dcbin;         /* first DCbin magnitudes are set to 1e-6 (src/stft_fft.m:31); must be >= 1 */
    int32_t splice;        /* p.Splice (src/frame_splice.m), 0 = none */
    double preemph;        /* p.preemph */
    double pow;            /* p.pow: features are |STFT|.^pow + nonzerofloor */
    double nonzerofloor;   /* p.nonzerofloor */
    const double* window;  /* framelength values, p.win_STFT */
} snmf_stft_params;

/* Number of frames src/stft_fft.m:21 processes for an n_samples signal (its trailing all-zero
 * columns are the ones run_basis_train.m:61 removes).  Pure host arithmetic, never fails. */
int64_t snmf_stft_num_frames(const snmf_stft_params* sp, int64_t n_samples);

/* TF_mag of run_basis_train.m:60-63 / run_basis_DNMF.m:13-16: F x n_frames, F = (2*splice+1)*(fftlength/2+1).
 * samples: float audio (host or device); V_out: host or device, leading dimension ld >= F. */
int snmf_stft_features_f32(snmf_ctx* ctx, const snmf_stft_params* sp, const float* samples, int64_t n_samples,
                           int samples_on_device, float* V_out, int64_t ld, int out_on_device,
                           int32_t* n_frames_out);
/* Same, written straight into a plan's resident V (plan F must equal the feature rows and plan T the
 * frame count); the V floor of src/sparse_nmf.m:169 is applied as in snmf_plan_set_v. */
int snmf_plan_set_v_from_audio_f32(snmf_plan* plan, const snmf_stft_params* sp, const float* samples,
                                   int64_t n_samples, int samples_on_device);
/* Mel projection of run_basis_train.m:70-78: out (K*M x T) = blockdiag(mel) * V (K*n x T);
 * mel: M x n ROW-major host matrix (mel_matrix(...)'), V / out host or device (both the same side). */
int snmf_mel_features_f32(snmf_ctx* ctx, const float* mel, int32_t M, int32_t n, int32_t K, const float* V,
                          int64_t ldv, int32_t T, float* out, int64_t ldo, int on_device);
/* TF_DD of src/TF_DD.m:1-9 (run_basis_train.m:64-67, p.domain_DD): recursive average along the frames, row by row,
 * X_DD(:,1) = X(:,1), X_DD(:,l) = alpha_eta X_DD(:,l-1) + (1 - alpha_eta) X(:,l).  X / out: F x T column-major, host or
 * device (both the same side); out may be X. */
int snmf_tf_dd_f32(snmf_ctx* ctx, double alpha_eta, int32_t F, int32_t T, const float* X, int64_t ldx, float* out,
                   int64_t ldo, int on_device);

/* ---- the training callers, device-resident ------------------------------------------------------- */
/* h = rand(r, n) of src/sparse_nmf.m:133-134 for a caller that supplies no init_h: Philox-4x32-10 keyed by `seed`, counter =
 * column-major element index / 4, value = ((x >> 9) + 0.5) * 2^-23 (exactly representable, strictly inside (0, 1)), written straight into the plan's resident H
 * (MATLAB's legacy rand('seed', s) stream is not reproducible; a wrapper that wants ITS draws passes them to snmf_plan_set_h).
 * Every entry below that takes `H0` uses this generator when H0 is NULL. */
int snmf_plan_set_h_random(snmf_plan* plan, uint64_t seed);

/* B_hat = run_basis_DNMF(x, d, B, p), the 3-solve loop run_basis_DNMF.m:36-55 on formed features:
 *     [~, A_hat]   = sparse_nmf(Y, p)   H-only,  init_w = B                                         (:37-40)
 *     [B_hat_x, ~] = sparse_nmf(X, p)   W-only,  init_w = B(:,1:R_x),        init_h = A_hat(1:R_x,:)      (:43-47)
 *     [B_hat_d, ~] = sparse_nmf(D, p)   W-only,  init_w = B(:,R_x+1:R_x+R_d), init_h = A_hat(R_x+1:end,:)  (:49-53)
 *     B_hat = [B_hat_x, B_hat_d]                                                                   (:55)
 * Result-identical to three snmf_sparse_nmf_* calls, but Y, X, D cross PCIe once each (X and D on a second stream under solve
 * 1), A_hat never leaves HBM, and only B_hat (and A_hat if asked for) comes back.
 *   p      : F, T, r = R_x + R_d, beta, max_iter, conv_eps, cost_check, floor_v, scalar sparsity; the update masks are set by
 *            the loop (p->w_update_ind / h_update_ind are ignored)
 *   Y, X, D: F x T host matrices (mixture / clean / noise features, :13-34), never modified
 *   B      : F x (R_x + R_d) exemplar basis;  H0: (R_x + R_d) x T initial activations of solve 1 (leading dimension r) or NULL
 *   B_hat  : F x (R_x + R_d) out;  A_hat: (R_x + R_d) x T out or NULL;  n_iter_out: 3 iteration counts or NULL */
int snmf_run_basis_dnmf_f64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, const double* Y, int64_t ldY,
                            const double* X, int64_t ldX, const double* D, int64_t ldD, const double* B, int64_t ldB,
                            const double* H0, uint64_t seed, double* B_hat, int64_t ldBh, double* A_hat, int64_t ldA,
                            int32_t* n_iter_out);
int snmf_run_basis_dnmf_f32(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, const float* Y, int64_t ldY,
                            const float* X, int64_t ldX, const float* D, int64_t ldD, const float* B, int64_t ldB,
                            const float* H0, uint64_t seed, float* B_hat, int64_t ldBh, float* A_hat, int64_t ldA,
                            int32_t* n_iter_out);
/* The same from the two WAVEFORMS, as the reference's function takes them (run_basis_DNMF.m:1): truncation to equal length
 * (:5-9), y = x + d (:10), the three feature sets (:13-34) and the loop on the device -- only audio in, B_hat out.
 * mel != NULL: run_basis_DNMF_Mel.m (mel: mel_M x (fftlength/2+1) ROW-major = mel_matrix(...)', features projected as :21-69,
 * B the Mel exemplar basis).  p->F / p->T must equal the feature rows and snmf_stft_num_frames(sp, min(n_x, n_d)). */
int snmf_run_basis_dnmf_audio_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                  const float* x, int64_t n_x, const float* d, int64_t n_d, const float* mel, int32_t mel_M,
                                  const double* B, int64_t ldB, const double* H0, uint64_t seed, double* B_hat, int64_t ldBh,
                                  double* A_hat, int64_t ldA, int32_t* n_iter_out);
/* run_basis_train.m:58-91 for one event class from its assembled training signal: TF_mag (:60-63; alpha_eta_dd >= 0: TF_DD,
 * :64-67), TF_Mel (:70-78; mel / B_Mel NULL: DFT only), exemplar columns sample_idx (r ZERO-based frame indices -- the wrapper
 * draws them, rng(1); randsample(...), :80-81), and the two full-update solves (:84-91; train_exemplar != 0: none, the exemplars
 * are returned).  V is formed in HBM and never crosses PCIe.  p: F = DFT feature rows, T = frames, r = number of exemplars,
 * solver fields.  B_DFT: F x r, A_DFT: r x T or NULL, B_Mel: (2*splice+1)*mel_M x r, A_Mel: r x T or NULL (all fp64, tight);
 * the post-normalisation (+1e-9, :113-116) and the k-means rank reduction (:118-134) stay with the caller. */
int snmf_run_basis_train_audio_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                   const float* mel, int32_t mel_M, const float* s_full, int64_t n_samples,
                                   const int64_t* sample_idx, int32_t train_exemplar, const double* H0, uint64_t seed,
                                   double* B_DFT, double* A_DFT, double* B_Mel, double* A_Mel, int32_t* n_iter_out);

/* ---- the fp64 mode of the front-end and of the training callers (added within 5) -----------------
 * The entries above take float samples and compute in fp32 whatever the type of the host matrices.  These compute in double
 * from the samples to the dictionaries, as snmf_sparse_nmf_fp64 does for one solve: samples, Mel table, features and factors
 * are double, y = x + d is formed in double, the transform is a double FFT on host-computed double twiddles, every matrix
 * lives in HBM tight and column-major, and every solve runs the kernels of snmf_sparse_nmf_fp64.  Every sum has a fixed order:
 * two calls on one input give the same bits.  One device; there is no _multi_ form.
 *
 * Front-end: arguments and meaning of the _f32 namesakes (host or device buffers), all values double. */
int snmf_stft_features_fp64(snmf_ctx* ctx, const snmf_stft_params* sp, const double* samples, int64_t n_samples,
                            int samples_on_device, double* V_out, int64_t ld, int out_on_device, int32_t* n_frames_out);
int snmf_mel_features_fp64(snmf_ctx* ctx, const double* mel, int32_t M, int32_t n, int32_t K, const double* V, int64_t ldv,
                           int32_t T, double* out, int64_t ldo, int on_device);
/* (the first column comes out as the input's, bit for bit) */
int snmf_tf_dd_fp64(snmf_ctx* ctx, double alpha_eta, int32_t F, int32_t T, const double* X, int64_t ldx, double* out,
                    int64_t ldo, int on_device);
/* The 3-solve loop on formed features: arguments and meaning of snmf_run_basis_dnmf_f64.  Y, X, D are uploaded once each,
 * A_hat never leaves HBM between the solves (solves 2 / 3 take copies of its row blocks as init_h: the solve rescales its
 * init_h, src/sparse_nmf.m:157-159), only B_hat (and A_hat if asked for) comes back.  Bit-identical to three
 * snmf_sparse_nmf_fp64 calls.  H0 == NULL: the Philox stream of snmf_plan_set_h_random written as doubles (its values hold
 * 24 bits: the fp32 entries start from the same numbers).  A non-scalar p->sparsity_kind is SNMF_ERR_DIM. */
int snmf_run_basis_dnmf_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, const double* Y, int64_t ldY,
                             const double* X, int64_t ldX, const double* D, int64_t ldD, const double* B, int64_t ldB,
                             const double* H0, uint64_t seed, double* B_hat, int64_t ldBh, double* A_hat, int64_t ldA,
                             int32_t* n_iter_out);
/* As snmf_run_basis_dnmf_audio_f64 with x, d and mel as doubles (mel != NULL: run_basis_DNMF_Mel.m).  p->F / p->T that do
 * not match the features are SNMF_ERR_DIM. */
int snmf_run_basis_dnmf_audio_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                   const double* x, int64_t n_x, const double* d, int64_t n_d, const double* mel, int32_t mel_M,
                                   const double* B, int64_t ldB, const double* H0, uint64_t seed, double* B_hat, int64_t ldBh,
                                   double* A_hat, int64_t ldA, int32_t* n_iter_out);
/* As snmf_run_basis_train_audio_f64 with s_full and mel as doubles: TF_DD, train_exemplar, both full-update solves (both
 * start from the same H0) and the mel == NULL DFT-only form.  A sparsity vector or matrix is SNMF_ERR_UNSUPPORTED. */
int snmf_run_basis_train_audio_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                    const double* mel, int32_t mel_M, const double* s_full, int64_t n_samples,
                                    const int64_t* sample_idx, int32_t train_exemplar, const double* H0, uint64_t seed,
                                    double* B_DFT, double* A_DFT, double* B_Mel, double* A_Mel, int32_t* n_iter_out);

/* ---- missing-data imputation variants --------------------------------
 * [v_MDI, h, objective] = snmf_mdi(v, Dm, p)     src/snmf_mdi.m:1      (binary observed mask)
 * [v_MDI, h, objective] = snmf_mdi_Sm(v, Sm, p)  src/snmf_mdi_Sm.m:1   (soft mask in [0,1])
 * The same solver with a masked start (:175), a re-imputation of v after every iteration (:251-254)
 * and a gain-matched final imputation (:296-306).  A plan becomes an MDI solve by giving it a mask
 * (F x T, 1 = observed) before snmf_plan_set_v / snmf_plan_init; at least one factor must be updated.
 * The wrappers map p.sparsity_mdi and p.conv_eps_mdi onto the plan's sparsity / conv_eps. */
int snmf_plan_set_mask_f64(snmf_plan* plan, const double* M, int64_t ld, int on_device);
int snmf_plan_set_mask_f32(snmf_plan* plan, const float* M, int64_t ld, int on_device);
/* v_MDI (:296-306) after snmf_plan_run: F x T, observed entries kept, the rest Nt .* max(w*h, flr). */
int snmf_plan_get_v_mdi_f64(snmf_plan* plan, double* V, int64_t ld, int on_device);
int snmf_plan_get_v_mdi_f32(snmf_plan* plan, float* V, int64_t ld, int on_device);
/* The fp64 mode of the missing-data solves (added within ABI 5: a new entry only): src/snmf_mdi.m:163-306 and
 * src/snmf_mdi_Sm.m:163-309 in fp64 from end to end, a one-shot call like snmf_sparse_nmf_fp64 and with its kernels.  The
 * iteration is that entry's (src/sparse_nmf.m:157-286 == src/snmf_mdi.m:163-295) plus three element-wise steps on the mask:
 * the masked start v = max(v .* M, flr) (:175, in the place of the floor of v: p->floor_v is ignored), the re-imputation
 * v = max(v .* M + max(w*h, flr) .* (1 - M), flr) after the W step of EVERY iteration (:251-254 / snmf_mdi_Sm.m:251-260;
 * one pass that also forms the objective of the imputed v, :257-268; with cost_check = 0 the imputation alone), and the
 * gain-matched final imputation (:296-306 / snmf_mdi_Sm.m:302-309): Nt = sum_f(v .* M) ./ max(sum_f(max(w*h, flr) .* M), flr)
 * per frame, V_mdi = max(v .* M + Nt .* max(w*h, flr) .* (1 - M), flr).  A frame without an observed entry has Nt = 0: its
 * entries come out as flr = 1e-9.  After a convergence stop (:281-292) v and w*h are those of the stop iteration.
 *   V, M     F x T (ldV, ldM >= F), never modified; M: 1 = observed, 0 = missing, or a soft mask in [0, 1]
 *   W0, H0   F x r and r x T, tight, read-only (init_w, init_h; :116-140)
 *   sparsity as in snmf_sparse_nmf_fp64 and of all three forms: it carries p.sparsity_mdi, and p->conv_eps p.conv_eps_mdi (:87-93)
 *   V_mdi    F x T (ldVm >= F);  H r x T;  W F x r or NULL;  div_out, cost_out (max_iter doubles each), n_iter_out: or NULL
 * Unlike the fp32 missing-data plan (snmf_plan_set_mask_*) it takes any F, T, r the device memory holds, and a solve with
 * neither factor updated, as the reference does: w*h stays the initial one, the imputation and the gain step run.  A partial
 * w_update_ind works as in snmf_sparse_nmf_fp64; a partial h_update_ind is SNMF_ERR_DIM.  A NULL V, M, W0, H0, V_mdi or H and a
 * leading dimension below F are SNMF_ERR_INVALID, a failed allocation is SNMF_ERR_NOMEM; every device block is freed on every
 * way out and the context stays usable.  Every reduction has a fixed order: two calls on one input give the same bits, and
 * M == 1 everywhere gives the W, H and objective of snmf_sparse_nmf_fp64 bit for bit. */
int snmf_mdi_fp64(snmf_ctx* ctx, const snmf_params* p, const double* V, int64_t ldV, const double* M, int64_t ldM,
                  const double* W0, const double* H0, const double* sparsity, double* V_mdi, int64_t ldVm, double* W,
                  double* H, double* div_out, double* cost_out, int32_t* n_iter_out);

/* ---- online separation loop (BASELINE config 3) -------------------
 * Device-resident replacement of the per-frame function
 *   [x_hat_i, d_hat_i, x_tilde, g] = bnmf_sep_event_RT_IS16(y, l, g, p)   src/bnmf_sep_event_RT_IS16.m:1
 * together with its state g (src/init_buff.m:17-42) and the hop queueing / overlap-add / int16 output of
 * the driver loop src/NTF_sep_event_RT.m:54-135, for the configuration the reference ships
 * (blk_len_sep = 1, Splice = 0, one channel; B_sep_mode 'DFT', or 'Mel' through snmf_online_set_mel).
 * Per frame: STFT -> H-only solve against [B_DFT_x, B_DFT_d] -> reconstructions, block sparsity,
 * adaptive beta, Wiener / MMSE gain -> noise-reference rings and (when triggered) the W-only
 * adaptation solve + dictionary re-assembly -> inverse STFT, overlap-add.  Only PCM in, PCM out and a
 * 32-byte status per frame cross PCIe. */
typedef struct snmf_online snmf_online;

typedef struct snmf_online_params {
    /* signal (settings/initial_setting_SNMF_NAT.m:21-37,53,88-92) */
    int32_t fftlength, framelength, frameshift;
    int32_t dcbin, dcbin_back;
    int32_t delay;            /* p.delay: frames before the first hop is written */
    double preemph, pow, nonzerofloor, overlapscale;
    /* dictionaries */
    int32_t R_x, R_d;
    /* per-frame and adaptation solves (src/sparse_nmf.m parameters) */
    double beta_div;          /* 1 = 'kl', 2 = 'ed', 0 = 'is' */
    double sparsity;
    int32_t max_iter, cost_check;
    double conv_eps;
    /* enhancement filter (:221-261) */
    int32_t enhance_method;   /* 0 = 'Wiener', 1 = 'MMSE' */
    int32_t init_N_len;
    double alpha_eta, alpha_d, beta, beta_max;
    /* block sparsity (src/blk_sparse.m) */
    int32_t blk_sparse, P_len_k, P_len_l, blk_gap;
    double alpha_p;
    /* noise dictionary adaptation (:263-347) */
    int32_t adapt_train_N, R_a, m_a;
    double overlap_m_a, Ar_up;
    int32_t class_outputs;    /* also synthesise the event / noise estimates (x_hat, d_hat) */
    /* semi-supervised frame solve (:125-139): the frame solve also updates the noise (N) or the event (E)
     * columns of its private copy of W; only the activations are used afterwards, as in the reference */
    int32_t basis_update_N, basis_update_E;
} snmf_online_params;

typedef struct snmf_online_frame {   /* per-frame diagnostics, in frame order */
    int32_t n_iter;           /* iterations of the frame solve */
    int32_t trig;             /* adaptation condition :266 */
    int32_t solved;           /* an adaptation solve ran */
    int32_t n_up;             /* sum(r_up) */
    int32_t adapt_iters;      /* iterations of the adaptation solve */
    float beta, A_x_mag, A_d_mag, Q_control;
} snmf_online_frame;

/* B_DFT_x: F x R_x, B_DFT_d: F x R_d (column-major, F = fftlength/2+1); H0: r values standing in for
 * rand(r,1) of src/sparse_nmf.m:133-134 (the same vector every frame, as the reference re-seeds per call);
 * Ad_blk0: R_a x m_a standing in for rand(R_a, m_a) of src/init_buff.m:39; windows: framelength values. */
int snmf_online_create(snmf_ctx* ctx, const snmf_online_params* p, const float* B_DFT_x, const float* B_DFT_d,
                       const float* H0, const float* Ad_blk0, const float* win_stft, const float* win_istft,
                       snmf_online** out);
/* B_sep_mode = 'Mel' (src/bnmf_sep_event_RT_IS16.m:106-120; src/init_buff.m:45-47): call once right after create.
 * melmat: F_order x F ROW-major (g.melmat = mel_matrix(fs, F_order, fftlength, 1, fs/2)'); B_Mel_x / B_Mel_d:
 * F_order x R_x / R_d column-major.  mel_conv = p.MelConv (0: Mel activations on the DFT bases). */
int snmf_online_set_mel(snmf_online* o, int32_t F_order, int32_t mel_conv, const float* melmat, const float* B_Mel_x,
                        const float* B_Mel_d);
/* Current B_Mel_d (Mel mode adapts this one; B_DFT_d stays). */
int snmf_online_get_mel_basis_f32(snmf_online* o, float* B_Mel_d, int64_t ld);
/* Feed n PCM samples (int16-valued floats); every complete hop becomes a frame.  flush != 0 ends the
 * stream the way the driver does at end of file (delay+1 all-zero frames, src/NTF_sep_event_RT.m:69-76).
 * Outputs (host, each may be NULL): the denoised signal before rounding, the int16 the driver writes, and
 * with class_outputs the event / noise estimates; capacity `cap` samples each, *n_out samples written
 * (at most (n/frameshift + delay + 2) * frameshift). */
int snmf_online_process_f32(snmf_online* o, const float* pcm, int64_t n, int flush, float* x_tilde_f32,
                            int16_t* x_tilde_i16, float* x_hat_f32, float* d_hat_f32, int64_t cap, int64_t* n_out);
/* Current B_DFT_d (what src/NTF_sep_event_RT.m:138-140 saves to B_D_u.mat). */
int snmf_online_get_basis_f32(snmf_online* o, float* B_DFT_d, int64_t ld);
/* Diagnostics of the most recent frames: the separator keeps a ring of the newest 65536 frames (a real-time stream
 * runs unbounded); copies the oldest min(cap, *n) of them in order, *n = frames held (= all frames for shorter runs). */
int snmf_online_trace(snmf_online* o, snmf_online_frame* out, int64_t cap, int64_t* n);
void snmf_online_destroy(snmf_online* o);
/* Added within 5.  The fp64 mode of the separator.  The loop is a feedback system (activations -> adapted noise
 * dictionary -> next activations) that amplifies a perturbation about tenfold per 100 frames, so the fp32 path leaves the
 * fp64 reference's trajectory after a few hundred frames (docs/WIDENING.md, "Parity horizon").  A separator made here takes
 * every input in fp64 and keeps every step from PCM to the fed-back state in fp64 (transforms, frame solve, post-filter
 * state, adaptation solve, synthesis); it holds the reference's per-frame decisions over whole recordings.
 * Scope: B_sep_mode 'DFT' and the supervised frame solve, every other field of snmf_online_params.  basis_update_N /
 * basis_update_E here, and snmf_online_set_mel on such a separator, return SNMF_ERR_UNSUPPORTED; so does a geometry whose
 * adaptation solve does not fit one cooperative launch (fftlength > 1024 or R_a > 64 with adapt_train_N set).
 * snmf_online_process_f32 on it runs the fp64 path and rounds the float outputs; snmf_online_trace,
 * snmf_online_get_basis_f32 and snmf_online_destroy work on both kinds. */
int snmf_online_create_f64(snmf_ctx* ctx, const snmf_online_params* p, const double* B_DFT_x, const double* B_DFT_d,
                           const double* H0, const double* Ad_blk0, const double* win_stft, const double* win_istft,
                           snmf_online** out);
/* Added within 5.  snmf_online_process_f32 with fp64 samples in and out (pcm: int16-valued doubles); the int16 stream is
 * the fp64 value rounded half away from zero.  SNMF_ERR_STATE on a separator made by snmf_online_create. */
int snmf_online_process_f64(snmf_online* o, const double* pcm, int64_t n, int flush, double* x_tilde_f64,
                            int16_t* x_tilde_i16, double* x_hat_f64, double* d_hat_f64, int64_t cap, int64_t* n_out);
/* Added within 5.  The fp64 master of the current B_DFT_d; both kinds of separator hold one. */
int snmf_online_get_basis_f64(snmf_online* o, double* B_DFT_d, int64_t ld);
/* Added within 5.  The per-class estimates x_hat_i / d_hat_i, the first two results of
 * [x_hat_i, d_hat_i, x_tilde, g] = bnmf_sep_event_RT_IS16(y, l, g, p): p.EVENT_NUM / p.EVENT_RANK / p.NOISE_NUM / p.NOISE_RANK
 * (settings/initial_setting_SNMF_NAT.m:40-44) cut the two dictionaries into classes of consecutive columns.  Ranks are the
 * reference's 1-based starts: event class i covers columns event_rank[i] .. event_rank[i+1]-1 of B_x, the last one up to R_x,
 * and noise class i the same of B_d (src/bnmf_sep_event_RT_IS16.m:158-163, :180-185).  Per frame the class spectrum is
 * B_DFT(:,R_i) * A(R_i) -- 'Mel' with MelConv = 1: melmat' * (B_Mel(:,R_i) * A(R_i)), :165-171, :187-195 -- from the frame's
 * activations and the dictionary the frame solve saw (:141), before this frame's adaptation replaces it (:336); a
 * semi-supervised solve's private W is not used.  The class signal is synth_ifft_buff of it times overlapscale (:350-361),
 * overlap-added as x_hat / d_hat are (src/NTF_sep_event_RT.m:112-126): the gain does not touch it and no frame is gated.
 * The sums over the classes are x_hat's and d_hat's spectra, so x_tilde, the adaptation and every decision stay as they are.
 * Works on separators of both precisions; call after create, before or after snmf_online_set_mel, before the first sample.
 *   SNMF_ERR_STATE        a separator created without class_outputs; samples were already fed
 *   SNMF_ERR_INVALID      a count below 1, a rank below 1, ranks not strictly ascending, a last start above R_x / R_d
 *   SNMF_ERR_UNSUPPORTED  a first rank above 1 (Xm_hat_sum, the sum over the classes, feeds the gain, :201: the reference would
 *                         silently drop the leading columns from the filter); more than 32 classes on a side; 'Mel' with
 *                         MelConv = 1 when (event_num + noise_num) * F_order floats exceed a workgroup's LDS */
int snmf_online_set_classes(snmf_online* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num,
                            const int32_t* noise_rank);
/* Added within 5.  snmf_online_process_f32 / _f64 plus the class signals: x_hat_i event_num x cap and d_hat_i noise_num x cap,
 * class-major (class i at x_hat_i + i * cap), *n_out samples written per class.  Either may be NULL.  Without
 * snmf_online_set_classes there is one class per side: x_hat_i = x_hat, d_hat_i = d_hat.  The plain process entries keep
 * working on a separator that has classes; they do not return them. */
int snmf_online_process_classes_f32(snmf_online* o, const float* pcm, int64_t n, int flush, float* x_tilde_f32,
                                    int16_t* x_tilde_i16, float* x_hat_f32, float* d_hat_f32, float* x_hat_i_f32,
                                    float* d_hat_i_f32, int64_t cap, int64_t* n_out);
int snmf_online_process_classes_f64(snmf_online* o, const double* pcm, int64_t n, int flush, double* x_tilde_f64,
                                    int16_t* x_tilde_i16, double* x_hat_f64, double* d_hat_f64, double* x_hat_i_f64,
                                    double* d_hat_i_f64, int64_t cap, int64_t* n_out);

/* ---- batched online separation: S independent streams per launch ------------------------
 * The reference's real workload enhances many recordings, each an independent chain of the per-frame function
 * with its own adapted dictionary (Do_MultiBatch_IS16_20160324.m:178-205: one NTF_sep_event_RT per noise type x SNR,
 * B_D_u.mat deleted between the chains at :187).  Here S such chains share one snmf_online_params and advance frame by
 * frame in shared launches, with no host round trip per frame: stream k has its own PCM, its own noise dictionary and
 * its own state g (src/init_buff.m:17-42), and its output equals what snmf_online_* produces for it alone.
 * Scope: B_sep_mode 'DFT', or 'Mel' through snmf_online_batch_set_mel; the supervised frame solve of the register-resident
 * frame kernel (F <= 513, R_x + R_d <= 200), R_a and m_a <= 128; anything else returns SNMF_ERR_UNSUPPORTED.
 * snmf_online_batch_create_f64 makes the same batch in fp64 (DFT mode; its own envelope is given there). */
typedef struct snmf_online_batch snmf_online_batch;
/* src/init_buff.m for S streams.  B_DFT_x: F x R_x, shared; B_DFT_d0: F x R_d x S, the initial noise dictionary of
 * every stream (e.g. each stream's B_D_u.mat, src/NTF_sep_event_RT.m:27-31); H0: r x S (rand(r,1) of
 * src/sparse_nmf.m:133-134 per stream); Ad_blk0: R_a x m_a x S (rand(R_a, m_a) of src/init_buff.m:39 per stream);
 * the windows are shared.  All column-major. */
int snmf_online_batch_create(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const float* B_DFT_x,
                             const float* B_DFT_d0, const float* H0, const float* Ad_blk0, const float* win_stft,
                             const float* win_istft, snmf_online_batch** out);
/* The driver loop of src/NTF_sep_event_RT.m:54-135 for every stream, as snmf_online_process_f32 per stream: pcm[k] holds
 * n[k] samples of stream k (n[k] may be 0); flush (may be NULL) ends stream k where flush[k] != 0.  Outputs are arrays
 * of S host pointers (each array and each entry may be NULL), capacity cap[k] samples; n_out[k] samples written. */
int snmf_online_batch_process_f32(snmf_online_batch* b, const float* const* pcm, const int64_t* n, const int32_t* flush,
                                  float* const* x_tilde_f32, int16_t* const* x_tilde_i16, float* const* x_hat_f32,
                                  float* const* d_hat_f32, const int64_t* cap, int64_t* n_out);
/* Current B_DFT_d of stream k (src/NTF_sep_event_RT.m:138-140). */
int snmf_online_batch_get_basis_f32(snmf_online_batch* b, int32_t k, float* B_DFT_d, int64_t ld);
/* Added within 5.  src/NTF_sep_event_RT.m:27-38 + init_buff for the streams slots[0..n) (distinct): each starts a new
 * recording, as Do_MultiBatch_IS16_20160324.m:183-205 runs file after file.  Every piece of the stream's state returns to
 * what snmf_online_batch_create gives a stream with these inputs (rings, smoothed statistics, overlap-add tails, the
 * dictionary images; the host queue, history, frame count and trace are cleared).
 * B_DFT_d: F x R_d x n column-major fp64, or NULL = keep each stream's current (adapted) dictionary, i.e.
 *          load('B_D_u.mat'); the fp64 master is kept as it is, without an fp32 round trip.  A new dictionary also
 *          becomes the stream's fixed columns (B_Mel_d in DFT mode, src/bnmf_sep_event_RT_IS16.m:328); a carry keeps them.
 * H0: r x n, Ad_blk0: R_a x m_a x n, or NULL = the values the stream last started with.
 * A stream that has consumed samples and has not been flushed returns SNMF_ERR_STATE, and so does a failed batch; a
 * stream that has never been fed may be restarted.  The other streams do not change.  Ordered on the context's stream
 * before the next process call; no synchronise beyond the uploads.
 * On a Mel-mode batch this is exactly snmf_online_batch_restart_mel with B_Mel_d = NULL (each stream keeps its B_Mel_d). */
int snmf_online_batch_restart(snmf_online_batch* b, int32_t n, const int32_t* slots, const double* B_DFT_d,
                              const float* H0, const float* Ad_blk0);
/* Added within 5.  Stream k's fp64 master of B_DFT_d (what a carry by snmf_online_batch_restart keeps). */
int snmf_online_batch_get_basis_f64(snmf_online_batch* b, int32_t k, double* B_DFT_d, int64_t ld);
/* Added within 5.  B_sep_mode = 'Mel' for every stream (src/bnmf_sep_event_RT_IS16.m:106-120, :165-171, :205-211, :298-318),
 * as snmf_online_set_mel: call after create and before the first process call (after it: SNMF_ERR_STATE).
 * melmat: F_order x F ROW-major, shared; B_Mel_x: F_order x R_x, shared; B_Mel_d: F_order x R_d x S, every stream's start
 * (column-major per stream, streams consecutive, fp32).  F_order outside [2, F] or a NULL argument: SNMF_ERR_INVALID.
 * The frame solve runs at F_order rows on [B_Mel_x | B_Mel_d] and the adaptation updates B_Mel_d (its fp64 master);
 * B_DFT_d is never adapted.  mel_conv = p.MelConv (0: the Mel activations drive the stream's B_DFT bases).  Every stream
 * restarts with its B_Mel_d and keeps its B_DFT_d, H0 and Ad_blk0. */
int snmf_online_batch_set_mel(snmf_online_batch* b, int32_t F_order, int32_t mel_conv, const float* melmat, const float* B_Mel_x,
                              const float* B_Mel_d);
/* Added within 5.  snmf_online_batch_restart with the Mel dictionary too (src/NTF_sep_event_RT.m:27-38, :137-139 save and
 * load both): B_Mel_d F_order x R_d x n column-major fp64, or NULL = keep each stream's current fp64 master (no fp32 round
 * trip).  A non-NULL B_Mel_d on a batch that is not in Mel mode returns SNMF_ERR_STATE. */
int snmf_online_batch_restart_mel(snmf_online_batch* b, int32_t n, const int32_t* slots, const double* B_DFT_d,
                                  const double* B_Mel_d, const float* H0, const float* Ad_blk0);
/* Added within 5.  Stream k's current B_Mel_d (F_order x R_d; f64: the master a carry keeps).  SNMF_ERR_STATE when the
 * batch is not in Mel mode. */
int snmf_online_batch_get_mel_basis_f32(snmf_online_batch* b, int32_t k, float* B_Mel_d, int64_t ld);
int snmf_online_batch_get_mel_basis_f64(snmf_online_batch* b, int32_t k, double* B_Mel_d, int64_t ld);
/* Added within 5.  snmf_online_set_classes for the batch: ONE partition for all streams (the settings are shared), same
 * semantics and status codes.  Call after create, before or after snmf_online_batch_set_mel, before the first process call
 * (after it: SNMF_ERR_STATE; so does a batch created without class_outputs).  snmf_online_batch_restart also resets the
 * listed streams' class overlap-add tails, like those of x_hat / d_hat. */
int snmf_online_batch_set_classes(snmf_online_batch* b, int32_t event_num, const int32_t* event_rank, int32_t noise_num,
                                  const int32_t* noise_rank);
/* Added within 5.  snmf_online_batch_process_f32 plus the class signals: x_hat_i_f32 / d_hat_i_f32 are arrays of S host
 * pointers (each array and each entry may be NULL) to event_num x cap[k] / noise_num x cap[k] floats, class-major.  A
 * stream's class signals do not depend on the other streams of the batch.  Without
 * snmf_online_batch_set_classes there is one class per side (x_hat / d_hat). */
int snmf_online_batch_process_classes_f32(snmf_online_batch* b, const float* const* pcm, const int64_t* n, const int32_t* flush,
                                          float* const* x_tilde_f32, int16_t* const* x_tilde_i16, float* const* x_hat_f32,
                                          float* const* d_hat_f32, float* const* x_hat_i_f32, float* const* d_hat_i_f32,
                                          const int64_t* cap, int64_t* n_out);
/* Added within 5.  The fp64 mode of the batch: snmf_online_create_f64 for S streams.  Every array crosses in fp64 (layouts as
 * snmf_online_batch_create) and every step from PCM to each stream's fed-back dictionary runs in fp64 on the device, so every
 * stream holds the fp64 reference's per-frame decisions over whole recordings and chains of recordings.  Same handle type,
 * same destroy.  Scope: B_sep_mode 'DFT', the supervised frame solve, every beta_div, Wiener / MMSE, block sparsity,
 * adaptation on or off, class outputs, restart.  SNMF_ERR_UNSUPPORTED: basis_update_N / basis_update_E; with adaptation
 * R_a > 64, m_a > 128 or a ring whose LDS image exceeds a compute unit's (the message names the limit); a transform or
 * dictionary whose frame solve does not fit the LDS.
 * On such a batch snmf_online_batch_restart (H0 / Ad_blk0 widened from fp32), _get_basis_f64, _set_classes and _trace work as
 * on an fp32 batch; snmf_online_batch_get_basis_f32 returns the fp64 dictionary rounded; snmf_online_batch_set_mel,
 * _restart_mel and _get_mel_basis_* return SNMF_ERR_UNSUPPORTED; snmf_online_batch_process_f32 /
 * _process_classes_f32 return SNMF_ERR_STATE with n_out zeroed, as the _f64 process entries do on an fp32 batch.  A refused
 * call leaves the handle usable. */
int snmf_online_batch_create_f64(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* B_DFT_x,
                                 const double* B_DFT_d0, const double* H0, const double* Ad_blk0, const double* win_stft,
                                 const double* win_istft, snmf_online_batch** out);
/* Added within 5.  snmf_online_batch_process_f32 / _process_classes_f32 of an fp64 batch: fp64 PCM and outputs; the int16
 * stream is the fp64 value rounded half away from zero. */
int snmf_online_batch_process_f64(snmf_online_batch* b, const double* const* pcm, const int64_t* n, const int32_t* flush,
                                  double* const* x_tilde_f64, int16_t* const* x_tilde_i16, double* const* x_hat_f64,
                                  double* const* d_hat_f64, const int64_t* cap, int64_t* n_out);
int snmf_online_batch_process_classes_f64(snmf_online_batch* b, const double* const* pcm, const int64_t* n, const int32_t* flush,
                                          double* const* x_tilde_f64, int16_t* const* x_tilde_i16, double* const* x_hat_f64,
                                          double* const* d_hat_f64, double* const* x_hat_i_f64, double* const* d_hat_i_f64,
                                          const int64_t* cap, int64_t* n_out);
/* Added within 5.  snmf_online_batch_restart of an fp64 batch with H0 (r x n) and Ad_blk0 (R_a x m_a x n) in fp64, so that a
 * new recording starts from exactly the draws its fp64 reference run uses.  SNMF_ERR_STATE on an fp32 batch. */
int snmf_online_batch_restart_f64(snmf_online_batch* b, int32_t n, const int32_t* slots, const double* B_DFT_d, const double* H0,
                                  const double* Ad_blk0);
/* Added within 5.  Settings and an event dictionary of its own for every stream of an fp64 batch: the consumer of the pairs
 * (B_x, B_d) that snmf_run_basis_dnmf_batch_fp64 re-trains per noise type, and of the reference's comparison runs, which
 * enhance one corpus under several settings files (adapt_train_N, sparsity, max_iter, Wiener / MMSE, alpha_eta, alpha_d, beta).
 * snmf_online_stream_settings holds, in the units of snmf_online_params, the fields a stream may have of its own; everything
 * else of snmf_online_params is the batch's geometry and stays shared: the transform and windows, delay, DCbin(_back), preemph,
 * pow, nonzerofloor, R_x, R_d, R_a, m_a, P_len_l, cost_check, class_outputs and the class partition. */
typedef struct snmf_online_stream_settings {
    double beta_div, sparsity, conv_eps;
    int32_t max_iter;
    int32_t enhance_method, init_N_len;
    double alpha_eta, alpha_d, beta, beta_max;
    int32_t blk_sparse, P_len_k, blk_gap;
    double alpha_p;
    int32_t adapt_train_N;
    double overlap_m_a, Ar_up;
} snmf_online_stream_settings;
/* snmf_online_batch_create_f64 with B_DFT_x F x R_x x S (stream k's event dictionary at k * F * R_x) and settings[S]
 * (NULL: p's for every stream; p's own values of these fields are then the only ones used).  Every entry is checked like p
 * itself, on the shared geometry, with the same status codes.  The rings exist when any stream needs them (P_len_l columns
 * with a block-sparse stream, R_a x m_a with an adapting one); Ad_blk0 (R_a x m_a x S) is required when any stream adapts, and
 * the entries of streams that do not are not used.  The ring envelope of snmf_online_batch_create_f64 is checked for every
 * divergence (beta_div 1, 2, other) that an adapting stream uses.  Stream k's outputs, trace and dictionary are bit for bit
 * those of a batch of one created by snmf_online_batch_create_f64 with its dictionary pair and its settings in p. */
int snmf_online_batch_create_streams_f64(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* B_DFT_x,
                                         const double* B_DFT_d0, const double* H0, const double* Ad_blk0,
                                         const snmf_online_stream_settings* settings, const double* win_stft,
                                         const double* win_istft, snmf_online_batch** out);
/* snmf_online_batch_restart_f64 that may also give the listed streams another event dictionary (B_DFT_x F x R_x x n, NULL:
 * each keeps its own) and other settings (settings[n], NULL: each keeps its own).  A stream that adapts after the call needs
 * an Ad_blk0, here or from an earlier call (SNMF_ERR_INVALID otherwise).  A refused call leaves the batch as it was.
 * SNMF_ERR_STATE on an fp32 batch. */
int snmf_online_batch_restart_streams_f64(snmf_online_batch* b, int32_t n, const int32_t* slots, const double* B_DFT_x,
                                          const double* B_DFT_d, const double* H0, const double* Ad_blk0,
                                          const snmf_online_stream_settings* settings);
/* Stream k's settings as they were last given (p's for a batch made by snmf_online_batch_create_f64).  SNMF_ERR_STATE on an
 * fp32 batch. */
int snmf_online_batch_get_settings(snmf_online_batch* b, int32_t k, snmf_online_stream_settings* out);
/* Added within 5.  A stream's state g as a value the caller holds: the fourth result of
 * [x_hat_i, d_hat_i, x_tilde, g] = bnmf_sep_event_RT_IS16(y, l, g, p) (src/init_buff.m:17-47,
 * src/bnmf_sep_event_RT_IS16.m:385-420) together with the driver's variables around it (the frame buffer, the samples not
 * yet framed, the overlap-add tails).  One stream's state is one RECORD of info.bytes bytes: a header (magic, layout
 * version, the snmf_online_state_info it was taken under, so that a record on disk describes itself) and the fields of
 * snmf_online_state_field_id behind it, each at the offset snmf_online_state_field reports.  Float fields have the batch's
 * element type (float on an fp32 batch, double on an fp64 batch); the dictionary masters are double on both.  Matrices
 * are column-major and tight.  Rings stand in the reference's order, oldest column first, as lambda_d_blk and Ad_blk stand
 * after the shift-and-append of :282, :285 and r_blk as src/blk_sparse.m returns it; the device keeps column c of a ring in
 * slot (n_push + c) % m_a (r_blk: (l - 1 + c) % P_len_l), and a restored stream has its columns in the slots they had.
 * Not state: B_DFT_x, the per-stream settings, the class partition and the windows (configuration: the target slot has
 * them already, from create or restart); the trace; r_up and every derived dictionary image (rebuilt from the masters). */
#define SNMF_ONLINE_STATE_MAGIC 0x47534E4Fu /* "ONSG" */
#define SNMF_ONLINE_STATE_VERSION 1
typedef struct snmf_online_state_info {
    int32_t elem_size;     /* 4: fp32 batch, 8: fp64 batch */
    int32_t mel, mel_conv; /* B_sep_mode 'Mel', MelConv */
    int32_t F, F_order;    /* F_order: 0 outside Mel mode */
    int32_t R_x, R_d, R_a, m_a, P_len_l; /* R_a, m_a, P_len_l: the rings as the batch holds them (1 where unused) */
    int32_t framelength, frameshift, ntail;
    int32_t class_outputs, n_classes;
    int32_t reserved;
    int64_t bytes;         /* of one record */
} snmf_online_state_info;
typedef enum snmf_online_state_field_id {
    SNMF_STATE_XM_TILDE = 0,  /* F                       g.Xm_tilde */
    SNMF_STATE_LAMBDA_DAV,    /* F                       g.lambda_dav */
    SNMF_STATE_R_BLK,         /* F x P_len_l             g.r_blk */
    SNMF_STATE_LAMBDA_D_BLK,  /* F x m_a                 g.lambda_d_blk, time order */
    SNMF_STATE_AD_BLK,        /* R_a x m_a               g.Ad_blk, time order */
    SNMF_STATE_N_PUSH,        /* int32                   pushes into the two rings so far */
    SNMF_STATE_UPDATE_SWITCH, /* int32                   g.update_switch */
    SNMF_STATE_B_DFT_D,       /* F x R_d double          the fp64 master */
    SNMF_STATE_B_FIX,         /* F x R_d double          the fixed columns of :328 */
    SNMF_STATE_B_MEL_D,       /* F_order x R_d double    Mel mode: the adapted master (count 0 otherwise) */
    SNMF_STATE_H0,            /* R_x + R_d               the stream's draw */
    SNMF_STATE_AD_BLK0,       /* R_a x m_a               the stream's draw (a later carry-restart reuses it) */
    SNMF_STATE_L,             /* int64                   1-based index of the next frame */
    SNMF_STATE_Y_HIST,        /* framelength - frameshift   the driver's frame buffer behind the last hop */
    SNMF_STATE_PENDING,       /* frameshift (capacity)   samples fed but not yet framed; the first PENDING_COUNT hold */
    SNMF_STATE_PENDING_COUNT, /* int32                   < frameshift */
    SNMF_STATE_X_TILDE_TAIL,  /* ntail                   the overlap-add tail: the last nov - 1 synthesised frames (framelength
                                                          each, oldest first; nov = ceil(framelength / frameshift)), which the
                                                          overlap-add of src/NTF_sep_event_RT.m:121-124 sums */
    SNMF_STATE_X_HAT_TAIL,    /* ntail                   with class_outputs (count 0 otherwise) */
    SNMF_STATE_D_HAT_TAIL,    /* ntail                   with class_outputs */
    SNMF_STATE_CLASS_TAILS,   /* ntail x n_classes       with a partition set */
    SNMF_STATE_FIELD_COUNT
} snmf_online_state_field_id;
typedef enum snmf_online_state_type { SNMF_STATE_F32 = 0, SNMF_STATE_F64 = 1, SNMF_STATE_I32 = 2, SNMF_STATE_I64 = 3 } snmf_online_state_type;
/* The geometry and record size of the batch's streams, as they are now (snmf_online_batch_set_mel / _set_classes and, on an
 * fp64 batch, a restart that makes the rings grow change them). */
int snmf_online_batch_state_info(snmf_online_batch* b, snmf_online_state_info* out);
/* Where `field` (an snmf_online_state_field_id) lies in a record taken under `info`: byte offset, element count and element type.  A pure host function:
 * it reads nothing but `info` (its `bytes` included: it is recomputed, and returned through info only by
 * snmf_online_batch_state_info).  Any of offset / count / type may be NULL.  An unknown field or a nonsensical info:
 * SNMF_ERR_INVALID. */
int snmf_online_state_field(const snmf_online_state_info* info, int32_t field, int64_t* offset, int64_t* count, int32_t* type);
/* The records of the streams slots[0..n) (distinct), consecutive, info.bytes each, into `records` (cap bytes).  Allowed
 * between process calls on a stream that was not flushed; a flushed stream returns SNMF_ERR_STATE (what survives it is the
 * dictionary, snmf_online_batch_get_basis_f64).  The streams are not disturbed.  One gather launch and one copy, whatever n. */
int snmf_online_batch_get_state(snmf_online_batch* b, int32_t n, const int32_t* slots, void* records, int64_t cap);
/* Streams slots[0..n) (distinct) take the n consecutive records in `records` (bytes in all).  Allowed on any slot, fresh,
 * running or finished; the slot is then a running stream at frame l with an empty trace (the batch counts as started:
 * snmf_online_batch_set_mel / _set_classes come before, as before the first process call).  The headers are checked against
 * the handle before the device is touched: bad magic or version, or too few bytes: SNMF_ERR_INVALID; another element size,
 * mode, geometry or class count: SNMF_ERR_DIM (the message names the field); n_push < 0, update_switch < 1, l < 1 or a
 * pending count >= frameshift: SNMF_ERR_INVALID.  A refused call changes nothing.  One upload, one scatter launch and the
 * dictionary refresh of a restart, whatever n; the stream's next frames have the bits of the stream the record came from. */
int snmf_online_batch_set_state(snmf_online_batch* b, int32_t n, const int32_t* slots, const void* records, int64_t bytes);
/* Added within 5.  The output capacity that holds one flushed recording of n_samples fed in any number of calls:
 * (n_samples / frameshift + delay + 3) * frameshift samples.  A pure function of the handle's settings; a NULL handle or a
 * negative n_samples gives 0. */
int64_t snmf_online_batch_out_capacity(const snmf_online_batch* b, int64_t n_samples);
/* Added within 5.  A corpus on the batch: the per-target loop of Do_MultiBatch_IS16_20160324.m:183-205 with
 * run_ntf_sep_RT.m:10-41 inside it.  A CHAIN is a list of recordings enhanced in turn by src/NTF_sep_event_RT.m: its first
 * file starts from the chain's B_DFT_d (the delete('B_D_u.mat') of :187) and every later file from the dictionary its
 * predecessor adapted, carried on the device in fp64.  The S streams of `b` are slots that take chains from a queue in
 * chain order; a slot whose file ended is restarted before it is fed again, as snmf_online_batch_restart with all-NULL
 * arrays for the next file of its chain and with the next chain's dictionary and draws for a new chain.  Chain c uses its
 * own H0 / Ad_blk0 for all its files.  With fewer chains than slots the spare slots are never touched; a chain without
 * files gives no outputs.  Every file's signals and final dictionary are bit for bit those of the same sequence of
 * restart / process calls made by hand on one stream, and depend neither on S, chunk_hops, the slot nor the other chains.
 * Files are numbered in chain order: file j of chain c is entry n_files[0] + ... + n_files[c - 1] + j of every per-file array.
 *   n_chains, n_files[n_chains]          chains and files per chain (0 allowed)
 *   pcm[i], n_samples[i]                 file i's samples (float for _f32, double for _f64; pcm[i] may be NULL when n_samples[i] is 0)
 *   B_DFT_d    F x R_d x n_chains        every chain's start dictionary, fp64, as snmf_online_batch_restart takes it
 *   B_Mel_d    F_order x R_d x n_chains  Mel batch: every chain's start B_Mel_d (required there; elsewhere NULL, otherwise SNMF_ERR_STATE)
 *   H0         r x n_chains              float for _f32, double for _f64, as the restart entries take them
 *   Ad_blk0    R_a x m_a x n_chains      likewise; required only when the batch adapts
 *   chunk_hops                           hops fed to every busy slot per internal process call; 0 = one device chunk
 *                                        (16384 / S hops, at least 1, at most 4096).  It changes no bit of the result.  Any
 *                                        larger value is fine: more than the longest file holds means whole files per call,
 *                                        and the driver's buffers are sized by the files, never by this number.
 * Outputs, per file; each array and each entry may be NULL:
 *   x_tilde_i16[i], x_tilde_f[i]         the enhanced signal, capacity cap[i] samples each (snmf_online_batch_out_capacity
 *                                        suffices; less than (n_samples[i] / frameshift + delay + 1) * frameshift is SNMF_ERR_INVALID)
 *   n_out[i]                             samples written for file i
 *   B_out[i]                             the dictionary after file i, tight, fp64: the master snmf_online_batch_get_basis_f64
 *                                        returns (F x R_d), on a Mel batch the one of _get_mel_basis_f64 (F_order x R_d)
 * On a batch with class outputs only x_tilde is written.  Everything is checked before the device is touched:
 * SNMF_ERR_INVALID for a NULL handle, NULL or inconsistent counts and arrays; SNMF_ERR_STATE (every n_out zeroed) for the
 * entry of the other precision, for a failed batch and for a batch with a stream that has consumed samples and was not
 * flushed -- the handle stays usable; SNMF_ERR_UNSUPPORTED on a batch with settings or event dictionaries per stream
 * (snmf_online_batch_create_streams_f64, or snmf_online_batch_restart_streams_f64 with either): chains with settings of
 * their own stay with the caller's own loop over restart_streams_f64 for now.  After SNMF_OK every used stream is flushed:
 * the handle runs another corpus or is driven by hand.  An error of a restart or process call inside the run is returned
 * as it is; n_out then holds the files that were finished. */
int snmf_online_batch_run_chains_f32(snmf_online_batch* b, int32_t n_chains, const int32_t* n_files, const float* const* pcm,
                                     const int64_t* n_samples, const double* B_DFT_d, const double* B_Mel_d, const float* H0,
                                     const float* Ad_blk0, int32_t chunk_hops, int16_t* const* x_tilde_i16, float* const* x_tilde_f32,
                                     const int64_t* cap, int64_t* n_out, double* const* B_out);
int snmf_online_batch_run_chains_f64(snmf_online_batch* b, int32_t n_chains, const int32_t* n_files, const double* const* pcm,
                                     const int64_t* n_samples, const double* B_DFT_d, const double* B_Mel_d, const double* H0,
                                     const double* Ad_blk0, int32_t chunk_hops, int16_t* const* x_tilde_i16, double* const* x_tilde_f64,
                                     const int64_t* cap, int64_t* n_out, double* const* B_out);
/* Diagnostics of stream k's most recent frames (the newest 65536 per stream), as snmf_online_trace. */
int snmf_online_batch_trace(snmf_online_batch* b, int32_t k, snmf_online_frame* out, int64_t cap, int64_t* n);
void snmf_online_batch_destroy(snmf_online_batch* b);

/* ---- the single-stream separator (snmf_online): its state g as a record, and its next file in place ----
 * Declared here because the record is the one above: the same snmf_online_state_info, the same fields at the offsets
 * snmf_online_state_field reports, SNMF_ONLINE_STATE_VERSION 1.  A record taken from either kind of separator is accepted
 * by the other of the same configuration (precision, mode, geometry, class count). */
/* Added within 5.  The geometry and record size of this separator as it is now (after snmf_online_set_mel /
 * snmf_online_set_classes), field by field what snmf_online_batch_state_info reports for a batch of its configuration:
 * R_a, m_a and P_len_l are 1 where unused, elem_size is 4 (snmf_online_create) or 8 (snmf_online_create_f64), F_order is 0
 * outside Mel mode. */
int snmf_online_stream_state_info(snmf_online* o, snmf_online_state_info* out);
/* Added within 5.  One record of info.bytes into `record` (cap bytes).  Allowed between process calls, also before the
 * first one; a flushed separator or one whose earlier call failed returns SNMF_ERR_STATE.  The separator is not disturbed.
 * One gather launch and one copy. */
int snmf_online_get_state(snmf_online* o, void* record, int64_t cap);
/* Added within 5.  The separator takes the record (`bytes` long).  Allowed on a fresh, running or finished separator; it is
 * then a running stream at frame l with an empty trace, and its next frames have the bits of the stream the record came
 * from.  The header checks and their status codes are those of snmf_online_batch_set_state: bad magic or version, or too
 * few bytes: SNMF_ERR_INVALID; another element size, mode, geometry or class count: SNMF_ERR_DIM (the message names the
 * field); n_push < 0, update_switch < 1, l < 1 or a pending count >= frameshift: SNMF_ERR_INVALID; a separator whose earlier
 * call failed: SNMF_ERR_STATE.  A refused call changes nothing.  One upload, one scatter launch and the dictionary refresh
 * a creation does. */
int snmf_online_set_state(snmf_online* o, const void* record, int64_t bytes);
/* Added within 5.  src/NTF_sep_event_RT.m:27-38 + init_buff for a finished (flushed) or never-fed separator: it starts a new
 * recording in place, with the semantics of snmf_online_batch_restart / _restart_mel for one stream.  Every piece of state
 * returns to what creation gives with these inputs.  B_DFT_d (F x R_d, fp64) NULL keeps the current fp64 master as it is
 * (load('B_D_u.mat'), no fp32 round trip) and the fixed columns of :328; a new B_DFT_d also becomes the fixed columns.
 * B_Mel_d (F_order x R_d, fp64) has the same rules on a Mel-mode separator; non-NULL outside Mel mode: SNMF_ERR_STATE.  H0
 * (R_x + R_d) / Ad_blk0 (R_a x m_a) NULL: the values the separator last started with.  A separator that has consumed samples
 * and was not flushed, one whose earlier call failed, or the entry of the other precision: SNMF_ERR_STATE.  Ordered on the
 * context's stream; it does not synchronise beyond the uploads. */
int snmf_online_restart_f32(snmf_online* o, const double* B_DFT_d, const double* B_Mel_d, const float* H0, const float* Ad_blk0);
/* Added within 5.  snmf_online_restart_f32 for a separator made by snmf_online_create_f64: the draws cross in fp64.  (Mel mode
 * is not an fp64 mode: a non-NULL B_Mel_d is SNMF_ERR_STATE.) */
int snmf_online_restart_f64(snmf_online* o, const double* B_DFT_d, const double* B_Mel_d, const double* H0, const double* Ad_blk0);

/* ---- multi-GPU solves: one process, several devices ------------------------------------- */
/* The reference's host is ONE MATLAB interpreter (run_basis_train.m:88, run_basis_DNMF.m:40,47,53 call sparse_nmf from
 * a single thread), so the MEX shim cannot bring a process-per-GPU launcher with it: this is the entry that puts the
 * multi-GPU path behind the same call.  The frame axis is sharded over `n_dev` ranks (columns are independent given
 * W, src/sparse_nmf.m:189-208), rank g on devices[g] (a device may appear more than once: the ranks then share it --
 * single-GPU testing); W is replicated.  Per iteration ONE exchange of the fp64 statistics
 *     [ G or Q | P (beta != 1) | rowsum(H) | div | sum(S.*H) ]        (src/sparse_nmf.m:215-239, :248-261)
 * as a one-shot all-reduce over peer-mapped (fine-grained) memory: every rank stores its buffer into its slot on every
 * peer, every rank sums the slots in rank order, so the W replicas and the stop decision (:272-284) are bit-identical everywhere.
 * H-only solves exchange only the two cost scalars.  Call order as for a plan: create -> set_v / set_w / set_h
 * [/ set_sparsity] -> init -> run -> get_*.  Matrices are HOST buffers of the WHOLE problem (V: F x T, H: r x T,
 * column-major; every rank's shard moves through its own pinned pipeline, all ranks at once); params->T is the total frame
 * count.  snmf_multi_run creates its rank threads per call and restores
 * the calling thread's current HIP device before it returns; the one-shot entries use min(n_dev, T) ranks.
 *   col_begin: n_dev + 1 ascending column offsets (col_begin[0] = 0, col_begin[n_dev] = T), or NULL = balanced. */
typedef struct snmf_multi snmf_multi;
int snmf_multi_create(const int32_t* devices, int32_t n_dev, const snmf_params* params, const int64_t* col_begin,
                      snmf_multi** out);
void snmf_multi_destroy(snmf_multi* m);
/* What a device list keeps for the life of the process (csrc/snmf_multi.h, MultiTeam): per rank two contexts -- each with
 * up to 3 x 16 MiB of pinned host bounce buffers, as much device staging and the cached device blocks of destroyed plans --
 * plus the fine-grained gather buffers, arrival words and events; an 8-device list retains about 1.5 GB of pinned host
 * memory after one run_basis_dnmf(devices = ...) call.  At most SNMF_TEAM_CACHE (default 2) idle device lists are kept; a
 * team on which a run FAILED is never kept (its exchange numbers and arrival words may disagree between the ranks).
 * snmf_multi_release_cache destroys every idle team now and returns how many it destroyed (teams in use are not touched):
 * call it when the host is done with its device lists -- a MEX file from its mexAtExit hook (integration/sparse_nmf_mex.cpp
 * does).  snmf_multi_cached_teams: idle teams currently held. */
int32_t snmf_multi_release_cache(void);
int32_t snmf_multi_cached_teams(void);
/* How push and sum of the per-iteration exchange are ordered (csrc/snmf_multi.h).  FLAGS: on the devices (arrival words
 * polled by the summing kernel; a rank's host thread only enqueues) -- AUTO picks it when every rank has a device of its
 * own.  EVENTS: hipEvents + a host barrier per iteration -- AUTO picks it when ranks share a device (single-GPU testing),
 * where FLAGS can stall on a shared hardware queue until its 5 s device-side time-out.  FLAGS across two PHYSICAL devices
 * has only been exercised where tests/test_gpu_multi_abi.py finds two devices.  Between init and the first run only. */
#define SNMF_EXCHANGE_AUTO 0
#define SNMF_EXCHANGE_FLAGS 1
#define SNMF_EXCHANGE_EVENTS 2
int snmf_multi_set_exchange(snmf_multi* m, int32_t mode);
int snmf_multi_set_v_f64(snmf_multi* m, const double* V, int64_t ld);
int snmf_multi_set_v_f32(snmf_multi* m, const float* V, int64_t ld);
int snmf_multi_set_w_f64(snmf_multi* m, const double* W, int64_t ld);
int snmf_multi_set_w_f32(snmf_multi* m, const float* W, int64_t ld);
int snmf_multi_set_h_f64(snmf_multi* m, const double* H, int64_t ld);
int snmf_multi_set_h_f32(snmf_multi* m, const float* H, int64_t ld);
/* r doubles (RVEC) or r x T, leading dimension r (FULL) */
int snmf_multi_set_sparsity_f64(snmf_multi* m, const double* S);
int snmf_multi_set_sparsity_f32(snmf_multi* m, const float* S);
int snmf_multi_init(snmf_multi* m);
/* as snmf_plan_run; one host thread per rank issues that rank's launches, the ranks meet only in the exchange */
int snmf_multi_run(snmf_multi* m, int32_t n_iters, int32_t* iters_done);
int snmf_multi_get_w_f64(snmf_multi* m, double* W, int64_t ld);
int snmf_multi_get_w_f32(snmf_multi* m, float* W, int64_t ld);
/* the replica of W held by one rank (the replicas are bit-identical by construction; tests check it) */
int snmf_multi_get_w_rank_f64(snmf_multi* m, int32_t rank, double* W, int64_t ld);
int snmf_multi_get_h_f64(snmf_multi* m, double* H, int64_t ld);
int snmf_multi_get_h_f32(snmf_multi* m, float* H, int64_t ld);
int snmf_multi_get_objective(snmf_multi* m, double* div_out, double* cost_out, int32_t* n_iter_out);
/* One-shot drop-in with a device list: snmf_sparse_nmf_f64 / _f32 sharded over `n_dev` ranks. */
int snmf_sparse_nmf_multi_f64(const int32_t* devices, int32_t n_dev, const snmf_params* p, const double* V, int64_t ldV,
                              double* W, double* H, const double* sparsity, double* div_out, double* cost_out,
                              int32_t* n_iter_out);
int snmf_sparse_nmf_multi_f32(const int32_t* devices, int32_t n_dev, const snmf_params* p, const float* V, int64_t ldV,
                              float* W, float* H, const float* sparsity, double* div_out, double* cost_out,
                              int32_t* n_iter_out);
/* B_hat = run_basis_DNMF(x, d, B, p) with a device list (run_basis_DNMF.m:36-55; BASELINE config 4): snmf_run_basis_dnmf_f64 / _f32
 * with the frames of all three solves sharded over `n_dev` ranks of this process -- the same arguments, `devices` in place of the
 * context.  Y, X, D cross PCIe once each (every rank its shard, all ranks at once, X and D under solve 1), each rank keeps ITS
 * columns of A_hat in HBM for solves 2 / 3, one exchange of the W statistics per iteration, only B_hat (and A_hat when asked
 * for) comes back.  H0 == NULL: rank g draws columns [col_g, col_g+1) of the (R_x + R_d) x T Philox draw, so the result does not
 * depend on the number of ranks beyond the order in which the ranks' statistics are summed (a few fp32 ulp on B_hat; A_hat
 * bit for bit).  The ranks' contexts, gather buffers and peer-access grants are built once per device list and kept for later calls
 * on the same list (csrc/snmf_multi.h: teams; the two most recently used idle lists, SNMF_TEAM_CACHE=n overrides, 0 = none). */
int snmf_run_basis_dnmf_multi_f64(const int32_t* devices, int32_t n_dev, const snmf_params* p, int32_t R_x, int32_t R_d,
                                  const double* Y, int64_t ldY, const double* X, int64_t ldX, const double* D, int64_t ldD,
                                  const double* B, int64_t ldB, const double* H0, uint64_t seed, double* B_hat, int64_t ldBh,
                                  double* A_hat, int64_t ldA, int32_t* n_iter_out);
int snmf_run_basis_dnmf_multi_f32(const int32_t* devices, int32_t n_dev, const snmf_params* p, int32_t R_x, int32_t R_d,
                                  const float* Y, int64_t ldY, const float* X, int64_t ldX, const float* D, int64_t ldD,
                                  const float* B, int64_t ldB, const float* H0, uint64_t seed, float* B_hat, int64_t ldBh,
                                  float* A_hat, int64_t ldA, int32_t* n_iter_out);

/* ---- batched offline solve: many independent factorizations in shared launches ----------- */
/* Added within 5 (new entries only).  B independent problems V_b ~ W_b * H_b -- src/sparse_nmf.m:157-286 each -- advance in
 * SHARED launches: per iteration one H step over every (problem, 32-frame tile), one W-statistics launch over every
 * (problem, 64-frame chunk) and one finish launch over every (problem, column of W).  A solve of a few hundred to a few
 * thousand frames fills a quarter of the device and is bound by its three launch boundaries per iteration; a batch of them
 * is not ("Batched offline solve", has the measured table).  Shared by the batch: F, r and one snmf_params with
 * the meaning its fields have in snmf_sparse_nmf_f64 (every beta; sparsity SCALAR or RVEC; max_iter, conv_eps, cost_check
 * -- 0: no objective, no stop --, floor_v; w_update_ind full, partial or none; h_update_ind all or none, a partial one is
 * SNMF_ERR_DIM).  Per problem: its frame count T_b >= 1, V_b, the initial factors, the results and the objective.
 * Arithmetic: the fp32 solver's (f32 MFMA products, fp64 statistics and fp64 master copy of W, fp64 objective).
 * Independent solves: problem b stops at the iteration where ITS test (:272-284) fires, with the factors, the div / cost
 * vectors and the n_iter of a solve that ran alone; it is frozen on the device from then on.  The host does not synchronise
 * per iteration: it polls a device counter of stopped problems every 8 iterations, and the run ends when all have stopped or
 * at max_iter.  The bits of problem b depend on its own inputs and p only -- not on B, its slot, the other problems' sizes
 * or stop indices, nor on the entry (one-shot or resident, one run or several): every sum has a fixed order per problem
 * and no floating-point atomics are used.  They are NOT the bits of snmf_sparse_nmf_f64 on the same problem (other
 * summation orders); both are within the same tolerances of the double-precision algorithm.
 * Envelope: F <= 513, r <= 200, any T_b >= 1; B and the sum of T_b are limited by memory (and 2^26 tiles).  Outside it, and
 * for SNMF_SPARSITY_FULL: SNMF_ERR_UNSUPPORTED, the message names the limit.  A failed allocation is SNMF_ERR_NOMEM, frees
 * every block of the batch and leaves the context usable.  NULL arguments, an index outside [0, B), T_b < 1, ldV < F:
 * SNMF_ERR_INVALID.
 * Call order: create -> [set_sparsity for RVEC] -> set_problem for every k -> run -> get.  run before every problem (and
 * an RVEC sparsity) is set, get before run, set_sparsity after run: SNMF_ERR_STATE.  snmf_batch_run(b, n): n more
 * iterations (0: up to max_iter); a later call continues, and run(10) + run(0) gives the bits of one run(0).  A
 * set_problem after a run starts a NEW batch on the handle: every problem is then set again.
 *   snmf_batch_create       p->T is ignored; T: n_problems frame counts
 *   snmf_batch_set_problem  V F x T_k (ldV >= F, floored at 1e-9 when p->floor_v), W0 F x r, H0 r x T_k (tight, read-only)
 *   snmf_batch_get          W F x r, H r x T_k (tight), div_out / cost_out max_iter doubles (zero-filled, then the recorded
 *                           values), n_iter_out; any of them may be NULL
 *   snmf_batch_describe     the geometry (tiles, chunks, grids, LDS) as text */
typedef struct snmf_batch snmf_batch;
int snmf_batch_create(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out);
int snmf_batch_set_problem_f64(snmf_batch* b, int32_t k, const double* V, int64_t ldV, const double* W0, const double* H0);
int snmf_batch_set_problem_f32(snmf_batch* b, int32_t k, const float* V, int64_t ldV, const float* W0, const float* H0);
int snmf_batch_set_sparsity_f64(snmf_batch* b, const double* sparsity /* r */);
int snmf_batch_run(snmf_batch* b, int32_t n_iters);
int snmf_batch_get_f64(snmf_batch* b, int32_t k, double* W, double* H, double* div_out, double* cost_out, int32_t* n_iter_out);
int snmf_batch_get_f32(snmf_batch* b, int32_t k, float* W, float* H, double* div_out, double* cost_out, int32_t* n_iter_out);
int snmf_batch_describe(const snmf_batch* b, char* buf, size_t buflen);
void snmf_batch_destroy(snmf_batch* b);
/* One-shot: create, set, run to the end, get, destroy; the arrays move through the context's chunked transfer pipeline.
 * T, ldV: n entries; V, W0, H0, W, H: n pointers each (the layouts of set_problem / get); sparsity: NULL for SCALAR, r doubles
 * for RVEC; div_out / cost_out: NULL or n pointers to max_iter doubles (single entries may be NULL); n_iter_out: NULL or n. */
int snmf_sparse_nmf_batch_f64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const double* const* V,
                              const int64_t* ldV, const double* const* W0, const double* const* H0, const double* sparsity,
                              double* const* W, double* const* H, double* const* div_out, double* const* cost_out,
                              int32_t* n_iter_out);
int snmf_sparse_nmf_batch_f32(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const float* const* V,
                              const int64_t* ldV, const float* const* W0, const float* const* H0, const double* sparsity,
                              float* const* W, float* const* H, double* const* div_out, double* const* cost_out,
                              int32_t* n_iter_out);

/* Added within 5.  The fp64 mode of the batch: snmf_sparse_nmf_fp64 for n_problems problems in shared launches (DESIGN.md,
 * "Batched offline solve in the fp64 mode").  fp64 storage, every contraction on the f64 MFMA, every intermediate in HBM,
 * tight and unpadded; one grouped GEMM kernel forms each product of an iteration for all problems from a device table of
 * (problem, 64 x 64 tile, split of 2048), and every element-wise pass and reduction is the single fp64 solve's, with the
 * problem as one more grid index.  THE CONTRACT: W, H, div, cost and n_iter of problem b are bit for bit those of
 * snmf_sparse_nmf_fp64 run alone on V_b, W0_b, H0_b with the same settings -- whatever B, the slot, the other problems'
 * sizes and stop indices, and the entry (one-shot or resident, one run or several).
 * Envelope: no F or r limit of its own (the fp32 batch's F <= 513, r <= 200 do not apply); at most 65535 problems, 2^31 - 1
 * tiles in one grouped product, 65535 row-sum chunks of 256 frames in one problem, and the device's free memory -- all checked
 * before anything is allocated: SNMF_ERR_UNSUPPORTED, the message names the limit.  Refused as by snmf_batch_create: a
 * partial h_update_ind (SNMF_ERR_DIM), SNMF_SPARSITY_FULL (SNMF_ERR_UNSUPPORTED), n_problems < 1, T_b < 1, NULL
 * (SNMF_ERR_INVALID) -- before the device is touched.
 * The handle is an snmf_batch and the call order is the one above: create_fp64 -> [set_sparsity for RVEC] -> set_problem for
 * every k -> run -> get.  Every snmf_batch_* entry works on it: set_problem_f64, or _f32 (widened on the way in);
 * set_sparsity_f64; run, with continuation (run(n) + run(0) gives the bits of one run(0)); a set_problem after a run starts a
 * NEW batch; get_f64, or _f32 (the fp64 results rounded to nearest on the way out); describe (tables, grids, launches per
 * iteration, bytes); destroy.  p->floor_v = 0 leaves V unfloored, as in the fp32 batch. */
int snmf_batch_create_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out);
/* One-shot in the fp64 mode: the argument list of snmf_sparse_nmf_batch_f64. */
int snmf_sparse_nmf_batch_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const double* const* V,
                               const int64_t* ldV, const double* const* W0, const double* const* H0, const double* sparsity,
                               double* const* W, double* const* H, double* const* div_out, double* const* cost_out,
                               int32_t* n_iter_out);

/* Added within 5.  A rank of its own for every problem of an fp64 batch: r holds n_problems ranks, problem k factorizes V_k
 * (F x T_k) into W_k (F x r[k]) and H_k (r[k] x T_k).  F and the settings stay shared.  p->r must be the largest r[k]
 * (SNMF_ERR_DIM otherwise).  THE CONTRACT is that of snmf_batch_create_fp64: W, H, div, cost and n_iter of problem k are bit for
 * bit those of snmf_sparse_nmf_fp64 run alone on V_k, W0_k, H0_k with p->r = r[k] -- whatever the ranks, frame counts and order
 * of the problems around it -- and n_problems equal ranks give the bits of snmf_batch_create_fp64 with that rank.  The same
 * kernels run: each finds its problem's rank and offsets in the device table of problems.
 * The handle is an snmf_batch: snmf_batch_set_problem_f64 / _f32 (W0 F x r[k], H0 r[k] x T_k, tight), _run, _get_f64 / _f32
 * (W F x r[k], H r[k] x T_k, tight), _describe (which also reports the smallest, the largest and the sum of the ranks) and
 * _destroy work on it as on any other.  Refused before the device is touched: NULL r, r[k] < 1 (SNMF_ERR_INVALID);
 * a sparsity that is not SNMF_SPARSITY_SCALAR, a w_update_ind or h_update_ind that is neither all ones nor all zeros
 * (SNMF_ERR_UNSUPPORTED: an r-vector has no meaning across ranks); and what snmf_batch_create_fp64 refuses.  Uniform-only, as
 * before: the fp32 engine (snmf_batch_create) and missing-data batches (snmf_batch_create_mdi_fp64).  The DNMF batches with a
 * rank pair per problem are snmf_run_basis_dnmf_batch_ranks_fp64 and snmf_run_basis_dnmf_audio_batch_ranks_fp64. */
int snmf_batch_create_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const int32_t* r,
                                 snmf_batch** out);

/* Added within 5.  Settings of its own for every problem of an fp64 batch: the divergence, the sparsity weight, the stop
 * threshold and the iteration limit, so that a sweep over them is one batch.  s holds n_problems entries.  p gives F, cost_check,
 * floor_v and the masks, which stay shared; p->beta, p->sparsity_scalar and p->conv_eps are ignored; p->max_iter must be the
 * largest s[k].max_iter (SNMF_ERR_DIM otherwise), as p->r is the largest rank on snmf_batch_create_ranks_fp64.  r: a rank per
 * problem under the rules of that entry, or NULL for p->r in every problem.
 * THE CONTRACT: W, H, div, cost and n_iter of problem k are bit for bit those of snmf_sparse_nmf_fp64 run alone on it with s[k]
 * in the place of the four fields -- whatever the settings, ranks, sizes and order of the problems around it.  A problem whose
 * stop test never fires ends after exactly s[k].max_iter iterations with n_iter = s[k].max_iter, with cost_check = 0 too;
 * n_problems equal settings give the bits of snmf_batch_create_fp64 / _ranks_fp64 with those settings in p; run(n) + run(0)
 * gives the bits of run(0), also where a problem's own max_iter falls inside the first run.
 * The handle is an snmf_batch: set_problem_f64 / _f32, run, get_f64 / _f32 (p->max_iter entries of div and cost, zero past the
 * problem's own count), describe (which also reports the number of distinct modes and the smallest and largest max_iter) and
 * destroy work on it as on any other.  The kernels find a problem's settings in the device table of problems; the passes that
 * are compiled per divergence are launched once per divergence present.
 * Refused before the device is touched: NULL s, a non-zero reserved (SNMF_ERR_INVALID); a field of s[k] that snmf_params would
 * be refused for (that status, the message names the problem); a sparsity kind other than SNMF_SPARSITY_SCALAR
 * (SNMF_ERR_UNSUPPORTED); and what snmf_batch_create_fp64 / _ranks_fp64 refuse.  There is no fp32 form and no missing-data form
 * (a masked handle with settings is SNMF_ERR_UNSUPPORTED); the DNMF batches take settings per problem through
 * snmf_run_basis_dnmf_batch_ranks_fp64 and snmf_run_basis_dnmf_audio_batch_ranks_fp64. */
typedef struct snmf_problem_settings {
    double beta;        /* divergence order: 1 kl, 2 ed, 0 is, else generic */
    double sparsity;    /* scalar */
    double conv_eps;    /* 0: no stop test */
    int32_t max_iter;
    int32_t reserved;   /* 0 */
} snmf_problem_settings;

int snmf_batch_create_settings_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const int32_t* r,
                                    const snmf_problem_settings* s, snmf_batch** out);

/* Added within 5.  The missing-data solves in the batch: snmf_mdi_fp64 (src/snmf_mdi.m / src/snmf_mdi_Sm.m) for n_problems
 * problems, each with a mask of its own (M_b F x T_b, 1 = observed, soft masks in [0, 1]), in the shared launches of the fp64
 * batch ("Batched missing-data solves").  fp64 only: the fused fp32 missing-data kernels have no batched form.
 * THE CONTRACT: V_mdi, H, W, div, cost and n_iter of problem b are bit for bit those of snmf_mdi_fp64 run alone on V_b, M_b,
 * W0_b, H0_b with the same settings -- whatever B, the slot, the other problems and the entry (one-shot or resident).
 * snmf_batch_create_mdi_fp64 makes an fp64 batch whose problems carry masks: the validation, refusals and envelope of
 * snmf_batch_create_fp64, checked before the device is touched; the masks take one more F x sum(T_b) block of doubles and
 * reading v_MDI one of F x max(T_b), both counted in the free-memory check and in describe().  p->floor_v has no meaning
 * (the masked start v = max(v .* M, 1e-9) floors, as in snmf_mdi_fp64).
 * The call order is the batch's: create_mdi -> [set_sparsity for RVEC] -> set_problem_mdi for every k -> run -> get / get_v_mdi.
 *   snmf_batch_set_problem_mdi_f64  V and M F x T_k (ldV, ldM >= F), W0 F x r, H0 r x T_k: a problem and its mask in one call.
 *                                   On a batch made without masks: SNMF_ERR_STATE.  On a masked batch snmf_batch_set_problem_f64
 *                                   / _f32 return SNMF_ERR_STATE.  Either refusal leaves the handle as it was.
 *   snmf_batch_get_v_mdi_f64        the gain-matched final imputation (src/snmf_mdi.m:296-306) of problem k from the state the
 *                                   last run left, F x T_k (ld >= F).  The problem's V, its estimate and its mask are not
 *                                   written: a later run continues as if nothing had been read.  With max_iter = 0 it is the
 *                                   imputation from the scaled initial factors, as in snmf_mdi_fp64.  Before the first run and on a
 *                                   batch made without masks: SNMF_ERR_STATE.
 * snmf_batch_set_sparsity_f64, _run, _get_f64 / _f32, _describe and _destroy are the entries above. */
int snmf_batch_create_mdi_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out);
int snmf_batch_set_problem_mdi_f64(snmf_batch* b, int32_t k, const double* V, int64_t ldV, const double* M, int64_t ldM,
                                   const double* W0, const double* H0);
int snmf_batch_get_v_mdi_f64(snmf_batch* b, int32_t k, double* V_mdi, int64_t ld);
/* One-shot: the arguments of snmf_sparse_nmf_batch_fp64 plus M / ldM (n pointers, n leading dimensions) and the outputs V_mdi (n
 * pointers, F x T_k each) with ldVm (n leading dimensions, or NULL: tight).  W may be NULL, and so may single entries of it. */
int snmf_mdi_batch_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const double* const* V,
                        const int64_t* ldV, const double* const* M, const int64_t* ldM, const double* const* W0,
                        const double* const* H0, const double* sparsity, double* const* V_mdi, const int64_t* ldVm,
                        double* const* W, double* const* H, double* const* div_out, double* const* cost_out, int32_t* n_iter_out);

/* Added within 5.  run_basis_DNMF (run_basis_DNMF.m:36-55) for n_problems problems at once, one per noise type or class as in the
 * loop of Do_MultiBatch_IS16_20160324.m:139-148 ("Batched DNMF re-training").  The problems share F, R_x, R_d and
 * the settings; problem k has its own frame count T[k], its own B_k and its own initial activations H0_k.  The three solves
 * run as three batches on the engines above -- the mixtures (r = R_x + R_d, H only), the clean features (r = R_x, W only) and
 * the noise features (r = R_d, W only) -- and A_hat passes from the first into the other two on the device; every problem
 * stops each of its solves at its own iteration.  One-shot entries, no handle.
 * Every matrix is tight and column-major: Y_k, X_k, D_k F x T[k]; B_k F x (R_x + R_d); H0_k (R_x + R_d) x T[k]; the outputs
 * B_hat_k F x (R_x + R_d) and A_hat_k (R_x + R_d) x T[k].  Y, X, D, B, H0, B_hat: n_problems pointers each.  A_hat: NULL, or
 * n_problems pointers of which single ones may be NULL (not wanted).  n_iter: NULL, or 3 per problem (solves 1, 2, 3).
 * p->r = R_x + R_d; p->T is ignored; the masks of p are ignored (the loop sets its own).
 *   _f64 / _f32  the fp32 engine (snmf_batch_create) from double / float host arrays.  THE CONTRACT: bit for bit three chained
 *                snmf_sparse_nmf_batch_* calls with the loop's masks, init_w = B_k / its column blocks and init_h = H0_k /
 *                the row blocks of A_hat_k.  Envelope: the fp32 batch's (F <= 513, R_x + R_d <= 200), SNMF_ERR_UNSUPPORTED.
 *   _fp64        the fp64 engine (snmf_batch_create_fp64).  THE CONTRACT: B_hat_k, A_hat_k and the three counts are bit for bit
 *                those of snmf_run_basis_dnmf_fp64 run alone on problem k.
 * In both, the results of a problem depend on its own inputs and the settings only, not on the batch around it.
 * Refused before the device is touched: NULL arguments, n_problems < 1, T[k] < 1 (SNMF_ERR_INVALID); R_x < 1, R_d < 1,
 * p->r != R_x + R_d, a sparsity that is not SNMF_SPARSITY_SCALAR (SNMF_ERR_DIM, as snmf_run_basis_dnmf_*). */
int snmf_run_basis_dnmf_batch_f64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n_problems, const int32_t* T,
                                  const double* const* Y, const double* const* X, const double* const* D, const double* const* B,
                                  const double* const* H0, double* const* B_hat, double* const* A_hat, int32_t* n_iter);
int snmf_run_basis_dnmf_batch_f32(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n_problems, const int32_t* T,
                                  const float* const* Y, const float* const* X, const float* const* D, const float* const* B,
                                  const float* const* H0, float* const* B_hat, float* const* A_hat, int32_t* n_iter);
int snmf_run_basis_dnmf_batch_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n_problems, const int32_t* T,
                                   const double* const* Y, const double* const* X, const double* const* D, const double* const* B,
                                   const double* const* H0, double* const* B_hat, double* const* A_hat, int32_t* n_iter);

/* Added within 5.  The spectrogram front-end for n_signals signals at once: what snmf_stft_features_f32 / _fp64 give for each
 * signal alone (and, with mel != NULL -- row-major mel_M x (fftlength/2+1), as snmf_mel_features_* take it -- what
 * snmf_mel_features_* make of that), bit for bit, from launches shared by all signals: their number does not depend on n_signals.
 * Host arrays in and out; the samples go up as one slab.  samples, n_samples, V_out: n_signals entries each; V_out[k] is tight,
 * rows x n_frames_out[k] with rows = (2 * splice + 1) * (fftlength/2+1), or (2 * splice + 1) * mel_M with mel (the matrices of a
 * batch are tight, as in snmf_run_basis_dnmf_batch_*).  n_frames_out: NULL, or n_signals counts.  A signal shorter than one frame gives
 * n_frames_out[k] = 0 and nothing of it is read or written, as in the single entry.  Refused before the device is touched: NULL
 * arguments, n_signals < 1, mel_M < 1 with mel (SNMF_ERR_INVALID), the refusals of the single entry for sp. */
int snmf_stft_features_batch_f32(snmf_ctx* ctx, const snmf_stft_params* sp, int32_t n_signals, const float* const* samples,
                                 const int64_t* n_samples, const float* mel, int32_t mel_M, float* const* V_out, int32_t* n_frames_out);
int snmf_stft_features_batch_fp64(snmf_ctx* ctx, const snmf_stft_params* sp, int32_t n_signals, const double* const* samples,
                                  const int64_t* n_samples, const double* mel, int32_t mel_M, double* const* V_out,
                                  int32_t* n_frames_out);

/* Added within 5.  run_basis_DNMF (run_basis_DNMF.m:1-55; with mel its twin run_basis_DNMF_Mel.m) for n_problems pairs of
 * WAVEFORMS at once: snmf_run_basis_dnmf_batch_* with the features formed on the device, as snmf_run_basis_dnmf_audio_* form them
 * for one pair.  Problem k: x_k (n_x[k] samples) and d_k (n_d[k] samples) are cut to their common length (:5-9), y_k = x_k + d_k
 * in the sample type (:10), T_k = snmf_stft_num_frames(sp, min(n_x[k], n_d[k])).  The waveforms cross as one slab; the three
 * feature sets of all problems are written by shared launches straight into the three resident batches, and A_hat passes between
 * them on the device.  p->F must be the feature rows, (2 * splice + 1) * (fftlength/2+1), or (2 * splice + 1) * mel_M with mel
 * (SNMF_ERR_DIM); p->r = R_x + R_d; p->T and the masks of p are ignored.  Every matrix is tight and column-major, as in
 * snmf_run_basis_dnmf_batch_*: B_k, B_hat_k F x (R_x + R_d); H0_k, A_hat_k (R_x + R_d) x T_k.  H0: NULL, or n_problems pointers of
 * which single ones may be NULL: such a problem starts from the Philox draw of snmf_plan_set_h_random keyed by seed[k] (seed:
 * n_problems entries, read only there).  A_hat: NULL, or pointers of which single ones may be NULL.  n_iter: NULL, or 3 per problem.
 *   _f64   the fp32 engine, named after its host type like snmf_run_basis_dnmf_audio_f64: float samples and Mel table, fp32
 *          features.  THE CONTRACT: bit for bit snmf_run_basis_dnmf_batch_f64 fed the outputs of snmf_stft_features_f32
 *          (+ snmf_mel_features_f32) on y_k, x_k, d_k widened to double, B_k, and H0_k or the draw.  Envelope: the fp32 batch's
 *          (F <= 513, R_x + R_d <= 200), SNMF_ERR_UNSUPPORTED.
 *   _fp64  the fp64 engine: double samples and Mel table, everything in double, no limit on F or r of its own.  THE CONTRACT:
 *          B_hat_k, A_hat_k and the three counts are bit for bit those of snmf_run_basis_dnmf_audio_fp64 run alone on
 *          (x_k, d_k, B_k) with the same H0_k, or with H0 = NULL and the same seed.
 * Refused before the device is touched: NULL arguments, n_problems < 1, a problem shorter than one analysis frame, mel_M < 1
 * with mel, a problem without H0 when seed is NULL (SNMF_ERR_INVALID); the refusals of the single entry for sp; R_x < 1,
 * R_d < 1, p->r != R_x + R_d, a sparsity that is not SNMF_SPARSITY_SCALAR (SNMF_ERR_DIM).  A failed allocation is
 * SNMF_ERR_NOMEM; everything is freed and the context stays usable.  One-shot entries: no handle, no device list. */
int snmf_run_basis_dnmf_audio_batch_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                        int32_t n_problems, const float* const* x, const int64_t* n_x, const float* const* d,
                                        const int64_t* n_d, const float* mel, int32_t mel_M, const double* const* B,
                                        const double* const* H0, const uint64_t* seed, double* const* B_hat, double* const* A_hat,
                                        int32_t* n_iter);
int snmf_run_basis_dnmf_audio_batch_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                         int32_t n_problems, const double* const* x, const int64_t* n_x, const double* const* d,
                                         const int64_t* n_d, const double* mel, int32_t mel_M, const double* const* B,
                                         const double* const* H0, const uint64_t* seed, double* const* B_hat, double* const* A_hat,
                                         int32_t* n_iter);

/* Added within 5.  snmf_run_basis_dnmf_batch_fp64 and snmf_run_basis_dnmf_audio_batch_fp64 with a rank pair and, optionally,
 * settings per problem: the sweep over R_x / R_d, max_iter and the sparsity weight of the reference's settings files as one call.
 * R_x and R_d hold n_problems ranks each; s: NULL (the four fields of p for every problem), or n_problems entries
 * (snmf_problem_settings, as on snmf_batch_create_settings_fp64) of which s[k] is used in all three solves of problem k, as the
 * reference passes one p through them (run_basis_DNMF.m:37-53).  The other arguments keep the order of the namesakes.
 * p->r must be the largest R_x[k] + R_d[k]; with s, p->max_iter must be the largest s[k].max_iter and p->beta,
 * p->sparsity_scalar and p->conv_eps are ignored (SNMF_ERR_DIM otherwise: the rules of snmf_batch_create_ranks_fp64 /
 * _settings_fp64, whose code makes the three resident batches -- ranks R_x[k] + R_d[k], R_x[k] and R_d[k]).  Every matrix is
 * tight: B_k, B_hat_k F x (R_x[k] + R_d[k]), B_hat_k = [B_hat_x, B_hat_d] with the noise part at column R_x[k]; H0_k, A_hat_k
 * (R_x[k] + R_d[k]) x T_k.  In the audio form an H0_k that is not given is the Philox draw keyed by seed[k] with R_x[k] + R_d[k] rows.
 * THE CONTRACT: B_hat_k, A_hat_k and the three counts are bit for bit those of snmf_run_basis_dnmf_fp64 (the matrix form) or
 * snmf_run_basis_dnmf_audio_fp64 (the audio form) run alone on problem k with R_x[k], R_d[k] and s[k] in the place of the four
 * fields -- whatever the ranks, settings, sizes and order of the problems around it; n_problems equal pairs with s = NULL give
 * the bits of the namesake.  A_hat passes between the batches on the device, problem k's rows at problem k's own offsets.
 * Refused before the device is touched: NULL R_x or R_d, R_x[k] < 1, R_d[k] < 1, a sparsity that is not SNMF_SPARSITY_SCALAR
 * (SNMF_ERR_DIM, as the namesakes refuse a bad scalar); a non-zero reserved (SNMF_ERR_INVALID) or a field of s[k] that
 * snmf_params would be refused for (that status; the message names the problem); and what the namesakes and the two create
 * entries refuse.  There is no fp32 form: the fp32 batch engine has one rank and one settings struct for all problems. */
int snmf_run_basis_dnmf_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const int32_t* R_x, const int32_t* R_d,
                                         const snmf_problem_settings* s, int32_t n_problems, const int32_t* T, const double* const* Y,
                                         const double* const* X, const double* const* D, const double* const* B,
                                         const double* const* H0, double* const* B_hat, double* const* A_hat, int32_t* n_iter);
int snmf_run_basis_dnmf_audio_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, const int32_t* R_x,
                                               const int32_t* R_d, const snmf_problem_settings* s, int32_t n_problems,
                                               const double* const* x, const int64_t* n_x, const double* const* d, const int64_t* n_d,
                                               const double* mel, int32_t mel_M, const double* const* B, const double* const* H0,
                                               const uint64_t* seed, double* const* B_hat, double* const* A_hat, int32_t* n_iter);

/* Added within 5.  Basis training (run_basis_train.m:58-91) for the training signals of n_problems event classes or noise types
 * at once -- the loop l = 1:length(DB_path_list) of the reference: snmf_run_basis_train_audio_* for every signal, with the
 * features of all signals formed by the grouped front-end and the two solves of every problem run as two resident batches
 * ("Batched basis training").  The problems share the settings; problem k has its own signal (n_samples[k] samples),
 * frame count T_k = snmf_stft_num_frames(sp, n_samples[k]) and exemplar columns sample_idx[k] (p->r indices, 0-based).
 * The samples cross as one slab.  TF_mag of every signal is written straight into the DFT batch, TF_DD (alpha_eta_dd >= 0; < 0:
 * off) runs in place there, TF_Mel is projected from there into the Mel batch, each batch gathers init_w = V(:, sample_idx) from
 * its own, still unfloored V on the device, and both solves of a problem start from the same H0.  mel (row-major mel_M x
 * (fftlength/2+1)) and B_Mel go together; without them only the DFT solve runs.  p->F must be (2 * splice + 1) * (fftlength/2+1)
 * (SNMF_ERR_DIM); p->r = cluster_buff * R; p->T and the masks of p are ignored (every row and column is updated, :85-86).
 * Every matrix is tight and column-major: B_DFT_k F x r, B_Mel_k (2 * splice + 1) * mel_M x r, H0_k, A_DFT_k, A_Mel_k r x T_k.
 * samples, n_samples, sample_idx, B_DFT (and B_Mel): n_problems entries each.  H0: NULL, or n_problems pointers of which single
 * ones may be NULL: such a problem starts from the Philox draw of snmf_plan_set_h_random keyed by seed[k] (seed: n_problems
 * entries, read only there).  A_DFT, A_Mel: NULL, or pointers of which single ones may be NULL.  n_iter: NULL, or 2 per problem
 * (the DFT and the Mel solve).  train_exemplar != 0 (:84, :93-96): nothing is solved, B_DFT_k and B_Mel_k are the gathered
 * exemplar columns, H0, seed, A_DFT and A_Mel are not looked at and n_iter is zeroed.
 *   _f64   the fp32 engine, named after its host type like snmf_run_basis_train_audio_f64: float samples and Mel table, fp32
 *          features.  THE CONTRACT: B_*_k, A_*_k and the counts are bit for bit those of snmf_sparse_nmf_batch_f64 on the features
 *          snmf_stft_features_f32 (then snmf_tf_dd_f32, then snmf_mel_features_f32 on that) give for signal k, widened to double,
 *          with init_w their columns sample_idx[k] and init_h = H0_k or the draw.  Envelope: the fp32 batch's (F <= 513,
 *          r <= 200), SNMF_ERR_UNSUPPORTED.
 *   _fp64  the fp64 engine: double samples and Mel table, everything in double.  THE CONTRACT: bit for bit
 *          snmf_run_basis_train_audio_fp64 run alone on signal k with the same H0_k, or with H0 = NULL and the same seed.
 * Refused before the device is touched: NULL arguments, n_problems < 1, a signal shorter than one analysis frame, mel without
 * B_Mel or the reverse, mel_M < 1 with mel, a problem without H0 when seed is NULL (SNMF_ERR_INVALID); the refusals of the single
 * entry for sp; p->F that is not the feature rows, an index outside [0, T_k) (SNMF_ERR_DIM); a sparsity that is not
 * SNMF_SPARSITY_SCALAR and the fp32 envelope (SNMF_ERR_UNSUPPORTED).  One-shot entries: no handle, no device list. */
int snmf_run_basis_train_audio_batch_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                         const float* mel, int32_t mel_M, int32_t n_problems, const float* const* samples,
                                         const int64_t* n_samples, const int64_t* const* sample_idx, int32_t train_exemplar,
                                         const double* const* H0, const uint64_t* seed, double* const* B_DFT, double* const* A_DFT,
                                         double* const* B_Mel, double* const* A_Mel, int32_t* n_iter);
int snmf_run_basis_train_audio_batch_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                          const double* mel, int32_t mel_M, int32_t n_problems, const double* const* samples,
                                          const int64_t* n_samples, const int64_t* const* sample_idx, int32_t train_exemplar,
                                          const double* const* H0, const uint64_t* seed, double* const* B_DFT, double* const* A_DFT,
                                          double* const* B_Mel, double* const* A_Mel, int32_t* n_iter);

/* Added within 5.  The step before basis training, run_basis_train.m:16-57 with src/vadenergy_simple.m:1-32: the training signal
 * s_full of n_classes classes assembled on the device from their clips ("Training signals from clips").  The clips
 * cross as they come off disk -- int16 PCM (_i16: s = pcm / 32768 * 32767, :26-27) or doubles already scaled wavread(.) * 32767
 * (_f64) -- and every s_full stays in HBM behind the handle, for snmf_run_basis_train_signals_batch_* below.  The caller shuffles
 * and subsamples (:17, :21): class k consumes its n_clips[k] clips in the order given.  clips and clip_len run over all clips of
 * all classes in class order; mode has one entry per class (VAD_set / p.train_ANOT):
 *   mode 1  src/vadenergy_simple.m: bg_mean = mean(|s(1:bg_len)|); frames k = 1 .. floor(len / shift) - 1 of frame_len samples
 *           from 1 + (k-1) * shift, shift = frame_len / 2; a frame is voiced when (mean|frame| - bg_mean) / mean|frame| > thr (a
 *           0/0 or -inf compares false); a sample is voiced when a frame covering it is; the clip becomes nonzeros(s .* vad): exact
 *           zeros inside voiced stretches are dropped too (:37).  file_len_max is not applied.
 *   mode 2  the clip becomes s(v_start:v_end), range[2c], range[2c+1] of clip c (1-based, inclusive; range is read only for the
 *           clips of mode-2 classes and may be NULL when there is none).  Zeros stay.
 *   mode 0  the clip becomes s(1:file_len_max) when it is longer; file_len_max <= 0: no cut.  Zeros stay.
 * Then s = s / sqrt(var(s)) (two passes, N - 1), s = s / max|s| * 30000 (:44-45), element by element in that order, and the clip
 * is appended; when the length then EXCEEDS seq_len_max the signal is cut to exactly seq_len_max and the later clips are not
 * used (:50-53; a length equal to the limit does not stop).  All arithmetic is fp64.  The sums are formed in a fixed tree order
 * (not MATLAB's sequential one): the signals are the same bits from run to run and within a few ulp of the reference's.
 * TWO DEVIATIONS, where the reference fails or produces NaN: a clip with no kept sample contributes nothing and counts as used
 * (MATLAB appends an empty vector); a clip among the consumed ones whose
 * variance, as computed, is not a positive finite number -- one kept sample, a constant clip -- makes the call fail with
 * SNMF_ERR_INVALID, naming the class and the clip: no handle is returned and the context stays usable (MATLAB writes NaN into
 * s_full and trains NaN dictionaries).
 * Refused before the device is touched: NULL arguments, n_classes < 1, a class with no clip, a mode outside 0..2, a mode-2 class
 * with range == NULL, frame_len odd or < 2, bg_len < 1, seq_len_max < 0 (SNMF_ERR_INVALID); a clip without a sample, a mode-1 clip
 * shorter than bg_len (an index error in MATLAB), a range outside [1, len] or with v_start > v_end (SNMF_ERR_DIM).  A class whose
 * assembled length is 0 or shorter than one analysis frame assembles fine: the training entry refuses it.
 * snmf_train_signals_info: n_samples and clips_used receive one entry per class (any of the three may be NULL).
 * snmf_train_signals_get_f64: s_full of class k (n_samples[k] doubles; run_basis_train.m:96 writes s_full ./ 32767 as the class's
 * wav).  snmf_train_signals_destroy gives the slab back (it may follow the context's own destruction; every other entry needs the
 * context alive). */
typedef struct snmf_train_signals snmf_train_signals;
typedef struct {
    int32_t frame_len, bg_len; /* src/vadenergy_simple.m:19 (0.02 * fs), run_basis_train.m:32 (0.05 * fs) */
    double thr;                /* run_basis_train.m:35 */
    int64_t seq_len_max, file_len_max; /* p.train_seq_len_max, p.train_file_len_max (samples) */
} snmf_assemble_params;
int snmf_train_signals_assemble_i16(snmf_ctx* ctx, const snmf_assemble_params* ap, int32_t n_classes, const int32_t* n_clips,
                                    const int16_t* const* clips, const int64_t* clip_len, const int32_t* mode, const int64_t* range,
                                    snmf_train_signals** out);
int snmf_train_signals_assemble_f64(snmf_ctx* ctx, const snmf_assemble_params* ap, int32_t n_classes, const int32_t* n_clips,
                                    const double* const* clips, const int64_t* clip_len, const int32_t* mode, const int64_t* range,
                                    snmf_train_signals** out);
int snmf_train_signals_info(const snmf_train_signals* signals, int32_t* n_classes, int64_t* n_samples, int32_t* clips_used);
int snmf_train_signals_get_f64(const snmf_train_signals* signals, int32_t k, double* s_full);
int snmf_train_signals_destroy(snmf_train_signals* signals);
/* Added within 5.  snmf_run_basis_train_audio_batch_* on the signals of a handle: n_problems and n_samples are the handle's, the
 * sample slab of the grouped front-end is filled from the resident signals by one launch (a copy for the fp64 engine, round to
 * nearest to float for the fp32 engine) and the rest is the same code.  THE CONTRACTS: _fp64 is bit for bit
 * snmf_run_basis_train_audio_batch_fp64 on the signals snmf_train_signals_get_f64 returns, _f64 bit for bit
 * snmf_run_basis_train_audio_batch_f64 on those signals rounded to float.  Every refusal of those entries carries over (a class
 * shorter than one analysis frame included); a handle of another context is SNMF_ERR_INVALID. */
int snmf_run_basis_train_signals_batch_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                           const float* mel, int32_t mel_M, const snmf_train_signals* signals,
                                           const int64_t* const* sample_idx, int32_t train_exemplar, const double* const* H0,
                                           const uint64_t* seed, double* const* B_DFT, double* const* A_DFT, double* const* B_Mel,
                                           double* const* A_Mel, int32_t* n_iter);
int snmf_run_basis_train_signals_batch_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                            const double* mel, int32_t mel_M, const snmf_train_signals* signals,
                                            const int64_t* const* sample_idx, int32_t train_exemplar, const double* const* H0,
                                            const uint64_t* seed, double* const* B_DFT, double* const* A_DFT, double* const* B_Mel,
                                            double* const* A_Mel, int32_t* n_iter);

/* Added within 5.  snmf_run_basis_train_audio_batch_fp64 and snmf_run_basis_train_signals_batch_fp64 with a dictionary size per
 * problem: n_atoms holds n_problems counts (cluster_buff * R_k), and p->r must be the largest (SNMF_ERR_DIM otherwise; an entry
 * < 1 or a NULL n_atoms is SNMF_ERR_INVALID).  sample_idx[k] holds n_atoms[k] indices; H0_k, A_DFT_k and A_Mel_k are
 * n_atoms[k] x T_k; B_DFT_k and B_Mel_k have n_atoms[k] columns.  Everything else -- arguments, refusals, the front-end, the two
 * resident batches (made by snmf_batch_create_ranks_fp64's code) -- is the namesake's.  THE CONTRACT: problem k is bit for bit
 * snmf_run_basis_train_audio_fp64 run alone on signal k with p->r = n_atoms[k] and the same H0_k, or with H0 = NULL and the same
 * seed.  There is no fp32 form: the fp32 batch engine has one rank for all problems. */
int snmf_run_basis_train_audio_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                const double* mel, int32_t mel_M, int32_t n_problems, const double* const* samples,
                                                const int64_t* n_samples, const int32_t* n_atoms, const int64_t* const* sample_idx,
                                                int32_t train_exemplar, const double* const* H0, const uint64_t* seed,
                                                double* const* B_DFT, double* const* A_DFT, double* const* B_Mel, double* const* A_Mel,
                                                int32_t* n_iter);
int snmf_run_basis_train_signals_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                  const double* mel, int32_t mel_M, const snmf_train_signals* signals,
                                                  const int32_t* n_atoms, const int64_t* const* sample_idx, int32_t train_exemplar,
                                                  const double* const* H0, const uint64_t* seed, double* const* B_DFT,
                                                  double* const* A_DFT, double* const* B_Mel, double* const* A_Mel, int32_t* n_iter);

/* Added within 5.  The two entries above with settings per problem (snmf_problem_settings, as on
 * snmf_batch_create_settings_fp64): the argument lists of the _ranks_fp64 namesakes plus s, n_problems entries.  n_atoms may be
 * NULL: p->r atoms for every problem.  Both resident batches, DFT and Mel, are made with the settings; p->beta,
 * p->sparsity_scalar and p->conv_eps are ignored and p->max_iter must be the largest s[k].max_iter.  THE CONTRACT: signal k is
 * bit for bit snmf_run_basis_train_audio_fp64 run alone with s[k] in the place of the four fields.  NULL s: SNMF_ERR_INVALID;
 * everything else is refused as by the namesakes and by snmf_batch_create_settings_fp64, before the device is touched. */
int snmf_run_basis_train_audio_batch_settings_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                   const double* mel, int32_t mel_M, int32_t n_problems, const double* const* samples,
                                                   const int64_t* n_samples, const int32_t* n_atoms, const int64_t* const* sample_idx,
                                                   int32_t train_exemplar, const double* const* H0, const uint64_t* seed,
                                                   double* const* B_DFT, double* const* A_DFT, double* const* B_Mel, double* const* A_Mel,
                                                   int32_t* n_iter, const snmf_problem_settings* s);
int snmf_run_basis_train_signals_batch_settings_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                     const double* mel, int32_t mel_M, const snmf_train_signals* signals,
                                                     const int32_t* n_atoms, const int64_t* const* sample_idx, int32_t train_exemplar,
                                                     const double* const* H0, const uint64_t* seed, double* const* B_DFT,
                                                     double* const* A_DFT, double* const* B_Mel, double* const* A_Mel, int32_t* n_iter,
                                                     const snmf_problem_settings* s);

/* ---- instrumentation (bench.py: HIP-event timing on the engine's own stream) ------------ */
/* Average device time in milliseconds per launch of the named kernel family over the launches
 * recorded since snmf_ctx_timing(ctx, 1) was switched on.  Families: "hstep", "wstats",
 * "wapply", "reduce", "wfin", and "assemble" (the ten launches of one snmf_train_signals_assemble_* call).  Timing inserts hipEvents around each launch (off by default). */
int snmf_ctx_timing(snmf_ctx* ctx, int enable);
/* Host <-> device transfer counters of a context since the last reset (host arrays move as a pipeline of column chunks through
 * pinned bounce buffers, csrc/snmf_tu_xfer.hip).  out8 = { host->device: bytes of the callers' arrays, wall seconds inside the
 * calls, seconds of host-side copying, calls;  device->host: the same four }. */
int snmf_ctx_xfer_stats(snmf_ctx* ctx, double* out8, int reset);
int snmf_ctx_timing_get(snmf_ctx* ctx, const char* family, double* avg_ms, int64_t* launches);
/* Kernel geometry chosen for a plan, for DESIGN.md / profiles bookkeeping. */
int snmf_plan_describe(const snmf_plan* plan, char* buf, size_t buflen);
/* The same text for a plan of parameters p on a device of n_cu compute units, without a device: p is validated as by
 * snmf_plan_create, and the text is what snmf_plan_describe gives for such a plan without an observed/missing mask. */
int snmf_plan_geometry_describe(const snmf_params* p, int32_t n_cu, char* buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* SNMF_H_ */
