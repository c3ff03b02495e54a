// snmf_batch_host.h -- the host driver of the batched offline solve (include/snmf.h: snmf_batch_*), once for its two modes.
// Host code only.  A handle is the common state below plus one engine: the fp32 engine (snmf_tu_batch.hip, the kernels of
// snmf_batch.h) or the fp64 engine (snmf_tu_batch64.hip, the grouped kernels of snmf_batch64.h).  The kernels and the device
// layouts of the two have nothing in common; the life of the handle -- what is validated when it is made, which call is
// allowed when, how far a run goes, when the host looks at the stopped counter, what get() reports -- is the same and is
// written here.  The modes are told apart where the handle is made (snmf_batch_create / snmf_batch_create_fp64) and nowhere else:
// nothing in this file asks which engine it drives.
// A handle made by snmf_batch_create_mdi_fp64 is a batch of missing-data solves (`masked`): its problems are set together with
// their masks (batch_set_problem_mdi), and the imputed V of a problem can be read (batch_get_v_mdi); everything else -- run, get,
// describe, destroy, the new batch on a used handle -- is the life below, unchanged.
// A handle made by snmf_batch_create_ranks_fp64 carries a rank per problem (`ranks`): problem k's W is F x ranks[k] and its H
// ranks[k] x T_k wherever a call below says r; p.r is the largest of them.  The life is the same; what such a handle refuses
// (batch_create, take_h0) it refuses before any device work; its activations go over through take_h0_rows.
// A handle made by snmf_batch_create_settings_fp64 carries settings per problem (`settings`): problem k's divergence, sparsity
// weight, stop threshold and iteration limit wherever a call below says p.beta, p.sparsity_scalar, p.conv_eps or p.max_iter;
// p.max_iter is the largest of the limits.  A run goes to that, the engine freezes a problem at its own limit and counts it in
// the stopped counter, and get() reports the problem's own n_iter.  An engine that has no such form refuses in build().
#pragma once
#include <functional>
#include <memory>

#include "snmf_internal.h"

struct snmf_batch {
    // ---- the common state of a batch
    snmf_ctx* ctx = nullptr;
    snmf_params p{};  // (its mask pointers are cleared: upd_h, upd_w and w_ind are their reading)
    int B = 0;
    std::vector<int32_t> ranks;  // one rank per problem; empty: every problem has p.r
    int rank_of(int k) const { return ranks.empty() ? p.r : ranks[k]; }
    std::vector<snmf_problem_settings> settings;  // settings per problem; empty: every problem has those of p
    snmf_problem_settings settings_of(int k) const {
        return settings.empty() ? snmf_problem_settings{p.beta, p.sparsity_scalar, p.conv_eps, p.max_iter, 0} : settings[k];
    }
    bool any_can_stop = false;  // the stop test of some problem can fire (a conv_eps > 0 with the objective computed)
    bool own_max_iter = false;  // some problem ends at a max_iter of its own, below p.max_iter
    bool upd_h = true, upd_w = true;
    std::vector<uint8_t> w_ind;
    std::vector<uint8_t> have;
    int n_have = 0;
    bool have_s = false, ran = false;
    bool masked = false;  // a batch of missing-data solves: set by the engine that was made for one, before batch_create
    int it_done = 0;
    std::vector<double> h_div, h_cost;  // the objective histories on the host, hist_len() entries per problem
    int hist_len() const { return std::max(1, p.max_iter); }

    // ---- the engine: what each mode does in its own way
    virtual ~snmf_batch() {}  // frees the device memory
    // the mode's limits on F and r (p is validated): they are refused before the frame counts are looked at
    virtual int check_shape() const { return SNMF_OK; }
    // checks the limits that depend on the frame counts, allocates and builds; the common state above is filled in, and a failure
    // leaves what was allocated to the destructor
    virtual int build(const int32_t* T) = 0;
    virtual int reset() = 0;  // the device state of a batch that has not run
    virtual int upload_sparsity(const double* sparsity) = 0;  // r entries; the caller's array may go on return
    // problem k from host arrays, and its initial scaling (src/sparse_nmf.m:157-169).  H0 == nullptr: V, W0 and the scaling of W
    // only -- the problem's H0 is still to come, for every problem at once, through take_h0 or draw_h0.  V == nullptr: W0 (and H0)
    // only -- V of every problem is written on the device, through v_blocks / v_written.  W0 == nullptr: W0 of every problem has
    // been taken on the device, through take_w0, and H0 is scaled by the norms that left
    virtual int load(int k, const double* V, int64_t ldV, const double* W0, const double* H0) = 0;
    virtual int load(int k, const float* V, int64_t ldV, const float* W0, const float* H0) = 0;
    // init_w of every problem = its rank_of(k) columns of idx (0-based, host; the problems' entries packed one behind the other,
    // k * r .. k * r + r on a uniform batch) of the problem's own V block, as it lies there
    // when the call is made (between v_blocks and v_written: the unfloored V), gathered by one launch over all problems; then,
    // with unit_columns, the initial scaling load() runs after its W0 upload (:157-158), so that the state is that of
    // load(k, nullptr, ld, W0, nullptr) with the same values.  Without unit_columns the gathered columns stay as they are and
    // fetch(k, W, nullptr) reads them (run_basis_train.m:84: the exemplars are the dictionary): such a batch does not run.
    virtual int take_w0(const int64_t* idx, bool unit_columns = true) = 0;
    // V of every problem from device memory instead of a host pointer.  v_blocks hands out where problem k's V lies -- column t at
    // V + t * ld, F rows of v_elem() bytes -- after making everything around those entries what load() leaves there (the fp32
    // engine: zeroed pad rows and pad frames); work on the context's stream then writes every entry of every block, and v_written
    // runs what load() runs after its upload (the V floor of :169), so that the solve sees what load() would have left.
    struct VBlock {
        void* V;
        int64_t ld;
    };
    virtual size_t v_elem() const = 0;
    virtual int v_blocks(std::vector<VBlock>* out) = 0;
    virtual int v_written() = 0;
    // H0 of the problems with draw[k] != 0 on the device: the Philox stream of snmf_plan_set_h_random keyed by seed[k], element
    // index in the column-major r x T_k matrix; then, for those problems, the initial scaling of H (:159-160) by the norms load()
    // left.  Each of them must have been loaded with H0 == nullptr.
    virtual int draw_h0(const uint64_t* seed, const uint8_t* draw) = 0;
    // H0 of every problem from rows [row0, row0 + r) of the result H of `src` -- another engine of this kind with the same frame
    // counts, whose run has ended -- then the initial scaling of H (:159-160) by the norms load() left: what load() does with
    // a host H0, without H leaving the device.  Every problem must have been loaded with H0 == nullptr.
    virtual int take_h0(snmf_batch& src, int row0) = 0;
    // take_h0 between batches whose problems have ranks of their own: problem k takes rows [row0[k], row0[k] + rank_of(k)) of its
    // source's H (row0: host, B entries; row0[k] + rank_of(k) <= the source's rank of k), then the same scaling.  Either batch may
    // be one with or without ranks or settings.  An engine that has no rank per problem refuses.
    virtual int take_h0_rows(snmf_batch&, const int32_t*) {
        return fail(SNMF_ERR_UNSUPPORTED, "this batch engine hands no activations over between batches with a rank per problem");
    }
    // a masked batch: problem k with its mask (1 = observed), the initial scaling and the masked start (src/snmf_mdi.m:175)
    virtual int load_mdi(int, const double*, int64_t, const double*, int64_t, const double*, const double*) {
        return fail(SNMF_ERR_UNSUPPORTED, "this batch engine has no missing-data form");
    }
    // a masked batch: the gain-matched final imputation (:296-306) of problem k to the host; the problem's state is not written
    virtual int fetch_v_mdi(int, double*, int64_t) { return fail(SNMF_ERR_UNSUPPORTED, "this batch engine has no missing-data form"); }
    virtual int iterate(int it) = 0;  // enqueues iteration it (it_done == it - 1)
    virtual int close_run() = 0;      // enqueues what a run that ends at it_done still owes
    struct Device {                   // what a run reads back: the stopped counter, the B states of the engine's own type, the histories
        const int* n_stopped;
        const void* states;
        void* h_states;
        size_t state_bytes;
        const double *divh, *costh;
    };
    virtual Device device() = 0;
    virtual bool stopped(int k, int* n_iter) const = 0;  // from the states read back last
    virtual int n_recorded(int k) const = 0;             // valid history entries of problem k
    virtual int fetch(int k, double* W, double* H) = 0;  // W and / or H of problem k to the host
    virtual int fetch(int k, float* W, float* H) = 0;
    virtual void describe(char* buf, size_t buflen) const = 0;
};

snmf_batch* batch64_new(bool masked = false);  // snmf_tu_batch64.hip: an fp64 engine (masked: of missing-data solves), not built yet
snmf_batch* batch32_new();                     // snmf_tu_batch.hip: an fp32 engine, not built yet

#define BATCH_CHECK(b)                                          \
    if (!(b)) return fail(SNMF_ERR_INVALID, "batch is NULL");   \
    (void)hipGetLastError();                                    \
    HIP_TRY(hipSetDevice((b)->ctx->device))

// The settings per problem of a batch, checked without a device: the shared fields of p, then every s[k] as the four fields of an
// snmf_params (a refusal names the problem), the scalar sparsity and p->max_iter = the largest limit.  q_out (may be nullptr)
// receives p with T = 1 and the four fields of s[0] in the place of the ones the entry ignores.
inline int batch_check_settings(const char* entry, const snmf_params* p, int32_t n, const snmf_problem_settings* s, snmf_params* q_out) {
    if (!p || !s) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    snmf_params q = *p;
    q.T = 1;  // (ignored: every problem brings its own)
    q.beta = 1.0, q.sparsity_scalar = 0.0, q.conv_eps = 0.0, q.max_iter = 0;
    SN_TRY(validate_params(&q));
    int mi_max = 0;
    for (int k = n - 1; k >= 0; --k) {  // (downwards: q ends with the fields of s[0])
        if (s[k].reserved != 0) return fail(SNMF_ERR_INVALID, "%s: problem %d: reserved must be 0 (got %d)", entry, k, s[k].reserved);
        q.beta = s[k].beta, q.sparsity_scalar = s[k].sparsity, q.conv_eps = s[k].conv_eps, q.max_iter = s[k].max_iter;
        const int rc = validate_params(&q);
        if (rc != SNMF_OK) {
            const std::string why = snmf_last_error();
            return fail(rc, "%s: problem %d: %s", entry, k, why.c_str());
        }
        mi_max = std::max(mi_max, (int)s[k].max_iter);
    }
    if (p->sparsity_kind != SNMF_SPARSITY_SCALAR)
        return fail(SNMF_ERR_UNSUPPORTED, "%s: a batch with settings per problem takes a scalar sparsity", entry);
    if (p->max_iter != mi_max) return fail(SNMF_ERR_DIM, "%s: params->max_iter = %d must be the largest max_iter, %d", entry, p->max_iter, mi_max);
    q.max_iter = mi_max;
    if (q_out) *q_out = q;
    return SNMF_OK;
}

// Takes the engine `b` over (a failure deletes it).  entry: the C entry's name, for the messages.  Every refusal here and the
// engine's own limits come before the device is touched.  with_ranks: r holds a rank per problem (p_in->r is the largest); such a
// batch takes a scalar sparsity and masks that are all ones or all zeros, and has no missing-data form.  with_settings: s holds
// settings per problem (batch_check_settings); such a batch takes a scalar sparsity and has no missing-data form.
inline int batch_create(const char* entry, snmf_batch* b, snmf_ctx* ctx, const snmf_params* p_in, int32_t n_problems, const int32_t* T,
                        snmf_batch** out, bool with_ranks = false, const int32_t* r = nullptr, bool with_settings = false,
                        const snmf_problem_settings* s = nullptr) {
    std::unique_ptr<snmf_batch> own(b);
    if (!ctx || !p_in || !T || !out || (with_ranks && !r) || (with_settings && !s)) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    *out = nullptr;
    if (n_problems < 1) return fail(SNMF_ERR_INVALID, "%s: n_problems must be at least 1 (got %d)", entry, n_problems);
    b->p = *p_in;
    b->p.T = 1;  // (ignored: every problem brings its own)
    if (with_settings) {
        SN_TRY(batch_check_settings(entry, p_in, n_problems, s, &b->p));
        if (b->masked) return fail(SNMF_ERR_UNSUPPORTED, "%s: a missing-data batch has one settings struct for all problems", entry);
        b->settings.assign(s, s + n_problems);
    }
    SN_TRY(validate_params(&b->p));
    if (with_ranks) {
        int r_max = 0;
        for (int i = 0; i < n_problems; ++i) {
            if (r[i] < 1) return fail(SNMF_ERR_INVALID, "%s: problem %d has rank %d (at least 1)", entry, i, r[i]);
            r_max = std::max(r_max, (int)r[i]);
        }
        if (b->p.r != r_max) return fail(SNMF_ERR_DIM, "%s: params->r = %d must be the largest rank, %d", entry, b->p.r, r_max);
        if (b->masked) return fail(SNMF_ERR_UNSUPPORTED, "%s: a missing-data batch has one rank for all problems", entry);
        if (b->p.sparsity_kind != SNMF_SPARSITY_SCALAR)
            return fail(SNMF_ERR_UNSUPPORTED, "%s: a batch with a rank per problem takes a scalar sparsity", entry);
        for (int m = 0; m < 2; ++m) {
            const uint8_t* ind = m ? b->p.h_update_ind : b->p.w_update_ind;
            int n_on = 0;
            for (int k = 0; ind && k < r_max; ++k) n_on += ind[k] != 0;
            if (ind && n_on != 0 && n_on != r_max)
                return fail(SNMF_ERR_UNSUPPORTED, "%s: a batch with a rank per problem takes a %s_update_ind of all ones or all zeros (%d of %d are set)",
                            entry, m ? "h" : "w", n_on, r_max);
        }
        b->ranks.assign(r, r + n_problems);
    }
    int n_h = 0, n_w = 0;
    b->w_ind.resize(b->p.r);
    SN_TRY(read_update_masks(&b->p, &n_h, &n_w, b->w_ind.data()));
    if (b->p.sparsity_kind == SNMF_SPARSITY_FULL)
        return fail(SNMF_ERR_UNSUPPORTED, "the batched solve takes a scalar or an r-vector sparsity, not an r x n matrix");
    SN_TRY(b->check_shape());
    for (int i = 0; i < n_problems; ++i)
        if (T[i] < 1) return fail(SNMF_ERR_INVALID, "problem %d has T = %d frames (at least 1)", i, T[i]);
    b->ctx = ctx;
    b->p.w_update_ind = b->p.h_update_ind = nullptr;
    b->B = n_problems;
    b->upd_h = n_h > 0;
    b->upd_w = n_w > 0;
    b->have.assign(n_problems, 0);
    b->have_s = b->p.sparsity_kind == SNMF_SPARSITY_SCALAR;
    for (int i = 0; i < n_problems; ++i) {
        const snmf_problem_settings si = b->settings_of(i);
        b->any_can_stop |= b->p.cost_check != 0 && si.conv_eps > 0.0;
        b->own_max_iter |= si.max_iter != b->p.max_iter;
    }
    SN_TRY(b->build(T));
    *out = own.release();
    return SNMF_OK;
}

inline int batch_set_sparsity(snmf_batch* b, const double* sparsity) {
    BATCH_CHECK(b);
    if (!sparsity) return fail(SNMF_ERR_INVALID, "sparsity is NULL");
    if (b->p.sparsity_kind != SNMF_SPARSITY_RVEC) return fail(SNMF_ERR_STATE, "the batch was not created with SNMF_SPARSITY_RVEC");
    if (b->ran) return fail(SNMF_ERR_STATE, "snmf_batch_set_sparsity_f64 after snmf_batch_run");
    SN_TRY(b->upload_sparsity(sparsity));
    b->have_s = true;
    return SNMF_OK;
}

// what every set_problem entry does before it loads: the index, and the new batch a set after a run starts
inline int batch_begin_set(snmf_batch* b, int32_t k) {
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (b->ran) {  // a new batch on the same handle: every problem is set again
        std::fill(b->have.begin(), b->have.end(), 0);
        b->n_have = 0;
        b->ran = false;
        b->it_done = 0;
        SN_TRY(b->reset());
    }
    return SNMF_OK;
}
inline void batch_mark_set(snmf_batch* b, int32_t k) {
    if (!b->have[k]) {
        b->have[k] = 1;
        ++b->n_have;
    }
}

template <typename TT>
int batch_set_problem(snmf_batch* b, int32_t k, const TT* V, int64_t ldV, const TT* W0, const TT* H0) {
    BATCH_CHECK(b);
    if (b->masked)  // (refused before anything changes: the handle stays as it was)
        return fail(SNMF_ERR_STATE, "snmf_batch_set_problem on a missing-data batch: its problems are set by snmf_batch_set_problem_mdi_f64");
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (!V || !W0 || !H0) return fail(SNMF_ERR_INVALID, "snmf_batch_set_problem: V, W0 or H0 of problem %d is NULL", k);
    if (ldV < b->p.F) return fail(SNMF_ERR_INVALID, "ldV = %lld is below F = %d", (long long)ldV, b->p.F);
    SN_TRY(batch_begin_set(b, k));
    SN_TRY(b->load(k, V, ldV, W0, H0));
    batch_mark_set(b, k);
    return SNMF_OK;
}

// a problem of a masked batch and its mask in one call: a problem never exists without its mask
inline int batch_set_problem_mdi(snmf_batch* b, int32_t k, const double* V, int64_t ldV, const double* M, int64_t ldM, const double* W0,
                                 const double* H0) {
    BATCH_CHECK(b);
    if (!b->masked)
        return fail(SNMF_ERR_STATE, "snmf_batch_set_problem_mdi_f64 on a batch that was not made by snmf_batch_create_mdi_fp64");
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (!V || !M || !W0 || !H0) return fail(SNMF_ERR_INVALID, "snmf_batch_set_problem_mdi_f64: V, M, W0 or H0 of problem %d is NULL", k);
    if (ldV < b->p.F || ldM < b->p.F)
        return fail(SNMF_ERR_INVALID, "ldV = %lld, ldM = %lld: each must be at least F = %d", (long long)ldV, (long long)ldM, b->p.F);
    SN_TRY(batch_begin_set(b, k));
    SN_TRY(b->load_mdi(k, V, ldV, M, ldM, W0, H0));
    batch_mark_set(b, k);
    return SNMF_OK;
}

inline int batch_run(snmf_batch* b, int32_t n_iters) {
    BATCH_CHECK(b);
    if (n_iters < 0) return fail(SNMF_ERR_INVALID, "n_iters must be >= 0 (0: up to max_iter)");
    if (b->n_have != b->B) return fail(SNMF_ERR_STATE, "snmf_batch_run: %d of %d problems are set", b->n_have, b->B);
    if (!b->have_s) return fail(SNMF_ERR_STATE, "snmf_batch_run: the sparsity vector is not set (snmf_batch_set_sparsity_f64)");
    hipStream_t st = b->ctx->stream;
    const int max_iter = b->p.max_iter;
    const int target = n_iters == 0 ? max_iter : (int)std::min<long long>(max_iter, (long long)b->it_done + n_iters);
    // (some problem can stop before the run's end: by its stop test, or at an iteration limit of its own)
    const bool cc = b->p.cost_check != 0, can_stop = b->any_can_stop || b->own_max_iter;
    const snmf_batch::Device d = b->device();
    b->ran = true;
    // A stopped problem is frozen on the device (its workgroups return at once) and its n_iter comes from its device state, so
    // when the host looks changes no result: it only ends the loop once every problem has stopped.
    int stopped = 0;
    auto poll = [&]() {
        HIP_TRY(hipMemcpyAsync(&stopped, d.n_stopped, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return (int)SNMF_OK;
    };
    if (can_stop && b->it_done > 0) SN_TRY(poll());  // (a batch that has not run has a counter of zero)
    for (int it = b->it_done + 1; it <= target && stopped < b->B; ++it) {
        SN_TRY(b->iterate(it));
        b->it_done = it;
        if (can_stop && it % kPollEvery == 0 && it < max_iter) SN_TRY(poll());  // (at max_iter the closing synchronise follows anyway)
    }
    if (stopped < b->B) SN_TRY(b->close_run());
    const size_t nB = (size_t)b->B, nh = nB * b->hist_len();
    b->h_div.assign(nh, 0.0);
    b->h_cost.assign(nh, 0.0);
    HIP_TRY(hipMemcpyAsync(d.h_states, d.states, d.state_bytes * nB, hipMemcpyDeviceToHost, st));
    if (cc) {
        HIP_TRY(hipMemcpyAsync(b->h_div.data(), d.divh, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(b->h_cost.data(), d.costh, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

template <typename TT>
int batch_get(snmf_batch* b, int32_t k, TT* W, TT* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    BATCH_CHECK(b);
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (!b->ran) return fail(SNMF_ERR_STATE, "snmf_batch_get before snmf_batch_run");
    SN_TRY(b->fetch(k, W, H));
    const int mi = b->p.max_iter, n_rec = b->n_recorded(k);
    const size_t h0 = (size_t)k * b->hist_len();
    for (int i = 0; i < mi; ++i) {
        if (div_out) div_out[i] = i < n_rec ? b->h_div[h0 + i] : 0.0;
        if (cost_out) cost_out[i] = i < n_rec ? b->h_cost[h0 + i] : 0.0;
    }
    int n_iter = 0;
    if (n_iter_out) *n_iter_out = b->stopped(k, &n_iter) ? n_iter : b->it_done;
    return SNMF_OK;
}

// v_MDI of problem k from the state the last run left (after run(n): of the iterate reached); a later run continues unchanged
inline int batch_get_v_mdi(snmf_batch* b, int32_t k, double* V_mdi, int64_t ld) {
    BATCH_CHECK(b);
    if (!b->masked) return fail(SNMF_ERR_STATE, "snmf_batch_get_v_mdi_f64 on a batch that was not made by snmf_batch_create_mdi_fp64");
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (!V_mdi) return fail(SNMF_ERR_INVALID, "V_mdi is NULL");
    if (ld < b->p.F) return fail(SNMF_ERR_INVALID, "ld = %lld is below F = %d", (long long)ld, b->p.F);
    if (!b->ran) return fail(SNMF_ERR_STATE, "snmf_batch_get_v_mdi_f64 before snmf_batch_run");
    return b->fetch_v_mdi(k, V_mdi, ld);
}

// ---- run_basis_DNMF.m:36-55 for a batch of (Y, X, D, B) problems (include/snmf.h: snmf_run_basis_dnmf_batch_*) -----------------
// Three engines of one kind, made by `make`, over the same frame counts: the Y-batch (r = R_x + R_d, H only), the X-batch
// (r = R_x, W only) and the D-batch (r = R_d, W only).  Each phase is one batch_run, so every problem stops each of its three
// solves at its own iteration and the polling is the batch's; between the phases A_hat goes from the Y-engine into the other two
// through take_h0 and never leaves the device.  Like the rest of this file, the driver does not ask which engine it drives.
// The matrix form (dnmf_batch) and the audio form (snmf_run_basis_dnmf_audio_batch_*, snmf_tu_frontend_batch.hip) share it:
// dnmf_batch_phases has the three phases, DnmfInputs says where V and H0 come from.  Two drivers make the engines and say how A_hat
// goes over: dnmf_batch_run (one R_x, one R_d, one settings struct: take_h0) and dnmf_batch_run_ranks (a rank pair and settings per
// problem, the fp64 engine: take_h0_rows).
struct BatchOwner {  // an engine that dies with the call
    snmf_batch* b = nullptr;
    ~BatchOwner() {
        if (!b) return;
        hipSetDevice(b->ctx->device);
        hipStreamSynchronize(b->ctx->stream);
        delete b;
    }
};

// Where V of the three phases and H0 of solve 1 come from.  The matrix form: host arrays, through load().  The audio form
// (snmf_tu_frontend_batch.hip): `device_v` writes the features of every problem of phase `kind` (0, 1, 2: the mixtures, the clean, the
// noise signals) into the blocks the phase's engine hands out, and an H0_k that is not given is drawn on the device from seed[k].
template <typename TT>
struct DnmfInputs {
    const TT* const* V[3] = {nullptr, nullptr, nullptr};  // Y, X, D: tight F x T[k] on the host, or all three nullptr
    std::function<int(int kind, const std::vector<snmf_batch::VBlock>& blocks, size_t elem)> device_v;
    const TT* const* H0 = nullptr;                          // the audio form: may be nullptr, or hold nullptr entries
    const uint64_t* seed = nullptr;                         // n, read where H0_k is not given
};

// The three phases on engines that have been made: e1 the Y-batch, e2 the X-batch, e3 the D-batch.  rx_of(k): the columns of B_k
// (and of B_hat_k) in front of the noise part, R_x of problem k.  hand_over(e, noise): init_h of every problem of e from A_hat in
// e1 -- the first R_x rows, or with `noise` the rows behind them.
template <typename TT, typename RxOf, typename HandOver>
int dnmf_batch_phases(snmf_batch* e1, snmf_batch* e2, snmf_batch* e3, int32_t n, int F, const DnmfInputs<TT>& in, const TT* const* B,
                      TT* const* B_hat, TT* const* A_hat, int32_t* n_iter, RxOf rx_of, HandOver hand_over) {
    // V and init_w = B(:, col0 + (1:r)) of every problem of a phase: from the host through load(), V from the device where it is formed there
    auto set_phase = [&](snmf_batch* e, int kind, bool noise, const TT* const* H0) -> int {
        for (int i = 0; i < n; ++i) {
            const size_t col0 = noise ? (size_t)rx_of(i) : 0;
            SN_TRY(e->load(i, in.V[kind] ? in.V[kind][i] : (const TT*)nullptr, (int64_t)F, B[i] + (size_t)F * col0, H0 ? H0[i] : (const TT*)nullptr));
            batch_mark_set(e, i);
        }
        if (in.V[kind]) return SNMF_OK;
        std::vector<snmf_batch::VBlock> blocks;
        SN_TRY(e->v_blocks(&blocks));
        SN_TRY(in.device_v(kind, blocks, e->v_elem()));
        return e->v_written();
    };
    SN_TRY(set_phase(e1, 0, false, in.H0));  // p.init_w = B   (:39)
    {
        std::vector<uint8_t> draw(n, 0);
        bool any = false;
        for (int i = 0; i < n; ++i) any |= (draw[i] = (!in.H0 || !in.H0[i]) ? 1 : 0) != 0;
        if (any) SN_TRY(e1->draw_h0(in.seed, draw.data()));
    }
    SN_TRY(batch_run(e1, 0));  // [~, A_hat] = sparse_nmf(Y, p)   (:40)
    // a W-only phase: init_h = A_hat(row0 + (1:r), :) from the Y-engine
    auto w_phase = [&](snmf_batch* e, int kind, bool noise) -> int {
        SN_TRY(set_phase(e, kind, noise, nullptr));
        SN_TRY(hand_over(e, noise));
        return batch_run(e, 0);
    };
    SN_TRY(w_phase(e2, 1, false));  // :43-47
    SN_TRY(w_phase(e3, 2, true));   // :49-53
    for (int i = 0; i < n; ++i) {
        int32_t* ni = n_iter ? n_iter + 3 * (size_t)i : nullptr;
        SN_TRY(batch_get<TT>(e1, i, (TT*)nullptr, A_hat ? A_hat[i] : (TT*)nullptr, nullptr, nullptr, ni));
        SN_TRY(batch_get<TT>(e2, i, B_hat[i], (TT*)nullptr, nullptr, nullptr, ni ? ni + 1 : nullptr));  // B_hat = [B_hat_x, B_hat_d]   (:55)
        SN_TRY(batch_get<TT>(e3, i, B_hat[i] + (size_t)F * rx_of(i), (TT*)nullptr, nullptr, nullptr, ni ? ni + 2 : nullptr));
    }
    return SNMF_OK;
}

// Every matrix tight and column-major: Y_k, X_k, D_k F x T[k], B_k F x (R_x + R_d), H0_k (R_x + R_d) x T[k]; B_hat_k and A_hat_k
// likewise (A_hat, or single entries of it, may be NULL); n_iter: NULL or 3 per problem.  The masks of p are ignored (the loop
// sets its own, :37-38, :43-44, :49-50).  Every refusal comes before the device is touched; the caller has checked `in`.
template <typename TT>
int dnmf_batch_run(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n,
                   const int32_t* T, const DnmfInputs<TT>& in, const TT* const* B, TT* const* B_hat, TT* const* A_hat, int32_t* n_iter) {
    // (as loop3_create of snmf_tu_dnmf.hip)
    if (R_x < 1 || R_d < 1 || p->r != R_x + R_d) return fail(SNMF_ERR_DIM, "params->r = %d must equal R_x + R_d = %d + %d", p->r, R_x, R_d);
    if (p->sparsity_kind != SNMF_SPARSITY_SCALAR)
        return fail(SNMF_ERR_DIM, "run_basis_DNMF needs a scalar p.sparsity (its W-only solves have R_x / R_d rows)");
    const std::vector<uint8_t> on(p->r, 1), off(p->r, 0);
    snmf_params q = *p;
    BatchOwner e1, e2, e3;
    q.w_update_ind = off.data(), q.h_update_ind = on.data();  // :37-38
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &e1.b));  // (its limits on F and r are the widest of the three)
    q.w_update_ind = on.data(), q.h_update_ind = off.data();  // :43-44, :49-50
    q.r = R_x;
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &e2.b));
    q.r = R_d;
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &e3.b));
    return dnmf_batch_phases<TT>(e1.b, e2.b, e3.b, n, p->F, in, B, B_hat, A_hat, n_iter, [&](int) { return R_x; },
                                 [&](snmf_batch* e, bool noise) { return e->take_h0(*e1.b, noise ? R_x : 0); });
}

// The same loop with a rank pair (R_x[k], R_d[k]) per problem and, with s, settings per problem (the fp64 engine only: the
// engines are made through the code behind snmf_batch_create_ranks_fp64 / _settings_fp64, which an engine without such a form
// refuses).  The Y-batch has the ranks R_x[k] + R_d[k], the X-batch R_x[k], the D-batch R_d[k]; problem k has the same s[k] in
// all three solves, as the reference passes one p through them (:37-53).  B_k, B_hat_k are F x (R_x[k] + R_d[k]), H0_k, A_hat_k
// (R_x[k] + R_d[k]) x T[k]; p->r must be the largest sum and, with s, p->max_iter the largest limit.  A_hat goes over through
// take_h0_rows.  The uniform driver above launches what it did: this one shares the phases with it and nothing else.
template <typename TT>
int dnmf_batch_run_ranks(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, const int32_t* R_x, const int32_t* R_d,
                         const snmf_problem_settings* s, int32_t n, const int32_t* T, const DnmfInputs<TT>& in, const TT* const* B,
                         TT* const* B_hat, TT* const* A_hat, int32_t* n_iter) {
    if (!R_x || !R_d) return fail(SNMF_ERR_DIM, "%s: R_x and R_d hold a rank per problem (got NULL)", entry);
    std::vector<int32_t> r1(n), rx0(n, 0), rx(R_x, R_x + n);
    int mx = 0, md = 0;
    for (int i = 0; i < n; ++i) {
        if (R_x[i] < 1 || R_d[i] < 1) return fail(SNMF_ERR_DIM, "%s: problem %d has R_x = %d, R_d = %d (at least 1 each)", entry, i, R_x[i], R_d[i]);
        if ((long long)R_x[i] + R_d[i] > 0x7fffffffLL) return fail(SNMF_ERR_DIM, "%s: problem %d: R_x + R_d overflows", entry, i);
        r1[i] = R_x[i] + R_d[i];
        mx = std::max(mx, (int)R_x[i]), md = std::max(md, (int)R_d[i]);
    }
    if (p->sparsity_kind != SNMF_SPARSITY_SCALAR)
        return fail(SNMF_ERR_DIM, "run_basis_DNMF needs a scalar p.sparsity (its W-only solves have R_x / R_d rows)");
    const int m1 = *std::max_element(r1.begin(), r1.end());
    if (p->r != m1) return fail(SNMF_ERR_DIM, "%s: params->r = %d must be the largest R_x + R_d, %d", entry, p->r, m1);
    const std::vector<uint8_t> on(m1, 1), off(m1, 0);
    snmf_params q = *p;
    BatchOwner e1, e2, e3;
    q.w_update_ind = off.data(), q.h_update_ind = on.data();  // :37-38
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &e1.b, true, r1.data(), s != nullptr, s));  // (p->r is the largest sum, or refused)
    q.w_update_ind = on.data(), q.h_update_ind = off.data();  // :43-44, :49-50
    q.r = mx;
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &e2.b, true, R_x, s != nullptr, s));
    q.r = md;
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &e3.b, true, R_d, s != nullptr, s));
    return dnmf_batch_phases<TT>(e1.b, e2.b, e3.b, n, p->F, in, B, B_hat, A_hat, n_iter, [&](int i) { return (int)rx[i]; },
                                 [&](snmf_batch* e, bool noise) { return e->take_h0_rows(*e1.b, noise ? rx.data() : rx0.data()); });
}

// the matrix form (snmf_run_basis_dnmf_batch_*, _ranks_fp64): its own refusals and where V and H0 come from, then the loop on host arrays
template <typename TT>
int dnmf_batch_inputs(const char* entry, snmf_ctx* ctx, const snmf_params* p, int32_t n, const int32_t* T, const TT* const* Y, const TT* const* X,
                      const TT* const* D, const TT* const* B, const TT* const* H0, TT* const* B_hat, DnmfInputs<TT>* in) {
    if (!ctx || !p || !T || !Y || !X || !D || !B || !H0 || !B_hat) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    if (n < 1) return fail(SNMF_ERR_INVALID, "%s: n_problems must be at least 1 (got %d)", entry, n);
    for (int i = 0; i < n; ++i) {
        if (!Y[i] || !X[i] || !D[i] || !B[i] || !H0[i] || !B_hat[i]) return fail(SNMF_ERR_INVALID, "%s: an array of problem %d is NULL", entry, i);
        if (T[i] < 1) return fail(SNMF_ERR_INVALID, "problem %d has T = %d frames (at least 1)", i, T[i]);
    }
    in->V[0] = Y, in->V[1] = X, in->V[2] = D;
    in->H0 = H0;
    return SNMF_OK;
}
template <typename TT>
int dnmf_batch(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n,
               const int32_t* T, const TT* const* Y, const TT* const* X, const TT* const* D, const TT* const* B, const TT* const* H0,
               TT* const* B_hat, TT* const* A_hat, int32_t* n_iter) {
    DnmfInputs<TT> in;
    SN_TRY(dnmf_batch_inputs<TT>(entry, ctx, p, n, T, Y, X, D, B, H0, B_hat, &in));
    return dnmf_batch_run<TT>(entry, make, ctx, p, R_x, R_d, n, T, in, B, B_hat, A_hat, n_iter);
}
// with a rank pair and (s != nullptr) settings per problem
template <typename TT>
int dnmf_batch_ranks(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, const int32_t* R_x, const int32_t* R_d,
                     const snmf_problem_settings* s, int32_t n, const int32_t* T, const TT* const* Y, const TT* const* X, const TT* const* D,
                     const TT* const* B, const TT* const* H0, TT* const* B_hat, TT* const* A_hat, int32_t* n_iter) {
    DnmfInputs<TT> in;
    SN_TRY(dnmf_batch_inputs<TT>(entry, ctx, p, n, T, Y, X, D, B, H0, B_hat, &in));
    return dnmf_batch_run_ranks<TT>(entry, make, ctx, p, R_x, R_d, s, n, T, in, B, B_hat, A_hat, n_iter);
}

// ---- run_basis_train.m:58-91 for a batch of training signals (include/snmf.h: snmf_run_basis_train_audio_batch_*) -----------------
// Two engines of one kind, made by `make`, over the same frame counts, both with every row and column updated (:85-86): the DFT
// engine (p->F rows) and, with F_mel > 0, the Mel engine (F_mel rows), r = p->r = cluster_buff * R each -- or, with `ranks`, problem
// k at ranks[k] = cluster_buff * R_k in both (p->r the largest); with `s`, problem k with the settings s[k] in both.  `device_v` (the grouped
// front-end of snmf_tu_frontend_batch.hip) writes TF_mag -- TF_DD applied where asked -- of every signal into the DFT engine's V
// blocks and TF_Mel, projected from those blocks, into the Mel engine's; both engines then gather their exemplar columns from
// the still unfloored V (the single entry's order, snmf_tu_dnmf.hip), run their floor, take the same H0 and solve.  Nothing
// between the sample slab and the results crosses to the host.  The driver does not ask which engine it drives.
template <typename TT>
struct TrainInputs {
    // the features of every signal into `dft` and, unless it is empty, `mel`: blocks of `elem`-byte entries
    std::function<int(const std::vector<snmf_batch::VBlock>& dft, const std::vector<snmf_batch::VBlock>& mel, size_t elem)> device_v;
    const int64_t* idx = nullptr;    // the exemplar columns of every problem, packed (n * p->r without ranks), 0-based, checked by the caller
    bool exemplar = false;           // train_Exemplar (:84, :93-96): the exemplars are the dictionaries and nothing is solved
    const TT* const* H0 = nullptr;   // may be nullptr, or hold nullptr entries: drawn on the device from seed[k]
    const uint64_t* seed = nullptr;
};

// B_DFT_k F x r, B_Mel_k F_mel x r, A_*_k r x T[k] (r: the problem's own with ranks), tight and column-major (A_DFT, A_Mel, or single entries of them, may be NULL);
// n_iter: NULL or 2 per problem.  The masks of p are ignored.  Every refusal comes before the device is touched; the caller has
// checked `in` and the pointers.
template <typename TT>
int train_batch_run(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, int32_t F_mel, int32_t n, const int32_t* T,
                    const TrainInputs<TT>& in, TT* const* B_DFT, TT* const* A_DFT, TT* const* B_Mel, TT* const* A_Mel, int32_t* n_iter,
                    const int32_t* ranks = nullptr, const snmf_problem_settings* s = nullptr) {
    snmf_params q = *p;
    q.w_update_ind = q.h_update_ind = nullptr;
    if (F_mel > 0) {  // the Mel engine's limits before the DFT engine allocates
        std::unique_ptr<snmf_batch> probe(make());
        probe->p = q;
        probe->p.F = F_mel;
        SN_TRY(probe->check_shape());
    }
    BatchOwner ed, em;
    SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &ed.b, ranks != nullptr, ranks, s != nullptr, s));
    if (F_mel > 0) {
        q.F = F_mel;
        SN_TRY(batch_create(entry, make(), ctx, &q, n, T, &em.b, ranks != nullptr, ranks, s != nullptr, s));
    }
    snmf_batch* const eng[2] = {ed.b, em.b};
    const int n_eng = em.b ? 2 : 1;
    std::vector<snmf_batch::VBlock> vd, vm;
    SN_TRY(ed.b->v_blocks(&vd));
    if (em.b) SN_TRY(em.b->v_blocks(&vm));
    SN_TRY(in.device_v(vd, vm, ed.b->v_elem()));                                      // :60-78
    for (int j = 0; j < n_eng; ++j) SN_TRY(eng[j]->take_w0(in.idx, !in.exemplar));  // B_*_init = TF_*(:, sample_idx)   (:82-83)
    if (in.exemplar) {
        for (int i = 0; i < n; ++i) {
            SN_TRY(ed.b->fetch(i, B_DFT[i], (TT*)nullptr));
            if (em.b) SN_TRY(em.b->fetch(i, B_Mel[i], (TT*)nullptr));
            if (n_iter) n_iter[2 * (size_t)i] = n_iter[2 * (size_t)i + 1] = 0;
        }
        return SNMF_OK;
    }
    for (int j = 0; j < n_eng; ++j) SN_TRY(eng[j]->v_written());
    std::vector<uint8_t> draw(n, 0);
    bool any = false;
    for (int i = 0; i < n; ++i) any |= (draw[i] = (!in.H0 || !in.H0[i]) ? 1 : 0) != 0;
    for (int j = 0; j < n_eng; ++j) {  // the reference re-seeds inside every sparse_nmf call: both solves of a problem start from the same H0
        snmf_batch* e = eng[j];
        for (int i = 0; i < n; ++i) {
            if (!draw[i]) SN_TRY(e->load(i, (const TT*)nullptr, (int64_t)e->p.F, (const TT*)nullptr, in.H0[i]));
            batch_mark_set(e, i);
        }
        if (any) SN_TRY(e->draw_h0(in.seed, draw.data()));
    }
    for (int j = 0; j < n_eng; ++j) SN_TRY(batch_run(eng[j], 0));  // :88, :91
    for (int i = 0; i < n; ++i) {
        int32_t* ni = n_iter ? n_iter + 2 * (size_t)i : nullptr;
        SN_TRY(batch_get<TT>(ed.b, i, B_DFT[i], A_DFT ? A_DFT[i] : (TT*)nullptr, nullptr, nullptr, ni));
        if (em.b) SN_TRY(batch_get<TT>(em.b, i, B_Mel[i], A_Mel ? A_Mel[i] : (TT*)nullptr, nullptr, nullptr, ni ? ni + 1 : nullptr));
        else if (ni) ni[1] = 0;
    }
    return SNMF_OK;
}
