// snmf_tu_batch.hip -- the batched offline solver (include/snmf.h: snmf_batch_*, snmf_sparse_nmf_batch_*): host driver of the
// kernels in snmf_batch.h.  B independent problems of one (F, r) and one settings struct, each with its own frame count,
// advance in shared launches: per iteration one H step over every (problem, tile), one W-statistics launch over every
// (problem, chunk) and one finish launch over every (problem, column); a problem whose stop test fired is frozen on the
// device and the host only polls a counter of stopped problems every kPollEvery iterations.
// A handle made by snmf_batch_create_fp64 carries the fp64 state of snmf_tu_batch64.hip instead (b->b64): every entry below
// hands such a handle over at its top, and nothing else of the fp32 batch knows about it.
#include "snmf_internal.h"
#include "snmf_batch.h"
#include "snmf_batch64_host.h"

namespace {
constexpr int kPollEvery = 8;
}

struct snmf_batch {
    Batch64* b64 = nullptr;  // the fp64 mode: the whole state of the batch (only ctx is filled in here)
    snmf_ctx* ctx = nullptr;
    snmf_params p{};
    int B = 0, bm = BM_KL;
    bool upd_h = true, upd_w = true;
    std::vector<uint8_t> w_ind;
    std::vector<BProb> prob;
    int n_tiles = 0, n_chunks = 0;
    BatchArgs a{};
    int NA = 1, n_fg = 1, n_kg = 1;
    size_t lds_h = 0, lds_w = 0;
    std::vector<void*> blocks;  // every device block of the batch
    double* Wraw = nullptr;
    BState* st = nullptr;
    int* n_stopped = nullptr;
    // state
    std::vector<uint8_t> have;
    int n_have = 0;
    bool have_s = false, ran = false;
    int cur = 0, it_done = 0;
    bool obj_done = false;  // the objective of iterate it_done is folded (the last pass of the previous run)
    std::vector<BState> h_st;
    std::vector<double> h_div, h_cost;
};

static void batch_free(snmf_batch* b) {
    batch64_destroy(b->b64);
    for (void* q : b->blocks) hipFree(q);
    delete b;
}

static int batch_reset(snmf_batch* b) {
    std::fill(b->have.begin(), b->have.end(), 0);
    b->n_have = 0;
    b->ran = false;
    b->cur = 0;
    b->it_done = 0;
    b->obj_done = false;
    hipStream_t st = b->ctx->stream;
    HIP_TRY(hipMemsetAsync(b->st, 0, sizeof(BState) * (size_t)b->B, st));
    HIP_TRY(hipMemsetAsync(b->n_stopped, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(b->a.divh, 0, sizeof(double) * (size_t)b->B * std::max(1, b->p.max_iter), st));
    HIP_TRY(hipMemsetAsync(b->a.costh, 0, sizeof(double) * (size_t)b->B * std::max(1, b->p.max_iter), st));
    return SNMF_OK;
}

#define BATCH_CHECK(b)                                          \
    if (!(b)) return fail(SNMF_ERR_INVALID, "batch is NULL");   \
    (void)hipGetLastError();                                    \
    HIP_TRY(hipSetDevice((b)->ctx->device))

extern "C" void snmf_batch_destroy(snmf_batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    batch_free(b);
}

extern "C" int snmf_batch_create(snmf_ctx* ctx, const snmf_params* p_in, int32_t n_problems, const int32_t* T, snmf_batch** out) {
    if (!ctx || !p_in || !T || !out) return fail(SNMF_ERR_INVALID, "snmf_batch_create: NULL argument");
    *out = nullptr;
    if (n_problems < 1) return fail(SNMF_ERR_INVALID, "snmf_batch_create: n_problems must be at least 1 (got %d)", n_problems);
    snmf_params p = *p_in;
    p.T = 1;  // (ignored: every problem brings its own)
    SN_TRY(validate_params(&p));
    const int F = p.F, r = p.r;
    int n_h = 0, n_w = 0;
    for (int k = 0; k < r; ++k) {
        n_h += p.h_update_ind ? p.h_update_ind[k] != 0 : 1;
        n_w += p.w_update_ind ? p.w_update_ind[k] != 0 : 1;
    }
    if (n_h != 0 && n_h != r)
        return fail(SNMF_ERR_DIM, "partial h_update_ind (%d of %d rows): dimension mismatch in src/sparse_nmf.m:192/197/202", n_h, r);
    if (p.sparsity_kind == SNMF_SPARSITY_FULL)
        return fail(SNMF_ERR_UNSUPPORTED, "the batched solve takes a scalar or an r-vector sparsity, not an r x n matrix");
    if (F > kBMaxF) return fail(SNMF_ERR_UNSUPPORTED, "F = %d is above the batch kernels' limit of %d rows", F, kBMaxF);
    if (r > kBMaxR) return fail(SNMF_ERR_UNSUPPORTED, "r = %d is above the batch kernels' limit of %d components", r, kBMaxR);
    long long tiles = 0, chunks = 0;
    for (int i = 0; i < n_problems; ++i) {
        if (T[i] < 1) return fail(SNMF_ERR_INVALID, "problem %d has T = %d frames (at least 1)", i, T[i]);
        const long long nt = (T[i] + 31) / 32;
        tiles += nt;
        chunks += (nt + kBChunkTiles - 1) / kBChunkTiles;
    }
    if (tiles > (1LL << 26)) return fail(SNMF_ERR_UNSUPPORTED, "%lld frame tiles are above the batch's limit of 2^26", tiles);
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));

    snmf_batch* b = new snmf_batch();
    b->ctx = ctx;
    b->p = p;
    b->p.w_update_ind = b->p.h_update_ind = nullptr;
    b->B = n_problems;
    b->upd_h = n_h > 0;
    b->upd_w = n_w > 0;
    b->bm = p.beta == 1.0 ? BM_KL : (p.beta == 2.0 ? BM_EUC : BM_GEN);
    b->w_ind.resize(r);
    for (int k = 0; k < r; ++k) b->w_ind[k] = p.w_update_ind ? p.w_update_ind[k] != 0 : 1;
    b->have.assign(n_problems, 0);
    b->n_tiles = (int)tiles;
    b->n_chunks = (int)chunks;
    std::vector<BTile> tt((size_t)tiles), cc((size_t)chunks);
    b->prob.resize(n_problems);
    {
        int t0 = 0, c0 = 0;
        for (int i = 0; i < n_problems; ++i) {
            BProb& q = b->prob[i];
            q.T = T[i];
            q.tile0 = t0;
            q.n_tiles = (T[i] + 31) / 32;
            q.chunk0 = c0;
            q.n_chunks = (q.n_tiles + kBChunkTiles - 1) / kBChunkTiles;
            for (int l = 0; l < q.n_tiles; ++l) tt[(size_t)t0 + l] = BTile{i, l};
            for (int l = 0; l < q.n_chunks; ++l) cc[(size_t)c0 + l] = BTile{i, l};
            t0 += q.n_tiles;
            c0 += q.n_chunks;
        }
    }
    // geometry
    BatchArgs& a = b->a;
    a.F = F;
    a.r = r;
    a.xr = (F > 32 && F % 32 == 1) ? 1 : 0;
    a.nf = a.xr ? (F - 1) / 32 : (F + 31) / 32;
    a.Fm = 32 * a.nf;
    a.Fp = a.xr ? a.Fm + 4 : a.Fm;
    a.Fq = a.xr ? a.Fm + 8 : a.Fm;
    a.nk = (r + 31) / 32;
    a.rp = 32 * a.nk;
    a.nqk = (r + 7) / 8;
    a.n_mat = b->bm == BM_KL ? 1 : 2;
    a.ldh = a.rp + 4;
    a.cf = std::min(a.nf, b->bm == BM_KL ? 16 : 8);
    a.ldr = 32 * a.cf + 12;
    a.S = kBW / a.nk;
    a.nfg = std::min(a.nf, b->bm == BM_KL ? 8 : 4);  // (two images: at most two accumulator pairs per wave)
    a.nkg = std::min(a.nk, b->bm == BM_KL ? 8 : 4);
    a.ldrw = 32 * a.nfg + 12;
    b->n_fg = (a.nf + a.nfg - 1) / a.nfg;
    b->n_kg = (a.nk + a.nkg - 1) / a.nkg;
    {
        const int n_out = a.nfg * a.nkg, na = (n_out + kBW - 1) / kBW;
        b->NA = na <= 1 ? 1 : (na <= 2 ? 2 : (na <= 4 ? 4 : 8));
    }
    a.max_iter = std::max(1, p.max_iter);
    a.cost_check = p.cost_check;
    a.beta = (float)p.beta;
    a.inv_bb1 = (p.beta != 0.0 && p.beta != 1.0) ? (float)(1.0 / (p.beta * (p.beta - 1.0))) : 0.f;
    a.conv_eps = p.conv_eps;
    b->lds_h = 16 * sizeof(double) +
               sizeof(float) * ((size_t)32 * a.ldh + std::max((size_t)a.n_mat * 32 * a.ldr, (size_t)a.nk * a.S * a.n_mat * 1024));
    b->lds_w = sizeof(float) * ((size_t)32 * a.ldh + (size_t)a.n_mat * 32 * a.ldrw);
    if (std::max(b->lds_h, b->lds_w) > ctx->lds_max) {
        const size_t need = std::max(b->lds_h, b->lds_w);
        delete b;
        return fail(SNMF_ERR_UNSUPPORTED, "the batch kernels need %zu bytes of LDS, the device has %zu", need, ctx->lds_max);
    }
    a.sWt = (long long)a.Fm * a.rp;
    a.sWk = (long long)a.Fq * a.rp;
    a.sWc = (long long)a.Fp * a.rp;

    // allocations (zero-filled: the pads of every layout stay zero for the life of the batch)
    int s = SNMF_OK;
    auto alloc = [&](auto** q, size_t n) {
        if (s != SNMF_OK) return;
        s = dalloc(q, n);
        if (s != SNMF_OK) return;
        b->blocks.push_back((void*)*q);
        using E = typename std::remove_pointer<typename std::remove_pointer<decltype(q)>::type>::type;
        if (hipMemsetAsync((void*)*q, 0, std::max<size_t>(n, 1) * sizeof(E), ctx->stream) != hipSuccess)
            s = fail(SNMF_ERR_NO_DEVICE, "hipMemsetAsync failed");
    };
    const size_t Tt = (size_t)tiles * 32, nB = (size_t)n_problems;
    float *V = nullptr, *lamk = nullptr;
    uint8_t* w_ind = nullptr;
    BProb* dprob = nullptr;
    BTile *dtiles = nullptr, *dchunks = nullptr;
    alloc(&V, Tt * a.Fp);
    alloc(&a.H[0], Tt * a.rp);
    alloc(&a.H[1], Tt * a.rp);
    alloc(&a.Wt4, nB * a.sWt);
    alloc(&a.Wk4, nB * a.sWk);
    alloc(&a.Wc, nB * a.sWc);
    alloc(&b->Wraw, (size_t)a.sWc);
    alloc(&a.wx, nB * a.rp);
    alloc(&a.colsum, nB * a.rp);
    alloc(&a.wn0, nB * a.rp);
    alloc(&lamk, (size_t)a.rp);
    alloc(&w_ind, (size_t)r);
    if (b->upd_w) {
        alloc(&a.slabs, (size_t)chunks * a.n_mat * a.sWc);
        alloc(&a.spart, (size_t)chunks * a.rp);
    }
    alloc(&a.part, (size_t)tiles * 2);
    alloc(&a.divh, nB * a.max_iter);
    alloc(&a.costh, nB * a.max_iter);
    alloc(&dprob, nB);
    alloc(&dtiles, (size_t)tiles);
    alloc(&dchunks, (size_t)chunks);
    alloc(&b->st, nB);
    alloc(&b->n_stopped, 1);
    if (s != SNMF_OK) {
        (void)hipGetLastError();
        batch_free(b);
        return s;
    }
    a.V = V;
    a.Wraw = b->Wraw;
    a.lamk = lamk;
    a.w_ind = w_ind;
    a.prob = dprob;
    a.tiles = dtiles;
    a.chunks = dchunks;
    a.st = b->st;
    a.n_stopped = b->n_stopped;
    hipStream_t st = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        if (s == SNMF_OK && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
            s = fail(SNMF_ERR_NO_DEVICE, "hipMemcpyAsync (batch tables) failed");
    };
    std::vector<float> lk(a.rp, 0.f);
    if (p.sparsity_kind == SNMF_SPARSITY_SCALAR) {
        for (int k = 0; k < r; ++k) lk[k] = (float)p.sparsity_scalar;
        b->have_s = true;
    }
    up(lamk, lk.data(), sizeof(float) * a.rp);
    up(w_ind, b->w_ind.data(), (size_t)r);
    up(dprob, b->prob.data(), sizeof(BProb) * nB);
    up(dtiles, tt.data(), sizeof(BTile) * (size_t)tiles);
    up(dchunks, cc.data(), sizeof(BTile) * (size_t)chunks);
    if (s == SNMF_OK && hipStreamSynchronize(st) != hipSuccess) s = fail(SNMF_ERR_NO_DEVICE, "hipStreamSynchronize failed");
    if (s != SNMF_OK) {
        batch_free(b);
        return s;
    }
    *out = b;
    return SNMF_OK;
}

extern "C" int snmf_batch_create_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out) {
    if (!ctx || !p || !T || !out) return fail(SNMF_ERR_INVALID, "snmf_batch_create_fp64: NULL argument");
    *out = nullptr;
    Batch64* b64 = nullptr;
    SN_TRY(batch64_create(ctx, p, n_problems, T, &b64));
    snmf_batch* b = new snmf_batch();
    b->ctx = ctx;
    b->b64 = b64;
    *out = b;
    return SNMF_OK;
}

extern "C" int snmf_batch_set_sparsity_f64(snmf_batch* b, const double* sparsity) {
    BATCH_CHECK(b);
    if (b->b64) return batch64_set_sparsity(b->b64, sparsity);
    if (!sparsity) return fail(SNMF_ERR_INVALID, "sparsity is NULL");
    if (b->p.sparsity_kind != SNMF_SPARSITY_RVEC) return fail(SNMF_ERR_STATE, "the batch was not created with SNMF_SPARSITY_RVEC");
    if (b->ran) return fail(SNMF_ERR_STATE, "snmf_batch_set_sparsity_f64 after snmf_batch_run");
    std::vector<float> lk(b->a.rp, 0.f);
    for (int k = 0; k < b->a.r; ++k) lk[k] = (float)sparsity[k];
    HIP_TRY(hipMemcpyAsync(const_cast<float*>(b->a.lamk), lk.data(), sizeof(float) * b->a.rp, hipMemcpyHostToDevice, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));  // (lk leaves scope)
    b->have_s = true;
    return SNMF_OK;
}

template <int BM>
static int launch_fin(snmf_batch* b, int b0, int nb, int init, int it, int fold, int cur) {
    hipLaunchKernelGGL((k_bfin<BM>), dim3(b->a.r, nb), dim3(256), 0, b->ctx->stream, b->a, b0, init, it, fold, cur);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
static int launch_fin_bm(snmf_batch* b, int b0, int nb, int init, int it, int fold, int cur) {
    return b->bm == BM_KL ? launch_fin<BM_KL>(b, b0, nb, init, it, fold, cur)
                          : (b->bm == BM_EUC ? launch_fin<BM_EUC>(b, b0, nb, init, it, fold, cur)
                                             : launch_fin<BM_GEN>(b, b0, nb, init, it, fold, cur));
}

template <typename TT>
static int set_problem(snmf_batch* b, int32_t k, const TT* V, int64_t ldV, const TT* W0, const TT* H0) {
    BATCH_CHECK(b);
    if (b->b64) return batch64_set_problem(b->b64, k, V, ldV, W0, H0);
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (!V || !W0 || !H0) return fail(SNMF_ERR_INVALID, "snmf_batch_set_problem: V, W0 or H0 of problem %d is NULL", k);
    if (ldV < b->a.F) return fail(SNMF_ERR_INVALID, "ldV = %lld is below F = %d", (long long)ldV, b->a.F);
    if (b->ran) SN_TRY(batch_reset(b));  // a new batch on the same handle: every problem is set again
    const BatchArgs& a = b->a;
    const BProb& q = b->prob[k];
    const size_t fr0 = (size_t)q.tile0 * 32;
    const int Tp = q.n_tiles * 32;
    SN_TRY((xfer_pack_in<TT, float>(b->ctx, V, ldV, a.F, q.T, const_cast<float*>(a.V) + fr0 * a.Fp, a.Fp, Tp, b->p.floor_v != 0)));
    SN_TRY((xfer_pack_in<TT, float>(b->ctx, H0, a.r, a.r, q.T, a.H[0] + fr0 * a.rp, a.rp, Tp, false)));
    SN_TRY((xfer_pack_in<TT, double>(b->ctx, W0, a.F, a.F, a.r, b->Wraw, a.Fp, a.rp, false)));
    SN_TRY(launch_fin_bm(b, k, 1, 1, 0, 0, 0));  // :157-158
    hipLaunchKernelGGL(k_bscale, dim3(std::min(1024, grid_for((size_t)q.T * a.rp))), dim3(256), 0, b->ctx->stream, a, (int)k);  // :159
    HIP_TRY(hipGetLastError());
    if (!b->have[k]) {
        b->have[k] = 1;
        ++b->n_have;
    }
    return SNMF_OK;
}
extern "C" int snmf_batch_set_problem_f64(snmf_batch* b, int32_t k, const double* V, int64_t ldV, const double* W0, const double* H0) {
    return set_problem<double>(b, k, V, ldV, W0, H0);
}
extern "C" int snmf_batch_set_problem_f32(snmf_batch* b, int32_t k, const float* V, int64_t ldV, const float* W0, const float* H0) {
    return set_problem<float>(b, k, V, ldV, W0, H0);
}

template <int BM>
static int launch_bh(snmf_batch* b, int cur, int upd, int obj) {
    SN_TRY(ensure_dyn_lds(b->ctx->device, (const void*)k_bh<BM>, b->lds_h));
    hipLaunchKernelGGL((k_bh<BM>), dim3(b->n_tiles), dim3(kBThr), b->lds_h, b->ctx->stream, b->a, cur, upd, obj);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
static int launch_bh_bm(snmf_batch* b, int cur, int upd, int obj) {
    return b->bm == BM_KL ? launch_bh<BM_KL>(b, cur, upd, obj)
                          : (b->bm == BM_EUC ? launch_bh<BM_EUC>(b, cur, upd, obj) : launch_bh<BM_GEN>(b, cur, upd, obj));
}
template <int BM, int NA>
static int launch_bw(snmf_batch* b, int hn) {
    SN_TRY(ensure_dyn_lds(b->ctx->device, (const void*)k_bw<BM, NA>, b->lds_w));
    hipLaunchKernelGGL((k_bw<BM, NA>), dim3(b->n_chunks, b->n_fg, b->n_kg), dim3(kBThr), b->lds_w, b->ctx->stream, b->a, hn);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
template <int BM>
static int launch_bw_na(snmf_batch* b, int hn) {
    switch (b->NA) {
        case 1: return launch_bw<BM, 1>(b, hn);
        case 2: return launch_bw<BM, 2>(b, hn);
        case 4:
            if (BM == BM_KL) return launch_bw<BM_KL, 4>(b, hn);
            break;
        case 8:
            if (BM == BM_KL) return launch_bw<BM_KL, 8>(b, hn);
            break;
    }
    return fail(SNMF_ERR_INTERNAL, "batch W statistics: no kernel for %d accumulators", b->NA);
}
static int launch_bw_bm(snmf_batch* b, int hn) {
    return b->bm == BM_KL ? launch_bw_na<BM_KL>(b, hn) : (b->bm == BM_EUC ? launch_bw_na<BM_EUC>(b, hn) : launch_bw_na<BM_GEN>(b, hn));
}
static int launch_fold(snmf_batch* b, int j, int cur) {
    hipLaunchKernelGGL(k_bfold, dim3(b->B), dim3(256), 0, b->ctx->stream, b->a, j, cur);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

extern "C" int snmf_batch_run(snmf_batch* b, int32_t n_iters) {
    BATCH_CHECK(b);
    if (b->b64) return batch64_run(b->b64, n_iters);
    if (n_iters < 0) return fail(SNMF_ERR_INVALID, "n_iters must be >= 0 (0: up to max_iter)");
    if (b->n_have != b->B) return fail(SNMF_ERR_STATE, "snmf_batch_run: %d of %d problems are set", b->n_have, b->B);
    if (!b->have_s) return fail(SNMF_ERR_STATE, "snmf_batch_run: the sparsity vector is not set (snmf_batch_set_sparsity_f64)");
    hipStream_t st = b->ctx->stream;
    const int max_iter = b->p.max_iter;
    const int target = n_iters == 0 ? max_iter : (int)std::min<long long>(max_iter, (long long)b->it_done + n_iters);
    const bool cc = b->p.cost_check != 0, can_stop = cc && b->p.conv_eps > 0.0;
    b->ran = true;
    int stopped = 0;
    if (can_stop) {
        HIP_TRY(hipMemcpyAsync(&stopped, b->n_stopped, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    int since_poll = 0;
    for (int j = b->it_done + 1; j <= target && stopped < b->B; ++j) {
        // the objective of iterate j - 1 is what the H step of iteration j reads (Lam = W * H of that iterate)
        const int fold = (cc && j > 1 && !b->obj_done) ? 1 : 0;
        if (b->upd_h || fold) SN_TRY(launch_bh_bm(b, b->cur, b->upd_h ? 1 : 0, fold));
        const int hn = b->upd_h ? b->cur ^ 1 : b->cur;
        if (b->upd_w) {
            SN_TRY(launch_bw_bm(b, hn));
            SN_TRY(launch_fin_bm(b, 0, b->B, 0, j, fold, b->cur));
        } else if (fold) {
            SN_TRY(launch_fold(b, j - 1, b->cur));
        }
        b->cur = hn;
        b->it_done = j;
        b->obj_done = false;
        if (can_stop && ++since_poll >= kPollEvery) {
            since_poll = 0;
            HIP_TRY(hipMemcpyAsync(&stopped, b->n_stopped, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    if (cc && b->it_done >= 1 && !b->obj_done && stopped < b->B) {  // the objective (and the stop test) of the last iterate
        SN_TRY(launch_bh_bm(b, b->cur, 0, 1));
        SN_TRY(launch_fold(b, b->it_done, b->cur));
        b->obj_done = true;
    }
    const size_t nB = (size_t)b->B, nh = nB * b->a.max_iter;
    b->h_st.resize(nB);
    b->h_div.resize(nh);
    b->h_cost.resize(nh);
    HIP_TRY(hipMemcpyAsync(b->h_st.data(), b->st, sizeof(BState) * nB, hipMemcpyDeviceToHost, st));
    if (cc) {
        HIP_TRY(hipMemcpyAsync(b->h_div.data(), b->a.divh, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(b->h_cost.data(), b->a.costh, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

template <typename TT>
static int get_problem(snmf_batch* b, int32_t k, TT* W, TT* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    BATCH_CHECK(b);
    if (b->b64) return batch64_get(b->b64, k, W, H, div_out, cost_out, n_iter_out);
    if (k < 0 || k >= b->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, b->B);
    if (!b->ran) return fail(SNMF_ERR_STATE, "snmf_batch_get before snmf_batch_run");
    const BatchArgs& a = b->a;
    const BProb& q = b->prob[k];
    const BState& s = b->h_st[k];
    const int n_iter = s.stop ? s.n_iter : b->it_done;
    if (W) SN_TRY((xfer_unpack_out<TT, double>(b->ctx, a.Wc + (size_t)k * a.sWc, a.Fp, a.F, a.r, W, a.F)));
    if (H) {
        const float* src = a.H[s.stop ? s.hsel : b->cur] + (size_t)q.tile0 * 32 * a.rp;
        SN_TRY((xfer_unpack_out<TT, float>(b->ctx, src, a.rp, a.r, q.T, H, a.r)));
    }
    const int mi = b->p.max_iter;
    for (int i = 0; i < mi; ++i) {
        const bool rec = b->p.cost_check && i < s.n_rec;
        if (div_out) div_out[i] = rec ? b->h_div[(size_t)k * a.max_iter + i] : 0.0;
        if (cost_out) cost_out[i] = rec ? b->h_cost[(size_t)k * a.max_iter + i] : 0.0;
    }
    if (n_iter_out) *n_iter_out = n_iter;
    return SNMF_OK;
}
extern "C" int snmf_batch_get_f64(snmf_batch* b, int32_t k, double* W, double* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    return get_problem<double>(b, k, W, H, div_out, cost_out, n_iter_out);
}
extern "C" int snmf_batch_get_f32(snmf_batch* b, int32_t k, float* W, float* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    return get_problem<float>(b, k, W, H, div_out, cost_out, n_iter_out);
}

extern "C" int snmf_batch_describe(const snmf_batch* b, char* buf, size_t buflen) {
    if (!b || !buf || buflen == 0) return fail(SNMF_ERR_INVALID, "snmf_batch_describe: NULL argument");
    if (b->b64) return batch64_describe(b->b64, buf, buflen);
    const BatchArgs& a = b->a;
    const char* bmn = b->bm == BM_KL ? "kl" : (b->bm == BM_EUC ? "ed" : "beta");
    snprintf(buf, buflen,
             "batch B=%d F=%d r=%d %s upd_h=%d upd_w=%d xr=%d nf=%d nk=%d tiles=%d chunks=%d | k_bh grid=%d x%d lds=%zu cf=%d S=%d | "
             "k_bw grid=(%d,%d,%d) x%d lds=%zu NA=%d | k_bfin grid=(%d,%d) x256 | poll_every=%d",
             b->B, a.F, a.r, bmn, (int)b->upd_h, (int)b->upd_w, a.xr, a.nf, a.nk, b->n_tiles, b->n_chunks, b->n_tiles, kBThr, b->lds_h,
             a.cf, a.S, b->n_chunks, b->n_fg, b->n_kg, kBThr, b->lds_w, b->NA, a.r, b->B, kPollEvery);
    return SNMF_OK;
}

template <typename TT>
static int batch_oneshot(snmf_ctx* ctx, const snmf_params* p, int32_t n, const int32_t* T, const TT* const* V, const int64_t* ldV,
                         const TT* const* W0, const TT* const* H0, const double* sparsity, TT* const* W, TT* const* H,
                         double* const* div_out, double* const* cost_out, int32_t* n_iter_out, bool fp64 = false) {
    if (!ctx || !p || !T || !V || !ldV || !W0 || !H0 || !W || !H) return fail(SNMF_ERR_INVALID, "snmf_sparse_nmf_batch: NULL argument");
    if (p->sparsity_kind == SNMF_SPARSITY_RVEC && !sparsity) return fail(SNMF_ERR_INVALID, "SNMF_SPARSITY_RVEC needs the sparsity vector");
    for (int i = 0; i < n; ++i)
        if (!V[i] || !W0[i] || !H0[i] || !W[i] || !H[i]) return fail(SNMF_ERR_INVALID, "snmf_sparse_nmf_batch: an array of problem %d is NULL", i);
    snmf_batch* b = nullptr;
    SN_TRY(fp64 ? snmf_batch_create_fp64(ctx, p, n, T, &b) : snmf_batch_create(ctx, p, n, T, &b));
    int s = SNMF_OK;
    if (p->sparsity_kind == SNMF_SPARSITY_RVEC) SN_STEP(s, snmf_batch_set_sparsity_f64(b, sparsity));
    for (int i = 0; i < n; ++i) SN_STEP(s, set_problem<TT>(b, i, V[i], ldV[i], W0[i], H0[i]));
    SN_STEP(s, snmf_batch_run(b, 0));
    for (int i = 0; i < n; ++i)
        SN_STEP(s, get_problem<TT>(b, i, W[i], H[i], div_out ? div_out[i] : nullptr, cost_out ? cost_out[i] : nullptr,
                                   n_iter_out ? n_iter_out + i : nullptr));
    snmf_batch_destroy(b);
    return s;
}
extern "C" int snmf_sparse_nmf_batch_f64(snmf_ctx* ctx, const snmf_params* p, int32_t n, const int32_t* T, const double* const* V,
                                         const int64_t* ldV, const double* const* W0, const double* const* H0, const double* sparsity,
                                         double* const* W, double* const* H, double* const* div_out, double* const* cost_out,
                                         int32_t* n_iter_out) {
    return batch_oneshot<double>(ctx, p, n, T, V, ldV, W0, H0, sparsity, W, H, div_out, cost_out, n_iter_out);
}
extern "C" int snmf_sparse_nmf_batch_f32(snmf_ctx* ctx, const snmf_params* p, int32_t n, const int32_t* T, const float* const* V,
                                         const int64_t* ldV, const float* const* W0, const float* const* H0, const double* sparsity,
                                         float* const* W, float* const* H, double* const* div_out, double* const* cost_out,
                                         int32_t* n_iter_out) {
    return batch_oneshot<float>(ctx, p, n, T, V, ldV, W0, H0, sparsity, W, H, div_out, cost_out, n_iter_out);
}
extern "C" int snmf_sparse_nmf_batch_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n, const int32_t* T, const double* const* V,
                                          const int64_t* ldV, const double* const* W0, const double* const* H0, const double* sparsity,
                                          double* const* W, double* const* H, double* const* div_out, double* const* cost_out,
                                          int32_t* n_iter_out) {
    return batch_oneshot<double>(ctx, p, n, T, V, ldV, W0, H0, sparsity, W, H, div_out, cost_out, n_iter_out, true);
}
