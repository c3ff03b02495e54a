// snmf_tu_batch.hip -- the batched offline solver (include/snmf.h: snmf_batch_*, snmf_sparse_nmf_batch_*): the C entries and the
// fp32 engine, the host side of the kernels in snmf_batch.h.  B independent problems of one (F, r) and one settings struct, each
// with its own frame count, advance in shared launches: per iteration one H step over every (problem, tile), one W-statistics
// launch over every (problem, chunk) and one finish launch over every (problem, column); a problem whose stop test fired is
// frozen on the device.  The life of the handle -- validation, call order, the run loop and its polls of the stopped counter,
// what get() reports -- is snmf_batch_host.h's, shared with the fp64 engine of snmf_tu_batch64.hip; the entries that make a
// handle (snmf_batch_create, _create_fp64 and _create_mdi_fp64: the fp64 engine with masks) are the one place that chooses between
// the engines.  The batched DNMF loop (snmf_run_basis_dnmf_batch_*) is dnmf_batch of the same header on three engines of one kind.
#include "snmf_internal.h"
#include "snmf_batch.h"
#include "snmf_batch_host.h"

namespace {

struct Batch32 final : snmf_batch {
    int bm = BM_KL;
    std::vector<BProb> prob;
    int n_tiles = 0, n_chunks = 0;
    BatchArgs a{};
    int NA = 1, n_fg = 1, n_kg = 1;
    size_t lds_h = 0, lds_w = 0;
    std::vector<void*> blocks;  // every device block of the batch
    double* Wraw = nullptr;
    int cur = 0;
    bool obj_done = false;  // the objective of iterate it_done is folded (the last pass of the previous run)
    std::vector<BState> h_st;

    ~Batch32() override {
        for (void* q : blocks) hipFree(q);
    }
    int check_shape() const override {
        if (p.F > kBMaxF) return fail(SNMF_ERR_UNSUPPORTED, "F = %d is above the batch kernels' limit of %d rows", p.F, kBMaxF);
        if (p.r > kBMaxR) return fail(SNMF_ERR_UNSUPPORTED, "r = %d is above the batch kernels' limit of %d components", p.r, kBMaxR);
        return SNMF_OK;
    }
    int build(const int32_t* T) override;
    int reset() override;
    int upload_sparsity(const double* sparsity) override;
    int load(int k, const double* V, int64_t ldV, const double* W0, const double* H0) override { return load_t(k, V, ldV, W0, H0); }
    int load(int k, const float* V, int64_t ldV, const float* W0, const float* H0) override { return load_t(k, V, ldV, W0, H0); }
    int take_h0(snmf_batch& src, int row0) override;
    int take_w0(const int64_t* idx, bool unit_columns) override;
    size_t v_elem() const override { return sizeof(float); }
    int v_blocks(std::vector<VBlock>* out) override;
    int v_written() override;
    int draw_h0(const uint64_t* seed, const uint8_t* draw) override;
    int iterate(int j) override;
    int close_run() override;
    Device device() override { return Device{a.n_stopped, a.st, h_st.data(), sizeof(BState), a.divh, a.costh}; }
    bool stopped(int k, int* n_iter) const override {
        *n_iter = h_st[k].n_iter;
        return h_st[k].stop != 0;
    }
    int n_recorded(int k) const override { return p.cost_check ? h_st[k].n_rec : 0; }
    int fetch(int k, double* W, double* H) override { return fetch_t(k, W, H); }
    int fetch(int k, float* W, float* H) override { return fetch_t(k, W, H); }
    void describe(char* buf, size_t buflen) const override;

    template <typename TT>
    int load_t(int k, const TT* V, int64_t ldV, const TT* W0, const TT* H0);
    int scale_h0(int k);
    template <typename TT>
    int fetch_t(int k, TT* W, TT* H);
};

int Batch32::reset() {
    cur = 0;
    obj_done = false;
    hipStream_t s = ctx->stream;
    HIP_TRY(hipMemsetAsync(a.st, 0, sizeof(BState) * (size_t)B, s));
    HIP_TRY(hipMemsetAsync(a.n_stopped, 0, sizeof(int), s));
    HIP_TRY(hipMemsetAsync(a.divh, 0, sizeof(double) * (size_t)B * a.max_iter, s));
    HIP_TRY(hipMemsetAsync(a.costh, 0, sizeof(double) * (size_t)B * a.max_iter, s));
    return SNMF_OK;
}

int Batch32::build(const int32_t* T) {
    const int F = p.F, r = p.r, n_problems = B;
    if (!ranks.empty())  // (the LDS geometry nk, nqk, S, nkg of this engine is one per launch; no entry leads here)
        return fail(SNMF_ERR_UNSUPPORTED, "the fp32 batch engine has one rank for all problems (a rank per problem: snmf_batch_create_ranks_fp64)");
    if (!settings.empty())  // (the divergence is a template argument of every launch of this engine; no entry leads here)
        return fail(SNMF_ERR_UNSUPPORTED, "the fp32 batch engine has one settings struct for all problems (settings per problem: snmf_batch_create_settings_fp64)");
    long long tiles = 0, chunks = 0;
    for (int i = 0; i < n_problems; ++i) {
        const long long nt = (T[i] + 31) / 32;
        tiles += nt;
        chunks += (nt + kBChunkTiles - 1) / kBChunkTiles;
    }
    if (tiles > (1LL << 26)) return fail(SNMF_ERR_UNSUPPORTED, "%lld frame tiles are above the batch's limit of 2^26", tiles);
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));

    bm = p.beta == 1.0 ? BM_KL : (p.beta == 2.0 ? BM_EUC : BM_GEN);
    n_tiles = (int)tiles;
    n_chunks = (int)chunks;
    std::vector<BTile> tt((size_t)tiles), cc((size_t)chunks);
    prob.resize(n_problems);
    h_st.resize(n_problems);
    {
        int t0 = 0, c0 = 0;
        for (int i = 0; i < n_problems; ++i) {
            BProb& q = prob[i];
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
    a.n_mat = bm == BM_KL ? 1 : 2;
    a.ldh = a.rp + 4;
    a.cf = std::min(a.nf, bm == BM_KL ? 16 : 8);
    a.ldr = 32 * a.cf + 12;
    a.S = kBW / a.nk;
    a.nfg = std::min(a.nf, bm == BM_KL ? 8 : 4);  // (two images: at most two accumulator pairs per wave)
    a.nkg = std::min(a.nk, bm == BM_KL ? 8 : 4);
    a.ldrw = 32 * a.nfg + 12;
    n_fg = (a.nf + a.nfg - 1) / a.nfg;
    n_kg = (a.nk + a.nkg - 1) / a.nkg;
    {
        const int n_out = a.nfg * a.nkg, na = (n_out + kBW - 1) / kBW;
        NA = na <= 1 ? 1 : (na <= 2 ? 2 : (na <= 4 ? 4 : 8));
    }
    a.max_iter = hist_len();
    a.cost_check = p.cost_check;
    a.beta = (float)p.beta;
    a.inv_bb1 = (p.beta != 0.0 && p.beta != 1.0) ? (float)(1.0 / (p.beta * (p.beta - 1.0))) : 0.f;
    a.conv_eps = p.conv_eps;
    lds_h = 16 * sizeof(double) +
            sizeof(float) * ((size_t)32 * a.ldh + std::max((size_t)a.n_mat * 32 * a.ldr, (size_t)a.nk * a.S * a.n_mat * 1024));
    lds_w = sizeof(float) * ((size_t)32 * a.ldh + (size_t)a.n_mat * 32 * a.ldrw);
    if (std::max(lds_h, lds_w) > ctx->lds_max)
        return fail(SNMF_ERR_UNSUPPORTED, "the batch kernels need %zu bytes of LDS, the device has %zu", std::max(lds_h, lds_w), ctx->lds_max);
    a.sWt = (long long)a.Fm * a.rp;
    a.sWk = (long long)a.Fq * a.rp;
    a.sWc = (long long)a.Fp * a.rp;

    // allocations (zero-filled: the pads of every layout stay zero for the life of the batch, and the state is that of reset())
    int s = SNMF_OK;
    auto alloc = [&](auto** q, size_t n) {
        if (s != SNMF_OK) return;
        s = dalloc(q, n);
        if (s != SNMF_OK) return;
        blocks.push_back((void*)*q);
        using E = typename std::remove_pointer<typename std::remove_pointer<decltype(q)>::type>::type;
        if (hipMemsetAsync((void*)*q, 0, std::max<size_t>(n, 1) * sizeof(E), ctx->stream) != hipSuccess)
            s = fail(SNMF_ERR_NO_DEVICE, "hipMemsetAsync failed");
    };
    const size_t Tt = (size_t)tiles * 32, nB = (size_t)n_problems;
    float *V = nullptr, *lamk = nullptr;
    uint8_t* d_w_ind = nullptr;
    BProb* dprob = nullptr;
    BTile *dtiles = nullptr, *dchunks = nullptr;
    alloc(&V, Tt * a.Fp);
    alloc(&a.H[0], Tt * a.rp);
    alloc(&a.H[1], Tt * a.rp);
    alloc(&a.Wt4, nB * a.sWt);
    alloc(&a.Wk4, nB * a.sWk);
    alloc(&a.Wc, nB * a.sWc);
    alloc(&Wraw, (size_t)a.sWc);
    alloc(&a.wx, nB * a.rp);
    alloc(&a.colsum, nB * a.rp);
    alloc(&a.wn0, nB * a.rp);
    alloc(&lamk, (size_t)a.rp);
    alloc(&d_w_ind, (size_t)r);
    if (upd_w) {
        alloc(&a.slabs, (size_t)chunks * a.n_mat * a.sWc);
        alloc(&a.spart, (size_t)chunks * a.rp);
    }
    alloc(&a.part, (size_t)tiles * 2);
    alloc(&a.divh, nB * a.max_iter);
    alloc(&a.costh, nB * a.max_iter);
    alloc(&dprob, nB);
    alloc(&dtiles, (size_t)tiles);
    alloc(&dchunks, (size_t)chunks);
    alloc(&a.st, nB);
    alloc(&a.n_stopped, 1);
    if (s != SNMF_OK) {
        (void)hipGetLastError();
        return s;
    }
    a.V = V;
    a.Wraw = Wraw;
    a.lamk = lamk;
    a.w_ind = d_w_ind;
    a.prob = dprob;
    a.tiles = dtiles;
    a.chunks = dchunks;
    hipStream_t st = ctx->stream;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        if (s == SNMF_OK && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
            s = fail(SNMF_ERR_NO_DEVICE, "hipMemcpyAsync (batch tables) failed");
    };
    std::vector<float> lk(a.rp, 0.f);
    if (p.sparsity_kind == SNMF_SPARSITY_SCALAR)
        for (int k = 0; k < r; ++k) lk[k] = (float)p.sparsity_scalar;
    up(lamk, lk.data(), sizeof(float) * a.rp);
    up(d_w_ind, w_ind.data(), (size_t)r);
    up(dprob, prob.data(), sizeof(BProb) * nB);
    up(dtiles, tt.data(), sizeof(BTile) * (size_t)tiles);
    up(dchunks, cc.data(), sizeof(BTile) * (size_t)chunks);
    if (s == SNMF_OK && hipStreamSynchronize(st) != hipSuccess) s = fail(SNMF_ERR_NO_DEVICE, "hipStreamSynchronize failed");
    return s;
}

int Batch32::upload_sparsity(const double* sparsity) {
    std::vector<float> lk(a.rp, 0.f);
    for (int k = 0; k < a.r; ++k) lk[k] = (float)sparsity[k];
    HIP_TRY(hipMemcpyAsync(const_cast<float*>(a.lamk), lk.data(), sizeof(float) * a.rp, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (lk leaves scope)
    return SNMF_OK;
}

// wraw: where the init pass reads the initial W (default: the upload buffer of load())
template <int BM>
int launch_fin(Batch32* b, int b0, int nb, int init, int it, int fold, int cur, const double* wraw) {
    BatchArgs q = b->a;
    if (wraw) q.Wraw = wraw;
    hipLaunchKernelGGL((k_bfin<BM>), dim3(b->a.r, nb), dim3(256), 0, b->ctx->stream, q, b0, init, it, fold, cur);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
int launch_fin_bm(Batch32* b, int b0, int nb, int init, int it, int fold, int cur, const double* wraw = nullptr) {
    return b->bm == BM_KL ? launch_fin<BM_KL>(b, b0, nb, init, it, fold, cur, wraw)
                          : (b->bm == BM_EUC ? launch_fin<BM_EUC>(b, b0, nb, init, it, fold, cur, wraw)
                                             : launch_fin<BM_GEN>(b, b0, nb, init, it, fold, cur, wraw));
}

template <typename TT>
int Batch32::load_t(int k, const TT* V, int64_t ldV, const TT* W0, const TT* H0) {
    const BProb& q = prob[k];
    const size_t fr0 = (size_t)q.tile0 * 32;
    const int Tp = q.n_tiles * 32;
    if (V) SN_TRY((xfer_pack_in<TT, float>(ctx, V, ldV, a.F, q.T, const_cast<float*>(a.V) + fr0 * a.Fp, a.Fp, Tp, p.floor_v != 0)));
    if (H0) SN_TRY((xfer_pack_in<TT, float>(ctx, H0, a.r, a.r, q.T, a.H[0] + fr0 * a.rp, a.rp, Tp, false)));
    if (W0) {
        SN_TRY((xfer_pack_in<TT, double>(ctx, W0, a.F, a.F, a.r, Wraw, a.Fp, a.rp, false)));
        SN_TRY(launch_fin_bm(this, k, 1, 1, 0, 0, 0));  // :157-158
    }
    return H0 ? scale_h0(k) : SNMF_OK;
}

int Batch32::scale_h0(int k) {  // :159
    hipLaunchKernelGGL(k_bscale, dim3(std::min(1024, grid_for((size_t)prob[k].T * a.rp))), dim3(256), 0, ctx->stream, a, k);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// One launch over every (problem, tile) of this batch -- the tile table of the H step -- copies the rows from the buffer that holds
// each problem's stop iterate in `src` (what its fetch_t reads); then the scaling load() does, problem by problem.
int Batch32::take_h0(snmf_batch& src_, int row0) {
    const Batch32* src = dynamic_cast<const Batch32*>(&src_);
    if (!src || src == this) return fail(SNMF_ERR_INTERNAL, "take_h0: the source is not another fp32 batch engine");
    if (!src->ran || src->ctx != ctx) return fail(SNMF_ERR_STATE, "take_h0: the source batch has not run on this context");
    if (row0 < 0 || row0 + a.r > src->a.r) return fail(SNMF_ERR_DIM, "take_h0: rows [%d, %d) of an H of %d rows", row0, row0 + a.r, src->a.r);
    if (src->B != B) return fail(SNMF_ERR_DIM, "take_h0: %d problems from a batch of %d", B, src->B);
    for (int k = 0; k < B; ++k)  // (equal frame counts give equal tile tables)
        if (src->prob[k].T != prob[k].T) return fail(SNMF_ERR_DIM, "take_h0: problem %d has %d frames, its source %d", k, prob[k].T, src->prob[k].T);
    cur = 0;
    hipLaunchKernelGGL(k_btake_h, dim3(n_tiles), dim3(256), 0, ctx->stream, a, (const float*)src->a.H[0], (const float*)src->a.H[1],
                       (const BState*)src->a.st, src->cur, src->a.rp, row0);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < B; ++k) SN_TRY(scale_h0(k));
    return SNMF_OK;
}

// One launch over every (problem, element of F x r) gathers the columns, widened, straight into each problem's fp64 master copy,
// which has the layout of load()'s upload buffer.  The initial scaling is then load()'s launch per problem, reading its column
// where it writes it: a workgroup of k_bfin holds its whole column in registers before it stores the first entry.
int Batch32::take_w0(const int64_t* idx, bool unit_columns) {
    if (!idx) return fail(SNMF_ERR_INVALID, "take_w0: NULL argument");
    int64_t* d_idx = nullptr;
    SN_TRY(dalloc(&d_idx, (size_t)B * a.r));
    blocks.push_back(d_idx);
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(d_idx, idx, sizeof(int64_t) * (size_t)B * a.r, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's array may go)
    hipLaunchKernelGGL(k_btake_w, dim3(std::min(1024, grid_for((size_t)a.F * a.r)), B), dim3(256), 0, st, a, (const int64_t*)d_idx, a.Wc,
                       a.sWc);
    HIP_TRY(hipGetLastError());
    if (!unit_columns) return SNMF_OK;
    for (int k = 0; k < B; ++k) SN_TRY(launch_fin_bm(this, k, 1, 1, 0, 0, 0, a.Wc + (size_t)k * a.sWc));  // :157-158
    return SNMF_OK;
}

// The whole V block is zeroed -- the pad rows and pad frames of every problem, as xfer_pack_in leaves them -- and problem k's
// F x T_k entries lie at its first tile, a frame every Fp floats.
int Batch32::v_blocks(std::vector<VBlock>* out) {
    float* V = const_cast<float*>(a.V);
    HIP_TRY(hipMemsetAsync(V, 0, sizeof(float) * (size_t)n_tiles * 32 * a.Fp, ctx->stream));
    out->resize(B);
    for (int k = 0; k < B; ++k) (*out)[k] = VBlock{V + (size_t)prob[k].tile0 * 32 * a.Fp, (int64_t)a.Fp};
    return SNMF_OK;
}

int Batch32::v_written() {  // the floor k_pack applies on the way in (:169), one launch over every problem
    if (!p.floor_v) return SNMF_OK;
    int maxT = 1;
    for (const BProb& q : prob) maxT = std::max(maxT, q.T);
    hipLaunchKernelGGL(k_bfloor_v, dim3(std::min(1024, grid_for((size_t)maxT * a.Fp)), B), dim3(256), 0, ctx->stream, a, const_cast<float*>(a.V));
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int Batch32::draw_h0(const uint64_t* seed, const uint8_t* draw) {
    if (!seed || !draw) return fail(SNMF_ERR_INVALID, "draw_h0: NULL argument");
    uint64_t* d_seed = nullptr;
    uint8_t* d_draw = nullptr;
    SN_TRY(dalloc(&d_seed, (size_t)B));
    blocks.push_back(d_seed);
    SN_TRY(dalloc(&d_draw, (size_t)B));
    blocks.push_back(d_draw);
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(d_seed, seed, sizeof(uint64_t) * (size_t)B, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_draw, draw, (size_t)B, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's arrays may go)
    int max_tiles = 1;
    for (const BProb& q : prob) max_tiles = std::max(max_tiles, q.n_tiles);
    cur = 0;
    hipLaunchKernelGGL(k_brand_h, dim3(std::min(1024, grid_for((size_t)max_tiles * 32 * a.rp)), B), dim3(256), 0, st, a, (const uint64_t*)d_seed,
                       (const uint8_t*)d_draw);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < B; ++k)
        if (draw[k]) SN_TRY(scale_h0(k));
    return SNMF_OK;
}

template <int BM>
int launch_bh(Batch32* b, int cur, int upd, int obj) {
    SN_TRY(ensure_dyn_lds(b->ctx->device, (const void*)k_bh<BM>, b->lds_h));
    hipLaunchKernelGGL((k_bh<BM>), dim3(b->n_tiles), dim3(kBThr), b->lds_h, b->ctx->stream, b->a, cur, upd, obj);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
int launch_bh_bm(Batch32* b, int cur, int upd, int obj) {
    return b->bm == BM_KL ? launch_bh<BM_KL>(b, cur, upd, obj)
                          : (b->bm == BM_EUC ? launch_bh<BM_EUC>(b, cur, upd, obj) : launch_bh<BM_GEN>(b, cur, upd, obj));
}
template <int BM, int NA>
int launch_bw(Batch32* b, int hn) {
    SN_TRY(ensure_dyn_lds(b->ctx->device, (const void*)k_bw<BM, NA>, b->lds_w));
    hipLaunchKernelGGL((k_bw<BM, NA>), dim3(b->n_chunks, b->n_fg, b->n_kg), dim3(kBThr), b->lds_w, b->ctx->stream, b->a, hn);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
template <int BM>
int launch_bw_na(Batch32* b, int hn) {
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
int launch_bw_bm(Batch32* b, int hn) {
    return b->bm == BM_KL ? launch_bw_na<BM_KL>(b, hn) : (b->bm == BM_EUC ? launch_bw_na<BM_EUC>(b, hn) : launch_bw_na<BM_GEN>(b, hn));
}
int launch_fold(Batch32* b, int j, int cur) {
    hipLaunchKernelGGL(k_bfold, dim3(b->B), dim3(256), 0, b->ctx->stream, b->a, j, cur);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int Batch32::iterate(int j) {
    // the objective of iterate j - 1 is what the H step of iteration j reads (Lam = W * H of that iterate)
    const int fold = (p.cost_check && j > 1 && !obj_done) ? 1 : 0;
    if (upd_h || fold) SN_TRY(launch_bh_bm(this, cur, upd_h ? 1 : 0, fold));
    const int hn = upd_h ? cur ^ 1 : cur;
    if (upd_w) {
        SN_TRY(launch_bw_bm(this, hn));
        SN_TRY(launch_fin_bm(this, 0, B, 0, j, fold, cur));
    } else if (fold) {
        SN_TRY(launch_fold(this, j - 1, cur));
    }
    cur = hn;
    obj_done = false;
    return SNMF_OK;
}

int Batch32::close_run() {
    if (p.cost_check && it_done >= 1 && !obj_done) {  // the objective (and the stop test) of the last iterate
        SN_TRY(launch_bh_bm(this, cur, 0, 1));
        SN_TRY(launch_fold(this, it_done, cur));
        obj_done = true;
    }
    return SNMF_OK;
}

template <typename TT>
int Batch32::fetch_t(int k, TT* W, TT* H) {
    const BProb& q = prob[k];
    const BState& s = h_st[k];
    if (W) SN_TRY((xfer_unpack_out<TT, double>(ctx, a.Wc + (size_t)k * a.sWc, a.Fp, a.F, a.r, W, a.F)));
    if (H) {
        const float* src = a.H[s.stop ? s.hsel : cur] + (size_t)q.tile0 * 32 * a.rp;
        SN_TRY((xfer_unpack_out<TT, float>(ctx, src, a.rp, a.r, q.T, H, a.r)));
    }
    return SNMF_OK;
}

void Batch32::describe(char* buf, size_t buflen) const {
    const char* bmn = bm == BM_KL ? "kl" : (bm == BM_EUC ? "ed" : "beta");
    snprintf(buf, buflen,
             "batch B=%d F=%d r=%d %s upd_h=%d upd_w=%d xr=%d nf=%d nk=%d tiles=%d chunks=%d | k_bh grid=%d x%d lds=%zu cf=%d S=%d | "
             "k_bw grid=(%d,%d,%d) x%d lds=%zu NA=%d | k_bfin grid=(%d,%d) x256 | poll_every=%d",
             B, a.F, a.r, bmn, (int)upd_h, (int)upd_w, a.xr, a.nf, a.nk, n_tiles, n_chunks, n_tiles, kBThr, lds_h, a.cf, a.S, n_chunks,
             n_fg, n_kg, kBThr, lds_w, NA, a.r, B, kPollEvery);
}

}  // namespace

// ---- the C entries: the driver of snmf_batch_host.h on whichever engine the handle was made with ------------------------------
extern "C" int snmf_batch_create(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out) {
    return batch_create("snmf_batch_create", new Batch32(), ctx, p, n_problems, T, out);
}
extern "C" int snmf_batch_create_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out) {
    return batch_create("snmf_batch_create_fp64", batch64_new(), ctx, p, n_problems, T, out);
}
extern "C" int snmf_batch_create_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const int32_t* r,
                                            snmf_batch** out) {
    return batch_create("snmf_batch_create_ranks_fp64", batch64_new(), ctx, p, n_problems, T, out, true, r);
}
extern "C" int snmf_batch_create_settings_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, const int32_t* r,
                                               const snmf_problem_settings* s, snmf_batch** out) {
    const char* entry = "snmf_batch_create_settings_fp64";
    if (!s) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return batch_create(entry, batch64_new(), ctx, p, n_problems, T, out, r != nullptr, r, true, s);
}
extern "C" int snmf_batch_create_mdi_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, snmf_batch** out) {
    return batch_create("snmf_batch_create_mdi_fp64", batch64_new(true), ctx, p, n_problems, T, out);
}
extern "C" void snmf_batch_destroy(snmf_batch* b) {
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
    delete b;
}
extern "C" int snmf_batch_set_sparsity_f64(snmf_batch* b, const double* sparsity) { return batch_set_sparsity(b, sparsity); }
extern "C" int snmf_batch_set_problem_f64(snmf_batch* b, int32_t k, const double* V, int64_t ldV, const double* W0, const double* H0) {
    return batch_set_problem<double>(b, k, V, ldV, W0, H0);
}
extern "C" int snmf_batch_set_problem_f32(snmf_batch* b, int32_t k, const float* V, int64_t ldV, const float* W0, const float* H0) {
    return batch_set_problem<float>(b, k, V, ldV, W0, H0);
}
extern "C" int snmf_batch_set_problem_mdi_f64(snmf_batch* b, int32_t k, const double* V, int64_t ldV, const double* M, int64_t ldM,
                                              const double* W0, const double* H0) {
    return batch_set_problem_mdi(b, k, V, ldV, M, ldM, W0, H0);
}
extern "C" int snmf_batch_get_v_mdi_f64(snmf_batch* b, int32_t k, double* V_mdi, int64_t ld) { return batch_get_v_mdi(b, k, V_mdi, ld); }
extern "C" int snmf_batch_run(snmf_batch* b, int32_t n_iters) { return batch_run(b, n_iters); }
extern "C" int snmf_batch_get_f64(snmf_batch* b, int32_t k, double* W, double* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    return batch_get<double>(b, k, W, H, div_out, cost_out, n_iter_out);
}
extern "C" int snmf_batch_get_f32(snmf_batch* b, int32_t k, float* W, float* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    return batch_get<float>(b, k, W, H, div_out, cost_out, n_iter_out);
}
extern "C" int snmf_batch_describe(const snmf_batch* b, char* buf, size_t buflen) {
    if (!b || !buf || buflen == 0) return fail(SNMF_ERR_INVALID, "snmf_batch_describe: NULL argument");
    b->describe(buf, buflen);
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
    for (int i = 0; i < n; ++i) SN_STEP(s, batch_set_problem<TT>(b, i, V[i], ldV[i], W0[i], H0[i]));
    SN_STEP(s, snmf_batch_run(b, 0));
    for (int i = 0; i < n; ++i)
        SN_STEP(s, batch_get<TT>(b, i, W[i], H[i], div_out ? div_out[i] : nullptr, cost_out ? cost_out[i] : nullptr,
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

// the missing-data one-shot: create_mdi, set every problem with its mask, run to the end, get, read v_MDI, destroy
extern "C" int snmf_mdi_batch_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t n, const int32_t* T, const double* const* V,
                                   const int64_t* ldV, const double* const* M, const int64_t* ldM, const double* const* W0,
                                   const double* const* H0, const double* sparsity, double* const* V_mdi, const int64_t* ldVm,
                                   double* const* W, double* const* H, double* const* div_out, double* const* cost_out,
                                   int32_t* n_iter_out) {
    if (!ctx || !p || !T || !V || !ldV || !M || !ldM || !W0 || !H0 || !V_mdi || !H) return fail(SNMF_ERR_INVALID, "snmf_mdi_batch_fp64: NULL argument");
    if (p->sparsity_kind == SNMF_SPARSITY_RVEC && !sparsity) return fail(SNMF_ERR_INVALID, "SNMF_SPARSITY_RVEC needs the sparsity vector");
    for (int i = 0; i < n; ++i)
        if (!V[i] || !M[i] || !W0[i] || !H0[i] || !V_mdi[i] || !H[i])
            return fail(SNMF_ERR_INVALID, "snmf_mdi_batch_fp64: an array of problem %d is NULL", i);
    // every leading dimension before anything runs: ldVm[i] is only looked at when problem i is read back, after the solve and
    // after the results of the problems before it have been written
    for (int i = 0; i < n; ++i)
        if (ldV[i] < p->F || ldM[i] < p->F || (ldVm && ldVm[i] < p->F))
            return fail(SNMF_ERR_INVALID, "snmf_mdi_batch_fp64: problem %d has ldV = %lld, ldM = %lld, ldVm = %lld: each must be at least F = %d", i,
                        (long long)ldV[i], (long long)ldM[i], (long long)(ldVm ? ldVm[i] : p->F), p->F);
    snmf_batch* b = nullptr;
    SN_TRY(snmf_batch_create_mdi_fp64(ctx, p, n, T, &b));
    int s = SNMF_OK;
    if (p->sparsity_kind == SNMF_SPARSITY_RVEC) SN_STEP(s, snmf_batch_set_sparsity_f64(b, sparsity));
    for (int i = 0; i < n; ++i) SN_STEP(s, batch_set_problem_mdi(b, i, V[i], ldV[i], M[i], ldM[i], W0[i], H0[i]));
    SN_STEP(s, snmf_batch_run(b, 0));
    for (int i = 0; i < n; ++i) {
        SN_STEP(s, batch_get<double>(b, i, W ? W[i] : nullptr, H[i], div_out ? div_out[i] : nullptr, cost_out ? cost_out[i] : nullptr,
                                     n_iter_out ? n_iter_out + i : nullptr));
        SN_STEP(s, batch_get_v_mdi(b, i, V_mdi[i], ldVm ? ldVm[i] : (int64_t)p->F));
    }
    snmf_batch_destroy(b);
    return s;
}

// run_basis_DNMF for a batch: dnmf_batch of snmf_batch_host.h on three engines of the entry's kind
snmf_batch* batch32_new() { return new Batch32(); }
static snmf_batch* make32() { return batch32_new(); }
static snmf_batch* make64() { return batch64_new(); }
extern "C" int snmf_run_basis_dnmf_batch_f64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n_problems,
                                             const int32_t* T, const double* const* Y, const double* const* X, const double* const* D,
                                             const double* const* B, const double* const* H0, double* const* B_hat, double* const* A_hat,
                                             int32_t* n_iter) {
    return dnmf_batch<double>("snmf_run_basis_dnmf_batch_f64", make32, ctx, p, R_x, R_d, n_problems, T, Y, X, D, B, H0, B_hat, A_hat, n_iter);
}
extern "C" int snmf_run_basis_dnmf_batch_f32(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n_problems,
                                             const int32_t* T, const float* const* Y, const float* const* X, const float* const* D,
                                             const float* const* B, const float* const* H0, float* const* B_hat, float* const* A_hat,
                                             int32_t* n_iter) {
    return dnmf_batch<float>("snmf_run_basis_dnmf_batch_f32", make32, ctx, p, R_x, R_d, n_problems, T, Y, X, D, B, H0, B_hat, A_hat, n_iter);
}
extern "C" int snmf_run_basis_dnmf_batch_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, int32_t n_problems,
                                              const int32_t* T, const double* const* Y, const double* const* X, const double* const* D,
                                              const double* const* B, const double* const* H0, double* const* B_hat, double* const* A_hat,
                                              int32_t* n_iter) {
    return dnmf_batch<double>("snmf_run_basis_dnmf_batch_fp64", make64, ctx, p, R_x, R_d, n_problems, T, Y, X, D, B, H0, B_hat, A_hat, n_iter);
}
extern "C" int snmf_run_basis_dnmf_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const int32_t* R_x, const int32_t* R_d,
                                                    const snmf_problem_settings* s, int32_t n_problems, const int32_t* T,
                                                    const double* const* Y, const double* const* X, const double* const* D,
                                                    const double* const* B, const double* const* H0, double* const* B_hat,
                                                    double* const* A_hat, int32_t* n_iter) {
    return dnmf_batch_ranks<double>("snmf_run_basis_dnmf_batch_ranks_fp64", make64, ctx, p, R_x, R_d, s, n_problems, T, Y, X, D, B, H0, B_hat,
                                    A_hat, n_iter);
}
