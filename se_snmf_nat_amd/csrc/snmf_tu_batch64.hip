// snmf_tu_batch64.hip -- the fp64 engine of a batched offline solve (snmf_batch_create_fp64): the host side of the grouped
// kernels in snmf_batch64.h, behind the driver of snmf_batch_host.h.  An iteration is solve64_run's (snmf_tu_solve64.hip), launch
// for launch, with every launch grouped over the problems; the tables that map a workgroup to (problem, tile, split) and the
// per-problem GEMM arguments are built once, when the batch is made, from the frame counts and the addresses of the one device
// block.  A translation unit of its own: the fp32 batch, its kernels and its geometry are not touched.
// A masked engine (snmf_batch_create_mdi_fp64) is the same engine with solve64_run's missing-data steps: one more F x sum(T_b)
// block for the masks, the masked start when a problem is set, the grouped re-imputation (fused with the objective when there is
// one) at the end of an iteration, and the gain-matched final imputation into a scratch block when v_MDI is read.  Without masks
// nothing of this is allocated or launched.
// With a rank per problem (snmf_batch_create_ranks_fp64) nothing else is launched either: the tables are built from r_i where they
// were built from r, the packed arrays are sized by the sums of r_i and r_i T_i, and the grids that count columns or rows of a
// rank-sized matrix are sized for the largest rank.
// With settings per problem (snmf_batch_create_settings_fp64) the problems may differ in divergence: the passes compiled per
// divergence are launched once per divergence present, the second H and W products (the denominators) have tile and sum tables
// over the problems that are not KL, the column and row sums cover the KL problems, and a Euclidean problem's products read V
// and Lam where the others read R and D.  With one divergence present the launches of an iteration are what they were.
#include "snmf_internal.h"
#include "snmf_batch64.h"
#include "snmf_batch_host.h"
#include "snmf_host64.h"

namespace {

constexpr int kElemGridMax = 2048;  // workgroups per problem of an element-wise pass (grid-stride beyond)
constexpr long long kGridXMax = 0x7fffffffLL;
constexpr int kGridYMax = 65535;

inline long long tiles_of(int M, int N) { return (long long)((M + 63) / 64) * ((N + 63) / 64); }

struct Family {  // the table of one product family: Lam = W*H | W'*R, W'*D | R*H', D*H'
    B64Tile* tiles = nullptr;
    long long n = 0;
};
struct Product {  // one product of a family: every problem's arguments, and the problems whose partials are to be added
    Gemm64Args* args = nullptr;
    B64Sum* sums = nullptr;
    int n_sums = 0;
    long long sum_n_max = 0;
};

struct Batch64 final : snmf_batch {
    bool has[4] = {false, false, false, false};  // the modes (S64_*) present among the problems
    int n_modes = 0, min_mi = 0;                 // distinct modes; the smallest iteration limit (a.max_iter is the largest)
    bool any_kl = false, any_nonkl = false;
    std::vector<uint8_t> limit_at;               // cost_check = 0 with settings: some problem's own limit is iteration it
    std::vector<B64Prob> prob;
    std::vector<long long> z0;  // first double of each problem's split partials
    long long sumT = 0, sumRz = 0, sumZ = 0;
    long long sumR = 0, sumRT = 0, sumSp = 0;  // columns of W, elements of H, row-sum partials of all problems
    int maxT = 0, max_rowz = 0, min_r = 0;
    B64Args a{};
    double* S = nullptr;
    double* zbuf = nullptr;
    double* Mblk = nullptr;   // masked: the masks, F x sum(T_b) at V's frame offsets (a.M is the kernels' read-only view)
    double* Vm = nullptr;     // masked: F x max T_b, where the final imputation of one problem is formed before it is copied out
    size_t mask_bytes = 0;
    bool lam_done = false;    // Lam = max(W * H, flr) of the scaled initial factors has been formed since the last reset
    B64Prob* dprob = nullptr;
    uint8_t* dwi = nullptr;
    Family fLam, fH, fW, fHd, fWd;  // fHd, fWd: the H and W families over the problems that are not KL (pDen, pP)
    Product pLam, pNum, pDen, pQ, pP;
    B64Sum* sRow = nullptr;  // the row sums of H of the KL problems, n_row entries
    int n_row = 0;
    void* block = nullptr;
    size_t bytes = 0;
    int launches = 0;  // per iteration
    std::vector<Solve64State> h_st;

    ~Batch64() override {
        if (block) hipFree(block);
    }
    int build(const int32_t* T) override;
    int reset() override;
    int upload_sparsity(const double* sparsity) override;
    int load(int k, const double* V, int64_t ldV, const double* W0, const double* H0) override { return load_t(k, V, ldV, W0, H0); }
    int load(int k, const float* V, int64_t ldV, const float* W0, const float* H0) override { return load_t(k, V, ldV, W0, H0); }
    int load_mdi(int k, const double* V, int64_t ldV, const double* M, int64_t ldM, const double* W0, const double* H0) override {
        return load_t(k, V, ldV, W0, H0, M, ldM);
    }
    int take_h0(snmf_batch& src, int row0) override;
    int take_h0_rows(snmf_batch& src, const int32_t* row0) override;
    int take_w0(const int64_t* idx, bool unit_columns) override;
    size_t v_elem() const override { return sizeof(double); }
    int v_blocks(std::vector<VBlock>* out) override;
    int v_written() override;
    int draw_h0(const uint64_t* seed, const uint8_t* draw) override;
    int fetch_v_mdi(int k, double* V_mdi, int64_t ld) override;
    int iterate(int it) override;
    int close_run() override { return SNMF_OK; }  // (the objective and the stop test of an iteration run inside it)
    Device device() override { return Device{a.n_stopped, a.st, h_st.data(), sizeof(Solve64State), a.divh, a.costh}; }
    bool stopped(int k, int* n_iter) const override {
        *n_iter = h_st[k].n_iter;
        return h_st[k].stop != 0;
    }
    int n_recorded(int) const override { return p.max_iter; }  // (the device histories are zero where nothing was recorded)
    int fetch(int k, double* W, double* H) override { return fetch_t(k, W, H); }
    int fetch(int k, float* W, float* H) override { return fetch_t(k, W, H); }
    void describe(char* buf, size_t buflen) const override;

    template <typename TT>
    int load_t(int k, const TT* V, int64_t ldV, const TT* W0, const TT* H0, const TT* M = nullptr, int64_t ldM = 0);
    int scale_h0(int k);
    template <typename TT>
    int fetch_t(int k, TT* W, TT* H);
};

// the walk over the device block (the same for measuring and for carving)
size_t carve(Batch64* s, void* base) {
    const snmf_params& p = s->p;
    const size_t F = p.F, r = p.r, nB = s->B, sT = (size_t)s->sumT, sR = (size_t)s->sumR, sRT = (size_t)s->sumRT;
    // kl / ed: every problem is; a mixed batch has the arrays of every mode present, each sized for all problems
    const bool kl = !s->any_nonkl, ed = !s->has[S64_KL] && !s->has[S64_IS] && !s->has[S64_GEN];
    const bool need_d = s->has[S64_IS] || s->has[S64_GEN], need_kl = s->any_kl;
    B64Args& a = s->a;
    Carve64 c(base);
    a.V = c.get<double>(F * sT);
    a.Lam = c.get<double>(F * sT);
    s->Mblk = s->Vm = nullptr;
    if (s->masked) {
        s->Mblk = c.get<double>(F * sT);
        s->Vm = c.get<double>(F * (size_t)s->maxT);
    }
    a.M = s->Mblk;
    a.R = ed ? nullptr : c.get<double>(F * sT);
    a.D = need_d ? c.get<double>(F * sT) : nullptr;
    a.H = c.get<double>(sRT);
    a.W = c.get<double>(F * sR);
    a.Num = a.Den = a.cs = a.Q = a.P = a.hs = a.sp = nullptr;
    if (s->upd_h) {
        a.Num = c.get<double>(sRT);
        if (!kl) a.Den = c.get<double>(sRT);
        if (need_kl) a.cs = c.get<double>(sR);
    }
    if (s->upd_w) {
        a.Q = c.get<double>(F * sR);
        if (!kl) a.P = c.get<double>(F * sR);
        if (need_kl) {
            a.hs = c.get<double>(sR);
            a.sp = c.get<double>((size_t)s->sumSp);
        }
    }
    s->zbuf = s->sumZ ? c.get<double>((size_t)s->sumZ) : nullptr;
    a.wn = c.get<double>(sR);
    a.part = c.get<double>(nB * 2 * kS64Blocks);
    a.divh = c.get<double>(nB * a.max_iter);
    a.costh = c.get<double>(nB * a.max_iter);
    s->S = p.sparsity_kind == SNMF_SPARSITY_RVEC ? c.get<double>(r) : nullptr;
    a.st = c.get<Solve64State>(nB);
    a.n_stopped = c.get<int>(1);
    s->dwi = c.get<uint8_t>(r);
    s->dprob = c.get<B64Prob>(nB);
    s->fLam.tiles = c.get<B64Tile>((size_t)s->fLam.n);
    s->pLam.args = c.get<Gemm64Args>(nB);
    s->pLam.sums = c.get<B64Sum>(nB);
    if (s->upd_h) {
        s->fH.tiles = c.get<B64Tile>((size_t)s->fH.n);
        s->pNum.args = c.get<Gemm64Args>(nB);
        s->pNum.sums = c.get<B64Sum>(nB);
        if (!kl) {
            s->fHd.tiles = c.get<B64Tile>((size_t)s->fHd.n);
            s->pDen.args = c.get<Gemm64Args>(nB);
            s->pDen.sums = c.get<B64Sum>(nB);
        }
    }
    if (s->upd_w) {
        s->fW.tiles = c.get<B64Tile>((size_t)s->fW.n);
        s->pQ.args = c.get<Gemm64Args>(nB);
        s->pQ.sums = c.get<B64Sum>(nB);
        if (!kl) {
            s->fWd.tiles = c.get<B64Tile>((size_t)s->fWd.n);
            s->pP.args = c.get<Gemm64Args>(nB);
            s->pP.sums = c.get<B64Sum>(nB);
        }
        if (need_kl) s->sRow = c.get<B64Sum>(nB);
    }
    a.S = s->S;
    a.w_ind = s->dwi;
    a.prob = s->dprob;
    return c.off;
}

int Batch64::reset() {
    hipStream_t st = ctx->stream;
    const size_t nB = (size_t)B;
    h_st.assign(nB, Solve64State{0, 0, INFINITY});  // src/sparse_nmf.m:168
    lam_done = false;
    int n0 = 0;  // settings per problem: a problem with max_iter = 0 beside others is stopped before the first iteration
    if (a.own_limit)
        for (size_t k = 0; k < nB; ++k)
            if (prob[k].max_iter == 0) h_st[k].stop = 1, ++n0;
    HIP_TRY(hipMemcpyAsync(a.st, h_st.data(), sizeof(Solve64State) * nB, hipMemcpyHostToDevice, st));
    if (n0) HIP_TRY(hipMemcpyAsync(a.n_stopped, &n0, sizeof(int), hipMemcpyHostToDevice, st));  // (the synchronise below keeps n0 alive)
    else HIP_TRY(hipMemsetAsync(a.n_stopped, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(a.divh, 0, sizeof(double) * nB * a.max_iter, st));  // :171-173
    HIP_TRY(hipMemsetAsync(a.costh, 0, sizeof(double) * nB * a.max_iter, st));
    HIP_TRY(hipStreamSynchronize(st));  // (h_st is a pageable source, and the next run reads the states back into it)
    return SNMF_OK;
}

// Checks the grid and memory limits before anything is allocated, then allocates and builds the tables.
int Batch64::build(const int32_t* T) {
    const int F = p.F, n_problems = B;
    if (n_problems > kGridYMax)
        return fail(SNMF_ERR_UNSUPPORTED, "%d problems are above the fp64 batch's limit of %d (a launch grid's second dimension)", n_problems,
                    kGridYMax);

    // ---- sizes, from the frame counts, the ranks and the modes alone
    prob.resize(n_problems);
    z0.resize(n_problems);
    min_r = rank_of(0);
    min_mi = settings_of(0).max_iter;
    for (int i = 0; i < n_problems; ++i) {
        B64Prob& q = prob[i];
        const int r = rank_of(i);
        const snmf_problem_settings si = settings_of(i);  // (the one settings struct on a handle made without settings per problem)
        q.mode = si.beta == 1.0 ? S64_KL : (si.beta == 2.0 ? S64_ED : (si.beta == 0.0 ? S64_IS : S64_GEN));
        q.max_iter = si.max_iter;
        q.beta = si.beta;
        q.div_scale = q.mode == S64_GEN ? si.beta * (si.beta - 1.0) : 1.0;
        q.sparsity = si.sparsity;
        q.conv_eps = si.conv_eps;
        has[q.mode] = true;
        min_mi = std::min(min_mi, (int)si.max_iter);
        q.T = T[i];
        q.n_rowz = (T[i] + kS64RowChunk - 1) / kS64RowChunk;
        q.r = r;
        q.fr0 = sumT;
        q.rz0 = sumRz;
        q.h0 = sumRT;
        q.w0 = sumR;
        q.sp0 = sumSp;
        sumT += T[i];
        sumRz += q.n_rowz;
        sumRT += (long long)r * T[i];
        sumR += r;
        sumSp += (long long)r * q.n_rowz;
        min_r = std::min(min_r, r);
        maxT = std::max(maxT, T[i]);
        max_rowz = std::max(max_rowz, q.n_rowz);
        fLam.n += tiles_of(F, T[i]) * n_splits(r, kS64ChunkK);
        if (upd_h) fH.n += tiles_of(r, T[i]) * n_splits(F, kS64ChunkK);
        if (upd_w) fW.n += tiles_of(F, r) * n_splits(T[i], kS64ChunkK);
        if (q.mode != S64_KL) {  // the denominators W' * D and D * H'
            if (upd_h) fHd.n += tiles_of(r, T[i]) * n_splits(F, kS64ChunkK);
            if (upd_w) fWd.n += tiles_of(F, r) * n_splits(T[i], kS64ChunkK);
        }
        // split partials: the largest over this problem's products (carve64 of the single solve)
        size_t need = split_partials(F, T[i], r, kS64ChunkK);
        if (upd_h) need = std::max(need, split_partials(r, T[i], F, kS64ChunkK));
        if (upd_w) need = std::max(need, split_partials(F, r, T[i], kS64ChunkK));
        z0[i] = sumZ;
        sumZ += (long long)need;
    }
    // ---- grid limits, before anything is allocated
    const long long most = std::max(fLam.n, std::max(fH.n, fW.n));
    if (most > kGridXMax)
        return fail(SNMF_ERR_UNSUPPORTED, "%lld tiles in one grouped product are above the launch grid's limit of %lld", most, kGridXMax);
    if (max_rowz > kGridYMax)
        return fail(SNMF_ERR_UNSUPPORTED, "T = %d frames give %d row-sum chunks, above the launch grid's limit of %d", maxT, max_rowz,
                    kGridYMax);
    a.F = F, a.r = p.r;
    a.kind = p.sparsity_kind;
    a.max_iter = std::max(1, p.max_iter);
    a.own_limit = settings.empty() ? 0 : 1;
    n_modes = (int)has[0] + (int)has[1] + (int)has[2] + (int)has[3];
    any_kl = has[S64_KL];
    any_nonkl = n_modes > (any_kl ? 1 : 0);
    const bool kl = !any_nonkl;
    if (a.own_limit && !p.cost_check) {  // the iterations after which k_b64_limit has a problem to stop
        limit_at.assign((size_t)p.max_iter + 1, 0);
        for (const B64Prob& q : prob) limit_at[q.max_iter] = 1;
    }
    bytes = carve(this, nullptr);
    mask_bytes = masked ? sizeof(double) * (size_t)F * (size_t)sumT : 0;

    // ---- the device
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    if (bytes > mem_free)
        return fail(SNMF_ERR_UNSUPPORTED, "the fp64 batch needs %zu bytes of device memory, %zu of %zu are free", bytes, mem_free, mem_total);
    {
        hipError_t e = hipMalloc(&block, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            block = nullptr;
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
    }
    if (carve(this, block) != bytes) return fail(SNMF_ERR_INTERNAL, "fp64 batch: the two walks over the device block differ");

    // ---- tables: per problem the arguments gemm64() makes for it alone, then (split, tile) in the single launch's order
    std::vector<B64Tile> tLam((size_t)fLam.n), tH((size_t)fH.n), tW((size_t)fW.n), tHd((size_t)fHd.n), tWd((size_t)fWd.n);
    std::vector<Gemm64Args> gLam(n_problems), gNum(n_problems), gDen(n_problems), gQ(n_problems), gP(n_problems);
    std::vector<B64Sum> uLam, uNum, uDen, uQ, uP, uRow;
    auto split_entry = [&](std::vector<B64Sum>& u, Product& pr, double* zb, int nz, double* C, long long rsC, long long csC, int M, int N,
                           bool do_floor, const int* stop) {
        if (nz == 1) return;
        const long long n = (long long)M * N;
        u.push_back(B64Sum{zb, C, n, rsC, csC, nz, M, do_floor ? 1 : 0, stop});
        pr.sum_n_max = std::max(pr.sum_n_max, n);
    };
    auto add_tiles = [&](std::vector<B64Tile>& t, size_t& at, int i, const Gemm64Args& g, int nz) {
        const int nt = (int)s64_gemm_tiles(g);
        for (int z = 0; z < nz; ++z)
            for (int l = 0; l < nt; ++l) t[at++] = B64Tile{i, l, z};
    };
    size_t atLam = 0, atH = 0, atW = 0, atHd = 0, atWd = 0;
    for (int i = 0; i < n_problems; ++i) {
        const B64Prob& q = prob[i];
        const int Ti = q.T, r = q.r;
        const bool kl_i = q.mode == S64_KL, ed_i = q.mode == S64_ED;
        const double* Rm = ed_i ? a.V : a.R;  // Euclidean: R = V, D = Lam are used where they lie
        const double* Dm = ed_i ? a.Lam : a.D;
        const long long oFT = q.fr0 * F, oRT = q.h0, oFR = q.w0 * F;
        double* zb = zbuf ? zbuf + z0[i] : nullptr;
        const int* stop = &a.st[i].stop;
        double *W = a.W + oFR, *H = a.H + oRT;
        {  // Lam = max(W * H, flr)
            const int nz = s64_gemm_plan(&gLam[i], W, 1, F, H, 1, r, a.Lam + oFT, 1, F, F, Ti, r, true, zb, stop);
            add_tiles(tLam, atLam, i, gLam[i], nz);
            split_entry(uLam, pLam, zb, nz, a.Lam + oFT, 1, F, F, Ti, true, stop);
        }
        if (upd_h) {  // W' * R, W' * D
            const int nz = s64_gemm_plan(&gNum[i], W, F, 1, Rm + oFT, 1, F, a.Num + oRT, 1, r, r, Ti, F, false, zb, stop);
            add_tiles(tH, atH, i, gNum[i], nz);
            split_entry(uNum, pNum, zb, nz, a.Num + oRT, 1, r, r, Ti, false, stop);
            if (!kl_i) {
                s64_gemm_plan(&gDen[i], W, F, 1, Dm + oFT, 1, F, a.Den + oRT, 1, r, r, Ti, F, false, zb, stop);
                add_tiles(tHd, atHd, i, gDen[i], nz);
                split_entry(uDen, pDen, zb, nz, a.Den + oRT, 1, r, r, Ti, false, stop);
            }
        }
        if (upd_w) {  // R * H', D * H'
            const int nz = s64_gemm_plan(&gQ[i], Rm + oFT, 1, F, H, r, 1, a.Q + oFR, 1, F, F, r, Ti, false, zb, stop);
            add_tiles(tW, atW, i, gQ[i], nz);
            split_entry(uQ, pQ, zb, nz, a.Q + oFR, 1, F, F, r, false, stop);
            if (!kl_i) {
                s64_gemm_plan(&gP[i], Dm + oFT, 1, F, H, r, 1, a.P + oFR, 1, F, F, r, Ti, false, zb, stop);
                add_tiles(tWd, atWd, i, gP[i], nz);
                split_entry(uP, pP, zb, nz, a.P + oFR, 1, F, F, r, false, stop);
            } else {  // the row sums of H: k_s64_sumz(dsp, n_rowz, r, r, dhs, 1, 0, 0) of the single solve
                uRow.push_back(B64Sum{a.sp + q.sp0, a.hs + q.w0, (long long)r, 1, 0, q.n_rowz, r, 0, stop});
            }
        }
    }
    if ((long long)atLam != fLam.n || (long long)atH != fH.n || (long long)atW != fW.n || (long long)atHd != fHd.n || (long long)atWd != fWd.n)
        return fail(SNMF_ERR_INTERNAL, "fp64 batch: a tile table does not have the size it was measured at");
    hipStream_t st = ctx->stream;
    int rc = SNMF_OK;
    auto up = [&](void* dst, const void* src, size_t bytes) {
        if (rc == SNMF_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
            rc = fail(SNMF_ERR_NO_DEVICE, "hipMemcpyAsync (fp64 batch tables) failed");
    };
    auto up_product = [&](Product& pr, const std::vector<Gemm64Args>& g, const std::vector<B64Sum>& u) {
        if (!pr.args) return;
        up(pr.args, g.data(), sizeof(Gemm64Args) * g.size());
        pr.n_sums = (int)u.size();
        up(pr.sums, u.data(), sizeof(B64Sum) * u.size());
    };
    up(dprob, prob.data(), sizeof(B64Prob) * (size_t)n_problems);
    up(dwi, w_ind.data(), (size_t)p.r);
    up(fLam.tiles, tLam.data(), sizeof(B64Tile) * tLam.size());
    if (fH.tiles) up(fH.tiles, tH.data(), sizeof(B64Tile) * tH.size());
    if (fW.tiles) up(fW.tiles, tW.data(), sizeof(B64Tile) * tW.size());
    if (fHd.tiles) up(fHd.tiles, tHd.data(), sizeof(B64Tile) * tHd.size());
    if (fWd.tiles) up(fWd.tiles, tWd.data(), sizeof(B64Tile) * tWd.size());
    up_product(pLam, gLam, uLam);
    up_product(pNum, gNum, uNum);
    up_product(pDen, gDen, uDen);
    up_product(pQ, gQ, uQ);
    up_product(pP, gP, uP);
    n_row = (int)uRow.size();
    if (sRow) up(sRow, uRow.data(), sizeof(B64Sum) * uRow.size());
    if (rc == SNMF_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(SNMF_ERR_NO_DEVICE, "hipStreamSynchronize failed");
    if (rc != SNMF_OK) return rc;
    SN_TRY(reset());
    // launches of one iteration with the objective
    {
        auto prod = [](const Product& pr) { return pr.args ? 1 + (pr.n_sums ? 1 : 0) : 0; };
        int n = 0;
        const int lam = prod(pLam), ratio = n_modes - (has[S64_ED] ? 1 : 0), upd = (any_kl ? 1 : 0) + (any_nonkl ? 1 : 0);
        if (upd_h) n += ratio + prod(pNum) + (any_kl ? 1 : 0) + (kl ? 0 : prod(pDen)) + upd + lam;
        if (upd_w) n += ratio + prod(pQ) + (any_kl ? 2 : 0) + (kl ? 0 : prod(pP)) + upd + lam;
        if (p.cost_check) n += n_modes + 1;
        else if (masked) n += 1;  // the re-imputation runs objective or not (src/snmf_mdi.m:251-254)
        launches = n;
    }
    return SNMF_OK;
}

int Batch64::upload_sparsity(const double* sparsity) {
    HIP_TRY(hipMemcpyAsync(S, sparsity, sizeof(double) * (size_t)a.r, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the caller's array may go)
    return SNMF_OK;
}

template <typename TT>
int Batch64::load_t(int k, const TT* V, int64_t ldV, const TT* W0, const TT* H0, const TT* M, int64_t ldM) {
    const B64Prob& q = prob[k];
    const int F = a.F, r = q.r, T = q.T;
    const long long nFT = (long long)F * T;
    double *dV = a.V + q.fr0 * F, *dH = a.H + q.h0, *dW = a.W + q.w0 * F, *dwn = a.wn + q.w0;
    hipStream_t st = ctx->stream;
    // (tight on the device; fp32 arrays are widened on the way in)
    if (!V && masked) return fail(SNMF_ERR_UNSUPPORTED, "a missing-data batch takes its V from the host");
    if (V) SN_TRY((xfer_pack_in<TT, double>(ctx, V, ldV, F, T, dV, F, T, false)));
    if (masked) SN_TRY((xfer_pack_in<TT, double>(ctx, M, ldM, F, T, Mblk + q.fr0 * F, F, T, false)));
    if (H0) SN_TRY((xfer_pack_in<TT, double>(ctx, H0, r, r, T, dH, r, T, false)));
    // the initial scaling (:157-169) with the single solve's own kernels, on this problem's arrays
    if (W0) {
        SN_TRY((xfer_pack_in<TT, double>(ctx, W0, F, F, r, dW, F, r, false)));
        hipLaunchKernelGGL((k_s64_wupd<true, false>), dim3(r), dim3(256), 0, st, dW, nullptr, nullptr, nullptr, nullptr, F, dwn, &a.st[k].stop);
        HIP_TRY(hipGetLastError());
    }
    if (H0) SN_TRY(scale_h0(k));
    if (masked) {  // src/snmf_mdi.m:175, the masked start (it floors: floor_v has no meaning here)
        hipLaunchKernelGGL(k_s64_mdi_start, dim3(grid64(nFT)), dim3(256), 0, st, dV, (const double*)(Mblk + q.fr0 * F), nFT);
        HIP_TRY(hipGetLastError());
    } else if (p.floor_v && V) {  // (a V written on the device is floored by v_written)
        hipLaunchKernelGGL(k_s64_floor, dim3(grid64(nFT)), dim3(256), 0, st, dV, nFT);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

int Batch64::scale_h0(int k) {  // :159-160, with the single solve's own kernel
    const B64Prob& q = prob[k];
    const long long nRT = (long long)q.r * q.T;
    hipLaunchKernelGGL(k_s64_hscale, dim3(grid64(nRT)), dim3(256), 0, ctx->stream, a.H + q.h0, a.wn + q.w0, q.r, nRT);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int elem_grid(const Batch64* s, long long rows);

// One launch with the problem as a grid index copies the rows (a stopped problem's H is its stop iterate: nothing writes it
// after the test has fired); then the scaling load() does, problem by problem.
int Batch64::take_h0(snmf_batch& src_, int row0) {
    const Batch64* src = dynamic_cast<const Batch64*>(&src_);
    if (!src || src == this) return fail(SNMF_ERR_INTERNAL, "take_h0: the source is not another fp64 batch engine");
    if (!ranks.empty() || !src->ranks.empty())
        return fail(SNMF_ERR_UNSUPPORTED, "take_h0: a batch with a rank per problem hands no activations over (the DNMF batches share their ranks)");
    if (!src->ran || src->ctx != ctx) return fail(SNMF_ERR_STATE, "take_h0: the source batch has not run on this context");
    if (row0 < 0 || row0 + a.r > src->a.r) return fail(SNMF_ERR_DIM, "take_h0: rows [%d, %d) of an H of %d rows", row0, row0 + a.r, src->a.r);
    if (src->B != B) return fail(SNMF_ERR_DIM, "take_h0: %d problems from a batch of %d", B, src->B);
    for (int k = 0; k < B; ++k)  // (equal frame counts give equal frame offsets)
        if (src->prob[k].T != prob[k].T) return fail(SNMF_ERR_DIM, "take_h0: problem %d has %d frames, its source %d", k, prob[k].T, src->prob[k].T);
    hipLaunchKernelGGL(k_b64_take_h, dim3(elem_grid(this, a.r), B), dim3(256), 0, ctx->stream, a, (const double*)src->a.H, src->a.r, row0);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < B; ++k) SN_TRY(scale_h0(k));
    return SNMF_OK;
}

// take_h0 for any two fp64 batches, with or without ranks and settings: problem k takes rows [row0[k], row0[k] + r_k) of its
// source's H, both at their own prefix offsets.  One launch reads both tables of problems and the row offsets from the device.
int Batch64::take_h0_rows(snmf_batch& src_, const int32_t* row0) {
    const Batch64* src = dynamic_cast<const Batch64*>(&src_);
    if (!src || src == this) return fail(SNMF_ERR_INTERNAL, "take_h0_rows: the source is not another fp64 batch engine");
    if (!row0) return fail(SNMF_ERR_INVALID, "take_h0_rows: NULL argument");
    if (!src->ran || src->ctx != ctx) return fail(SNMF_ERR_STATE, "take_h0_rows: the source batch has not run on this context");
    if (src->B != B) return fail(SNMF_ERR_DIM, "take_h0_rows: %d problems from a batch of %d", B, src->B);
    for (int k = 0; k < B; ++k) {
        if (src->prob[k].T != prob[k].T)
            return fail(SNMF_ERR_DIM, "take_h0_rows: problem %d has %d frames, its source %d", k, prob[k].T, src->prob[k].T);
        if (row0[k] < 0 || (long long)row0[k] + prob[k].r > src->prob[k].r)
            return fail(SNMF_ERR_DIM, "take_h0_rows: problem %d: rows [%d, %lld) of an H of %d rows", k, row0[k], (long long)row0[k] + prob[k].r,
                        src->prob[k].r);
    }
    struct Tmp {  // (a table of this call alone: the device block is carved once, when the batch is made)
        void* q = nullptr;
        ~Tmp() {
            if (q) hipFree(q);
        }
    } tmp;
    const size_t bytes = sizeof(int32_t) * (size_t)B;
    {
        hipError_t e = hipMalloc(&tmp.q, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            tmp.q = nullptr;
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
    }
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(tmp.q, row0, bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_b64_take_h_rows, dim3(elem_grid(this, a.r), B), dim3(256), 0, st, a, (const B64Prob*)src->dprob, (const double*)src->a.H,
                       (const int32_t*)tmp.q);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < B; ++k) SN_TRY(scale_h0(k));
    HIP_TRY(hipStreamSynchronize(st));  // (the table is freed on return, and the caller's array may go)
    return SNMF_OK;
}

// One launch with the problem as a grid index gathers the columns into each problem's W; then the scaling load() does after its
// W0 upload, problem by problem.
int Batch64::take_w0(const int64_t* idx, bool unit_columns) {
    if (!idx) return fail(SNMF_ERR_INVALID, "take_w0: NULL argument");
    if (masked) return fail(SNMF_ERR_UNSUPPORTED, "a missing-data batch takes its W0 from the host");
    struct Tmp {  // (a table of this call alone: the device block is carved once, when the batch is made)
        void* q = nullptr;
        ~Tmp() {
            if (q) hipFree(q);
        }
    } tmp;
    const size_t bytes = sizeof(int64_t) * (size_t)sumR;
    {
        hipError_t e = hipMalloc(&tmp.q, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            tmp.q = nullptr;
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
    }
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(tmp.q, idx, bytes, hipMemcpyHostToDevice, st));
    const int g = (int)std::min<long long>(((long long)a.F * a.r + 255) / 256, kElemGridMax);
    hipLaunchKernelGGL(k_b64_take_w, dim3(g, B), dim3(256), 0, st, a, (const int64_t*)tmp.q);
    HIP_TRY(hipGetLastError());
    if (unit_columns)
        for (int k = 0; k < B; ++k) {  // :157-158
            hipLaunchKernelGGL((k_s64_wupd<true, false>), dim3(prob[k].r), dim3(256), 0, st, a.W + prob[k].w0 * a.F, nullptr, nullptr, nullptr,
                               nullptr, a.F, a.wn + prob[k].w0, &a.st[k].stop);
            HIP_TRY(hipGetLastError());
        }
    HIP_TRY(hipStreamSynchronize(st));  // (the table is freed on return, and the caller's array may go)
    return SNMF_OK;
}

// The layout is tight: problem k's F x T_k matrix at its frame offset, nothing around it to prepare.
int Batch64::v_blocks(std::vector<VBlock>* out) {
    if (masked) return fail(SNMF_ERR_UNSUPPORTED, "a missing-data batch takes its V from the host");
    out->resize(B);
    for (int k = 0; k < B; ++k) (*out)[k] = VBlock{a.V + prob[k].fr0 * a.F, (int64_t)a.F};
    return SNMF_OK;
}

int Batch64::v_written() {  // the floor load() applies (:169): element-wise, so one launch over the block of every problem
    if (!p.floor_v) return SNMF_OK;
    const long long n = (long long)a.F * sumT;
    hipLaunchKernelGGL(k_s64_floor, dim3(grid64(n)), dim3(256), 0, ctx->stream, a.V, n);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int Batch64::draw_h0(const uint64_t* seed, const uint8_t* draw) {
    if (!seed || !draw) return fail(SNMF_ERR_INVALID, "draw_h0: NULL argument");
    struct Tmp {  // (a table of this call alone: the device block is carved once, when the batch is made)
        void* q = nullptr;
        ~Tmp() {
            if (q) hipFree(q);
        }
    } tmp;
    const size_t nB = (size_t)B;
    {
        hipError_t e = hipMalloc(&tmp.q, nB * 9);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            tmp.q = nullptr;
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", nB * 9, hipGetErrorString(e));
        }
    }
    uint64_t* d_seed = (uint64_t*)tmp.q;
    uint8_t* d_draw = (uint8_t*)tmp.q + nB * 8;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(d_seed, seed, 8 * nB, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_draw, draw, nB, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_b64_rand_h, dim3(elem_grid(this, (a.r + 3) / 4), B), dim3(256), 0, st, a, (const uint64_t*)d_seed, (const uint8_t*)d_draw);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < B; ++k)
        if (draw[k]) SN_TRY(scale_h0(k));
    HIP_TRY(hipStreamSynchronize(st));  // (the table is freed on return)
    return SNMF_OK;
}

int product(Batch64* s, const Family& f, const Product& pr) {
    hipStream_t st = s->ctx->stream;
    hipLaunchKernelGGL(k_b64_gemm, dim3((unsigned)f.n), dim3(256), 0, st, (const Gemm64Args*)pr.args, (const B64Tile*)f.tiles);
    HIP_TRY(hipGetLastError());
    if (pr.n_sums) {
        hipLaunchKernelGGL(k_b64_sumz, dim3(grid64(pr.sum_n_max), pr.n_sums), dim3(256), 0, st, (const B64Sum*)pr.sums);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

template <typename K>
int grouped(Batch64* s, K kern, dim3 grid) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s->ctx->stream, s->a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int elem_grid(const Batch64* s, long long rows) {
    return (int)std::max<long long>(1, std::min<long long>((rows * s->maxT + 255) / 256, kElemGridMax));
}

// (the passes compiled per mode: one launch per mode present, whose workgroups return at once on a problem of another mode)
int ratio(Batch64* s) {
    const dim3 g(elem_grid(s, s->a.F), s->B);
    if (s->has[S64_KL]) SN_TRY(grouped(s, k_b64_ratio<S64_KL>, g));
    if (s->has[S64_IS]) SN_TRY(grouped(s, k_b64_ratio<S64_IS>, g));
    if (s->has[S64_GEN]) SN_TRY(grouped(s, k_b64_ratio<S64_GEN>, g));
    return SNMF_OK;  // Euclidean: R = V, D = Lam
}

int objective(Batch64* s) {
    const dim3 g(kS64Blocks, s->B);
    if (s->has[S64_KL]) SN_TRY(grouped(s, k_b64_obj<S64_KL>, g));
    if (s->has[S64_ED]) SN_TRY(grouped(s, k_b64_obj<S64_ED>, g));
    if (s->has[S64_IS]) SN_TRY(grouped(s, k_b64_obj<S64_IS>, g));
    if (s->has[S64_GEN]) SN_TRY(grouped(s, k_b64_obj<S64_GEN>, g));
    return SNMF_OK;
}

// the re-imputation and the objective of the imputed v in one pass, in the place of objective() on a masked batch
int mdi_objective(Batch64* s) {
    const dim3 g(kS64Blocks, s->B);
    if (s->has[S64_KL]) SN_TRY(grouped(s, k_b64_mdi_obj<S64_KL>, g));
    if (s->has[S64_ED]) SN_TRY(grouped(s, k_b64_mdi_obj<S64_ED>, g));
    if (s->has[S64_IS]) SN_TRY(grouped(s, k_b64_mdi_obj<S64_IS>, g));
    if (s->has[S64_GEN]) SN_TRY(grouped(s, k_b64_mdi_obj<S64_GEN>, g));
    return SNMF_OK;
}

// One iteration, the launches of solve64_run grouped over the problems.
int Batch64::iterate(int it) {
    hipStream_t st = ctx->stream;
    const int r = a.r;
    auto lam = [&]() { return product(this, fLam, pLam); };  // lambda = max(w * h, flr)
    if (it == 1) {                                           // of the scaled initial factors
        SN_TRY(lam());
        lam_done = true;
    }
    const dim3 g_rt(elem_grid(this, r), B), g_col(r, B);
    if (upd_h) {  // :189-208
        SN_TRY(ratio(this));
        SN_TRY(product(this, fH, pNum));
        if (any_nonkl) SN_TRY(product(this, fHd, pDen));
        if (any_kl) {
            SN_TRY(grouped(this, k_b64_colsum, g_col));
            SN_TRY(grouped(this, k_b64_hupd<true>, g_rt));
        }
        if (any_nonkl) SN_TRY(grouped(this, k_b64_hupd<false>, g_rt));
        SN_TRY(lam());
    }
    if (upd_w) {  // :212-244
        SN_TRY(ratio(this));
        SN_TRY(product(this, fW, pQ));
        if (any_nonkl) SN_TRY(product(this, fWd, pP));
        if (any_kl) {
            SN_TRY(grouped(this, k_b64_rowsum, dim3((r + 255) / 256, max_rowz, B)));
            hipLaunchKernelGGL(k_b64_sumz, dim3(grid64(r), n_row), dim3(256), 0, st, (const B64Sum*)sRow);
            HIP_TRY(hipGetLastError());
            SN_TRY(grouped(this, k_b64_wupd<true>, g_col));
        }
        if (any_nonkl) SN_TRY(grouped(this, k_b64_wupd<false>, g_col));
        SN_TRY(lam());
    }
    if (masked && !p.cost_check)  // src/snmf_mdi.m:251-254: v is re-imputed in every iteration, objective or not
        SN_TRY(grouped(this, k_b64_mdi_impute, dim3(elem_grid(this, a.F), B)));
    if (p.cost_check) {  // :248-284
        SN_TRY(masked ? mdi_objective(this) : objective(this));
        hipLaunchKernelGGL(k_b64_stop, dim3(B), dim3(256), 0, st, a, it);
        HIP_TRY(hipGetLastError());
    } else if (!limit_at.empty() && it < p.max_iter && limit_at[it]) {  // settings per problem: the limits below the largest
        hipLaunchKernelGGL(k_b64_limit, dim3((B + 255) / 256), dim3(256), 0, st, a, B, it);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

template <typename TT>
int Batch64::fetch_t(int k, TT* W, TT* H) {
    // (fp32 arrays receive the fp64 results rounded to nearest)
    const B64Prob& q = prob[k];
    if (W) SN_TRY((xfer_unpack_out<TT, double>(ctx, a.W + q.w0 * a.F, a.F, a.F, q.r, W, a.F)));
    if (H) SN_TRY((xfer_unpack_out<TT, double>(ctx, a.H + q.h0, q.r, q.r, q.T, H, q.r)));
    return SNMF_OK;
}

// src/snmf_mdi.m:296-306 for problem k with the single solve's own kernel, into the scratch block: V, Lam and the mask of the
// problem are read only, so a later run continues as if nothing had been read.
int Batch64::fetch_v_mdi(int k, double* V_mdi, int64_t ld) {
    const B64Prob& q = prob[k];
    const int F = a.F, T = q.T;
    const long long o = q.fr0 * F, groups = ((long long)T + 3) / 4;  // a wave per frame
    if (!lam_done) {  // max_iter = 0: no iteration ran, and the single solve imputes from Lam of the scaled initial factors
        SN_TRY(product(this, fLam, pLam));
        lam_done = true;
    }
    hipLaunchKernelGGL(k_s64_mdi_final, dim3((unsigned)std::min<long long>(groups, 65536)), dim3(256), 0, ctx->stream,
                       (const double*)(a.V + o), (const double*)(Mblk + o), (const double*)(a.Lam + o), F, (long long)T, Vm);
    HIP_TRY(hipGetLastError());
    return xfer_unpack_out<double, double>(ctx, Vm, F, F, T, V_mdi, ld);
}

void Batch64::describe(char* buf, size_t buflen) const {
    const char* mn = n_modes > 1 ? "mixed" : (has[S64_KL] ? "kl" : (has[S64_ED] ? "ed" : (has[S64_IS] ? "is" : "beta")));
    const int ge = elem_grid(this, a.F), gh = elem_grid(this, a.r);
    int n = snprintf(buf, buflen,
             "batch fp64 B=%d F=%d r=%d %s upd_h=%d upd_w=%d frames=%lld | k_b64_gemm tables (problem, 64x64 tile, split of %d): "
             "lam=%lld h=%lld w=%lld x256 | k_b64_sumz entries lam=%d h=%d w=%d rows=%d | k_b64_ratio grid=(%d,%d) k_b64_hupd grid=(%d,%d) "
             "k_b64_colsum/k_b64_wupd grid=(%d,%d) k_b64_rowsum grid=(%d,%d,%d) %s grid=(%d,%d) k_b64_stop grid=%d | "
             "launches_per_iter=%d bytes=%zu poll_every=%d",
             B, a.F, a.r, mn, (int)upd_h, (int)upd_w, sumT, kS64ChunkK, fLam.n, fH.n, fW.n, pLam.n_sums, pNum.n_sums, pQ.n_sums,
             n_row, ge, B, gh, B, a.r, B, (a.r + 255) / 256, max_rowz, B, masked ? "k_b64_mdi_obj" : "k_b64_obj", kS64Blocks, B, B, launches, bytes, kPollEvery);
    if (!ranks.empty() && n > 0 && (size_t)n < buflen)  // (r above is the largest)
        n += snprintf(buf + n, buflen - (size_t)n, " | ranks: min=%d max=%d sum=%lld h_elems=%lld", min_r, a.r, sumR, sumRT);
    if (!settings.empty() && n > 0 && (size_t)n < buflen)
        n += snprintf(buf + n, buflen - (size_t)n, " | settings: modes=%d max_iter min=%d max=%d h_den_tiles=%lld w_den_tiles=%lld", n_modes, min_mi,
                      p.max_iter, fHd.n, fWd.n);
    if (masked && n > 0 && (size_t)n < buflen)  // (bytes above counts both blocks)
        snprintf(buf + n, buflen - (size_t)n, " | mdi: k_b64_mdi_impute grid=(%d,%d) mask_bytes=%zu v_mdi_scratch_bytes=%zu", ge, B,
                 mask_bytes, sizeof(double) * (size_t)a.F * (size_t)maxT);
}

}  // namespace

snmf_batch* batch64_new(bool masked) {
    Batch64* b = new Batch64();
    b->masked = masked;
    return b;
}
