// snmf_tu_batch64.hip -- the fp64 state of a batched offline solve (snmf_batch_create_fp64): host driver of the grouped
// kernels in snmf_batch64.h.  The loop is solve64_run's (snmf_tu_solve64.hip), launch for launch, with every launch grouped
// over the problems; the tables that map a workgroup to (problem, tile, split) and the per-problem GEMM arguments are built
// once, when the batch is made, from the frame counts and the addresses of the one device block.  A translation unit of its
// own: the fp32 batch, its kernels and its geometry are not touched.
#include "snmf_internal.h"
#include "snmf_batch64.h"
#include "snmf_batch64_host.h"

namespace {

constexpr int kPollEvery = 8;
constexpr int kElemGridMax = 2048;  // workgroups per problem of an element-wise pass (grid-stride beyond)
constexpr long long kGridXMax = 0x7fffffffLL;
constexpr int kGridYMax = 65535;

inline int grid64(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192)); }
inline int n_splits(int K) { return (K + kS64ChunkK - 1) / kS64ChunkK; }
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

// pieces of the one device block, 256-byte aligned, in a fixed order; base == nullptr only measures
struct Carve {
    char* base;
    size_t off = 0;
    explicit Carve(void* b) : base((char*)b) {}
    template <typename E>
    E* get(size_t n) {
        E* q = base ? (E*)(base + off) : nullptr;
        off += (std::max<size_t>(n, 1) * sizeof(E) + 255) & ~(size_t)255;
        return q;
    }
};

}  // namespace

struct Batch64 {
    snmf_ctx* ctx = nullptr;
    snmf_params p{};
    int B = 0, mode = S64_KL;
    bool upd_h = true, upd_w = true;
    std::vector<uint8_t> w_ind;
    std::vector<B64Prob> prob;
    std::vector<long long> z0;  // first double of each problem's split partials
    long long sumT = 0, sumRz = 0, sumZ = 0;
    int maxT = 0, max_rowz = 0;
    B64Args a{};
    double* S = nullptr;
    double* zbuf = nullptr;
    B64Prob* dprob = nullptr;
    uint8_t* dwi = nullptr;
    Family fLam, fH, fW;
    Product pLam, pNum, pDen, pQ, pP;
    B64Sum* sRow = nullptr;
    void* block = nullptr;
    size_t bytes = 0;
    int launches = 0;  // per iteration
    // state
    std::vector<uint8_t> have;
    int n_have = 0;
    bool have_s = false, ran = false;
    int it_done = 0;
    std::vector<Solve64State> h_st;
    std::vector<double> h_div, h_cost;
};

namespace {

// the walk over the device block (the same for measuring and for carving)
size_t carve(Batch64* s, void* base) {
    const snmf_params& p = s->p;
    const size_t F = p.F, r = p.r, nB = s->B, sT = (size_t)s->sumT;
    const bool kl = s->mode == S64_KL, ed = s->mode == S64_ED;
    B64Args& a = s->a;
    Carve c(base);
    a.V = c.get<double>(F * sT);
    a.Lam = c.get<double>(F * sT);
    a.R = ed ? nullptr : c.get<double>(F * sT);
    a.D = (ed || kl) ? nullptr : c.get<double>(F * sT);
    a.H = c.get<double>(r * sT);
    a.W = c.get<double>(nB * F * r);
    a.Num = a.Den = a.cs = a.Q = a.P = a.hs = a.sp = nullptr;
    if (s->upd_h) {
        a.Num = c.get<double>(r * sT);
        if (!kl) a.Den = c.get<double>(r * sT);
        else a.cs = c.get<double>(nB * r);
    }
    if (s->upd_w) {
        a.Q = c.get<double>(nB * F * r);
        if (!kl) a.P = c.get<double>(nB * F * r);
        else {
            a.hs = c.get<double>(nB * r);
            a.sp = c.get<double>((size_t)s->sumRz * r);
        }
    }
    s->zbuf = s->sumZ ? c.get<double>((size_t)s->sumZ) : nullptr;
    a.wn = c.get<double>(nB * r);
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
            s->pDen.args = c.get<Gemm64Args>(nB);
            s->pDen.sums = c.get<B64Sum>(nB);
        }
    }
    if (s->upd_w) {
        s->fW.tiles = c.get<B64Tile>((size_t)s->fW.n);
        s->pQ.args = c.get<Gemm64Args>(nB);
        s->pQ.sums = c.get<B64Sum>(nB);
        if (!kl) {
            s->pP.args = c.get<Gemm64Args>(nB);
            s->pP.sums = c.get<B64Sum>(nB);
        } else {
            s->sRow = c.get<B64Sum>(nB);
        }
    }
    a.S = s->S;
    a.w_ind = s->dwi;
    a.prob = s->dprob;
    return c.off;
}

int reset_state(Batch64* s) {
    std::fill(s->have.begin(), s->have.end(), 0);
    s->n_have = 0;
    s->ran = false;
    s->it_done = 0;
    hipStream_t st = s->ctx->stream;
    const size_t nB = (size_t)s->B;
    s->h_st.assign(nB, Solve64State{0, 0, INFINITY});  // src/sparse_nmf.m:168
    HIP_TRY(hipMemcpyAsync(s->a.st, s->h_st.data(), sizeof(Solve64State) * nB, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->a.n_stopped, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(s->a.divh, 0, sizeof(double) * nB * s->a.max_iter, st));  // :171-173
    HIP_TRY(hipMemsetAsync(s->a.costh, 0, sizeof(double) * nB * s->a.max_iter, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

}  // namespace

void batch64_destroy(Batch64* s) {
    if (!s) return;
    if (s->block) hipFree(s->block);
    delete s;
}

int batch64_create(snmf_ctx* ctx, const snmf_params* p_in, int32_t n_problems, const int32_t* T, Batch64** out) {
    *out = nullptr;
    if (n_problems < 1) return fail(SNMF_ERR_INVALID, "snmf_batch_create_fp64: n_problems must be at least 1 (got %d)", n_problems);
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
    for (int i = 0; i < n_problems; ++i)
        if (T[i] < 1) return fail(SNMF_ERR_INVALID, "problem %d has T = %d frames (at least 1)", i, T[i]);
    if (n_problems > kGridYMax)
        return fail(SNMF_ERR_UNSUPPORTED, "%d problems are above the fp64 batch's limit of %d (a launch grid's second dimension)", n_problems,
                    kGridYMax);

    Batch64* s = new Batch64();
    struct Guard {
        Batch64* s;
        ~Guard() { batch64_destroy(s); }
    } guard{s};
    s->ctx = ctx;
    s->p = p;
    s->p.w_update_ind = s->p.h_update_ind = nullptr;
    s->B = n_problems;
    s->upd_h = n_h > 0;
    s->upd_w = n_w > 0;
    s->mode = p.beta == 1.0 ? S64_KL : (p.beta == 2.0 ? S64_ED : (p.beta == 0.0 ? S64_IS : S64_GEN));
    s->w_ind.resize(r);
    for (int k = 0; k < r; ++k) s->w_ind[k] = p.w_update_ind ? p.w_update_ind[k] != 0 : 1;
    s->have.assign(n_problems, 0);
    const bool kl = s->mode == S64_KL, ed = s->mode == S64_ED;

    // ---- sizes, from the frame counts alone
    s->prob.resize(n_problems);
    s->z0.resize(n_problems);
    for (int i = 0; i < n_problems; ++i) {
        B64Prob& q = s->prob[i];
        q.T = T[i];
        q.n_rowz = (T[i] + kS64RowChunk - 1) / kS64RowChunk;
        q.fr0 = s->sumT;
        q.rz0 = s->sumRz;
        s->sumT += T[i];
        s->sumRz += q.n_rowz;
        s->maxT = std::max(s->maxT, T[i]);
        s->max_rowz = std::max(s->max_rowz, q.n_rowz);
        s->fLam.n += tiles_of(F, T[i]) * n_splits(r);
        if (s->upd_h) s->fH.n += tiles_of(r, T[i]) * n_splits(F);
        if (s->upd_w) s->fW.n += tiles_of(F, r) * n_splits(T[i]);
        // split partials: the largest nz * M * N over this problem's products that are split at all (carve64 of the single solve)
        long long need = 0;
        auto want = [&](long long M, long long N, int K) {
            const int nz = n_splits(K);
            if (nz > 1) need = std::max(need, (long long)nz * M * N);
        };
        want(F, T[i], r);
        if (s->upd_h) want(r, T[i], F);
        if (s->upd_w) want(F, r, T[i]);
        s->z0[i] = s->sumZ;
        s->sumZ += need;
    }
    // ---- grid limits, before anything is allocated
    const long long most = std::max(s->fLam.n, std::max(s->fH.n, s->fW.n));
    if (most > kGridXMax)
        return fail(SNMF_ERR_UNSUPPORTED, "%lld tiles in one grouped product are above the launch grid's limit of %lld", most, kGridXMax);
    if (s->max_rowz > kGridYMax)
        return fail(SNMF_ERR_UNSUPPORTED, "T = %d frames give %d row-sum chunks, above the launch grid's limit of %d", s->maxT, s->max_rowz,
                    kGridYMax);
    B64Args& a = s->a;
    a.F = F, a.r = r;
    a.kind = p.sparsity_kind;
    a.max_iter = std::max(1, p.max_iter);
    a.scalar = p.sparsity_scalar;
    a.beta = p.beta;
    a.conv_eps = p.conv_eps;
    a.div_scale = s->mode == S64_GEN ? p.beta * (p.beta - 1.0) : 1.0;
    s->bytes = carve(s, nullptr);

    // ---- the device
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    size_t mem_free = 0, mem_total = 0;
    HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
    if (s->bytes > mem_free)
        return fail(SNMF_ERR_UNSUPPORTED, "the fp64 batch needs %zu bytes of device memory, %zu of %zu are free", s->bytes, mem_free, mem_total);
    {
        hipError_t e = hipMalloc(&s->block, s->bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            s->block = nullptr;
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", s->bytes, hipGetErrorString(e));
        }
    }
    if (carve(s, s->block) != s->bytes) return fail(SNMF_ERR_INTERNAL, "fp64 batch: the two walks over the device block differ");

    // ---- tables: per problem the arguments gemm64() makes for it alone, then (split, tile) in the single launch's order
    const double* Rm = ed ? a.V : a.R;
    const double* Dm = ed ? a.Lam : a.D;
    std::vector<B64Tile> tLam((size_t)s->fLam.n), tH((size_t)s->fH.n), tW((size_t)s->fW.n);
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
    size_t atLam = 0, atH = 0, atW = 0;
    for (int i = 0; i < n_problems; ++i) {
        const B64Prob& q = s->prob[i];
        const int Ti = q.T;
        const long long oFT = q.fr0 * F, oRT = q.fr0 * r, oFR = (long long)i * F * r;
        double* zb = s->zbuf ? s->zbuf + s->z0[i] : nullptr;
        const int* stop = &a.st[i].stop;
        double *W = a.W + oFR, *H = a.H + oRT;
        {  // Lam = max(W * H, flr)
            const int nz = s64_gemm_plan(&gLam[i], W, 1, F, H, 1, r, a.Lam + oFT, 1, F, F, Ti, r, true, zb, stop);
            add_tiles(tLam, atLam, i, gLam[i], nz);
            split_entry(uLam, s->pLam, zb, nz, a.Lam + oFT, 1, F, F, Ti, true, stop);
        }
        if (s->upd_h) {  // W' * R, W' * D
            const int nz = s64_gemm_plan(&gNum[i], W, F, 1, Rm + oFT, 1, F, a.Num + oRT, 1, r, r, Ti, F, false, zb, stop);
            add_tiles(tH, atH, i, gNum[i], nz);
            split_entry(uNum, s->pNum, zb, nz, a.Num + oRT, 1, r, r, Ti, false, stop);
            if (!kl) {
                s64_gemm_plan(&gDen[i], W, F, 1, Dm + oFT, 1, F, a.Den + oRT, 1, r, r, Ti, F, false, zb, stop);
                split_entry(uDen, s->pDen, zb, nz, a.Den + oRT, 1, r, r, Ti, false, stop);
            }
        }
        if (s->upd_w) {  // R * H', D * H'
            const int nz = s64_gemm_plan(&gQ[i], Rm + oFT, 1, F, H, r, 1, a.Q + oFR, 1, F, F, r, Ti, false, zb, stop);
            add_tiles(tW, atW, i, gQ[i], nz);
            split_entry(uQ, s->pQ, zb, nz, a.Q + oFR, 1, F, F, r, false, stop);
            if (!kl) {
                s64_gemm_plan(&gP[i], Dm + oFT, 1, F, H, r, 1, a.P + oFR, 1, F, F, r, Ti, false, zb, stop);
                split_entry(uP, s->pP, zb, nz, a.P + oFR, 1, F, F, r, false, stop);
            } else {  // the row sums of H: k_s64_sumz(dsp, n_rowz, r, r, dhs, 1, 0, 0) of the single solve
                uRow.push_back(B64Sum{a.sp + q.rz0 * r, a.hs + (long long)i * r, (long long)r, 1, 0, q.n_rowz, r, 0, stop});
            }
        }
    }
    if ((long long)atLam != s->fLam.n || (long long)atH != s->fH.n || (long long)atW != s->fW.n)
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
    up(s->dprob, s->prob.data(), sizeof(B64Prob) * (size_t)n_problems);
    up(s->dwi, s->w_ind.data(), (size_t)r);
    up(s->fLam.tiles, tLam.data(), sizeof(B64Tile) * tLam.size());
    if (s->fH.tiles) up(s->fH.tiles, tH.data(), sizeof(B64Tile) * tH.size());
    if (s->fW.tiles) up(s->fW.tiles, tW.data(), sizeof(B64Tile) * tW.size());
    up_product(s->pLam, gLam, uLam);
    up_product(s->pNum, gNum, uNum);
    up_product(s->pDen, gDen, uDen);
    up_product(s->pQ, gQ, uQ);
    up_product(s->pP, gP, uP);
    if (s->sRow) up(s->sRow, uRow.data(), sizeof(B64Sum) * uRow.size());
    if (rc == SNMF_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(SNMF_ERR_NO_DEVICE, "hipStreamSynchronize failed");
    if (rc != SNMF_OK) return rc;
    SN_TRY(reset_state(s));
    s->have_s = p.sparsity_kind == SNMF_SPARSITY_SCALAR;
    // launches of one iteration with the objective
    {
        auto prod = [](const Product& pr) { return pr.args ? 1 + (pr.n_sums ? 1 : 0) : 0; };
        int n = 0;
        const int lam = prod(s->pLam), ratio = ed ? 0 : 1;
        if (s->upd_h) n += ratio + prod(s->pNum) + (kl ? 1 : prod(s->pDen)) + 1 + lam;
        if (s->upd_w) n += ratio + prod(s->pQ) + (kl ? 2 : prod(s->pP)) + 1 + lam;
        if (p.cost_check) n += 2;
        s->launches = n;
    }
    guard.s = nullptr;
    *out = s;
    return SNMF_OK;
}

int batch64_set_sparsity(Batch64* s, const double* sparsity) {
    if (!sparsity) return fail(SNMF_ERR_INVALID, "sparsity is NULL");
    if (s->p.sparsity_kind != SNMF_SPARSITY_RVEC) return fail(SNMF_ERR_STATE, "the batch was not created with SNMF_SPARSITY_RVEC");
    if (s->ran) return fail(SNMF_ERR_STATE, "snmf_batch_set_sparsity_f64 after snmf_batch_run");
    HIP_TRY(hipMemcpyAsync(s->S, sparsity, sizeof(double) * (size_t)s->a.r, hipMemcpyHostToDevice, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));  // (the caller's array may go)
    s->have_s = true;
    return SNMF_OK;
}

template <typename TT>
static int set_problem64(Batch64* s, int32_t k, const TT* V, int64_t ldV, const TT* W0, const TT* H0) {
    if (k < 0 || k >= s->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, s->B);
    if (!V || !W0 || !H0) return fail(SNMF_ERR_INVALID, "snmf_batch_set_problem: V, W0 or H0 of problem %d is NULL", k);
    const B64Args& a = s->a;
    if (ldV < a.F) return fail(SNMF_ERR_INVALID, "ldV = %lld is below F = %d", (long long)ldV, a.F);
    if (s->ran) SN_TRY(reset_state(s));  // a new batch on the same handle: every problem is set again
    const B64Prob& q = s->prob[k];
    const int F = a.F, r = a.r, T = q.T;
    const long long nFT = (long long)F * T, nRT = (long long)r * T;
    double *dV = a.V + q.fr0 * F, *dH = a.H + q.fr0 * r, *dW = a.W + (long long)k * F * r, *dwn = a.wn + (long long)k * r;
    hipStream_t st = s->ctx->stream;
    // (tight on the device; fp32 arrays are widened on the way in)
    SN_TRY((xfer_pack_in<TT, double>(s->ctx, V, ldV, F, T, dV, F, T, false)));
    SN_TRY((xfer_pack_in<TT, double>(s->ctx, H0, r, r, T, dH, r, T, false)));
    SN_TRY((xfer_pack_in<TT, double>(s->ctx, W0, F, F, r, dW, F, r, false)));
    // the initial scaling (:157-169) with the single solve's own kernels, on this problem's arrays
    hipLaunchKernelGGL((k_s64_wupd<true, false>), dim3(r), dim3(256), 0, st, dW, nullptr, nullptr, nullptr, nullptr, F, dwn, &a.st[k].stop);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_s64_hscale, dim3(grid64(nRT)), dim3(256), 0, st, dH, dwn, r, nRT);
    HIP_TRY(hipGetLastError());
    if (s->p.floor_v) {
        hipLaunchKernelGGL(k_s64_floor, dim3(grid64(nFT)), dim3(256), 0, st, dV, nFT);
        HIP_TRY(hipGetLastError());
    }
    if (!s->have[k]) {
        s->have[k] = 1;
        ++s->n_have;
    }
    return SNMF_OK;
}
int batch64_set_problem(Batch64* s, int32_t k, const double* V, int64_t ldV, const double* W0, const double* H0) {
    return set_problem64<double>(s, k, V, ldV, W0, H0);
}
int batch64_set_problem(Batch64* s, int32_t k, const float* V, int64_t ldV, const float* W0, const float* H0) {
    return set_problem64<float>(s, k, V, ldV, W0, H0);
}

namespace {

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

int ratio(Batch64* s) {
    const dim3 g(elem_grid(s, s->a.F), s->B);
    switch (s->mode) {
        case S64_KL: return grouped(s, k_b64_ratio<S64_KL>, g);
        case S64_IS: return grouped(s, k_b64_ratio<S64_IS>, g);
        case S64_GEN: return grouped(s, k_b64_ratio<S64_GEN>, g);
        default: return SNMF_OK;  // Euclidean: R = V, D = Lam
    }
}

int objective(Batch64* s) {
    const dim3 g(kS64Blocks, s->B);
    switch (s->mode) {
        case S64_KL: return grouped(s, k_b64_obj<S64_KL>, g);
        case S64_ED: return grouped(s, k_b64_obj<S64_ED>, g);
        case S64_IS: return grouped(s, k_b64_obj<S64_IS>, g);
        default: return grouped(s, k_b64_obj<S64_GEN>, g);
    }
}

}  // namespace

int batch64_run(Batch64* s, int32_t n_iters) {
    if (n_iters < 0) return fail(SNMF_ERR_INVALID, "n_iters must be >= 0 (0: up to max_iter)");
    if (s->n_have != s->B) return fail(SNMF_ERR_STATE, "snmf_batch_run: %d of %d problems are set", s->n_have, s->B);
    if (!s->have_s) return fail(SNMF_ERR_STATE, "snmf_batch_run: the sparsity vector is not set (snmf_batch_set_sparsity_f64)");
    hipStream_t st = s->ctx->stream;
    const B64Args& a = s->a;
    const int max_iter = s->p.max_iter, B = s->B, r = a.r;
    const int target = n_iters == 0 ? max_iter : (int)std::min<long long>(max_iter, (long long)s->it_done + n_iters);
    const bool cc = s->p.cost_check != 0, can_stop = cc && s->p.conv_eps > 0.0, kl = s->mode == S64_KL;
    auto lam = [&]() { return product(s, s->fLam, s->pLam); };  // lambda = max(w * h, flr)
    if (!s->ran) SN_TRY(lam());                                 // of the scaled initial factors
    s->ran = true;
    int stopped = 0;
    if (can_stop && s->it_done > 0) {
        HIP_TRY(hipMemcpyAsync(&stopped, a.n_stopped, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const dim3 g_rt(elem_grid(s, r), B), g_col(r, B);
    for (int it = s->it_done + 1; it <= target && stopped < B; ++it) {
        if (s->upd_h) {  // :189-208
            SN_TRY(ratio(s));
            SN_TRY(product(s, s->fH, s->pNum));
            if (!kl) SN_TRY(product(s, s->fH, s->pDen));
            else SN_TRY(grouped(s, k_b64_colsum, g_col));
            SN_TRY(kl ? grouped(s, k_b64_hupd<true>, g_rt) : grouped(s, k_b64_hupd<false>, g_rt));
            SN_TRY(lam());
        }
        if (s->upd_w) {  // :212-244
            SN_TRY(ratio(s));
            SN_TRY(product(s, s->fW, s->pQ));
            if (!kl) SN_TRY(product(s, s->fW, s->pP));
            else {
                SN_TRY(grouped(s, k_b64_rowsum, dim3((r + 255) / 256, s->max_rowz, B)));
                hipLaunchKernelGGL(k_b64_sumz, dim3(grid64(r), B), dim3(256), 0, st, (const B64Sum*)s->sRow);
                HIP_TRY(hipGetLastError());
            }
            SN_TRY(kl ? grouped(s, k_b64_wupd<true>, g_col) : grouped(s, k_b64_wupd<false>, g_col));
            SN_TRY(lam());
        }
        if (cc) {  // :248-284
            SN_TRY(objective(s));
            hipLaunchKernelGGL(k_b64_stop, dim3(B), dim3(256), 0, st, a, it);
            HIP_TRY(hipGetLastError());
        }
        s->it_done = it;
        if (can_stop && it % kPollEvery == 0 && it < max_iter) {  // the host looks every 8 iterations; a stopped problem's workgroups are no-ops
            HIP_TRY(hipMemcpyAsync(&stopped, a.n_stopped, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    const size_t nB = (size_t)B, nh = nB * a.max_iter;
    s->h_st.resize(nB);
    s->h_div.assign(nh, 0.0);
    s->h_cost.assign(nh, 0.0);
    HIP_TRY(hipMemcpyAsync(s->h_st.data(), a.st, sizeof(Solve64State) * nB, hipMemcpyDeviceToHost, st));
    if (cc) {
        HIP_TRY(hipMemcpyAsync(s->h_div.data(), a.divh, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(s->h_cost.data(), a.costh, sizeof(double) * nh, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

template <typename TT>
static int get_problem64(Batch64* s, int32_t k, TT* W, TT* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    if (k < 0 || k >= s->B) return fail(SNMF_ERR_INVALID, "problem index %d outside [0, %d)", k, s->B);
    if (!s->ran) return fail(SNMF_ERR_STATE, "snmf_batch_get before snmf_batch_run");
    const B64Args& a = s->a;
    const B64Prob& q = s->prob[k];
    const Solve64State& hs = s->h_st[k];
    // (fp32 arrays receive the fp64 results rounded to nearest)
    if (W) SN_TRY((xfer_unpack_out<TT, double>(s->ctx, a.W + (long long)k * a.F * a.r, a.F, a.F, a.r, W, a.F)));
    if (H) SN_TRY((xfer_unpack_out<TT, double>(s->ctx, a.H + q.fr0 * a.r, a.r, a.r, q.T, H, a.r)));
    const int mi = s->p.max_iter;
    for (int i = 0; i < mi; ++i) {
        if (div_out) div_out[i] = s->h_div[(size_t)k * a.max_iter + i];
        if (cost_out) cost_out[i] = s->h_cost[(size_t)k * a.max_iter + i];
    }
    if (n_iter_out) *n_iter_out = hs.stop ? hs.n_iter : s->it_done;
    return SNMF_OK;
}
int batch64_get(Batch64* s, int32_t k, double* W, double* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    return get_problem64<double>(s, k, W, H, div_out, cost_out, n_iter_out);
}
int batch64_get(Batch64* s, int32_t k, float* W, float* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    return get_problem64<float>(s, k, W, H, div_out, cost_out, n_iter_out);
}

int batch64_describe(const Batch64* s, char* buf, size_t buflen) {
    const B64Args& a = s->a;
    const char* mn = s->mode == S64_KL ? "kl" : (s->mode == S64_ED ? "ed" : (s->mode == S64_IS ? "is" : "beta"));
    const int ge = elem_grid(s, a.F), gh = elem_grid(s, a.r);
    snprintf(buf, buflen,
             "batch fp64 B=%d F=%d r=%d %s upd_h=%d upd_w=%d frames=%lld | k_b64_gemm tables (problem, 64x64 tile, split of %d): "
             "lam=%lld h=%lld w=%lld x256 | k_b64_sumz entries lam=%d h=%d w=%d rows=%d | k_b64_ratio grid=(%d,%d) k_b64_hupd grid=(%d,%d) "
             "k_b64_colsum/k_b64_wupd grid=(%d,%d) k_b64_rowsum grid=(%d,%d,%d) k_b64_obj grid=(%d,%d) k_b64_stop grid=%d | "
             "launches_per_iter=%d bytes=%zu poll_every=%d",
             s->B, a.F, a.r, mn, (int)s->upd_h, (int)s->upd_w, s->sumT, kS64ChunkK, s->fLam.n, s->fH.n, s->fW.n, s->pLam.n_sums,
             s->pNum.n_sums, s->pQ.n_sums, s->sRow ? s->B : 0, ge, s->B, gh, s->B, a.r, s->B, (a.r + 255) / 256, s->max_rowz, s->B,
             kS64Blocks, s->B, s->B, s->launches, s->bytes, kPollEvery);
    return SNMF_OK;
}
