// snmf_tu_solve64.hip -- the fp64 solve mode, kernels in snmf_solve64.h: solve64_core runs one solve on device pointers
// with a workspace of the caller's, snmf_sparse_nmf_fp64 is allocation, upload and download around it; solve64_mdi_core and
// snmf_mdi_fp64 are the same two with a mask (the missing-data solve of src/snmf_mdi.m / src/snmf_mdi_Sm.m).  A translation
// unit of its own: the fp32 plan, its kernels and its geometry are not touched, and compile to the code they compiled to before.
#include "snmf_internal.h"
#include "snmf_solve64.h"
#include "snmf_solve64_core.h"
#include "snmf_host64.h"

namespace {

// every device block of one solve; freed on every way out (a failed allocation leaks nothing)
struct Blocks64 {
    std::vector<void*> ptrs;
    hipStream_t st = nullptr;
    ~Blocks64() {
        if (st) hipStreamSynchronize(st);
        for (void* q : ptrs) hipFree(q);
    }
    int get(double** p, size_t n) { return get_bytes((void**)p, std::max<size_t>(n, 1) * sizeof(double)); }
    int get_bytes(void** p, size_t bytes) {
        *p = nullptr;
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
        ptrs.push_back(*p);
        return SNMF_OK;
    }
};

struct Solve64 {
    hipStream_t st = nullptr;
    int* stop = nullptr;    // &state->stop
    double* zbuf = nullptr; // split partials, tight column-major M x N each
};

// C = A * B with the contraction cut into splits of kS64ChunkK; one split stores straight into C, several go through
// their partials and k_s64_sumz (chunk order).  s64_gemm_plan (snmf_solve64.h) chooses the operands and strides.
int gemm64(const Solve64& s, const double* A, long long rsA, long long csA, const double* B, long long rsB, long long csB, double* C,
           long long rsC, long long csC, int M, int N, int K, bool do_floor) {
    Gemm64Args g;
    const int nz = s64_gemm_plan(&g, A, rsA, csA, B, rsB, csB, C, rsC, csC, M, N, K, do_floor, s.zbuf, s.stop);
    const bool direct = nz == 1;
    const long long tiles = s64_gemm_tiles(g);
    if (tiles > 0x7fffffffLL || nz > 65535) return fail(SNMF_ERR_UNSUPPORTED, "fp64 solve: %lld tiles / %d splits exceed the launch grid", tiles, nz);
    hipLaunchKernelGGL(k_s64_gemm, dim3((unsigned)tiles, nz), dim3(256), 0, s.st, g);
    HIP_TRY(hipGetLastError());
    if (!direct) {
        const long long n = (long long)M * N;
        hipLaunchKernelGGL(k_s64_sumz, dim3(grid64(n)), dim3(256), 0, s.st, s.zbuf, nz, n, M, C, rsC, csC, do_floor ? 1 : 0, s.stop);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

template <int MODE>
int ratio64(const Solve64& s, const double* V, const double* Lam, double* R, double* D, long long n, double beta) {
    hipLaunchKernelGGL(k_s64_ratio<MODE>, dim3(grid64(n)), dim3(256), 0, s.st, V, Lam, R, D, n, beta, s.stop);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

template <int MODE>
int obj64(const Solve64& s, const double* V, const double* Lam, long long n_v, double beta, const double* H, int kind, double scalar,
          const double* S, int r, long long n_h, double* part) {
    hipLaunchKernelGGL(k_s64_obj<MODE>, dim3(kS64Blocks), dim3(256), 0, s.st, V, Lam, n_v, beta, H, kind, scalar, S, r, n_h, part, s.stop);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// the re-imputation of src/snmf_mdi.m:251-254 with the objective of :257-268 in the same pass
template <int MODE>
int mdi_obj64(const Solve64& s, double* V, const double* M, const double* Lam, long long n_v, double beta, const double* H, int kind,
              double scalar, const double* S, int r, long long n_h, double* part) {
    hipLaunchKernelGGL(k_s64_mdi_obj<MODE>, dim3(kS64Blocks), dim3(256), 0, s.st, V, M, Lam, n_v, beta, H, kind, scalar, S, r, n_h, part, s.stop);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// the host's reading of the update masks (src/sparse_nmf.m:142-148, :176-179) and of beta
struct Shape64 {
    bool upd_h = true, upd_w = true;
    int mode = S64_KL;
    std::vector<uint8_t> w_ind;
};

int shape64(const snmf_params* p, Shape64* s) {
    SN_TRY(validate_params(p));
    s->w_ind.resize(p->r);
    int n_h = 0, n_w = 0;
    SN_TRY(read_update_masks(p, &n_h, &n_w, s->w_ind.data()));
    s->upd_h = n_h > 0, s->upd_w = n_w > 0;
    const double beta = p->beta;
    s->mode = beta == 1.0 ? S64_KL : (beta == 2.0 ? S64_ED : (beta == 0.0 ? S64_IS : S64_GEN));
    return SNMF_OK;
}

// The workspace of one solve, carved out of one block in a fixed order (Carve64); the same walk measures it.
struct Work64 {
    double *Lam, *R = nullptr, *D = nullptr, *Num = nullptr, *Den = nullptr, *Q = nullptr, *P = nullptr;
    double *cs = nullptr, *hs = nullptr, *sp = nullptr, *wn, *part, *div, *cost, *z = nullptr;
    uint8_t* wi;
    Solve64State* state;
};

size_t carve64(const snmf_params* p, const Shape64& sh, void* base, Work64* w) {
    const int F = p->F, T = p->T, r = p->r;
    const size_t nFT = (size_t)F * T, nRT = (size_t)r * T, nFR = (size_t)F * r;
    const bool kl = sh.mode == S64_KL, ed = sh.mode == S64_ED;
    Carve64 c(base);
    w->Lam = c.get<double>(nFT);
    if (!ed) w->R = c.get<double>(nFT);
    if (!ed && !kl) w->D = c.get<double>(nFT);
    if (sh.upd_h) {
        w->Num = c.get<double>(nRT);
        if (!kl) w->Den = c.get<double>(nRT);
        else w->cs = c.get<double>(r);
    }
    if (sh.upd_w) {
        w->Q = c.get<double>(nFR);
        if (!kl) w->P = c.get<double>(nFR);
        else {
            w->hs = c.get<double>(r);
            w->sp = c.get<double>((size_t)((T + kS64RowChunk - 1) / kS64RowChunk) * r);
        }
    }
    size_t need = split_partials(F, T, r, kS64ChunkK);                         // Lam = W * H
    if (sh.upd_h) need = std::max(need, split_partials(r, T, F, kS64ChunkK));  // W' * R, W' * D
    if (sh.upd_w) need = std::max(need, split_partials(F, r, T, kS64ChunkK));  // R * H', D * H'
    if (need) w->z = c.get<double>(need);
    w->wn = c.get<double>(r);
    w->part = c.get<double>(2 * kS64Blocks);
    w->div = c.get<double>(std::max(p->max_iter, 1));
    w->cost = c.get<double>(std::max(p->max_iter, 1));
    w->wi = c.get<uint8_t>(r);
    w->state = c.get<Solve64State>(1);
    return c.off;
}

}  // namespace

int solve64_ws_bytes(const snmf_params* p, size_t* bytes) {
    Shape64 sh;
    SN_TRY(shape64(p, &sh));
    Work64 w;
    *bytes = carve64(p, sh, nullptr, &w);
    return SNMF_OK;
}

namespace {

// The one body of solve64_core (dM == nullptr: the launches of the plain solve, nothing else) and solve64_mdi_core.
int solve64_run(snmf_ctx* ctx, const snmf_params* p, double* dV, const double* dM, double* dW, double* dH, const double* dS, void* ws,
                size_t ws_bytes, double* dVm, double* div_out, double* cost_out, int32_t* n_iter_out) {
    Shape64 sh;
    SN_TRY(shape64(p, &sh));
    const int F = p->F, T = p->T, r = p->r, max_iter = p->max_iter, kind = p->sparsity_kind;
    const bool upd_h = sh.upd_h, upd_w = sh.upd_w;
    const double beta = p->beta;
    const int mode = sh.mode;
    const bool kl = mode == S64_KL, ed = mode == S64_ED;
    Work64 w;
    if (carve64(p, sh, ws, &w) > ws_bytes || !ws) return fail(SNMF_ERR_INTERNAL, "fp64 solve: workspace of %zu bytes is too small", ws_bytes);
    hipStream_t st = ctx->stream;
    const long long nFT = (long long)F * T, nRT = (long long)r * T;
    const int n_rowz = (T + kS64RowChunk - 1) / kS64RowChunk;
    double *dLam = w.Lam, *dR = w.R, *dD = w.D, *dNum = w.Num, *dDen = w.Den, *dQ = w.Q, *dP = w.P;
    double *dcs = w.cs, *dhs = w.hs, *dsp = w.sp, *dwn = w.wn, *dpart = w.part, *ddiv = w.div, *dcost = w.cost;
    uint8_t* dwi = w.wi;
    Solve64State* dst = w.state;

    HIP_TRY(hipMemcpyAsync(dwi, sh.w_ind.data(), (size_t)r, hipMemcpyHostToDevice, st));
    Solve64State h_state;
    h_state.stop = 0, h_state.n_iter = 0, h_state.last_cost = INFINITY;  // :168
    HIP_TRY(hipMemcpyAsync(dst, &h_state, sizeof(h_state), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ddiv, 0, (size_t)std::max(max_iter, 1) * 8, st));   // :171-173
    HIP_TRY(hipMemsetAsync(dcost, 0, (size_t)std::max(max_iter, 1) * 8, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the host sources are pageable: they may be reused from here on)

    Solve64 s;
    s.st = st, s.stop = &dst->stop, s.zbuf = w.z;
    const double scalar = p->sparsity_scalar;
    // ---- initial scaling (:157-169)
    hipLaunchKernelGGL((k_s64_wupd<true, false>), dim3(r), dim3(256), 0, st, dW, nullptr, nullptr, nullptr, nullptr, F, dwn, s.stop);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_s64_hscale, dim3(grid64(nRT)), dim3(256), 0, st, dH, dwn, r, nRT);
    HIP_TRY(hipGetLastError());
    if (dM) {  // src/snmf_mdi.m:175, the masked start (it floors: floor_v has no meaning here)
        hipLaunchKernelGGL(k_s64_mdi_start, dim3(grid64(nFT)), dim3(256), 0, st, dV, dM, nFT);
        HIP_TRY(hipGetLastError());
    } else if (p->floor_v) {
        hipLaunchKernelGGL(k_s64_floor, dim3(grid64(nFT)), dim3(256), 0, st, dV, nFT);
        HIP_TRY(hipGetLastError());
    }
    auto lam = [&]() { return gemm64(s, dW, 1, F, dH, 1, r, dLam, 1, F, F, T, r, true); };  // lambda = max(w * h, flr)
    auto ratio = [&]() -> int {
        switch (mode) {
            case S64_KL: return ratio64<S64_KL>(s, dV, dLam, dR, dD, nFT, beta);
            case S64_IS: return ratio64<S64_IS>(s, dV, dLam, dR, dD, nFT, beta);
            case S64_GEN: return ratio64<S64_GEN>(s, dV, dLam, dR, dD, nFT, beta);
            default: return SNMF_OK;  // Euclidean: R = V, D = Lam
        }
    };
    const double* Rm = ed ? dV : dR;
    const double* Dm = ed ? dLam : dD;
    SN_TRY(lam());

    const bool polling = p->cost_check && p->conv_eps > 0.0;
    const double div_scale = mode == S64_GEN ? beta * (beta - 1.0) : 1.0;
    for (int it = 1; it <= max_iter; ++it) {
        if (upd_h) {  // :189-208
            SN_TRY(ratio());
            SN_TRY(gemm64(s, dW, F, 1, Rm, 1, F, dNum, 1, r, r, T, F, false));  // W' * R
            if (!kl) SN_TRY(gemm64(s, dW, F, 1, Dm, 1, F, dDen, 1, r, r, T, F, false));  // W' * D
            else {
                hipLaunchKernelGGL(k_s64_colsum, dim3(r), dim3(256), 0, st, dW, F, dcs, s.stop);
                HIP_TRY(hipGetLastError());
            }
            if (kl) hipLaunchKernelGGL(k_s64_hupd<true>, dim3(grid64(nRT)), dim3(256), 0, st, dH, dNum, dDen, dcs, kind, scalar, dS, r, nRT, s.stop);
            else hipLaunchKernelGGL(k_s64_hupd<false>, dim3(grid64(nRT)), dim3(256), 0, st, dH, dNum, dDen, dcs, kind, scalar, dS, r, nRT, s.stop);
            HIP_TRY(hipGetLastError());
            SN_TRY(lam());
        }
        if (upd_w) {  // :212-244
            SN_TRY(ratio());
            SN_TRY(gemm64(s, Rm, 1, F, dH, r, 1, dQ, 1, F, F, r, T, false));  // R * H'
            if (!kl) SN_TRY(gemm64(s, Dm, 1, F, dH, r, 1, dP, 1, F, F, r, T, false));  // D * H'
            else {
                hipLaunchKernelGGL(k_s64_rowsum, dim3((r + 255) / 256, n_rowz), dim3(256), 0, st, dH, r, T, kS64RowChunk, dsp, s.stop);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_s64_sumz, dim3(grid64(r)), dim3(256), 0, st, dsp, n_rowz, (long long)r, r, dhs, 1LL, 0LL, 0, s.stop);
                HIP_TRY(hipGetLastError());
            }
            if (kl) hipLaunchKernelGGL((k_s64_wupd<true, true>), dim3(r), dim3(256), 0, st, dW, dQ, dP, dhs, dwi, F, dwn, s.stop);
            else hipLaunchKernelGGL((k_s64_wupd<false, true>), dim3(r), dim3(256), 0, st, dW, dQ, dP, dhs, dwi, F, dwn, s.stop);
            HIP_TRY(hipGetLastError());
            SN_TRY(lam());
        }
        if (dM && !p->cost_check) {  // src/snmf_mdi.m:251-254: v is re-imputed in every iteration, objective or not
            hipLaunchKernelGGL(k_s64_mdi_impute, dim3(grid64(nFT)), dim3(256), 0, st, dV, dM, dLam, nFT, s.stop);
            HIP_TRY(hipGetLastError());
        }
        if (p->cost_check) {  // :248-284
            if (dM) {
                switch (mode) {  // (the re-imputation and the objective of the imputed v in one pass)
                    case S64_KL: SN_TRY((mdi_obj64<S64_KL>(s, dV, dM, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                    case S64_ED: SN_TRY((mdi_obj64<S64_ED>(s, dV, dM, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                    case S64_IS: SN_TRY((mdi_obj64<S64_IS>(s, dV, dM, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                    default: SN_TRY((mdi_obj64<S64_GEN>(s, dV, dM, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                }
            } else {
                switch (mode) {
                    case S64_KL: SN_TRY((obj64<S64_KL>(s, dV, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                    case S64_ED: SN_TRY((obj64<S64_ED>(s, dV, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                    case S64_IS: SN_TRY((obj64<S64_IS>(s, dV, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                    default: SN_TRY((obj64<S64_GEN>(s, dV, dLam, nFT, beta, dH, kind, scalar, dS, r, nRT, dpart))); break;
                }
            }
            hipLaunchKernelGGL(k_s64_stop, dim3(1), dim3(256), 0, st, dpart, kS64Blocks, it, p->conv_eps, div_scale, ddiv, dcost, dst);
            HIP_TRY(hipGetLastError());
            if (polling && it % kPollEvery == 0 && it < max_iter) {  // the kernels past a stop are no-ops
                HIP_TRY(hipMemcpyAsync(&h_state, dst, sizeof(h_state), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (h_state.stop) break;
            }
        }
    }
    if (dM) {  // src/snmf_mdi.m:296-306: V and Lam are those of the last iteration that ran (the stop iteration after a stop)
        const long long groups = ((long long)T + 3) / 4;  // a wave per frame
        hipLaunchKernelGGL(k_s64_mdi_final, dim3((unsigned)std::min<long long>(groups, 65536)), dim3(256), 0, st, dV, dM, dLam, F, (long long)T, dVm);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(&h_state, dst, sizeof(h_state), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<double> hd(std::max(max_iter, 1)), hc(std::max(max_iter, 1));
    HIP_TRY(hipMemcpy(hd.data(), ddiv, hd.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hc.data(), dcost, hc.size() * 8, hipMemcpyDeviceToHost));
    if (div_out) std::copy(hd.begin(), hd.begin() + max_iter, div_out);
    if (cost_out) std::copy(hc.begin(), hc.begin() + max_iter, cost_out);
    if (n_iter_out) *n_iter_out = h_state.stop ? h_state.n_iter : max_iter;
    return SNMF_OK;
}

}  // namespace

int solve64_core(snmf_ctx* ctx, const snmf_params* p, double* dV, double* dW, double* dH, const double* dS, void* ws, size_t ws_bytes,
                 double* div_out, double* cost_out, int32_t* n_iter_out) {
    return solve64_run(ctx, p, dV, nullptr, dW, dH, dS, ws, ws_bytes, nullptr, div_out, cost_out, n_iter_out);
}

int solve64_mdi_core(snmf_ctx* ctx, const snmf_params* p, double* dV, const double* dM, double* dW, double* dH, const double* dS, void* ws,
                     size_t ws_bytes, double* dVm, double* div_out, double* cost_out, int32_t* n_iter_out) {
    if (!dM || !dVm) return fail(SNMF_ERR_INTERNAL, "fp64 missing-data solve: no mask or no output");
    return solve64_run(ctx, p, dV, dM, dW, dH, dS, ws, ws_bytes, dVm, div_out, cost_out, n_iter_out);
}

// the one-shot entry: allocation, upload and download around solve64_core
extern "C" int snmf_sparse_nmf_fp64(snmf_ctx* ctx, const snmf_params* p, const double* V, int64_t ldV, const double* W0,
                                    const double* H0, const double* sparsity, double* W, double* H, double* div_out,
                                    double* cost_out, int32_t* n_iter_out) {
    if (!ctx) return fail(SNMF_ERR_INVALID, "ctx is NULL");
    if (!V || !W || !H || !W0 || !H0) return fail(SNMF_ERR_INVALID, "V, W and H must be non-NULL");
    size_t ws_bytes = 0;
    SN_TRY(solve64_ws_bytes(p, &ws_bytes));
    const int F = p->F, T = p->T, r = p->r;
    if (ldV < F) return fail(SNMF_ERR_INVALID, "ldV = %lld < F = %d", (long long)ldV, F);
    const int kind = p->sparsity_kind;
    if (kind != SNMF_SPARSITY_SCALAR && !sparsity) return fail(SNMF_ERR_INVALID, "sparsity array required for this sparsity_kind");

    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Blocks64 mem;
    mem.st = st;
    const long long nFT = (long long)F * T, nRT = (long long)r * T, nFR = (long long)F * r;
    double *dV, *dW, *dH, *dS = nullptr;
    void* ws;
    SN_TRY(mem.get(&dV, nFT));
    SN_TRY(mem.get(&dW, nFR));
    SN_TRY(mem.get(&dH, nRT));
    const size_t n_s = kind == SNMF_SPARSITY_SCALAR ? 0 : (kind == SNMF_SPARSITY_RVEC ? (size_t)r : (size_t)nRT);
    if (n_s) SN_TRY(mem.get(&dS, n_s));
    SN_TRY(mem.get_bytes(&ws, ws_bytes));

    // upload (tight column-major on the device)
    if (ldV == F || T == 1) HIP_TRY(hipMemcpyAsync(dV, V, (size_t)nFT * 8, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpy2DAsync(dV, (size_t)F * 8, V, (size_t)ldV * 8, (size_t)F * 8, (size_t)T, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dW, W0, (size_t)nFR * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dH, H0, (size_t)nRT * 8, hipMemcpyHostToDevice, st));
    if (n_s) HIP_TRY(hipMemcpyAsync(dS, sparsity, n_s * 8, hipMemcpyHostToDevice, st));
    SN_TRY(solve64_core(ctx, p, dV, dW, dH, dS, ws, ws_bytes, div_out, cost_out, n_iter_out));
    HIP_TRY(hipMemcpyAsync(W, dW, (size_t)nFR * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(H, dH, (size_t)nRT * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

// the one-shot missing-data entry: allocation, upload and download around solve64_mdi_core
extern "C" int snmf_mdi_fp64(snmf_ctx* ctx, const snmf_params* p, const double* V, int64_t ldV, const double* M, int64_t ldM,
                             const double* W0, const double* H0, const double* sparsity, double* V_mdi, int64_t ldVm, double* W,
                             double* H, double* div_out, double* cost_out, int32_t* n_iter_out) {
    if (!ctx) return fail(SNMF_ERR_INVALID, "ctx is NULL");
    if (!V || !M || !W0 || !H0 || !V_mdi || !H) return fail(SNMF_ERR_INVALID, "V, M, W0, H0, V_mdi and H must be non-NULL");
    size_t ws_bytes = 0;
    SN_TRY(solve64_ws_bytes(p, &ws_bytes));
    const int F = p->F, T = p->T, r = p->r;
    if (ldV < F || ldM < F || ldVm < F)
        return fail(SNMF_ERR_INVALID, "ldV = %lld, ldM = %lld, ldVm = %lld: each must be at least F = %d", (long long)ldV, (long long)ldM, (long long)ldVm, F);
    const int kind = p->sparsity_kind;
    if (kind != SNMF_SPARSITY_SCALAR && !sparsity) return fail(SNMF_ERR_INVALID, "sparsity array required for this sparsity_kind");

    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Blocks64 mem;
    mem.st = st;
    const long long nFT = (long long)F * T, nRT = (long long)r * T, nFR = (long long)F * r;
    double *dV, *dM, *dW, *dH, *dS = nullptr;
    void* ws;
    SN_TRY(mem.get(&dV, nFT));
    SN_TRY(mem.get(&dM, nFT));
    SN_TRY(mem.get(&dW, nFR));
    SN_TRY(mem.get(&dH, nRT));
    const size_t n_s = kind == SNMF_SPARSITY_SCALAR ? 0 : (kind == SNMF_SPARSITY_RVEC ? (size_t)r : (size_t)nRT);
    if (n_s) SN_TRY(mem.get(&dS, n_s));
    SN_TRY(mem.get_bytes(&ws, ws_bytes));

    // upload (tight column-major on the device)
    auto up = [&](double* d, const double* h, int64_t ld) {
        if (ld == F || T == 1) return hipMemcpyAsync(d, h, (size_t)nFT * 8, hipMemcpyHostToDevice, st);
        return hipMemcpy2DAsync(d, (size_t)F * 8, h, (size_t)ld * 8, (size_t)F * 8, (size_t)T, hipMemcpyHostToDevice, st);
    };
    HIP_TRY(up(dV, V, ldV));
    HIP_TRY(up(dM, M, ldM));
    HIP_TRY(hipMemcpyAsync(dW, W0, (size_t)nFR * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dH, H0, (size_t)nRT * 8, hipMemcpyHostToDevice, st));
    if (n_s) HIP_TRY(hipMemcpyAsync(dS, sparsity, n_s * 8, hipMemcpyHostToDevice, st));
    // (v_MDI takes the place of the imputed v: the last kernel reads and writes each element in one lane)
    SN_TRY(solve64_mdi_core(ctx, p, dV, dM, dW, dH, dS, ws, ws_bytes, dV, div_out, cost_out, n_iter_out));
    if (ldVm == F || T == 1) HIP_TRY(hipMemcpyAsync(V_mdi, dV, (size_t)nFT * 8, hipMemcpyDeviceToHost, st));
    else HIP_TRY(hipMemcpy2DAsync(V_mdi, (size_t)ldVm * 8, dV, (size_t)F * 8, (size_t)F * 8, (size_t)T, hipMemcpyDeviceToHost, st));
    if (W) HIP_TRY(hipMemcpyAsync(W, dW, (size_t)nFR * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(H, dH, (size_t)nRT * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}
