// snmf_tu_online_f64.hip -- the fp64 mode of the single-stream online separator (snmf_online_create_f64 /
// snmf_online_process_f64), kernels in snmf_online_f64.h.  A translation unit of its own, so that the single-stream fp32
// kernels' code does not move.  The snmf_online handle lives in snmf_tu_online.hip; it holds an OnlineF64 and forwards.
#include "snmf_internal.h"
#include "snmf_online_f64.h"
#include "snmf_online_f64_host.h"
#include "snmf_online_classes.h"

namespace {
constexpr size_t kTraceCap64 = 1u << 16;  // the newest 65536 frames, as snmf_online_trace
constexpr int64_t kChunk64 = 4096;        // frames per device batch
constexpr double kFlr64 = 1e-9;           // src/sparse_nmf.m:166, as a double (the engine's kFlr is its fp32 rounding)
}

struct OnlineF64 {
    snmf_ctx* ctx = nullptr;
    snmf_online_params p{};
    int F = 0, r = 0, N = 0, nov = 0, Ra = 1, ma = 1, Pl = 1;
    // state, all fp64
    double *B = nullptr, *Bfix = nullptr, *Btmp = nullptr;                    // [B_DFT_x | B_DFT_d], the original B_DFT_d, scratch
    double *Wn = nullptr, *WnT = nullptr, *wn = nullptr, *csum = nullptr;     // images of the frame solve (k_wnorm64)
    double *H0 = nullptr, *lambda_dav = nullptr, *Xm_tilde = nullptr, *r_blk = nullptr, *ldblk = nullptr, *adblk = nullptr;
    double *Vad = nullptr, *Had = nullptr, *win_s = nullptr, *win_i = nullptr, *tail = nullptr, *tail_x = nullptr, *tail_d = nullptr;
    double2* tw = nullptr;
    uint8_t *rup = nullptr, *w_ind = nullptr;
    OnlineDev* dev = nullptr;
    OnlineStatus* h_status = nullptr;  // pinned
    // cooperative adaptation solve (k_wadapt64)
    int wa_nwg = 0;
    size_t wa_lds = 0;
    double *wa_W = nullptr, *wa_p1 = nullptr, *wa_p2 = nullptr;
    int* wa_nit = nullptr;
    unsigned* wa_bar = nullptr;
    // per-call buffers (grown on demand)
    int cap_frames = 0;
    double *sig = nullptr, *Ym = nullptr, *Xt = nullptr, *Xh = nullptr, *Dh = nullptr, *syn = nullptr, *outf = nullptr, *A = nullptr,
           *recon = nullptr;
    double2* Yph = nullptr;
    int16_t* out16 = nullptr;
    int* nit = nullptr;
    OnlineStatus* status = nullptr;
    // per-class outputs (online_f64_set_classes): n_ev event classes then n_cls - n_ev noise classes; n_cls = 0: none set
    int n_ev = 0, n_cls = 0;
    int* cls = nullptr;          // [n_cls + 1] column ranges over [B_x | B_d] (snmf_online_classes.h)
    double* tail_c = nullptr;    // [n_cls][nov - 1 frames] one overlap-add tail per class
    double *Xc = nullptr, *syn_c = nullptr, *out_c = nullptr;  // per call, class-major: spectra, synthesis frames, hops
    // host state of the driver loop
    std::vector<double> pending, hist;
    int64_t l = 0;  // frames processed
    bool finished = false, failed = false;
    std::deque<snmf_online_frame> trace;
};

static void f64_free_call_buffers(OnlineF64* o) {
    void* ptrs[] = {o->sig, o->Ym, o->Xt, o->Xh, o->Dh, o->syn, o->outf, o->A, o->recon, o->Yph, o->out16, o->nit, o->status,
                    o->Xc, o->syn_c, o->out_c};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->Xc = o->syn_c = o->out_c = nullptr;
    o->sig = o->Ym = o->Xt = o->Xh = o->Dh = o->syn = o->outf = o->A = o->recon = nullptr;
    o->Yph = nullptr;
    o->out16 = nullptr;
    o->nit = nullptr;
    o->status = nullptr;
    o->cap_frames = 0;
}

void online_f64_destroy(OnlineF64* o) {
    if (!o) return;
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
    f64_free_call_buffers(o);
    void* ptrs[] = {o->B, o->Bfix, o->Btmp, o->Wn, o->WnT, o->wn, o->csum, o->H0, o->lambda_dav, o->Xm_tilde, o->r_blk, o->ldblk,
                    o->adblk, o->Vad, o->Had, o->win_s, o->win_i, o->tail, o->tail_x, o->tail_d, o->tw, o->rup, o->w_ind, o->dev,
                    o->wa_W, o->wa_p1, o->wa_p2, o->wa_nit, o->wa_bar, o->cls, o->tail_c};
    for (void* q : ptrs)
        if (q) hipFree(q);
    if (o->h_status) hipHostFree(o->h_status);
    delete o;
}

// the dictionary changed: wn, w ./ wn in both orientations, its column sums (src/sparse_nmf.m:157-159)
static int f64_refresh_images(OnlineF64* o) {
    hipLaunchKernelGGL(k_wnorm64, dim3(o->r), dim3(256), 0, o->ctx->stream, (const double*)o->B, o->F, o->r, o->Wn, o->WnT, o->wn, o->csum);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// `p` has passed snmf_tu_online.hip's validation
int online_f64_create(snmf_ctx* ctx, const snmf_online_params* p, const double* Bx, const double* Bd, const double* H0,
                      const double* Ad0, const double* win_stft, const double* win_istft, OnlineF64** out) {
    *out = nullptr;
    if (p->basis_update_N || p->basis_update_E)
        return fail(SNMF_ERR_UNSUPPORTED, "fp64 online separator: basis_update_N / basis_update_E (semi-supervised frame solve) is not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = p->fftlength, F = N / 2 + 1, r = p->R_x + p->R_d, sz = p->framelength, hop = p->frameshift;
    const int Ra = p->adapt_train_N ? p->R_a : 1, ma = p->adapt_train_N ? p->m_a : 1, Pl = p->blk_sparse ? p->P_len_l : 1;
    const size_t lds_fft = (size_t)2 * N * sizeof(double2), lds_solve = (size_t)(4 * F + 3 * r + 32) * 8, lds_post = (size_t)(r + 6 * F) * 8;
    if (lds_fft > ctx->lds_max || lds_solve > ctx->lds_max || lds_post > ctx->lds_max)
        return fail(SNMF_ERR_UNSUPPORTED, "fp64 online separator: fftlength %d with R_x + R_d = %d does not fit the LDS", N, r);
    int wa_nwg = 0;
    size_t wa_lds = 0;
    if (p->adapt_train_N) {
        int coop = 0;
        hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, ctx->device);
        wa_nwg = (F + kWa64RB - 1) / kWa64RB;
        wa_lds = wadapt64_lds_doubles(Ra, ma) * 8;
        if (!coop || Ra > kWa64RP || wa_nwg > ctx->n_cu || wa_nwg > 2 * kWaQ || wa_lds > ctx->lds_max)
            return fail(SNMF_ERR_UNSUPPORTED,
                        "fp64 online separator: the adaptation solve needs a cooperative launch of %d workgroups (<= %d), R_a = %d <= %d and "
                        "%zu bytes of LDS (<= %zu)", wa_nwg, std::min(ctx->n_cu, 2 * kWaQ), Ra, kWa64RP, wa_lds, ctx->lds_max);
    }
    OnlineF64* o = new OnlineF64();
    o->ctx = ctx;
    o->p = *p;
    o->F = F; o->r = r; o->N = N; o->Ra = Ra; o->ma = ma; o->Pl = Pl;
    o->nov = (sz + hop - 1) / hop;
    o->wa_nwg = wa_nwg;
    o->wa_lds = wa_lds;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * sz;
    int s = SNMF_OK;
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->B, (size_t)F * r); D(&o->Bfix, (size_t)F * p->R_d); D(&o->Btmp, (size_t)F * p->R_d);
    D(&o->Wn, (size_t)F * r); D(&o->WnT, (size_t)F * r); D(&o->wn, (size_t)r); D(&o->csum, (size_t)r); D(&o->H0, (size_t)r);
    D(&o->lambda_dav, (size_t)F); D(&o->Xm_tilde, (size_t)F); D(&o->r_blk, (size_t)F * Pl); D(&o->ldblk, (size_t)F * ma);
    D(&o->adblk, (size_t)Ra * ma); D(&o->Vad, (size_t)F * ma); D(&o->Had, (size_t)Ra * ma); D(&o->win_s, (size_t)sz);
    D(&o->win_i, (size_t)sz); D(&o->tail, ntail); D(&o->tw, (size_t)N / 2);
    if (p->class_outputs) {
        D(&o->tail_x, ntail);
        D(&o->tail_d, ntail);
    }
    D(&o->rup, (size_t)Ra); D(&o->w_ind, (size_t)Ra); D(&o->dev, (size_t)1);
    if (p->adapt_train_N) {
        D(&o->wa_W, (size_t)Ra * F);
        D(&o->wa_p1, (size_t)wa_nwg * (2 * kWa64RP + 1));
        D(&o->wa_p2, (size_t)wa_nwg * kWa64RP);
        D(&o->wa_nit, (size_t)1);
        D(&o->wa_bar, (size_t)1);
    }
    if (s == SNMF_OK && hipHostMalloc((void**)&o->h_status, sizeof(OnlineStatus)) != hipSuccess) s = fail(SNMF_ERR_NOMEM, "hipHostMalloc");
    if (s != SNMF_OK) {
        online_f64_destroy(o);
        return s;
    }
    std::vector<double2> htw(N / 2);
    for (int q = 0; q < N / 2; ++q) {
        const double ang = -2.0 * M_PI * (double)q / (double)N;
        htw[q] = make_double2(cos(ang), sin(ang));
    }
    OnlineDev d0{0, 1, 0, 0};  // update_switch = 1 (src/init_buff.m:42)
    hipMemcpyAsync(o->B, Bx, (size_t)F * p->R_x * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->B + (size_t)F * p->R_x, Bd, (size_t)F * p->R_d * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->Bfix, Bd, (size_t)F * p->R_d * 8, hipMemcpyHostToDevice, st);  // B_Mel_d in DFT mode (:328)
    hipMemcpyAsync(o->H0, H0, (size_t)r * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->win_s, win_stft, (size_t)sz * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->win_i, win_istft, (size_t)sz * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->tw, htw.data(), htw.size() * sizeof(double2), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->dev, &d0, sizeof d0, hipMemcpyHostToDevice, st);
    hipMemsetAsync(o->lambda_dav, 0, (size_t)F * 8, st);
    hipMemsetAsync(o->Xm_tilde, 0, (size_t)F * 8, st);
    hipMemsetAsync(o->r_blk, 0, (size_t)F * Pl * 8, st);
    hipMemsetAsync(o->ldblk, 0, (size_t)F * ma * 8, st);
    hipMemsetAsync(o->adblk, 0, (size_t)Ra * ma * 8, st);
    hipMemsetAsync(o->tail, 0, ntail * 8, st);
    if (p->class_outputs) {
        hipMemsetAsync(o->tail_x, 0, ntail * 8, st);
        hipMemsetAsync(o->tail_d, 0, ntail * 8, st);
    }
    hipMemsetAsync(o->rup, 0, (size_t)Ra, st);
    hipMemsetAsync(o->w_ind, 0, (size_t)Ra, st);
    if (p->adapt_train_N) hipMemcpyAsync(o->adblk, Ad0, (size_t)Ra * ma * 8, hipMemcpyHostToDevice, st);  // column-major R_a x m_a
    s = f64_refresh_images(o);
    hipError_t e = hipStreamSynchronize(st);
    if (s == SNMF_OK && e != hipSuccess) s = fail(SNMF_ERR_NO_DEVICE, "fp64 online create: %s", hipGetErrorString(e));
    if (s != SNMF_OK) {
        online_f64_destroy(o);
        return s;
    }
    o->hist.assign((size_t)(sz - hop), 0.0);
    *out = o;
    return SNMF_OK;
}

// snmf_online_set_classes on an fp64 separator (the handle's owner has checked class_outputs)
int online_f64_set_classes(OnlineF64* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num, const int32_t* noise_rank) {
    if (o->l != 0 || !o->pending.empty() || o->finished) return fail(SNMF_ERR_STATE, "snmf_online_set_classes must precede the first sample");
    std::vector<int> cls;
    SN_TRY(online_class_ranges(event_num, event_rank, noise_num, noise_rank, o->p.R_x, o->p.R_d, &cls));
    const int nc = event_num + noise_num;
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    f64_free_call_buffers(o);  // the class-major call buffers depend on the class count
    for (void** q : {(void**)&o->cls, (void**)&o->tail_c}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    o->n_ev = o->n_cls = 0;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * o->p.framelength;
    SN_TRY(dalloc(&o->cls, cls.size()));
    SN_TRY(dalloc(&o->tail_c, (size_t)nc * ntail));
    HIP_TRY(hipMemcpyAsync(o->cls, cls.data(), cls.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(o->tail_c, 0, (size_t)nc * ntail * 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    o->n_ev = event_num;
    o->n_cls = nc;
    return SNMF_OK;
}

void online_f64_class_counts(OnlineF64* o, int* n_event, int* n_noise) {
    *n_event = o->n_cls ? o->n_ev : 1;
    *n_noise = o->n_cls ? o->n_cls - o->n_ev : 1;
}

static int f64_reserve(OnlineF64* o, int n) {
    if (n <= o->cap_frames) return SNMF_OK;
    hipStreamSynchronize(o->ctx->stream);
    f64_free_call_buffers(o);
    const int cap = std::max(n, 64);
    const size_t F = o->F, sz = o->p.framelength, hop = o->p.frameshift;
    SN_TRY(dalloc(&o->sig, (sz - hop) + (size_t)cap * hop));
    SN_TRY(dalloc(&o->Ym, F * cap));
    SN_TRY(dalloc(&o->Yph, F * cap));
    SN_TRY(dalloc(&o->Xt, F * cap));
    if (o->p.class_outputs) {
        SN_TRY(dalloc(&o->Xh, F * cap));
        SN_TRY(dalloc(&o->Dh, F * cap));
    }
    SN_TRY(dalloc(&o->syn, (size_t)(cap + o->nov - 1) * sz));
    SN_TRY(dalloc(&o->outf, (size_t)cap * hop));
    SN_TRY(dalloc(&o->out16, (size_t)cap * hop));
    SN_TRY(dalloc(&o->A, (size_t)cap * o->r));
    SN_TRY(dalloc(&o->recon, (size_t)cap * 2 * F));
    SN_TRY(dalloc(&o->nit, (size_t)cap));
    SN_TRY(dalloc(&o->status, (size_t)cap));
    if (o->n_cls) {
        SN_TRY(dalloc(&o->Xc, (size_t)o->n_cls * F * cap));
        SN_TRY(dalloc(&o->syn_c, (size_t)o->n_cls * (cap + o->nov - 1) * sz));
        SN_TRY(dalloc(&o->out_c, (size_t)o->n_cls * cap * hop));
    }
    o->cap_frames = cap;
    return SNMF_OK;
}

// :296-336 once the status says the solve is due
static int f64_adapt(OnlineF64* o, int32_t* iters) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const int F = o->F;
    double* Bd = o->B + (size_t)F * p.R_x;
    const size_t n = (size_t)F * p.m_a + (size_t)p.R_a * p.m_a + p.R_a;
    hipLaunchKernelGGL(k_oprep64, dim3(grid_for(n)), dim3(256), 0, st, (const double*)o->ldblk, (const double*)o->adblk,
                       (const uint8_t*)o->rup, (const OnlineDev*)o->dev, F, p.R_a, p.m_a, o->Vad, o->Had, o->w_ind);
    HIP_TRY(hipGetLastError());
    WAdapt64Args wa{};
    wa.V = o->Vad; wa.H = o->Had; wa.W0 = Bd; wa.w_ind = o->w_ind; wa.Wout = o->wa_W; wa.part1 = o->wa_p1; wa.part2 = o->wa_p2;
    wa.n_iter_out = o->wa_nit; wa.bar = o->wa_bar; wa.F = F; wa.Ra = p.R_a; wa.ma = p.m_a; wa.max_iter = p.max_iter;
    wa.cost_check = p.cost_check; wa.beta = p.beta_div; wa.sparsity = p.sparsity; wa.flr = kFlr64; wa.conv_eps = p.conv_eps;
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_wadapt64, o->wa_lds));
    HIP_TRY(hipMemsetAsync(o->wa_bar, 0, 4, st));
    void* kargs[] = {&wa};
    hipError_t e = hipLaunchCooperativeKernel((const void*)k_wadapt64, dim3(o->wa_nwg), dim3(kWa64NT), kargs, (unsigned)o->wa_lds, st);
    if (e != hipSuccess) return fail(SNMF_ERR_NO_DEVICE, "fp64 adaptation solve: cooperative launch refused: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(iters, o->wa_nit, 4, hipMemcpyDeviceToHost, st));
    // the verdict is read BEFORE the solve's W is merged: a timed-out grid barrier leaves wa_W invalid
    HIP_TRY(hipStreamSynchronize(st));
    if (*iters < 0) return fail(SNMF_ERR_INTERNAL, "fp64 adaptation kernel: grid barrier timed out (dictionary left untouched)");
    hipLaunchKernelGGL(k_oassemble64, dim3(p.R_d), dim3(256), 0, st, (const double*)Bd, (const double*)o->wa_W, F, (const double*)o->Bfix,
                       (const uint8_t*)o->rup, F, p.R_a, p.R_d, o->Btmp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(Bd, o->Btmp, (size_t)F * p.R_d * 8, hipMemcpyDeviceToDevice, st));
    return f64_refresh_images(o);  // next frame's init_w (:140-146)
}

// n frames whose samples are sig = [history | n hops] (host); appends the hops the driver would write
static int f64_run_frames(OnlineF64* o, const std::vector<double>& sig, int n, std::vector<double>* outf, std::vector<int16_t>* out16,
                          std::vector<double>* xh, std::vector<double>* dh, std::vector<std::vector<double>>* xc) {
    const snmf_online_params& p = o->p;
    const int F = o->F, r = o->r, sz = p.framelength, hop = p.frameshift, nov = o->nov;
    hipStream_t st = o->ctx->stream;
    SN_TRY(f64_reserve(o, n));
    HIP_TRY(hipMemcpyAsync(o->sig, sig.data(), sig.size() * 8, hipMemcpyHostToDevice, st));
    const size_t lds_fft = (size_t)2 * o->N * sizeof(double2);
    OStftArgsT<double> sa{};
    sa.sig = o->sig; sa.sz = sz; sa.hop = hop; sa.dcbin = p.dcbin; sa.preemph = p.preemph; sa.win = o->win_s; sa.tw = o->tw;
    sa.powv = p.pow; sa.floorv = p.nonzerofloor; sa.Ym = o->Ym; sa.Yph = o->Yph; sa.ld = F; sa.n_frames = n;
    int s = SNMF_OK;
    by_logn([&](auto L) {
        s = ensure_dyn_lds(o->ctx->device, (const void*)k_ostft64<decltype(L)::value>, lds_fft);
        if (s == SNMF_OK) hipLaunchKernelGGL(k_ostft64<decltype(L)::value>, dim3(n), dim3(256), lds_fft, st, sa);
    }, o->N);
    SN_TRY(s);
    HIP_TRY(hipGetLastError());
    const size_t lds_solve = (size_t)(4 * F + 3 * r + 32) * 8, lds_post = (size_t)(r + 6 * F) * 8;
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_hsolve64, lds_solve));
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_opost64, lds_post));
    auto solve_args = [&](int i, int cnt) {
        HSolve64Args h{};
        h.Wn = o->Wn; h.WnT = o->WnT; h.wn = o->wn; h.csum = o->csum; h.H0 = o->H0; h.V = o->Ym + (size_t)i * F;
        h.A = o->A + (size_t)i * r; h.recon = o->recon + (size_t)i * 2 * F; h.n_iter = o->nit + i;
        h.F = F; h.r = r; h.Rx = p.R_x; h.max_iter = p.max_iter; h.cost_check = p.cost_check; h.n = cnt;
        h.beta = p.beta_div; h.sparsity = p.sparsity; h.conv_eps = p.conv_eps; h.flr = kFlr64;
        return h;
    };
    auto post_args = [&](int i, int64_t l, int cnt) {
        OPostArgsT<double> a{};
        a.A = o->A + (size_t)i * r; a.hst = o->nit + i; a.recon = o->recon + (size_t)i * 2 * F; a.Ym = o->Ym + (size_t)i * F;
        a.lambda_dav = o->lambda_dav; a.Xm_tilde = o->Xm_tilde; a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk;
        a.rup = o->rup; a.dev = o->dev; a.status = o->status + i;
        a.Xt_out = o->Xt + (size_t)i * F;
        a.Xh_out = o->Xh ? o->Xh + (size_t)i * F : nullptr;
        a.Dh_out = o->Dh ? o->Dh + (size_t)i * F : nullptr;
        a.F = F; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.Pk = p.P_len_k; a.dcbin = p.dcbin; a.gap = p.blk_gap;
        a.l = (int)std::min<int64_t>(l, 1 << 30);
        a.blk_sparse = p.blk_sparse; a.adapt = p.adapt_train_N; a.wiener = p.enhance_method == 0; a.init_N_len = p.init_N_len;
        a.switch_at = (int)std::floor(p.overlap_m_a * p.m_a);
        a.alpha_p = p.alpha_p; a.alpha_eta = p.alpha_eta; a.alpha_d = p.alpha_d; a.beta0 = p.beta; a.beta_max = p.beta_max; a.Ar_up = p.Ar_up;
        a.flr = p.nonzerofloor;
        a.n = cnt; a.a_stride = r; a.recon_len = F;
        return a;
    };
    auto record = [&](const OnlineStatus& hs) -> snmf_online_frame {
        snmf_online_frame tr{};
        tr.n_iter = hs.n_iter; tr.trig = hs.trig; tr.n_up = hs.n_up; tr.beta = hs.beta; tr.A_x_mag = hs.A_x_mag; tr.A_d_mag = hs.A_d_mag;
        tr.Q_control = hs.Q_control;
        return tr;
    };
    // the class spectra of `cnt` frames from frame i on (:158-202), behind their solves and before the adaptation (k_oclass64)
    auto class_spectra = [&](int i, int cnt) -> int {
        hipLaunchKernelGGL(k_oclass64, dim3((F + 255) / 256, cnt), dim3(256), 0, st, (const double*)o->B, (const double*)(o->A + (size_t)i * r), r,
                           (const int*)o->cls, o->n_cls, F, cnt, o->Xc + (size_t)i * F, (int64_t)o->cap_frames * F);
        HIP_TRY(hipGetLastError());
        return SNMF_OK;
    };
    auto push = [&](const snmf_online_frame& tr) {
        o->trace.push_back(tr);
        if (o->trace.size() > kTraceCap64) o->trace.pop_front();
    };
    if (!p.adapt_train_N) {
        // Fixed dictionary: the frame solves of the batch as one grid, then one k_opost64 launch walks the recurrences.
        hipLaunchKernelGGL(k_hsolve64, dim3(n), dim3(1024), lds_solve, st, solve_args(0, n));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_opost64, dim3(1), dim3(1024), lds_post, st, post_args(0, o->l + 1, n));
        HIP_TRY(hipGetLastError());
        if (o->n_cls) SN_TRY(class_spectra(0, n));
        std::vector<OnlineStatus> hst((size_t)n);
        HIP_TRY(hipMemcpyAsync(hst.data(), o->status, (size_t)n * sizeof(OnlineStatus), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (const OnlineStatus& hs : hst) push(record(hs));
    } else {
        for (int i = 0; i < n; ++i) {
            hipLaunchKernelGGL(k_hsolve64, dim3(1), dim3(1024), lds_solve, st, solve_args(i, 1));
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_opost64, dim3(1), dim3(1024), lds_post, st, post_args(i, o->l + 1 + i, 1));
            HIP_TRY(hipGetLastError());
            if (o->n_cls) SN_TRY(class_spectra(i, 1));
            HIP_TRY(hipMemcpyAsync(o->h_status, o->status + i, sizeof(OnlineStatus), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const OnlineStatus hs = *o->h_status;
            snmf_online_frame tr = record(hs);
            if (hs.do_solve && hs.n_up > 0) {
                int32_t it = 0;
                SN_TRY(f64_adapt(o, &it));
                tr.solved = 1;
                tr.adapt_iters = it;
            }
            push(tr);
        }
    }
    // inverse STFT of the n frames behind the nov-1 frames kept from the previous call, overlap-add
    const int l0 = (int)std::min<int64_t>(o->l + 1, 1 << 30);
    const int i_first = (int)std::max<int64_t>(0, (int64_t)p.delay + 1 - l0);
    const int n_out = std::max(0, n - i_first);
    auto synth = [&](const double* mag, std::vector<double>* of, std::vector<int16_t>* o16, double* tail) -> int {
        if (nov > 1) HIP_TRY(hipMemcpyAsync(o->syn, tail, (size_t)(nov - 1) * sz * 8, hipMemcpyDeviceToDevice, st));
        OIstftArgsT<double> ia{};
        ia.mag = mag; ia.ph = o->Yph; ia.ld = F; ia.n_frames = n; ia.sz = sz; ia.dcb = p.dcbin_back; ia.powv = p.pow;
        ia.scale = p.overlapscale / (double)o->N; ia.preemph = p.preemph; ia.win = o->win_i; ia.tw = o->tw;
        ia.syn = o->syn + (size_t)(nov - 1) * sz;
        int s2 = SNMF_OK;
        by_logn([&](auto L) {
            s2 = ensure_dyn_lds(o->ctx->device, (const void*)k_oistft64<decltype(L)::value>, lds_fft);
            if (s2 == SNMF_OK) hipLaunchKernelGGL(k_oistft64<decltype(L)::value>, dim3(n), dim3(256), lds_fft, st, ia);
        }, o->N);
        SN_TRY(s2);
        HIP_TRY(hipGetLastError());
        if (n_out > 0) {
            hipLaunchKernelGGL(k_oola64, dim3(grid_for((size_t)n_out * hop)), dim3(256), 0, st, (const double*)o->syn, n, l0, p.delay, sz, hop,
                               nov, i_first, n_out, o->outf, o16 ? o->out16 : nullptr);
            HIP_TRY(hipGetLastError());
            if (of) {
                const size_t at = of->size();
                of->resize(at + (size_t)n_out * hop);
                HIP_TRY(hipMemcpyAsync(of->data() + at, o->outf, (size_t)n_out * hop * 8, hipMemcpyDeviceToHost, st));
            }
            if (o16) {
                const size_t at = o16->size();
                o16->resize(at + (size_t)n_out * hop);
                HIP_TRY(hipMemcpyAsync(o16->data() + at, o->out16, (size_t)n_out * hop * 2, hipMemcpyDeviceToHost, st));
            }
        }
        if (nov > 1) HIP_TRY(hipMemcpyAsync(tail, o->syn + (size_t)n * sz, (size_t)(nov - 1) * sz * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SNMF_OK;
    };
    SN_TRY(synth(o->Xt, outf, out16, o->tail));
    if (p.class_outputs) {  // x_hat / d_hat of :350-361 (summed over the classes), same synthesis
        SN_TRY(synth(o->Xh, xh, nullptr, o->tail_x));
        SN_TRY(synth(o->Dh, dh, nullptr, o->tail_d));
    }
    if (o->n_cls) {
        // x_hat_i / d_hat_i (:356-361): the class-major stack, each class through the same inverse STFT and overlap-add on its
        // own tail; the launches are queued back to back and synchronised once
        const int nc = o->n_cls;
        const size_t ntl = (size_t)(nov - 1) * sz, syn_cs = (size_t)(o->cap_frames + nov - 1) * sz, out_cs = (size_t)o->cap_frames * hop;
        if (nov > 1) HIP_TRY(hipMemcpy2DAsync(o->syn_c, syn_cs * 8, o->tail_c, ntl * 8, ntl * 8, (size_t)nc, hipMemcpyDeviceToDevice, st));
        for (int c = 0; c < nc; ++c) {
            OIstftArgsT<double> ia{};
            ia.mag = o->Xc + (size_t)c * o->cap_frames * F; ia.ph = o->Yph; ia.ld = F; ia.n_frames = n; ia.sz = sz; ia.dcb = p.dcbin_back;
            ia.powv = p.pow; ia.scale = p.overlapscale / (double)o->N; ia.preemph = p.preemph; ia.win = o->win_i; ia.tw = o->tw;
            ia.syn = o->syn_c + (size_t)c * syn_cs + ntl;
            int s2 = SNMF_OK;
            by_logn([&](auto L) {
                s2 = ensure_dyn_lds(o->ctx->device, (const void*)k_oistft64<decltype(L)::value>, lds_fft);
                if (s2 == SNMF_OK) hipLaunchKernelGGL(k_oistft64<decltype(L)::value>, dim3(n), dim3(256), lds_fft, st, ia);
            }, o->N);
            SN_TRY(s2);
            HIP_TRY(hipGetLastError());
            if (n_out <= 0) continue;
            hipLaunchKernelGGL(k_oola64, dim3(grid_for((size_t)n_out * hop)), dim3(256), 0, st, (const double*)(o->syn_c + (size_t)c * syn_cs), n,
                               l0, p.delay, sz, hop, nov, i_first, n_out, o->out_c + (size_t)c * out_cs, (int16_t*)nullptr);
            HIP_TRY(hipGetLastError());
            if (xc) {
                std::vector<double>& v = (*xc)[c];
                const size_t at = v.size();
                v.resize(at + (size_t)n_out * hop);
                HIP_TRY(hipMemcpyAsync(v.data() + at, o->out_c + (size_t)c * out_cs, (size_t)n_out * hop * 8, hipMemcpyDeviceToHost, st));
            }
        }
        if (nov > 1)
            HIP_TRY(hipMemcpy2DAsync(o->tail_c, ntl * 8, o->syn_c + (size_t)n * sz, syn_cs * 8, ntl * 8, (size_t)nc, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    o->l += n;
    return SNMF_OK;
}

int online_f64_process(OnlineF64* o, const double* pcm, int64_t n, int flush, double* xt, int16_t* xt_i16, double* xh, double* dh,
                       double* xhi, double* dhi, int64_t cap, int64_t* n_out) {
    if (n_out) *n_out = 0;
    if (n < 0 || (n > 0 && !pcm)) return fail(SNMF_ERR_INVALID, "pcm is NULL");
    if (o->finished) return fail(SNMF_ERR_STATE, "the stream was flushed; create a new separator");
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a batch; the separator state is not reusable, create a new one");
    if ((xh || dh || xhi || dhi) && !o->p.class_outputs) return fail(SNMF_ERR_STATE, "class outputs were not requested at creation");
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    const int sz = o->p.framelength, hop = o->p.frameshift;
    o->pending.insert(o->pending.end(), pcm, pcm + n);
    const int64_t nfr = (int64_t)(o->pending.size() / (size_t)hop);
    const int64_t tail_frames = flush ? o->p.delay + 1 : 0;
    const int64_t max_out = (nfr + tail_frames) * hop;
    if ((xt || xt_i16 || xh || dh || xhi || dhi) && cap < max_out) {
        o->pending.resize(o->pending.size() - (size_t)n);
        return fail(SNMF_ERR_INVALID, "output capacity %lld < %lld samples", (long long)cap, (long long)max_out);
    }
    std::vector<double> of, ox, od;
    std::vector<int16_t> o16;
    // class signals: with a partition set they come from the class kernel; without one x_hat / d_hat are the one class per side
    const bool cls_set = o->n_cls > 0, want_c = cls_set && (xhi || dhi);
    std::vector<std::vector<double>> oc(want_c ? o->n_cls : 0);
    std::vector<double>* px = (xh || (xhi && !cls_set)) ? &ox : nullptr;
    std::vector<double>* pd = (dh || (dhi && !cls_set)) ? &od : nullptr;
    const int64_t chunk = cls_set ? std::max<int64_t>(64, kChunk64 / o->n_cls) : kChunk64;  // (class-major buffers grow with the classes)
    int64_t done = 0;
    while (done < nfr) {
        const int nb = (int)std::min(chunk, nfr - done);
        std::vector<double> sig(o->hist);
        sig.insert(sig.end(), o->pending.begin() + done * hop, o->pending.begin() + (done + nb) * hop);
        if (int rc = f64_run_frames(o, sig, nb, xt ? &of : nullptr, xt_i16 ? &o16 : nullptr, px, pd, want_c ? &oc : nullptr)) {
            o->failed = true;  // frames of this call were consumed and the device state advanced: never retry on it
            return rc;
        }
        o->hist.assign(sig.end() - (sz - hop), sig.end());
        done += nb;
    }
    o->pending.erase(o->pending.begin(), o->pending.begin() + nfr * hop);
    if (flush) {
        // a partial hop is dropped and delay+1 all-zero frames follow (src/NTF_sep_event_RT.m:69-76)
        std::vector<double> sig((size_t)(sz - hop) + (size_t)tail_frames * hop, 0.0);
        if (int rc = f64_run_frames(o, sig, (int)tail_frames, xt ? &of : nullptr, xt_i16 ? &o16 : nullptr, px, pd, want_c ? &oc : nullptr)) {
            o->failed = true;
            return rc;
        }
        o->pending.clear();
        o->finished = true;
    }
    if (xt) std::memcpy(xt, of.data(), of.size() * 8);
    if (xt_i16) std::memcpy(xt_i16, o16.data(), o16.size() * 2);
    if (xh) std::memcpy(xh, ox.data(), ox.size() * 8);
    if (dh) std::memcpy(dh, od.data(), od.size() * 8);
    size_t nc_out = 0;
    if (cls_set) {
        for (int c = 0; c < (int)oc.size(); ++c) {
            double* dst = c < o->n_ev ? (xhi ? xhi + (size_t)c * cap : nullptr) : (dhi ? dhi + (size_t)(c - o->n_ev) * cap : nullptr);
            if (dst) std::memcpy(dst, oc[c].data(), oc[c].size() * 8);
            nc_out = std::max(nc_out, oc[c].size());
        }
    } else {
        if (xhi) std::memcpy(xhi, ox.data(), ox.size() * 8);
        if (dhi) std::memcpy(dhi, od.data(), od.size() * 8);
    }
    if (n_out) *n_out = (int64_t)std::max(std::max(std::max(of.size(), o16.size()), std::max(ox.size(), od.size())), nc_out);
    return SNMF_OK;
}

int online_f64_get_basis(OnlineF64* o, double* Bd, int64_t ld) {
    if (ld < o->F) return fail(SNMF_ERR_INVALID, "ld < F");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    HIP_TRY(hipMemcpy2D(Bd, (size_t)ld * 8, o->B + (size_t)o->F * o->p.R_x, (size_t)o->F * 8, (size_t)o->F * 8, (size_t)o->p.R_d,
                        hipMemcpyDeviceToHost));
    return SNMF_OK;
}

int online_f64_trace(OnlineF64* o, snmf_online_frame* out, int64_t cap, int64_t* n) {
    if (n) *n = (int64_t)o->trace.size();
    if (out && cap > 0) std::copy_n(o->trace.begin(), (size_t)std::min<int64_t>(cap, (int64_t)o->trace.size()), out);
    return SNMF_OK;
}
