// snmf_tu_online_f64.hip -- the fp64 mode of the single-stream online separator (snmf_online_create_f64 /
// snmf_online_process_f64), kernels in snmf_online_f64.h.  A translation unit of its own, so that the single-stream fp32
// kernels' code does not move.  The snmf_online handle lives in snmf_tu_online.hip; it holds an OnlineF64 and forwards.
// The host driver is snmf_online_host.h, shared with the fp32 mode.  What is left here: the handle's own members (the frame
// solve's images of the dictionary, the cooperative adaptation solve's buffers, the frame solves' call buffers), creation,
// and the mode's steps of the driver (om_*): the fp64 kernels' launches with their LDS sizes.
#include "snmf_internal.h"
#include "snmf_online_f64.h"
#include "snmf_online_f64_host.h"
#include "snmf_online_host.h"

namespace {
constexpr double kFlr64 = 1e-9;  // src/sparse_nmf.m:166, as a double (the engine's kFlr is its fp32 rounding)
}

struct OnlineF64 : OnlineState<double> {
    double *Wn = nullptr, *WnT = nullptr, *wn = nullptr, *csum = nullptr;  // images of the frame solve (k_wnorm64)
    uint8_t* w_ind = nullptr;
    // cooperative adaptation solve (k_wadapt64)
    int wa_nwg = 0;
    size_t wa_lds = 0;
    double *wa_W = nullptr, *wa_p1 = nullptr, *wa_p2 = nullptr;
    int* wa_nit = nullptr;
    unsigned* wa_bar = nullptr;
    // per-call buffers of the frame solves: activations, reconstructions, iteration counts, statuses
    double *A = nullptr, *recon = nullptr;
    int* nit = nullptr;
    OnlineStatus* status = nullptr;
};

static void om_free_call(OnlineF64* o) {
    void* ptrs[] = {o->A, o->recon, o->nit, o->status};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->A = o->recon = nullptr;
    o->nit = nullptr;
    o->status = nullptr;
}

static int om_reserve(OnlineF64* o, int cap) {
    SN_TRY(dalloc(&o->A, (size_t)cap * o->r));
    SN_TRY(dalloc(&o->recon, (size_t)cap * 2 * o->F));
    SN_TRY(dalloc(&o->nit, (size_t)cap));
    SN_TRY(dalloc(&o->status, (size_t)cap));
    return SNMF_OK;
}

void online_f64_destroy(OnlineF64* o) {
    if (!o) return;
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
    online_free_state(o);
    void* ptrs[] = {o->Wn, o->WnT, o->wn, o->csum, o->w_ind, o->wa_W, o->wa_p1, o->wa_p2, o->wa_nit, o->wa_bar};
    for (void* q : ptrs)
        if (q) hipFree(q);
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
    const int N = p->fftlength, F = N / 2 + 1, r = p->R_x + p->R_d;
    const int Ra = p->adapt_train_N ? p->R_a : 1, ma = p->adapt_train_N ? p->m_a : 1;
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
    int s = online_alloc_state(o, ctx, p);
    o->wa_nwg = wa_nwg;
    o->wa_lds = wa_lds;
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->Wn, (size_t)F * r); D(&o->WnT, (size_t)F * r); D(&o->wn, (size_t)r); D(&o->csum, (size_t)r); D(&o->w_ind, (size_t)Ra);
    if (p->adapt_train_N) {
        D(&o->wa_W, (size_t)Ra * F);
        D(&o->wa_p1, (size_t)wa_nwg * (2 * kWa64RP + 1));
        D(&o->wa_p2, (size_t)wa_nwg * kWa64RP);
        D(&o->wa_nit, (size_t)1);
        D(&o->wa_bar, (size_t)1);
    }
    if (s != SNMF_OK) {
        online_f64_destroy(o);
        return s;
    }
    std::vector<double2> htw;
    hipMemcpyAsync(o->B, Bx, (size_t)F * p->R_x * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->B + (size_t)F * p->R_x, Bd, (size_t)F * p->R_d * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->Bfix, Bd, (size_t)F * p->R_d * 8, hipMemcpyHostToDevice, st);  // B_Mel_d in DFT mode (:328)
    online_upload_state(o, H0, Ad0, win_stft, win_istft, htw);
    hipMemsetAsync(o->w_ind, 0, (size_t)Ra, st);
    s = f64_refresh_images(o);
    hipError_t e = hipStreamSynchronize(st);
    if (s == SNMF_OK && e != hipSuccess) s = fail(SNMF_ERR_NO_DEVICE, "fp64 online create: %s", hipGetErrorString(e));
    if (s != SNMF_OK) {
        online_f64_destroy(o);
        return s;
    }
    o->hist.assign((size_t)(p->framelength - p->frameshift), 0.0);
    *out = o;
    return SNMF_OK;
}

// snmf_online_set_classes on an fp64 separator (the handle's owner has checked class_outputs)
int online_f64_set_classes(OnlineF64* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num, const int32_t* noise_rank) {
    std::vector<int> cls;
    SN_TRY(online_class_table(o, event_num, event_rank, noise_num, noise_rank, &cls));
    return online_install_classes(o, cls, event_num, event_num + noise_num);
}

void online_f64_class_counts(OnlineF64* o, int* n_event, int* n_noise) {
    *n_event = o->n_cls ? o->n_ev : 1;
    *n_noise = o->n_cls ? o->n_cls - o->n_ev : 1;
}

// ---- the mode's steps of the shared driver (snmf_online_host.h) ------------------------------------------------------------
static size_t f64_lds_fft(const OnlineF64* o) { return (size_t)2 * o->N * sizeof(double2); }

static int om_stft(OnlineF64* o, int n) {
    const size_t lds_fft = f64_lds_fft(o);
    const OStftArgsT<double> sa = online_stft_args(o, n);
    int s = SNMF_OK;
    by_logn([&](auto L) {
        s = ensure_dyn_lds(o->ctx->device, (const void*)k_ostft64<decltype(L)::value>, lds_fft);
        if (s == SNMF_OK) hipLaunchKernelGGL(k_ostft64<decltype(L)::value>, dim3(n), dim3(256), lds_fft, o->ctx->stream, sa);
    }, o->N);
    SN_TRY(s);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// frame solve, post-filter and class spectra (:158-202, k_oclass64) of `cnt` frames from frame i of the run on: one launch
// each, the frame solves as one grid
static int f64_solve_post(OnlineF64* o, int i, int cnt, const OnlineStatus** st_out) {
    const snmf_online_params& p = o->p;
    const int F = o->F, r = o->r;
    hipStream_t st = o->ctx->stream;
    const size_t lds_solve = (size_t)(4 * F + 3 * r + 32) * 8, lds_post = (size_t)(r + 6 * F) * 8;
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_hsolve64, lds_solve));
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_opost64, lds_post));
    HSolve64Args h{};
    h.Wn = o->Wn; h.WnT = o->WnT; h.wn = o->wn; h.csum = o->csum; h.H0 = o->H0; h.V = o->Ym + (size_t)i * F;
    h.A = o->A + (size_t)i * r; h.recon = o->recon + (size_t)i * 2 * F; h.n_iter = o->nit + i;
    h.F = F; h.r = r; h.Rx = p.R_x; h.max_iter = p.max_iter; h.cost_check = p.cost_check; h.n = cnt;
    h.beta = p.beta_div; h.sparsity = p.sparsity; h.conv_eps = p.conv_eps; h.flr = kFlr64;
    hipLaunchKernelGGL(k_hsolve64, dim3(cnt), dim3(1024), lds_solve, st, h);
    HIP_TRY(hipGetLastError());
    OPostArgsT<double> a = online_post_args(o, i, o->l + 1 + i);
    a.A = o->A + (size_t)i * r; a.hst = o->nit + i; a.recon = o->recon + (size_t)i * 2 * F; a.status = o->status + i;
    a.n = cnt; a.a_stride = r; a.recon_len = F;
    hipLaunchKernelGGL(k_opost64, dim3(1), dim3(1024), lds_post, st, a);
    HIP_TRY(hipGetLastError());
    if (o->n_cls) {  // behind the solves and before the adaptation
        hipLaunchKernelGGL(k_oclass64, dim3((F + 255) / 256, cnt), dim3(256), 0, st, (const double*)o->B, (const double*)(o->A + (size_t)i * r), r,
                           (const int*)o->cls, o->n_cls, F, cnt, o->Xc + (size_t)i * F, (int64_t)o->cap_frames * F);
        HIP_TRY(hipGetLastError());
    }
    *st_out = o->status + i;
    return SNMF_OK;
}

static bool om_one_launch(const OnlineF64* o) { return !o->p.adapt_train_N; }
static int om_solve_run(OnlineF64* o, int n, const OnlineStatus** st) { return f64_solve_post(o, 0, n, st); }
static int om_solve_frame(OnlineF64* o, int i, const OnlineStatus** st) { return f64_solve_post(o, i, 1, st); }

// :296-336 once the status says the solve is due
static int om_adapt(OnlineF64* o, int32_t* iters) {
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

static int om_istft(OnlineF64* o, const double* mag, int n, double* syn) {
    const size_t lds_fft = f64_lds_fft(o);
    const OIstftArgsT<double> ia = online_istft_args(o, mag, n, syn);
    int s = SNMF_OK;
    by_logn([&](auto L) {
        s = ensure_dyn_lds(o->ctx->device, (const void*)k_oistft64<decltype(L)::value>, lds_fft);
        if (s == SNMF_OK) hipLaunchKernelGGL(k_oistft64<decltype(L)::value>, dim3(n), dim3(256), lds_fft, o->ctx->stream, ia);
    }, o->N);
    SN_TRY(s);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// each class through the same inverse STFT, behind its own tail
static int om_istft_class(OnlineF64* o, int c, int n, size_t syn_cs) {
    return om_istft(o, o->Xc + (size_t)c * o->cap_frames * o->F, n, o->syn_c + c * syn_cs + (size_t)(o->nov - 1) * o->p.framelength);
}

static int om_ola(OnlineF64* o, const double* syn, int n, int l0, int i_first, int n_out, double* out, int16_t* out16) {
    const snmf_online_params& p = o->p;
    hipLaunchKernelGGL(k_oola64, dim3(grid_for((size_t)n_out * p.frameshift)), dim3(256), 0, o->ctx->stream, syn, n, l0, p.delay, p.framelength,
                       p.frameshift, o->nov, i_first, n_out, out, out16);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// ---- the state record and the restart (the driver's last section; kernels k_ostate_get64 / k_ostate_put64) ---------------
static void om_state_mode(const OnlineF64*, int* mel, int* mel_conv, int* n1) { *mel = *mel_conv = *n1 = 0; }  // DFT mode only

static int om_state_launch(OnlineF64* o, const OStateArgs<double>& a, int64_t l, bool put) {
    if (put) hipLaunchKernelGGL(k_ostate_put64, dim3(1, kStN, kStParts), dim3(256), 0, o->ctx->stream, a);
    else hipLaunchKernelGGL(k_ostate_get64, dim3(1, kStN, kStParts), dim3(256), 0, o->ctx->stream, a, l);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static int om_refresh_dict(OnlineF64* o) { return f64_refresh_images(o); }

// ---- the entries snmf_tu_online.hip forwards to ----------------------------------------------------------------------------
int online_f64_process(OnlineF64* o, const double* pcm, int64_t n, int flush, double* xt, int16_t* xt_i16, double* xh, double* dh,
                       double* xhi, double* dhi, int64_t cap, int64_t* n_out) {
    return online_process(o, pcm, n, flush, xt, xt_i16, xh, dh, xhi, dhi, cap, n_out);
}

int online_f64_get_basis(OnlineF64* o, double* Bd, int64_t ld) { return online_get_basis_f64(o, Bd, ld); }

int online_f64_trace(OnlineF64* o, snmf_online_frame* out, int64_t cap, int64_t* n) { return online_trace_read(o, out, cap, n); }

void online_f64_state_info(OnlineF64* o, snmf_online_state_info* out) { online_state_info(o, out); }
int online_f64_get_state(OnlineF64* o, void* record, int64_t cap) { return online_get_state(o, record, cap); }
int online_f64_set_state(OnlineF64* o, const void* record, int64_t bytes) { return online_set_state(o, record, bytes); }

int online_f64_restart(OnlineF64* o, const double* Bd, const double* H0, const double* Ad) {
    SN_TRY(online_restart_check(o));
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    return online_restart(o, Bd, H0, Ad);
}
