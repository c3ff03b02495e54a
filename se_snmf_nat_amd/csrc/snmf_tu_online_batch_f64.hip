// snmf_tu_online_batch_f64.hip -- the fp64 mode of the batched online separator (snmf_online_batch_create_f64 /
// snmf_online_batch_process_f64), kernels in snmf_online_batch_f64.h.  A translation unit of its own, so that the fp32 batch
// kernels' and the single-stream fp64 kernels' code does not move.  The snmf_online_batch handle lives in
// snmf_tu_online_batch.hip; it holds an OnlineBatchF64 and forwards.
// The host driver (hop queues, chunk loop, framing, synthesis, trace) is snmf_online_batch_host.h, shared with the fp32 mode;
// here are the handle, its creation / restart, and the fp64 steps the driver calls (obm_*).
#include "snmf_internal.h"
#include "snmf_online_batch_f64.h"
#include "snmf_online_batch_f64_host.h"
#include "snmf_online_batch_host.h"
#include "snmf_online_classes.h"

namespace {
constexpr double kFlr64 = 1e-9;            // src/sparse_nmf.m:166, as a double
}

struct OnlineBatchF64 : OBatchState<double> {
    // per stream, device
    double *B = nullptr, *Bfix = nullptr, *Btmp = nullptr;                   // [B_DFT_x | B_DFT_d], the dictionary each stream started with, scratch
    double *Wn = nullptr, *WnT = nullptr, *wn = nullptr, *csum = nullptr;    // images of the frame solve (k_obrefresh64)
    double *H0 = nullptr, *Ad0 = nullptr, *lambda_dav = nullptr, *Xm_tilde = nullptr, *r_blk = nullptr, *ldblk = nullptr, *adblk = nullptr;
    double *Wu = nullptr, *Wm = nullptr, *Q = nullptr, *P = nullptr, *Vt = nullptr;  // k_wadapt_batch64's result and scratch
    double *win_s = nullptr, *win_i = nullptr, *Bxd = nullptr;  // shared
    double2* tw = nullptr;
    double *rs_B = nullptr, *rs_H = nullptr, *rs_A = nullptr;  // restart uploads (sized for all S streams)
    // per chunk, device (obm_reserve): the frame solves' activations, reconstructions and iteration counts
    double *A = nullptr, *reco = nullptr;
    int* nit = nullptr;
    OPostArgsT<double> post_a{};  // the post-filter's launch arguments of the current chunk (obm_begin_chunk)
};

static size_t b64_lds_fft(const OnlineBatchF64* o) { return (size_t)2 * o->N * sizeof(double2); }
static size_t b64_lds_solve(const OnlineBatchF64* o) { return (size_t)(4 * o->F + 3 * o->r + 32) * 8; }
static size_t b64_lds_post(const OnlineBatchF64* o) { return (size_t)(o->r + 6 * o->F) * 8; }

static void obm_free_chunk(OnlineBatchF64* o) {
    void* ptrs[] = {o->A, o->reco, o->nit};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->A = o->reco = nullptr;
    o->nit = nullptr;
}

static int obm_reserve(OnlineBatchF64* o, size_t slots) {
    SN_TRY(dalloc(&o->A, (size_t)o->r * slots));
    SN_TRY(dalloc(&o->reco, 2 * (size_t)o->F * slots));
    SN_TRY(dalloc(&o->nit, slots));
    return SNMF_OK;
}

// the slots count (frame, stream, class): the class-major buffers Xc / out_c grow with the classes
static int obm_chunk_frames(const OnlineBatchF64* o) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(4096, kBChunkSlots / ((int64_t)o->S * std::max(1, o->n_cls))));
}

void online_batch_f64_destroy(OnlineBatchF64* o) {
    if (!o) return;
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
    obatch_free_chunk(o);
    void* ptrs[] = {o->B, o->Bfix, o->Btmp, o->Wn, o->WnT, o->wn, o->csum, o->H0, o->Ad0, o->lambda_dav, o->Xm_tilde, o->r_blk, o->ldblk,
                    o->adblk, o->Wu, o->Wm, o->Q, o->P, o->Vt, o->tail, o->tail_x, o->tail_d, o->rup, o->dev, o->win_s, o->win_i, o->Bxd,
                    o->tw, o->rs_slots, o->rs_B, o->rs_H, o->rs_A, o->cls, o->tail_c, o->meta_i, o->meta_l};
    for (void* q : ptrs)
        if (q) hipFree(q);
    delete o;
}

// The streams slots[0..n) start a new recording (ob_restart of snmf_tu_online_batch.hip): the uploads, one k_obrestart64, one
// k_obrefresh64 over their columns, and their host state.  Ordered on ctx->stream, no synchronise.
static int b64_restart(OnlineBatchF64* o, int n, const int32_t* slots, const double* Bd, const double* H0, const double* Ad) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const size_t F = o->F, nA = (size_t)o->Ra * o->ma;
    HIP_TRY(hipMemcpyAsync(o->rs_slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (Bd) HIP_TRY(hipMemcpyAsync(o->rs_B, Bd, (size_t)n * p.R_d * F * 8, hipMemcpyHostToDevice, st));
    if (H0) HIP_TRY(hipMemcpyAsync(o->rs_H, H0, (size_t)n * o->r * 8, hipMemcpyHostToDevice, st));
    if (Ad) HIP_TRY(hipMemcpyAsync(o->rs_A, Ad, (size_t)n * nA * 8, hipMemcpyHostToDevice, st));
    ORestart64Args a{};
    a.slots = o->rs_slots; a.Bx = o->Bxd; a.Bd = Bd ? o->rs_B : nullptr; a.H0n = H0 ? o->rs_H : nullptr; a.Adn = Ad ? o->rs_A : nullptr;
    a.B = o->B; a.Bfix = o->Bfix; a.H0 = o->H0; a.Ad0 = o->Ad0; a.adblk = o->adblk; a.ldblk = o->ldblk; a.lambda_dav = o->lambda_dav;
    a.Xm_tilde = o->Xm_tilde; a.r_blk = o->r_blk; a.tail = o->tail; a.tail_x = o->tail_x; a.tail_d = o->tail_d; a.rup = o->rup;
    a.dev = o->dev; a.F = o->F; a.r = o->r; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl;
    a.adapt = p.adapt_train_N; a.ntail = (int64_t)o->ntail;
    hipLaunchKernelGGL(k_obrestart64, dim3(n, kRs64N, kRs64Parts), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < n && o->tail_c; ++i)  // the class tails of the stream, like tail_x / tail_d: one strided fill over its classes
        HIP_TRY(hipMemset2DAsync(o->tail_c + (size_t)slots[i] * o->ntail, (size_t)o->S * o->ntail * 8, 0, o->ntail * 8, (size_t)o->n_cls, st));
    ORefresh64Args ra{};
    ra.slots = o->rs_slots; ra.S = o->S; ra.B = o->B; ra.Wn = o->Wn; ra.WnT = o->WnT; ra.wn = o->wn; ra.csum = o->csum;
    ra.F = o->F; ra.r = o->r; ra.Rx = p.R_x; ra.k0 = 0;
    hipLaunchKernelGGL(k_obrefresh64, dim3(o->r, n), dim3(256), 0, st, ra);
    HIP_TRY(hipGetLastError());
    obatch_restart_host(o, n, slots);
    return SNMF_OK;
}

int online_batch_f64_create(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* Bx, const double* Bd0, const double* H0,
                            const double* Ad0, const double* win_stft, const double* win_istft, OnlineBatchF64** out) {
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = p->fftlength, F = N / 2 + 1, r = p->R_x + p->R_d, sz = p->framelength, hop = p->frameshift, Rd = p->R_d;
    OnlineBatchF64* o = new OnlineBatchF64();
    o->ctx = ctx;
    o->p = *p;
    o->S = S; o->F = F; o->r = r; o->N = N;
    o->nov = (sz + hop - 1) / hop;
    o->Ra = p->adapt_train_N ? p->R_a : 1;
    o->ma = p->adapt_train_N ? p->m_a : 1;
    o->Pl = p->blk_sparse ? p->P_len_l : 1;
    int s = SNMF_OK;
    if (b64_lds_fft(o) > ctx->lds_max || b64_lds_solve(o) > ctx->lds_max || b64_lds_post(o) > ctx->lds_max)
        s = fail(SNMF_ERR_UNSUPPORTED, "fp64 batched separator: fftlength %d with R_x + R_d = %d does not fit the LDS (%zu bytes)", N, r,
                 ctx->lds_max);
    if (s == SNMF_OK && p->adapt_train_N) {
        const size_t need = wbatch64_lds(o->Ra, o->ma, p->beta_div == 1.0);
        if (o->Ra > kWb64RP || o->ma > kWb64MaxMa || need > ctx->lds_max)
            s = fail(SNMF_ERR_UNSUPPORTED,
                     "fp64 batched adaptation: R_a = %d, m_a = %d is outside k_wadapt_batch64's envelope (R_a <= %d, m_a <= %d, %zu bytes of LDS "
                     "<= %zu)", o->Ra, o->ma, kWb64RP, kWb64MaxMa, need, ctx->lds_max);
    }
    if (s != SNMF_OK) {
        delete o;
        return s;
    }
    const size_t SS = (size_t)S, Fb = (size_t)(F + kWb64RB - 1) / kWb64RB * kWb64RB;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * sz;
    o->ntail = ntail;
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->B, SS * r * F); D(&o->Bfix, SS * Rd * F); D(&o->Btmp, SS * Rd * F);
    D(&o->Wn, SS * r * F); D(&o->WnT, SS * r * F); D(&o->wn, SS * r); D(&o->csum, SS * r); D(&o->H0, SS * r);
    D(&o->lambda_dav, SS * F); D(&o->Xm_tilde, SS * F); D(&o->r_blk, SS * F * o->Pl); D(&o->ldblk, SS * F * o->ma);
    D(&o->adblk, SS * o->Ra * o->ma); D(&o->Ad0, SS * o->Ra * o->ma); D(&o->rup, SS * o->Ra); D(&o->dev, SS); D(&o->tail, SS * ntail);
    if (p->class_outputs) {
        D(&o->tail_x, SS * ntail);
        D(&o->tail_d, SS * ntail);
    }
    if (p->adapt_train_N) {
        D(&o->Wu, SS * o->Ra * F); D(&o->Wm, SS * Fb * kWb64RP); D(&o->Q, SS * Fb * kWb64RP); D(&o->Vt, SS * Fb * o->ma);
        if (p->beta_div != 1.0) D(&o->P, SS * Fb * kWb64RP);
    }
    D(&o->win_s, (size_t)sz); D(&o->win_i, (size_t)sz); D(&o->tw, (size_t)N / 2); D(&o->Bxd, (size_t)F * p->R_x);
    D(&o->rs_slots, SS); D(&o->rs_B, SS * Rd * F); D(&o->rs_H, SS * r); D(&o->rs_A, SS * o->Ra * o->ma);
    D(&o->meta_i, 6 * SS); D(&o->meta_l, 3 * SS);
    if (s != SNMF_OK) {
        online_batch_f64_destroy(o);
        return s == SNMF_ERR_NOMEM ? fail(SNMF_ERR_NOMEM, "fp64 batched separator: device memory for %d streams", S) : s;
    }
    std::vector<double2> htw(N / 2);
    for (int q = 0; q < N / 2; ++q) {
        const double ang = -2.0 * M_PI * (double)q / (double)N;
        htw[q] = make_double2(cos(ang), sin(ang));
    }
    int e = 0;
    auto H = [&](hipError_t x) { if (x != hipSuccess && !e) e = (int)x; };
    H(hipMemcpyAsync(o->win_s, win_stft, (size_t)sz * 8, hipMemcpyHostToDevice, st));
    H(hipMemcpyAsync(o->win_i, win_istft, (size_t)sz * 8, hipMemcpyHostToDevice, st));
    H(hipMemcpyAsync(o->tw, htw.data(), htw.size() * sizeof(double2), hipMemcpyHostToDevice, st));
    H(hipMemcpyAsync(o->Bxd, Bx, (size_t)F * p->R_x * 8, hipMemcpyHostToDevice, st));
    o->pending.assign(SS, {});
    o->hist.assign(SS, {});
    o->l.assign(SS, 0);
    o->finished.assign(SS, 0);
    o->trace.resize(SS);
    // every stream's state g: a restart of all S streams (the one initialisation path)
    std::vector<int32_t> all(SS);
    for (int k = 0; k < S; ++k) all[k] = k;
    const int rc = e ? SNMF_OK : b64_restart(o, S, all.data(), Bd0, H0, p->adapt_train_N ? Ad0 : nullptr);
    H(hipStreamSynchronize(st));
    if (e || rc) {
        online_batch_f64_destroy(o);
        if (!e) return rc;
        return fail(e == (int)hipErrorOutOfMemory ? SNMF_ERR_NOMEM : SNMF_ERR_NO_DEVICE, "fp64 online batch create: %s",
                    hipGetErrorString((hipError_t)e));
    }
    *out = o;
    return SNMF_OK;
}

int online_batch_f64_set_classes(OnlineBatchF64* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num,
                                 const int32_t* noise_rank) {
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    if (!o->p.class_outputs) return fail(SNMF_ERR_STATE, "class outputs were not requested at creation");
    if (o->started) return fail(SNMF_ERR_STATE, "snmf_online_batch_set_classes must precede the first process call");
    std::vector<int> cls;
    SN_TRY(online_class_ranges(event_num, event_rank, noise_num, noise_rank, o->p.R_x, o->p.R_d, &cls));
    return obatch_install_classes(o, cls, event_num, event_num + noise_num);
}

// the frame solves of frame `step` of every stream (step < 0: all C frames of the chunk), one workgroup per (frame, stream)
static int obm_frame_solve(OnlineBatchF64* o, const OBatchFrames& fr, int step, int C) {
    const snmf_online_params& p = o->p;
    HSolve64Args h{};
    h.Wn = o->Wn; h.WnT = o->WnT; h.wn = o->wn; h.csum = o->csum; h.H0 = o->H0; h.V = o->Ym; h.A = o->A; h.recon = o->reco; h.n_iter = o->nit;
    h.F = o->F; h.r = o->r; h.Rx = p.R_x; h.max_iter = p.max_iter; h.cost_check = p.cost_check; h.n = C * o->S;
    h.beta = p.beta_div; h.sparsity = p.sparsity; h.conv_eps = p.conv_eps; h.flr = kFlr64;
    hipLaunchKernelGGL(k_obhsolve64, dim3(step >= 0 ? 1 : C, o->S), dim3(1024), b64_lds_solve(o), o->ctx->stream, h, fr, step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static int obm_class_spectra(OnlineBatchF64* o, const OBatchFrames& fr, int step, int C) {
    hipLaunchKernelGGL(k_obclass64, dim3((o->F + 255) / 256, o->S, step >= 0 ? 1 : C), dim3(256), 0, o->ctx->stream, (const double*)o->B,
                       (const double*)o->A, (const int*)o->cls, o->n_cls, o->F, o->r, o->Xc, (int64_t)o->C * o->S * o->F, fr, step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// adaptation (gated on the device) + re-assembly + dictionary refresh after frame `step` of every stream
static int obm_adapt(OnlineBatchF64* o, const OBatchFrames& fr, int step) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    WBatch64Args w{};
    w.status = o->status; w.nfr = fr.nfr; w.step = step; w.S = o->S; w.ldblk = o->ldblk; w.adblk = o->adblk; w.rup = o->rup; w.dev = o->dev;
    w.B = o->B; w.Wu = o->Wu; w.Wm = o->Wm; w.Q = o->Q; w.P = o->P; w.Vt = o->Vt; w.iters = o->iters;
    w.F = o->F; w.r = o->r; w.Rx = p.R_x; w.Ra = o->Ra; w.ma = o->ma; w.max_iter = p.max_iter; w.cost_check = p.cost_check;
    w.beta = p.beta_div; w.sparsity = p.sparsity; w.flr = kFlr64; w.conv_eps = p.conv_eps;
    const size_t lds = wbatch64_lds(o->Ra, o->ma, p.beta_div == 1.0);
    auto launch = [&](auto kern) -> int {
        SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)kern, lds));
        hipLaunchKernelGGL(kern, dim3(o->S), dim3(kWb64NT), lds, st, w);
        HIP_TRY(hipGetLastError());
        return SNMF_OK;
    };
    if (p.beta_div == 1.0) SN_TRY(launch(k_wadapt_batch64<kWb64KL>));
    else if (p.beta_div == 2.0) SN_TRY(launch(k_wadapt_batch64<kWb64ED>));
    else SN_TRY(launch(k_wadapt_batch64<kWb64GEN>));
    hipLaunchKernelGGL(k_obassemble64, dim3(p.R_d, o->S), dim3(256), 0, st, (const OnlineStatus*)o->status, fr.nfr, step, o->S,
                       (const double*)o->B, (const double*)o->Wu, (const double*)o->Bfix, (const uint8_t*)o->rup, o->F, o->r, p.R_x, o->Ra,
                       p.R_d, o->Btmp);
    HIP_TRY(hipGetLastError());
    ORefresh64Args ra{};
    ra.status = o->status; ra.nfr = fr.nfr; ra.step = step; ra.S = o->S; ra.Btmp = o->Btmp; ra.B = o->B; ra.Wn = o->Wn; ra.WnT = o->WnT;
    ra.wn = o->wn; ra.csum = o->csum; ra.F = o->F; ra.r = o->r; ra.Rx = p.R_x; ra.k0 = p.R_x;
    hipLaunchKernelGGL(k_obrefresh64, dim3(p.R_d, o->S), dim3(256), 0, st, ra);  // next frame's init_w (:140-146)
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// STFT of every frame of the chunk, the dynamic LDS of the chunk's frame solves and post-filter, and the post-filter's arguments
static int obm_begin_chunk(OnlineBatchF64* o, const OBatchFrames& fr, int C) {
    const snmf_online_params& p = o->p;
    const int S = o->S;
    hipStream_t st = o->ctx->stream;
    const size_t lds_fft = b64_lds_fft(o);
    OStftArgsT<double> sa{};
    sa.sig = o->sig; sa.sz = p.framelength; sa.hop = p.frameshift; sa.dcbin = p.dcbin; sa.preemph = p.preemph; sa.win = o->win_s; sa.tw = o->tw;
    sa.powv = p.pow; sa.floorv = p.nonzerofloor; sa.Ym = o->Ym; sa.Yph = o->Yph; sa.ld = o->F; sa.n_frames = C;
    int rc = SNMF_OK;
    by_logn([&](auto L) {
        rc = ensure_dyn_lds(o->ctx->device, (const void*)k_obstft64<decltype(L)::value>, lds_fft);
        if (rc == SNMF_OK) hipLaunchKernelGGL(k_obstft64<decltype(L)::value>, dim3(C, S), dim3(256), lds_fft, st, sa, fr);
    }, o->N);
    SN_TRY(rc);
    HIP_TRY(hipGetLastError());
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_obhsolve64, b64_lds_solve(o)));
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_obpost64, b64_lds_post(o)));
    OPostArgsT<double>& a = o->post_a;  // (stream 0's pointers; k_obpost64 re-bases them)
    a.A = o->A; a.hst = o->nit; a.recon = o->reco; a.Ym = o->Ym; a.lambda_dav = o->lambda_dav; a.Xm_tilde = o->Xm_tilde;
    a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk; a.rup = o->rup; a.dev = o->dev; a.status = o->status;
    a.Xt_out = o->Xt; a.Xh_out = o->Xh; a.Dh_out = o->Dh;
    a.F = o->F; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.Pk = p.P_len_k; a.dcbin = p.dcbin; a.gap = p.blk_gap;
    a.l = 1; a.blk_sparse = p.blk_sparse; a.adapt = p.adapt_train_N; a.wiener = p.enhance_method == 0; a.init_N_len = p.init_N_len;
    a.switch_at = (int)std::floor(p.overlap_m_a * p.m_a);
    a.alpha_p = p.alpha_p; a.alpha_eta = p.alpha_eta; a.alpha_d = p.alpha_d; a.beta0 = p.beta; a.beta_max = p.beta_max; a.Ar_up = p.Ar_up;
    a.flr = p.nonzerofloor;
    a.recon_len = o->F; a.n = 1; a.a_stride = o->r;
    return SNMF_OK;
}

static int obm_post(OnlineBatchF64* o, const OBatchFrames& fr, int step) {
    hipLaunchKernelGGL(k_obpost64, dim3(o->S), dim3(1024), b64_lds_post(o), o->ctx->stream, o->post_a, fr, step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// the synthesis of one signal: k_obtail64 (store = 0: the stream's tail into the buffer's head; 1: back out), k_obistft64, k_obola64
static int obm_tail(OnlineBatchF64* o, double* tail, const OBatchFrames& fr, int64_t syn_stride, int store) {
    hipLaunchKernelGGL(k_obtail64, dim3(o->S), dim3(256), 0, o->ctx->stream, o->syn, tail, fr.nfr, syn_stride, o->nov, o->p.framelength, store);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static int obm_istft(OnlineBatchF64* o, const double* mag, const OBatchFrames& fr, int C, int64_t syn_stride) {
    const snmf_online_params& p = o->p;
    const int S = o->S, nov = o->nov;
    hipStream_t st = o->ctx->stream;
    const size_t lds_fft = b64_lds_fft(o);
    OIstftArgsT<double> ia{};
    ia.mag = mag; ia.ph = o->Yph; ia.ld = o->F; ia.n_frames = C; ia.sz = p.framelength; ia.dcb = p.dcbin_back; ia.powv = p.pow;
    ia.scale = p.overlapscale / (double)o->N; ia.preemph = p.preemph; ia.win = o->win_i; ia.tw = o->tw; ia.syn = o->syn;
    int rc = SNMF_OK;
    by_logn([&](auto L) {
        rc = ensure_dyn_lds(o->ctx->device, (const void*)k_obistft64<decltype(L)::value>, lds_fft);
        if (rc == SNMF_OK) hipLaunchKernelGGL(k_obistft64<decltype(L)::value>, dim3(C, S), dim3(256), lds_fft, st, ia, fr.nfr, S, syn_stride, nov);
    }, o->N);
    SN_TRY(rc);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static int obm_ola(OnlineBatchF64* o, int gx, const OBatchFrames& fr, int64_t syn_stride, const int* d_if, const int* d_no, const int64_t* d_oo,
                   double* of, int16_t* o16) {
    const snmf_online_params& p = o->p;
    hipLaunchKernelGGL(k_obola64, dim3(gx, o->S), dim3(256), 0, o->ctx->stream, (const double*)o->syn, syn_stride, fr, d_if, d_no, d_oo, p.delay,
                       p.framelength, p.frameshift, o->nov, of, o16);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int online_batch_f64_process(OnlineBatchF64* o, const double* const* pcm, const int64_t* n, const int32_t* flush, double* const* xt,
                             int16_t* const* xt_i16, double* const* xh, double* const* dh, double* const* xhi, double* const* dhi,
                             const int64_t* cap, int64_t* n_out) {
    return obatch_process(o, pcm, n, flush, xt, xt_i16, xh, dh, xhi, dhi, cap, n_out);
}

int online_batch_f64_restart(OnlineBatchF64* o, int32_t n, const int32_t* slots, const double* Bd, const double* H0, const double* Ad) {
    SN_TRY(obatch_restart_check(o, n, slots));
    if (n == 0) return SNMF_OK;
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    if (int rc = b64_restart(o, n, slots, Bd, H0, o->p.adapt_train_N ? Ad : nullptr)) {
        o->failed = true;  // some of the listed streams may be half reset
        return rc;
    }
    return SNMF_OK;
}

void online_batch_f64_dims(OnlineBatchF64* o, int* r, int* ra_ma) {
    *r = o->r;
    *ra_ma = o->Ra * o->ma;
}

int online_batch_f64_get_basis(OnlineBatchF64* o, int32_t k, double* Bd, int64_t ld) {
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    if (ld < o->F) return fail(SNMF_ERR_INVALID, "ld < F");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    const size_t F = o->F;
    HIP_TRY(hipMemcpy2D(Bd, (size_t)ld * 8, o->B + (size_t)k * o->r * F + (size_t)o->p.R_x * F, F * 8, F * 8, (size_t)o->p.R_d,
                        hipMemcpyDeviceToHost));
    return SNMF_OK;
}

int online_batch_f64_trace(OnlineBatchF64* o, int32_t k, snmf_online_frame* out, int64_t cap, int64_t* n) { return obatch_trace(o, k, out, cap, n); }
