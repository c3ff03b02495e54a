// snmf_tu_online_batch_f64.hip -- the fp64 mode of the batched online separator (snmf_online_batch_create_f64 /
// snmf_online_batch_process_f64), kernels in snmf_online_batch_f64.h.  A translation unit of its own, so that the fp32 batch
// kernels' and the single-stream fp64 kernels' code does not move.  The snmf_online_batch handle lives in
// snmf_tu_online_batch.hip; it holds an OnlineBatchF64 and forwards.
// Host side as the fp32 batch: per stream the hop queue / history / flush logic, on the device one fixed sequence of
// launches per frame step for all streams (frame solves, post-filter, class spectra, gated adaptation / re-assembly /
// refresh) -- with the dictionary fixed, one launch of each for the whole chunk.  A chunk synchronises ONCE.
#include "snmf_internal.h"
#include "snmf_online_batch_f64.h"
#include "snmf_online_batch_f64_host.h"
#include "snmf_online_classes.h"

namespace {
constexpr size_t kB64TraceCap = 1u << 16;   // per stream: the newest 65536 frames, as snmf_online_trace
constexpr int64_t kB64ChunkSlots = 16384;  // (frame, stream) slots of one device chunk
constexpr double kFlr64 = 1e-9;            // src/sparse_nmf.m:166, as a double
}

struct OnlineBatchF64 {
    snmf_ctx* ctx = nullptr;
    snmf_online_params p{};
    int S = 0, F = 0, r = 0, N = 0, nov = 0, Ra = 1, ma = 1, Pl = 1;
    bool started = false;  // a process call was made (set_classes must come first)
    // per stream, device
    double *B = nullptr, *Bfix = nullptr, *Btmp = nullptr;                   // [B_DFT_x | B_DFT_d], the dictionary each stream started with, scratch
    double *Wn = nullptr, *WnT = nullptr, *wn = nullptr, *csum = nullptr;    // images of the frame solve (k_obrefresh64)
    double *H0 = nullptr, *Ad0 = nullptr, *lambda_dav = nullptr, *Xm_tilde = nullptr, *r_blk = nullptr, *ldblk = nullptr, *adblk = nullptr;
    double *Wu = nullptr, *Wm = nullptr, *Q = nullptr, *P = nullptr, *Vt = nullptr;  // k_wadapt_batch64's result and scratch
    double *tail = nullptr, *tail_x = nullptr, *tail_d = nullptr;
    uint8_t* rup = nullptr;
    OnlineDev* dev = nullptr;
    double *win_s = nullptr, *win_i = nullptr, *Bxd = nullptr;  // shared
    double2* tw = nullptr;
    // restart uploads (sized for all S streams)
    int* rs_slots = nullptr;
    double *rs_B = nullptr, *rs_H = nullptr, *rs_A = nullptr;
    size_t ntail = 0;
    // per chunk, device (grown on demand)
    int C = 0;  // frames per stream per chunk
    size_t cap_sig = 0, cap_out = 0;
    double *sig = nullptr, *Ym = nullptr, *A = nullptr, *reco = nullptr, *Xt = nullptr, *Xh = nullptr, *Dh = nullptr, *syn = nullptr, *outf = nullptr;
    double2* Yph = nullptr;
    int16_t* out16 = nullptr;
    int *nit = nullptr, *iters = nullptr;
    OnlineStatus* status = nullptr;
    // per-class outputs: n_ev event classes then n_cls - n_ev noise classes; n_cls = 0: none set
    int n_ev = 0, n_cls = 0;
    int* cls = nullptr;            // [n_cls + 1] column ranges over [B_x | B_d] (snmf_online_classes.h)
    double* tail_c = nullptr;      // [n_cls][S][ntail] one overlap-add tail per class and stream
    double *Xc = nullptr, *out_c = nullptr;  // per chunk, class-major: spectra [n_cls][C * S][F], hops [n_cls][cap_out]
    int* meta_i = nullptr;         // [6][S] nfr, nreal, l0, i_first, n_out, (pad)
    int64_t* meta_l = nullptr;     // [3][S] off, zoff, out_off
    // host state, per stream
    std::vector<std::vector<double>> pending, hist;
    std::vector<int64_t> l;
    std::vector<uint8_t> finished;
    std::vector<std::deque<snmf_online_frame>> trace;
    bool failed = false;
};

static size_t b64_lds_fft(const OnlineBatchF64* o) { return (size_t)2 * o->N * sizeof(double2); }
static size_t b64_lds_solve(const OnlineBatchF64* o) { return (size_t)(4 * o->F + 3 * o->r + 32) * 8; }
static size_t b64_lds_post(const OnlineBatchF64* o) { return (size_t)(o->r + 6 * o->F) * 8; }

static void b64_free_chunk(OnlineBatchF64* o) {
    void* ptrs[] = {o->sig, o->Ym, o->A, o->reco, o->Xt, o->Xh, o->Dh, o->syn, o->outf, o->Yph, o->out16, o->nit, o->iters, o->status,
                    o->Xc, o->out_c};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->sig = o->Ym = o->A = o->reco = o->Xt = o->Xh = o->Dh = o->syn = o->outf = o->Xc = o->out_c = nullptr;
    o->Yph = nullptr;
    o->out16 = nullptr;
    o->nit = o->iters = nullptr;
    o->status = nullptr;
    o->C = 0;
    o->cap_sig = o->cap_out = 0;
}

void online_batch_f64_destroy(OnlineBatchF64* o) {
    if (!o) return;
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
    b64_free_chunk(o);
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
    const int sz = p.framelength, hop = p.frameshift;
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        o->pending[s].clear();
        o->hist[s].assign((size_t)(sz - hop), 0.0);
        o->l[s] = 0;
        o->finished[s] = 0;
        o->trace[s].clear();
    }
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
    const int nc = event_num + noise_num;
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    b64_free_chunk(o);  // the class-major chunk buffers depend on the class count
    for (void** q : {(void**)&o->cls, (void**)&o->tail_c}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    o->n_ev = o->n_cls = 0;
    const size_t nt = (size_t)nc * o->S * o->ntail;
    SN_TRY(dalloc(&o->cls, cls.size()));
    SN_TRY(dalloc(&o->tail_c, nt));
    HIP_TRY(hipMemcpyAsync(o->cls, cls.data(), cls.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(o->tail_c, 0, nt * 8, st));
    HIP_TRY(hipStreamSynchronize(st));
    o->n_ev = event_num;
    o->n_cls = nc;
    return SNMF_OK;
}

// chunk buffers for C frames per stream and the given signal / output sizes
static int b64_reserve(OnlineBatchF64* o, int C, size_t n_sig, size_t n_out) {
    if (C <= o->C && n_sig <= o->cap_sig && n_out <= o->cap_out) return SNMF_OK;
    hipStreamSynchronize(o->ctx->stream);
    C = std::max(C, o->C);
    n_sig = std::max(n_sig, o->cap_sig);
    n_out = std::max(n_out, o->cap_out);
    b64_free_chunk(o);
    const size_t slots = (size_t)C * o->S, F = o->F, sz = o->p.framelength;
    SN_TRY(dalloc(&o->sig, n_sig));
    SN_TRY(dalloc(&o->Ym, F * slots));
    SN_TRY(dalloc(&o->Yph, F * slots));
    SN_TRY(dalloc(&o->A, (size_t)o->r * slots));
    SN_TRY(dalloc(&o->reco, 2 * F * slots));
    SN_TRY(dalloc(&o->Xt, F * slots));
    if (o->p.class_outputs) {
        SN_TRY(dalloc(&o->Xh, F * slots));
        SN_TRY(dalloc(&o->Dh, F * slots));
    }
    SN_TRY(dalloc(&o->syn, (size_t)o->S * (C + o->nov - 1) * sz));
    SN_TRY(dalloc(&o->outf, 3 * std::max<size_t>(n_out, 1)));  // x_tilde | x_hat | d_hat
    SN_TRY(dalloc(&o->out16, std::max<size_t>(n_out, 1)));
    if (o->n_cls) {
        SN_TRY(dalloc(&o->Xc, (size_t)o->n_cls * F * slots));
        SN_TRY(dalloc(&o->out_c, (size_t)o->n_cls * std::max<size_t>(n_out, 1)));
    }
    SN_TRY(dalloc(&o->nit, slots));
    SN_TRY(dalloc(&o->iters, slots));
    SN_TRY(dalloc(&o->status, slots));
    o->C = C;
    o->cap_sig = n_sig;
    o->cap_out = n_out;
    return SNMF_OK;
}

// the frame solves of frame `step` of every stream (step < 0: all C frames of the chunk), one workgroup per (frame, stream)
static int b64_frame_solve(OnlineBatchF64* o, const OBatchFrames& fr, int step, int C) {
    const snmf_online_params& p = o->p;
    HSolve64Args h{};
    h.Wn = o->Wn; h.WnT = o->WnT; h.wn = o->wn; h.csum = o->csum; h.H0 = o->H0; h.V = o->Ym; h.A = o->A; h.recon = o->reco; h.n_iter = o->nit;
    h.F = o->F; h.r = o->r; h.Rx = p.R_x; h.max_iter = p.max_iter; h.cost_check = p.cost_check; h.n = C * o->S;
    h.beta = p.beta_div; h.sparsity = p.sparsity; h.conv_eps = p.conv_eps; h.flr = kFlr64;
    hipLaunchKernelGGL(k_obhsolve64, dim3(step >= 0 ? 1 : C, o->S), dim3(1024), b64_lds_solve(o), o->ctx->stream, h, fr, step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static int b64_class_spectra(OnlineBatchF64* o, const OBatchFrames& fr, int step, int C) {
    hipLaunchKernelGGL(k_obclass64, dim3((o->F + 255) / 256, o->S, step >= 0 ? 1 : C), dim3(256), 0, o->ctx->stream, (const double*)o->B,
                       (const double*)o->A, (const int*)o->cls, o->n_cls, o->F, o->r, o->Xc, (int64_t)o->C * o->S * o->F, fr, step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// adaptation (gated on the device) + re-assembly + dictionary refresh after frame `step` of every stream
static int b64_adapt(OnlineBatchF64* o, const OBatchFrames& fr, int step) {
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

// One device chunk: stream s runs nfr[s] frames (its next nreal[s] PCM frames, then nfr - nreal flush frames).  Appends
// every stream's output hops and trace records.
struct B64Sink {
    std::vector<double> f, x, d;
    std::vector<int16_t> i16;
    std::vector<std::vector<double>> c;  // [n_cls] the class signals
};
static int b64_run_chunk(OnlineBatchF64* o, const std::vector<int>& nfr, const std::vector<int>& nreal, const std::vector<int64_t>& consumed,
                         bool want_f, bool want_i16, bool want_cls, bool want_ci, std::vector<B64Sink>& sink) {
    const snmf_online_params& p = o->p;
    const int S = o->S, F = o->F, sz = p.framelength, hop = p.frameshift, nov = o->nov;
    hipStream_t st = o->ctx->stream;
    const int C = *std::max_element(nfr.begin(), nfr.end());
    if (C == 0) return SNMF_OK;
    // host framing: stream s's samples = [history | its hops of this chunk], then sz zeros for its flush frames
    std::vector<int> mi(6 * (size_t)S, 0);
    std::vector<int64_t> ml(3 * (size_t)S, 0);
    int* h_nfr = mi.data(); int* h_nreal = h_nfr + S; int* h_l0 = h_nreal + S; int* h_if = h_l0 + S; int* h_no = h_if + S;
    int64_t* h_off = ml.data(); int64_t* h_zoff = h_off + S; int64_t* h_oo = h_zoff + S;
    size_t n_sig = 0, n_out = 0;
    for (int s = 0; s < S; ++s) {
        h_nfr[s] = nfr[s];
        h_nreal[s] = nreal[s];
        h_l0[s] = (int)std::min<int64_t>(o->l[s] + 1, 1 << 30);
        h_if[s] = (int)std::max<int64_t>(0, (int64_t)p.delay + 1 - h_l0[s]);
        h_no[s] = std::max(0, nfr[s] - h_if[s]);
        h_off[s] = (int64_t)n_sig;
        if (nreal[s] > 0) n_sig += (size_t)(sz - hop) + (size_t)nreal[s] * hop;
        h_zoff[s] = (int64_t)n_sig;
        if (nfr[s] > nreal[s]) n_sig += (size_t)sz;
        h_oo[s] = (int64_t)n_out;
        n_out += (size_t)h_no[s] * hop;
    }
    std::vector<double> sig(std::max<size_t>(n_sig, 1), 0.0);
    for (int s = 0; s < S; ++s) {
        if (nreal[s] <= 0) continue;
        double* d = sig.data() + h_off[s];
        std::copy(o->hist[s].begin(), o->hist[s].end(), d);
        std::copy(o->pending[s].begin() + consumed[s] * hop, o->pending[s].begin() + (consumed[s] + nreal[s]) * hop, d + (sz - hop));
    }
    SN_TRY(b64_reserve(o, C, sig.size(), n_out));
    HIP_TRY(hipMemcpyAsync(o->sig, sig.data(), sig.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->meta_i, mi.data(), mi.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->meta_l, ml.data(), ml.size() * 8, hipMemcpyHostToDevice, st));
    OBatchFrames fr{};
    fr.nfr = o->meta_i; fr.nreal = o->meta_i + S; fr.l0 = o->meta_i + 2 * S; fr.off = o->meta_l; fr.zoff = o->meta_l + S; fr.S = S;
    const int* d_if = o->meta_i + 3 * S;
    const int* d_no = o->meta_i + 4 * S;
    const int64_t* d_oo = o->meta_l + 2 * S;
    // STFT of every frame of the chunk
    const size_t lds_fft = b64_lds_fft(o), lds_post = b64_lds_post(o);
    OStftArgsT<double> sa{};
    sa.sig = o->sig; sa.sz = sz; sa.hop = hop; sa.dcbin = p.dcbin; sa.preemph = p.preemph; sa.win = o->win_s; sa.tw = o->tw;
    sa.powv = p.pow; sa.floorv = p.nonzerofloor; sa.Ym = o->Ym; sa.Yph = o->Yph; sa.ld = F; sa.n_frames = C;
    int rc = SNMF_OK;
    by_logn([&](auto L) {
        rc = ensure_dyn_lds(o->ctx->device, (const void*)k_obstft64<decltype(L)::value>, lds_fft);
        if (rc == SNMF_OK) hipLaunchKernelGGL(k_obstft64<decltype(L)::value>, dim3(C, S), dim3(256), lds_fft, st, sa, fr);
    }, o->N);
    SN_TRY(rc);
    HIP_TRY(hipGetLastError());
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_obhsolve64, b64_lds_solve(o)));
    SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_obpost64, lds_post));
    // post-filter arguments (stream 0's pointers; k_obpost64 re-bases them)
    OPostArgsT<double> a{};
    a.A = o->A; a.hst = o->nit; a.recon = o->reco; a.Ym = o->Ym; a.lambda_dav = o->lambda_dav; a.Xm_tilde = o->Xm_tilde;
    a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk; a.rup = o->rup; a.dev = o->dev; a.status = o->status;
    a.Xt_out = o->Xt; a.Xh_out = o->Xh; a.Dh_out = o->Dh;
    a.F = F; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.Pk = p.P_len_k; a.dcbin = p.dcbin; a.gap = p.blk_gap;
    a.l = 1; a.blk_sparse = p.blk_sparse; a.adapt = p.adapt_train_N; a.wiener = p.enhance_method == 0; a.init_N_len = p.init_N_len;
    a.switch_at = (int)std::floor(p.overlap_m_a * p.m_a);
    a.alpha_p = p.alpha_p; a.alpha_eta = p.alpha_eta; a.alpha_d = p.alpha_d; a.beta0 = p.beta; a.beta_max = p.beta_max; a.Ar_up = p.Ar_up;
    a.flr = p.nonzerofloor;
    a.recon_len = F; a.n = 1; a.a_stride = o->r;
    HIP_TRY(hipMemsetAsync(o->iters, 0, (size_t)C * S * 4, st));
    if (!p.adapt_train_N) {
        // fixed dictionaries: every frame solve of the chunk in one launch, then one post-filter launch walks the frames
        SN_TRY(b64_frame_solve(o, fr, -1, C));
        hipLaunchKernelGGL(k_obpost64, dim3(S), dim3(1024), lds_post, st, a, fr, -1);
        HIP_TRY(hipGetLastError());
        if (o->n_cls) SN_TRY(b64_class_spectra(o, fr, -1, C));
    } else {
        for (int i = 0; i < C; ++i) {  // one frame step of every stream, nothing decided on the host
            SN_TRY(b64_frame_solve(o, fr, i, C));
            hipLaunchKernelGGL(k_obpost64, dim3(S), dim3(1024), lds_post, st, a, fr, i);
            HIP_TRY(hipGetLastError());
            if (o->n_cls) SN_TRY(b64_class_spectra(o, fr, i, C));
            SN_TRY(b64_adapt(o, fr, i));
        }
    }
    // inverse STFT behind each stream's kept frames, overlap-add
    const int64_t syn_stride = (int64_t)(C + nov - 1) * sz;
    auto synth = [&](const double* mag, double* tail, double* of, int16_t* o16) -> int {
        if (nov > 1) {
            hipLaunchKernelGGL(k_obtail64, dim3(S), dim3(256), 0, st, o->syn, tail, fr.nfr, syn_stride, nov, sz, 0);
            HIP_TRY(hipGetLastError());
        }
        OIstftArgsT<double> ia{};
        ia.mag = mag; ia.ph = o->Yph; ia.ld = F; ia.n_frames = C; ia.sz = sz; ia.dcb = p.dcbin_back; ia.powv = p.pow;
        ia.scale = p.overlapscale / (double)o->N; ia.preemph = p.preemph; ia.win = o->win_i; ia.tw = o->tw; ia.syn = o->syn;
        int r2 = SNMF_OK;
        by_logn([&](auto L) {
            r2 = ensure_dyn_lds(o->ctx->device, (const void*)k_obistft64<decltype(L)::value>, lds_fft);
            if (r2 == SNMF_OK)
                hipLaunchKernelGGL(k_obistft64<decltype(L)::value>, dim3(C, S), dim3(256), lds_fft, st, ia, fr.nfr, S, syn_stride, nov);
        }, o->N);
        SN_TRY(r2);
        HIP_TRY(hipGetLastError());
        if (n_out > 0) {
            const int gx = std::max(1, std::min(64, (int)((size_t)C * hop / 256 + 1)));
            hipLaunchKernelGGL(k_obola64, dim3(gx, S), dim3(256), 0, st, (const double*)o->syn, syn_stride, fr, d_if, d_no, d_oo, p.delay, sz,
                               hop, nov, of, o16);
            HIP_TRY(hipGetLastError());
        }
        if (nov > 1) {
            hipLaunchKernelGGL(k_obtail64, dim3(S), dim3(256), 0, st, o->syn, tail, fr.nfr, syn_stride, nov, sz, 1);
            HIP_TRY(hipGetLastError());
        }
        return SNMF_OK;
    };
    // the three signals go to the thirds of outf: x_tilde, x_hat, d_hat
    std::vector<double> hf, hx, hd;
    std::vector<int16_t> h16;
    auto fetch = [&](std::vector<double>& v, const double* src) -> int {
        v.resize(n_out);
        if (n_out) HIP_TRY(hipMemcpyAsync(v.data(), src, n_out * 8, hipMemcpyDeviceToHost, st));
        return SNMF_OK;
    };
    SN_TRY(synth(o->Xt, o->tail, o->outf, want_i16 ? o->out16 : nullptr));
    if (want_f) SN_TRY(fetch(hf, o->outf));
    if (want_i16) {
        h16.resize(n_out);
        if (n_out) HIP_TRY(hipMemcpyAsync(h16.data(), o->out16, n_out * 2, hipMemcpyDeviceToHost, st));
    }
    if (p.class_outputs) {  // x_hat / d_hat of :350-361, same synthesis
        SN_TRY(synth(o->Xh, o->tail_x, o->outf + n_out, nullptr));
        SN_TRY(synth(o->Dh, o->tail_d, o->outf + 2 * n_out, nullptr));
        if (want_cls) {
            SN_TRY(fetch(hx, o->outf + n_out));
            SN_TRY(fetch(hd, o->outf + 2 * n_out));
        }
    }
    // x_hat_i / d_hat_i (:356-361): each class of the class-major stack through the same synthesis on its own tails
    std::vector<std::vector<double>> hc(want_ci ? o->n_cls : 0);
    for (int c = 0; c < o->n_cls; ++c) {
        double* oc = o->out_c + (size_t)c * std::max<size_t>(o->cap_out, 1);
        SN_TRY(synth(o->Xc + (size_t)c * o->C * S * F, o->tail_c + (size_t)c * S * o->ntail, oc, nullptr));
        if (want_ci) SN_TRY(fetch(hc[c], oc));
    }
    // statuses + adaptation verdicts of the chunk: one copy each
    std::vector<OnlineStatus> hs((size_t)C * S);
    std::vector<int> hit((size_t)C * S);
    HIP_TRY(hipMemcpyAsync(hs.data(), o->status, hs.size() * sizeof(OnlineStatus), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hit.data(), o->iters, hit.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int s = 0; s < S; ++s) {
        for (int i = 0; i < nfr[s]; ++i) {
            const OnlineStatus& q = hs[(size_t)i * S + s];
            snmf_online_frame tr{};
            tr.n_iter = q.n_iter; tr.trig = q.trig; tr.n_up = q.n_up; tr.beta = q.beta; tr.A_x_mag = q.A_x_mag; tr.A_d_mag = q.A_d_mag;
            tr.Q_control = q.Q_control;
            if (p.adapt_train_N && q.do_solve && q.n_up > 0) {
                tr.solved = 1;
                tr.adapt_iters = hit[(size_t)i * S + s];
            }
            o->trace[s].push_back(tr);
            if (o->trace[s].size() > kB64TraceCap) o->trace[s].pop_front();
        }
        const size_t a0 = (size_t)h_oo[s], n = (size_t)h_no[s] * hop;
        if (want_f) sink[s].f.insert(sink[s].f.end(), hf.begin() + a0, hf.begin() + a0 + n);
        if (want_i16) sink[s].i16.insert(sink[s].i16.end(), h16.begin() + a0, h16.begin() + a0 + n);
        if (want_cls) {
            sink[s].x.insert(sink[s].x.end(), hx.begin() + a0, hx.begin() + a0 + n);
            sink[s].d.insert(sink[s].d.end(), hd.begin() + a0, hd.begin() + a0 + n);
        }
        if (want_ci) {
            sink[s].c.resize(hc.size());
            for (size_t c = 0; c < hc.size(); ++c) sink[s].c[c].insert(sink[s].c[c].end(), hc[c].begin() + a0, hc[c].begin() + a0 + n);
        }
        if (nreal[s] > 0) {  // history for the next chunk: the last sz - hop samples this stream framed
            const double* end = sig.data() + h_off[s] + (sz - hop) + (size_t)nreal[s] * hop;
            o->hist[s].assign(end - (sz - hop), end);
        }
        o->l[s] += nfr[s];
    }
    return SNMF_OK;
}

int online_batch_f64_process(OnlineBatchF64* o, const double* const* pcm, const int64_t* n, const int32_t* flush, double* const* xt,
                             int16_t* const* xt_i16, double* const* xh, double* const* dh, double* const* xhi, double* const* dhi,
                             const int64_t* cap, int64_t* n_out) {
    if (!n || !pcm) return fail(SNMF_ERR_INVALID, "pcm / n is NULL");
    const int S = o->S;
    const snmf_online_params& p = o->p;
    const int hop = p.frameshift;
    if (n_out)
        for (int s = 0; s < S; ++s) n_out[s] = 0;
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    if ((xh || dh || xhi || dhi) && !p.class_outputs) return fail(SNMF_ERR_STATE, "class outputs were not requested at creation");
    const bool any_out = xt || xt_i16 || xh || dh || xhi || dhi;
    if (any_out && !cap) return fail(SNMF_ERR_INVALID, "cap is NULL");
    std::vector<int64_t> nfr_tot(S), tail(S);
    for (int s = 0; s < S; ++s) {
        if (n[s] < 0 || (n[s] > 0 && !pcm[s])) return fail(SNMF_ERR_INVALID, "stream %d: pcm is NULL", s);
        if (o->finished[s] && (n[s] > 0 || (flush && flush[s])))
            return fail(SNMF_ERR_STATE, "stream %d was flushed; restart it before feeding it", s);
        nfr_tot[s] = ((int64_t)o->pending[s].size() + n[s]) / hop;
        tail[s] = (flush && flush[s] && !o->finished[s]) ? p.delay + 1 : 0;
        const int64_t need = (nfr_tot[s] + tail[s]) * hop;
        auto short_cap = [&](const void* const* v) { return v && v[s] && cap[s] < need; };
        if (short_cap((const void* const*)xt) || short_cap((const void* const*)xt_i16) || short_cap((const void* const*)xh) ||
            short_cap((const void* const*)dh) || short_cap((const void* const*)xhi) || short_cap((const void* const*)dhi))
            return fail(SNMF_ERR_INVALID, "stream %d: output capacity %lld < %lld samples", s, (long long)cap[s], (long long)need);
    }
    o->started = true;
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    for (int s = 0; s < S; ++s)
        if (n[s] > 0) o->pending[s].insert(o->pending[s].end(), pcm[s], pcm[s] + n[s]);
    // chunks: up to C frames per stream, each stream's PCM frames first, then its flush frames
    const int nc1 = std::max(1, o->n_cls);  // (the class-major buffers grow with the classes)
    const int C = (int)std::max<int64_t>(1, std::min<int64_t>(4096, kB64ChunkSlots / ((int64_t)S * nc1)));
    std::vector<int64_t> done(S, 0);
    std::vector<B64Sink> sink(S);
    // class signals: with a partition set they come from the class kernel; without one x_hat / d_hat are the one class per side
    const bool cls_set = o->n_cls > 0, wci = cls_set && (xhi || dhi);
    const bool wf = xt != nullptr, wi = xt_i16 != nullptr, wc = xh || dh || (!cls_set && (xhi || dhi));
    for (;;) {
        std::vector<int> nfr(S), nreal(S);
        bool any = false;
        for (int s = 0; s < S; ++s) {
            const int64_t left = nfr_tot[s] + tail[s] - done[s];
            nfr[s] = (int)std::min<int64_t>(C, left);
            nreal[s] = (int)std::max<int64_t>(0, std::min<int64_t>(nfr[s], nfr_tot[s] - done[s]));
            any |= nfr[s] > 0;
        }
        if (!any) break;
        if (int rc = b64_run_chunk(o, nfr, nreal, done, wf, wi, wc, wci, sink)) {
            o->failed = true;  // frames of this call were consumed and the device state advanced: never retry on it
            return rc;
        }
        for (int s = 0; s < S; ++s) done[s] += nfr[s];
    }
    for (int s = 0; s < S; ++s) {
        o->pending[s].erase(o->pending[s].begin(), o->pending[s].begin() + nfr_tot[s] * hop);
        if (tail[s]) {
            o->pending[s].clear();  // a partial hop is dropped (src/NTF_sep_event_RT.m:69-76)
            o->finished[s] = 1;
        }
        const B64Sink& k = sink[s];
        if (wf && xt[s]) std::memcpy(xt[s], k.f.data(), k.f.size() * 8);
        if (wi && xt_i16[s]) std::memcpy(xt_i16[s], k.i16.data(), k.i16.size() * 2);
        if (xh && xh[s]) std::memcpy(xh[s], k.x.data(), k.x.size() * 8);
        if (dh && dh[s]) std::memcpy(dh[s], k.d.data(), k.d.size() * 8);
        size_t nc_out = 0;
        if (cls_set) {
            for (int c = 0; c < (int)k.c.size(); ++c) {
                double* dst = c < o->n_ev ? ((xhi && xhi[s]) ? xhi[s] + (size_t)c * cap[s] : nullptr)
                                          : ((dhi && dhi[s]) ? dhi[s] + (size_t)(c - o->n_ev) * cap[s] : nullptr);
                if (dst) std::memcpy(dst, k.c[c].data(), k.c[c].size() * 8);
                nc_out = std::max(nc_out, k.c[c].size());
            }
        } else {
            if (xhi && xhi[s]) std::memcpy(xhi[s], k.x.data(), k.x.size() * 8);
            if (dhi && dhi[s]) std::memcpy(dhi[s], k.d.data(), k.d.size() * 8);
        }
        if (n_out) n_out[s] = (int64_t)std::max(std::max(std::max(k.f.size(), k.i16.size()), std::max(k.x.size(), k.d.size())), nc_out);
    }
    return SNMF_OK;
}

int online_batch_f64_restart(OnlineBatchF64* o, int32_t n, const int32_t* slots, const double* Bd, const double* H0, const double* Ad) {
    if (n < 0 || n > o->S) return fail(SNMF_ERR_INVALID, "restart of %d streams in a batch of %d", n, o->S);
    if (n > 0 && !slots) return fail(SNMF_ERR_INVALID, "slots is NULL");
    std::vector<uint8_t> seen(o->S, 0);
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (s < 0 || s >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", s, o->S);
        if (seen[s]) return fail(SNMF_ERR_INVALID, "stream %d listed twice", s);
        seen[s] = 1;
    }
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (!o->finished[s] && (o->l[s] > 0 || !o->pending[s].empty()))
            return fail(SNMF_ERR_STATE, "stream %d is in the middle of a recording; flush it before a restart", s);
    }
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

int online_batch_f64_trace(OnlineBatchF64* o, int32_t k, snmf_online_frame* out, int64_t cap, int64_t* n) {
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    const auto& tr = o->trace[k];
    if (n) *n = (int64_t)tr.size();
    if (out && cap > 0) std::copy_n(tr.begin(), (size_t)std::min<int64_t>(cap, (int64_t)tr.size()), out);
    return SNMF_OK;
}
