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
    double *Wn = nullptr, *WnT = nullptr, *wn = nullptr, *csum = nullptr;    // images of the frame solve (k_obrefresh64)
    double *Wu = nullptr, *Wm = nullptr, *Q = nullptr, *P = nullptr, *Vt = nullptr;  // k_wadapt_batch64's result and scratch
    // per chunk, device (obm_reserve): the frame solves' activations, reconstructions and iteration counts
    double *A = nullptr, *reco = nullptr;
    int* nit = nullptr;
    OPostArgsT<double> post_a{};  // the post-filter's launch arguments of the current chunk (obm_begin_chunk)
    // settings per stream: the device table the kernels read, its host mirror (the uploads' source), and the entries as given
    OStreamSettings* set = nullptr;
    std::vector<OStreamSettings> hset;
    std::vector<snmf_online_stream_settings> uset;
    std::vector<uint8_t> has_ad0;  // per stream: Ad0 holds an Ad_blk0 the stream was given
};

// snmf_online_params -> the per-stream part of it
static snmf_online_stream_settings b64_settings_of(const snmf_online_params& p) {
    snmf_online_stream_settings q{};
    q.beta_div = p.beta_div; q.sparsity = p.sparsity; q.conv_eps = p.conv_eps; q.max_iter = p.max_iter;
    q.enhance_method = p.enhance_method; q.init_N_len = p.init_N_len;
    q.alpha_eta = p.alpha_eta; q.alpha_d = p.alpha_d; q.beta = p.beta; q.beta_max = p.beta_max;
    q.blk_sparse = p.blk_sparse; q.P_len_k = p.P_len_k; q.blk_gap = p.blk_gap; q.alpha_p = p.alpha_p;
    q.adapt_train_N = p.adapt_train_N; q.overlap_m_a = p.overlap_m_a; q.Ar_up = p.Ar_up;
    return q;
}

static OStreamSettings b64_table_entry(const snmf_online_stream_settings& q, int m_a) {
    OStreamSettings t{};
    t.beta_div = q.beta_div; t.sparsity = q.sparsity; t.conv_eps = q.conv_eps; t.max_iter = q.max_iter;
    t.enhance_method = q.enhance_method; t.init_N_len = q.init_N_len;
    t.alpha_eta = q.alpha_eta; t.alpha_d = q.alpha_d; t.beta = q.beta; t.beta_max = q.beta_max;
    t.blk_sparse = q.blk_sparse ? 1 : 0; t.P_len_k = q.P_len_k; t.blk_gap = q.blk_gap; t.alpha_p = q.alpha_p;
    t.adapt_train_N = q.adapt_train_N ? 1 : 0; t.switch_at = (int)std::floor(q.overlap_m_a * m_a); t.Ar_up = q.Ar_up;
    return t;
}

// what the streams' settings ask of the shared allocations
struct B64Needs {
    bool adapt = false, blk = false, nonkl = false;
    bool cls[3] = {false, false, false};  // divergence classes among the adapting streams (kWb64KL / ED / GEN)
};

static B64Needs b64_needs(const std::vector<OStreamSettings>& hs) {
    B64Needs n;
    for (const OStreamSettings& q : hs) {
        n.blk |= q.blk_sparse != 0;
        if (!q.adapt_train_N) continue;
        n.adapt = true;
        n.cls[wbatch64_class(q.beta_div)] = true;
        n.nonkl |= q.beta_div != 1.0;
    }
    return n;
}

// k_wadapt_batch64's envelope for every divergence class that adapts: R_a <= 64, m_a <= 128, the class's LDS image <= a compute unit's
static int b64_check_ring(const snmf_ctx* ctx, const snmf_online_params& p, const B64Needs& nd) {
    if (!nd.adapt) return SNMF_OK;
    for (int c = 0; c < 3; ++c) {
        if (!nd.cls[c]) continue;
        const size_t need = wbatch64_lds(p.R_a, p.m_a, c == kWb64KL);
        if (p.R_a > kWb64RP || p.m_a > kWb64MaxMa || need > ctx->lds_max)
            return fail(SNMF_ERR_UNSUPPORTED,
                        "fp64 batched adaptation: R_a = %d, m_a = %d is outside k_wadapt_batch64's envelope (R_a <= %d, m_a <= %d, %zu bytes of LDS "
                        "<= %zu)", p.R_a, p.m_a, kWb64RP, kWb64MaxMa, need, ctx->lds_max);
    }
    return SNMF_OK;
}

// The rings and the adaptation scratch, sized by what any stream needs: r_blk at P_len_l with a block-sparse stream, ldblk /
// adblk / Ad0 / rup and k_wadapt_batch64's scratch at R_a x m_a with an adapting one, P with an adapting stream off KL.  They
// only grow.  A ring that grows was used by no stream (a stream that does not use a ring never reads it), so it starts zeroed.
static int b64_fit_rings(OnlineBatchF64* o, const B64Needs& nd) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const size_t SS = (size_t)o->S, F = (size_t)o->F, Fb = (size_t)(o->F + kWb64RB - 1) / kWb64RB * kWb64RB;
    const int Ra = nd.adapt ? p.R_a : o->Ra, ma = nd.adapt ? p.m_a : o->ma, Pl = nd.blk ? p.P_len_l : o->Pl;
    auto renew = [&](auto** ptr, size_t n) -> int {
        if (*ptr) HIP_TRY(hipFree(*ptr));
        *ptr = nullptr;
        SN_TRY(dalloc(ptr, n));
        HIP_TRY(hipMemsetAsync(*ptr, 0, n * sizeof(**ptr), st));
        return SNMF_OK;
    };
    const bool grow_a = !o->adblk || Ra != o->Ra || ma != o->ma, grow_p = !o->r_blk || Pl != o->Pl;
    if ((grow_a || grow_p) && (o->adblk || o->r_blk)) HIP_TRY(hipStreamSynchronize(st));  // nothing in flight reads what is freed
    if (grow_p) {
        o->Pl = Pl;
        SN_TRY(renew(&o->r_blk, SS * F * Pl));
    }
    if (grow_a) {
        o->Ra = Ra;
        o->ma = ma;
        const size_t nA = (size_t)Ra * ma;
        SN_TRY(renew(&o->ldblk, SS * F * ma));
        SN_TRY(renew(&o->adblk, SS * nA));
        SN_TRY(renew(&o->Ad0, SS * nA));
        SN_TRY(renew(&o->rup, SS * Ra));
        SN_TRY(renew(&o->rs_A, SS * nA));
        std::fill(o->has_ad0.begin(), o->has_ad0.end(), 0);
    }
    if (nd.adapt && !o->Wu) {
        SN_TRY(dalloc(&o->Wu, SS * o->Ra * F));
        SN_TRY(dalloc(&o->Wm, SS * Fb * kWb64RP));
        SN_TRY(dalloc(&o->Q, SS * Fb * kWb64RP));
        SN_TRY(dalloc(&o->Vt, SS * Fb * o->ma));
    }
    if (nd.nonkl && !o->P) SN_TRY(dalloc(&o->P, SS * Fb * kWb64RP));
    return SNMF_OK;
}

// the driver's view of the table: which streams adapt (it steps frame by frame when any does)
static void b64_publish_adapt(OnlineBatchF64* o) {
    o->adapt_s.resize(o->hset.size());
    for (size_t k = 0; k < o->hset.size(); ++k) o->adapt_s[k] = (uint8_t)o->hset[k].adapt_train_N;
}

static size_t obm_lds_fft(const OnlineBatchF64* o) { return (size_t)2 * o->N * sizeof(double2); }  // the driver's hook, and k_obstft64's
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
    obatch_free_state(o);
    void* ptrs[] = {o->Wn, o->WnT, o->wn, o->csum, o->Wu, o->Wm, o->Q, o->P, o->Vt, o->set};
    for (void* q : ptrs)
        if (q) hipFree(q);
    delete o;
}

// Every column's dictionary images of the streams in rs_slots: the launch that ends a restart and follows a set-state (the
// driver's obm_state_refresh).
static int obm_state_refresh(OnlineBatchF64* o, int n) {
    ORefresh64Args ra{};
    ra.slots = o->rs_slots; ra.S = o->S; ra.B = o->B; ra.Wn = o->Wn; ra.WnT = o->WnT; ra.wn = o->wn; ra.csum = o->csum;
    ra.F = o->F; ra.r = o->r; ra.Rx = o->p.R_x; ra.k0 = 0;
    hipLaunchKernelGGL(k_obrefresh64, dim3(o->r, n), dim3(256), 0, o->ctx->stream, ra);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// The streams slots[0..n) start a new recording (obatch_restart): the fp64 mode's own are the listed streams' settings entries
// (the host table holds them already) and event dictionaries, uploaded ahead of the restart kernel, and has_ad0.  Bx: n x Rx x F,
// the listed streams' new event dictionaries, or NULL = each keeps its own.  Ad (n x Ra x ma) is read only when one of the
// listed streams adapts.
static int b64_restart(OnlineBatchF64* o, int n, const int32_t* slots, const double* Bx, const double* Bd, const double* H0, const double* Ad) {
    hipStream_t st = o->ctx->stream;
    const size_t nX = (size_t)o->p.R_x * o->F;
    bool adapts = false;
    for (int i = 0; i < n; ++i) adapts |= o->hset[slots[i]].adapt_train_N != 0;
    if (!adapts) Ad = nullptr;
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipMemcpyAsync(o->set + slots[i], &o->hset[slots[i]], sizeof(OStreamSettings), hipMemcpyHostToDevice, st));
        if (Bx) HIP_TRY(hipMemcpyAsync(o->Bxd + (size_t)slots[i] * nX, Bx + (size_t)i * nX, nX * 8, hipMemcpyHostToDevice, st));
        if (Ad) o->has_ad0[slots[i]] = 1;
    }
    return obatch_restart(o, n, slots, Bd, H0, Ad, (int64_t)nX, [&](const ORestartCommon<double>& a) {
        hipLaunchKernelGGL(k_obrestart64, dim3(n, kRsShared, kRsParts), dim3(256), 0, st, a, (const OStreamSettings*)o->set);
    });
}

int online_batch_f64_create(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* Bx, int bx_per_stream, const double* Bd0,
                            const double* H0, const double* Ad0, const snmf_online_stream_settings* settings, const double* win_stft,
                            const double* win_istft, OnlineBatchF64** out) {
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = p->fftlength, F = N / 2 + 1, r = p->R_x + p->R_d, sz = p->framelength, hop = p->frameshift, Rd = p->R_d;
    OnlineBatchF64* o = new OnlineBatchF64();
    o->ctx = ctx;
    o->p = *p;
    o->S = S; o->F = F; o->r = r; o->N = N;
    o->nov = (sz + hop - 1) / hop;
    o->uset.assign((size_t)S, b64_settings_of(*p));  // settings == NULL: S copies of p
    if (settings) o->uset.assign(settings, settings + S);
    for (const snmf_online_stream_settings& q : o->uset) o->hset.push_back(b64_table_entry(q, p->m_a));
    o->has_ad0.assign((size_t)S, 0);
    const B64Needs nd = b64_needs(o->hset);
    int s = SNMF_OK;
    if (obm_lds_fft(o) > ctx->lds_max || b64_lds_solve(o) > ctx->lds_max || b64_lds_post(o) > ctx->lds_max)
        s = fail(SNMF_ERR_UNSUPPORTED, "fp64 batched separator: fftlength %d with R_x + R_d = %d does not fit the LDS (%zu bytes)", N, r,
                 ctx->lds_max);
    if (s == SNMF_OK) s = b64_check_ring(ctx, *p, nd);
    if (s == SNMF_OK && nd.adapt && !Ad0) s = fail(SNMF_ERR_INVALID, "Ad_blk0 is required when a stream's adapt_train_N is set");
    if (s != SNMF_OK) {
        delete o;
        return s;
    }
    const size_t SS = (size_t)S;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * sz;
    o->ntail = ntail;
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->B, SS * r * F); D(&o->Bfix, SS * Rd * F); D(&o->Btmp, SS * Rd * F);
    D(&o->Wn, SS * r * F); D(&o->WnT, SS * r * F); D(&o->wn, SS * r); D(&o->csum, SS * r); D(&o->H0, SS * r);
    D(&o->lambda_dav, SS * F); D(&o->Xm_tilde, SS * F); D(&o->dev, SS); D(&o->tail, SS * ntail); D(&o->set, SS);
    if (s == SNMF_OK) s = b64_fit_rings(o, nd);  // r_blk, ldblk, adblk, Ad0, rup, rs_A and the adaptation scratch
    if (p->class_outputs) {
        D(&o->tail_x, SS * ntail);
        D(&o->tail_d, SS * ntail);
    }
    D(&o->win_s, (size_t)sz); D(&o->win_i, (size_t)sz); D(&o->tw, (size_t)N / 2); D(&o->Bxd, SS * F * p->R_x);
    D(&o->rs_slots, SS); D(&o->rs_B, SS * Rd * F); D(&o->rs_H, SS * r);
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
    {  // every stream's B_x: S dictionaries as they come, or the one dictionary uploaded once and copied on the device
        const size_t nX = (size_t)F * p->R_x;
        H(hipMemcpyAsync(o->Bxd, Bx, (bx_per_stream ? SS : 1) * nX * 8, hipMemcpyHostToDevice, st));
        for (size_t k = 1; k < SS && !bx_per_stream; ++k) H(hipMemcpyAsync(o->Bxd + k * nX, o->Bxd, nX * 8, hipMemcpyDeviceToDevice, st));
    }
    o->pending.assign(SS, {});
    o->hist.assign(SS, {});
    o->l.assign(SS, 0);
    o->finished.assign(SS, 0);
    o->trace.resize(SS);
    // every stream's state g: a restart of all S streams (the one initialisation path)
    std::vector<int32_t> all(SS);
    for (int k = 0; k < S; ++k) all[k] = k;
    b64_publish_adapt(o);
    const int rc = e ? SNMF_OK : b64_restart(o, S, all.data(), nullptr, Bd0, H0, Ad0);
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
    h.F = o->F; h.r = o->r; h.Rx = p.R_x; h.cost_check = p.cost_check; h.n = C * o->S; h.flr = kFlr64;  // (the rest: the stream's table entry)
    hipLaunchKernelGGL(k_obhsolve64, dim3(step >= 0 ? 1 : C, o->S), dim3(1024), b64_lds_solve(o), o->ctx->stream, h,
                       (const OStreamSettings*)o->set, fr, step);
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
    w.set = o->set; w.F = o->F; w.r = o->r; w.Rx = p.R_x; w.Ra = o->Ra; w.ma = o->ma; w.cost_check = p.cost_check; w.flr = kFlr64;
    const B64Needs nd = b64_needs(o->hset);
    // one launch per divergence class present among the adapting streams, each with its own LDS image
    auto launch = [&](auto kern, int kl) -> int {
        const size_t lds = wbatch64_lds(o->Ra, o->ma, kl);
        SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)kern, lds));
        hipLaunchKernelGGL(kern, dim3(o->S), dim3(kWb64NT), lds, st, w);
        HIP_TRY(hipGetLastError());
        return SNMF_OK;
    };
    if (nd.cls[kWb64KL]) SN_TRY(launch(k_wadapt_batch64<kWb64KL>, 1));
    if (nd.cls[kWb64ED]) SN_TRY(launch(k_wadapt_batch64<kWb64ED>, 0));
    if (nd.cls[kWb64GEN]) SN_TRY(launch(k_wadapt_batch64<kWb64GEN>, 0));
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
    const size_t lds_fft = obm_lds_fft(o);
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
    a.F = o->F; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.dcbin = p.dcbin;
    a.l = 1; a.flr = p.nonzerofloor;  // (the filter's and the trigger's settings: the stream's table entry, set by k_obpost64)
    a.recon_len = o->F; a.n = 1; a.a_stride = o->r;
    return SNMF_OK;
}

static int obm_post(OnlineBatchF64* o, const OBatchFrames& fr, int step) {
    hipLaunchKernelGGL(k_obpost64, dim3(o->S), dim3(1024), b64_lds_post(o), o->ctx->stream, o->post_a, (const OStreamSettings*)o->set, fr,
                       step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int online_batch_f64_process(OnlineBatchF64* o, const double* const* pcm, const int64_t* n, const int32_t* flush, double* const* xt,
                             int16_t* const* xt_i16, double* const* xh, double* const* dh, double* const* xhi, double* const* dhi,
                             const int64_t* cap, int64_t* n_out) {
    return obatch_process(o, pcm, n, flush, xt, xt_i16, xh, dh, xhi, dhi, cap, n_out);
}

int online_batch_f64_restart(OnlineBatchF64* o, int32_t n, const int32_t* slots, const double* Bx, const double* Bd, const double* H0,
                             const double* Ad, const snmf_online_stream_settings* settings) {
    SN_TRY(obatch_restart_check(o, n, slots));
    if (n == 0) return SNMF_OK;
    // the table as it would stand, checked before anything changes: a refused restart leaves the batch as it was
    std::vector<OStreamSettings> hs = o->hset;
    for (int i = 0; i < n && settings; ++i) hs[slots[i]] = b64_table_entry(settings[i], o->p.m_a);
    const B64Needs nd = b64_needs(hs);
    SN_TRY(b64_check_ring(o->ctx, o->p, nd));
    const bool grows = nd.adapt && (o->Ra != o->p.R_a || o->ma != o->p.m_a);  // (the rings as they are hold nobody's Ad_blk0)
    for (int i = 0; i < n; ++i)
        if (hs[slots[i]].adapt_train_N && !Ad && (grows || !o->has_ad0[slots[i]]))
            return fail(SNMF_ERR_INVALID, "stream %d adapts and was never given an Ad_blk0", slots[i]);
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    int rc = b64_fit_rings(o, nd);
    if (rc == SNMF_OK) {
        o->hset = hs;
        for (int i = 0; i < n && settings; ++i) o->uset[slots[i]] = settings[i];
        b64_publish_adapt(o);  // the driver's launch structure follows the table
        rc = b64_restart(o, n, slots, Bx, Bd, H0, Ad);
    }
    if (rc) {
        o->failed = true;  // some of the listed streams may be half reset
        return rc;
    }
    return SNMF_OK;
}

int online_batch_f64_get_settings(OnlineBatchF64* o, int32_t k, snmf_online_stream_settings* out) {
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    *out = o->uset[k];
    return SNMF_OK;
}

void online_batch_f64_dims(OnlineBatchF64* o, int* r, int* ra_ma) {
    *r = o->r;
    *ra_ma = o->Ra * o->ma;
}

int online_batch_f64_idle(const OnlineBatchF64* o) { return obatch_idle_check(o); }

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

// ---- get-state / set-state (the driver's section in snmf_online_batch_host.h; kernels k_obstate_get64 / k_obstate_put64) ----
static void obm_state_mode(const OnlineBatchF64*, int* mel, int* mel_conv, int* n1) { *mel = *mel_conv = *n1 = 0; }  // DFT mode only

static int obm_state_launch(OnlineBatchF64* o, const OStateArgs<double>& a, int n, bool put) {
    if (put) hipLaunchKernelGGL(k_obstate_put64, dim3(n, kStN, kStParts), dim3(256), 0, o->ctx->stream, a);
    else hipLaunchKernelGGL(k_obstate_get64, dim3(n, kStN, kStParts), dim3(256), 0, o->ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// Ad0 now holds the record's Ad_blk0 (a ring that grows later forgets it, as b64_fit_rings does for every stream)
static void obm_state_installed(OnlineBatchF64* o, int n, const int32_t* slots) {
    for (int i = 0; i < n; ++i) o->has_ad0[slots[i]] = 1;
}

void online_batch_f64_state_info(OnlineBatchF64* o, snmf_online_state_info* out) { obatch_state_info(o, out); }

int online_batch_f64_get_state(OnlineBatchF64* o, int32_t n, const int32_t* slots, void* records, int64_t cap) {
    return obatch_get_state(o, n, slots, records, cap);
}

int online_batch_f64_set_state(OnlineBatchF64* o, int32_t n, const int32_t* slots, const void* records, int64_t bytes) {
    return obatch_set_state(o, n, slots, records, bytes);
}
