// snmf_tu_online_batch.hip -- the batched online separator behind the C ABI (snmf_online_batch_*), kernels in
// snmf_online_batch.h.  A translation unit of its own, so that the single-stream kernels' code does not move.
// The host driver (hop queues, chunk loop, framing, synthesis, trace) is snmf_online_batch_host.h, shared with the fp64 mode;
// here are the handle, its creation / Mel conversion / restart, and the fp32 steps the driver calls (obm_*).
#include <new>

#include "snmf_internal.h"
#include "snmf_online_batch.h"
#include "snmf_online_batch_chains.h"
#include "snmf_online_batch_f64_host.h"  // the fp64 mode's host entry points (its kernels live in snmf_tu_online_batch_f64.hip)
#include "snmf_online_batch_host.h"
#include "snmf_online_classes.h"

struct snmf_online_batch : OBatchState<float> {
    OnlineBatchF64* f64 = nullptr;  // non-null: an fp64 batch (snmf_online_batch_create_f64); only ctx, p, S and F are then used
    bool per_stream = false;        // fp64 batch: streams were given settings or event dictionaries of their own
    int RA2 = 64;
    int Fs = 0;                                // rows of the solves: F, or F_order in Mel mode
    int mel = 0, mel_conv = 0, n1 = 0;         // B_sep_mode = 'Mel' (snmf_online_batch_set_mel)
    snmf_plan* hp = nullptr;  // the frame solve's geometry, sparsity and beta (one plan serves every stream)
    // per stream, device: the frame solve's images of the dictionary (k_obrefresh), k_wadapt_batch's result and scratch
    double *wn = nullptr, *Wu = nullptr;
    float *Wcf = nullptr, *wx = nullptr, *dphv = nullptr, *Hin = nullptr;
    float *G = nullptr, *P = nullptr, *Vt = nullptr;
    // Mel mode: melmat [n1][F] and B_Mel_x [Rx][n1] (fp64) shared; per stream the fp64 Mel master [r][n1], the adaptation's
    // melmat * lambda_d_blk [ma][n1] and, with MelConv = 0, the fp32 [B_DFT_x | B_DFT_d] [r][F]
    float *melmat = nullptr, *Vm = nullptr, *Bdf = nullptr;
    double *Bmx = nullptr, *Bm = nullptr, *rs_Bm = nullptr;  // (rs_Bm: the restart upload of B_Mel_d, sized for all S streams)
    // per chunk, device (obm_reserve): the solve's input, Mel features, activations, reconstructions (Fs rows), state and histories
    float *Vp = nullptr, *Ymel = nullptr, *Hout = nullptr, *reco = nullptr;
    DevState* st = nullptr;
    double *divh = nullptr, *costh = nullptr;
    // the post-filter's launch arguments of the current chunk (ob_post_args)
    OPostArgs post_a{};
    OBatchPost post_bp{};
    size_t post_lds = 0;
};

static void obm_free_chunk(snmf_online_batch* o) {
    void* ptrs[] = {o->Vp, o->Ymel, o->Hout, o->reco, o->st, o->divh, o->costh};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->Vp = o->Ymel = o->Hout = o->reco = nullptr;
    o->st = nullptr;
    o->divh = o->costh = nullptr;
}

static int obm_reserve(snmf_online_batch* o, size_t slots) {
    const snmf_plan* pl = o->hp;
    SN_TRY(dalloc(&o->Vp, (size_t)pl->Fp * slots));
    if (o->mel) SN_TRY(dalloc(&o->Ymel, (size_t)o->n1 * slots));
    SN_TRY(dalloc(&o->Hout, (size_t)pl->rp * slots));
    SN_TRY(dalloc(&o->reco, 2 * (size_t)o->Fs * slots));
    SN_TRY(dalloc(&o->st, slots));
    SN_TRY(dalloc(&o->divh, slots * o->p.max_iter));
    SN_TRY(dalloc(&o->costh, slots * o->p.max_iter));
    return SNMF_OK;
}

// as inherited: the slots bound the per-slot solve buffers; the class count does not enter, though Xc grows with it
static int obm_chunk_frames(const snmf_online_batch* o) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, kBChunkSlots / o->S)); }

extern "C" void snmf_online_batch_destroy(snmf_online_batch* o) {
    if (!o) return;
    if (o->f64) {
        online_batch_f64_destroy(o->f64);
        delete o;
        return;
    }
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
    if (o->hp) snmf_plan_destroy(o->hp);
    obatch_free_state(o);
    void* ptrs[] = {o->wn, o->Wu, o->Wcf, o->wx, o->dphv, o->Hin, o->G, o->P, o->Vt, o->melmat, o->Vm, o->Bdf, o->Bmx, o->Bm, o->rs_Bm};
    for (void* q : ptrs)
        if (q) hipFree(q);
    delete o;
}

// the single-stream separator's checks (snmf_tu_online.hip: online_validate) plus the batch's scope
static int ob_validate(const snmf_online_params* p, int32_t S) {
    if (!p) return fail(SNMF_ERR_INVALID, "online params is NULL");
    if (S < 1) return fail(SNMF_ERR_INVALID, "the batch needs at least one stream");
    const int N = p->fftlength;
    if (N < 64 || N > 4096 || (N & (N - 1))) return fail(SNMF_ERR_UNSUPPORTED, "fftlength must be a power of two in [64,4096]");
    if (p->framelength < 1 || p->framelength > N || p->frameshift < 1 || p->frameshift > p->framelength)
        return fail(SNMF_ERR_INVALID, "need 1 <= frameshift <= framelength <= fftlength");
    const int F = N / 2 + 1;
    if (p->dcbin < 0 || p->dcbin > F || p->dcbin_back < 0 || p->dcbin_back > F || p->delay < 0)
        return fail(SNMF_ERR_INVALID, "bad DCbin / DCbin_back / delay");
    if (p->R_x < 1 || p->R_d < 1) return fail(SNMF_ERR_INVALID, "R_x and R_d must be positive");
    if (p->max_iter < 1) return fail(SNMF_ERR_INVALID, "max_iter must be positive");
    if (p->enhance_method != 0 && p->enhance_method != 1) return fail(SNMF_ERR_INVALID, "enhance_method: 0 Wiener, 1 MMSE");
    if (p->blk_sparse) {
        if (p->blk_gap < 1 || p->blk_gap % 2 == 0) return fail(SNMF_ERR_INVALID, "blk_gap must be odd (src/blk_sparse.m:4)");
        if (p->P_len_k < 2 || p->P_len_k % 2 || p->P_len_l < 1) return fail(SNMF_ERR_INVALID, "P_len_k must be even and >= 2, P_len_l >= 1");
        if (p->P_len_k + p->dcbin > F) return fail(SNMF_ERR_INVALID, "P_len_k + DCbin exceeds the number of bins");
    }
    if (p->adapt_train_N) {
        if (p->R_a < 1 || p->R_a > p->R_d || p->m_a < 1) return fail(SNMF_ERR_INVALID, "need 1 <= R_a <= R_d and m_a >= 1");
        if (p->R_a > 128 || p->m_a > 128)
            return fail(SNMF_ERR_UNSUPPORTED, "batched adaptation: R_a and m_a must be <= 128 (k_wadapt_batch's lanes)");
    }
    if (p->basis_update_N || p->basis_update_E)
        return fail(SNMF_ERR_UNSUPPORTED, "batched separator: semi-supervised frame solves (basis_update_N / _E) are not supported");
    return SNMF_OK;
}

// Every column's dictionary images (set_w + the init mode of k_wapply) of the streams in rs_slots, from the solve's dictionary
// (Mel: the Mel master): the launch that ends a restart and follows a set-state (the driver's obm_state_refresh).
static int obm_state_refresh(snmf_online_batch* o, int n) {
    const snmf_online_params& p = o->p;
    ORefreshArgs ra{};
    ra.slots = o->rs_slots; ra.S = o->S; ra.B = o->mel ? o->Bm : o->B; ra.Wcf = o->Wcf; ra.wx = o->wx; ra.dphv = o->dphv; ra.wn = o->wn;
    ra.Hin = o->Hin; ra.H0 = o->H0; ra.lamk = o->hp->lamk; ra.F = o->Fs; ra.r = o->r; ra.Rx = p.R_x; ra.rp = o->hp->rp; ra.Fp = o->hp->Fp;
    ra.xr = o->Fs > 64 * o->hp->frame_fb; ra.k0 = 0;
    hipLaunchKernelGGL(k_obrefresh, dim3(o->r, n), dim3(256), 0, o->ctx->stream, ra);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// The streams slots[0..n) start a new recording (obatch_restart): the fp32 mode's own are the upload of the new B_Mel_d and,
// around the shared arguments, the frame solve's images and the Mel masters.  Arguments are checked by the caller; Bmd
// (Mel mode) is n x Rd x n1 fp64 or NULL (carry).
static int ob_restart(snmf_online_batch* o, int n, const int32_t* slots, const double* Bd, const double* Bmd, const float* H0,
                      const float* Ad) {
    hipStream_t st = o->ctx->stream;
    if (Bmd) HIP_TRY(hipMemcpyAsync(o->rs_Bm, Bmd, (size_t)n * o->p.R_d * o->n1 * 8, hipMemcpyHostToDevice, st));
    return obatch_restart(o, n, slots, Bd, H0, Ad, 0, [&](const ORestartCommon<float>& c) {
        ORestartArgs a{};
        a.c = c; a.Wcf = o->Wcf; a.wx = o->wx; a.dphv = o->dphv; a.Hin = o->Hin; a.wn = o->wn;
        a.Bmx = o->Bmx; a.Bmd = Bmd ? o->rs_Bm : nullptr; a.Bm = o->Bm; a.Bdf = o->Bdf;
        a.rp = o->hp->rp; a.Fp = o->hp->Fp; a.adapt = o->p.adapt_train_N; a.n1 = o->n1;
        hipLaunchKernelGGL(k_obrestart, dim3(n, kRsN, kRsParts), dim3(256), 0, st, a);
    });
}

// the frame solve's plan: rows x 1, rank r, H-only (its register-resident kernel must admit the shape)
static int ob_make_plan(snmf_ctx* ctx, const snmf_online_params* p, int rows, snmf_plan** out) {
    const int r = p->R_x + p->R_d;
    snmf_params hp{};
    hp.F = rows; hp.T = 1; hp.r = r; hp.beta = p->beta_div; hp.max_iter = p->max_iter; hp.conv_eps = p->conv_eps;
    hp.cost_check = p->cost_check; hp.floor_v = 1; hp.sparsity_kind = SNMF_SPARSITY_SCALAR; hp.sparsity_scalar = p->sparsity;
    std::vector<uint8_t> zeros(r, 0), ones(r, 1);
    hp.w_update_ind = zeros.data();
    hp.h_update_ind = ones.data();
    SN_TRY(snmf_plan_create(ctx, &hp, out));
    if (!(*out)->frame_fb)
        return fail(SNMF_ERR_UNSUPPORTED, "batched separator: F = %d, r = %d is outside the frame kernel's envelope (F <= 513, r <= 200)", rows, r);
    return SNMF_OK;
}

extern "C" int snmf_online_batch_create(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const float* Bx, const float* Bd0,
                                        const float* H0, const float* Ad0, const float* win_stft, const float* win_istft,
                                        snmf_online_batch** out) {
    if (!ctx || !out || !Bx || !Bd0 || !H0 || !win_stft || !win_istft) return fail(SNMF_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SN_TRY(ob_validate(p, S));
    if (p->adapt_train_N && !Ad0) return fail(SNMF_ERR_INVALID, "Ad_blk0 is required when adapt_train_N is set");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int N = p->fftlength, F = N / 2 + 1, r = p->R_x + p->R_d, sz = p->framelength, hop = p->frameshift, Rd = p->R_d;
    snmf_online_batch* o = new snmf_online_batch();
    o->ctx = ctx;
    o->p = *p;
    o->S = S;
    o->F = F;
    o->r = r;
    o->N = N;
    o->nov = (sz + hop - 1) / hop;
    o->Ra = p->adapt_train_N ? p->R_a : 1;
    o->ma = p->adapt_train_N ? p->m_a : 1;
    o->Pl = p->blk_sparse ? p->P_len_l : 1;
    o->RA2 = (o->Ra + 63) / 64 * 64;
    o->Fs = F;
    int s = SNMF_OK;
    auto A = [&](int v) { if (s == SNMF_OK) s = v; };
    A(ob_make_plan(ctx, p, F, &o->hp));
    if (s == SNMF_OK && p->adapt_train_N && wbatch_lds(o->Ra, o->ma, o->RA2, p->beta_div == 1.0) > ctx->lds_max)
        A(fail(SNMF_ERR_UNSUPPORTED, "batched adaptation: R_a x m_a too large for one workgroup's LDS"));
    if (s != SNMF_OK) {
        snmf_online_batch_destroy(o);
        return s;
    }
    const size_t SS = (size_t)S, rp = o->hp->rp, Fp = o->hp->Fp, Fb = (size_t)(F + kWbRB - 1) / kWbRB * kWbRB;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * sz;
    o->ntail = ntail;
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->B, SS * r * F); D(&o->Bfix, SS * Rd * F); D(&o->Btmp, SS * Rd * F); D(&o->wn, SS * rp);
    D(&o->Wcf, SS * rp * Fp); D(&o->wx, SS * rp); D(&o->dphv, SS * rp); D(&o->Hin, SS * rp); D(&o->H0, SS * r);
    D(&o->lambda_dav, SS * F); D(&o->Xm_tilde, SS * F); D(&o->r_blk, SS * F * o->Pl); D(&o->ldblk, SS * F * o->ma);
    D(&o->adblk, SS * o->Ra * o->ma); D(&o->Ad0, SS * o->Ra * o->ma); D(&o->rup, SS * o->Ra); D(&o->dev, SS); D(&o->tail, SS * ntail);
    if (p->class_outputs) {
        D(&o->tail_x, SS * ntail);
        D(&o->tail_d, SS * ntail);
    }
    if (p->adapt_train_N) {
        D(&o->Wu, SS * o->Ra * F); D(&o->G, SS * Fb * o->RA2); D(&o->Vt, SS * Fb * o->ma);
        if (p->beta_div != 1.0) D(&o->P, SS * Fb * o->RA2);
    }
    D(&o->win_s, (size_t)sz); D(&o->win_i, (size_t)sz); D(&o->tw, (size_t)N / 2); D(&o->Bxd, (size_t)F * p->R_x);
    D(&o->rs_slots, SS); D(&o->rs_B, SS * Rd * F); D(&o->rs_H, SS * r); D(&o->rs_A, SS * o->Ra * o->ma);
    D(&o->meta_i, 6 * SS); D(&o->meta_l, 3 * SS);
    if (s != SNMF_OK) {
        snmf_online_batch_destroy(o);
        return s == SNMF_ERR_NOMEM ? fail(SNMF_ERR_NOMEM, "batched separator: device memory for %d streams", S) : s;
    }
    std::vector<float2> htw(N / 2);
    for (int q = 0; q < N / 2; ++q) {
        const double ang = -2.0 * M_PI * (double)q / (double)N;
        htw[q] = make_float2((float)cos(ang), (float)sin(ang));
    }
    std::vector<double> hx((size_t)F * p->R_x), hd(SS * Rd * F);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = (double)Bx[i];
    for (size_t i = 0; i < hd.size(); ++i) hd[i] = (double)Bd0[i];
    int e = 0;
    auto H = [&](hipError_t x) { if (x != hipSuccess && !e) e = (int)x; };
    H(hipMemcpyAsync(o->win_s, win_stft, (size_t)sz * 4, hipMemcpyHostToDevice, st));
    H(hipMemcpyAsync(o->win_i, win_istft, (size_t)sz * 4, hipMemcpyHostToDevice, st));
    H(hipMemcpyAsync(o->tw, htw.data(), htw.size() * 8, hipMemcpyHostToDevice, st));
    H(hipMemcpyAsync(o->Bxd, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, st));
    o->pending.assign(SS, {});
    o->hist.assign(SS, {});
    o->l.assign(SS, 0);
    o->finished.assign(SS, 0);
    o->trace.resize(SS);
    // every stream's state g: a restart of all S streams (the one initialisation path)
    std::vector<int32_t> all(SS);
    for (int k = 0; k < S; ++k) all[k] = k;
    const int rc = e ? SNMF_OK : ob_restart(o, S, all.data(), hd.data(), nullptr, H0, p->adapt_train_N ? Ad0 : nullptr);
    H(hipStreamSynchronize(st));
    if (e || rc) {
        snmf_online_batch_destroy(o);
        if (!e) return rc;
        return fail(e == (int)hipErrorOutOfMemory ? SNMF_ERR_NOMEM : SNMF_ERR_NO_DEVICE, "online batch create: %s",
                    hipGetErrorString((hipError_t)e));
    }
    *out = o;
    return SNMF_OK;
}

// B_sep_mode = 'Mel' (src/bnmf_sep_event_RT_IS16.m:106-120, src/init_buff.m:45-47), as snmf_online_set_mel: the frame solve
// is rebuilt at F_order rows and every stream restarts through ob_restart with the given B_Mel_d (its B_DFT_d, H0 and
// Ad_blk0 are kept).
extern "C" int snmf_online_batch_set_mel(snmf_online_batch* o, int32_t F_order, int32_t mel_conv, const float* melmat, const float* BMx,
                                         const float* BMd) {
    if (!o || !melmat || !BMx || !BMd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) return fail(SNMF_ERR_UNSUPPORTED, "fp64 batched separator: B_sep_mode 'Mel' is not supported");
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    if (o->started) return fail(SNMF_ERR_STATE, "snmf_online_batch_set_mel must precede the first process call");
    if (F_order < 2 || F_order > o->F) return fail(SNMF_ERR_INVALID, "F_order must be in [2, fftlength/2+1]");
    if (mel_conv && (size_t)o->n_cls * F_order * 4 > o->ctx->lds_max)
        return fail(SNMF_ERR_UNSUPPORTED, "MelConv = 1 with %d classes at F_order = %d: the class kernel's Mel products do not fit the LDS", o->n_cls, F_order);
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    const snmf_online_params& p = o->p;
    const int n1 = F_order, S = o->S, r = o->r, F = o->F, Rx = p.R_x, Rd = p.R_d;
    snmf_plan* hp = nullptr;
    if (int rc = ob_make_plan(o->ctx, &p, n1, &hp)) {
        if (hp) snmf_plan_destroy(hp);
        return rc;
    }
    // from here on a failure leaves the batch half converted
    o->failed = true;
    snmf_plan_destroy(o->hp);
    o->hp = hp;
    obatch_free_chunk(o);  // Vp / Ymel / reco depend on the solve's rows
    for (void** q : {(void**)&o->Wcf, (void**)&o->melmat, (void**)&o->Vm, (void**)&o->Bdf, (void**)&o->Bmx, (void**)&o->Bm, (void**)&o->rs_Bm}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    const size_t SS = (size_t)S;
    SN_TRY(dalloc(&o->Wcf, SS * hp->rp * hp->Fp));
    SN_TRY(dalloc(&o->melmat, (size_t)n1 * F));
    SN_TRY(dalloc(&o->Bmx, (size_t)n1 * Rx));
    SN_TRY(dalloc(&o->Bm, SS * r * n1));
    SN_TRY(dalloc(&o->rs_Bm, SS * Rd * n1));
    if (p.adapt_train_N) SN_TRY(dalloc(&o->Vm, SS * o->ma * n1));
    if (!mel_conv) SN_TRY(dalloc(&o->Bdf, SS * r * F));
    std::vector<double> hx((size_t)n1 * Rx), hd(SS * Rd * n1);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = (double)BMx[i];
    for (size_t i = 0; i < hd.size(); ++i) hd[i] = (double)BMd[i];
    HIP_TRY(hipMemcpyAsync(o->melmat, melmat, (size_t)n1 * F * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->Bmx, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, st));
    o->mel = 1;
    o->mel_conv = mel_conv != 0;
    o->n1 = n1;
    o->Fs = n1;
    std::vector<int32_t> all(SS);
    for (int k = 0; k < S; ++k) all[k] = k;
    SN_TRY(ob_restart(o, S, all.data(), nullptr, hd.data(), nullptr, nullptr));
    HIP_TRY(hipStreamSynchronize(st));
    o->failed = false;
    return SNMF_OK;
}

/* snmf_online_set_classes for the batch: one partition for all streams (src/bnmf_sep_event_RT_IS16.m:158-202, :350-361). */
extern "C" int snmf_online_batch_set_classes(snmf_online_batch* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num,
                                             const int32_t* noise_rank) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) return online_batch_f64_set_classes(o->f64, event_num, event_rank, noise_num, noise_rank);
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    if (!o->p.class_outputs) return fail(SNMF_ERR_STATE, "class outputs were not requested at creation");
    if (o->started) return fail(SNMF_ERR_STATE, "snmf_online_batch_set_classes must precede the first process call");
    std::vector<int> cls;
    SN_TRY(online_class_ranges(event_num, event_rank, noise_num, noise_rank, o->p.R_x, o->p.R_d, &cls));
    const int nc = event_num + noise_num;
    if (o->mel && o->mel_conv && (size_t)nc * o->n1 * 4 > o->ctx->lds_max)
        return fail(SNMF_ERR_UNSUPPORTED, "MelConv = 1 with %d classes at F_order = %d: the class kernel's Mel products do not fit the LDS", nc, o->n1);
    return obatch_install_classes(o, cls, event_num, nc);
}

// the frame solves of frame `step` of every stream (step < 0: all C frames of the chunk; slots [first * S, (first + nf) * S)),
// one workgroup per (frame, stream)
static int obm_frame_solve(snmf_online_batch* o, const OBatchFrames&, int step, int C) {
    snmf_plan* pl = o->hp;
    const int first = step < 0 ? 0 : step, nf = step < 0 ? C : 1;
    const size_t off = (size_t)first * o->S;
    StepArgs a = make_args(pl);
    a.V = o->Vp + off * pl->Fp;
    a.Hin = o->Hin;
    a.Hout = o->Hout + off * pl->rp;
    a.n_tiles = 1;
    a.wx = o->wx;
    a.dphv = o->dphv;
    a.S = nullptr;
    SmallArgs sa{};
    sa.max_iter = pl->p.max_iter;
    sa.cost_check = pl->p.cost_check;
    sa.conv_eps = pl->p.conv_eps;
    sa.divh = o->divh + off * pl->p.max_iter;
    sa.costh = o->costh + off * pl->p.max_iter;
    sa.st = o->st + off;
    sa.tps = 1;
    sa.recon = o->reco + off * 2 * o->Fs;  // (Mel without MelConv leaves them unread: k_obpost forms B_DFT * A)
    sa.wn = o->wn;
    sa.Rx = o->p.R_x;
    const bool obj = pl->p.cost_check != 0;
    auto launch = [&](auto kern) -> int {
        SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)kern, pl->lds_frame));
        hipLaunchKernelGGL(kern, dim3(nf, o->S), dim3(512), pl->lds_frame, o->ctx->stream, a, sa, (const float*)o->Wcf);
        HIP_TRY(hipGetLastError());
        return SNMF_OK;
    };
    auto by_bm = [&](auto fbc, auto kbc) -> int {
        constexpr int FB = decltype(fbc)::value, KB = decltype(kbc)::value;
        auto by_obj = [&](auto bmc) -> int {
            constexpr int BM = decltype(bmc)::value;
            return obj ? launch(k_hsolve_frame<FB, KB, BM, true, true, true>) : launch(k_hsolve_frame<FB, KB, BM, false, true, true>);
        };
        if (pl->bm == BM_KL) return by_obj(std::integral_constant<int, BM_KL>{});
        if (pl->bm == BM_EUC) return by_obj(std::integral_constant<int, BM_EUC>{});
        return by_obj(std::integral_constant<int, BM_GEN>{});
    };
    using I4 = std::integral_constant<int, 4>;
    using I8 = std::integral_constant<int, 8>;
    using I16 = std::integral_constant<int, 16>;
    using I25 = std::integral_constant<int, 25>;
    if (pl->frame_fb == 4) return pl->frame_kb == 16 ? by_bm(I4{}, I16{}) : by_bm(I4{}, I25{});
    return pl->frame_kb == 16 ? by_bm(I8{}, I16{}) : by_bm(I8{}, I25{});
}

// the class spectra (:158-202) of frame `step` of every stream (step < 0: all C frames of the chunk): behind the frame solves,
// before the adaptation replaces the dictionaries (k_obclass)
static int obm_class_spectra(snmf_online_batch* o, const OBatchFrames& fr, int step, int C) {
    const bool mc = o->mel && o->mel_conv;
    OBatchClassArgs c{};
    c.B = mc ? o->Bm : o->B; c.A = o->Hout; c.cls = o->cls; c.melmat = o->melmat; c.out = o->Xc;
    c.cstride = (int64_t)o->C * o->S * o->F; c.n_cls = o->n_cls; c.F = o->F; c.n1 = o->n1; c.mel_conv = mc; c.rp = o->hp->rp; c.r = o->r;
    const size_t lds = mc ? (size_t)o->n_cls * o->n1 * 4 : 0;
    if (lds) SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_obclass, lds));
    hipLaunchKernelGGL(k_obclass, dim3((o->F + 255) / 256, o->S, step >= 0 ? 1 : C), dim3(256), lds, o->ctx->stream, c, fr, step);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// adaptation (gated on the device) + re-assembly + dictionary refresh after frame `step` of every stream
static int obm_adapt(snmf_online_batch* o, const OBatchFrames& fr, int step) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    snmf_plan* pl = o->hp;
    const StepArgs sa = make_args(pl);
    // DFT mode adapts B_DFT_d on lambda_d_blk (:320-338); Mel mode adapts the Mel master's B_Mel_d on melmat * lambda_d_blk
    // (:298-318), whose fixed columns are its own (:309)
    double* Bs = o->mel ? o->Bm : o->B;
    if (o->mel) {
        hipLaunchKernelGGL(k_obprep_mel, dim3(o->ma, o->S), dim3(256), 0, st, (const OnlineStatus*)o->status, fr.nfr, step, o->S,
                           (const float*)o->ldblk, (const float*)o->melmat, o->F, o->n1, o->ma, o->Vm);
        HIP_TRY(hipGetLastError());
    }
    WBatchArgs w{};
    w.status = o->status; w.nfr = fr.nfr; w.step = step; w.S = o->S; w.ldblk = o->mel ? o->Vm : o->ldblk; w.adblk = o->adblk;
    w.rup = o->rup; w.dev = o->dev; w.B = Bs; w.Wu = o->Wu; w.G = o->G; w.P = o->P; w.Vt = o->Vt; w.iters = o->iters;
    w.F = o->Fs; w.r = o->r; w.Rx = p.R_x; w.Ra = o->Ra; w.ma = o->ma; w.max_iter = p.max_iter; w.cost_check = p.cost_check;
    w.RA2 = o->RA2; w.sparsity = (float)p.sparsity; w.flr = kFlr; w.beta = sa.beta; w.inv_bb1 = sa.inv_bb1; w.conv_eps = p.conv_eps;
    const size_t lds = wbatch_lds(o->Ra, o->ma, o->RA2, pl->bm == BM_KL);
    auto launch = [&](auto kern) -> int {
        SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)kern, lds));
        hipLaunchKernelGGL(kern, dim3(o->S), dim3(kWbNT), lds, st, w);
        HIP_TRY(hipGetLastError());
        return SNMF_OK;
    };
    if (pl->bm == BM_KL) SN_TRY(launch(k_wadapt_batch<BM_KL>));
    else if (pl->bm == BM_EUC) SN_TRY(launch(k_wadapt_batch<BM_EUC>));
    else SN_TRY(launch(k_wadapt_batch<BM_GEN>));
    const double* Bfix = o->mel ? o->Bm + (size_t)p.R_x * o->n1 : o->Bfix;
    const int64_t sfix = o->mel ? (int64_t)o->r * o->n1 : (int64_t)p.R_d * o->F;
    hipLaunchKernelGGL(k_obassemble, dim3(p.R_d, o->S), dim3(256), 0, st, (const OnlineStatus*)o->status, fr.nfr, step, o->S,
                       (const double*)Bs, (const double*)o->Wu, Bfix, sfix, (const uint8_t*)o->rup, o->Fs, o->r, p.R_x, o->Ra, p.R_d,
                       o->Btmp);
    HIP_TRY(hipGetLastError());
    ORefreshArgs ra{};
    ra.status = o->status; ra.nfr = fr.nfr; ra.step = step; ra.S = o->S; ra.Btmp = o->Btmp; ra.B = Bs; ra.Wcf = o->Wcf;
    ra.wx = o->wx; ra.dphv = o->dphv; ra.wn = o->wn; ra.Hin = o->Hin; ra.H0 = o->H0; ra.lamk = pl->lamk; ra.F = o->Fs; ra.r = o->r;
    ra.Rx = p.R_x; ra.rp = pl->rp; ra.Fp = pl->Fp; ra.xr = o->Fs > 64 * pl->frame_fb; ra.k0 = p.R_x;
    hipLaunchKernelGGL(k_obrefresh, dim3(p.R_d, o->S), dim3(256), 0, st, ra);  // next frame's init_w (:140-146)
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static void ob_post_args(snmf_online_batch* o);

// STFT of every frame of the chunk (in Mel mode the solve input is the Mel features, :106-120), and the chunk's post-filter arguments
static int obm_begin_chunk(snmf_online_batch* o, const OBatchFrames& fr, int C) {
    const snmf_online_params& p = o->p;
    const int S = o->S, F = o->F;
    hipStream_t st = o->ctx->stream;
    OStftArgs sa{};
    sa.sig = o->sig; sa.sz = p.framelength; sa.hop = p.frameshift; sa.dcbin = p.dcbin; sa.preemph = (float)p.preemph; sa.win = o->win_s;
    sa.tw = o->tw; sa.powv = (float)p.pow; sa.floorv = (float)p.nonzerofloor; sa.Ym = o->Ym; sa.Yph = o->Yph; sa.ld = F; sa.n_frames = C;
    if (!o->mel) {
        by_logn([&](auto L) { hipLaunchKernelGGL(k_obstft<decltype(L)::value>, dim3(C, S), dim3(256), 0, st, sa, fr, o->Vp, o->hp->Fp); }, o->N);
        HIP_TRY(hipGetLastError());
    } else {
        by_logn([&](auto L) { hipLaunchKernelGGL((k_obstft<decltype(L)::value, false>), dim3(C, S), dim3(256), 0, st, sa, fr, o->Vp, o->hp->Fp); },
                   o->N);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_obmel, dim3(C, S), dim3(256), (size_t)o->n1 * 4, st, (const float*)o->Ym, (const float*)o->melmat, fr.nfr, S, F,
                           o->n1, o->Ymel, o->Vp, o->hp->Fp);
        HIP_TRY(hipGetLastError());
    }
    ob_post_args(o);
    return SNMF_OK;
}

// post-filter arguments of a chunk (stream 0's pointers; k_obpost re-bases them)
static void ob_post_args(snmf_online_batch* o) {
    const snmf_online_params& p = o->p;
    const int F = o->F;
    OPostArgs& a = o->post_a;
    a.A = o->Hout; a.hst = o->st; a.B = nullptr; a.recon = o->reco; a.Ym = o->Ym; a.lambda_dav = o->lambda_dav; a.Xm_tilde = o->Xm_tilde;
    a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk; a.rup = o->rup; a.dev = o->dev; a.status = o->status;
    a.Xt_out = o->Xt; a.Xh_out = o->Xh; a.Dh_out = o->Dh;
    a.F = F; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.Pk = p.P_len_k; a.dcbin = p.dcbin; a.gap = p.blk_gap;
    a.l = 1; a.blk_sparse = p.blk_sparse; a.adapt = p.adapt_train_N; a.wiener = p.enhance_method == 0; a.init_N_len = p.init_N_len;
    a.switch_at = (int)std::floor(p.overlap_m_a * p.m_a);
    a.alpha_p = (float)p.alpha_p; a.alpha_eta = (float)p.alpha_eta; a.alpha_d = (float)p.alpha_d; a.beta0 = (float)p.beta;
    a.beta_max = (float)p.beta_max; a.Ar_up = (float)p.Ar_up; a.flr = (float)p.nonzerofloor;
    a.mel = o->mel; a.mel_conv = o->mel_conv; a.n1 = o->n1; a.melmat = o->melmat; a.Ymel = o->mel ? o->Ymel : nullptr; a.Bmf = nullptr;
    a.recon_len = o->Fs; a.n = 1; a.a_stride = 0;
    OBatchPost& bp = o->post_bp;
    bp.rp = o->hp->rp; bp.sB = 0;
    if (o->mel && !o->mel_conv) {  // coupled dictionaries: the Mel activations on the stream's DFT bases (:158-202)
        a.recon = nullptr;
        a.B = o->Bdf;
        bp.sB = (int64_t)o->r * F;
    }
    o->post_lds = (size_t)(o->r + 7 * F + 3 * o->n1) * 4;
}

static int obm_post(snmf_online_batch* o, const OBatchFrames& fr, int step) {
    OBatchPost bp = o->post_bp;
    bp.fr = fr;
    bp.step = step;
    hipLaunchKernelGGL(k_obpost, dim3(o->S), dim3(1024), o->post_lds, o->ctx->stream, o->post_a, bp);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static size_t obm_lds_fft(const snmf_online_batch*) { return 0; }  // k_obistft<LOGN, float>'s FFT buffers are static LDS

// snmf_online_batch_process_f32 / snmf_online_batch_process_classes_f32 (xhi_f32 / dhi_f32: the class signals, class-major at cap[s])
static int ob_process(snmf_online_batch* o, const float* const* pcm, const int64_t* n, const int32_t* flush, float* const* xt_f32,
                      int16_t* const* xt_i16, float* const* xh_f32, float* const* dh_f32, float* const* xhi_f32, float* const* dhi_f32,
                      const int64_t* cap, int64_t* n_out) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) {  // (the order of obatch_process's first checks)
        if (!n || !pcm) return fail(SNMF_ERR_INVALID, "pcm / n is NULL");
        if (n_out)
            for (int s = 0; s < o->S; ++s) n_out[s] = 0;
        return fail(SNMF_ERR_STATE, "snmf_online_batch_process_f32 on an fp64 batch: use snmf_online_batch_process_f64");
    }
    return obatch_process(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, xhi_f32, dhi_f32, cap, n_out);
}

extern "C" int snmf_online_batch_process_f32(snmf_online_batch* o, const float* const* pcm, const int64_t* n, const int32_t* flush,
                                             float* const* xt_f32, int16_t* const* xt_i16, float* const* xh_f32, float* const* dh_f32,
                                             const int64_t* cap, int64_t* n_out) {
    return ob_process(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, nullptr, nullptr, cap, n_out);
}

extern "C" int snmf_online_batch_process_classes_f32(snmf_online_batch* o, const float* const* pcm, const int64_t* n, const int32_t* flush,
                                                     float* const* xt_f32, int16_t* const* xt_i16, float* const* xh_f32,
                                                     float* const* dh_f32, float* const* xhi_f32, float* const* dhi_f32,
                                                     const int64_t* cap, int64_t* n_out) {
    return ob_process(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, xhi_f32, dhi_f32, cap, n_out);
}

extern "C" int snmf_online_batch_get_basis_f32(snmf_online_batch* o, int32_t k, float* Bd, int64_t ld) {
    if (!o || !Bd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    if (ld < o->F) return fail(SNMF_ERR_INVALID, "ld < F");
    const size_t F = o->F, Rd = o->p.R_d;
    std::vector<double> h(F * Rd);
    if (o->f64) {  // the fp64 dictionary, rounded
        SN_TRY(online_batch_f64_get_basis(o->f64, k, h.data(), (int64_t)F));
    } else {
        HIP_TRY(hipSetDevice(o->ctx->device));
        HIP_TRY(hipStreamSynchronize(o->ctx->stream));
        HIP_TRY(hipMemcpy(h.data(), o->B + (size_t)k * o->r * F + (size_t)o->p.R_x * F, h.size() * 8, hipMemcpyDeviceToHost));
    }
    for (size_t j = 0; j < Rd; ++j)
        for (size_t f = 0; f < F; ++f) Bd[j * ld + f] = (float)h[j * F + f];  // the single-stream separator's fp32 mirror
    return SNMF_OK;
}

extern "C" int snmf_online_batch_get_basis_f64(snmf_online_batch* o, int32_t k, double* Bd, int64_t ld) {
    if (!o || !Bd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) return online_batch_f64_get_basis(o->f64, k, Bd, ld);
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    if (ld < o->F) return fail(SNMF_ERR_INVALID, "ld < F");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    const size_t F = o->F, Rd = o->p.R_d;
    std::vector<double> h(F * Rd);
    HIP_TRY(hipMemcpy(h.data(), o->B + (size_t)k * o->r * F + (size_t)o->p.R_x * F, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < Rd; ++j) std::copy_n(h.data() + j * F, F, Bd + j * ld);  // the fp64 master, as a carry keeps it
    return SNMF_OK;
}

static int ob_restart_checked(snmf_online_batch* o, int32_t n, const int32_t* slots, const double* Bd, const double* Bmd, const float* H0,
                              const float* Ad) {
    SN_TRY(obatch_restart_check(o, n, slots));
    if (n == 0) return SNMF_OK;
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    if (int rc = ob_restart(o, n, slots, Bd, Bmd, H0, o->p.adapt_train_N ? Ad : nullptr)) {
        o->failed = true;  // some of the listed streams may be half reset
        return rc;
    }
    return SNMF_OK;
}

extern "C" int snmf_online_batch_restart(snmf_online_batch* o, int32_t n, const int32_t* slots, const double* Bd, const float* H0,
                                         const float* Ad) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) {  // H0 / Ad_blk0 widened; snmf_online_batch_restart_f64 takes them in fp64
        if (n < 0 || n > o->S) return fail(SNMF_ERR_INVALID, "restart of %d streams in a batch of %d", n, o->S);  // (before H0 / Ad_blk0 are read)
        int r = 0, na = 0;
        online_batch_f64_dims(o->f64, &r, &na);
        const size_t m = (size_t)n;
        std::vector<double> h(H0 ? H0 : nullptr, H0 ? H0 + m * r : nullptr), a(Ad ? Ad : nullptr, Ad ? Ad + m * na : nullptr);
        return online_batch_f64_restart(o->f64, n, slots, nullptr, Bd, H0 ? h.data() : nullptr, Ad ? a.data() : nullptr, nullptr);
    }
    return ob_restart_checked(o, n, slots, Bd, nullptr, H0, Ad);  // Mel mode: B_Mel_d carried
}

extern "C" int snmf_online_batch_restart_mel(snmf_online_batch* o, int32_t n, const int32_t* slots, const double* Bd, const double* Bmd,
                                             const float* H0, const float* Ad) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) return fail(SNMF_ERR_UNSUPPORTED, "fp64 batched separator: B_sep_mode 'Mel' is not supported");
    if (Bmd && !o->mel) return fail(SNMF_ERR_STATE, "B_Mel_d given to a batch that is not in Mel mode");
    return ob_restart_checked(o, n, slots, Bd, Bmd, H0, Ad);
}

// stream k's B_Mel_d (the fp64 master), n1 x Rd
static int ob_mel_basis(snmf_online_batch* o, int32_t k, int64_t ld, std::vector<double>& h) {
    if (o->f64) return fail(SNMF_ERR_UNSUPPORTED, "fp64 batched separator: B_sep_mode 'Mel' is not supported");
    if (!o->mel) return fail(SNMF_ERR_STATE, "not in Mel mode");
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    if (ld < o->n1) return fail(SNMF_ERR_INVALID, "ld < F_order");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    const size_t n1 = o->n1;
    h.resize(n1 * o->p.R_d);
    HIP_TRY(hipMemcpy(h.data(), o->Bm + (size_t)k * o->r * n1 + (size_t)o->p.R_x * n1, h.size() * 8, hipMemcpyDeviceToHost));
    return SNMF_OK;
}

extern "C" int snmf_online_batch_get_mel_basis_f32(snmf_online_batch* o, int32_t k, float* BMd, int64_t ld) {
    if (!o || !BMd) return fail(SNMF_ERR_INVALID, "NULL argument");
    std::vector<double> h;
    SN_TRY(ob_mel_basis(o, k, ld, h));
    const size_t n1 = o->n1;
    for (size_t j = 0; j < (size_t)o->p.R_d; ++j)
        for (size_t m = 0; m < n1; ++m) BMd[j * ld + m] = (float)h[j * n1 + m];  // the single-stream separator's fp32 mirror
    return SNMF_OK;
}

extern "C" int snmf_online_batch_get_mel_basis_f64(snmf_online_batch* o, int32_t k, double* BMd, int64_t ld) {
    if (!o || !BMd) return fail(SNMF_ERR_INVALID, "NULL argument");
    std::vector<double> h;
    SN_TRY(ob_mel_basis(o, k, ld, h));
    const size_t n1 = o->n1;
    for (size_t j = 0; j < (size_t)o->p.R_d; ++j) std::copy_n(h.data() + j * n1, n1, BMd + j * ld);  // what a carry keeps
    return SNMF_OK;
}

extern "C" int snmf_online_batch_trace(snmf_online_batch* o, int32_t k, snmf_online_frame* out, int64_t cap, int64_t* n) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) return online_batch_f64_trace(o->f64, k, out, cap, n);
    return obatch_trace(o, k, out, cap, n);
}

// ---- get-state / set-state (the driver's section in snmf_online_batch_host.h; kernels k_obstate_get / k_obstate_put) ----
static void obm_state_mode(const snmf_online_batch* o, int* mel, int* mel_conv, int* n1) {
    *mel = o->mel;
    *mel_conv = o->mel_conv;
    *n1 = o->n1;
}

// the record's B_Mel_d and the fp32 image of its B_DFT_d go to the Mel masters
static int obm_state_launch(snmf_online_batch* o, const OStateArgs<float>& a0, int n, bool put) {
    OStateArgs<float> a = a0;
    a.Bm = o->mel ? o->Bm : nullptr;
    a.Bdf = o->Bdf;  // (allocated only in Mel mode with MelConv = 0)
    a.n1 = o->n1;
    if (put) hipLaunchKernelGGL(k_obstate_put, dim3(n, kStN, kStParts), dim3(256), 0, o->ctx->stream, a);
    else hipLaunchKernelGGL(k_obstate_get, dim3(n, kStN, kStParts), dim3(256), 0, o->ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static void obm_state_installed(snmf_online_batch*, int, const int32_t*) {}

extern "C" int snmf_online_state_field(const snmf_online_state_info* info, int32_t field, int64_t* offset, int64_t* count, int32_t* type) {
    if (!info) return fail(SNMF_ERR_INVALID, "info is NULL");
    if (field < 0 || field >= SNMF_STATE_FIELD_COUNT) return fail(SNMF_ERR_INVALID, "no state field %d", field);
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    if (ostate_layout(*info, off, cnt, typ) < 0) return fail(SNMF_ERR_INVALID, "not the state info of a batch");
    if (offset) *offset = off[field];
    if (count) *count = cnt[field];
    if (type) *type = typ[field];
    return SNMF_OK;
}

extern "C" int snmf_online_batch_state_info(snmf_online_batch* o, snmf_online_state_info* out) {
    if (!o || !out) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) online_batch_f64_state_info(o->f64, out);
    else obatch_state_info(o, out);
    return SNMF_OK;
}

extern "C" int snmf_online_batch_get_state(snmf_online_batch* o, int32_t n, const int32_t* slots, void* records, int64_t cap) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) return online_batch_f64_get_state(o->f64, n, slots, records, cap);
    return obatch_get_state(o, n, slots, records, cap);
}

extern "C" int snmf_online_batch_set_state(snmf_online_batch* o, int32_t n, const int32_t* slots, const void* records, int64_t bytes) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (o->f64) return online_batch_f64_set_state(o->f64, n, slots, records, bytes);
    return obatch_set_state(o, n, slots, records, bytes);
}

// ---- fp64 mode (snmf_online_batch_f64.h): every input crosses in fp64 and every step from PCM to the fed-back state is fp64 ----
// the handle around a created fp64 batch
static int ob_wrap_f64(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, OnlineBatchF64* f, snmf_online_batch** out) {
    snmf_online_batch* o = new snmf_online_batch();
    o->ctx = ctx;
    o->f64 = f;
    o->p = *p;
    o->S = S;
    o->F = p->fftlength / 2 + 1;
    *out = o;
    return SNMF_OK;
}

extern "C" int snmf_online_batch_create_f64(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* Bx, const double* Bd0,
                                            const double* H0, const double* Ad0, const double* win_stft, const double* win_istft,
                                            snmf_online_batch** out) {
    if (!ctx || !out || !Bx || !Bd0 || !H0 || !win_stft || !win_istft) return fail(SNMF_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SN_TRY(ob_validate(p, S));  // (refuses basis_update_N / _E)
    if (p->adapt_train_N && !Ad0) return fail(SNMF_ERR_INVALID, "Ad_blk0 is required when adapt_train_N is set");
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    OnlineBatchF64* f = nullptr;
    SN_TRY(online_batch_f64_create(ctx, p, S, Bx, 0, Bd0, H0, Ad0, nullptr, win_stft, win_istft, &f));
    return ob_wrap_f64(ctx, p, S, f, out);
}

// `p` with one stream's settings in the place of its own: what ob_validate checks for that stream
static snmf_online_params ob_with_settings(const snmf_online_params& p, const snmf_online_stream_settings& q) {
    snmf_online_params m = p;
    m.beta_div = q.beta_div; m.sparsity = q.sparsity; m.conv_eps = q.conv_eps; m.max_iter = q.max_iter;
    m.enhance_method = q.enhance_method; m.init_N_len = q.init_N_len;
    m.alpha_eta = q.alpha_eta; m.alpha_d = q.alpha_d; m.beta = q.beta; m.beta_max = q.beta_max;
    m.blk_sparse = q.blk_sparse; m.P_len_k = q.P_len_k; m.blk_gap = q.blk_gap; m.alpha_p = q.alpha_p;
    m.adapt_train_N = q.adapt_train_N; m.overlap_m_a = q.overlap_m_a; m.Ar_up = q.Ar_up;
    return m;
}

extern "C" int snmf_online_batch_create_streams_f64(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* Bx, const double* Bd0,
                                                    const double* H0, const double* Ad0, const snmf_online_stream_settings* settings,
                                                    const double* win_stft, const double* win_istft, snmf_online_batch** out) {
    if (!ctx || !out || !Bx || !Bd0 || !H0 || !win_stft || !win_istft) return fail(SNMF_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SN_TRY(ob_validate(p, S));
    bool adapts = settings ? false : p->adapt_train_N != 0;
    for (int k = 0; k < S && settings; ++k) {  // every stream's settings on the shared geometry
        const snmf_online_params m = ob_with_settings(*p, settings[k]);
        SN_TRY(ob_validate(&m, S));
        adapts |= m.adapt_train_N != 0;
    }
    if (adapts && !Ad0) return fail(SNMF_ERR_INVALID, "Ad_blk0 is required when adapt_train_N is set");
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    OnlineBatchF64* f = nullptr;
    SN_TRY(online_batch_f64_create(ctx, p, S, Bx, 1, Bd0, H0, Ad0, settings, win_stft, win_istft, &f));
    SN_TRY(ob_wrap_f64(ctx, p, S, f, out));
    (*out)->per_stream = true;
    return SNMF_OK;
}

extern "C" int snmf_online_batch_restart_streams_f64(snmf_online_batch* o, int32_t n, const int32_t* slots, const double* Bx, const double* Bd,
                                                     const double* H0, const double* Ad, const snmf_online_stream_settings* settings) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (!o->f64) return fail(SNMF_ERR_STATE, "snmf_online_batch_restart_streams_f64 needs a batch made by snmf_online_batch_create_f64 / _create_streams_f64");
    if (n < 0 || n > o->S) return fail(SNMF_ERR_INVALID, "restart of %d streams in a batch of %d", n, o->S);  // (before settings are read)
    for (int i = 0; i < n && settings; ++i) {
        const snmf_online_params m = ob_with_settings(o->p, settings[i]);
        SN_TRY(ob_validate(&m, o->S));
    }
    SN_TRY(online_batch_f64_restart(o->f64, n, slots, Bx, Bd, H0, Ad, settings));
    if (n > 0 && (Bx || settings)) o->per_stream = true;
    return SNMF_OK;
}

extern "C" int snmf_online_batch_get_settings(snmf_online_batch* o, int32_t k, snmf_online_stream_settings* out) {
    if (!o || !out) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (!o->f64) return fail(SNMF_ERR_STATE, "snmf_online_batch_get_settings needs a batch made by snmf_online_batch_create_f64 / _create_streams_f64");
    return online_batch_f64_get_settings(o->f64, k, out);
}

static int ob_process_f64(snmf_online_batch* o, const double* const* pcm, const int64_t* n, const int32_t* flush, double* const* xt,
                          int16_t* const* xt_i16, double* const* xh, double* const* dh, double* const* xhi, double* const* dhi,
                          const int64_t* cap, int64_t* n_out) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (!o->f64) {
        if (n_out)
            for (int s = 0; s < o->S; ++s) n_out[s] = 0;
        return fail(SNMF_ERR_STATE, "snmf_online_batch_process_f64 needs a batch made by snmf_online_batch_create_f64");
    }
    return online_batch_f64_process(o->f64, pcm, n, flush, xt, xt_i16, xh, dh, xhi, dhi, cap, n_out);
}

extern "C" int snmf_online_batch_process_f64(snmf_online_batch* o, const double* const* pcm, const int64_t* n, const int32_t* flush,
                                             double* const* xt_f64, int16_t* const* xt_i16, double* const* xh_f64, double* const* dh_f64,
                                             const int64_t* cap, int64_t* n_out) {
    return ob_process_f64(o, pcm, n, flush, xt_f64, xt_i16, xh_f64, dh_f64, nullptr, nullptr, cap, n_out);
}

extern "C" int snmf_online_batch_process_classes_f64(snmf_online_batch* o, const double* const* pcm, const int64_t* n, const int32_t* flush,
                                                     double* const* xt_f64, int16_t* const* xt_i16, double* const* xh_f64,
                                                     double* const* dh_f64, double* const* xhi_f64, double* const* dhi_f64,
                                                     const int64_t* cap, int64_t* n_out) {
    return ob_process_f64(o, pcm, n, flush, xt_f64, xt_i16, xh_f64, dh_f64, xhi_f64, dhi_f64, cap, n_out);
}

extern "C" int snmf_online_batch_restart_f64(snmf_online_batch* o, int32_t n, const int32_t* slots, const double* Bd, const double* H0,
                                             const double* Ad) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    if (!o->f64) return fail(SNMF_ERR_STATE, "snmf_online_batch_restart_f64 needs a batch made by snmf_online_batch_create_f64");
    return online_batch_f64_restart(o->f64, n, slots, nullptr, Bd, H0, Ad, nullptr);
}

// ---- chains of recordings over the batch's slots (snmf_online_batch_chains.h) ----
extern "C" int64_t snmf_online_batch_out_capacity(const snmf_online_batch* o, int64_t n_samples) {
    if (!o || n_samples < 0) return 0;
    return (n_samples / o->p.frameshift + o->p.delay + 3) * (int64_t)o->p.frameshift;
}

// the three calls the driver makes are the public entries of the batch's precision
template <typename T>
struct ObChainOps;
template <>
struct ObChainOps<float> {
    snmf_online_batch* o;
    int restart(int n, const int32_t* slots, const double* Bd, const double* Bmd, const float* H0, const float* Ad) {
        return snmf_online_batch_restart_mel(o, n, slots, Bd, Bmd, H0, Ad);
    }
    int process(const float* const* pcm, const int64_t* n, const int32_t* flush, float* const* xt, int16_t* const* x16, const int64_t* cap,
                int64_t* n_out) {
        return snmf_online_batch_process_f32(o, pcm, n, flush, xt, x16, nullptr, nullptr, cap, n_out);
    }
    int basis(int k, double* dst) {
        return o->mel ? snmf_online_batch_get_mel_basis_f64(o, k, dst, o->n1) : snmf_online_batch_get_basis_f64(o, k, dst, o->F);
    }
};
template <>
struct ObChainOps<double> {
    snmf_online_batch* o;
    int restart(int n, const int32_t* slots, const double* Bd, const double*, const double* H0, const double* Ad) {
        return snmf_online_batch_restart_f64(o, n, slots, Bd, H0, Ad);
    }
    int process(const double* const* pcm, const int64_t* n, const int32_t* flush, double* const* xt, int16_t* const* x16, const int64_t* cap,
                int64_t* n_out) {
        return snmf_online_batch_process_f64(o, pcm, n, flush, xt, x16, nullptr, nullptr, cap, n_out);
    }
    int basis(int k, double* dst) { return snmf_online_batch_get_basis_f64(o, k, dst, o->F); }
};

template <typename T>
static int ob_run_chains(snmf_online_batch* o, const OChainsArgs<T>& a) {
    if (!o) return fail(SNMF_ERR_INVALID, "online batch handle is NULL");
    constexpr bool f64 = sizeof(T) == 8;
    const snmf_online_params& p = o->p;
    OChainsGeom g{};
    g.S = o->S; g.hop = p.frameshift; g.delay = p.delay;
    g.nB = (size_t)o->F * p.R_d;
    g.step0 = std::max<int64_t>(1, std::min<int64_t>(4096, kBChunkSlots / o->S));
    if (o->f64) {
        int r = 0, na = 0;
        online_batch_f64_dims(o->f64, &r, &na);
        g.r = (size_t)r;
        g.nA = p.adapt_train_N ? (size_t)na : 0;
    } else {
        g.r = (size_t)o->r;
        g.nA = p.adapt_train_N ? (size_t)o->Ra * o->ma : 0;
        g.nBm = o->mel ? (size_t)o->n1 * p.R_d : 0;
    }
    int64_t nf = 0;
    SN_TRY(ochains_check_args(g, a, &nf));
    if (a.n_out)
        for (int64_t i = 0; i < nf; ++i) a.n_out[i] = 0;
    if (f64 != (o->f64 != nullptr))
        return fail(SNMF_ERR_STATE, f64 ? "snmf_online_batch_run_chains_f64 needs a batch made by snmf_online_batch_create_f64"
                                        : "snmf_online_batch_run_chains_f32 on an fp64 batch: use snmf_online_batch_run_chains_f64");
    if (o->per_stream)
        return fail(SNMF_ERR_UNSUPPORTED, "run over chains: a batch with settings or event dictionaries per stream is not supported");
    if (a.Bmd && !g.nBm) return fail(SNMF_ERR_STATE, "B_Mel_d given to a batch that is not in Mel mode");
    SN_TRY(o->f64 ? online_batch_f64_idle(o->f64) : obatch_idle_check(o));
    if (nf == 0) return SNMF_OK;
    ObChainOps<T> ops{o};
    try {
        return ochains_run(g, a, ops);
    } catch (const std::bad_alloc&) {  // the driver's own buffers (sized by the data, before the first call) or a copy of a chunk
        return fail(SNMF_ERR_NOMEM, "run over chains: out of host memory");
    }
}

extern "C" int snmf_online_batch_run_chains_f32(snmf_online_batch* o, int32_t n_chains, const int32_t* n_files, const float* const* pcm,
                                                const int64_t* n_samples, const double* Bd, const double* Bmd, const float* H0,
                                                const float* Ad, int32_t chunk_hops, int16_t* const* xt_i16, float* const* xt_f32,
                                                const int64_t* cap, int64_t* n_out, double* const* B_out) {
    return ob_run_chains<float>(o, OChainsArgs<float>{n_chains, n_files, pcm, n_samples, Bd, Bmd, H0, Ad, chunk_hops, xt_i16, xt_f32, cap,
                                                      n_out, B_out});
}

extern "C" int snmf_online_batch_run_chains_f64(snmf_online_batch* o, int32_t n_chains, const int32_t* n_files, const double* const* pcm,
                                                const int64_t* n_samples, const double* Bd, const double* Bmd, const double* H0,
                                                const double* Ad, int32_t chunk_hops, int16_t* const* xt_i16, double* const* xt_f64,
                                                const int64_t* cap, int64_t* n_out, double* const* B_out) {
    return ob_run_chains<double>(o, OChainsArgs<double>{n_chains, n_files, pcm, n_samples, Bd, Bmd, H0, Ad, chunk_hops, xt_i16, xt_f64, cap,
                                                        n_out, B_out});
}
