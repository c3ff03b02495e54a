// snmf_tu_online.hip -- the online separation loop behind the C ABI (snmf_online_*), kernels in snmf_online.h, the per-frame arithmetic in snmf_online_common.h.
#include "snmf_internal.h"

// ---- online separation loop (include/snmf.h: snmf_online_*) -------------------------------------
// Host side of src/bnmf_sep_event_RT_IS16.m + the frame loop of src/NTF_sep_event_RT.m:54-135.  The
// host only sequences launches: per frame it reads one 32-byte status (did the adaptation condition
// fire?) and, when it did, runs the W-only adaptation solve through the engine's ordinary plan.
// The host driver is snmf_online_host.h, shared with the fp64 mode.  What is left here: the C entries and the snmf_online
// handle's own members (the engine's plans, Mel mode, the fp32 mirrors of the dictionaries), validation and creation, and
// the fp32 mode's steps of the driver (om_*).
#include "snmf_online.h"
#include "snmf_online_f64_host.h"  // the fp64 mode's host entry points (its kernels live in snmf_tu_online_f64.hip)
#include "snmf_online_host.h"

struct snmf_online : OnlineState<float> {
    OnlineF64* f64 = nullptr;  // non-null: an fp64 separator (snmf_online_create_f64); only ctx and p are then used
    int Fs = 0;                // rows of the solves: F, or F_order in Mel mode
    int mel = 0, mel_conv = 0, n1 = 0;  // B_sep_mode = 'Mel' (snmf_online_set_mel)
    float *melmat = nullptr, *Bmf = nullptr, *Ymel = nullptr;
    double *Bm = nullptr, *Bmtmp = nullptr;  // [n1 x r] Mel dictionaries [B_Mel_x | B_Mel_d], fp64 like B
    snmf_plan* hp = nullptr;  // frame solve: Fs x 1, rank r, H-only
    snmf_plan* ap = nullptr;  // adaptation solve: F x m_a, rank R_a, W-only
    snmf_plan* hsemi = nullptr;  // semi-supervised frame solve (basis_update_N / _E): generic path, W reset every frame
    snmf_plan* hb = nullptr;  // fixed dictionary (no adaptation): the frame solves of a whole batch in one launch
    DevState* bst = nullptr;
    double *bdiv = nullptr, *bcost = nullptr;
    OnlineStatus* bstatus = nullptr;
    float *recon1 = nullptr, *breco = nullptr;  // B_x*A_x | B_d*A_d from the frame solve: one frame / a batch
    // cooperative single-launch adaptation solve (k_wadapt)
    bool wadapt = false;
    int wa_nwg = 0;
    size_t wa_lds = 0;
    double *wa_W = nullptr, *wa_p1 = nullptr, *wa_p2 = nullptr, *wa_cost = nullptr;
    int* wa_nit = nullptr;
    unsigned* wa_bar = nullptr;
    float* Bf = nullptr;  // fp32 mirror of B (fp64 like the engine's W master copy, k_wapply) for the reconstructions
    OnlineStatus* status = nullptr;
    DevState* hst = nullptr;
    double *hdiv = nullptr, *hcost = nullptr;
};

// the one-launch frame solves' plan and buffers, and the Mel features: they depend on the solve geometry
static void om_free_call(snmf_online* o) {
    if (o->hb) {
        snmf_plan_destroy(o->hb);
        o->hb = nullptr;
    }
    void* ptrs[] = {o->bst, o->bdiv, o->bcost, o->bstatus, o->breco, o->Ymel};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->bst = nullptr;
    o->bdiv = o->bcost = nullptr;
    o->bstatus = nullptr;
    o->breco = o->Ymel = nullptr;
}

extern "C" void snmf_online_destroy(snmf_online* o) {
    if (!o) return;
    if (o->f64) {
        online_f64_destroy(o->f64);
        delete o;
        return;
    }
    hipSetDevice(o->ctx->device);
    hipStreamSynchronize(o->ctx->stream);
#ifdef SNMF_PROF_WA
    {
        unsigned long long pf[10] = {0};
        hipMemcpyFromSymbol(pf, HIP_SYMBOL(g_wa_prof), sizeof pf);
        if (pf[9]) {
            static const char* nm[8] = {"setup", "product Lam'", "product G + partial sums", "exchange A", "W update + partial sums", "exchange B", "normalise", "store"};
            fprintf(stderr, "[SNMF_PROF_WA] %llu solves, %.2f loops per solve; k cycles per solve:", pf[9], (double)pf[8] / pf[9]);
            for (int i = 0; i < 8; ++i) fprintf(stderr, " %s=%.1f", nm[i], (double)pf[i] / pf[9] * 1e-3);
            fprintf(stderr, "\n");
            unsigned long long z[10] = {0};
            hipMemcpyToSymbol(HIP_SYMBOL(g_wa_prof), z, sizeof z);
        }
    }
#endif
    if (o->hp) snmf_plan_destroy(o->hp);
    if (o->ap) snmf_plan_destroy(o->ap);
    if (o->hsemi) snmf_plan_destroy(o->hsemi);
    online_free_state(o);
    void* ptrs[] = {o->status, o->hst, o->hdiv, o->hcost, o->Bf, o->recon1, o->wa_W, o->wa_p1, o->wa_p2, o->wa_cost, o->wa_nit, o->wa_bar,
                    o->melmat, o->Bmf, o->Bm, o->Bmtmp};
    for (void* q : ptrs)
        if (q) hipFree(q);
    delete o;
}

static int online_validate(const snmf_online_params* p) {
    if (!p) return fail(SNMF_ERR_INVALID, "online params is NULL");
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
    }
    return SNMF_OK;
}

// (re)create the resident solves for o->Fs rows: the frame solve, the optional semi-supervised variant, the
// adaptation plan and the cooperative adaptation kernel's buffers
static int online_make_solvers(snmf_online* o) {
    const snmf_online_params* p = &o->p;
    snmf_ctx* ctx = o->ctx;
    const int F = o->Fs, r = o->r;
    const int Ra = p->adapt_train_N ? p->R_a : 1, ma = p->adapt_train_N ? p->m_a : 1;
    hipStreamSynchronize(ctx->stream);
    for (snmf_plan** q : {&o->hp, &o->hsemi, &o->ap}) {
        if (*q) snmf_plan_destroy(*q);
        *q = nullptr;
    }
    for (void** q : {(void**)&o->wa_W, (void**)&o->wa_p1, (void**)&o->wa_p2, (void**)&o->wa_cost, (void**)&o->wa_nit, (void**)&o->wa_bar}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    o->wadapt = false;
    int s = SNMF_OK;
    auto A = [&](int v) { if (s == SNMF_OK) s = v; };
    // the two resident solves
    snmf_params hp{};
    hp.F = F; hp.T = 1; hp.r = r; hp.beta = p->beta_div; hp.max_iter = p->max_iter; hp.conv_eps = p->conv_eps;
    hp.cost_check = p->cost_check; hp.floor_v = 1; hp.sparsity_kind = SNMF_SPARSITY_SCALAR; hp.sparsity_scalar = p->sparsity;
    std::vector<uint8_t> zeros(std::max(r, Ra), 0), ones(std::max(r, Ra), 1);
    hp.w_update_ind = zeros.data();  // supervised (:139)
    hp.h_update_ind = ones.data();   // :148
    A(snmf_plan_create(ctx, &hp, &o->hp));
    // !small_ok (F + r too large for the persistent single-launch kernels, e.g. the exemplar setting R_x = R_d = 500 of
    // settings/bak_IS16_results/initial_setting_Exemplar.m:47-48): the frame solve runs through the ordinary plan loop
    if (p->basis_update_N || p->basis_update_E) {
        snmf_params sp = hp;
        std::vector<uint8_t> wm(r, 0);
        for (int k = 0; k < r; ++k) wm[k] = p->basis_update_N ? (k >= p->R_x) : (k < p->R_x);  // :125-131
        sp.w_update_ind = wm.data();
        A(snmf_plan_create(ctx, &sp, &o->hsemi));
    }
    if (p->adapt_train_N) {
        snmf_params ap = hp;
        ap.T = ma; ap.r = Ra;
        ap.w_update_ind = ones.data();   // :330 (the per-solve subset r_up is written on the device)
        ap.h_update_ind = zeros.data();  // :331
        A(snmf_plan_create(ctx, &ap, &o->ap));
    }
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    if (p->adapt_train_N && p->beta_div == 1.0 && p->R_a <= kWaRP && !getenv("SNMF_NO_WADAPT")) {
        int coop = 0;
        hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, ctx->device);
        o->wa_nwg = (F + kWaRB - 1) / kWaRB;
        o->wa_lds = (size_t)(kWaRB * kWaRP + 4 * kWaRP + 32 + 256) * 8 +
                    (size_t)(2 * kWaRB * kWaRP + kWaRP + 2 * kWaRB * p->m_a + p->R_a * p->m_a + p->m_a * (kWaRP + 1) +
                             ((p->m_a <= 128 && p->m_a % 4 == 0) ? p->R_a * 128 + p->m_a * kWaRP : 0)) * 4;  // (+ the products' operand images)
        o->wadapt = coop != 0 && o->wa_nwg <= ctx->n_cu && o->wa_nwg <= 2 * kWaQ && o->wa_lds <= 160 * 1024;
        if (o->wadapt) {
            D(&o->wa_W, (size_t)p->R_a * F);
            D(&o->wa_p1, (size_t)o->wa_nwg * (kWaRP + 1));
            D(&o->wa_p2, (size_t)o->wa_nwg * 2 * kWaRP);
            D(&o->wa_cost, (size_t)p->max_iter);
            D(&o->wa_nit, (size_t)1);
            D(&o->wa_bar, (size_t)1);
        }
    }
    return s;
}

extern "C" int snmf_online_create(snmf_ctx* ctx, const snmf_online_params* p, const float* Bx, const float* Bd, const float* H0,
                                  const float* Ad0, const float* win_stft, const float* win_istft, snmf_online** out) {
    if (!ctx || !out || !Bx || !Bd || !H0 || !win_stft || !win_istft) return fail(SNMF_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SN_TRY(online_validate(p));
    if (p->adapt_train_N && !Ad0) return fail(SNMF_ERR_INVALID, "Ad_blk0 is required when adapt_train_N is set");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    snmf_online* o = new snmf_online();
    int s = online_alloc_state(o, ctx, p);
    const int F = o->F, r = o->r;
    o->Fs = F;
    if (s == SNMF_OK) s = online_make_solvers(o);
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->Bf, (size_t)F * r);
    D(&o->recon1, (size_t)2 * F);
    D(&o->status, (size_t)1); D(&o->hst, (size_t)1);
    D(&o->hdiv, (size_t)p->max_iter); D(&o->hcost, (size_t)p->max_iter);
    if (s != SNMF_OK) {
        snmf_online_destroy(o);
        return s;
    }
    std::vector<float2> htw;
    std::vector<double> hB((size_t)F * r);
    for (size_t i = 0; i < (size_t)F * p->R_x; ++i) hB[i] = (double)Bx[i];
    for (size_t i = 0; i < (size_t)F * p->R_d; ++i) hB[(size_t)F * p->R_x + i] = (double)Bd[i];
    hipMemcpyAsync(o->B, hB.data(), hB.size() * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->Bfix, hB.data() + (size_t)F * p->R_x, (size_t)F * p->R_d * 8, hipMemcpyHostToDevice, st);  // B_Mel_d in DFT mode (:328)
    hipMemcpyAsync(o->Bf, Bx, (size_t)F * p->R_x * 4, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->Bf + (size_t)F * p->R_x, Bd, (size_t)F * p->R_d * 4, hipMemcpyHostToDevice, st);
    online_upload_state(o, H0, Ad0, win_stft, win_istft, htw);
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        snmf_online_destroy(o);
        return fail(SNMF_ERR_NO_DEVICE, "online create: %s", hipGetErrorString(e));
    }
    s = set_w<double>(o->hp, o->B, F, 1);
    if (s != SNMF_OK) {
        snmf_online_destroy(o);
        return s;
    }
    o->hist.assign((size_t)(p->framelength - p->frameshift), 0.f);
    *out = o;
    return SNMF_OK;
}

// B_sep_mode = 'Mel' (src/bnmf_sep_event_RT_IS16.m:106-120, src/init_buff.m:45-47): the solves run on Mel features
extern "C" int snmf_online_set_mel(snmf_online* o, int32_t F_order, int32_t mel_conv, const float* melmat, const float* BMx,
                                   const float* BMd) {
    if (!o || !melmat || !BMx || !BMd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) return fail(SNMF_ERR_UNSUPPORTED, "fp64 online separator: B_sep_mode 'Mel' is not supported");
    if (o->l != 0 || !o->pending.empty()) return fail(SNMF_ERR_STATE, "snmf_online_set_mel must precede the first process call");
    if (F_order < 2 || F_order > o->F) return fail(SNMF_ERR_INVALID, "F_order must be in [2, fftlength/2+1]");
    if (mel_conv && (size_t)o->n_cls * F_order * 4 > o->ctx->lds_max)
        return fail(SNMF_ERR_UNSUPPORTED, "MelConv = 1 with %d classes at F_order = %d: the class kernel's Mel products do not fit the LDS", o->n_cls, F_order);
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    const int n1 = F_order, r = o->r, F = o->F, Rx = o->p.R_x, Rd = o->p.R_d;
    o->mel = 1;
    o->mel_conv = mel_conv != 0;
    o->n1 = n1;
    o->Fs = n1;
    SN_TRY(online_make_solvers(o));
    for (void** q : {(void**)&o->melmat, (void**)&o->Bmf, (void**)&o->Bm, (void**)&o->Bmtmp}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    SN_TRY(dalloc(&o->melmat, (size_t)n1 * F));
    SN_TRY(dalloc(&o->Bmf, (size_t)n1 * r));
    SN_TRY(dalloc(&o->Bm, (size_t)n1 * r));
    SN_TRY(dalloc(&o->Bmtmp, (size_t)n1 * Rd));
    std::vector<double> hB((size_t)n1 * r);
    for (size_t i = 0; i < (size_t)n1 * Rx; ++i) hB[i] = (double)BMx[i];
    for (size_t i = 0; i < (size_t)n1 * Rd; ++i) hB[(size_t)n1 * Rx + i] = (double)BMd[i];
    HIP_TRY(hipMemcpyAsync(o->Bm, hB.data(), hB.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->Bmf, BMx, (size_t)n1 * Rx * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->Bmf + (size_t)n1 * Rx, BMd, (size_t)n1 * Rd * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->melmat, melmat, (size_t)n1 * F * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    SN_TRY(set_w<double>(o->hp, o->Bm, n1, 1));
    online_free_call_buffers(o);  // batch buffers depend on the solve geometry
    return SNMF_OK;
}

/* Current B_Mel_d (n1 x R_d): what the Mel-mode adaptation updates (src/bnmf_sep_event_RT_IS16.m:318). */
extern "C" int snmf_online_get_mel_basis_f32(snmf_online* o, float* BMd, int64_t ld) {
    if (!o || !BMd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (!o->mel) return fail(SNMF_ERR_STATE, "not in Mel mode");
    if (ld < o->n1) return fail(SNMF_ERR_INVALID, "ld < F_order");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    HIP_TRY(hipMemcpy2D(BMd, (size_t)ld * 4, o->Bmf + (size_t)o->n1 * o->p.R_x, (size_t)o->n1 * 4, (size_t)o->n1 * 4, (size_t)o->p.R_d,
                        hipMemcpyDeviceToHost));
    return SNMF_OK;
}

/* p.EVENT_RANK / p.NOISE_RANK (settings/initial_setting_SNMF_NAT.m:40-44): the class partition of x_hat_i / d_hat_i
 * (src/bnmf_sep_event_RT_IS16.m:158-202, :350-361). */
extern "C" int snmf_online_set_classes(snmf_online* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num,
                                       const int32_t* noise_rank) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (!o->p.class_outputs) return fail(SNMF_ERR_STATE, "class outputs were not requested at creation");
    if (o->f64) return online_f64_set_classes(o->f64, event_num, event_rank, noise_num, noise_rank);
    std::vector<int> cls;
    SN_TRY(online_class_table(o, event_num, event_rank, noise_num, noise_rank, &cls));
    const int nc = event_num + noise_num;
    if (o->mel && o->mel_conv && (size_t)nc * o->n1 * 4 > o->ctx->lds_max)
        return fail(SNMF_ERR_UNSUPPORTED, "MelConv = 1 with %d classes at F_order = %d: the class kernel's Mel products do not fit the LDS", nc, o->n1);
    return online_install_classes(o, cls, event_num, nc);
}

static int om_reserve(snmf_online* o, int cap) {
    if (o->mel) SN_TRY(dalloc(&o->Ymel, (size_t)o->n1 * cap));
    if (!o->p.adapt_train_N && !o->hsemi && o->hp->small_ok) {
        snmf_params bp = o->hp->p;
        bp.T = cap;
        std::vector<uint8_t> zeros(o->r, 0), ones(o->r, 1);
        bp.w_update_ind = zeros.data();
        bp.h_update_ind = ones.data();
        SN_TRY(snmf_plan_create(o->ctx, &bp, &o->hb));
        SN_TRY(set_w<double>(o->hb, o->mel ? o->Bm : o->B, o->Fs, 1));
        SN_TRY(dalloc(&o->bst, (size_t)cap));
        SN_TRY(dalloc(&o->bdiv, (size_t)cap * o->p.max_iter));
        SN_TRY(dalloc(&o->bcost, (size_t)cap * o->p.max_iter));
        SN_TRY(dalloc(&o->bstatus, (size_t)cap));
        SN_TRY(dalloc(&o->breco, (size_t)cap * 2 * o->Fs));
    }
    return SNMF_OK;
}

// the frame solve (:148-154): V = Ym (device), W resident, H0 the fixed start; leaves A in hp->H[0]
static int online_solve_frame(snmf_online* o, const float* dV, const float** A_out, const DevState** st_out, const float** recon_out) {
    hipStream_t st = o->ctx->stream;
    if (o->hsemi) {
        // semi-supervised: an ordinary solve with part of W free; init_w = [B_DFT_x, B_DFT_d] again every frame (:140-146)
        snmf_plan* ps = o->hsemi;
        SN_TRY(set_v<float>(ps, dV, o->Fs, 1));
        SN_TRY(set_w<double>(ps, o->mel ? o->Bm : o->B, o->Fs, 1));
        SN_TRY(set_h<float>(ps, o->H0, o->r, 1));
        SN_TRY(snmf_plan_init(ps));
        SN_TRY(snmf_plan_run(ps, o->p.max_iter, nullptr));
        int idx = 0;
        SN_TRY(result_h_index(ps, &idx));
        *A_out = ps->H[idx];
        *st_out = ps->st;
        *recon_out = nullptr;
        return SNMF_OK;
    }
    snmf_plan* pl = o->hp;
    if (!pl->small_ok) {
        // large rank: the ordinary plan loop (16-frame tiles), one solve per frame; reconstructions are formed in k_opost
        SN_TRY(set_v<float>(pl, dV, o->Fs, 1));
        SN_TRY(set_h<float>(pl, o->H0, o->r, 1));
        SN_TRY(snmf_plan_init(pl));  // W and its norms are reused unless the adaptation has replaced the dictionary
        SN_TRY(snmf_plan_run(pl, o->p.max_iter, nullptr));
        int idx = 0;
        SN_TRY(result_h_index(pl, &idx));
        *A_out = pl->H[idx];
        *st_out = pl->st;
        *recon_out = nullptr;
        return SNMF_OK;
    }
    *A_out = pl->H[0];
    *st_out = o->hst;
    *recon_out = (pl->frame_fb && (!o->mel || o->mel_conv)) ? o->recon1 : nullptr;  // Mel without MelConv: B_DFT*A, formed in k_opost
    const size_t nVp = (size_t)pl->Fp * pl->Tp;
    hipLaunchKernelGGL(k_pack<float>, dim3(grid_for(nVp)), dim3(256), 0, st, dV, (int64_t)o->Fs, o->Fs, 1, pl->V, pl->Fp, pl->Tp, kFlr,
                       pl->p.floor_v ? 1 : 0);
    HIP_TRY(hipGetLastError());
    pl->have_v = true;
    if (pl->w_dirty) SN_TRY(launch_wapply(pl, pl->stats, 0, false, true));  // wn, w./wn (:157-159)
    pl->w_dirty = false;
    pl->cur = 0;
    hipLaunchKernelGGL(k_tile_h0<float>, dim3(grid_for((size_t)pl->rp)), dim3(256), 0, st, (const float*)o->H0, pl->wn, o->r, pl->rp, 1,
                       1, pl->H[0]);  // h .* wn' (:160)
    HIP_TRY(hipGetLastError());
    pl->have_h = true;
    pl->inited = false;
    HIP_TRY(hipMemsetAsync(o->hst, 0, sizeof(DevState), st));
    return launch_small(pl, 1, 1, o->hdiv, o->hcost, o->hst, (o->mel && !o->mel_conv) ? nullptr : o->recon1, o->p.R_x);
}

// the class spectra of n frames from frame i0 of the call on (:158-202): activations A + i*a_stride, the dictionary as the
// frame solve saw it -- so this is queued behind the solve and before anything of the adaptation (k_oclass, snmf_online.h)
static int online_class_spectra(snmf_online* o, const float* A, int a_stride, int i0, int n) {
    const bool mc = o->mel && o->mel_conv;
    OClassArgs c{};
    c.B = mc ? o->Bmf : o->Bf; c.A = A; c.cls = o->cls; c.melmat = o->melmat; c.out = o->Xc + (size_t)i0 * o->F;
    c.cstride = (int64_t)o->cap_frames * o->F; c.n_cls = o->n_cls; c.F = o->F; c.n1 = o->n1; c.mel_conv = mc; c.n = n; c.a_stride = a_stride;
    const size_t lds = mc ? (size_t)o->n_cls * o->n1 * 4 : 0;
    if (lds) SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_oclass, lds));
    hipLaunchKernelGGL(k_oclass, dim3((o->F + 255) / 256, n), dim3(256), lds, o->ctx->stream, c);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// :296-336 once the status says the solve is due
static int om_adapt(snmf_online* o, int32_t* iters) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    snmf_plan* ap = o->ap;
    // DFT mode adapts B_DFT_d on lambda_d_blk (:320-338); Mel mode adapts B_Mel_d on melmat*lambda_d_blk (:298-318)
    const int Fs = o->Fs;
    double* Ball = o->mel ? o->Bm : o->B;
    double* Bd = Ball + (size_t)Fs * p.R_x;
    double* Btmp = o->mel ? o->Bmtmp : o->Btmp;
    float* mirror = (o->mel ? o->Bmf : o->Bf) + (size_t)Fs * p.R_x;
    const double* Bfix = o->mel ? Bd : o->Bfix;  // columns beyond R_a never change; :328 takes them from B_Mel_d
    if (o->mel) {
        hipLaunchKernelGGL(k_oprep_mel, dim3(p.m_a), dim3(256), 0, st, (const float*)o->ldblk, (const float*)o->adblk, (const uint8_t*)o->rup,
                           (const OnlineDev*)o->dev, (const float*)o->melmat, o->F, o->n1, p.R_a, p.m_a, o->Vad, o->Had, ap->w_ind);
    } else {
        const size_t n = (size_t)o->F * p.m_a + (size_t)p.R_a * p.m_a + p.R_a;
        hipLaunchKernelGGL(k_oprep, dim3(grid_for(n)), dim3(256), 0, st, (const float*)o->ldblk, (const float*)o->adblk,
                           (const uint8_t*)o->rup, (const OnlineDev*)o->dev, o->F, p.R_a, p.m_a, o->Vad, o->Had, ap->w_ind);
    }
    HIP_TRY(hipGetLastError());
    const double* Wres = nullptr;
    int ldw = 0;
    if (o->wadapt) {
        // the whole solve in one cooperative launch (k_wadapt)
        WAdaptArgs wa{};
        wa.V = o->Vad; wa.H = o->Had; wa.W0 = Bd; wa.w_ind = ap->w_ind; wa.Wout = o->wa_W; wa.part1 = o->wa_p1; wa.part2 = o->wa_p2;
        wa.costh = o->wa_cost; wa.n_iter_out = o->wa_nit; wa.F = Fs; wa.Ra = p.R_a; wa.ma = p.m_a; wa.max_iter = p.max_iter;
        wa.cost_check = p.cost_check; wa.sparsity = (float)p.sparsity; wa.flr = kFlr; wa.conv_eps = p.conv_eps;
        SN_TRY(ensure_dyn_lds(o->ctx->device, (const void*)k_wadapt, o->wa_lds));
        wa.bar = o->wa_bar;
        HIP_TRY(hipMemsetAsync(o->wa_bar, 0, 4, st));
        void* kargs[] = {&wa};
        if (hipLaunchCooperativeKernel((const void*)k_wadapt, dim3(o->wa_nwg), dim3(kWaNT), kargs, (unsigned)o->wa_lds, st) == hipSuccess) {
            HIP_TRY(hipMemcpyAsync(iters, o->wa_nit, 4, hipMemcpyDeviceToHost, st));
            // the solve's verdict is read BEFORE its W is merged into the dictionary: a timed-out grid barrier leaves
            // wa_W invalid, and B_d, its fp32 mirror and the frame-solve plan must not see it
            HIP_TRY(hipStreamSynchronize(st));
            if (*iters < 0) return fail(SNMF_ERR_INTERNAL, "adaptation kernel: grid barrier timed out (dictionary left untouched)");
            Wres = o->wa_W;
            ldw = Fs;
        } else {
            (void)hipGetLastError();  // cooperative launch refused (e.g. CUs not all available): generic path from now on
            o->wadapt = false;
        }
    }
    if (!Wres) {
        SN_TRY(set_v<float>(ap, o->Vad, Fs, 1));       // lambda_d_blk[_Mel] (floored at 1e-9 inside, sparse_nmf.m:169)
        SN_TRY(set_w<double>(ap, Bd, Fs, 1));          // init_w: first R_a noise columns (:332)
        SN_TRY(set_h<float>(ap, o->Had, p.R_a, 1));    // init_h (:333)
        SN_TRY(snmf_plan_init(ap));
        SN_TRY(snmf_plan_run(ap, p.max_iter, iters));
        Wres = ap->Wc;
        ldw = ap->Fp;
    }
    hipLaunchKernelGGL(k_oassemble, dim3(p.R_d), dim3(256), 0, st, (const double*)Bd, Wres, ldw, Bfix, (const uint8_t*)o->rup, Fs, p.R_a,
                       p.R_d, Btmp, mirror);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(Bd, Btmp, (size_t)Fs * p.R_d * 8, hipMemcpyDeviceToDevice, st));
    SN_TRY(set_w<double>(o->hp, Ball, Fs, 1));         // next frame's init_w (:140-146)
    return SNMF_OK;  // `iters` is already on the host (both paths synchronised when they read it)
}

// ---- the other steps of the shared driver (snmf_online_host.h) -------------------------------------------------------------
static int om_stft(snmf_online* o, int n) {
    hipStream_t st = o->ctx->stream;
    const OStftArgs sa = online_stft_args(o, n);
    by_logn([&](auto L) { hipLaunchKernelGGL(k_ostft<decltype(L)::value>, dim3(n), dim3(256), 0, st, sa); }, o->N);
    HIP_TRY(hipGetLastError());
    if (o->mel) {
        hipLaunchKernelGGL(k_omel_frame, dim3(n), dim3(256), (size_t)(o->n1 + 2) * 4, st, (const float*)o->Ym, (const float*)o->melmat, o->F, o->n1, n,
                           o->Ymel);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

// the post-filter's launch for one frame (the one-launch path sets A, hst, recon, status, n and a_stride itself)
static OPostArgs online_post_frame_args(const snmf_online* o, int i, int64_t l) {
    OPostArgs a = online_post_args(o, i, l);
    a.B = o->Bf;
    a.n = 1;
    a.a_stride = 0;
    a.mel = o->mel; a.mel_conv = o->mel_conv; a.n1 = o->n1; a.melmat = o->melmat; a.Bmf = o->Bmf;
    a.Ymel = o->mel ? o->Ymel + (size_t)i * o->n1 : nullptr;
    a.recon_len = o->Fs;
    return a;
}

static int online_launch_post(snmf_online* o, const OPostArgs& a) {
    hipLaunchKernelGGL(k_opost, dim3(1), dim3(1024), (size_t)(o->r + 7 * o->F + 3 * o->n1) * 4, o->ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static bool om_one_launch(const snmf_online* o) { return !o->p.adapt_train_N && !o->hsemi && o->hb; }

// Fixed dictionary: all frame solves of the run in ONE launch (one workgroup per frame, W normalised once), then ONE k_opost
// launch walks the sequential post-filter recurrences.
static int om_solve_run(snmf_online* o, int n, const OnlineStatus** st_out) {
    hipStream_t st = o->ctx->stream;
    snmf_plan* pl = o->hb;
    const size_t nVp = (size_t)pl->Fp * pl->Tp;
    hipLaunchKernelGGL(k_pack<float>, dim3(grid_for(nVp)), dim3(256), 0, st, (const float*)(o->mel ? o->Ymel : o->Ym), (int64_t)o->Fs, o->Fs, n,
                       pl->V, pl->Fp, pl->Tp, kFlr, pl->p.floor_v ? 1 : 0);
    HIP_TRY(hipGetLastError());
    pl->have_v = true;
    if (pl->w_dirty) SN_TRY(launch_wapply(pl, pl->stats, 0, false, true));
    pl->w_dirty = false;
    pl->cur = 0;
    hipLaunchKernelGGL(k_tile_h0<float>, dim3(grid_for((size_t)n * pl->rp)), dim3(256), 0, st, (const float*)o->H0, pl->wn, o->r, pl->rp,
                       1, n, pl->H[0]);
    HIP_TRY(hipGetLastError());
    pl->have_h = true;
    pl->inited = false;
    HIP_TRY(hipMemsetAsync(o->bst, 0, (size_t)n * sizeof(DevState), st));
    SN_TRY(launch_small(pl, n, 1, o->bdiv, o->bcost, o->bst, (o->mel && !o->mel_conv) ? nullptr : o->breco, o->p.R_x));
    OPostArgs a = online_post_frame_args(o, 0, o->l + 1);
    a.A = pl->H[0]; a.hst = o->bst; a.status = o->bstatus; a.n = n; a.a_stride = pl->rp;
    a.recon = (pl->frame_fb && (!o->mel || o->mel_conv)) ? o->breco : nullptr;
    SN_TRY(online_launch_post(o, a));
    if (o->n_cls) SN_TRY(online_class_spectra(o, pl->H[0], pl->rp, 0, n));
    *st_out = o->bstatus;
    return SNMF_OK;
}

static int om_solve_frame(snmf_online* o, int i, const OnlineStatus** st_out) {
    OPostArgs a = online_post_frame_args(o, i, o->l + 1 + i);
    SN_TRY(online_solve_frame(o, o->mel ? o->Ymel + (size_t)i * o->n1 : o->Ym + (size_t)i * o->F, &a.A, &a.hst, &a.recon));
    a.status = o->status;
    SN_TRY(online_launch_post(o, a));
    if (o->n_cls) SN_TRY(online_class_spectra(o, a.A, 0, i, 1));
    *st_out = o->status;
    return SNMF_OK;
}

static int om_istft(snmf_online* o, const float* mag, int n, float* syn) {
    const OIstftArgs ia = online_istft_args(o, mag, n, syn);
    by_logn([&](auto L) { hipLaunchKernelGGL(k_oistft<decltype(L)::value>, dim3(n), dim3(256), 0, o->ctx->stream, ia); }, o->N);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// the whole class-major stack through ONE inverse-STFT launch, queued when the driver asks for the first class
static int om_istft_class(snmf_online* o, int c, int n, size_t syn_cs) {
    if (c) return SNMF_OK;
    const OIstftArgs ia = online_istft_args(o, (const float*)o->Xc, n, o->syn_c + (size_t)(o->nov - 1) * o->p.framelength);
    const int64_t mag_cs = (int64_t)o->cap_frames * o->F;
    by_logn([&](auto L) {
        hipLaunchKernelGGL(k_oistft_cls<decltype(L)::value>, dim3(n, o->n_cls), dim3(256), 0, o->ctx->stream, ia, mag_cs, (int64_t)syn_cs);
    }, o->N);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

static int om_ola(snmf_online* o, const float* syn, int n, int l0, int i_first, int n_out, float* out, int16_t* out16) {
    const snmf_online_params& p = o->p;
    hipLaunchKernelGGL(k_oola, dim3(grid_for((size_t)n_out * p.frameshift)), dim3(256), 0, o->ctx->stream, syn, n, l0, p.delay, p.framelength,
                       p.frameshift, o->nov, i_first, n_out, out, out16);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// snmf_online_process_f32 on an fp64 separator: the fp64 path, float outputs rounded from its doubles
static int online_f64_process_rounded(snmf_online* o, const float* pcm, int64_t n, int flush, float* xt_f32, int16_t* xt_i16,
                                      float* xh_f32, float* dh_f32, float* xhi_f32, float* dhi_f32, int64_t cap, int64_t* n_out) {
    if (n_out) *n_out = 0;
    if (n < 0 || (n > 0 && !pcm)) return fail(SNMF_ERR_INVALID, "pcm is NULL");  // (before pcm is read here)
    std::vector<double> x(pcm, pcm + n);
    // what this call can write at most (n hops, one left over from earlier calls, the flush frames), not the caller's cap
    const int64_t hop = o->p.frameshift, most = (n / hop + 1 + (flush ? o->p.delay + 1 : 0)) * hop;
    const size_t c = (size_t)std::max<int64_t>(std::min(cap, most), 0);
    int n_ev = 1, n_no = 1;
    online_f64_class_counts(o->f64, &n_ev, &n_no);
    std::vector<double> xt(xt_f32 ? c : 0), xh(xh_f32 ? c : 0), dh(dh_f32 ? c : 0), xhi(xhi_f32 ? c * n_ev : 0), dhi(dhi_f32 ? c * n_no : 0);
    int64_t m = 0;
    SN_TRY(online_f64_process(o->f64, x.data(), n, flush, xt_f32 ? xt.data() : nullptr, xt_i16, xh_f32 ? xh.data() : nullptr,
                              dh_f32 ? dh.data() : nullptr, xhi_f32 ? xhi.data() : nullptr, dhi_f32 ? dhi.data() : nullptr, (int64_t)c, &m));
    for (int64_t i = 0; i < m; ++i) {
        if (xt_f32) xt_f32[i] = (float)xt[i];
        if (xh_f32) xh_f32[i] = (float)xh[i];
        if (dh_f32) dh_f32[i] = (float)dh[i];
    }
    for (int k = 0; xhi_f32 && k < n_ev; ++k)  // (class-major at the caller's cap)
        for (int64_t i = 0; i < m; ++i) xhi_f32[(size_t)k * cap + i] = (float)xhi[(size_t)k * c + i];
    for (int k = 0; dhi_f32 && k < n_no; ++k)
        for (int64_t i = 0; i < m; ++i) dhi_f32[(size_t)k * cap + i] = (float)dhi[(size_t)k * c + i];
    if (n_out) *n_out = m;
    return SNMF_OK;
}

// snmf_online_process_f32 / snmf_online_process_classes_f32 (xhi_f32 / dhi_f32: the class signals, class-major at `cap`)
static int online_process_f32(snmf_online* o, const float* pcm, int64_t n, int flush, float* xt_f32, int16_t* xt_i16, float* xh_f32,
                              float* dh_f32, float* xhi_f32, float* dhi_f32, int64_t cap, int64_t* n_out) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (o->f64) return online_f64_process_rounded(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, xhi_f32, dhi_f32, cap, n_out);
    return online_process(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, xhi_f32, dhi_f32, cap, n_out);
}

extern "C" int snmf_online_process_f32(snmf_online* o, const float* pcm, int64_t n, int flush, float* xt_f32, int16_t* xt_i16,
                                       float* xh_f32, float* dh_f32, int64_t cap, int64_t* n_out) {
    return online_process_f32(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, nullptr, nullptr, cap, n_out);
}

extern "C" int snmf_online_process_classes_f32(snmf_online* o, const float* pcm, int64_t n, int flush, float* xt_f32, int16_t* xt_i16,
                                               float* xh_f32, float* dh_f32, float* xhi_f32, float* dhi_f32, int64_t cap, int64_t* n_out) {
    return online_process_f32(o, pcm, n, flush, xt_f32, xt_i16, xh_f32, dh_f32, xhi_f32, dhi_f32, cap, n_out);
}

extern "C" int snmf_online_get_basis_f32(snmf_online* o, float* Bd, int64_t ld) {
    if (!o || !Bd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) {
        const int F = o->p.fftlength / 2 + 1;
        if (ld < F) return fail(SNMF_ERR_INVALID, "ld < F");
        std::vector<double> B((size_t)F * o->p.R_d);
        SN_TRY(online_f64_get_basis(o->f64, B.data(), F));
        for (int j = 0; j < o->p.R_d; ++j)
            for (int f = 0; f < F; ++f) Bd[(size_t)j * ld + f] = (float)B[(size_t)j * F + f];
        return SNMF_OK;
    }
    if (ld < o->F) return fail(SNMF_ERR_INVALID, "ld < F");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    HIP_TRY(hipMemcpy2D(Bd, (size_t)ld * 4, o->Bf + (size_t)o->F * o->p.R_x, (size_t)o->F * 4, (size_t)o->F * 4, (size_t)o->p.R_d,
                        hipMemcpyDeviceToHost));
    return SNMF_OK;
}

extern "C" int snmf_online_trace(snmf_online* o, snmf_online_frame* out, int64_t cap, int64_t* n) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (o->f64) return online_f64_trace(o->f64, out, cap, n);
    return online_trace_read(o, out, cap, n);
}

// ---- fp64 mode (snmf_online_f64.h): every input crosses in fp64 and every step from PCM to the fed-back state is fp64 ----
extern "C" int snmf_online_create_f64(snmf_ctx* ctx, const snmf_online_params* p, const double* Bx, const double* Bd, const double* H0,
                                      const double* Ad0, const double* win_stft, const double* win_istft, snmf_online** out) {
    if (!ctx || !out || !Bx || !Bd || !H0 || !win_stft || !win_istft) return fail(SNMF_ERR_INVALID, "NULL argument");
    *out = nullptr;
    SN_TRY(online_validate(p));
    if (p->adapt_train_N && !Ad0) return fail(SNMF_ERR_INVALID, "Ad_blk0 is required when adapt_train_N is set");
    OnlineF64* f = nullptr;
    SN_TRY(online_f64_create(ctx, p, Bx, Bd, H0, Ad0, win_stft, win_istft, &f));
    snmf_online* o = new snmf_online();
    o->ctx = ctx;
    o->p = *p;
    o->f64 = f;
    *out = o;
    return SNMF_OK;
}

extern "C" int snmf_online_process_f64(snmf_online* o, const double* pcm, int64_t n, int flush, double* xt_f64, int16_t* xt_i16,
                                       double* xh_f64, double* dh_f64, int64_t cap, int64_t* n_out) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (n_out) *n_out = 0;
    if (!o->f64) return fail(SNMF_ERR_STATE, "snmf_online_process_f64 needs a separator made by snmf_online_create_f64");
    return online_f64_process(o->f64, pcm, n, flush, xt_f64, xt_i16, xh_f64, dh_f64, nullptr, nullptr, cap, n_out);
}

extern "C" int snmf_online_process_classes_f64(snmf_online* o, const double* pcm, int64_t n, int flush, double* xt_f64, int16_t* xt_i16,
                                               double* xh_f64, double* dh_f64, double* xhi_f64, double* dhi_f64, int64_t cap,
                                               int64_t* n_out) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (n_out) *n_out = 0;
    if (!o->f64) return fail(SNMF_ERR_STATE, "snmf_online_process_classes_f64 needs a separator made by snmf_online_create_f64");
    return online_f64_process(o->f64, pcm, n, flush, xt_f64, xt_i16, xh_f64, dh_f64, xhi_f64, dhi_f64, cap, n_out);
}

extern "C" int snmf_online_get_basis_f64(snmf_online* o, double* Bd, int64_t ld) {
    if (!o || !Bd) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) return online_f64_get_basis(o->f64, Bd, ld);
    return online_get_basis_f64(o, Bd, ld);
}

// ---- the state g as a record, and the next file in place (the driver's last section; kernels k_ostate_get / k_ostate_put) ----
static void om_state_mode(const snmf_online* o, int* mel, int* mel_conv, int* n1) {
    *mel = o->mel;
    *mel_conv = o->mel_conv;
    *n1 = o->n1;
}

// the record's B_Mel_d goes to / comes from the Mel master
static int om_state_launch(snmf_online* o, const OStateArgs<float>& a0, int64_t l, bool put) {
    OStateArgs<float> a = a0;
    a.Bm = o->mel ? o->Bm : nullptr;
    a.n1 = o->n1;
    if (put) hipLaunchKernelGGL(k_ostate_put, dim3(1, kStN, kStParts), dim3(256), 0, o->ctx->stream, a);
    else hipLaunchKernelGGL(k_ostate_get, dim3(1, kStN, kStParts), dim3(256), 0, o->ctx->stream, a, l);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// The noise columns of the fp64 masters changed (a restart, a set-state): their fp32 mirrors, and the dictionary of the
// frame solves' plans as creation / snmf_online_set_mel and the adaptation leave it.
static int om_refresh_dict(snmf_online* o) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const size_t nD = (size_t)o->F * p.R_d, xD = (size_t)o->F * p.R_x;
    hipLaunchKernelGGL(k_omirror, dim3(grid_for(nD)), dim3(256), 0, st, (const double*)(o->B + xD), o->Bf + xD, nD);
    HIP_TRY(hipGetLastError());
    if (o->mel) {
        const size_t nM = (size_t)o->n1 * p.R_d, xM = (size_t)o->n1 * p.R_x;
        hipLaunchKernelGGL(k_omirror, dim3(grid_for(nM)), dim3(256), 0, st, (const double*)(o->Bm + xM), o->Bmf + xM, nM);
        HIP_TRY(hipGetLastError());
    }
    const double* W = o->mel ? o->Bm : o->B;
    SN_TRY(set_w<double>(o->hp, W, o->Fs, 1));
    if (o->hb) SN_TRY(set_w<double>(o->hb, W, o->Fs, 1));  // (the one-launch plan of a fixed dictionary holds its own copy)
    return SNMF_OK;
}

extern "C" int snmf_online_stream_state_info(snmf_online* o, snmf_online_state_info* out) {
    if (!o || !out) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (o->f64) online_f64_state_info(o->f64, out);
    else online_state_info(o, out);
    return SNMF_OK;
}

extern "C" int snmf_online_get_state(snmf_online* o, void* record, int64_t cap) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (o->f64) return online_f64_get_state(o->f64, record, cap);
    return online_get_state(o, record, cap);
}

extern "C" int snmf_online_set_state(snmf_online* o, const void* record, int64_t bytes) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (o->f64) return online_f64_set_state(o->f64, record, bytes);
    return online_set_state(o, record, bytes);
}

extern "C" int snmf_online_restart_f32(snmf_online* o, const double* Bd, const double* Bmd, const float* H0, const float* Ad) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (o->f64) return fail(SNMF_ERR_STATE, "snmf_online_restart_f32 needs a separator made by snmf_online_create; an fp64 one takes snmf_online_restart_f64");
    if (Bmd && !o->mel) return fail(SNMF_ERR_STATE, "B_Mel_d given to a separator that is not in Mel mode");
    SN_TRY(online_restart_check(o));
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    if (Bmd) {  // the Mel master's noise columns; its mirror follows in om_refresh_dict
        const hipError_t e = hipMemcpyAsync(o->Bm + (size_t)o->n1 * o->p.R_x, Bmd, (size_t)o->n1 * o->p.R_d * 8, hipMemcpyHostToDevice, o->ctx->stream);
        if (e != hipSuccess) {
            o->failed = true;
            return fail(SNMF_ERR_NO_DEVICE, "restart: upload of B_Mel_d: %s", hipGetErrorString(e));
        }
    }
    return online_restart(o, Bd, H0, Ad);
}

extern "C" int snmf_online_restart_f64(snmf_online* o, const double* Bd, const double* Bmd, const double* H0, const double* Ad) {
    if (!o) return fail(SNMF_ERR_INVALID, "online handle is NULL");
    if (!o->f64) return fail(SNMF_ERR_STATE, "snmf_online_restart_f64 needs a separator made by snmf_online_create_f64");
    if (Bmd) return fail(SNMF_ERR_STATE, "B_Mel_d given to a separator that is not in Mel mode");
    return online_f64_restart(o->f64, Bd, H0, Ad);
}
