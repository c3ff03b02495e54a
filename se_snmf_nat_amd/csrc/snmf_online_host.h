// snmf_online_host.h -- the host driver of the single-stream online separator, shared by its two precisions
// (snmf_tu_online.hip: fp32, handle snmf_online; snmf_tu_online_f64.hip: fp64, handle OnlineF64).
// Host code only: no kernel and no device function lives here.
//
// The hop queue / history / flush logic of a process call, one run of frames (STFT, frame solves with the gated adaptation,
// inverse STFT and overlap-add of x_tilde, x_hat / d_hat and the class stack), the common call buffers, the class table,
// the trace and the shared part of creation.
//
// A mode's handle H derives from OnlineState<T> and defines, as overloads on H*, the steps that differ between the modes:
//   int om_reserve(H*, int cap), void om_free_call(H*)        the mode's own call buffers (cap frames)
//   int om_stft(H*, int n)                                    STFT of the run's n frames (fp32: with the Mel projection)
//   bool om_one_launch(const H*)                              all frame solves of a run in one launch (nothing adapts between frames)
//   int om_solve_run(H*, int n, const OnlineStatus** st)      solve + post-filter + class spectra of the whole run; *st: its n statuses (device)
//   int om_solve_frame(H*, int i, const OnlineStatus** st)    the same for frame i of the run; *st: its status (device)
//   int om_adapt(H*, int32_t* iters)                          adaptation solve, re-assembly and dictionary refresh
//   int om_istft(H*, const T* mag, int n, T* syn)             inverse STFT of n frames
//   int om_istft_class(H*, int c, int n, size_t syn_cs)       inverse STFT of class c of the class-major stack
//   int om_ola(H*, const T* syn, n, l0, i_first, n_out, T* out, int16_t* out16)   overlap-add to output hops
//   void om_state_mode(const H*, mel, mel_conv, n1)           get-state / set-state: the mode a record is taken under
//   int om_state_launch(H*, OStateArgs<T>, int64_t l, put)    k_ostate_get / _put (k_ostate_get64 / _put64); fp32 adds its Mel master
//   int om_refresh_dict(H*)                                   the solves' images of the dictionary masters, as creation leaves them
//                                                             (fp32: the fp32 mirrors and the plans' W; fp64: k_wnorm64)
// The calls are resolved at compile time (argument-dependent lookup on the handle type); nothing is dispatched at run time.
//
// The state g as a value, and the next file in place (the last section): snmf_online_stream_state_info / _get_state /
// _set_state and snmf_online_restart_* are online_state_info, online_get_state, online_set_state and online_restart here.
// The record is the batched separator's (include/snmf.h: snmf_online_state_info, snmf_online_state_field): its layout, its
// header checks and its host fields are defined once in this file (ostate_layout, ostate_check_record, ostate_write_host,
// ostate_read_host) and used by snmf_online_batch_host.h too, and the device arrays cross through the batch's ostate_xfer
// with a one-stream OStateArgs -- the single-stream arrays are the batch's with S = 1, and the post-filter both kinds of
// separator run (snmf_online_common.h) keeps the rings in the slots the record's order assumes.
#pragma once
#include "snmf_internal.h"
#include "snmf_online_common.h"
#include "snmf_online_batch_common.h"  // OStateArgs, the kSt* rows
#include "snmf_online_classes.h"

constexpr size_t kTraceCap = 1u << 16;  // diagnostics ring: the newest 65536 frames (~11 min at 100 frames/s)
constexpr int64_t kOnlineChunk = 4096;  // frames per device batch of a process call

// one frame's status as the trace holds it (the batched separator's trace too)
inline snmf_online_frame online_frame_record(const OnlineStatus& hs) {
    snmf_online_frame tr{};
    tr.n_iter = hs.n_iter; tr.trig = hs.trig; tr.n_up = hs.n_up; tr.beta = hs.beta; tr.A_x_mag = hs.A_x_mag; tr.A_d_mag = hs.A_d_mag;
    tr.Q_control = hs.Q_control;
    return tr;
}

// What the two modes' handles hold in common; T is the mode's element type (float / double).
template <typename T>
struct OnlineState {
    using elem = T;
    snmf_ctx* ctx = nullptr;
    snmf_online_params p{};
    int F = 0, r = 0, N = 0, nov = 0, Ra = 1, ma = 1, Pl = 1;
    // state, device
    double *B = nullptr, *Bfix = nullptr, *Btmp = nullptr;  // [B_DFT_x | B_DFT_d] (fp64 in both modes), the original B_DFT_d, scratch
    T *H0 = nullptr, *lambda_dav = nullptr, *Xm_tilde = nullptr, *r_blk = nullptr, *ldblk = nullptr, *adblk = nullptr, *Vad = nullptr,
      *Had = nullptr, *win_s = nullptr, *win_i = nullptr, *tail = nullptr, *tail_x = nullptr, *tail_d = nullptr;
    T* Ad0 = nullptr;  // [Ra][ma] Ad_blk as the stream last started with it (a restart without a new draw, the state record)
    ocplx<T>* tw = nullptr;
    uint8_t* rup = nullptr;
    OnlineDev* dev = nullptr;
    OnlineStatus* h_status = nullptr;  // pinned
    // per-call buffers (grown on demand)
    int cap_frames = 0;
    T *sig = nullptr, *Ym = nullptr, *Xt = nullptr, *Xh = nullptr, *Dh = nullptr, *syn = nullptr, *outf = nullptr;
    ocplx<T>* Yph = nullptr;
    int16_t* out16 = nullptr;
    // per-class outputs (set_classes): n_ev event classes then n_cls - n_ev noise classes; n_cls = 0: none set
    int n_ev = 0, n_cls = 0;
    int* cls = nullptr;   // [n_cls + 1] column ranges over [B_x | B_d] (snmf_online_classes.h)
    T* tail_c = nullptr;  // [n_cls][nov - 1 frames] one overlap-add tail per class
    T *Xc = nullptr, *syn_c = nullptr, *out_c = nullptr;  // per call, class-major: spectra, synthesis frames, hops
    // host state of the driver loop
    std::vector<T> pending, hist;
    int64_t l = 0;  // frames processed
    bool finished = false;
    bool failed = false;  // a device batch failed midway: frame counter, history and rings are no longer consistent
    std::deque<snmf_online_frame> trace;  // bounded: the newest kTraceCap frames (a real-time stream runs for days)
    // get-state / set-state: the staging record on the device (grown on demand)
    unsigned char* st_slab = nullptr;
    size_t st_cap = 0;
};

// ---- creation and destruction: the part the modes share -------------------------------------------------------------------
// dimensions, the shared device state and the pinned status
template <class H>
int online_alloc_state(H* o, snmf_ctx* ctx, const snmf_online_params* p) {
    o->ctx = ctx;
    o->p = *p;
    const int N = p->fftlength, F = N / 2 + 1, r = p->R_x + p->R_d, sz = p->framelength, hop = p->frameshift;
    o->F = F; o->r = r; o->N = N;
    o->nov = (sz + hop - 1) / hop;
    const int Ra = o->Ra = p->adapt_train_N ? p->R_a : 1, ma = o->ma = p->adapt_train_N ? p->m_a : 1, Pl = o->Pl = p->blk_sparse ? p->P_len_l : 1;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * sz;
    int s = SNMF_OK;
    auto D = [&](auto** ptr, size_t n) { if (s == SNMF_OK) s = dalloc(ptr, n); };
    D(&o->B, (size_t)F * r); D(&o->Bfix, (size_t)F * p->R_d); D(&o->Btmp, (size_t)F * p->R_d); D(&o->H0, (size_t)r);
    D(&o->lambda_dav, (size_t)F); D(&o->Xm_tilde, (size_t)F); D(&o->r_blk, (size_t)F * Pl); D(&o->ldblk, (size_t)F * ma);
    D(&o->adblk, (size_t)Ra * ma); D(&o->Ad0, (size_t)Ra * ma); D(&o->Vad, (size_t)F * ma); D(&o->Had, (size_t)Ra * ma); D(&o->win_s, (size_t)sz);
    D(&o->win_i, (size_t)sz); D(&o->tail, ntail); D(&o->tw, (size_t)N / 2);
    if (p->class_outputs) {
        D(&o->tail_x, ntail);
        D(&o->tail_d, ntail);
    }
    D(&o->rup, (size_t)Ra); D(&o->dev, (size_t)1);
    if (s == SNMF_OK && hipHostMalloc((void**)&o->h_status, sizeof(OnlineStatus)) != hipSuccess) s = fail(SNMF_ERR_NOMEM, "hipHostMalloc");
    return s;
}

// src/init_buff.m:17-42 for the arrays a recording changes: zeroed rings and tails, the loop's scalars, Ad_blk from the
// stream's draw (zeros without adaptation).  Creation and a restart queue exactly this.
template <class H, typename T = typename H::elem>
int online_reset_state(H* o) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const size_t F = o->F, ntail = (size_t)std::max(1, o->nov - 1) * p.framelength, nA = (size_t)o->Ra * o->ma;
    static const OnlineDev d0{0, 1, 0, 0};  // update_switch = 1 (src/init_buff.m:42)
    HIP_TRY(hipMemcpyAsync(o->dev, &d0, sizeof d0, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(o->lambda_dav, 0, F * sizeof(T), st));
    HIP_TRY(hipMemsetAsync(o->Xm_tilde, 0, F * sizeof(T), st));
    HIP_TRY(hipMemsetAsync(o->r_blk, 0, F * o->Pl * sizeof(T), st));
    HIP_TRY(hipMemsetAsync(o->ldblk, 0, F * o->ma * sizeof(T), st));
    if (p.adapt_train_N) HIP_TRY(hipMemcpyAsync(o->adblk, o->Ad0, nA * sizeof(T), hipMemcpyDeviceToDevice, st));  // rand(R_a, m_a) (:39)
    else HIP_TRY(hipMemsetAsync(o->adblk, 0, nA * sizeof(T), st));
    HIP_TRY(hipMemsetAsync(o->tail, 0, ntail * sizeof(T), st));
    if (p.class_outputs) {
        HIP_TRY(hipMemsetAsync(o->tail_x, 0, ntail * sizeof(T), st));
        HIP_TRY(hipMemsetAsync(o->tail_d, 0, ntail * sizeof(T), st));
    }
    if (o->tail_c) HIP_TRY(hipMemsetAsync(o->tail_c, 0, (size_t)o->n_cls * ntail * sizeof(T), st));
    HIP_TRY(hipMemsetAsync(o->rup, 0, (size_t)o->Ra, st));
    return SNMF_OK;
}

// queued behind the mode's dictionary upload: start vector, the Ad_blk draw (column-major R_a x m_a; NULL without adaptation),
// windows, twiddles, and the state of a recording's start.
// The twiddle table `htw` is the caller's: it must stay alive until the caller has synchronised the stream.
template <class H, typename T = typename H::elem>
void online_upload_state(H* o, const T* H0, const T* Ad0, const T* win_stft, const T* win_istft, std::vector<ocplx<T>>& htw) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const int N = o->N, sz = p.framelength;
    htw.resize(N / 2);
    for (int q = 0; q < N / 2; ++q) {
        const double ang = -2.0 * M_PI * (double)q / (double)N;
        htw[q].x = (T)cos(ang);
        htw[q].y = (T)sin(ang);
    }
    hipMemcpyAsync(o->H0, H0, (size_t)o->r * sizeof(T), hipMemcpyHostToDevice, st);
    if (p.adapt_train_N) hipMemcpyAsync(o->Ad0, Ad0, (size_t)o->Ra * o->ma * sizeof(T), hipMemcpyHostToDevice, st);
    else hipMemsetAsync(o->Ad0, 0, (size_t)o->Ra * o->ma * sizeof(T), st);
    hipMemcpyAsync(o->win_s, win_stft, (size_t)sz * sizeof(T), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->win_i, win_istft, (size_t)sz * sizeof(T), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->tw, htw.data(), htw.size() * sizeof(ocplx<T>), hipMemcpyHostToDevice, st);
    (void)online_reset_state(o);  // (a failure here is sticky: the caller's synchronise reports it)
}

template <class H>
void online_free_call_buffers(H* o) {
    om_free_call(o);
    void* ptrs[] = {o->sig, o->Ym, o->Xt, o->Xh, o->Dh, o->syn, o->outf, o->Yph, o->out16, o->Xc, o->syn_c, o->out_c};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->sig = o->Ym = o->Xt = o->Xh = o->Dh = o->syn = o->outf = o->Xc = o->syn_c = o->out_c = nullptr;
    o->Yph = nullptr;
    o->out16 = nullptr;
    o->cap_frames = 0;
}

// the call buffers, and everything online_alloc_state and online_install_classes allocated
template <class H>
void online_free_state(H* o) {
    online_free_call_buffers(o);
    void* ptrs[] = {o->B,     o->Bfix, o->Btmp,   o->H0,     o->lambda_dav, o->Xm_tilde, o->r_blk, o->ldblk, o->adblk, o->Vad,  o->Had,    o->win_s,
                    o->win_i, o->tail, o->tail_x, o->tail_d, o->tw,         o->rup,      o->dev,   o->cls,   o->tail_c, o->Ad0, o->st_slab};
    for (void* q : ptrs)
        if (q) hipFree(q);
    if (o->h_status) hipHostFree(o->h_status);
}

// call buffers for n frames
template <class H>
int online_reserve(H* o, int n) {
    if (n <= o->cap_frames) return SNMF_OK;
    hipStreamSynchronize(o->ctx->stream);
    online_free_call_buffers(o);
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
    if (o->n_cls) {
        SN_TRY(dalloc(&o->Xc, (size_t)o->n_cls * F * cap));
        SN_TRY(dalloc(&o->syn_c, (size_t)o->n_cls * (cap + o->nov - 1) * sz));
        SN_TRY(dalloc(&o->out_c, (size_t)o->n_cls * cap * hop));
    }
    SN_TRY(om_reserve(o, cap));
    o->cap_frames = cap;
    return SNMF_OK;
}

// ---- classes, dictionary and trace ----------------------------------------------------------------------------------------
// snmf_online_set_classes, first half: the state check and the class table `cls` of p.EVENT_RANK / p.NOISE_RANK
template <class H>
int online_class_table(const H* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num, const int32_t* noise_rank,
                       std::vector<int>* cls) {
    if (o->l != 0 || !o->pending.empty() || o->finished) return fail(SNMF_ERR_STATE, "snmf_online_set_classes must precede the first sample");
    return online_class_ranges(event_num, event_rank, noise_num, noise_rank, o->p.R_x, o->p.R_d, cls);
}

// ... second half: the table of nc classes (event_num of them event classes) and one tail per class on the device
template <class H>
int online_install_classes(H* o, const std::vector<int>& cls, int event_num, int nc) {
    using T = typename H::elem;
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    online_free_call_buffers(o);  // the class-major call buffers depend on the class count
    for (void** q : {(void**)&o->cls, (void**)&o->tail_c}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    o->n_ev = o->n_cls = 0;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * o->p.framelength;
    SN_TRY(dalloc(&o->cls, cls.size()));
    SN_TRY(dalloc(&o->tail_c, (size_t)nc * ntail));
    HIP_TRY(hipMemcpyAsync(o->cls, cls.data(), cls.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(o->tail_c, 0, (size_t)nc * ntail * sizeof(T), st));
    HIP_TRY(hipStreamSynchronize(st));
    o->n_ev = event_num;
    o->n_cls = nc;
    return SNMF_OK;
}

// the fp64 master of the current B_DFT_d (both modes hold one)
template <class H>
int online_get_basis_f64(H* o, double* Bd, int64_t ld) {
    if (ld < o->F) return fail(SNMF_ERR_INVALID, "ld < F");
    HIP_TRY(hipSetDevice(o->ctx->device));
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    HIP_TRY(hipMemcpy2D(Bd, (size_t)ld * 8, o->B + (size_t)o->F * o->p.R_x, (size_t)o->F * 8, (size_t)o->F * 8, (size_t)o->p.R_d,
                        hipMemcpyDeviceToHost));
    return SNMF_OK;
}

template <class H>
int online_trace_read(const H* o, snmf_online_frame* out, int64_t cap, int64_t* n) {
    if (n) *n = (int64_t)o->trace.size();
    if (out && cap > 0) std::copy_n(o->trace.begin(), (size_t)std::min<int64_t>(cap, (int64_t)o->trace.size()), out);
    return SNMF_OK;
}

template <class H>
void online_trace_push(H* o, const snmf_online_frame& tr) {
    o->trace.push_back(tr);
    if (o->trace.size() > kTraceCap) o->trace.pop_front();
}

// ---- kernel arguments that read the same in both modes --------------------------------------------------------------------
template <class H, typename T = typename H::elem>
OStftArgsT<T> online_stft_args(const H* o, int n) {
    const snmf_online_params& p = o->p;
    OStftArgsT<T> sa{};
    sa.sig = o->sig; sa.sz = p.framelength; sa.hop = p.frameshift; sa.dcbin = p.dcbin; sa.preemph = (T)p.preemph; sa.win = o->win_s; sa.tw = o->tw;
    sa.powv = (T)p.pow; sa.floorv = (T)p.nonzerofloor; sa.Ym = o->Ym; sa.Yph = o->Yph; sa.ld = o->F; sa.n_frames = n;
    return sa;
}

template <class H, typename T = typename H::elem>
OIstftArgsT<T> online_istft_args(const H* o, const T* mag, int n, T* syn) {
    const snmf_online_params& p = o->p;
    OIstftArgsT<T> ia{};
    ia.mag = mag; ia.ph = o->Yph; ia.ld = o->F; ia.n_frames = n; ia.sz = p.framelength; ia.dcb = p.dcbin_back; ia.powv = (T)p.pow;
    ia.scale = (T)(p.overlapscale / (double)o->N); ia.preemph = (T)p.preemph; ia.win = o->win_i; ia.tw = o->tw;
    ia.syn = syn;
    return ia;
}

// the post-filter's arguments for frame i of the run, the l-th of the stream: everything but the frame solve's results
// (A, hst, recon, a_stride, recon_len), the status slot, the frame count n, B and the Mel fields
template <class H, typename T = typename H::elem>
OPostArgsT<T> online_post_args(const H* o, int i, int64_t l) {
    const snmf_online_params& p = o->p;
    const int F = o->F;
    OPostArgsT<T> a{};
    a.Ym = o->Ym + (size_t)i * F; a.lambda_dav = o->lambda_dav; a.Xm_tilde = o->Xm_tilde;
    a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk; a.rup = o->rup; a.dev = o->dev;
    a.Xt_out = o->Xt + (size_t)i * F;
    a.Xh_out = o->Xh ? o->Xh + (size_t)i * F : nullptr;
    a.Dh_out = o->Dh ? o->Dh + (size_t)i * F : nullptr;
    a.F = F; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.Pk = p.P_len_k; a.dcbin = p.dcbin; a.gap = p.blk_gap;
    a.l = (int)std::min<int64_t>(l, 1 << 30);
    a.blk_sparse = p.blk_sparse; a.adapt = p.adapt_train_N; a.wiener = p.enhance_method == 0; a.init_N_len = p.init_N_len;
    a.switch_at = (int)std::floor(p.overlap_m_a * p.m_a);
    a.alpha_p = (T)p.alpha_p; a.alpha_eta = (T)p.alpha_eta; a.alpha_d = (T)p.alpha_d; a.beta0 = (T)p.beta;
    a.beta_max = (T)p.beta_max; a.Ar_up = (T)p.Ar_up; a.flr = (T)p.nonzerofloor;
    return a;
}

// ---- one run of frames ------------------------------------------------------------------------------------------------------
// n frames whose samples are sig = [history | n hops] (host); appends the hops the driver would write
template <class H, typename T = typename H::elem>
int online_run_frames(H* o, const std::vector<T>& sig, int n, std::vector<T>* outf, std::vector<int16_t>* out16, std::vector<T>* xh,
                      std::vector<T>* dh, std::vector<std::vector<T>>* xc) {
    const snmf_online_params& p = o->p;
    const int sz = p.framelength, hop = p.frameshift, nov = o->nov;
    hipStream_t st = o->ctx->stream;
    SN_TRY(online_reserve(o, n));
    HIP_TRY(hipMemcpyAsync(o->sig, sig.data(), sig.size() * sizeof(T), hipMemcpyHostToDevice, st));
    SN_TRY(om_stft(o, n));
    const OnlineStatus* d_st = nullptr;
    if (om_one_launch(o)) {
        // Fixed dictionary: nothing the host decides sits between frames.  All frame solves of the run in ONE launch, then
        // ONE post-filter launch walks the sequential recurrences.
        SN_TRY(om_solve_run(o, n, &d_st));
        std::vector<OnlineStatus> hst((size_t)n);
        HIP_TRY(hipMemcpyAsync(hst.data(), d_st, (size_t)n * sizeof(OnlineStatus), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (const OnlineStatus& hs : hst) online_trace_push(o, online_frame_record(hs));
    } else {
        for (int i = 0; i < n; ++i) {
            SN_TRY(om_solve_frame(o, i, &d_st));
            HIP_TRY(hipMemcpyAsync(o->h_status, d_st, sizeof(OnlineStatus), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const OnlineStatus hs = *o->h_status;
            snmf_online_frame tr = online_frame_record(hs);
            if (hs.do_solve && hs.n_up > 0) {
                int32_t it = 0;
                SN_TRY(om_adapt(o, &it));
                tr.solved = 1;
                tr.adapt_iters = it;
            }
            online_trace_push(o, tr);
        }
    }
    // inverse STFT of the n frames behind the nov-1 frames kept from the previous call, overlap-add
    const int l0 = (int)std::min<int64_t>(o->l + 1, 1 << 30);
    const int i_first = (int)std::max<int64_t>(0, (int64_t)p.delay + 1 - l0);
    const int n_out = std::max(0, n - i_first);
    auto fetch = [&](auto* v, const auto* src) -> int {  // the run's n_out hops behind what `v` holds
        const size_t at = v->size();
        v->resize(at + (size_t)n_out * hop);
        HIP_TRY(hipMemcpyAsync(v->data() + at, src, (size_t)n_out * hop * sizeof(*src), hipMemcpyDeviceToHost, st));
        return SNMF_OK;
    };
    auto synth = [&](const T* mag, std::vector<T>* of, std::vector<int16_t>* o16, T* tail) -> int {
        if (nov > 1) HIP_TRY(hipMemcpyAsync(o->syn, tail, (size_t)(nov - 1) * sz * sizeof(T), hipMemcpyDeviceToDevice, st));
        SN_TRY(om_istft(o, mag, n, o->syn + (size_t)(nov - 1) * sz));
        if (n_out > 0) {
            SN_TRY(om_ola(o, o->syn, n, l0, i_first, n_out, o->outf, o16 ? o->out16 : nullptr));
            if (of) SN_TRY(fetch(of, o->outf));
            if (o16) SN_TRY(fetch(o16, o->out16));
        }
        if (nov > 1) HIP_TRY(hipMemcpyAsync(tail, o->syn + (size_t)n * sz, (size_t)(nov - 1) * sz * sizeof(T), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SNMF_OK;
    };
    SN_TRY(synth(o->Xt, outf, out16, o->tail));
    if (p.class_outputs) {  // x_hat / d_hat of :350-361 (summed over the classes), same synthesis
        SN_TRY(synth(o->Xh, xh, nullptr, o->tail_x));
        SN_TRY(synth(o->Dh, dh, nullptr, o->tail_d));
    }
    if (o->n_cls) {
        // x_hat_i / d_hat_i (:356-361): the class-major stack through the inverse STFT, one overlap-add per class on its own
        // tail; the launches are queued back to back and synchronised once
        const int nc = o->n_cls;
        const size_t ntl = (size_t)(nov - 1) * sz, syn_cs = (size_t)(o->cap_frames + nov - 1) * sz, out_cs = (size_t)o->cap_frames * hop;
        if (nov > 1)
            HIP_TRY(hipMemcpy2DAsync(o->syn_c, syn_cs * sizeof(T), o->tail_c, ntl * sizeof(T), ntl * sizeof(T), (size_t)nc, hipMemcpyDeviceToDevice, st));
        for (int c = 0; c < nc; ++c) {
            SN_TRY(om_istft_class(o, c, n, syn_cs));
            if (n_out <= 0) continue;
            SN_TRY(om_ola(o, o->syn_c + (size_t)c * syn_cs, n, l0, i_first, n_out, o->out_c + (size_t)c * out_cs, (int16_t*)nullptr));
            if (xc) SN_TRY(fetch(&(*xc)[c], o->out_c + (size_t)c * out_cs));
        }
        if (nov > 1)
            HIP_TRY(hipMemcpy2DAsync(o->tail_c, ntl * sizeof(T), o->syn_c + (size_t)n * sz, syn_cs * sizeof(T), ntl * sizeof(T), (size_t)nc,
                                     hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    o->l += n;
    return SNMF_OK;
}

// ---- the process call -------------------------------------------------------------------------------------------------------
// snmf_online_process_* / _process_classes_* behind the handle checks (xhi / dhi: the class signals, class-major at `cap`)
template <class H, typename T = typename H::elem>
int online_process(H* o, const T* pcm, int64_t n, int flush, T* xt, int16_t* xt_i16, T* xh, T* dh, T* xhi, T* dhi, int64_t cap,
                   int64_t* n_out) {
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
    std::vector<T> of, ox, od;
    std::vector<int16_t> o16;
    // class signals: with a partition set they come from the class kernel; without one x_hat / d_hat are the one class per side
    const bool cls_set = o->n_cls > 0, want_c = cls_set && (xhi || dhi);
    std::vector<std::vector<T>> oc(want_c ? o->n_cls : 0);
    std::vector<T>* px = (xh || (xhi && !cls_set)) ? &ox : nullptr;
    std::vector<T>* pd = (dh || (dhi && !cls_set)) ? &od : nullptr;
    auto run = [&](const std::vector<T>& sig, int nb) -> int {
        const int rc = online_run_frames(o, sig, nb, xt ? &of : nullptr, xt_i16 ? &o16 : nullptr, px, pd, want_c ? &oc : nullptr);
        if (rc) o->failed = true;  // frames of this call were consumed and the device state advanced: never retry on it
        return rc;
    };
    const int64_t chunk = cls_set ? std::max<int64_t>(64, kOnlineChunk / o->n_cls) : kOnlineChunk;  // (class-major buffers grow with the classes)
    int64_t done = 0;
    while (done < nfr) {
        const int nb = (int)std::min(chunk, nfr - done);
        std::vector<T> sig(o->hist);
        sig.insert(sig.end(), o->pending.begin() + done * hop, o->pending.begin() + (done + nb) * hop);
        SN_TRY(run(sig, nb));
        o->hist.assign(sig.end() - (sz - hop), sig.end());
        done += nb;
    }
    o->pending.erase(o->pending.begin(), o->pending.begin() + nfr * hop);
    if (flush) {
        // a partial hop is dropped and delay+1 all-zero frames follow (src/NTF_sep_event_RT.m:69-76)
        SN_TRY(run(std::vector<T>((size_t)(sz - hop) + (size_t)tail_frames * hop, T(0)), (int)tail_frames));
        o->pending.clear();
        o->finished = true;
    }
    if (xt) std::memcpy(xt, of.data(), of.size() * sizeof(T));
    if (xt_i16) std::memcpy(xt_i16, o16.data(), o16.size() * 2);
    if (xh) std::memcpy(xh, ox.data(), ox.size() * sizeof(T));
    if (dh) std::memcpy(dh, od.data(), od.size() * sizeof(T));
    size_t nc_out = 0;
    if (cls_set) {
        for (int c = 0; c < (int)oc.size(); ++c) {
            T* dst = c < o->n_ev ? (xhi ? xhi + (size_t)c * cap : nullptr) : (dhi ? dhi + (size_t)(c - o->n_ev) * cap : nullptr);
            if (dst) std::memcpy(dst, oc[c].data(), oc[c].size() * sizeof(T));
            nc_out = std::max(nc_out, oc[c].size());
        }
    } else {
        if (xhi) std::memcpy(xhi, ox.data(), ox.size() * sizeof(T));
        if (dhi) std::memcpy(dhi, od.data(), od.size() * sizeof(T));
    }
    if (n_out) *n_out = (int64_t)std::max(std::max(std::max(of.size(), o16.size()), std::max(ox.size(), od.size())), nc_out);
    return SNMF_OK;
}

// ---------------------------------------------------------------------------------------------
// The state g as a record (include/snmf.h: snmf_online_state_info, snmf_online_state_field): [magic, version,
// snmf_online_state_info | the fields of snmf_online_state_field_id].  One definition of the layout, of the header checks
// and of the fields the host holds (l, the pending samples, the frame buffer) for both kinds of separator.
// ---------------------------------------------------------------------------------------------
struct OStateHeader {
    uint32_t magic, version;
    snmf_online_state_info info;
};
static_assert(sizeof(OStateHeader) == 80, "record header: 8 bytes and a tight snmf_online_state_info");

// The layout of a record under `q`: per field its byte offset, element count and snmf_online_state_type.  Every offset is a
// multiple of 8.  Returns the record's bytes, or -1 for an info no separator reports.
inline int64_t ostate_layout(const snmf_online_state_info& q, int64_t* off, int64_t* cnt, int32_t* typ) {
    if ((q.elem_size != 4 && q.elem_size != 8) || q.F < 1 || q.F_order < 0 || q.R_x < 1 || q.R_d < 1 || q.R_a < 1 || q.m_a < 1 ||
        q.P_len_l < 1 || q.frameshift < 1 || q.framelength < q.frameshift || q.ntail < 0 || q.n_classes < 0 || (q.mel && q.F_order < 1))
        return -1;
    const int32_t E = q.elem_size == 4 ? SNMF_STATE_F32 : SNMF_STATE_F64;
    const int64_t F = q.F, nt = q.ntail;
    struct Row { int f; int64_t n; int32_t t; };
    const Row rows[SNMF_STATE_FIELD_COUNT] = {
        // the scalars first, then the arrays
        {SNMF_STATE_N_PUSH, 1, SNMF_STATE_I32}, {SNMF_STATE_UPDATE_SWITCH, 1, SNMF_STATE_I32}, {SNMF_STATE_L, 1, SNMF_STATE_I64},
        {SNMF_STATE_PENDING_COUNT, 1, SNMF_STATE_I32},
        {SNMF_STATE_XM_TILDE, F, E}, {SNMF_STATE_LAMBDA_DAV, F, E}, {SNMF_STATE_R_BLK, F * q.P_len_l, E},
        {SNMF_STATE_LAMBDA_D_BLK, F * q.m_a, E}, {SNMF_STATE_AD_BLK, (int64_t)q.R_a * q.m_a, E},
        {SNMF_STATE_B_DFT_D, F * q.R_d, SNMF_STATE_F64}, {SNMF_STATE_B_FIX, F * q.R_d, SNMF_STATE_F64},
        {SNMF_STATE_B_MEL_D, q.mel ? (int64_t)q.F_order * q.R_d : 0, SNMF_STATE_F64},
        {SNMF_STATE_H0, (int64_t)q.R_x + q.R_d, E}, {SNMF_STATE_AD_BLK0, (int64_t)q.R_a * q.m_a, E},
        {SNMF_STATE_Y_HIST, (int64_t)q.framelength - q.frameshift, E}, {SNMF_STATE_PENDING, (int64_t)q.frameshift, E},
        {SNMF_STATE_X_TILDE_TAIL, nt, E}, {SNMF_STATE_X_HAT_TAIL, q.class_outputs ? nt : 0, E},
        {SNMF_STATE_D_HAT_TAIL, q.class_outputs ? nt : 0, E}, {SNMF_STATE_CLASS_TAILS, nt * q.n_classes, E},
    };
    int64_t at = (int64_t)sizeof(OStateHeader);
    for (const Row& w : rows) {
        const int64_t sz = (w.t == SNMF_STATE_F32 || w.t == SNMF_STATE_I32) ? 4 : 8;
        if (w.f == SNMF_STATE_UPDATE_SWITCH) at -= 4;  // n_push and update_switch are one pair of int32 (OnlineDev's head)
        off[w.f] = at;
        cnt[w.f] = w.n;
        typ[w.f] = w.t;
        at = (at + w.n * sz + 7) / 8 * 8;
    }
    return at;
}

// the info of a separator (single-stream or batched: both handles hold these members) in the given mode, record size included
template <class O>
void ostate_info_of(const O* o, int mel, int mel_conv, int n1, size_t ntail, snmf_online_state_info* q) {
    *q = snmf_online_state_info{};
    q->elem_size = (int32_t)sizeof(typename O::elem);
    q->mel = mel; q->mel_conv = mel_conv; q->F = o->F; q->F_order = mel ? n1 : 0;
    q->R_x = o->p.R_x; q->R_d = o->p.R_d; q->R_a = o->Ra; q->m_a = o->ma; q->P_len_l = o->Pl;
    q->framelength = o->p.framelength; q->frameshift = o->p.frameshift; q->ntail = (int32_t)ntail;
    q->class_outputs = o->p.class_outputs ? 1 : 0; q->n_classes = o->n_cls;
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    q->bytes = ostate_layout(*q, off, cnt, typ);
}

// Record i of the n consecutive records in `records` (`bytes` in all) against the info `q` of the handle (`owner`: "batch" /
// "separator") and its layout `off`: the checks snmf_online_batch_set_state documents, in their order.  Reads nothing else.
inline int ostate_check_record(const void* records, int64_t bytes, int i, int n, const snmf_online_state_info& q, const int64_t* off,
                               const char* owner) {
    const size_t rb = (size_t)q.bytes, total = rb * (size_t)n;
    // record i begins where the handle's record size puts it; a record of another size fails its header check below
    if (bytes < 0 || (uint64_t)bytes < (size_t)i * rb + sizeof(OStateHeader))
        return fail(SNMF_ERR_INVALID, "records holds %lld bytes: too few for the header of record %d", (long long)bytes, i);
    const unsigned char* rec = (const unsigned char*)records + (size_t)i * rb;
    OStateHeader h;
    std::memcpy(&h, rec, sizeof h);
    if (h.magic != SNMF_ONLINE_STATE_MAGIC) return fail(SNMF_ERR_INVALID, "record %d: not a stream state (bad magic)", i);
    if (h.version != SNMF_ONLINE_STATE_VERSION)
        return fail(SNMF_ERR_INVALID, "record %d: layout version %u, this library reads %d", i, h.version, SNMF_ONLINE_STATE_VERSION);
    const snmf_online_state_info& r = h.info;
#define OSTATE_SAME(field)                                                                                                      \
    if (r.field != q.field)                                                                                                     \
        return fail(SNMF_ERR_DIM, "record %d: " #field " = %d, the %s has " #field " = %d", i, (int)r.field, owner, (int)q.field);
    OSTATE_SAME(elem_size) OSTATE_SAME(mel) OSTATE_SAME(mel_conv) OSTATE_SAME(F) OSTATE_SAME(F_order) OSTATE_SAME(R_x) OSTATE_SAME(R_d)
    OSTATE_SAME(R_a) OSTATE_SAME(m_a) OSTATE_SAME(P_len_l) OSTATE_SAME(framelength) OSTATE_SAME(frameshift) OSTATE_SAME(ntail)
    OSTATE_SAME(class_outputs) OSTATE_SAME(n_classes)
#undef OSTATE_SAME
    if (r.bytes != q.bytes) return fail(SNMF_ERR_INVALID, "record %d: %lld bytes, the layout gives %lld", i, (long long)r.bytes, (long long)q.bytes);
    if ((uint64_t)bytes < (size_t)(i + 1) * rb)
        return fail(SNMF_ERR_INVALID, "records holds %lld bytes, %d records need %zu", (long long)bytes, n, total);
    int32_t dv[2], np;
    int64_t l;
    std::memcpy(dv, rec + off[SNMF_STATE_N_PUSH], 8);
    std::memcpy(&l, rec + off[SNMF_STATE_L], 8);
    std::memcpy(&np, rec + off[SNMF_STATE_PENDING_COUNT], 4);
    if (dv[0] < 0) return fail(SNMF_ERR_INVALID, "record %d: n_push = %d", i, dv[0]);
    if (dv[1] < 1) return fail(SNMF_ERR_INVALID, "record %d: update_switch = %d", i, dv[1]);
    if (l < 1) return fail(SNMF_ERR_INVALID, "record %d: l = %lld", i, (long long)l);
    if (np < 0 || np >= q.frameshift) return fail(SNMF_ERR_INVALID, "record %d: %d pending samples at frameshift %d", i, np, q.frameshift);
    return SNMF_OK;
}

// What the host adds to a record the gather kernel has filled: the header, zeros wherever no field lies (two gets of one
// state are the same bytes), and the stream's host state: l (the frames processed; the record holds the next frame's
// 1-based index), the samples not yet framed and the frame buffer.
template <typename T>
void ostate_write_host(unsigned char* rec, const snmf_online_state_info& q, int64_t l_done, const std::vector<T>& pending,
                       const std::vector<T>& hist) {
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    ostate_layout(q, off, cnt, typ);
    const size_t rb = (size_t)q.bytes;
    std::vector<std::pair<int64_t, int64_t>> span;  // [begin, end) of every field, in record order
    for (int f = 0; f < SNMF_STATE_FIELD_COUNT; ++f)
        span.push_back({off[f], off[f] + cnt[f] * ((typ[f] == SNMF_STATE_F32 || typ[f] == SNMF_STATE_I32) ? 4 : 8)});
    std::sort(span.begin(), span.end());
    OStateHeader h{};
    h.magic = SNMF_ONLINE_STATE_MAGIC;
    h.version = SNMF_ONLINE_STATE_VERSION;
    h.info = q;
    std::memcpy(rec, &h, sizeof h);
    int64_t at = (int64_t)sizeof h;
    for (const auto& sp : span) {  // the gaps between fields
        if (sp.first > at) std::memset(rec + at, 0, (size_t)(sp.first - at));
        at = std::max(at, sp.second);
    }
    if ((int64_t)rb > at) std::memset(rec + at, 0, rb - (size_t)at);
    const int64_t l = l_done + 1;
    const int32_t np = (int32_t)pending.size();
    std::memcpy(rec + off[SNMF_STATE_L], &l, 8);
    std::memcpy(rec + off[SNMF_STATE_PENDING_COUNT], &np, 4);
    T* hs = (T*)(rec + off[SNMF_STATE_Y_HIST]);
    T* pd = (T*)(rec + off[SNMF_STATE_PENDING]);
    std::fill_n(hs, (size_t)cnt[SNMF_STATE_Y_HIST], T(0));
    std::copy(hist.begin(), hist.end(), hs);
    std::fill_n(pd, (size_t)cnt[SNMF_STATE_PENDING], T(0));
    std::copy(pending.begin(), pending.end(), pd);
}

// ... and what the host takes from a checked record
template <typename T>
void ostate_read_host(const unsigned char* rec, const snmf_online_state_info& q, int64_t* l_done, std::vector<T>* pending, std::vector<T>* hist) {
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    ostate_layout(q, off, cnt, typ);
    int64_t l;
    int32_t np;
    std::memcpy(&l, rec + off[SNMF_STATE_L], 8);
    std::memcpy(&np, rec + off[SNMF_STATE_PENDING_COUNT], 4);
    const T* hs = (const T*)(rec + off[SNMF_STATE_Y_HIST]);
    const T* pd = (const T*)(rec + off[SNMF_STATE_PENDING]);
    hist->assign(hs, hs + cnt[SNMF_STATE_Y_HIST]);
    pending->assign(pd, pd + np);
    *l_done = l - 1;
}

// the rows of a record under `q` as the transfer kernels address them (ostate_xfer, snmf_online_batch_common.h)
template <typename T>
void ostate_arg_offsets(const snmf_online_state_info& q, OStateArgs<T>* a) {
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    ostate_layout(q, off, cnt, typ);
    a->stride = q.bytes; a->off_l = off[SNMF_STATE_L];
    a->off[kStXm] = off[SNMF_STATE_XM_TILDE]; a->off[kStLam] = off[SNMF_STATE_LAMBDA_DAV]; a->off[kStRblk] = off[SNMF_STATE_R_BLK];
    a->off[kStLdblk] = off[SNMF_STATE_LAMBDA_D_BLK]; a->off[kStAdblk] = off[SNMF_STATE_AD_BLK]; a->off[kStBd] = off[SNMF_STATE_B_DFT_D];
    a->off[kStBfix] = off[SNMF_STATE_B_FIX]; a->off[kStBmd] = off[SNMF_STATE_B_MEL_D]; a->off[kStH0] = off[SNMF_STATE_H0];
    a->off[kStAd0] = off[SNMF_STATE_AD_BLK0]; a->off[kStTail] = off[SNMF_STATE_X_TILDE_TAIL]; a->off[kStTailX] = off[SNMF_STATE_X_HAT_TAIL];
    a->off[kStTailD] = off[SNMF_STATE_D_HAT_TAIL]; a->off[kStTailC] = off[SNMF_STATE_CLASS_TAILS]; a->off[kStDev] = off[SNMF_STATE_N_PUSH];
    a->off[kStBdf] = 0;
}

// ---------------------------------------------------------------------------------------------
// The single-stream separator: its state g out and in, and its next file in place.
// ---------------------------------------------------------------------------------------------
template <class H>
size_t online_ntail(const H* o) {
    return (size_t)std::max(1, o->nov - 1) * o->p.framelength;
}

template <class H>
void online_state_info(const H* o, snmf_online_state_info* q) {
    int mel = 0, mel_conv = 0, n1 = 0;
    om_state_mode(o, &mel, &mel_conv, &n1);
    ostate_info_of(o, mel, mel_conv, n1, online_ntail(o), q);
}

// the kernels' view of the separator and of a record under `q`: the batch's arrays with S = 1 (the kernels supply the slot
// list {0}; Bm, Bdf and n1 stay NULL / 0 here, the fp32 unit's om_state_launch sets its Mel master)
template <class H, typename T = typename H::elem>
OStateArgs<T> online_state_args(H* o, const snmf_online_state_info& q) {
    OStateArgs<T> a{};
    ostate_arg_offsets(q, &a);
    a.slab = o->st_slab;
    a.Xm_tilde = o->Xm_tilde; a.lambda_dav = o->lambda_dav; a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk; a.H0 = o->H0;
    a.Ad0 = o->Ad0; a.tail = o->tail; a.tail_x = o->tail_x; a.tail_d = o->tail_d; a.tail_c = o->n_cls ? o->tail_c : nullptr;
    a.B = o->B; a.Bfix = o->Bfix; a.dev = o->dev;
    a.S = 1; a.F = o->F; a.r = o->r; a.Rx = o->p.R_x; a.Rd = o->p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.n_cls = o->n_cls;
    a.ntail = (int64_t)online_ntail(o);
    return a;
}

template <class H>
int online_state_slab(H* o, size_t bytes) {
    if (bytes <= o->st_cap) return SNMF_OK;
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    if (o->st_slab) HIP_TRY(hipFree(o->st_slab));
    o->st_slab = nullptr;
    o->st_cap = 0;
    SN_TRY(dalloc(&o->st_slab, bytes));
    o->st_cap = bytes;
    return SNMF_OK;
}

// snmf_online_get_state behind the handle checks: one gather launch, one copy; the separator is not disturbed
template <class H, typename T = typename H::elem>
int online_get_state(H* o, void* record, int64_t cap) {
    if (!record) return fail(SNMF_ERR_INVALID, "record is NULL");
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a batch; the separator state is not reusable, create a new one");
    if (o->finished)
        return fail(SNMF_ERR_STATE, "the stream was flushed: what survives it is its dictionary (snmf_online_get_basis_f64); restart it or set a state");
    snmf_online_state_info q;
    online_state_info(o, &q);
    if (cap < 0 || (uint64_t)cap < (uint64_t)q.bytes)
        return fail(SNMF_ERR_INVALID, "record holds %lld bytes, the state needs %lld", (long long)cap, (long long)q.bytes);
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    SN_TRY(online_state_slab(o, (size_t)q.bytes));
    SN_TRY(om_state_launch(o, online_state_args(o, q), o->l + 1, false));
    HIP_TRY(hipMemcpyAsync(record, o->st_slab, (size_t)q.bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ostate_write_host<T>((unsigned char*)record, q, o->l, o->pending, o->hist);
    return SNMF_OK;
}

// snmf_online_set_state behind the handle checks: the header against the handle before the device is touched, then one
// upload, one scatter launch and the dictionary refresh of a creation
template <class H, typename T = typename H::elem>
int online_set_state(H* o, const void* record, int64_t bytes) {
    if (!record) return fail(SNMF_ERR_INVALID, "record is NULL");
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a batch; the separator state is not reusable, create a new one");
    snmf_online_state_info q;
    online_state_info(o, &q);
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    ostate_layout(q, off, cnt, typ);
    SN_TRY(ostate_check_record(record, bytes, 0, 1, q, off, "separator"));
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    SN_TRY(online_state_slab(o, (size_t)q.bytes));
    auto device = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(o->st_slab, record, (size_t)q.bytes, hipMemcpyHostToDevice, st));
        SN_TRY(om_state_launch(o, online_state_args(o, q), 0, true));  // (l: the record holds it)
        SN_TRY(om_refresh_dict(o));
        HIP_TRY(hipStreamSynchronize(st));  // the caller's buffer is free, and a fault is this call's
        return SNMF_OK;
    };
    if (int rc = device()) {
        o->failed = true;  // the stream may be half written
        return rc;
    }
    ostate_read_host<T>((const unsigned char*)record, q, &o->l, &o->pending, &o->hist);
    o->finished = false;
    o->trace.clear();  // the trace goes on from frame l
    return SNMF_OK;
}

// a restart's state check: not in the middle of a recording
template <class H>
int online_restart_check(const H* o) {
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a batch; the separator state is not reusable, create a new one");
    if (!o->finished && (o->l > 0 || !o->pending.empty()))
        return fail(SNMF_ERR_STATE, "the stream is in the middle of a recording; flush it before a restart");
    return SNMF_OK;
}

// The next file in place (src/NTF_sep_event_RT.m:27-38 + src/init_buff.m), behind online_restart_check and the mode's own
// uploads (fp32: a new B_Mel_d): Bd F x Rd fp64 or NULL (carry: the master and the fixed columns of :328 stay), H0 r or NULL,
// Ad Ra x ma or NULL (the values the stream last started with).  Everything else returns to what creation gives.  Ordered
// on ctx->stream, no synchronise (the uploads come from pageable host memory, which the runtime copies before it returns).
template <class H, typename T = typename H::elem>
int online_restart(H* o, const double* Bd, const T* H0, const T* Ad) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const size_t nD = (size_t)o->F * p.R_d;
    auto device = [&]() -> int {
        if (Bd) {
            HIP_TRY(hipMemcpyAsync(o->B + (size_t)o->F * p.R_x, Bd, nD * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(o->Bfix, Bd, nD * 8, hipMemcpyHostToDevice, st));  // B_Mel_d in DFT mode (:328)
        }
        if (H0) HIP_TRY(hipMemcpyAsync(o->H0, H0, (size_t)o->r * sizeof(T), hipMemcpyHostToDevice, st));
        if (Ad && p.adapt_train_N) HIP_TRY(hipMemcpyAsync(o->Ad0, Ad, (size_t)o->Ra * o->ma * sizeof(T), hipMemcpyHostToDevice, st));
        SN_TRY(online_reset_state(o));
        return om_refresh_dict(o);
    };
    if (int rc = device()) {
        o->failed = true;  // the stream may be half reset
        return rc;
    }
    o->pending.clear();
    o->hist.assign((size_t)(p.framelength - p.frameshift), T(0));
    o->l = 0;
    o->finished = false;
    o->trace.clear();
    return SNMF_OK;
}
