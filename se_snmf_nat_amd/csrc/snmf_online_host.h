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
// The calls are resolved at compile time (argument-dependent lookup on the handle type); nothing is dispatched at run time.
#pragma once
#include "snmf_internal.h"
#include "snmf_online_common.h"
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
    D(&o->adblk, (size_t)Ra * ma); D(&o->Vad, (size_t)F * ma); D(&o->Had, (size_t)Ra * ma); D(&o->win_s, (size_t)sz);
    D(&o->win_i, (size_t)sz); D(&o->tail, ntail); D(&o->tw, (size_t)N / 2);
    if (p->class_outputs) {
        D(&o->tail_x, ntail);
        D(&o->tail_d, ntail);
    }
    D(&o->rup, (size_t)Ra); D(&o->dev, (size_t)1);
    if (s == SNMF_OK && hipHostMalloc((void**)&o->h_status, sizeof(OnlineStatus)) != hipSuccess) s = fail(SNMF_ERR_NOMEM, "hipHostMalloc");
    return s;
}

// queued behind the mode's dictionary upload: start vector, windows, twiddles, the loop's scalars, zeroed rings and tails.
// The twiddle table `htw` is the caller's: it must stay alive until the caller has synchronised the stream.
template <class H, typename T = typename H::elem>
void online_upload_state(H* o, const T* H0, const T* win_stft, const T* win_istft, std::vector<ocplx<T>>& htw) {
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const int N = o->N, F = o->F, sz = p.framelength;
    const size_t ntail = (size_t)std::max(1, o->nov - 1) * sz;
    htw.resize(N / 2);
    for (int q = 0; q < N / 2; ++q) {
        const double ang = -2.0 * M_PI * (double)q / (double)N;
        htw[q].x = (T)cos(ang);
        htw[q].y = (T)sin(ang);
    }
    static const OnlineDev d0{0, 1, 0, 0};  // update_switch = 1 (src/init_buff.m:42)
    hipMemcpyAsync(o->H0, H0, (size_t)o->r * sizeof(T), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->win_s, win_stft, (size_t)sz * sizeof(T), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->win_i, win_istft, (size_t)sz * sizeof(T), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->tw, htw.data(), htw.size() * sizeof(ocplx<T>), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(o->dev, &d0, sizeof d0, hipMemcpyHostToDevice, st);
    hipMemsetAsync(o->lambda_dav, 0, (size_t)F * sizeof(T), st);
    hipMemsetAsync(o->Xm_tilde, 0, (size_t)F * sizeof(T), st);
    hipMemsetAsync(o->r_blk, 0, (size_t)F * o->Pl * sizeof(T), st);
    hipMemsetAsync(o->ldblk, 0, (size_t)F * o->ma * sizeof(T), st);
    hipMemsetAsync(o->adblk, 0, (size_t)o->Ra * o->ma * sizeof(T), st);
    hipMemsetAsync(o->tail, 0, ntail * sizeof(T), st);
    if (p.class_outputs) {
        hipMemsetAsync(o->tail_x, 0, ntail * sizeof(T), st);
        hipMemsetAsync(o->tail_d, 0, ntail * sizeof(T), st);
    }
    hipMemsetAsync(o->rup, 0, (size_t)o->Ra, st);
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
    void* ptrs[] = {o->B,     o->Bfix, o->Btmp,   o->H0,     o->lambda_dav, o->Xm_tilde, o->r_blk, o->ldblk, o->adblk, o->Vad, o->Had, o->win_s,
                    o->win_i, o->tail, o->tail_x, o->tail_d, o->tw,         o->rup,      o->dev,   o->cls,   o->tail_c};
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
