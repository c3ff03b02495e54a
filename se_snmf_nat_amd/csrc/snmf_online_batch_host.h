// snmf_online_batch_host.h -- the host driver of the batched online separator, shared by its two precisions
// (snmf_tu_online_batch.hip: fp32, handle snmf_online_batch; snmf_tu_online_batch_f64.hip: fp64, handle OnlineBatchF64).
// Host code only: no kernel or device function is defined here.  The kernel templates both modes share are defined in
// snmf_online_batch_common.h, and the driver launches them with the mode's element type.
//
// Per stream, the hop queue / history / flush logic of snmf_online_process_f32 (snmf_online_host.h); on the device, one fixed
// sequence of launches per frame step for all streams (frame solve, post-filter, class spectra, gated adaptation) -- with
// the dictionary fixed, one launch of each for the whole chunk.  A chunk synchronises ONCE: outputs, statuses and
// adaptation verdicts are copied back together at its end.
//
// A mode's handle H derives from OBatchState<T> and defines, as overloads on H*, the steps that differ between the modes:
//   int obm_chunk_frames(const H*)                               frames per stream of one device chunk
//   int obm_reserve(H*, size_t slots), void obm_free_chunk(H*)   the mode's own chunk buffers (slots = C * S)
//   int obm_begin_chunk(H*, fr, C)                               STFT of the chunk (fp32: with the Mel projection) and the chunk's post-filter arguments
//   int obm_frame_solve(H*, fr, step, C)                         frame `step` of every stream; step < 0: all C frames
//   int obm_post(H*, fr, step)                                   likewise
//   int obm_class_spectra(H*, fr, step, C)                       likewise (only with a class partition set)
//   int obm_adapt(H*, fr, step)                                  adaptation + re-assembly + dictionary refresh behind frame `step`
//   size_t obm_lds_fft(const H*)                                 dynamic LDS of the inverse STFT's two FFT buffers (fp32: 0, they are static)
//   void obm_state_mode(const H*, mel, mel_conv, n1)             get-state / set-state: the mode a record is taken under
//   int obm_state_launch(H*, const OStateArgs<T>&, n, put)       k_obstate_get / _put (k_obstate_get64 / _put64); fp32 adds its Mel masters (Bm, Bdf, n1: NULL / 0 as they come)
//   int obm_state_refresh(H*, n)                                 the dictionary images of the streams in rs_slots, as a restart's
//   void obm_state_installed(H*, n, slots)                       the mode's own host state behind a set
// A restart is obatch_restart: the mode uploads what is its own, then passes the launch of its restart kernel.
// The calls are resolved at compile time (argument-dependent lookup on the handle type); nothing is dispatched at run time.
#pragma once
#include "snmf_internal.h"
#include "snmf_online_batch_common.h"
#include "snmf_online_classes.h"  // by_logn: the FFT-size dispatch of the inverse STFT
#include "snmf_online_host.h"  // online_frame_record: a frame's status as the trace holds it

constexpr size_t kBTraceCap = 1u << 16;   // per stream: the newest 65536 frames, as snmf_online_trace
constexpr int64_t kBChunkSlots = 16384;  // (frame, stream) slots of one device chunk

// What the two modes' handles hold in common; T is the mode's element type (float / double).
template <typename T>
struct OBatchState {
    using elem = T;
    snmf_ctx* ctx = nullptr;
    snmf_online_params p{};
    int S = 0, F = 0, r = 0, N = 0, nov = 0, Ra = 1, ma = 1, Pl = 1;
    bool started = false;  // a process call was made (set_mel / set_classes must come first)
    bool failed = false;
    size_t ntail = 0;
    // per stream, device: the fp64 dictionaries [B_DFT_x | B_DFT_d] [S][r][F], the noise dictionary each stream started with
    // and the re-assembly's scratch [S][Rd][F]; H0 [S][r], Ad_blk0 [S][Ra][ma] and the post-filter's state and rings
    double *B = nullptr, *Bfix = nullptr, *Btmp = nullptr;
    T *H0 = nullptr, *Ad0 = nullptr, *lambda_dav = nullptr, *Xm_tilde = nullptr, *r_blk = nullptr, *ldblk = nullptr, *adblk = nullptr;
    T *tail = nullptr, *tail_x = nullptr, *tail_d = nullptr;
    uint8_t* rup = nullptr;
    OnlineDev* dev = nullptr;
    double* Bxd = nullptr;       // B_DFT_x in fp64 as a recording starts with it: fp32 one [Rx][F] for all, fp64 [S][Rx][F]
    T *win_s = nullptr, *win_i = nullptr;  // shared: the analysis / synthesis windows and the FFT's twiddles
    ocplx<T>* tw = nullptr;
    int* rs_slots = nullptr;     // restart uploads (sized for all S streams)
    double* rs_B = nullptr;
    T *rs_H = nullptr, *rs_A = nullptr;
    int* meta_i = nullptr;       // [6][S] nfr, nreal, l0, i_first, n_out, (pad)
    int64_t* meta_l = nullptr;   // [3][S] off, zoff, out_off
    // per-class outputs (set_classes): n_ev event classes then n_cls - n_ev noise classes; n_cls = 0: none set
    int n_ev = 0, n_cls = 0;
    int* cls = nullptr;          // [n_cls + 1] column ranges over [B_x | B_d] (snmf_online_classes.h)
    T* tail_c = nullptr;         // [n_cls][S][ntail] one overlap-add tail per class and stream
    // per chunk, device (grown on demand)
    int C = 0;  // frames per stream per chunk
    size_t cap_sig = 0, cap_out = 0;
    T *sig = nullptr, *Ym = nullptr, *Xt = nullptr, *Xh = nullptr, *Dh = nullptr, *syn = nullptr, *outf = nullptr;
    ocplx<T>* Yph = nullptr;
    int16_t* out16 = nullptr;
    T *Xc = nullptr, *out_c = nullptr;  // class-major: spectra [n_cls][C * S][F], hops [n_cls][cap_out]
    OnlineStatus* status = nullptr;
    int* iters = nullptr;
    // host state, per stream
    std::vector<std::vector<T>> pending, hist;
    std::vector<int64_t> l;
    std::vector<uint8_t> finished;
    std::vector<std::deque<snmf_online_frame>> trace;
    // a mode with settings per stream lists here which streams adapt; empty: p.adapt_train_N holds for every stream
    std::vector<uint8_t> adapt_s;
    // get-state / set-state: the staging slab of records (grown on demand)
    unsigned char* st_slab = nullptr;
    size_t st_cap = 0;
};

// stream s runs the noise-dictionary adaptation / any stream does (the launch structure of a chunk follows the latter)
template <class H>
bool obatch_adapts(const H* o, int s) {
    return o->adapt_s.empty() ? o->p.adapt_train_N != 0 : o->adapt_s[s] != 0;
}
template <class H>
bool obatch_any_adapts(const H* o) {
    if (o->adapt_s.empty()) return o->p.adapt_train_N != 0;
    return std::any_of(o->adapt_s.begin(), o->adapt_s.end(), [](uint8_t v) { return v != 0; });
}

// one stream's output hops of a process call
template <typename T>
struct OBatchSink {
    std::vector<T> f, x, d;
    std::vector<int16_t> i16;
    std::vector<std::vector<T>> c;  // [n_cls] the class signals
};

template <class H>
void obatch_free_chunk(H* o) {
    obm_free_chunk(o);
    void* ptrs[] = {o->sig, o->Ym, o->Xt, o->Xh, o->Dh, o->syn, o->outf, o->Yph, o->out16, o->status, o->iters, o->Xc, o->out_c};
    for (void* q : ptrs)
        if (q) hipFree(q);
    o->sig = o->Ym = o->Xt = o->Xh = o->Dh = o->syn = o->outf = o->Xc = o->out_c = nullptr;
    o->Yph = nullptr;
    o->out16 = nullptr;
    o->status = nullptr;
    o->iters = nullptr;
    o->C = 0;
    o->cap_sig = o->cap_out = 0;
}

// every device array of OBatchState (a mode's destroy frees its own besides)
template <class H>
void obatch_free_state(H* o) {
    obatch_free_chunk(o);
    void* ptrs[] = {o->B, o->Bfix, o->Btmp, o->H0, o->Ad0, o->lambda_dav, o->Xm_tilde, o->r_blk, o->ldblk, o->adblk, o->tail, o->tail_x,
                    o->tail_d, o->rup, o->dev, o->Bxd, o->win_s, o->win_i, o->tw, o->rs_slots, o->rs_B, o->rs_H, o->rs_A, o->meta_i,
                    o->meta_l, o->cls, o->tail_c, o->st_slab};
    for (void* q : ptrs)
        if (q) hipFree(q);
}

// chunk buffers for C frames per stream and the given signal / output sizes
template <class H>
int obatch_reserve(H* o, int C, size_t n_sig, size_t n_out) {
    if (C <= o->C && n_sig <= o->cap_sig && n_out <= o->cap_out) return SNMF_OK;
    hipStreamSynchronize(o->ctx->stream);
    C = std::max(C, o->C);
    n_sig = std::max(n_sig, o->cap_sig);
    n_out = std::max(n_out, o->cap_out);
    obatch_free_chunk(o);
    const size_t slots = (size_t)C * o->S, F = o->F, sz = o->p.framelength;
    SN_TRY(dalloc(&o->sig, n_sig));
    SN_TRY(dalloc(&o->Ym, F * slots));
    SN_TRY(dalloc(&o->Yph, F * slots));
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
    SN_TRY(dalloc(&o->status, slots));
    SN_TRY(dalloc(&o->iters, slots));
    SN_TRY(obm_reserve(o, slots));
    o->C = C;
    o->cap_sig = n_sig;
    o->cap_out = n_out;
    return SNMF_OK;
}

// set_classes behind the mode's own checks: the class table `cls` (online_class_ranges) of event_num + noise_num classes
template <class H>
int obatch_install_classes(H* o, const std::vector<int>& cls, int event_num, int nc) {
    using T = typename H::elem;
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    obatch_free_chunk(o);  // the class-major chunk buffers depend on the class count
    for (void** q : {(void**)&o->cls, (void**)&o->tail_c}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    o->n_ev = o->n_cls = 0;
    const size_t nt = (size_t)nc * o->S * o->ntail;
    SN_TRY(dalloc(&o->cls, cls.size()));
    SN_TRY(dalloc(&o->tail_c, nt));
    HIP_TRY(hipMemcpyAsync(o->cls, cls.data(), cls.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(o->tail_c, 0, nt * sizeof(T), st));
    HIP_TRY(hipStreamSynchronize(st));
    o->n_ev = event_num;
    o->n_cls = nc;
    return SNMF_OK;
}

// a restart's argument checks: the listed slots are valid, distinct and not in the middle of a recording
template <class H>
int obatch_restart_check(const H* o, int32_t n, const int32_t* slots) {
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
    return SNMF_OK;
}

// what a corpus run (snmf_online_batch_chains.h) must find: a batch that has not failed, with no stream in the middle of a recording
template <class H>
int obatch_idle_check(const H* o) {
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    for (int s = 0; s < o->S; ++s)
        if (!o->finished[s] && (o->l[s] > 0 || !o->pending[s].empty()))
            return fail(SNMF_ERR_STATE, "stream %d is in the middle of a recording; flush it before a run over chains", s);
    return SNMF_OK;
}

// the host state of streams that start a new recording (src/init_buff.m)
template <class H>
void obatch_restart_host(H* o, int n, const int32_t* slots) {
    const int sz = o->p.framelength, hop = o->p.frameshift;
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        o->pending[s].clear();
        o->hist[s].assign((size_t)(sz - hop), typename H::elem(0));
        o->l[s] = 0;
        o->finished[s] = 0;
        o->trace[s].clear();
    }
}

// The streams slots[0..n) start a new recording (src/NTF_sep_event_RT.m:27-38 + src/init_buff.m): the uploads, the mode's
// restart kernel (launch(a): orestart_common on `a`, plus the mode's own arrays), the class tails, one refresh over the
// streams' columns, and their host state.  Arguments are checked by the caller, and what is the mode's own (fp32: the Mel
// uploads; fp64: the settings entries and event dictionaries) is on the stream already.  Bd is n x Rd x F fp64 or NULL
// (carry), H0 n x r or NULL, Ad n x Ra x ma or NULL; sBx is the stride of Bxd per stream (0: one dictionary for all).
// Ordered on ctx->stream, no synchronise (the uploads come from pageable host memory, which the runtime copies before it
// returns).
template <class H, class Launch>
int obatch_restart(H* o, int n, const int32_t* slots, const double* Bd, const typename H::elem* H0, const typename H::elem* Ad, int64_t sBx,
                   Launch launch) {
    using T = typename H::elem;
    const snmf_online_params& p = o->p;
    hipStream_t st = o->ctx->stream;
    const size_t F = o->F, nA = (size_t)o->Ra * o->ma;
    HIP_TRY(hipMemcpyAsync(o->rs_slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (Bd) HIP_TRY(hipMemcpyAsync(o->rs_B, Bd, (size_t)n * p.R_d * F * 8, hipMemcpyHostToDevice, st));
    if (H0) HIP_TRY(hipMemcpyAsync(o->rs_H, H0, (size_t)n * o->r * sizeof(T), hipMemcpyHostToDevice, st));
    if (Ad) HIP_TRY(hipMemcpyAsync(o->rs_A, Ad, (size_t)n * nA * sizeof(T), hipMemcpyHostToDevice, st));
    ORestartCommon<T> a{};
    a.slots = o->rs_slots; a.Bx = o->Bxd; a.sBx = sBx; a.Bd = Bd ? o->rs_B : nullptr; a.H0n = H0 ? o->rs_H : nullptr;
    a.Adn = Ad ? o->rs_A : nullptr; a.B = o->B; a.Bfix = o->Bfix; a.H0 = o->H0; a.Ad0 = o->Ad0; a.adblk = o->adblk; a.ldblk = o->ldblk;
    a.lambda_dav = o->lambda_dav; a.Xm_tilde = o->Xm_tilde; a.r_blk = o->r_blk; a.tail = o->tail; a.tail_x = o->tail_x;
    a.tail_d = o->tail_d; a.rup = o->rup; a.dev = o->dev;
    a.F = o->F; a.r = o->r; a.Rx = p.R_x; a.Rd = p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.ntail = (int64_t)o->ntail;
    launch(a);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < n && o->tail_c; ++i)  // the class tails of the stream, like tail_x / tail_d: one strided fill over its classes
        HIP_TRY(hipMemset2DAsync(o->tail_c + (size_t)slots[i] * o->ntail, (size_t)o->S * o->ntail * sizeof(T), 0, o->ntail * sizeof(T),
                                 (size_t)o->n_cls, st));
    SN_TRY(obm_state_refresh(o, n));
    obatch_restart_host(o, n, slots);
    return SNMF_OK;
}

template <class H>
int obatch_trace(const H* o, int32_t k, snmf_online_frame* out, int64_t cap, int64_t* n) {
    if (k < 0 || k >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", k, o->S);
    const auto& tr = o->trace[k];
    if (n) *n = (int64_t)tr.size();
    if (out && cap > 0) std::copy_n(tr.begin(), (size_t)std::min<int64_t>(cap, (int64_t)tr.size()), out);
    return SNMF_OK;
}

// One device chunk: stream s runs nfr[s] frames (its next nreal[s] PCM frames, then nfr - nreal flush frames).  Appends
// every stream's output hops and trace records.
template <class H>
int obatch_run_chunk(H* o, const std::vector<int>& nfr, const std::vector<int>& nreal, const std::vector<int64_t>& consumed, bool want_f,
                     bool want_i16, bool want_cls, bool want_ci, std::vector<OBatchSink<typename H::elem>>& sink) {
    using T = typename H::elem;
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
    std::vector<T> sig(std::max<size_t>(n_sig, 1), T(0));
    for (int s = 0; s < S; ++s) {
        if (nreal[s] <= 0) continue;
        T* d = sig.data() + h_off[s];
        std::copy(o->hist[s].begin(), o->hist[s].end(), d);
        std::copy(o->pending[s].begin() + consumed[s] * hop, o->pending[s].begin() + (consumed[s] + nreal[s]) * hop, d + (sz - hop));
    }
    SN_TRY(obatch_reserve(o, C, sig.size(), n_out));
    HIP_TRY(hipMemcpyAsync(o->sig, sig.data(), sig.size() * sizeof(T), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->meta_i, mi.data(), mi.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->meta_l, ml.data(), ml.size() * 8, hipMemcpyHostToDevice, st));
    OBatchFrames fr{};
    fr.nfr = o->meta_i; fr.nreal = o->meta_i + S; fr.l0 = o->meta_i + 2 * S; fr.off = o->meta_l; fr.zoff = o->meta_l + S; fr.S = S;
    const int* d_if = o->meta_i + 3 * S;
    const int* d_no = o->meta_i + 4 * S;
    const int64_t* d_oo = o->meta_l + 2 * S;
    SN_TRY(obm_begin_chunk(o, fr, C));  // STFT of every frame of the chunk; the post-filter's arguments for its launches below
    HIP_TRY(hipMemsetAsync(o->iters, 0, (size_t)C * S * 4, st));
    if (!obatch_any_adapts(o)) {
        // fixed dictionaries: every frame solve of the chunk in one launch, then one post-filter launch walks the frames
        SN_TRY(obm_frame_solve(o, fr, -1, C));
        SN_TRY(obm_post(o, fr, -1));
        if (o->n_cls) SN_TRY(obm_class_spectra(o, fr, -1, C));
    } else {
        for (int i = 0; i < C; ++i) {  // one frame step of every stream, nothing decided on the host
            SN_TRY(obm_frame_solve(o, fr, i, C));
            SN_TRY(obm_post(o, fr, i));
            if (o->n_cls) SN_TRY(obm_class_spectra(o, fr, i, C));
            SN_TRY(obm_adapt(o, fr, i));
        }
    }
    // the synthesis of one signal: k_obtail (0: the streams' tails into the buffer's head), k_obistft behind each stream's
    // kept frames, k_obola to the output hops, k_obtail (1: the tails back out)
    const int64_t syn_stride = (int64_t)(C + nov - 1) * sz;
    const size_t lds_fft = obm_lds_fft(o);
    OIstftArgsT<T> ia{};
    ia.ph = o->Yph; ia.ld = F; ia.n_frames = C; ia.sz = sz; ia.dcb = p.dcbin_back; ia.powv = (T)p.pow;
    ia.scale = (T)(p.overlapscale / (double)o->N); ia.preemph = (T)p.preemph; ia.win = o->win_i; ia.tw = o->tw; ia.syn = o->syn;
    auto move_tail = [&](T* tail, int store) -> int {
        if (nov > 1) hipLaunchKernelGGL(k_obtail<T>, dim3(S), dim3(256), 0, st, o->syn, tail, fr.nfr, syn_stride, nov, sz, store);
        HIP_TRY(hipGetLastError());
        return SNMF_OK;
    };
    auto synth = [&](const T* mag, T* tail, T* of, int16_t* o16) -> int {
        SN_TRY(move_tail(tail, 0));
        ia.mag = mag;
        int rc = SNMF_OK;
        by_logn([&](auto L) {
            constexpr int LOGN = decltype(L)::value;
            if (lds_fft) rc = ensure_dyn_lds(o->ctx->device, (const void*)k_obistft<LOGN, T>, lds_fft);
            if (rc == SNMF_OK) hipLaunchKernelGGL((k_obistft<LOGN, T>), dim3(C, S), dim3(256), lds_fft, st, ia, fr.nfr, S, syn_stride, nov);
        }, o->N);
        SN_TRY(rc);
        HIP_TRY(hipGetLastError());
        if (n_out > 0) {
            const int gx = std::max(1, std::min(64, (int)((size_t)C * hop / 256 + 1)));
            hipLaunchKernelGGL(k_obola<T>, dim3(gx, S), dim3(256), 0, st, (const T*)o->syn, syn_stride, fr, d_if, d_no, d_oo, p.delay, sz, hop,
                               nov, of, o16);
            HIP_TRY(hipGetLastError());
        }
        return move_tail(tail, 1);
    };
    // the three signals go to the thirds of outf: x_tilde, x_hat, d_hat
    std::vector<T> hf, hx, hd;
    std::vector<int16_t> h16;
    auto fetch = [&](std::vector<T>& v, const T* src) -> int {
        v.resize(n_out);
        if (n_out) HIP_TRY(hipMemcpyAsync(v.data(), src, n_out * sizeof(T), hipMemcpyDeviceToHost, st));
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
    std::vector<std::vector<T>> hc(want_ci ? o->n_cls : 0);
    for (int c = 0; c < o->n_cls; ++c) {
        T* oc = o->out_c + (size_t)c * std::max<size_t>(o->cap_out, 1);
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
            snmf_online_frame tr = online_frame_record(q);
            if (obatch_adapts(o, s) && q.do_solve && q.n_up > 0) {
                tr.solved = 1;
                tr.adapt_iters = hit[(size_t)i * S + s];
            }
            o->trace[s].push_back(tr);
            if (o->trace[s].size() > kBTraceCap) o->trace[s].pop_front();
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
            const T* end = sig.data() + h_off[s] + (sz - hop) + (size_t)nreal[s] * hop;
            o->hist[s].assign(end - (sz - hop), end);
        }
        o->l[s] += nfr[s];
    }
    return SNMF_OK;
}

// snmf_online_batch_process_* / _process_classes_* behind the handle checks (xhi / dhi: the class signals, class-major at cap[s])
template <class H, typename T = typename H::elem>
int obatch_process(H* o, const T* const* pcm, const int64_t* n, const int32_t* flush, T* const* xt, int16_t* const* xt_i16, T* const* xh,
                   T* const* dh, T* const* xhi, T* const* dhi, const int64_t* cap, int64_t* n_out) {
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
    const int C = obm_chunk_frames(o);
    std::vector<int64_t> done(S, 0);
    std::vector<OBatchSink<T>> sink(S);
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
        if (int rc = obatch_run_chunk(o, nfr, nreal, done, wf, wi, wc, wci, sink)) {
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
        const OBatchSink<T>& k = sink[s];
        if (wf && xt[s]) std::memcpy(xt[s], k.f.data(), k.f.size() * sizeof(T));
        if (wi && xt_i16[s]) std::memcpy(xt_i16[s], k.i16.data(), k.i16.size() * 2);
        if (xh && xh[s]) std::memcpy(xh[s], k.x.data(), k.x.size() * sizeof(T));
        if (dh && dh[s]) std::memcpy(dh[s], k.d.data(), k.d.size() * sizeof(T));
        size_t nc_out = 0;
        if (cls_set) {
            for (int c = 0; c < (int)k.c.size(); ++c) {
                T* dst = c < o->n_ev ? ((xhi && xhi[s]) ? xhi[s] + (size_t)c * cap[s] : nullptr)
                                     : ((dhi && dhi[s]) ? dhi[s] + (size_t)(c - o->n_ev) * cap[s] : nullptr);
                if (dst) std::memcpy(dst, k.c[c].data(), k.c[c].size() * sizeof(T));
                nc_out = std::max(nc_out, k.c[c].size());
            }
        } else {
            if (xhi && xhi[s]) std::memcpy(xhi[s], k.x.data(), k.x.size() * sizeof(T));
            if (dhi && dhi[s]) std::memcpy(dhi[s], k.d.data(), k.d.size() * sizeof(T));
        }
        if (n_out) n_out[s] = (int64_t)std::max(std::max(std::max(k.f.size(), k.i16.size()), std::max(k.x.size(), k.d.size())), nc_out);
    }
    return SNMF_OK;
}

// ---------------------------------------------------------------------------------------------
// Get-state / set-state (snmf_online_batch_state_info / _get_state / _set_state; include/snmf.h).  A stream's state g is
// one record: [magic, version, snmf_online_state_info | the fields of snmf_online_state_field].  The device arrays cross
// through one staging slab of records and one kernel (k_obstate_get / _put); the host state (pending, hist, l) is written
// into / read from the same records here.  The record's layout, header checks and host fields are snmf_online_host.h's,
// shared with the single-stream separator.
// ---------------------------------------------------------------------------------------------
template <class H>
void obatch_state_info(const H* o, snmf_online_state_info* q) {
    int mel = 0, mel_conv = 0, n1 = 0;
    obm_state_mode(o, &mel, &mel_conv, &n1);
    ostate_info_of(o, mel, mel_conv, n1, o->ntail, q);
}

// the listed slots are valid and distinct, and the batch is usable
template <class H>
int obatch_state_slots(const H* o, int32_t n, const int32_t* slots, const char* what) {
    if (n < 0 || n > o->S) return fail(SNMF_ERR_INVALID, "%s of %d streams in a batch of %d", what, n, o->S);
    if (n > 0 && !slots) return fail(SNMF_ERR_INVALID, "slots is NULL");
    std::vector<uint8_t> seen(o->S, 0);
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (s < 0 || s >= o->S) return fail(SNMF_ERR_INVALID, "stream %d out of range [0, %d)", s, o->S);
        if (seen[s]) return fail(SNMF_ERR_INVALID, "stream %d listed twice", s);
        seen[s] = 1;
    }
    if (o->failed) return fail(SNMF_ERR_STATE, "an earlier call failed midway through a chunk; the batch state is not reusable, create a new one");
    return SNMF_OK;
}

// the kernel's view of the batch and of a record under `q`
template <class H, typename T = typename H::elem>
OStateArgs<T> obatch_state_args(H* o, const snmf_online_state_info& q) {
    OStateArgs<T> a{};
    ostate_arg_offsets(q, &a);
    a.slots = o->rs_slots; a.slab = o->st_slab;
    a.Xm_tilde = o->Xm_tilde; a.lambda_dav = o->lambda_dav; a.r_blk = o->r_blk; a.ldblk = o->ldblk; a.adblk = o->adblk; a.H0 = o->H0;
    a.Ad0 = o->Ad0; a.tail = o->tail; a.tail_x = o->tail_x; a.tail_d = o->tail_d; a.tail_c = o->n_cls ? o->tail_c : nullptr;
    a.B = o->B; a.Bfix = o->Bfix; a.dev = o->dev;
    a.S = o->S; a.F = o->F; a.r = o->r; a.Rx = o->p.R_x; a.Rd = o->p.R_d; a.Ra = o->Ra; a.ma = o->ma; a.Pl = o->Pl; a.n_cls = o->n_cls;
    a.ntail = (int64_t)o->ntail;
    return a;  // Bm, Bdf and n1 stay NULL / 0 here: DFT mode.  The fp32 unit's obm_state_launch sets them in Mel mode.
}

template <class H>
int obatch_state_slab(H* o, size_t bytes) {
    if (bytes <= o->st_cap) return SNMF_OK;
    HIP_TRY(hipStreamSynchronize(o->ctx->stream));
    if (o->st_slab) HIP_TRY(hipFree(o->st_slab));
    o->st_slab = nullptr;
    o->st_cap = 0;
    SN_TRY(dalloc(&o->st_slab, bytes));
    o->st_cap = bytes;
    return SNMF_OK;
}

template <class H, typename T = typename H::elem>
int obatch_get_state(H* o, int32_t n, const int32_t* slots, void* records, int64_t cap) {
    SN_TRY(obatch_state_slots(o, n, slots, "get_state"));
    if (n == 0) return SNMF_OK;
    if (!records) return fail(SNMF_ERR_INVALID, "records is NULL");
    for (int i = 0; i < n; ++i)
        if (o->finished[slots[i]])
            return fail(SNMF_ERR_STATE, "stream %d was flushed: what survives it is its dictionary (snmf_online_batch_get_basis_f64)", slots[i]);
    snmf_online_state_info q;
    obatch_state_info(o, &q);
    const size_t rb = (size_t)q.bytes, total = rb * (size_t)n;
    if (cap < 0 || (uint64_t)cap < total)
        return fail(SNMF_ERR_INVALID, "records holds %lld bytes, %d records need %zu", (long long)cap, n, total);
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    SN_TRY(obatch_state_slab(o, total));
    std::vector<int64_t> hl((size_t)n);
    for (int i = 0; i < n; ++i) hl[i] = o->l[slots[i]] + 1;
    HIP_TRY(hipMemcpyAsync(o->rs_slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->meta_l, hl.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));  // (a chunk uploads meta_l anew)
    OStateArgs<T> a = obatch_state_args(o, q);
    a.l = o->meta_l;
    SN_TRY(obm_state_launch(o, a, n, false));
    HIP_TRY(hipMemcpyAsync(records, o->st_slab, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the header, the host state, and zeros wherever the device wrote nothing (two gets of one state are the same bytes)
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        ostate_write_host<T>((unsigned char*)records + (size_t)i * rb, q, o->l[s], o->pending[s], o->hist[s]);
    }
    return SNMF_OK;
}

template <class H, typename T = typename H::elem>
int obatch_set_state(H* o, int32_t n, const int32_t* slots, const void* records, int64_t bytes) {
    SN_TRY(obatch_state_slots(o, n, slots, "set_state"));
    if (n == 0) return SNMF_OK;
    if (!records) return fail(SNMF_ERR_INVALID, "records is NULL");
    snmf_online_state_info q;
    obatch_state_info(o, &q);
    const size_t rb = (size_t)q.bytes, total = rb * (size_t)n;
    int64_t off[SNMF_STATE_FIELD_COUNT], cnt[SNMF_STATE_FIELD_COUNT];
    int32_t typ[SNMF_STATE_FIELD_COUNT];
    ostate_layout(q, off, cnt, typ);
    // every header against the handle, before the device is touched
    for (int i = 0; i < n; ++i) SN_TRY(ostate_check_record(records, bytes, i, n, q, off, "batch"));
    (void)hipGetLastError();  // clean sticky error state, see PLAN_CHECK
    HIP_TRY(hipSetDevice(o->ctx->device));
    hipStream_t st = o->ctx->stream;
    SN_TRY(obatch_state_slab(o, total));
    auto device = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(o->rs_slots, slots, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o->st_slab, records, total, hipMemcpyHostToDevice, st));
        OStateArgs<T> a = obatch_state_args(o, q);
        a.l = nullptr;  // the records hold it
        SN_TRY(obm_state_launch(o, a, n, true));
        SN_TRY(obm_state_refresh(o, n));  // the solve's images from the masters, by the kernel that follows an adaptation
        HIP_TRY(hipStreamSynchronize(st));  // the caller's buffer is free, and a fault is this call's
        return SNMF_OK;
    };
    if (int rc = device()) {
        o->failed = true;  // some of the listed streams may be half written
        return rc;
    }
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        ostate_read_host<T>((const unsigned char*)records + (size_t)i * rb, q, &o->l[s], &o->pending[s], &o->hist[s]);
        o->finished[s] = 0;
        o->trace[s].clear();  // the trace goes on from frame l
    }
    obm_state_installed(o, n, slots);
    o->started = true;  // running streams: set_mel / set_classes are behind us
    return SNMF_OK;
}
