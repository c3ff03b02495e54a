// snmf_tu_frontend_batch.hip -- the front-end grouped over the signals of a batch (the kernels of snmf_frontend_batch.h) and the
// three callers that need it:
//
//   snmf_stft_features_batch_f32 / _fp64             TF_mag (or TF_Mel) of n signals, tight host arrays in and out
//   snmf_run_basis_dnmf_audio_batch_f64 / _fp64      run_basis_DNMF.m:1-55 (and its Mel twin) for n pairs of WAVEFORMS
//   snmf_run_basis_dnmf_audio_batch_ranks_fp64       the fp64 entry with a rank pair and settings per problem
//   snmf_run_basis_train_audio_batch_f64 / _fp64     run_basis_train.m:58-91 for the training signals of n classes
//   snmf_run_basis_train_signals_batch_f64 / _fp64   the same on the signals a snmf_train_signals handle holds in HBM
//   snmf_run_basis_train_audio_batch_ranks_fp64, snmf_run_basis_train_signals_batch_ranks_fp64
//                                                    the two fp64 training entries with a dictionary size per problem
//
// The DNMF entries are dnmf_batch_run of snmf_batch_host.h -- the three resident batches of snmf_run_basis_dnmf_batch_* -- with V
// formed on the device: the truncated waveforms of every problem go up as ONE slab through the context's transfer pipeline
// (x_0 .. x_{n-1}, d_0 .. d_{n-1}), one launch forms y = x + d behind them, and for each of the three phases the features of all
// n signals are written by two to three launches straight into the blocks the phase's engine hands out.  A call launches the
// front-end 1 + 3 * (1 + [Splice > 0] + [mel]) times, whatever n.  Only the samples, B and a given H0 cross to the device.
// A translation unit of its own: nothing of the single front-ends or of the engines is touched.
#include "snmf_internal.h"
#include "snmf_frontend_batch.h"
#include "snmf_batch_host.h"
#include "snmf_assemble.h"

namespace {

constexpr int kMaxSignals = 65535;        // a launch grid's second dimension: the element-wise passes put the signal there
constexpr long long kMaxFrames = 0x7fffffffLL;  // a launch grid's first dimension: k_stft*_grp has a workgroup per frame
constexpr int kElemGrid = 1024;           // workgroups per signal of an element-wise pass (grid-stride beyond)
constexpr int kTabs = 4;                  // FeSig tables of a run: STFT, splice, Mel, TF_DD

template <typename S>
struct Types;
template <>
struct Types<float> {
    using C2 = float2;
    using Args = StftGrpArgs;
    static C2 make(double re, double im) { return make_float2((float)re, (float)im); }
};
template <>
struct Types<double> {
    using C2 = double2;
    using Args = Stft64GrpArgs;
    static C2 make(double re, double im) { return make_double2(re, im); }
};

template <int LOGN>
int launch_stft(snmf_ctx* ctx, unsigned frames, const StftGrpArgs& a) {
    hipLaunchKernelGGL(k_stft_grp<LOGN>, dim3(frames), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}
template <int LOGN>
int launch_stft(snmf_ctx* ctx, unsigned frames, const Stft64GrpArgs& a) {
    const size_t lds = (size_t)2 * (1 << LOGN) * sizeof(double2);
    SN_TRY(ensure_dyn_lds(ctx->device, (const void*)k_stft64_grp<LOGN>, lds));
    hipLaunchKernelGGL(k_stft64_grp<LOGN>, dim3(frames), dim3(256), lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// The grouped front-end of one call in the sample type S: the sample slab, the window, twiddles and Mel table (as the single
// front-end of that type makes them), the scratch of one run and the tables of every run.
template <typename S>
struct FeBatch {
    using C2 = typename Types<S>::C2;
    snmf_ctx* ctx = nullptr;
    snmf_stft_params sp{};
    int N = 0, nb = 0, Ks = 1, M = 0;  // FFT length, bins, spliced blocks, Mel channels (0: none)
    int64_t cap_frames = 0;
    int cap_sig = 0, cap_runs = 0, runs = 0;
    DevMem mem;
    S *slab = nullptr, *win = nullptr, *mel = nullptr, *tmp = nullptr, *scr = nullptr;
    double* carry = nullptr;  // TF_DD: [chunks of a run][DFT rows]
    C2* tw = nullptr;
    FeSig* tab = nullptr;
    std::vector<S> h_win, h_mel;  // (sources of asynchronous copies: they live as long as the device blocks)
    std::vector<C2> h_tw;
    std::vector<FeSig> h_tab;
    bool opened = false;

    int rows_dft() const { return Ks * nb; }

    // slab_elems samples; every run forms at most max_frames frames of at most max_sig signals.  With a Mel table the DFT-row
    // scratch is one run's: the runs of a call use it in turn; a caller whose runs all keep the DFT rows (run with dst_mel) asks
    // for none.  tfdd: the runs may apply TF_DD.
    int open(snmf_ctx* c, const snmf_stft_params* sp_in, const S* mel_host, int mel_M, int64_t slab_elems, int64_t max_frames, int max_sig,
             int n_runs, bool dft_scratch = true, bool tfdd = false) {
        ctx = c;
        sp = *sp_in;
        N = sp.fftlength, nb = N / 2 + 1, Ks = 2 * sp.splice + 1, M = mel_host ? mel_M : 0;
        cap_frames = max_frames, cap_sig = max_sig, cap_runs = n_runs;
        mem.st = ctx->stream;
        hipStream_t st = ctx->stream;
        h_win.resize(sp.framelength);
        for (int i = 0; i < sp.framelength; ++i) h_win[i] = (S)sp.window[i];
        h_tw.resize(N / 2);
        for (int q = 0; q < N / 2; ++q) {
            const double ang = -2.0 * M_PI * (double)q / (double)N;
            h_tw[q] = Types<S>::make(cos(ang), sin(ang));
        }
        SN_TRY(mem.get(&slab, (size_t)slab_elems));
        SN_TRY(mem.get(&win, h_win.size()));
        SN_TRY(mem.get(&tw, h_tw.size()));
        if (sp.splice > 0) SN_TRY(mem.get(&tmp, (size_t)nb * (size_t)max_frames));
        if (tfdd) SN_TRY(mem.get(&carry, (size_t)rows_dft() * (size_t)(max_frames / kDdGrpChunk + max_sig)));
        if (M) {
            if (dft_scratch) SN_TRY(mem.get(&scr, (size_t)rows_dft() * (size_t)max_frames));
            h_mel.resize((size_t)M * nb);
            if (sizeof(S) == 4) std::copy(mel_host, mel_host + h_mel.size(), h_mel.begin());  // k_mel reads the ABI's row-major M x n
            else                                                                                 // k_mel64 reads it transposed
                for (int m = 0; m < M; ++m)
                    for (int f = 0; f < nb; ++f) h_mel[(size_t)f * M + m] = mel_host[(size_t)m * nb + f];
            SN_TRY(mem.get(&mel, h_mel.size()));
            HIP_TRY(hipMemcpyAsync(mel, h_mel.data(), h_mel.size() * sizeof(S), hipMemcpyHostToDevice, st));
        }
        SN_TRY(mem.get(&tab, (size_t)kTabs * max_sig * n_runs));
        h_tab.resize((size_t)kTabs * max_sig * n_runs);
        HIP_TRY(hipMemcpyAsync(win, h_win.data(), h_win.size() * sizeof(S), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(tw, h_tw.data(), h_tw.size() * sizeof(C2), hipMemcpyHostToDevice, st));
        opened = true;
        return SNMF_OK;
    }

    // features of n signals: signal k starts at sample s0[k] of the slab, has T[k] >= 1 frames and goes to dst[k].
    // dst_mel == nullptr: dst receives the Mel rows when there is a Mel table (the DFT rows pass through the scratch), else the
    // DFT rows.  dst_mel != nullptr (needs the table): BOTH feature sets stay -- the DFT rows are formed in dst, the Mel rows are
    // projected from there into dst_mel, and no scratch is used.  alpha_dd >= 0: TF_DD runs in place on the DFT rows, wherever
    // they are, before the Mel pass reads them (run_basis_train.m:64-78).
    int run(int n, const int64_t* s0, const int32_t* T, const snmf_batch::VBlock* dst, const snmf_batch::VBlock* dst_mel = nullptr,
            double alpha_dd = -1.0) {
        const bool dd = alpha_dd >= 0.0;
        if (runs >= cap_runs || n > cap_sig || n < 1) return fail(SNMF_ERR_INTERNAL, "grouped front-end: run %d of %d with %d signals", runs, cap_runs, n);
        if ((dst_mel && !M) || (M && !dst_mel && !scr) || (dd && !carry)) return fail(SNMF_ERR_INTERNAL, "grouped front-end: a run it was not opened for");
        hipStream_t st = ctx->stream;
        const int S_ = sp.splice;
        FeSig* h = h_tab.data() + (size_t)kTabs * cap_sig * runs;
        FeSig* d = tab + (size_t)kTabs * cap_sig * runs;
        FeSig *h_st = h, *h_sp = h + cap_sig, *h_ml = h + 2 * (size_t)cap_sig, *h_dd = h + 3 * (size_t)cap_sig;
        int64_t f0 = 0, c0 = 0;  // frames, TF_DD chunks of the signals before k
        int maxT = 1;
        for (int k = 0; k < n; ++k) {
            const int64_t Tk = T[k];
            maxT = std::max(maxT, T[k]);
            S* t_k = tmp ? tmp + (size_t)nb * f0 : nullptr;
            // where the DFT rows of the signal are formed, and where its result goes
            const bool via_scr = M && !dst_mel;
            S* dft = via_scr ? scr + (size_t)rows_dft() * f0 : (S*)dst[k].V;
            const int64_t ld_dft = via_scr ? (int64_t)rows_dft() : dst[k].ld;
            const snmf_batch::VBlock& mo = dst_mel ? dst_mel[k] : dst[k];
            // the STFT writes the unspliced magnitudes (a splicing pass follows) or the DFT rows
            FeSig a{};
            a.s0 = s0[k], a.f0 = f0, a.T = T[k];
            if (S_ > 0) a.dst = t_k, a.ld_dst = nb;
            else a.dst = dft, a.ld_dst = ld_dft;
            h_st[k] = a;
            FeSig b{};
            b.T = T[k], b.src = t_k, b.ld_src = nb, b.dst = dft, b.ld_dst = ld_dft;
            h_sp[k] = b;
            FeSig m{};
            m.T = T[k], m.src = dft, m.ld_src = ld_dft, m.dst = mo.V, m.ld_dst = mo.ld;
            h_ml[k] = m;
            FeSig e{};
            e.T = T[k], e.f0 = c0, e.dst = dft, e.ld_dst = ld_dft;
            h_dd[k] = e;
            f0 += Tk;
            c0 += (Tk + kDdGrpChunk - 1) / kDdGrpChunk;
        }
        if (f0 > cap_frames || f0 > kMaxFrames) return fail(SNMF_ERR_INTERNAL, "grouped front-end: %lld frames in a run sized for %lld", (long long)f0, (long long)cap_frames);
        if (dd && c0 > cap_frames / kDdGrpChunk + cap_sig) return fail(SNMF_ERR_INTERNAL, "grouped front-end: %lld TF_DD chunks", (long long)c0);
        HIP_TRY(hipMemcpyAsync(d, h, sizeof(FeSig) * (size_t)kTabs * cap_sig, hipMemcpyHostToDevice, st));
        ++runs;
        typename Types<S>::Args a{};
        a.slab = slab, a.sig = d, a.n_sig = n;
        a.sz = sp.framelength, a.shift = sp.frameshift, a.dcbin = sp.dcbin;
        a.preemph = (S)sp.preemph;
        a.win = win, a.tw = tw;
        a.powv = (S)sp.pow;
        a.floorv = S_ == 0 ? (S)sp.nonzerofloor : (S)0;
        const unsigned frames = (unsigned)f0;
        switch (N) {
            case 64: SN_TRY(launch_stft<6>(ctx, frames, a)); break;
            case 128: SN_TRY(launch_stft<7>(ctx, frames, a)); break;
            case 256: SN_TRY(launch_stft<8>(ctx, frames, a)); break;
            case 512: SN_TRY(launch_stft<9>(ctx, frames, a)); break;
            case 1024: SN_TRY(launch_stft<10>(ctx, frames, a)); break;
            case 2048: SN_TRY(launch_stft<11>(ctx, frames, a)); break;
            default: SN_TRY(launch_stft<12>(ctx, frames, a)); break;
        }
        auto grid = [&](int rows) { return dim3((unsigned)std::max<long long>(1, std::min<long long>(((long long)rows * maxT + 255) / 256, kElemGrid)), (unsigned)n); };
        if (S_ > 0) {
            hipLaunchKernelGGL(k_splice_grp<S>, grid(rows_dft()), dim3(256), 0, st, (const FeSig*)(d + cap_sig), nb, S_, (S)sp.nonzerofloor);
            HIP_TRY(hipGetLastError());
        }
        if (dd) {  // the three passes of snmf_tf_dd_*, each one launch over every signal
            const FeSig* dt = d + 3 * (size_t)cap_sig;
            const int F = rows_dft();
            const dim3 g((unsigned)c0, (unsigned)((F + 255) / 256));
            hipLaunchKernelGGL(k_tfdd_carry_grp<S>, g, dim3(256), 0, st, dt, n, F, alpha_dd, carry);
            hipLaunchKernelGGL(k_tfdd_state_grp<S>, dim3((unsigned)((F + 255) / 256), (unsigned)n), dim3(256), 0, st, dt, F, alpha_dd, carry);
            hipLaunchKernelGGL(k_tfdd_apply_grp<S>, g, dim3(256), 0, st, dt, n, F, alpha_dd, (const double*)carry);
            HIP_TRY(hipGetLastError());
        }
        if (M) {
            hipLaunchKernelGGL(k_mel_grp<S>, grid(Ks * M), dim3(256), 0, st, (const FeSig*)(d + 2 * (size_t)cap_sig), (const S*)mel, M, nb, Ks);
            HIP_TRY(hipGetLastError());
        }
        return SNMF_OK;
    }
};

int check_batch_size(const char* entry, int32_t n, const char* what) {
    if (n < 1) return fail(SNMF_ERR_INVALID, "%s: %s must be at least 1 (got %d)", entry, what, n);
    if (n > kMaxSignals) return fail(SNMF_ERR_UNSUPPORTED, "%s: %d is above the limit of %d (a launch grid's second dimension)", entry, n, kMaxSignals);
    return SNMF_OK;
}

// ---- TF_mag / TF_Mel of n signals ----------------------------------------------------------------------------------------------
template <typename S>
int features_batch(const char* entry, snmf_ctx* ctx, const snmf_stft_params* sp, int32_t n, const S* const* samples, const int64_t* n_samples,
                   const S* mel, int32_t mel_M, S* const* V_out, int32_t* n_frames_out) {
    if (!ctx || !samples || !n_samples || !V_out) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    SN_TRY(check_batch_size(entry, n, "n_signals"));
    SN_TRY(validate_stft(sp));
    if (mel && mel_M < 1) return fail(SNMF_ERR_INVALID, "%s: mel_M must be positive", entry);
    const int nb = sp->fftlength / 2 + 1, Ks = 2 * sp->splice + 1;
    const int64_t rows = mel ? (int64_t)Ks * mel_M : (int64_t)Ks * nb;
    // the signals that have a frame: the others report 0 frames and nothing of theirs is read or written
    std::vector<int> who;
    std::vector<int32_t> T;
    std::vector<int64_t> len(n, 0), s0;
    int64_t sumT = 0, sumL = 0;
    for (int k = 0; k < n; ++k) {
        if (n_samples[k] < 0) return fail(SNMF_ERR_INVALID, "%s: signal %d has a negative length", entry, k);
        const int64_t Tk = snmf_stft_num_frames(sp, n_samples[k]);
        if (Tk > kMaxFrames) return fail(SNMF_ERR_UNSUPPORTED, "%s: signal %d has %lld frames", entry, k, (long long)Tk);
        if (Tk <= 0) continue;
        if (!samples[k] || !V_out[k]) return fail(SNMF_ERR_INVALID, "%s: an array of signal %d is NULL", entry, k);
        who.push_back(k);
        T.push_back((int32_t)Tk);
        s0.push_back(sumL);
        len[k] = n_samples[k];
        sumT += Tk;
        sumL += n_samples[k];
    }
    if (sumT > kMaxFrames) return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld frames are above the launch grid's limit", entry, (long long)sumT);
    if (rows > 0x7fffffffLL) return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld feature rows", entry, (long long)rows);
    if (n_frames_out) {
        for (int k = 0; k < n; ++k) n_frames_out[k] = 0;
        for (size_t j = 0; j < who.size(); ++j) n_frames_out[who[j]] = T[j];
    }
    if (who.empty()) return SNMF_OK;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    FeBatch<S> fe;
    SN_TRY(fe.open(ctx, sp, mel, mel_M, sumL, sumT, (int)who.size(), 1));
    SN_TRY(xfer_gather_in<S>(ctx, n, samples, len.data(), fe.slab));
    S* out = nullptr;
    SN_TRY(fe.mem.get(&out, (size_t)rows * (size_t)sumT));
    std::vector<snmf_batch::VBlock> dst(who.size());
    {
        int64_t c0 = 0;
        for (size_t j = 0; j < who.size(); ++j) {
            dst[j] = snmf_batch::VBlock{out + (size_t)rows * c0, rows};
            c0 += T[j];
        }
    }
    SN_TRY(fe.run((int)who.size(), s0.data(), T.data(), dst.data()));
    for (size_t j = 0; j < who.size(); ++j) {
        const int k = who[j];
        SN_TRY((xfer_unpack_out<S, S>(ctx, (const S*)dst[j].V, (int)rows, (int)rows, T[j], V_out[k], rows)));
    }
    return SNMF_OK;
}

// ---- run_basis_DNMF from the waveforms of n problems ------------------------------------------------------------------------------
// per_problem (snmf_run_basis_dnmf_audio_batch_ranks_fp64): problem k has the rank pair (R_xs[k], R_ds[k]) and, with st, the settings
// st[k]; R_x and R_d are not looked at.  The front-end does not know the ranks: the same slab and the same launches.
template <typename S>
int dnmf_audio_batch(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x,
                     int32_t R_d, int32_t n, const S* const* x, const int64_t* n_x, const S* const* d, const int64_t* n_d, const S* mel,
                     int32_t mel_M, const double* const* B, const double* const* H0, const uint64_t* seed, double* const* B_hat,
                     double* const* A_hat, int32_t* n_iter, bool per_problem = false, const int32_t* R_xs = nullptr,
                     const int32_t* R_ds = nullptr, const snmf_problem_settings* st = nullptr) {
    if (!ctx || !p || !x || !n_x || !d || !n_d || !B || !B_hat) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    SN_TRY(check_batch_size(entry, n, "n_problems"));
    SN_TRY(validate_stft(sp));
    if (mel && mel_M < 1) return fail(SNMF_ERR_INVALID, "%s: mel_M must be positive", entry);
    const int nb = sp->fftlength / 2 + 1, Ks = 2 * sp->splice + 1;
    const int64_t F = mel ? (int64_t)Ks * mel_M : (int64_t)Ks * nb;
    std::vector<int32_t> T(n);
    std::vector<int64_t> len(2 * (size_t)n), off(n);
    std::vector<const S*> src(2 * (size_t)n);
    int64_t sumL = 0, sumT = 0;
    for (int k = 0; k < n; ++k) {
        if (!x[k] || !d[k] || !B[k] || !B_hat[k]) return fail(SNMF_ERR_INVALID, "%s: an array of problem %d is NULL", entry, k);
        if ((!H0 || !H0[k]) && !seed) return fail(SNMF_ERR_INVALID, "%s: problem %d has no H0 and there are no seeds", entry, k);
        const int64_t L = std::min(n_x[k], n_d[k]);  // run_basis_DNMF.m:5-9
        const int64_t Tk = snmf_stft_num_frames(sp, L);
        if (Tk < 1) return fail(SNMF_ERR_INVALID, "%s: the signals of problem %d are shorter than one analysis frame", entry, k);
        if (Tk > kMaxFrames) return fail(SNMF_ERR_UNSUPPORTED, "%s: problem %d has %lld frames", entry, k, (long long)Tk);
        T[k] = (int32_t)Tk;
        off[k] = sumL;
        src[k] = x[k], src[(size_t)n + k] = d[k];
        len[k] = len[(size_t)n + k] = L;
        sumL += L;
        sumT += Tk;
    }
    if (sumT > kMaxFrames) return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld frames are above the launch grid's limit", entry, (long long)sumT);
    if (F != p->F) return fail(SNMF_ERR_DIM, "%s: the signals give %lld feature rows, params say %d", entry, (long long)F, p->F);
    (void)hipGetLastError();

    FeBatch<S> fe;  // (declared before the engines of dnmf_batch_run: it outlives them)
    DnmfInputs<double> in;
    in.H0 = H0;
    in.seed = seed;
    in.device_v = [&](int kind, const std::vector<snmf_batch::VBlock>& blocks, size_t elem) -> int {
        if (elem != sizeof(S) || (int)blocks.size() != n) return fail(SNMF_ERR_INTERNAL, "%s: the engine's V is not of the sample type", entry);
        hipStream_t st = ctx->stream;
        if (!fe.opened) {  // the slab [x | d | y], once: the engines exist, every refusal has been made
            SN_TRY(fe.open(ctx, sp, mel, mel_M, 3 * sumL, sumT, n, 3));
            SN_TRY(xfer_gather_in<S>(ctx, 2 * n, src.data(), len.data(), fe.slab));
            const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((sumL + 255) / 256, 8192));
            hipLaunchKernelGGL(k_add_grp<S>, dim3(g), dim3(256), 0, st, (const S*)fe.slab, (const S*)(fe.slab + sumL), fe.slab + 2 * sumL, sumL);  // :10
            HIP_TRY(hipGetLastError());
        }
        const int64_t base = kind == 0 ? 2 * sumL : (kind == 1 ? 0 : sumL);  // y, x, d
        std::vector<int64_t> s0(n);
        for (int k = 0; k < n; ++k) s0[k] = base + off[k];
        return fe.run(n, s0.data(), T.data(), blocks.data());
    };
    if (per_problem) return dnmf_batch_run_ranks<double>(entry, make, ctx, p, R_xs, R_ds, st, n, T.data(), in, B, B_hat, A_hat, n_iter);
    return dnmf_batch_run<double>(entry, make, ctx, p, R_x, R_d, n, T.data(), in, B, B_hat, A_hat, n_iter);
}

// ---- run_basis_train for the training signals of n classes -----------------------------------------------------------------------
// train_batch_run of snmf_batch_host.h with the features formed by ONE run of the grouped front-end: STFT (+ splice) into the DFT
// engine's blocks, TF_DD in place there, the Mel projection from those blocks into the Mel engine's.  The front-end launches
// 1 + [Splice > 0] + 3 [TF_DD] + [mel] times and each engine gathers its exemplars in one launch, whatever n.
// ts != nullptr (snmf_run_basis_train_signals_batch_*): the signals are the handle's, resident in HBM as doubles; samples and
// n_samples are not looked at, the lengths are the handle's and the sample slab is filled by one launch of k_sig_fill (a copy
// for double, round to nearest for float) instead of the transfer.  Everything else is the same code.
// n_atoms != nullptr (the _ranks_fp64 entries): problem k trains n_atoms[k] atoms -- sample_idx[k] holds that many indices, its
// outputs have that many columns / rows -- and p->r is the largest; nullptr: p->r for every problem.
// st != nullptr (the _settings_fp64 entries): problem k is solved with the settings st[k] in both engines.
template <typename S>
int train_audio_batch(const char* entry, snmf_batch* (*make)(), snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                      const S* mel, int32_t mel_M, int32_t n, const S* const* samples, const int64_t* n_samples,
                      const int64_t* const* sample_idx, int32_t train_exemplar, const double* const* H0, const uint64_t* seed,
                      double* const* B_DFT, double* const* A_DFT, double* const* B_Mel, double* const* A_Mel, int32_t* n_iter,
                      const snmf_train_signals* ts = nullptr, const int32_t* n_atoms = nullptr, const snmf_problem_settings* st = nullptr) {
    if (!ctx || !p || (!ts && (!samples || !n_samples)) || !sample_idx || !B_DFT) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    if (ts) {
        if (ts->ctx != ctx) return fail(SNMF_ERR_INVALID, "%s: the signals were assembled on another context", entry);
        n = (int32_t)ts->len.size();
        n_samples = ts->len.data();
    }
    SN_TRY(check_batch_size(entry, n, "n_problems"));
    SN_TRY(validate_stft(sp));
    if (n_atoms) {
        int r_max = 0;
        for (int k = 0; k < n; ++k) {
            if (n_atoms[k] < 1) return fail(SNMF_ERR_INVALID, "%s: problem %d has n_atoms = %d (at least 1)", entry, k, n_atoms[k]);
            r_max = std::max(r_max, (int)n_atoms[k]);
        }
        if (p->r != r_max) return fail(SNMF_ERR_DIM, "%s: params->r = %d must be the largest n_atoms, %d", entry, p->r, r_max);
    }
    if (st) {  // (the four fields of p are ignored: every s[k] is checked in their place)
        SN_TRY(batch_check_settings(entry, p, n, st, nullptr));
    } else {
        snmf_params q = *p;
        q.T = 1;  // (ignored: every problem brings its own)
        SN_TRY(validate_params(&q));
    }
    if ((mel != nullptr) != (B_Mel != nullptr)) return fail(SNMF_ERR_INVALID, "%s: mel and B_Mel must be given together", entry);
    if (mel && mel_M < 1) return fail(SNMF_ERR_INVALID, "%s: mel_M must be positive", entry);
    if (p->sparsity_kind != SNMF_SPARSITY_SCALAR)
        return fail(SNMF_ERR_UNSUPPORTED, "%s: a sparsity vector or matrix is not supported by the training entry (it takes the scalar of p)", entry);
    const int nb = sp->fftlength / 2 + 1, Ks = 2 * sp->splice + 1;
    const int64_t F = (int64_t)Ks * nb, Fm = mel ? (int64_t)Ks * mel_M : 0;
    std::vector<int32_t> T(n);
    std::vector<int64_t> len(n), s0(n), idx;
    int64_t sumL = 0, sumT = 0;
    for (int k = 0; k < n; ++k) {
        if ((!ts && !samples[k]) || !sample_idx[k] || !B_DFT[k] || (mel && !B_Mel[k])) return fail(SNMF_ERR_INVALID, "%s: an array of problem %d is NULL", entry, k);
        if (!train_exemplar && (!H0 || !H0[k]) && !seed) return fail(SNMF_ERR_INVALID, "%s: problem %d has no H0 and there are no seeds", entry, k);
        const int64_t Tk = snmf_stft_num_frames(sp, n_samples[k]);
        if (Tk < 1) return fail(SNMF_ERR_INVALID, "%s: the signal of problem %d is shorter than one analysis frame", entry, k);
        if (Tk > kMaxFrames) return fail(SNMF_ERR_UNSUPPORTED, "%s: problem %d has %lld frames", entry, k, (long long)Tk);
        T[k] = (int32_t)Tk;
        len[k] = n_samples[k];
        s0[k] = sumL;
        sumL += n_samples[k];
        sumT += Tk;
    }
    if (sumT > kMaxFrames) return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld frames are above the launch grid's limit", entry, (long long)sumT);
    if (F != p->F) return fail(SNMF_ERR_DIM, "%s: the signals give %lld feature rows, params say %d", entry, (long long)F, p->F);
    if (Fm > 0x7fffffffLL) return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld Mel feature rows", entry, (long long)Fm);
    for (int k = 0; k < n; ++k) {  // (packed: problem k's entries behind those of the problems before it)
        const int r = n_atoms ? n_atoms[k] : p->r;
        for (int j = 0; j < r; ++j) {
            const int64_t t = sample_idx[k][j];
            if (t < 0 || t >= T[k])
                return fail(SNMF_ERR_DIM, "%s: sample_idx[%d][%d] = %lld outside [0, %d)", entry, k, j, (long long)t, T[k]);
            idx.push_back(t);
        }
    }
    (void)hipGetLastError();

    std::vector<SigCopy> h_cp;  // (the source of an asynchronous copy: it lives as long as the front-end)
    FeBatch<S> fe;  // (declared before the engines of train_batch_run: it outlives them)
    TrainInputs<double> in;
    in.idx = idx.data();
    in.exemplar = train_exemplar != 0;
    in.H0 = H0;
    in.seed = seed;
    in.device_v = [&](const std::vector<snmf_batch::VBlock>& dft, const std::vector<snmf_batch::VBlock>& melb, size_t elem) -> int {
        if (elem != sizeof(S) || (int)dft.size() != n || (mel && (int)melb.size() != n))
            return fail(SNMF_ERR_INTERNAL, "%s: the engine's V is not of the sample type", entry);
        SN_TRY(fe.open(ctx, sp, mel, mel_M, sumL, sumT, n, 1, false, alpha_eta_dd >= 0.0));  // the engines exist, every refusal has been made
        if (ts) {
            h_cp.resize(n);
            int64_t maxL = 1;
            for (int k = 0; k < n; ++k) h_cp[k] = SigCopy{ts->out0[k], s0[k], len[k]}, maxL = std::max(maxL, len[k]);
            SigCopy* d_cp = nullptr;
            SN_TRY(fe.mem.get(&d_cp, (size_t)n));
            HIP_TRY(hipMemcpyAsync(d_cp, h_cp.data(), sizeof(SigCopy) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            const dim3 g((unsigned)std::min<int64_t>((maxL + 255) / 256, 8192), (unsigned)n);
            hipLaunchKernelGGL(k_sig_fill<S>, g, dim3(256), 0, ctx->stream, (const double*)ts->slab, (const SigCopy*)d_cp, fe.slab);
            HIP_TRY(hipGetLastError());
        } else {
            SN_TRY(xfer_gather_in<S>(ctx, n, samples, len.data(), fe.slab));
        }
        return fe.run(n, s0.data(), T.data(), dft.data(), mel ? melb.data() : nullptr, alpha_eta_dd);
    };
    return train_batch_run<double>(entry, make, ctx, p, (int32_t)Fm, n, T.data(), in, B_DFT, A_DFT, B_Mel, A_Mel, n_iter, n_atoms, st);
}

snmf_batch* make32() { return batch32_new(); }
snmf_batch* make64() { return batch64_new(); }

}  // namespace

extern "C" int snmf_run_basis_train_audio_batch_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                    const float* mel, int32_t mel_M, int32_t n_problems, const float* const* samples,
                                                    const int64_t* n_samples, const int64_t* const* sample_idx, int32_t train_exemplar,
                                                    const double* const* H0, const uint64_t* seed, double* const* B_DFT,
                                                    double* const* A_DFT, double* const* B_Mel, double* const* A_Mel, int32_t* n_iter) {
    return train_audio_batch<float>("snmf_run_basis_train_audio_batch_f64", make32, ctx, p, sp, alpha_eta_dd, mel, mel_M, n_problems, samples,
                                    n_samples, sample_idx, train_exemplar, H0, seed, B_DFT, A_DFT, B_Mel, A_Mel, n_iter);
}
extern "C" int snmf_run_basis_train_audio_batch_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                     const double* mel, int32_t mel_M, int32_t n_problems, const double* const* samples,
                                                     const int64_t* n_samples, const int64_t* const* sample_idx, int32_t train_exemplar,
                                                     const double* const* H0, const uint64_t* seed, double* const* B_DFT,
                                                     double* const* A_DFT, double* const* B_Mel, double* const* A_Mel, int32_t* n_iter) {
    return train_audio_batch<double>("snmf_run_basis_train_audio_batch_fp64", make64, ctx, p, sp, alpha_eta_dd, mel, mel_M, n_problems, samples,
                                     n_samples, sample_idx, train_exemplar, H0, seed, B_DFT, A_DFT, B_Mel, A_Mel, n_iter);
}

extern "C" int snmf_run_basis_train_signals_batch_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                      const float* mel, int32_t mel_M, const snmf_train_signals* signals,
                                                      const int64_t* const* sample_idx, int32_t train_exemplar, const double* const* H0,
                                                      const uint64_t* seed, double* const* B_DFT, double* const* A_DFT,
                                                      double* const* B_Mel, double* const* A_Mel, int32_t* n_iter) {
    const char* entry = "snmf_run_basis_train_signals_batch_f64";
    if (!signals) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return train_audio_batch<float>(entry, make32, ctx, p, sp, alpha_eta_dd, mel, mel_M, 0, nullptr, nullptr, sample_idx, train_exemplar, H0, seed,
                                    B_DFT, A_DFT, B_Mel, A_Mel, n_iter, signals);
}
extern "C" int snmf_run_basis_train_signals_batch_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                       const double* mel, int32_t mel_M, const snmf_train_signals* signals,
                                                       const int64_t* const* sample_idx, int32_t train_exemplar, const double* const* H0,
                                                       const uint64_t* seed, double* const* B_DFT, double* const* A_DFT,
                                                       double* const* B_Mel, double* const* A_Mel, int32_t* n_iter) {
    const char* entry = "snmf_run_basis_train_signals_batch_fp64";
    if (!signals) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return train_audio_batch<double>(entry, make64, ctx, p, sp, alpha_eta_dd, mel, mel_M, 0, nullptr, nullptr, sample_idx, train_exemplar, H0, seed,
                                     B_DFT, A_DFT, B_Mel, A_Mel, n_iter, signals);
}

extern "C" int snmf_run_basis_train_audio_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                           const double* mel, int32_t mel_M, int32_t n_problems, const double* const* samples,
                                                           const int64_t* n_samples, const int32_t* n_atoms, const int64_t* const* sample_idx,
                                                           int32_t train_exemplar, const double* const* H0, const uint64_t* seed,
                                                           double* const* B_DFT, double* const* A_DFT, double* const* B_Mel,
                                                           double* const* A_Mel, int32_t* n_iter) {
    const char* entry = "snmf_run_basis_train_audio_batch_ranks_fp64";
    if (!n_atoms) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return train_audio_batch<double>(entry, make64, ctx, p, sp, alpha_eta_dd, mel, mel_M, n_problems, samples, n_samples, sample_idx,
                                     train_exemplar, H0, seed, B_DFT, A_DFT, B_Mel, A_Mel, n_iter, nullptr, n_atoms);
}
extern "C" int snmf_run_basis_train_signals_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                             const double* mel, int32_t mel_M, const snmf_train_signals* signals,
                                                             const int32_t* n_atoms, const int64_t* const* sample_idx, int32_t train_exemplar,
                                                             const double* const* H0, const uint64_t* seed, double* const* B_DFT,
                                                             double* const* A_DFT, double* const* B_Mel, double* const* A_Mel,
                                                             int32_t* n_iter) {
    const char* entry = "snmf_run_basis_train_signals_batch_ranks_fp64";
    if (!signals || !n_atoms) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return train_audio_batch<double>(entry, make64, ctx, p, sp, alpha_eta_dd, mel, mel_M, 0, nullptr, nullptr, sample_idx, train_exemplar, H0, seed,
                                     B_DFT, A_DFT, B_Mel, A_Mel, n_iter, signals, n_atoms);
}

extern "C" int snmf_run_basis_train_audio_batch_settings_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                                              const double* mel, int32_t mel_M, int32_t n_problems, const double* const* samples,
                                                              const int64_t* n_samples, const int32_t* n_atoms, const int64_t* const* sample_idx,
                                                              int32_t train_exemplar, const double* const* H0, const uint64_t* seed,
                                                              double* const* B_DFT, double* const* A_DFT, double* const* B_Mel,
                                                              double* const* A_Mel, int32_t* n_iter, const snmf_problem_settings* s) {
    const char* entry = "snmf_run_basis_train_audio_batch_settings_fp64";
    if (!s) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return train_audio_batch<double>(entry, make64, ctx, p, sp, alpha_eta_dd, mel, mel_M, n_problems, samples, n_samples, sample_idx,
                                     train_exemplar, H0, seed, B_DFT, A_DFT, B_Mel, A_Mel, n_iter, nullptr, n_atoms, s);
}
extern "C" int snmf_run_basis_train_signals_batch_settings_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp,
                                                                double alpha_eta_dd, const double* mel, int32_t mel_M,
                                                                const snmf_train_signals* signals, const int32_t* n_atoms,
                                                                const int64_t* const* sample_idx, int32_t train_exemplar,
                                                                const double* const* H0, const uint64_t* seed, double* const* B_DFT,
                                                                double* const* A_DFT, double* const* B_Mel, double* const* A_Mel,
                                                                int32_t* n_iter, const snmf_problem_settings* s) {
    const char* entry = "snmf_run_basis_train_signals_batch_settings_fp64";
    if (!signals || !s) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    return train_audio_batch<double>(entry, make64, ctx, p, sp, alpha_eta_dd, mel, mel_M, 0, nullptr, nullptr, sample_idx, train_exemplar, H0, seed,
                                     B_DFT, A_DFT, B_Mel, A_Mel, n_iter, signals, n_atoms, s);
}

extern "C" int snmf_stft_features_batch_f32(snmf_ctx* ctx, const snmf_stft_params* sp, int32_t n_signals, const float* const* samples,
                                            const int64_t* n_samples, const float* mel, int32_t mel_M, float* const* V_out,
                                            int32_t* n_frames_out) {
    return features_batch<float>("snmf_stft_features_batch_f32", ctx, sp, n_signals, samples, n_samples, mel, mel_M, V_out, n_frames_out);
}
extern "C" int snmf_stft_features_batch_fp64(snmf_ctx* ctx, const snmf_stft_params* sp, int32_t n_signals, const double* const* samples,
                                             const int64_t* n_samples, const double* mel, int32_t mel_M, double* const* V_out,
                                             int32_t* n_frames_out) {
    return features_batch<double>("snmf_stft_features_batch_fp64", ctx, sp, n_signals, samples, n_samples, mel, mel_M, V_out, n_frames_out);
}

extern "C" int snmf_run_basis_dnmf_audio_batch_f64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                                   int32_t n_problems, const float* const* x, const int64_t* n_x, const float* const* d,
                                                   const int64_t* n_d, const float* mel, int32_t mel_M, const double* const* B,
                                                   const double* const* H0, const uint64_t* seed, double* const* B_hat,
                                                   double* const* A_hat, int32_t* n_iter) {
    return dnmf_audio_batch<float>("snmf_run_basis_dnmf_audio_batch_f64", make32, ctx, p, sp, R_x, R_d, n_problems, x, n_x, d, n_d, mel, mel_M, B,
                                   H0, seed, B_hat, A_hat, n_iter);
}
extern "C" int snmf_run_basis_dnmf_audio_batch_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                                    int32_t n_problems, const double* const* x, const int64_t* n_x, const double* const* d,
                                                    const int64_t* n_d, const double* mel, int32_t mel_M, const double* const* B,
                                                    const double* const* H0, const uint64_t* seed, double* const* B_hat,
                                                    double* const* A_hat, int32_t* n_iter) {
    return dnmf_audio_batch<double>("snmf_run_basis_dnmf_audio_batch_fp64", make64, ctx, p, sp, R_x, R_d, n_problems, x, n_x, d, n_d, mel, mel_M, B,
                                    H0, seed, B_hat, A_hat, n_iter);
}

extern "C" int snmf_run_basis_dnmf_audio_batch_ranks_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, const int32_t* R_x,
                                                          const int32_t* R_d, const snmf_problem_settings* s, int32_t n_problems,
                                                          const double* const* x, const int64_t* n_x, const double* const* d,
                                                          const int64_t* n_d, const double* mel, int32_t mel_M, const double* const* B,
                                                          const double* const* H0, const uint64_t* seed, double* const* B_hat,
                                                          double* const* A_hat, int32_t* n_iter) {
    return dnmf_audio_batch<double>("snmf_run_basis_dnmf_audio_batch_ranks_fp64", make64, ctx, p, sp, 0, 0, n_problems, x, n_x, d, n_d, mel, mel_M,
                                    B, H0, seed, B_hat, A_hat, n_iter, true, R_x, R_d, s);
}
