// snmf_online_batch_mex.cpp -- MATLAB MEX shim over the batched online separator of libsnmf_hip.so
// (include/snmf.h: snmf_online_batch_*), written like snmf_online_mex.cpp.
//
// The binding a maintainer of lordet01/SE_SNMF_NAT adds so that the per-target loop of
// Do_MultiBatch_IS16_20160324.m:183-205 -- chains of directories enhanced file after file by run_ntf_sep_RT.m, B_D_u.mat
// carried from file to file and deleted between chains -- runs as ONE call on S streams of an MI355X
// (integration/batch/run_ntf_sep_RT_chains.m is the MATLAB side).  Written against the documented MEX C API.  MATLAB is
// not available where this project is built and tested: __graft_entry__.build() syntax-checks this file against
// integration/mex_stub/mex.h, and the tests execute it under the test host (tests/test_online_chains_native_api.py: every
// argument check without a device; tests/test_gpu_online_chains_native.py: bit for bit against se_snmf_nat_amd/online.py,
// which makes the same C calls).
//
// Build:  mex -R2018a -I<repo>/include integration/snmf_online_batch_mex.cpp -L<repo>/se_snmf_nat_amd -lsnmf_hip
//
// Ragged data cross as one concatenated column plus a column of counts (no cell arrays).  Calls:
//   h = snmf_online_batch_mex('create', B_DFT_x, B_DFT_d, H0, Ad_blk0, p, S)
//         B_DFT_d F x R_d (shared) or F x (R_d*S); H0 r x 1 or r x S (r = R_x + R_d: its rows give R_d); Ad_blk0 R_a x m_a or
//         R_a x (m_a*S), read only with p.adapt_train_N
//   snmf_online_batch_mex('set_mel', h, melmat, B_Mel_x, B_Mel_d, MelConv)      B_Mel_d F_order x R_d or F_order x (R_d*S)
//   [x, n_out, xf] = snmf_online_batch_mex('process', h, pcm, n, flush)
//         pcm: the streams' samples, concatenated; n, flush: S x 1; x: the int16 outputs, concatenated; n_out: S x 1;
//         xf (optional): the float signal as double
//   snmf_online_batch_mex('restart', h, slots, B_DFT_d, H0, Ad_blk0[, B_Mel_d])
//         slots 1-based, distinct; each array [] (carry / keep) or one entry per listed slot, side by side; the seventh
//         argument on a Mel batch only
//   B = snmf_online_batch_mex('basis', h, k)         stream k's fp64 master of B_DFT_d (k 1-based)
//   B = snmf_online_batch_mex('mel_basis', h, k)     stream k's fp64 master of B_Mel_d
//   [x, n_out, B_out, xf] = snmf_online_batch_mex('chains', h, pcm, n_samples, n_files, B_DFT_d, H0, Ad_blk0, chunk_hops[, B_Mel_d])
//         snmf_online_batch_run_chains_*: n_files per chain, n_samples per file in chain order, pcm all files concatenated;
//         B_DFT_d F x (R_d*chains), H0 r x chains, Ad_blk0 R_a x (m_a*chains) ([] without adaptation), chunk_hops 0 = the
//         default; B_out F x (R_d*files): the dictionary after every file (Mel batch: B_Mel_d, F_order rows, and the tenth
//         argument is every chain's start B_Mel_d).  On an fp32 batch the start dictionaries are rounded to fp32, as 'create'
//         rounds them, so that a chain's bits do not depend on whether its slot was created or restarted with them.
//   snmf_online_batch_mex('destroy', h)
// Every array must be real double and is checked against the length the C ABI reads or writes -- a mismatch is snmf:dim, a
// wrong class snmf:type, a missing field of p snmf:field -- before the device is touched: counts that do not add up are
// refused before the handle is even looked at.  p.precision = 'fp64' selects the fp64 entries (DFT mode).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mex.h"
#include "snmf.h"

static snmf_ctx* g_ctx = nullptr;
struct batch_handle {
    snmf_online_batch* o;
    bool f64, adapt;
    size_t S, F, R_x, R_d, R_a, m_a, n1;  // n1: F_order once 'set_mel' was called, 0 before
};
static std::vector<batch_handle> g_handles;

static void at_exit() {
    for (batch_handle& h : g_handles)
        if (h.o) snmf_online_batch_destroy(h.o);
    g_handles.clear();
    if (g_ctx) {
        snmf_ctx_destroy(g_ctx);
        g_ctx = nullptr;
    }
}

static double fld(const mxArray* p, const char* name, double dflt, bool required = false) {
    const mxArray* f = mxGetField(p, 0, name);
    if (!f || mxIsEmpty(f)) {
        if (required) mexErrMsgIdAndTxt("snmf:field", "Reference to non-existent field '%s'.", name);
        return dflt;
    }
    return mxGetScalar(f);
}

static void need_double(const mxArray* a, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
}

static std::vector<float> to_f32(const double* d, size_t n) {
    std::vector<float> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = (float)d[i];
    return out;
}

static double scalar_arg(const mxArray* a, const char* what) {
    if (mxIsStruct(a) || mxGetNumberOfElements(a) != 1) mexErrMsgIdAndTxt("snmf:dim", "%s must be a scalar", what);
    need_double(a, what);
    return mxGetScalar(a);
}

static void need_size(const mxArray* a, size_t m, size_t n, const char* what) {
    need_double(a, what);
    if (mxGetNumberOfDimensions(a) != 2 || mxGetM(a) != m || mxGetN(a) != n)
        mexErrMsgIdAndTxt("snmf:dim", "%s must be %d x %d (got %d x %d)", what, (int)m, (int)n, (int)mxGetM(a), (int)mxGetN(a));
}

// m x n (one for all) or m x (n * S) (one per stream, side by side) -> the S entries, consecutive
static std::vector<double> per_stream(const mxArray* a, size_t m, size_t n, size_t S, const char* what) {
    need_double(a, what);
    const bool shared = mxGetNumberOfDimensions(a) == 2 && mxGetM(a) == m && mxGetN(a) == n;
    const bool each = mxGetNumberOfDimensions(a) == 2 && mxGetM(a) == m && mxGetN(a) == n * S;
    if (!shared && !each)
        mexErrMsgIdAndTxt("snmf:dim", "%s must be %d x %d or %d x %d (got %d x %d)", what, (int)m, (int)n, (int)m, (int)(n * S), (int)mxGetM(a),
                          (int)mxGetN(a));
    const double* d = mxGetDoubles(a);
    std::vector<double> out(m * n * S);
    for (size_t k = 0; k < S; ++k) std::memcpy(out.data() + k * m * n, d + (each ? k * m * n : 0), m * n * sizeof(double));
    return out;
}

// [] -> false; else m x (n * cnt), checked
static bool optional_size(const mxArray* a, size_t m, size_t n, size_t cnt, const char* what) {
    need_double(a, what);
    if (mxIsEmpty(a)) return false;
    need_size(a, m, n * cnt, what);
    return true;
}

// a vector of `what` holding non-negative whole numbers (counts) -> int64; `total`: their sum
static std::vector<int64_t> counts(const mxArray* a, const char* what, int64_t* total) {
    need_double(a, what);
    if (mxGetNumberOfDimensions(a) != 2 || (mxGetM(a) > 1 && mxGetN(a) > 1)) mexErrMsgIdAndTxt("snmf:dim", "%s must be a vector", what);
    const size_t n = mxGetNumberOfElements(a);
    const double* d = mxGetDoubles(a);
    std::vector<int64_t> out(n);
    int64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!(d[i] >= 0.0 && d[i] <= 2147483647.0) || d[i] != std::floor(d[i]))
            mexErrMsgIdAndTxt("snmf:dim", "%s(%d) = %g is not a count", what, (int)i + 1, d[i]);
        out[i] = (int64_t)d[i];
        sum += out[i];
    }
    *total = sum;
    return out;
}

static const double* vector_arg(const mxArray* a, const char* what, int64_t* n) {
    need_double(a, what);
    if (mxGetNumberOfDimensions(a) != 2 || (mxGetM(a) > 1 && mxGetN(a) > 1)) mexErrMsgIdAndTxt("snmf:dim", "%s must be a vector", what);
    *n = (int64_t)mxGetNumberOfElements(a);
    return mxGetDoubles(a);
}

// 1-based handle -> index into g_handles; a handle that was never made, or was destroyed, is snmf:handle
static size_t handle_index(const mxArray* a) {
    const double v = (mxIsStruct(a) || mxGetNumberOfElements(a) != 1) ? 0.0 : mxGetScalar(a);
    if (!(v >= 1.0 && v <= (double)g_handles.size()) || v != (double)(size_t)v || !g_handles[(size_t)v - 1].o)
        mexErrMsgIdAndTxt("snmf:handle", "invalid batch handle");
    return (size_t)v - 1;
}

// 1-based stream index of the handle
static int32_t stream_arg(const mxArray* a, const batch_handle& h) {
    const double v = scalar_arg(a, "k");
    if (!(v >= 1.0 && v <= (double)h.S) || v != std::floor(v)) mexErrMsgIdAndTxt("snmf:dim", "stream %g outside 1..%d", v, (int)h.S);
    return (int32_t)v - 1;
}

// the int16 and float signals of several streams / files as concatenated columns
template <typename T>
static void signals_out(int nlhs, mxArray* plhs[], int xf_at, const std::vector<std::vector<int16_t>>& x16, const std::vector<std::vector<T>>& xf,
                        const std::vector<int64_t>& n_out) {
    size_t total = 0;
    for (int64_t m : n_out) total += (size_t)m;
    plhs[0] = mxCreateNumericMatrix((mwSize)total, 1, mxINT16_CLASS, mxREAL);
    mxInt16* d16 = mxGetInt16s(plhs[0]);
    size_t at = 0;
    for (size_t i = 0; i < n_out.size(); ++i) {
        if (n_out[i]) std::memcpy(d16 + at, x16[i].data(), (size_t)n_out[i] * 2);
        at += (size_t)n_out[i];
    }
    if (nlhs > 1) {
        plhs[1] = mxCreateDoubleMatrix((mwSize)n_out.size(), 1, mxREAL);
        double* d = mxGetDoubles(plhs[1]);
        for (size_t i = 0; i < n_out.size(); ++i) d[i] = (double)n_out[i];
    }
    if (nlhs > xf_at) {
        plhs[xf_at] = mxCreateDoubleMatrix((mwSize)total, 1, mxREAL);
        double* d = mxGetDoubles(plhs[xf_at]);
        at = 0;
        for (size_t i = 0; i < n_out.size(); ++i)
            for (int64_t j = 0; j < n_out[i]; ++j) d[at++] = (double)xf[i][(size_t)j];
    }
}

template <typename T>
static std::vector<T> as_elem(const double* d, size_t n) {
    std::vector<T> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = (T)d[i];
    return out;
}

// 'process' behind its checks, in the handle's element type
template <typename T>
static void do_process(const batch_handle& h, int nlhs, mxArray* plhs[], const double* pcm, const std::vector<int64_t>& n, const double* fl) {
    const size_t S = h.S;
    std::vector<std::vector<T>> in(S), xf(S);
    std::vector<std::vector<int16_t>> x16(S);
    std::vector<const T*> pin(S);
    std::vector<T*> pf(S);
    std::vector<int16_t*> p16(S);
    std::vector<int64_t> cap(S), n_out(S, 0);
    std::vector<int32_t> flush(S);
    size_t at = 0;
    for (size_t k = 0; k < S; ++k) {
        in[k] = as_elem<T>(pcm + at, (size_t)n[k]);
        at += (size_t)n[k];
        cap[k] = snmf_online_batch_out_capacity(h.o, n[k]);
        xf[k].resize((size_t)cap[k]);
        x16[k].resize((size_t)cap[k]);
        pin[k] = n[k] ? in[k].data() : nullptr;
        pf[k] = xf[k].data();
        p16[k] = x16[k].data();
        flush[k] = fl[k] != 0;
    }
    int rc;
    if constexpr (sizeof(T) == 8)
        rc = snmf_online_batch_process_f64(h.o, pin.data(), n.data(), flush.data(), pf.data(), p16.data(), nullptr, nullptr, cap.data(), n_out.data());
    else
        rc = snmf_online_batch_process_f32(h.o, pin.data(), n.data(), flush.data(), pf.data(), p16.data(), nullptr, nullptr, cap.data(), n_out.data());
    if (rc != SNMF_OK) mexErrMsgIdAndTxt("snmf:process", "%s", snmf_last_error());
    signals_out(nlhs, plhs, 2, x16, xf, n_out);
}

// 'chains' behind its checks, in the handle's element type; Bd / Bmd are the start dictionaries as the library takes them
template <typename T>
static void do_chains(const batch_handle& h, int nlhs, mxArray* plhs[], const double* pcm, const std::vector<int64_t>& n_samples,
                      const std::vector<int64_t>& n_files, const double* Bd, const double* Bmd, const double* H0, const double* Ad,
                      int32_t chunk_hops) {
    const size_t nf = n_samples.size(), nc = n_files.size(), r = h.R_x + h.R_d;
    std::vector<std::vector<T>> in(nf), xf(nf);
    std::vector<std::vector<int16_t>> x16(nf);
    std::vector<const T*> pin(nf);
    std::vector<T*> pf(nf);
    std::vector<int16_t*> p16(nf);
    std::vector<double*> pB(nf);
    std::vector<int64_t> cap(nf), n_out(nf, 0);
    std::vector<int32_t> files(nc);
    for (size_t c = 0; c < nc; ++c) files[c] = (int32_t)n_files[c];
    const size_t rows = h.n1 ? h.n1 : h.F;
    mxArray* Bo = mxCreateDoubleMatrix((mwSize)rows, (mwSize)(h.R_d * nf), mxREAL);
    size_t at = 0;
    for (size_t i = 0; i < nf; ++i) {
        in[i] = as_elem<T>(pcm + at, (size_t)n_samples[i]);
        at += (size_t)n_samples[i];
        cap[i] = snmf_online_batch_out_capacity(h.o, n_samples[i]);
        xf[i].resize((size_t)cap[i]);
        x16[i].resize((size_t)cap[i]);
        pin[i] = n_samples[i] ? in[i].data() : nullptr;
        pf[i] = xf[i].data();
        p16[i] = x16[i].data();
        pB[i] = mxGetDoubles(Bo) + i * rows * h.R_d;
    }
    const std::vector<T> h0 = as_elem<T>(H0, r * nc), ad = Ad ? as_elem<T>(Ad, h.R_a * h.m_a * nc) : std::vector<T>();
    int rc;
    if constexpr (sizeof(T) == 8)
        rc = snmf_online_batch_run_chains_f64(h.o, (int32_t)nc, files.data(), pin.data(), n_samples.data(), Bd, Bmd, h0.data(),
                                              Ad ? ad.data() : nullptr, chunk_hops, p16.data(), pf.data(), cap.data(), n_out.data(), pB.data());
    else
        rc = snmf_online_batch_run_chains_f32(h.o, (int32_t)nc, files.data(), pin.data(), n_samples.data(), Bd, Bmd, h0.data(),
                                              Ad ? ad.data() : nullptr, chunk_hops, p16.data(), pf.data(), cap.data(), n_out.data(), pB.data());
    if (rc != SNMF_OK) {
        mxDestroyArray(Bo);
        mexErrMsgIdAndTxt("snmf:chains", "%s", snmf_last_error());
    }
    signals_out(nlhs, plhs, 3, x16, xf, n_out);
    if (nlhs > 2) plhs[2] = Bo;
    else mxDestroyArray(Bo);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (snmf_abi_version() != SNMF_ABI_VERSION)  // a stale libsnmf_hip.so must not be driven through newer prototypes
        mexErrMsgIdAndTxt("snmf:abi", "libsnmf_hip.so has ABI version %d, this MEX file was built against %d", snmf_abi_version(), SNMF_ABI_VERSION);
    if (nrhs < 1 || !mxIsChar(prhs[0]))
        mexErrMsgIdAndTxt("snmf:usage", "first argument: 'create' | 'set_mel' | 'process' | 'restart' | 'basis' | 'mel_basis' | 'chains' | 'destroy'");
    char cmd[16];
    mxGetString(prhs[0], cmd, sizeof cmd);
    const int max_out = !strcmp(cmd, "process") ? 3 : !strcmp(cmd, "chains") ? 4 : 1;
    if (nlhs > max_out) mexErrMsgIdAndTxt("snmf:nargout", "'%s' has at most %d outputs", cmd, max_out);
    if (!strcmp(cmd, "create")) {
        if (nrhs != 7) mexErrMsgIdAndTxt("snmf:usage", "create: B_DFT_x, B_DFT_d, H0, Ad_blk0, p, S");
        const mxArray* p = prhs[5];
        if (!mxIsStruct(p)) mexErrMsgIdAndTxt("snmf:type", "p must be a struct");
        char mode[8] = "DFT", meth[8] = "MMSE", cf[8] = "kl", prec[8] = "fp32";
        if (const mxArray* f = mxGetField(p, 0, "precision"))
            if (!mxIsEmpty(f) && mxGetString(f, prec, sizeof prec) != 0) prec[0] = 0;  // not a string, or too long to be one of the two
        if (strcmp(prec, "fp32") && strcmp(prec, "fp64")) mexErrMsgIdAndTxt("snmf:precision", "p.precision must be 'fp32' or 'fp64'");
        const bool f64 = !strcmp(prec, "fp64");
        if (const mxArray* f = mxGetField(p, 0, "B_sep_mode")) mxGetString(f, mode, sizeof mode);
        if (const mxArray* f = mxGetField(p, 0, "ENHANCE_METHOD")) mxGetString(f, meth, sizeof meth);
        if (const mxArray* f = mxGetField(p, 0, "cf")) mxGetString(f, cf, sizeof cf);
        if ((strcmp(mode, "DFT") && strcmp(mode, "Mel")) || fld(p, "Splice", 0) != 0 || fld(p, "blk_len_sep", 1) != 1)
            mexErrMsgIdAndTxt("snmf:unsupported", "only Splice=0, blk_len_sep=1, B_sep_mode 'DFT' or 'Mel' (then call 'set_mel')");
        const double Sv = scalar_arg(prhs[6], "S");
        if (!(Sv >= 1.0 && Sv <= 65536.0) || Sv != std::floor(Sv)) mexErrMsgIdAndTxt("snmf:dim", "S = %g is not a number of streams", Sv);
        const size_t S = (size_t)Sv;
        snmf_online_params q;
        std::memset(&q, 0, sizeof q);
        q.fftlength = (int32_t)fld(p, "fftlength", 0, true);
        q.framelength = (int32_t)fld(p, "framelength", 0, true);
        q.frameshift = (int32_t)fld(p, "frameshift", 0, true);
        q.dcbin = (int32_t)fld(p, "DCbin", 0, true);
        q.dcbin_back = (int32_t)fld(p, "DCbin_back", q.dcbin);
        q.delay = (int32_t)fld(p, "delay", 0, true);
        q.preemph = fld(p, "preemph", 0.0);
        q.pow = fld(p, "pow", 2.0);
        q.nonzerofloor = fld(p, "nonzerofloor", 1e-9);
        q.overlapscale = fld(p, "overlapscale", 0, true);
        need_double(prhs[1], "B_DFT_x");
        need_double(prhs[3], "H0");
        q.R_x = (int32_t)mxGetN(prhs[1]);
        q.R_d = (int32_t)mxGetM(prhs[3]) - q.R_x;  // H0 is r x 1 or r x S: its rows give the rank
        q.beta_div = !strcmp(cf, "is") ? 0.0 : !strcmp(cf, "kl") ? 1.0 : !strcmp(cf, "ed") ? 2.0 : fld(p, "beta_div", 1.0);
        q.sparsity = fld(p, "sparsity", 0.0);
        q.max_iter = (int32_t)fld(p, "max_iter", 100);
        q.cost_check = fld(p, "cost_check", 0, true) != 0;  // src/sparse_nmf.m:260
        q.conv_eps = fld(p, "conv_eps", 0.0);
        q.enhance_method = !strcmp(meth, "Wiener") ? 0 : 1;
        q.init_N_len = (int32_t)fld(p, "init_N_len", 0);
        q.alpha_eta = fld(p, "alpha_eta", 0.4);
        q.alpha_d = fld(p, "alpha_d", 0.6);
        q.beta = fld(p, "beta", 1.0);
        q.beta_max = fld(p, "beta_max", 1000.0);
        q.blk_sparse = fld(p, "blk_sparse", 0) != 0;
        q.P_len_k = (int32_t)fld(p, "P_len_k", 60);
        q.P_len_l = (int32_t)fld(p, "P_len_l", 20);
        q.blk_gap = (int32_t)fld(p, "blk_gap", 3);
        q.alpha_p = fld(p, "alpha_p", 0.4);
        q.adapt_train_N = fld(p, "adapt_train_N", 0) != 0;
        q.R_a = (int32_t)fld(p, "R_a", 1);
        q.m_a = (int32_t)fld(p, "m_a", 1);
        q.overlap_m_a = fld(p, "overlap_m_a", 0.01);
        q.Ar_up = fld(p, "Ar_up", 1.0);
        q.class_outputs = 0;
        q.basis_update_N = fld(p, "basis_update_N", 0) != 0;
        q.basis_update_E = fld(p, "basis_update_E", 0) != 0;
        const mxArray *ws = mxGetField(p, 0, "win_STFT"), *wi = mxGetField(p, 0, "win_ISTFT");
        if (!ws || !wi) mexErrMsgIdAndTxt("snmf:field", "p.win_STFT / p.win_ISTFT missing");
        // what the library reads from each array: F x R_x, F x R_d x S, r x S, R_a x m_a x S (only with adapt_train_N), framelength
        if (q.fftlength < 2 || q.framelength < 1 || q.frameshift < 1 || q.R_a < 1 || q.m_a < 1)
            mexErrMsgIdAndTxt("snmf:dim", "p.fftlength, p.framelength, p.frameshift, p.R_a and p.m_a must be positive");
        const size_t F = (size_t)q.fftlength / 2 + 1;
        if (q.R_x < 1 || q.R_d < 1) mexErrMsgIdAndTxt("snmf:dim", "B_DFT_x must not be empty and H0 must have R_x + R_d rows, R_d >= 1");
        need_size(prhs[1], F, (size_t)q.R_x, "B_DFT_x (fftlength/2+1 rows)");
        const std::vector<double> Bd = per_stream(prhs[2], F, (size_t)q.R_d, S, "B_DFT_d (fftlength/2+1 rows, R_d = rows of H0 - R_x columns)");
        const std::vector<double> H0 = per_stream(prhs[3], (size_t)q.R_x + (size_t)q.R_d, 1, S, "H0 (R_x + R_d rows)");
        const bool adapt = q.adapt_train_N != 0;  // without it the library never reads Ad_blk0: it gets NULL, [] is fine
        std::vector<double> Ad;
        if (adapt) Ad = per_stream(prhs[4], (size_t)q.R_a, (size_t)q.m_a, S, "Ad_blk0 (p.R_a x p.m_a)");
        else if (!mxIsEmpty(prhs[4])) need_double(prhs[4], "Ad_blk0");
        need_double(ws, "p.win_STFT");
        need_double(wi, "p.win_ISTFT");
        if (mxGetNumberOfElements(ws) != (size_t)q.framelength || mxGetNumberOfElements(wi) != (size_t)q.framelength)
            mexErrMsgIdAndTxt("snmf:dim", "p.win_STFT and p.win_ISTFT must have framelength = %d entries", q.framelength);
        if (!g_ctx) {
            if (snmf_ctx_create(&g_ctx, 0) != SNMF_OK) mexErrMsgIdAndTxt("snmf:device", "%s", snmf_last_error());
            mexAtExit(at_exit);
            mexLock();
        }
        snmf_online_batch* o = nullptr;
        if (f64) {
            // MATLAB already holds doubles: nothing is rounded on the way in
            if (snmf_online_batch_create_f64(g_ctx, &q, (int32_t)S, mxGetDoubles(prhs[1]), Bd.data(), H0.data(), adapt ? Ad.data() : nullptr,
                                             mxGetDoubles(ws), mxGetDoubles(wi), &o) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:create", "%s", snmf_last_error());
        } else {
            const std::vector<float> bx = to_f32(mxGetDoubles(prhs[1]), F * q.R_x), bd = to_f32(Bd.data(), Bd.size()), h0 = to_f32(H0.data(), H0.size());
            const std::vector<float> ad = to_f32(Ad.data(), Ad.size());
            const std::vector<float> w1 = to_f32(mxGetDoubles(ws), (size_t)q.framelength), w2 = to_f32(mxGetDoubles(wi), (size_t)q.framelength);
            if (snmf_online_batch_create(g_ctx, &q, (int32_t)S, bx.data(), bd.data(), h0.data(), adapt ? ad.data() : nullptr, w1.data(), w2.data(),
                                         &o) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:create", "%s", snmf_last_error());
        }
        g_handles.push_back(batch_handle{o, f64, adapt, S, F, (size_t)q.R_x, (size_t)q.R_d, (size_t)q.R_a, (size_t)q.m_a, 0});
        plhs[0] = mxCreateDoubleScalar((double)g_handles.size());
    } else if (!strcmp(cmd, "set_mel")) {
        // ('set_mel', h, melmat, B_Mel_x, B_Mel_d, MelConv): melmat = g.melmat (F_order x F), init_buff.m:46
        if (nrhs != 6) mexErrMsgIdAndTxt("snmf:usage", "set_mel: handle, melmat, B_Mel_x, B_Mel_d, MelConv");
        need_double(prhs[2], "melmat");
        need_double(prhs[3], "B_Mel_x");
        need_double(prhs[4], "B_Mel_d");
        const bool mel_conv = scalar_arg(prhs[5], "MelConv") != 0;
        const size_t hi = handle_index(prhs[1]);
        batch_handle& h = g_handles[hi];
        const size_t n1 = mxGetM(prhs[2]), F = mxGetN(prhs[2]);
        // the library reads F_order x F, F_order x R_x and F_order x R_d x S values, F, R_x, R_d and S being the handle's
        if (n1 < 1 || F != h.F) mexErrMsgIdAndTxt("snmf:dim", "melmat must be F_order x (fftlength/2+1 = %d)", (int)h.F);
        need_size(prhs[3], n1, h.R_x, "B_Mel_x (F_order x R_x)");
        const std::vector<double> bmd = per_stream(prhs[4], n1, h.R_d, h.S, "B_Mel_d (F_order x R_d)");
        const double* mm = mxGetDoubles(prhs[2]);
        std::vector<float> mr(n1 * F);  // MATLAB is column-major, the C ABI wants the rows contiguous
        for (size_t m = 0; m < n1; ++m)
            for (size_t f = 0; f < F; ++f) mr[m * F + f] = (float)mm[f * n1 + m];
        const std::vector<float> bx = to_f32(mxGetDoubles(prhs[3]), n1 * h.R_x), bd = to_f32(bmd.data(), bmd.size());
        if (snmf_online_batch_set_mel(h.o, (int32_t)n1, mel_conv, mr.data(), bx.data(), bd.data()) != SNMF_OK)
            mexErrMsgIdAndTxt("snmf:set_mel", "%s", snmf_last_error());
        h.n1 = n1;
    } else if (!strcmp(cmd, "process")) {
        if (nrhs != 5) mexErrMsgIdAndTxt("snmf:usage", "process: handle, pcm, n, flush");
        int64_t np = 0, total = 0, nfl = 0;
        const double* pcm = vector_arg(prhs[2], "pcm (double(pcm) after an 'int16=>int16' read)", &np);
        const std::vector<int64_t> n = counts(prhs[3], "n", &total);
        const double* fl = vector_arg(prhs[4], "flush", &nfl);
        if (total != np) mexErrMsgIdAndTxt("snmf:dim", "n sums to %lld samples, pcm holds %lld", (long long)total, (long long)np);
        if ((int64_t)n.size() != nfl) mexErrMsgIdAndTxt("snmf:dim", "n has %d entries, flush %d", (int)n.size(), (int)nfl);
        const batch_handle& h = g_handles[handle_index(prhs[1])];
        if (n.size() != h.S) mexErrMsgIdAndTxt("snmf:dim", "n and flush must have S = %d entries (got %d)", (int)h.S, (int)n.size());
        if (h.f64) do_process<double>(h, nlhs, plhs, pcm, n, fl);
        else do_process<float>(h, nlhs, plhs, pcm, n, fl);
    } else if (!strcmp(cmd, "restart")) {
        if (nrhs != 6 && nrhs != 7) mexErrMsgIdAndTxt("snmf:usage", "restart: handle, slots, B_DFT_d, H0, Ad_blk0[, B_Mel_d]");
        int64_t ns = 0;
        const double* sv = vector_arg(prhs[2], "slots", &ns);
        for (int i = 3; i < nrhs; ++i) need_double(prhs[i], i == 3 ? "B_DFT_d" : i == 4 ? "H0" : i == 5 ? "Ad_blk0" : "B_Mel_d");
        const batch_handle& h = g_handles[handle_index(prhs[1])];
        const size_t n = (size_t)ns;
        std::vector<int32_t> slots(n);
        std::vector<char> seen(h.S, 0);
        for (size_t i = 0; i < n; ++i) {
            if (!(sv[i] >= 1.0 && sv[i] <= (double)h.S) || sv[i] != std::floor(sv[i]) || seen[(size_t)sv[i] - 1])
                mexErrMsgIdAndTxt("snmf:dim", "slots must be distinct whole numbers in 1..%d (slots(%d) = %g)", (int)h.S, (int)i + 1, sv[i]);
            seen[(size_t)sv[i] - 1] = 1;
            slots[i] = (int32_t)sv[i] - 1;
        }
        if (nrhs == 7 && !h.n1) mexErrMsgIdAndTxt("snmf:usage", "restart: B_Mel_d is for a Mel batch ('set_mel' first)");
        const bool hasB = optional_size(prhs[3], h.F, h.R_d, n, "B_DFT_d (F x R_d per listed slot)");
        const bool hasH = optional_size(prhs[4], h.R_x + h.R_d, 1, n, "H0 (R_x + R_d rows, one column per listed slot)");
        const bool hasA = h.adapt && optional_size(prhs[5], h.R_a, h.m_a, n, "Ad_blk0 (R_a x m_a per listed slot)");
        const bool hasM = nrhs == 7 && optional_size(prhs[6], h.n1, h.R_d, n, "B_Mel_d (F_order x R_d per listed slot)");
        const double* Bd = hasB ? mxGetDoubles(prhs[3]) : nullptr;
        int rc;
        if (h.f64) {
            rc = snmf_online_batch_restart_f64(h.o, (int32_t)n, slots.data(), Bd, hasH ? mxGetDoubles(prhs[4]) : nullptr,
                                               hasA ? mxGetDoubles(prhs[5]) : nullptr);
        } else {
            const std::vector<float> h0 = hasH ? to_f32(mxGetDoubles(prhs[4]), (h.R_x + h.R_d) * n) : std::vector<float>();
            const std::vector<float> ad = hasA ? to_f32(mxGetDoubles(prhs[5]), h.R_a * h.m_a * n) : std::vector<float>();
            rc = snmf_online_batch_restart_mel(h.o, (int32_t)n, slots.data(), Bd, hasM ? mxGetDoubles(prhs[6]) : nullptr, hasH ? h0.data() : nullptr,
                                               hasA ? ad.data() : nullptr);
        }
        if (rc != SNMF_OK) mexErrMsgIdAndTxt("snmf:restart", "%s", snmf_last_error());
    } else if (!strcmp(cmd, "basis") || !strcmp(cmd, "mel_basis")) {
        if (nrhs != 3) mexErrMsgIdAndTxt("snmf:usage", "%s: handle, k", cmd);
        const bool mel = cmd[0] == 'm';
        scalar_arg(prhs[2], "k");
        const batch_handle& h = g_handles[handle_index(prhs[1])];
        const int32_t k = stream_arg(prhs[2], h);
        if (mel && !h.n1) mexErrMsgIdAndTxt("snmf:usage", "mel_basis: not a Mel batch ('set_mel' first)");
        const size_t rows = mel ? h.n1 : h.F;  // the library writes rows x R_d values at this leading dimension
        plhs[0] = mxCreateDoubleMatrix((mwSize)rows, (mwSize)h.R_d, mxREAL);
        const int rc = mel ? snmf_online_batch_get_mel_basis_f64(h.o, k, mxGetDoubles(plhs[0]), (int64_t)rows)
                           : snmf_online_batch_get_basis_f64(h.o, k, mxGetDoubles(plhs[0]), (int64_t)rows);
        if (rc != SNMF_OK) mexErrMsgIdAndTxt("snmf:basis", "%s", snmf_last_error());
    } else if (!strcmp(cmd, "chains")) {
        if (nrhs != 9 && nrhs != 10)
            mexErrMsgIdAndTxt("snmf:usage", "chains: handle, pcm, n_samples, n_files, B_DFT_d, H0, Ad_blk0, chunk_hops[, B_Mel_d]");
        int64_t np = 0, total = 0, nf = 0;
        const double* pcm = vector_arg(prhs[2], "pcm (double(pcm) after an 'int16=>int16' read)", &np);
        const std::vector<int64_t> n_samples = counts(prhs[3], "n_samples", &total);
        const std::vector<int64_t> n_files = counts(prhs[4], "n_files", &nf);
        for (int i = 5; i < nrhs; ++i)
            if (i != 8) need_double(prhs[i], i == 5 ? "B_DFT_d" : i == 6 ? "H0" : i == 7 ? "Ad_blk0" : "B_Mel_d");
        const double ch = scalar_arg(prhs[8], "chunk_hops");
        if (total != np) mexErrMsgIdAndTxt("snmf:dim", "n_samples sums to %lld samples, pcm holds %lld", (long long)total, (long long)np);
        if (nf != (int64_t)n_samples.size())
            mexErrMsgIdAndTxt("snmf:dim", "n_files sums to %lld files, n_samples has %d entries", (long long)nf, (int)n_samples.size());
        if (!(ch >= 0.0 && ch <= 2147483647.0) || ch != std::floor(ch)) mexErrMsgIdAndTxt("snmf:dim", "chunk_hops = %g (0: the default)", ch);
        const batch_handle& h = g_handles[handle_index(prhs[1])];
        const size_t nc = n_files.size();
        if ((nrhs == 10) != (h.n1 != 0)) mexErrMsgIdAndTxt("snmf:usage", "chains: B_Mel_d (tenth argument) is for a Mel batch, and required there");
        if (nc) {  // (no chains: nothing is read, [] will do)
            need_size(prhs[5], h.F, h.R_d * nc, "B_DFT_d (F x R_d per chain)");
            need_size(prhs[6], h.R_x + h.R_d, nc, "H0 (R_x + R_d rows, one column per chain)");
            if (h.adapt) need_size(prhs[7], h.R_a, h.m_a * nc, "Ad_blk0 (R_a x m_a per chain)");
            if (h.n1) need_size(prhs[9], h.n1, h.R_d * nc, "B_Mel_d (F_order x R_d per chain)");
        }
        const double* Ad = h.adapt && nc ? mxGetDoubles(prhs[7]) : nullptr;
        if (h.f64) {
            do_chains<double>(h, nlhs, plhs, pcm, n_samples, n_files, mxGetDoubles(prhs[5]), nullptr, mxGetDoubles(prhs[6]), Ad, (int32_t)ch);
        } else {  // the fp32 images of the start dictionaries, as 'create' and 'set_mel' take them
            std::vector<double> Bd(h.F * h.R_d * nc), Bmd(h.n1 * h.R_d * nc);
            for (size_t i = 0; i < Bd.size(); ++i) Bd[i] = (double)(float)mxGetDoubles(prhs[5])[i];
            for (size_t i = 0; i < Bmd.size(); ++i) Bmd[i] = (double)(float)mxGetDoubles(prhs[9])[i];
            do_chains<float>(h, nlhs, plhs, pcm, n_samples, n_files, Bd.data(), h.n1 ? Bmd.data() : nullptr, mxGetDoubles(prhs[6]), Ad, (int32_t)ch);
        }
    } else if (!strcmp(cmd, "destroy")) {
        if (nrhs != 2) mexErrMsgIdAndTxt("snmf:usage", "destroy: handle");
        const double v = scalar_arg(prhs[1], "handle");
        const size_t i = (v >= 1.0 && v <= (double)g_handles.size() && v == std::floor(v)) ? (size_t)v : 0;  // (anything else: nothing to destroy)
        if (i >= 1 && g_handles[i - 1].o) {
            snmf_online_batch_destroy(g_handles[i - 1].o);
            g_handles[i - 1].o = nullptr;
        }
    } else {
        mexErrMsgIdAndTxt("snmf:usage", "unknown command '%s'", cmd);
    }
}
