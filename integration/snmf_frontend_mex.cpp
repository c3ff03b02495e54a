// snmf_frontend_mex.cpp -- MATLAB MEX shim for the device spectrogram front-end of libsnmf_hip.so
// (C ABI: include/snmf.h, snmf_stft_features_f32 / snmf_mel_features_f32 and, in the fp64 mode, snmf_stft_features_fp64 /
// snmf_mel_features_fp64).
//
// Replaces, for the callers that build V before a solve, the feature lines of the reference:
//     [TF_mag, ~] = stft_fft(s, p.framelength, p.frameshift, p.fftlength, DC_bin, p.win_STFT, p.preemph);   run_basis_train.m:60
//     TF_mag = TF_mag(:, any(TF_mag,1)); [TF_mag, ~] = frame_splice(TF_mag, p);                              :61-62
//     TF_mag = TF_mag .^ p.pow + p.nonzerofloor;                                                             :63
//     TF_Mel(...) = melmat * TF_mag(...)                                                                     :70-78
// (run_basis_DNMF.m:13-34 and run_basis_DNMF_Mel.m form Y, X, D the same way).
//
//     TF_mag = snmf_frontend_mex('stft', s, p, DC_bin)        s: samples (real double vector), p: settings struct
//     TF_Mel = snmf_frontend_mex('mel', TF_mag, melmat, K)    melmat: F_order x (fftlength/2+1) (= mel_matrix(...)'), K = 2*Splice+1
//     TF_Mel = snmf_frontend_mex('mel', TF_mag, melmat, K, precision)
//   p.snmf_precision (resp. the fifth argument of 'mel') = 'fp64': computed in double from MATLAB's doubles (the *_fp64 entries);
//   'fp32', empty or absent: the default.  Any other string is an error.
//
// Written against the documented MEX C API.  MATLAB is not available where this project is built and tested:
// __graft_entry__.build() syntax-checks this file against integration/mex_stub/mex.h, and the tests execute it under a test
// host that implements that stub (tests/mexhost/, tests/test_mexhost.py, tests/test_gpu_mex.py).  Every argument is checked
// before the device is touched.  Build:
//     mex -R2018a -I<repo>/include integration/snmf_frontend_mex.cpp -L<repo>/se_snmf_nat_amd -lsnmf_hip
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mex.h"
#include "snmf.h"

static snmf_ctx* g_ctx = nullptr;

static void at_exit() {
    if (g_ctx) {
        snmf_ctx_destroy(g_ctx);
        g_ctx = nullptr;
    }
}
static void need_ctx() {
    if (g_ctx) return;
    if (snmf_ctx_create(&g_ctx, 0) != SNMF_OK) mexErrMsgIdAndTxt("snmf:device", "%s", snmf_last_error());
    mexLock();
    mexAtExit(at_exit);
}
static double field(const mxArray* s, const char* name) {
    const mxArray* f = mxGetField(s, 0, name);
    if (!f || mxIsEmpty(f)) mexErrMsgIdAndTxt("snmf:field", "Reference to non-existent field '%s'.", name);
    return mxGetScalar(f);
}
static double scalar_arg(const mxArray* a, const char* what) {
    if (mxIsStruct(a) || mxGetNumberOfElements(a) != 1) mexErrMsgIdAndTxt("snmf:dim", "%s must be a scalar", what);
    return mxGetScalar(a);
}
static std::vector<float> to_float(const mxArray* a, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
    const size_t n = mxGetNumberOfElements(a);
    const double* d = mxGetDoubles(a);
    std::vector<float> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = (float)d[i];
    return out;
}
// 'fp64': the fp64 mode; any other string but 'fp32' is an error (as opts.precision of sparse_nmf_mex.cpp)
static bool fp64_mode(const mxArray* pr, const char* what) {
    if (!pr || mxIsEmpty(pr)) return false;
    char prec[16] = "";
    if (!mxIsChar(pr) || mxGetString(pr, prec, sizeof prec) != 0) mexErrMsgIdAndTxt("snmf:type", "%s must be 'fp32' or 'fp64'", what);
    if (std::strcmp(prec, "fp64") == 0) return true;
    if (std::strcmp(prec, "fp32") != 0) mexErrMsgIdAndTxt("snmf:type", "%s must be 'fp32' or 'fp64' (got '%s')", what, prec);
    return false;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (snmf_abi_version() != SNMF_ABI_VERSION)  // a stale libsnmf_hip.so must not be driven through newer prototypes
        mexErrMsgIdAndTxt("snmf:abi", "libsnmf_hip.so has ABI version %d, this MEX file was built against %d", snmf_abi_version(), SNMF_ABI_VERSION);
    if (nrhs < 1 || !mxIsChar(prhs[0])) mexErrMsgIdAndTxt("snmf:nargin", "usage: snmf_frontend_mex('stft'|'mel', ...)");
    if (nlhs > 1) mexErrMsgIdAndTxt("snmf:nargout", "one output");
    char cmd[16];
    mxGetString(prhs[0], cmd, sizeof cmd);
    if (std::string(cmd) == "stft") {
        if (nrhs != 4 || !mxIsStruct(prhs[2])) mexErrMsgIdAndTxt("snmf:nargin", "TF_mag = snmf_frontend_mex('stft', s, p, DC_bin)");
        const mxArray* p = prhs[2];
        const bool f64 = fp64_mode(mxGetField(p, 0, "snmf_precision"), "p.snmf_precision");
        const std::vector<float> s = f64 ? std::vector<float>() : to_float(prhs[1], "s");
        if (f64 && (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1]))) mexErrMsgIdAndTxt("snmf:type", "s must be real double");
        const size_t n_s = mxGetNumberOfElements(prhs[1]);
        const mxArray* win = mxGetField(p, 0, "win_STFT");
        if (!win || !mxIsDouble(win)) mexErrMsgIdAndTxt("snmf:field", "Reference to non-existent field 'win_STFT'.");
        snmf_stft_params sp;
        std::memset(&sp, 0, sizeof sp);
        sp.framelength = (int32_t)field(p, "framelength");
        sp.frameshift = (int32_t)field(p, "frameshift");
        sp.fftlength = (int32_t)field(p, "fftlength");
        sp.dcbin = (int32_t)scalar_arg(prhs[3], "DC_bin");
        sp.splice = (int32_t)field(p, "Splice");
        sp.preemph = field(p, "preemph");
        sp.pow = field(p, "pow");
        sp.nonzerofloor = field(p, "nonzerofloor");
        if (mxGetNumberOfElements(win) != (size_t)sp.framelength) mexErrMsgIdAndTxt("snmf:dim", "win_STFT must have framelength entries");
        if (mxGetM(prhs[1]) > 1 && mxGetN(prhs[1]) > 1) mexErrMsgIdAndTxt("snmf:dim", "s must be a vector");
        sp.window = mxGetDoubles(win);
        need_ctx();
        const int64_t nfr = snmf_stft_num_frames(&sp, (int64_t)n_s);
        const size_t F = (size_t)(2 * sp.splice + 1) * (size_t)(sp.fftlength / 2 + 1);
        int32_t n_out = 0;
        if (f64) {  // doubles in, doubles out: straight from and into MATLAB's arrays
            plhs[0] = mxCreateDoubleMatrix(F, (size_t)(nfr > 0 ? nfr : 0), mxREAL);
            if (snmf_stft_features_fp64(g_ctx, &sp, mxGetDoubles(prhs[1]), (int64_t)n_s, 0, mxGetDoubles(plhs[0]), (int64_t)F, 0, &n_out) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:stft", "%s", snmf_last_error());
            return;
        }
        std::vector<float> V(F * (size_t)(nfr > 0 ? nfr : 1));
        if (snmf_stft_features_f32(g_ctx, &sp, s.data(), (int64_t)n_s, 0, V.data(), (int64_t)F, 0, &n_out) != SNMF_OK)
            mexErrMsgIdAndTxt("snmf:stft", "%s", snmf_last_error());
        plhs[0] = mxCreateDoubleMatrix(F, (size_t)n_out, mxREAL);
        double* o = mxGetDoubles(plhs[0]);
        for (size_t i = 0; i < F * (size_t)n_out; ++i) o[i] = (double)V[i];
    } else if (std::string(cmd) == "mel") {
        if (nrhs != 4 && nrhs != 5) mexErrMsgIdAndTxt("snmf:nargin", "TF_Mel = snmf_frontend_mex('mel', TF_mag, melmat, K[, precision])");
        const bool f64 = nrhs == 5 && fp64_mode(prhs[4], "precision");
        const std::vector<float> V = f64 ? std::vector<float>() : to_float(prhs[1], "TF_mag");
        if (f64 && (!mxIsDouble(prhs[1]) || mxIsComplex(prhs[1]))) mexErrMsgIdAndTxt("snmf:type", "TF_mag must be real double");
        const size_t rows = mxGetM(prhs[1]), T = mxGetN(prhs[1]);
        if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2])) mexErrMsgIdAndTxt("snmf:type", "melmat must be real double");
        const size_t M = mxGetM(prhs[2]), n = mxGetN(prhs[2]);
        const int K = (int)scalar_arg(prhs[3], "K");
        if (M < 1 || n < 1) mexErrMsgIdAndTxt("snmf:dim", "melmat must not be empty");
        if (K < 1 || rows != (size_t)K * n) mexErrMsgIdAndTxt("snmf:dim", "TF_mag must have K * size(melmat,2) rows");
        if (T == 0) {  // no frames: nothing for the device to do
            plhs[0] = mxCreateDoubleMatrix((size_t)K * M, 0, mxREAL);
            return;
        }
        need_ctx();
        // the C ABI takes melmat row-major (M x n); MATLAB stores it column-major
        const double* mm = mxGetDoubles(prhs[2]);
        if (f64) {
            std::vector<double> mel64(M * n);
            for (size_t i = 0; i < M; ++i)
                for (size_t j = 0; j < n; ++j) mel64[i * n + j] = mm[j * M + i];
            plhs[0] = mxCreateDoubleMatrix((size_t)K * M, T, mxREAL);
            if (snmf_mel_features_fp64(g_ctx, mel64.data(), (int32_t)M, (int32_t)n, K, mxGetDoubles(prhs[1]), (int64_t)rows, (int32_t)T,
                                                mxGetDoubles(plhs[0]), (int64_t)((size_t)K * M), 0) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:mel", "%s", snmf_last_error());
            return;
        }
        std::vector<float> mel(M * n);
        for (size_t i = 0; i < M; ++i)
            for (size_t j = 0; j < n; ++j) mel[i * n + j] = (float)mm[j * M + i];
        std::vector<float> out((size_t)K * M * T);
        if (snmf_mel_features_f32(g_ctx, mel.data(), (int32_t)M, (int32_t)n, K, V.data(), (int64_t)rows, (int32_t)T, out.data(),
                                  (int64_t)((size_t)K * M), 0) != SNMF_OK)
            mexErrMsgIdAndTxt("snmf:mel", "%s", snmf_last_error());
        plhs[0] = mxCreateDoubleMatrix((size_t)K * M, T, mxREAL);
        double* o = mxGetDoubles(plhs[0]);
        for (size_t i = 0; i < out.size(); ++i) o[i] = (double)out[i];
    } else {
        mexErrMsgIdAndTxt("snmf:cmd", "unknown command '%s'", cmd);
    }
}
