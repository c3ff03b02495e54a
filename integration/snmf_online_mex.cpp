// snmf_online_mex.cpp -- MATLAB MEX shim over the online-separation entry points of libsnmf_hip.so
// (include/snmf.h: snmf_online_*).
//
// The binding a maintainer of lordet01/SE_SNMF_NAT adds so that the frame loop of
// src/NTF_sep_event_RT.m:54-135 -- init_buff + one bnmf_sep_event_RT_IS16 call per hop -- runs on an
// MI355X (integration/NTF_sep_event_RT.m is the MATLAB side).  Written against the documented MEX C API.
// MATLAB is not available where this project is built and tested: __graft_entry__.build() syntax-checks this
// file against integration/mex_stub/mex.h, and the tests execute it under a test host that implements that stub
// (tests/mexhost/, tests/test_mexhost.py, tests/test_gpu_mex.py: bit for bit against se_snmf_nat_amd/online.py,
// which makes the same C calls).
//
// Build:  mex -R2018a -I<repo>/include integration/snmf_online_mex.cpp -L<repo>/se_snmf_nat_amd -lsnmf_hip
//
// Calls:
//   h = snmf_online_mex('create', B_DFT_x, B_DFT_d, H0, Ad_blk0, p)   p = the settings struct (global p)
//   snmf_online_mex('set_mel', h, melmat, B_Mel_x, B_Mel_d, MelConv)   B_sep_mode 'Mel': once, right after 'create'
//   x_tilde_int16 = snmf_online_mex('process', h, pcm, flush)          n x 1 int16
//   B_DFT_d = snmf_online_mex('basis', h, F, R_d)          g.B_DFT_d, saved to B_D_u.mat by src/NTF_sep_event_RT.m:138-140
//   snmf_online_mex('destroy', h)
// Every array is checked against the length the C ABI reads or writes (B_DFT_x / B_DFT_d: fftlength/2+1 rows, H0: R_x+R_d,
// Ad_blk0: R_a x m_a when p.adapt_train_N is set, the windows: framelength, 'basis': the F and R_d the handle was created
// with, 'set_mel': melmat F_order x F, B_Mel_x / B_Mel_d F_order x R_x / R_d) -- a mismatch is snmf:dim -- and all of
// 'create' is parsed before the device is touched.
// p.precision = 'fp64' selects the fp64 mode (snmf_online_create_f64 / _process_f64 / _get_basis_f64): MATLAB's doubles cross
// unrounded and every step from PCM to the adapted dictionary runs in fp64 on the device, so the separator follows the
// MATLAB trajectory over whole recordings (docs/WIDENING.md, "Parity horizon").  DFT mode, supervised frame solve.
// In both precisions every array argument, pcm included, must be real double (fread(fid, n, 'int16') returns doubles; an
// 'int16=>int16' read needs double(pcm) first).
// H0 = rand(R_x+R_d,1) after rand('seed',p.random_seed) and Ad_blk0 = rand(p.R_a,p.m_a) are drawn by the
// MATLAB wrapper with MATLAB's own generator (src/sparse_nmf.m:112-114,:133-134; src/init_buff.m:39).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mex.h"
#include "snmf.h"

static snmf_ctx* g_ctx = nullptr;
static std::vector<snmf_online*> g_handles;
static std::vector<char> g_is_f64;  // per handle: made by snmf_online_create_f64
struct handle_dims { size_t F, R_x, R_d; };
static std::vector<handle_dims> g_dims;  // per handle: what 'basis' writes and 'set_mel' reads is sized by these

static void at_exit() {
    for (snmf_online* o : g_handles)
        if (o) snmf_online_destroy(o);
    g_handles.clear();
    g_is_f64.clear();
    g_dims.clear();
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

static std::vector<float> to_f32(const mxArray* a, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
    const size_t n = mxGetNumberOfElements(a);
    const double* d = mxGetDoubles(a);
    std::vector<float> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = (float)d[i];
    return out;
}

static const double* dbl(const mxArray* a, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
    return mxGetDoubles(a);
}

static double scalar_arg(const mxArray* a, const char* what) {
    if (mxIsStruct(a) || mxGetNumberOfElements(a) != 1) mexErrMsgIdAndTxt("snmf:dim", "%s must be a scalar", what);
    return mxGetScalar(a);
}

static void need_size(const mxArray* a, size_t m, size_t n, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
    if (mxGetNumberOfDimensions(a) != 2 || mxGetM(a) != m || mxGetN(a) != n)
        mexErrMsgIdAndTxt("snmf:dim", "%s must be %d x %d (got %d x %d)", what, (int)m, (int)n, (int)mxGetM(a), (int)mxGetN(a));
}

static void need_numel(const mxArray* a, size_t n, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
    if (mxGetNumberOfElements(a) != n) mexErrMsgIdAndTxt("snmf:dim", "%s must have %d entries (got %d)", what, (int)n, (int)mxGetNumberOfElements(a));
}

// 1-based handle -> index into g_handles; a handle that was never made, or was destroyed, is snmf:handle
static size_t handle_index(const mxArray* a) {
    const double v = (mxIsStruct(a) || mxGetNumberOfElements(a) != 1) ? 0.0 : mxGetScalar(a);
    if (!(v >= 1.0 && v <= (double)g_handles.size()) || v != (double)(size_t)v || !g_handles[(size_t)v - 1])
        mexErrMsgIdAndTxt("snmf:handle", "invalid separator handle");
    return (size_t)v - 1;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (snmf_abi_version() != SNMF_ABI_VERSION)  // a stale libsnmf_hip.so must not be driven through newer prototypes
        mexErrMsgIdAndTxt("snmf:abi", "libsnmf_hip.so has ABI version %d, this MEX file was built against %d", snmf_abi_version(), SNMF_ABI_VERSION);
    if (nrhs < 1 || !mxIsChar(prhs[0])) mexErrMsgIdAndTxt("snmf:usage", "first argument: 'create' | 'set_mel' | 'process' | 'basis' | 'destroy'");
    if (nlhs > 1) mexErrMsgIdAndTxt("snmf:nargout", "one output");
    char cmd[16];
    mxGetString(prhs[0], cmd, sizeof cmd);
    if (!strcmp(cmd, "create")) {
        if (nrhs != 6) mexErrMsgIdAndTxt("snmf:usage", "create: B_DFT_x, B_DFT_d, H0, Ad_blk0, p");
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
        q.R_x = (int32_t)mxGetN(prhs[1]);
        q.R_d = (int32_t)mxGetN(prhs[2]);
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
        // what the library reads from each array: F x R_x, F x R_d, R_x + R_d, R_a x m_a (only with adapt_train_N), framelength
        if (q.fftlength < 2 || q.framelength < 1 || q.R_a < 1 || q.m_a < 1) mexErrMsgIdAndTxt("snmf:dim", "p.fftlength, p.framelength, p.R_a and p.m_a must be positive");
        const size_t F = (size_t)q.fftlength / 2 + 1;
        if (q.R_x < 1 || q.R_d < 1) mexErrMsgIdAndTxt("snmf:dim", "B_DFT_x and B_DFT_d must not be empty");
        need_size(prhs[1], F, (size_t)q.R_x, "B_DFT_x (fftlength/2+1 rows)");
        need_size(prhs[2], F, (size_t)q.R_d, "B_DFT_d (fftlength/2+1 rows)");
        need_numel(prhs[3], (size_t)q.R_x + (size_t)q.R_d, "H0 (R_x + R_d)");
        const bool adapt = q.adapt_train_N != 0;  // without it the library never reads Ad_blk0: it gets NULL, [] is fine
        if (adapt) need_size(prhs[4], (size_t)q.R_a, (size_t)q.m_a, "Ad_blk0 (p.R_a x p.m_a)");
        else if (!mxIsEmpty(prhs[4]) && (!mxIsDouble(prhs[4]) || mxIsComplex(prhs[4]))) mexErrMsgIdAndTxt("snmf:type", "Ad_blk0 must be real double or []");
        need_numel(ws, (size_t)q.framelength, "p.win_STFT (framelength)");
        need_numel(wi, (size_t)q.framelength, "p.win_ISTFT (framelength)");
        if (!g_ctx) {
            if (snmf_ctx_create(&g_ctx, 0) != SNMF_OK) mexErrMsgIdAndTxt("snmf:device", "%s", snmf_last_error());
            mexAtExit(at_exit);
            mexLock();
        }
        snmf_online* o = nullptr;
        if (f64) {
            // MATLAB already holds doubles: nothing is rounded on the way in
            if (snmf_online_create_f64(g_ctx, &q, dbl(prhs[1], "B_DFT_x"), dbl(prhs[2], "B_DFT_d"), dbl(prhs[3], "H0"),
                                       adapt ? dbl(prhs[4], "Ad_blk0") : nullptr, dbl(ws, "win_STFT"), dbl(wi, "win_ISTFT"), &o) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:create", "%s", snmf_last_error());
        } else {
            const std::vector<float> Bx = to_f32(prhs[1], "B_DFT_x"), Bd = to_f32(prhs[2], "B_DFT_d"), H0 = to_f32(prhs[3], "H0");
            const std::vector<float> Ad = adapt ? to_f32(prhs[4], "Ad_blk0") : std::vector<float>();
            const std::vector<float> w1 = to_f32(ws, "win_STFT"), w2 = to_f32(wi, "win_ISTFT");
            if (snmf_online_create(g_ctx, &q, Bx.data(), Bd.data(), H0.data(), adapt ? Ad.data() : nullptr, w1.data(), w2.data(), &o) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:create", "%s", snmf_last_error());
        }
        g_handles.push_back(o);
        g_is_f64.push_back(f64 ? 1 : 0);
        g_dims.push_back(handle_dims{F, (size_t)q.R_x, (size_t)q.R_d});
        plhs[0] = mxCreateDoubleScalar((double)g_handles.size());
    } else if (!strcmp(cmd, "set_mel")) {
        // snmf_online_mex('set_mel', h, melmat, B_Mel_x, B_Mel_d, MelConv): melmat = g.melmat (F_order x F), init_buff.m:46
        if (nrhs != 6) mexErrMsgIdAndTxt("snmf:usage", "set_mel: handle, melmat, B_Mel_x, B_Mel_d, MelConv");
        const size_t hi = handle_index(prhs[1]);
        snmf_online* o = g_handles[hi];
        if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2])) mexErrMsgIdAndTxt("snmf:type", "melmat must be real double");
        const mwSize n1 = mxGetM(prhs[2]), F = mxGetN(prhs[2]);
        // the library reads F_order x F, F_order x R_x and F_order x R_d values, F, R_x and R_d being the handle's
        if (n1 < 1 || F != g_dims[hi].F) mexErrMsgIdAndTxt("snmf:dim", "melmat must be F_order x (fftlength/2+1 = %d)", (int)g_dims[hi].F);
        need_size(prhs[3], n1, g_dims[hi].R_x, "B_Mel_x (F_order x R_x)");
        need_size(prhs[4], n1, g_dims[hi].R_d, "B_Mel_d (F_order x R_d)");
        const bool mel_conv = scalar_arg(prhs[5], "MelConv") != 0;
        const double* mm = mxGetDoubles(prhs[2]);
        std::vector<float> mr((size_t)n1 * F);  // MATLAB is column-major, the C ABI wants the rows contiguous
        for (mwSize m = 0; m < n1; ++m)
            for (mwSize f = 0; f < F; ++f) mr[(size_t)m * F + f] = (float)mm[(size_t)f * n1 + m];
        const std::vector<float> bx = to_f32(prhs[3], "B_Mel_x"), bd = to_f32(prhs[4], "B_Mel_d");
        if (snmf_online_set_mel(o, (int32_t)n1, mel_conv, mr.data(), bx.data(), bd.data()) != SNMF_OK)
            mexErrMsgIdAndTxt("snmf:set_mel", "%s", snmf_last_error());
    } else if (!strcmp(cmd, "process")) {
        if (nrhs != 4) mexErrMsgIdAndTxt("snmf:usage", "process: handle, pcm, flush");
        const size_t hi = handle_index(prhs[1]);
        snmf_online* o = g_handles[hi];
        const int flush = scalar_arg(prhs[3], "flush") != 0;
        if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2])) mexErrMsgIdAndTxt("snmf:type", "pcm must be real double (double(pcm) after an 'int16=>int16' read)");
        if (mxGetM(prhs[2]) > 1 && mxGetN(prhs[2]) > 1) mexErrMsgIdAndTxt("snmf:dim", "pcm must be a vector");
        const int64_t np = (int64_t)mxGetNumberOfElements(prhs[2]);
        const int64_t cap = np + 64 * 4096;
        std::vector<int16_t> out((size_t)cap);
        int64_t n = 0;
        if (g_is_f64[hi]) {
            if (snmf_online_process_f64(o, dbl(prhs[2], "pcm"), np, flush, nullptr, out.data(), nullptr, nullptr, cap, &n) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:process", "%s", snmf_last_error());
        } else {
            const std::vector<float> pcm = to_f32(prhs[2], "pcm");
            if (snmf_online_process_f32(o, pcm.data(), np, flush, nullptr, out.data(), nullptr, nullptr, cap, &n) != SNMF_OK)
                mexErrMsgIdAndTxt("snmf:process", "%s", snmf_last_error());
        }
        plhs[0] = mxCreateNumericMatrix((mwSize)n, 1, mxINT16_CLASS, mxREAL);
        std::memcpy(mxGetInt16s(plhs[0]), out.data(), (size_t)n * 2);
    } else if (!strcmp(cmd, "basis")) {
        if (nrhs != 4) mexErrMsgIdAndTxt("snmf:usage", "basis: handle, F, R_d");
        const size_t hi = handle_index(prhs[1]);
        snmf_online* o = g_handles[hi];
        // the library writes the handle's F x R_d values: the sizes the caller states must be those
        const double Fa = scalar_arg(prhs[2], "F"), Ra = scalar_arg(prhs[3], "R_d");
        if (Fa != (double)g_dims[hi].F || Ra != (double)g_dims[hi].R_d)
            mexErrMsgIdAndTxt("snmf:dim", "basis: this separator's B_DFT_d is %d x %d (asked for %g x %g)", (int)g_dims[hi].F, (int)g_dims[hi].R_d, Fa, Ra);
        const mwSize F = g_dims[hi].F, Rd = g_dims[hi].R_d;
        plhs[0] = mxCreateDoubleMatrix(F, Rd, mxREAL);
        double* d = mxGetDoubles(plhs[0]);
        if (g_is_f64[hi]) {  // the fp64 master, unrounded
            if (snmf_online_get_basis_f64(o, d, (int64_t)F) != SNMF_OK) mexErrMsgIdAndTxt("snmf:basis", "%s", snmf_last_error());
        } else {
            std::vector<float> B((size_t)F * Rd);
            if (snmf_online_get_basis_f32(o, B.data(), (int64_t)F) != SNMF_OK) mexErrMsgIdAndTxt("snmf:basis", "%s", snmf_last_error());
            for (size_t i = 0; i < B.size(); ++i) d[i] = (double)B[i];
        }
    } else if (!strcmp(cmd, "destroy")) {
        if (nrhs != 2) mexErrMsgIdAndTxt("snmf:usage", "destroy: handle");
        const double v = scalar_arg(prhs[1], "handle");
        const size_t i = (v >= 1.0 && v <= (double)g_handles.size()) ? (size_t)v : 0;  // (anything else: nothing to destroy)
        if (i >= 1 && g_handles[i - 1]) {
            snmf_online_destroy(g_handles[i - 1]);
            g_handles[i - 1] = nullptr;
        }
    } else {
        mexErrMsgIdAndTxt("snmf:usage", "unknown command '%s'", cmd);
    }
}
