// snmf_batch_mex.cpp -- MATLAB MEX shim over the batch engines of libsnmf_hip.so (include/snmf.h: snmf_sparse_nmf_batch_*,
// snmf_batch_*, snmf_run_basis_dnmf_batch_*, snmf_run_basis_dnmf_audio_batch_*, snmf_run_basis_train_audio_batch_*,
// snmf_train_signals_*, snmf_run_basis_train_signals_batch_*), command first, written like snmf_online_batch_mex.cpp.
//
// The binding a maintainer of lordet01/SE_SNMF_NAT adds so that the training stage of Do_MultiBatch_IS16_20160324.m:96-161 --
// run_basis_train over the event classes and the noise types, run_basis_DNMF / run_basis_DNMF_Mel per pair -- runs as one call
// per stage (integration/batch/sparse_nmf_batch.m, run_basis_train_batch.m and run_basis_DNMF_batch.m are the MATLAB side).
// Written against the documented MEX C API.  MATLAB is not available where this project is built and tested:
// __graft_entry__.build() syntax-checks this file against integration/mex_stub/mex.h, and the tests execute it under the test
// host (tests/test_batch_mex_api.py: every refusal without a device, also as a stand-alone program under the address and
// undefined-behaviour sanitizers; tests/test_gpu_batch_mex.py: every command bit for bit against the Python binding, which
// makes the same C calls).
//
// Build:  mex -R2018a -I<repo>/include integration/snmf_batch_mex.cpp -L<repo>/se_snmf_nat_amd -lsnmf_hip
//
// PACKED ARRAYS.  A list of per-problem matrices crosses as ONE real double array holding the matrices' column-major
// elements, one problem after the other (no cells); only its element count is looked at, except where a row count is taken
// from it (V, Y).  Equal-shaped problems are simply [V_1, V_2, ...].  The shapes come from count vectors (T, n_samples, n_x,
// clip_len, ..., p.r): n x 1 doubles holding whole numbers >= 1.  A rank-like argument (p.r, p.R_x, p.R_d, n_atoms) is a
// scalar, or a vector with one entry per problem; a vector whose entries all agree is the scalar.  Outputs come back packed
// the same way, as a matrix of side-by-side blocks where the blocks share the row count and as a column where they do not.
//
//   [W, H, div, cost, n_iter] = snmf_batch_mex('solve', V, T, W0, H0, p, settings)
//         V F x sum(T); W0 the F x r_k, H0 the r_k x T_k initial factors; p: r, cf / beta, sparsity (scalar, or r x 1 with one
//         rank), max_iter, conv_eps, cost_check, floor_v (default 1), w_update_ind, h_update_ind (r entries, or one for all).
//         W F x sum(r_k); H packed; div, cost max_iter x n (zero past a problem's stop); n_iter n x 1.
//         snmf_sparse_nmf_batch_f64 / _fp64; ranks or settings per problem: the resident fp64 handle
//         (snmf_batch_create_ranks_fp64 / _settings_fp64, set_problem, run, get, destroy)
//   [B_hat, A_hat, n_iter] = snmf_batch_mex('dnmf', Y, X, D, T, B, H0, p, settings)
//         Y, X, D F x sum(T); B the F x (R_x+R_d)_k bases; H0 the (R_x+R_d)_k x T_k activations of solve 1 (required);
//         p: R_x, R_d and the solver fields; p.snmf_single = 1: the arrays cross to the library as float
//         (snmf_run_basis_dnmf_batch_f32, fp32 engine only).  B_hat F x sum(r_k); A_hat packed; n_iter n x 3.
//         snmf_run_basis_dnmf_batch_f64 / _f32 / _fp64 / _ranks_fp64
//   [B_hat, A_hat, n_iter] = snmf_batch_mex('dnmf_audio', x, n_x, d, n_d, B, H0, p, melmat, settings)
//         x, d: the waveforms, concatenated; melmat [] (DFT) or F_order x (fftlength/2+1) = mel_matrix(...)'; H0 packed, or []:
//         problem k is drawn on the device, keyed by p.random_seed + k - 1.  p: the front-end fields, R_x, R_d, the solver fields.
//         snmf_run_basis_dnmf_audio_batch_f64 / _fp64 / _ranks_fp64
//   [B_DFT, B_Mel, A_DFT, A_Mel, n_iter] = snmf_batch_mex('train', s, n_samples, sample_idx, n_atoms, H0, p, melmat, DC_bin, settings)
//         s: the training signals, concatenated; sample_idx: the exemplar columns of every problem, concatenated, 1-BASED
//         (randsample); n_atoms = cluster_buff * R; H0 the n_atoms_k x T_k start of both solves, or []: drawn on the device,
//         every problem keyed by p.random_seed; p.train_Exemplar, p.domain_DD / p.alpha_eta as in run_basis_train.m:64-67,:84.
//         RAW results (the renormalisation of :113-116 and the k-means stay with the caller): B_DFT F x sum(n_atoms_k),
//         B_Mel likewise, A_DFT / A_Mel packed (0 with train_Exemplar), n_iter n x 2.
//         snmf_run_basis_train_audio_batch_f64 / _fp64 / _ranks_fp64 / _settings_fp64
//   h = snmf_batch_mex('assemble', clips, clip_len, n_clips, mode, range, p)
//         clips: all clips of all classes in class order, concatenated, as doubles wavread(.) * 32767; clip_len per clip;
//         n_clips and mode (0 cut, 1 VAD, 2 range) per class; range [] or 2 x clips, [v_start; v_end] 1-based and inclusive,
//         read for the clips of mode-2 classes; p: fs, train_seq_len_max, train_file_len_max.  snmf_train_signals_assemble_f64
//   [n_samples, clips_used] = snmf_batch_mex('signals_info', h)
//   s_full = snmf_batch_mex('signals_get', h, k)                 class k, 1-based
//   [B_DFT, B_Mel, A_DFT, A_Mel, n_iter] = snmf_batch_mex('train_signals', h, sample_idx, n_atoms, H0, p, melmat, DC_bin, settings)
//         'train' on the resident signals of h.  snmf_run_basis_train_signals_batch_f64 / _fp64 / _ranks_fp64 / _settings_fp64
//   snmf_batch_mex('signals_destroy', h)
//
//   settings: [] or n x 4, [beta sparsity conv_eps max_iter] per problem (beta: 0 is, 1 kl, 2 ed).  p.snmf_precision: 'fp32' (or
//   absent) or 'fp64'.  Ranks or settings per problem need 'fp64' (snmf:unsupported otherwise).  h is a 1-based index into a
//   registry kept here; the live handles and then the context are destroyed when the MEX file is cleared.
// Every array is checked for its class (snmf:type) and for the exact length the C ABI reads or writes (snmf:dim; a field of p:
// snmf:field; the precision: snmf:precision) before the context is created; a command on a handle checks what does not depend
// on the handle first, then the handle (snmf:handle), then the sizes the handle fixes.  A failed library call carries
// snmf_last_error() under snmf:<command>.  Left out: the missing-data batch (snmf_mdi_batch_fp64) and device lists.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mex.h"
#include "snmf.h"

static snmf_ctx* g_ctx = nullptr;
struct signals_handle {
    snmf_train_signals* s;
    std::vector<int64_t> len;  // samples of s_full per class
};
static std::vector<signals_handle> g_signals;

static void at_exit() {
    for (signals_handle& h : g_signals)
        if (h.s) snmf_train_signals_destroy(h.s);
    g_signals.clear();
    if (g_ctx) {
        snmf_ctx_destroy(g_ctx);
        g_ctx = nullptr;
    }
}
static void need_ctx() {
    if (g_ctx) return;
    if (snmf_ctx_create(&g_ctx, 0) != SNMF_OK) mexErrMsgIdAndTxt("snmf:device", "%s", snmf_last_error());
    mexLock();  // keeps the context, and with it the resident signals, alive between calls
    mexAtExit(at_exit);
}

// ---- arguments ---------------------------------------------------------------------------------------------------------------
static void need_double(const mxArray* a, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("snmf:type", "%s must be real double", what);
}
static void need_struct(const mxArray* a, const char* what) {
    if (!mxIsStruct(a) || mxGetNumberOfElements(a) != 1) mexErrMsgIdAndTxt("snmf:type", "%s must be a 1 x 1 struct", what);
}
static double field(const mxArray* s, const char* name) {
    const mxArray* f = mxGetField(s, 0, name);
    if (!f || mxIsEmpty(f) || mxIsStruct(f)) mexErrMsgIdAndTxt("snmf:field", "Reference to non-existent field '%s'.", name);
    return mxGetScalar(f);
}
static double field_or(const mxArray* s, const char* name, double dflt) {
    const mxArray* f = mxGetField(s, 0, name);
    return (!f || mxIsEmpty(f) || mxIsStruct(f)) ? dflt : mxGetScalar(f);
}
static double scalar_arg(const mxArray* a, const char* what) {
    if (mxIsStruct(a) || mxGetNumberOfElements(a) != 1) mexErrMsgIdAndTxt("snmf:dim", "%s must be a scalar", what);
    need_double(a, what);
    return mxGetScalar(a);
}
static bool is_vector(const mxArray* a) { return mxGetNumberOfDimensions(a) == 2 && (mxGetM(a) <= 1 || mxGetN(a) <= 1); }

// a whole number in [lo, hi], exactly representable
static bool whole(double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); }

// a count vector: doubles holding whole numbers in [lo, hi] -> int64; at least one entry
static std::vector<int64_t> counts(const mxArray* a, const char* what, double lo, double hi) {
    need_double(a, what);
    if (!is_vector(a)) mexErrMsgIdAndTxt("snmf:dim", "%s must be a vector", what);
    const size_t n = mxGetNumberOfElements(a);
    if (n < 1) mexErrMsgIdAndTxt("snmf:dim", "%s is empty: the batch must hold at least one problem", what);
    const double* d = mxGetDoubles(a);
    std::vector<int64_t> out(n);
    for (size_t i = 0; i < n; ++i) {
        if (!whole(d[i], lo, hi)) mexErrMsgIdAndTxt("snmf:dim", "%s(%d) = %g is not a whole number in [%g, %g]", what, (int)i + 1, d[i], lo, hi);
        out[i] = (int64_t)d[i];
    }
    return out;
}
static const double kI32 = 2147483647.0, kI53 = 9007199254740992.0;

static std::vector<int32_t> narrow(const std::vector<int64_t>& v) { return std::vector<int32_t>(v.begin(), v.end()); }
static int64_t sum(const std::vector<int64_t>& v) {
    int64_t s = 0;
    for (int64_t x : v) s += x;
    return s;
}
static int64_t dot(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    int64_t s = 0;
    for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
    return s;
}
static int64_t largest(const std::vector<int64_t>& v) {
    int64_t m = v[0];
    for (int64_t x : v) m = x > m ? x : m;
    return m;
}
static void same_length(size_t got, size_t n, const char* what, const char* ref) {
    if (got != n) mexErrMsgIdAndTxt("snmf:dim", "%s has %d entries, %s has %d", what, (int)got, ref, (int)n);
}

// a rank-like argument: a scalar (-> n times), or one entry per problem (n == 0: its own length decides)
struct ranks {
    std::vector<int64_t> v;
    bool mixed;  // the entries differ
};
static ranks ranks_arg(const mxArray* a, size_t n, const char* what) {
    ranks r;
    r.v = counts(a, what, 1.0, kI32);
    if (n && r.v.size() == 1) r.v.assign(n, r.v[0]);
    if (n) same_length(r.v.size(), n, what, "the batch");
    r.mixed = false;
    for (int64_t x : r.v) r.mixed = r.mixed || x != r.v[0];
    return r;
}

static const mxArray* need_field(const mxArray* p, const char* name) {
    const mxArray* f = mxGetField(p, 0, name);
    if (!f) mexErrMsgIdAndTxt("snmf:field", "Reference to non-existent field '%s'.", name);
    return f;
}

// a packed array: real double with exactly `want` elements
static const double* packed(const mxArray* a, const char* what, int64_t want) {
    need_double(a, what);
    if (mxGetNumberOfDimensions(a) != 2 || (int64_t)mxGetNumberOfElements(a) != want)
        mexErrMsgIdAndTxt("snmf:dim", "%s holds %lld elements, the counts give %lld", what, (long long)mxGetNumberOfElements(a), (long long)want);
    return mxGetDoubles(a);
}
// F x (anything): the row count comes from the array
static const double* packed_rows(const mxArray* a, const char* what, int64_t* F, int64_t cols) {
    need_double(a, what);
    if (mxGetNumberOfDimensions(a) != 2 || mxGetM(a) < 1 || (int64_t)mxGetN(a) != cols)
        mexErrMsgIdAndTxt("snmf:dim", "%s must be F x %lld, the problems side by side (got %d x %d)", what, (long long)cols, (int)mxGetM(a), (int)mxGetN(a));
    *F = (int64_t)mxGetM(a);
    return mxGetDoubles(a);
}

// p.snmf_precision = 'fp64': the fp64 engine; 'fp32' or absent: the default; anything else is snmf:precision
static bool fp64_mode(const mxArray* p) {
    const mxArray* pr = mxGetField(p, 0, "snmf_precision");
    if (!pr || mxIsEmpty(pr)) return false;
    char prec[16] = "";
    if (!mxIsChar(pr) || mxGetString(pr, prec, sizeof prec) != 0) prec[0] = 0;  // not a string, or too long to be one of the two
    if (std::strcmp(prec, "fp64") == 0) return true;
    if (std::strcmp(prec, "fp32") != 0) mexErrMsgIdAndTxt("snmf:precision", "p.snmf_precision must be 'fp32' or 'fp64'");
    return false;
}

// settings: [] -> false; else n x 4, [beta sparsity conv_eps max_iter] per problem (n == 0: the rows decide)
static bool settings_arg(const mxArray* a, size_t n, std::vector<snmf_problem_settings>& out) {
    need_double(a, "settings");
    out.clear();
    if (mxIsEmpty(a)) return false;
    const size_t rows = mxGetM(a);
    if (mxGetNumberOfDimensions(a) != 2 || mxGetN(a) != 4 || (n && rows != n))
        mexErrMsgIdAndTxt("snmf:dim", "settings must be [] or n x 4, [beta sparsity conv_eps max_iter] per problem (got %d x %d)", (int)rows, (int)mxGetN(a));
    const double* d = mxGetDoubles(a);
    out.resize(rows);
    for (size_t k = 0; k < rows; ++k) {
        std::memset(&out[k], 0, sizeof out[k]);
        out[k].beta = d[k];
        out[k].sparsity = d[rows + k];
        out[k].conv_eps = d[2 * rows + k];
        if (!whole(d[3 * rows + k], 0.0, kI32)) mexErrMsgIdAndTxt("snmf:dim", "settings(%d, 4) = %g is not an iteration limit", (int)k + 1, d[3 * rows + k]);
        out[k].max_iter = (int32_t)d[3 * rows + k];
    }
    return true;
}
static int32_t largest_limit(const std::vector<snmf_problem_settings>& s) {
    int32_t m = 0;
    for (const snmf_problem_settings& x : s) m = x.max_iter > m ? x.max_iter : m;
    return m;
}
static void fp64_only(bool f64, bool per_problem) {
    if (per_problem && !f64)
        mexErrMsgIdAndTxt("snmf:unsupported", "ranks or settings per problem need p.snmf_precision = 'fp64': the fp32 batch engine has one rank and one settings struct for all problems");
}

template <typename T>
static std::vector<T> as_elem(const double* d, size_t n) {
    std::vector<T> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = (T)d[i];  // a plain cast: round to nearest
    return out;
}
// the pointer table of a packed array: problem k starts size[k] elements after problem k - 1
template <typename T>
static std::vector<T*> table(T* base, const std::vector<int64_t>& size) {
    std::vector<T*> out(size.size());
    int64_t at = 0;
    for (size_t k = 0; k < size.size(); ++k) {
        out[k] = base + at;
        at += size[k];
    }
    return out;
}
static std::vector<int64_t> times(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    std::vector<int64_t> out(a.size());
    for (size_t i = 0; i < a.size(); ++i) out[i] = a[i] * b[i];
    return out;
}
static std::vector<int64_t> times(const std::vector<int64_t>& a, int64_t b) {
    std::vector<int64_t> out(a.size());
    for (size_t i = 0; i < a.size(); ++i) out[i] = a[i] * b;
    return out;
}

// melmat (F_order x nb, column-major in MATLAB) -> ROW-major float (double for the fp64 engine), as the C ABI reads it
template <typename T>
static std::vector<T> mel_rows(const mxArray* m, int nb) {
    const int M = (int)mxGetM(m);
    const double* d = mxGetDoubles(m);
    std::vector<T> out((size_t)M * nb);
    for (int j = 0; j < M; ++j)
        for (int f = 0; f < nb; ++f) out[(size_t)j * nb + f] = (T)d[(size_t)f * M + j];
    return out;
}
// [] -> 0; else the row count F_order of an F_order x nb table
static int mel_order(const mxArray* m, int nb) {
    need_double(m, "melmat");
    if (mxIsEmpty(m)) return 0;
    if (mxGetNumberOfDimensions(m) != 2 || (int)mxGetN(m) != nb)
        mexErrMsgIdAndTxt("snmf:dim", "melmat must be [] or F_order x (fftlength/2+1 = %d), mel_matrix(...)' (got %d x %d)", nb, (int)mxGetM(m), (int)mxGetN(m));
    return (int)mxGetM(m);
}
static void fill_stft(const mxArray* p, std::vector<double>& win, snmf_stft_params* sp, double dcbin) {
    std::memset(sp, 0, sizeof *sp);
    sp->framelength = (int32_t)field(p, "framelength");
    sp->frameshift = (int32_t)field(p, "frameshift");
    sp->fftlength = (int32_t)field(p, "fftlength");
    sp->dcbin = (int32_t)dcbin;
    sp->splice = (int32_t)field_or(p, "Splice", 0);
    sp->preemph = field_or(p, "preemph", 0.0);
    sp->pow = field(p, "pow");
    sp->nonzerofloor = field(p, "nonzerofloor");
    if (sp->framelength < 1 || sp->frameshift < 1 || sp->fftlength < 2 || sp->splice < 0)
        mexErrMsgIdAndTxt("snmf:field", "p.framelength, p.frameshift and p.fftlength must be positive, p.Splice not negative");
    const mxArray* w = mxGetField(p, 0, "win_STFT");
    if (!w || !mxIsDouble(w) || (int32_t)mxGetNumberOfElements(w) != sp->framelength)
        mexErrMsgIdAndTxt("snmf:field", "p.win_STFT must hold p.framelength doubles");
    win.assign(mxGetDoubles(w), mxGetDoubles(w) + sp->framelength);
    sp->window = win.data();
}
// the solver fields of the settings struct as src/sparse_nmf.m:79-110 reads them; p.cost_check has no default (:260)
static void fill_solver(const mxArray* p, snmf_params* q) {
    std::memset(q, 0, sizeof *q);
    char cf[8] = "kl";
    if (const mxArray* c = mxGetField(p, 0, "cf")) {
        if (!mxIsChar(c)) mexErrMsgIdAndTxt("snmf:type", "p.cf must be a string");
        mxGetString(c, cf, sizeof cf);
    }
    q->beta = !std::strcmp(cf, "is") ? 0.0 : !std::strcmp(cf, "kl") ? 1.0 : !std::strcmp(cf, "ed") ? 2.0 : field_or(p, "beta", 1.0);
    const double mi = field_or(p, "max_iter", 100);
    if (!whole(mi, 0.0, kI32)) mexErrMsgIdAndTxt("snmf:field", "p.max_iter = %g is not an iteration limit", mi);
    q->max_iter = (int32_t)mi;
    q->conv_eps = field_or(p, "conv_eps", 0.0);
    q->cost_check = field(p, "cost_check") != 0.0;
    q->floor_v = 1;
    q->T = 1;  // (ignored by every batch entry)
    q->sparsity_kind = SNMF_SPARSITY_SCALAR;
    const mxArray* s = mxGetField(p, 0, "sparsity");
    if (s && mxGetNumberOfElements(s) == 1) {
        need_double(s, "p.sparsity");
        q->sparsity_scalar = mxGetScalar(s);
    }
}
static void scalar_sparsity(const mxArray* p) {
    const mxArray* s = mxGetField(p, 0, "sparsity");
    if (s && mxGetNumberOfElements(s) > 1) mexErrMsgIdAndTxt("snmf:dim", "this command needs a scalar p.sparsity");
}
// the settings of train_Exemplar = 1 (run_basis_train.m:84): nothing is solved and the solver fields are not read
static void exemplar_solver(snmf_params* q) {
    std::memset(q, 0, sizeof *q);
    q->beta = 1.0;
    q->max_iter = 1;
    q->floor_v = 1;
    q->T = 1;
}
// a mask of p: absent -> all ones; r entries, or one entry for all; logical or double
static void fill_mask(const mxArray* p, const char* name, size_t r, std::vector<uint8_t>& out, bool all_or_none) {
    out.assign(r, 1);  // src/sparse_nmf.m:142-148
    const mxArray* f = mxGetField(p, 0, name);
    if (!f || mxIsEmpty(f)) return;
    const bool lg = mxIsLogical(f);
    if (!lg) need_double(f, name);
    const size_t n = mxGetNumberOfElements(f);
    if (n != r && n != 1) mexErrMsgIdAndTxt("snmf:dim", "p.%s must have r = %d entries, or one for all", name, (int)r);
    size_t on = 0;
    for (size_t i = 0; i < r; ++i) {
        const size_t j = n == 1 ? 0 : i;
        out[i] = lg ? (mxGetLogicals(f)[j] ? 1 : 0) : (mxGetDoubles(f)[j] != 0.0);
        on += out[i];
    }
    if (all_or_none && on != 0 && on != r)
        mexErrMsgIdAndTxt("snmf:unsupported", "with a rank per problem p.%s must be all ones or all zeros", name);
}
// p.random_seed as the key of the device generator, as snmf_dnmf_mex.cpp reads it: with H0 = [] a seed <= 0 ("do not re-seed",
// src/sparse_nmf.m:112) is an error, since a stateless generator cannot mean it
static uint64_t device_seed(const mxArray* p, bool needed) {
    const double sd = field_or(p, "random_seed", 1);
    if (!needed) return 1;
    if (!(sd >= 1.0 && sd <= kI53)) mexErrMsgIdAndTxt("snmf:field", "H0 = [] needs p.random_seed >= 1: the device generator is keyed by it");
    return (uint64_t)(int64_t)sd;
}
// 1-based handle -> index into g_signals; a handle that was never made, or was destroyed, is snmf:handle
static size_t signals_index(const mxArray* a) {
    const double v = (mxIsStruct(a) || !mxIsDouble(a) || mxGetNumberOfElements(a) != 1) ? 0.0 : mxGetScalar(a);
    if (!whole(v, 1.0, (double)g_signals.size()) || !g_signals[(size_t)v - 1].s) mexErrMsgIdAndTxt("snmf:handle", "invalid signals handle");
    return (size_t)v - 1;
}

// ---- results -----------------------------------------------------------------------------------------------------------------
// plhs[i] = a where the caller takes it (MATLAB always takes plhs[0]), else the array is given back
static void put(int nlhs, mxArray* plhs[], int i, mxArray* a) {
    if (i < (nlhs > 1 ? nlhs : 1)) plhs[i] = a;
    else mxDestroyArray(a);
}
// the packed result of blocks rows[k] x cols[k]: side by side where the rows agree, a column otherwise
static mxArray* packed_out(const std::vector<int64_t>& rows, const std::vector<int64_t>& cols) {
    bool same = true;
    for (int64_t r : rows) same = same && r == rows[0];
    return same ? mxCreateDoubleMatrix((mwSize)rows[0], (mwSize)sum(cols), mxREAL) : mxCreateDoubleMatrix((mwSize)dot(rows, cols), 1, mxREAL);
}
// C counts, `per` per problem -> n x per doubles
static mxArray* counts_out(const std::vector<int32_t>& c, size_t n, size_t per) {
    mxArray* a = mxCreateDoubleMatrix((mwSize)n, (mwSize)per, mxREAL);
    for (size_t k = 0; k < n; ++k)
        for (size_t j = 0; j < per; ++j) mxGetDoubles(a)[j * n + k] = (double)c[k * per + j];
    return a;
}
static void failed(const char* id) { mexErrMsgIdAndTxt(id, "%s", snmf_last_error()); }

// ---- 'solve' -----------------------------------------------------------------------------------------------------------------
static void do_solve(int nlhs, mxArray* plhs[], const mxArray* prhs[]) {
    const mxArray* p = prhs[5];
    need_struct(p, "p");
    const bool f64 = fp64_mode(p);
    const std::vector<int64_t> T = counts(prhs[2], "T", 1.0, kI32);
    const size_t n = T.size();
    int64_t F = 0;
    const double* V = packed_rows(prhs[1], "V", &F, sum(T));
    const ranks r = ranks_arg(need_field(p, "r"), n, "p.r");
    std::vector<snmf_problem_settings> st;
    const bool has_st = settings_arg(prhs[6], n, st);
    const double* W0 = packed(prhs[3], "W0", F * sum(r.v));
    const double* H0 = packed(prhs[4], "H0", dot(r.v, T));
    fp64_only(f64, r.mixed || has_st);
    snmf_params q;
    fill_solver(p, &q);
    q.F = (int32_t)F;
    q.r = (int32_t)largest(r.v);
    q.floor_v = field_or(p, "floor_v", 1.0) != 0.0;
    if (has_st) q.max_iter = largest_limit(st);
    std::vector<uint8_t> wi, hi;
    fill_mask(p, "w_update_ind", (size_t)q.r, wi, r.mixed);
    fill_mask(p, "h_update_ind", (size_t)q.r, hi, r.mixed);
    q.w_update_ind = wi.data();
    q.h_update_ind = hi.data();
    const double* sparsity = nullptr;
    if (const mxArray* s = mxGetField(p, 0, "sparsity")) {
        if (mxGetNumberOfElements(s) > 1) {  // src/sparse_nmf.m:153-154: an r-vector, with one rank and one settings struct only
            need_double(s, "p.sparsity");
            if (r.mixed || has_st) mexErrMsgIdAndTxt("snmf:unsupported", "ranks or settings per problem take a scalar p.sparsity");
            if (!is_vector(s) || (int64_t)mxGetNumberOfElements(s) != r.v[0]) mexErrMsgIdAndTxt("snmf:dim", "p.sparsity must be a scalar or r x 1");
            q.sparsity_kind = SNMF_SPARSITY_RVEC;
            sparsity = mxGetDoubles(s);
        }
    }
    const std::vector<int32_t> T32 = narrow(T), r32 = narrow(r.v);
    const std::vector<int64_t> wsz = times(r.v, F), hsz = times(r.v, T);
    const std::vector<const double*> pV = table(V, times(T, F)), pW0 = table(W0, wsz), pH0 = table(H0, hsz);
    const int64_t nh = q.max_iter > 0 ? q.max_iter : 1;

    need_ctx();
    mxArray *W = mxCreateDoubleMatrix((mwSize)F, (mwSize)sum(r.v), mxREAL), *H = packed_out(r.v, T);
    mxArray *div = mxCreateDoubleMatrix((mwSize)nh, (mwSize)n, mxREAL), *cost = mxCreateDoubleMatrix((mwSize)nh, (mwSize)n, mxREAL);
    const std::vector<double*> pW = table(mxGetDoubles(W), wsz), pH = table(mxGetDoubles(H), hsz);
    const std::vector<double*> pdiv = table(mxGetDoubles(div), std::vector<int64_t>(n, nh)), pcost = table(mxGetDoubles(cost), std::vector<int64_t>(n, nh));
    std::vector<int32_t> n_iter(n, 0);
    if (!r.mixed && !has_st) {
        const std::vector<int64_t> ldV(n, F);
        const int rc = f64 ? snmf_sparse_nmf_batch_fp64(g_ctx, &q, (int32_t)n, T32.data(), pV.data(), ldV.data(), pW0.data(), pH0.data(), sparsity, pW.data(),
                                                        pH.data(), pdiv.data(), pcost.data(), n_iter.data())
                           : snmf_sparse_nmf_batch_f64(g_ctx, &q, (int32_t)n, T32.data(), pV.data(), ldV.data(), pW0.data(), pH0.data(), sparsity, pW.data(),
                                                       pH.data(), pdiv.data(), pcost.data(), n_iter.data());
        if (rc != SNMF_OK) failed("snmf:solve");
    } else {  // the resident fp64 handle: create, set every problem, run to the end, get, destroy
        snmf_batch* b = nullptr;
        int rc = has_st ? snmf_batch_create_settings_fp64(g_ctx, &q, (int32_t)n, T32.data(), r.mixed ? r32.data() : nullptr, st.data(), &b)
                        : snmf_batch_create_ranks_fp64(g_ctx, &q, (int32_t)n, T32.data(), r32.data(), &b);
        if (rc != SNMF_OK) failed("snmf:solve");
        for (size_t k = 0; k < n && rc == SNMF_OK; ++k) rc = snmf_batch_set_problem_f64(b, (int32_t)k, pV[k], F, pW0[k], pH0[k]);
        if (rc == SNMF_OK) rc = snmf_batch_run(b, 0);
        for (size_t k = 0; k < n && rc == SNMF_OK; ++k) rc = snmf_batch_get_f64(b, (int32_t)k, pW[k], pH[k], pdiv[k], pcost[k], &n_iter[k]);
        snmf_batch_destroy(b);  // (it leaves the message of a failed call in place)
        if (rc != SNMF_OK) failed("snmf:solve");
    }
    put(nlhs, plhs, 0, W);
    put(nlhs, plhs, 1, H);
    put(nlhs, plhs, 2, div);
    put(nlhs, plhs, 3, cost);
    put(nlhs, plhs, 4, counts_out(n_iter, n, 1));
}

// ---- 'dnmf' and 'dnmf_audio' -------------------------------------------------------------------------------------------------
struct dnmf_ranks {
    ranks x, d;
    std::vector<int64_t> r;  // R_x[k] + R_d[k]
    bool mixed;
};
static dnmf_ranks dnmf_ranks_of(const mxArray* p, size_t n) {
    dnmf_ranks o;
    o.x = ranks_arg(need_field(p, "R_x"), n, "p.R_x");
    o.d = ranks_arg(need_field(p, "R_d"), n, "p.R_d");
    o.r.resize(n);
    for (size_t k = 0; k < n; ++k) o.r[k] = o.x.v[k] + o.d.v[k];
    o.mixed = o.x.mixed || o.d.mixed;
    return o;
}

template <typename T>
static int dnmf_call(const snmf_params* q, const dnmf_ranks& R, size_t n, const std::vector<int32_t>& T32, const std::vector<const T*>& Y,
                     const std::vector<const T*>& X, const std::vector<const T*>& D, const std::vector<const T*>& B, const std::vector<const T*>& H0,
                     const std::vector<T*>& Bh, const std::vector<T*>& Ah, int32_t* n_iter, bool f64) {
    if constexpr (sizeof(T) == 4)
        return snmf_run_basis_dnmf_batch_f32(g_ctx, q, (int32_t)R.x.v[0], (int32_t)R.d.v[0], (int32_t)n, T32.data(), Y.data(), X.data(), D.data(), B.data(),
                                             H0.data(), Bh.data(), Ah.data(), n_iter);
    else
        return f64 ? snmf_run_basis_dnmf_batch_fp64(g_ctx, q, (int32_t)R.x.v[0], (int32_t)R.d.v[0], (int32_t)n, T32.data(), Y.data(), X.data(), D.data(),
                                                    B.data(), H0.data(), Bh.data(), Ah.data(), n_iter)
                   : snmf_run_basis_dnmf_batch_f64(g_ctx, q, (int32_t)R.x.v[0], (int32_t)R.d.v[0], (int32_t)n, T32.data(), Y.data(), X.data(), D.data(),
                                                   B.data(), H0.data(), Bh.data(), Ah.data(), n_iter);
}

static void do_dnmf(int nlhs, mxArray* plhs[], const mxArray* prhs[]) {
    const mxArray* p = prhs[7];
    need_struct(p, "p");
    const bool f64 = fp64_mode(p);
    const std::vector<int64_t> T = counts(prhs[4], "T", 1.0, kI32);
    const size_t n = T.size();
    int64_t F = 0, F2 = 0, F3 = 0;
    const double* Y = packed_rows(prhs[1], "Y", &F, sum(T));
    const double* X = packed_rows(prhs[2], "X", &F2, sum(T));
    const double* D = packed_rows(prhs[3], "D", &F3, sum(T));
    if (F2 != F || F3 != F) mexErrMsgIdAndTxt("snmf:dim", "Y, X and D must have one size");
    const dnmf_ranks R = dnmf_ranks_of(p, n);
    std::vector<snmf_problem_settings> st;
    const bool has_st = settings_arg(prhs[8], n, st);
    const double* B = packed(prhs[5], "B", F * sum(R.r));
    const double* H0 = packed(prhs[6], "H0", dot(R.r, T));
    fp64_only(f64, R.mixed || has_st);
    const bool single = field_or(p, "snmf_single", 0) != 0.0;
    if (single && f64) mexErrMsgIdAndTxt("snmf:unsupported", "p.snmf_single is the fp32 engine's: the fp64 engine takes and returns doubles");
    scalar_sparsity(p);
    snmf_params q;
    fill_solver(p, &q);
    q.F = (int32_t)F;
    q.r = (int32_t)largest(R.r);
    if (has_st) q.max_iter = largest_limit(st);
    const std::vector<int32_t> T32 = narrow(T), rx = narrow(R.x.v), rd = narrow(R.d.v);
    const std::vector<int64_t> vsz = times(T, F), bsz = times(R.r, F), hsz = times(R.r, T);

    need_ctx();
    mxArray *Bh = mxCreateDoubleMatrix((mwSize)F, (mwSize)sum(R.r), mxREAL), *Ah = packed_out(R.r, T);
    std::vector<int32_t> n_iter(3 * n, 0);
    int rc;
    if (single) {  // the float images of the arrays in, the float results widened
        const std::vector<float> y = as_elem<float>(Y, (size_t)sum(vsz)), x = as_elem<float>(X, (size_t)sum(vsz)), d = as_elem<float>(D, (size_t)sum(vsz));
        const std::vector<float> b = as_elem<float>(B, (size_t)sum(bsz)), h = as_elem<float>(H0, (size_t)sum(hsz));
        std::vector<float> bh((size_t)sum(bsz)), ah((size_t)sum(hsz));
        rc = dnmf_call<float>(&q, R, n, T32, table(y.data(), vsz), table(x.data(), vsz), table(d.data(), vsz), table(b.data(), bsz), table(h.data(), hsz),
                              table(bh.data(), bsz), table(ah.data(), hsz), n_iter.data(), false);
        for (size_t i = 0; i < bh.size(); ++i) mxGetDoubles(Bh)[i] = (double)bh[i];
        for (size_t i = 0; i < ah.size(); ++i) mxGetDoubles(Ah)[i] = (double)ah[i];
    } else if (R.mixed || has_st) {
        const std::vector<const double*> pY = table(Y, vsz), pX = table(X, vsz), pD = table(D, vsz), pB = table(B, bsz), pH = table(H0, hsz);
        const std::vector<double*> pBh = table(mxGetDoubles(Bh), bsz), pAh = table(mxGetDoubles(Ah), hsz);
        rc = snmf_run_basis_dnmf_batch_ranks_fp64(g_ctx, &q, rx.data(), rd.data(), has_st ? st.data() : nullptr, (int32_t)n, T32.data(), pY.data(), pX.data(),
                                                  pD.data(), pB.data(), pH.data(), pBh.data(), pAh.data(), n_iter.data());
    } else {
        rc = dnmf_call<double>(&q, R, n, T32, table(Y, vsz), table(X, vsz), table(D, vsz), table(B, bsz), table(H0, hsz), table(mxGetDoubles(Bh), bsz),
                               table(mxGetDoubles(Ah), hsz), n_iter.data(), f64);
    }
    if (rc != SNMF_OK) failed("snmf:dnmf");
    put(nlhs, plhs, 0, Bh);
    put(nlhs, plhs, 1, Ah);
    put(nlhs, plhs, 2, counts_out(n_iter, n, 3));
}

// 'dnmf_audio' behind its checks, in the engine's sample type
template <typename T>
static int dnmf_audio_call(const snmf_params* q, const snmf_stft_params* sp, const dnmf_ranks& R, const snmf_problem_settings* st, size_t n, const double* x,
                           const std::vector<int64_t>& n_x, const double* d, const std::vector<int64_t>& n_d, const mxArray* melmat, int M, int nb,
                           const double* const* B, const double* const* H0, const uint64_t* seed, double* const* Bh, double* const* Ah, int32_t* n_iter) {
    std::vector<T> xs, ds, mel;
    const T *px, *pd;
    if constexpr (sizeof(T) == 8) {  // the fp64 engine reads MATLAB's doubles where they lie
        px = x;
        pd = d;
    } else {
        xs = as_elem<T>(x, (size_t)sum(n_x));
        ds = as_elem<T>(d, (size_t)sum(n_d));
        px = xs.data();
        pd = ds.data();
    }
    if (M) mel = mel_rows<T>(melmat, nb);
    const std::vector<const T*> tx = table(px, n_x), td = table(pd, n_d);
    const T* pm = M ? mel.data() : nullptr;
    if constexpr (sizeof(T) == 8) {
        if (R.mixed || st) {
            const std::vector<int32_t> rx = narrow(R.x.v), rd = narrow(R.d.v);
            return snmf_run_basis_dnmf_audio_batch_ranks_fp64(g_ctx, q, sp, rx.data(), rd.data(), st, (int32_t)n, tx.data(), n_x.data(), td.data(), n_d.data(), pm,
                                                              M, B, H0, seed, Bh, Ah, n_iter);
        }
        return snmf_run_basis_dnmf_audio_batch_fp64(g_ctx, q, sp, (int32_t)R.x.v[0], (int32_t)R.d.v[0], (int32_t)n, tx.data(), n_x.data(), td.data(), n_d.data(), pm,
                                                    M, B, H0, seed, Bh, Ah, n_iter);
    } else {
        return snmf_run_basis_dnmf_audio_batch_f64(g_ctx, q, sp, (int32_t)R.x.v[0], (int32_t)R.d.v[0], (int32_t)n, tx.data(), n_x.data(), td.data(), n_d.data(), pm,
                                                   M, B, H0, seed, Bh, Ah, n_iter);
    }
}

static void do_dnmf_audio(int nlhs, mxArray* plhs[], const mxArray* prhs[]) {
    const mxArray *p = prhs[7], *melmat = prhs[8];
    need_struct(p, "p");
    const bool f64 = fp64_mode(p);
    const std::vector<int64_t> n_x = counts(prhs[2], "n_x", 1.0, kI53), n_d = counts(prhs[4], "n_d", 1.0, kI53);
    const size_t n = n_x.size();
    same_length(n_d.size(), n, "n_d", "n_x");
    const double* x = packed(prhs[1], "x", sum(n_x));
    const double* d = packed(prhs[3], "d", sum(n_d));
    std::vector<double> win;
    snmf_stft_params sp;
    fill_stft(p, win, &sp, field(p, "DCbin"));
    const int nb = sp.fftlength / 2 + 1, K = 2 * sp.splice + 1, M = mel_order(melmat, nb);
    const int64_t F = M ? (int64_t)K * M : (int64_t)K * nb;
    std::vector<int64_t> T(n);
    for (size_t k = 0; k < n; ++k) {
        T[k] = snmf_stft_num_frames(&sp, n_x[k] < n_d[k] ? n_x[k] : n_d[k]);  // run_basis_DNMF.m:5-9
        if (T[k] < 1) mexErrMsgIdAndTxt("snmf:dim", "the signals of problem %d are shorter than one analysis frame", (int)k + 1);
    }
    const dnmf_ranks R = dnmf_ranks_of(p, n);
    std::vector<snmf_problem_settings> st;
    const bool has_st = settings_arg(prhs[9], n, st);
    const double* B = packed(prhs[5], "B", F * sum(R.r));
    need_double(prhs[6], "H0");
    const double* H0 = mxIsEmpty(prhs[6]) ? nullptr : packed(prhs[6], "H0", dot(R.r, T));
    fp64_only(f64, R.mixed || has_st);
    scalar_sparsity(p);
    snmf_params q;
    fill_solver(p, &q);
    q.F = (int32_t)F;
    q.r = (int32_t)largest(R.r);
    if (has_st) q.max_iter = largest_limit(st);
    const uint64_t seed = device_seed(p, !H0);
    std::vector<uint64_t> seeds(n);
    for (size_t k = 0; k < n; ++k) seeds[k] = seed + k;
    const std::vector<int64_t> bsz = times(R.r, F), hsz = times(R.r, T);
    const std::vector<const double*> pB = table(B, bsz), pH = H0 ? table(H0, hsz) : std::vector<const double*>();

    need_ctx();
    mxArray *Bh = mxCreateDoubleMatrix((mwSize)F, (mwSize)sum(R.r), mxREAL), *Ah = packed_out(R.r, T);
    const std::vector<double*> pBh = table(mxGetDoubles(Bh), bsz), pAh = table(mxGetDoubles(Ah), hsz);
    std::vector<int32_t> n_iter(3 * n, 0);
    const snmf_problem_settings* ps = has_st ? st.data() : nullptr;
    const int rc = f64 ? dnmf_audio_call<double>(&q, &sp, R, ps, n, x, n_x, d, n_d, melmat, M, nb, pB.data(), H0 ? pH.data() : nullptr, H0 ? nullptr : seeds.data(),
                                                 pBh.data(), pAh.data(), n_iter.data())
                       : dnmf_audio_call<float>(&q, &sp, R, ps, n, x, n_x, d, n_d, melmat, M, nb, pB.data(), H0 ? pH.data() : nullptr, H0 ? nullptr : seeds.data(),
                                                pBh.data(), pAh.data(), n_iter.data());
    if (rc != SNMF_OK) failed("snmf:dnmf_audio");
    put(nlhs, plhs, 0, Bh);
    put(nlhs, plhs, 1, Ah);
    put(nlhs, plhs, 2, counts_out(n_iter, n, 3));
}

// ---- 'train' and 'train_signals' ---------------------------------------------------------------------------------------------
// what both check before the signals are known: p, the Mel table, DC_bin, the classes of the arrays
struct train_head {
    bool f64, exemplar, has_st;
    std::vector<double> win;
    snmf_stft_params sp;
    int nb, K, M;
    double dd;
    snmf_params q;
    std::vector<snmf_problem_settings> st;
};
static void train_head_of(train_head& h, const mxArray* idx, const mxArray* atoms, const mxArray* H0, const mxArray* p, const mxArray* melmat,
                          const mxArray* dcbin, const mxArray* settings, size_t n) {
    need_struct(p, "p");
    h.f64 = fp64_mode(p);
    need_double(idx, "sample_idx");
    need_double(atoms, "n_atoms");
    need_double(H0, "H0");
    fill_stft(p, h.win, &h.sp, scalar_arg(dcbin, "DC_bin"));
    h.nb = h.sp.fftlength / 2 + 1;
    h.K = 2 * h.sp.splice + 1;
    h.M = mel_order(melmat, h.nb);
    if (!h.M) mexErrMsgIdAndTxt("snmf:dim", "melmat is required (run_basis_train.m:70-78 always forms TF_Mel)");
    h.exemplar = field_or(p, "train_Exemplar", 0) != 0.0;
    h.has_st = settings_arg(settings, n, h.st) && !h.exemplar;  // (the exemplars are the dictionaries: nothing is solved)
    if (h.exemplar) {
        exemplar_solver(&h.q);
    } else {
        scalar_sparsity(p);
        fill_solver(p, &h.q);
    }
    h.q.F = (int32_t)(h.K * h.nb);
    if (h.has_st) h.q.max_iter = largest_limit(h.st);
    h.dd = field_or(p, "domain_DD", 0) != 0.0 ? field(p, "alpha_eta") : -1.0;  // run_basis_train.m:64-67
}

// everything behind the signals' lengths: s == nullptr runs on the resident signals `sig`
static void do_train(int nlhs, mxArray* plhs[], train_head& h, const char* id, const std::vector<int64_t>& n_samples, const double* s, const snmf_train_signals* sig,
                     const mxArray* idx, const mxArray* atoms, const mxArray* H0a, const mxArray* p, const mxArray* melmat) {
    const size_t n = n_samples.size();
    const ranks A = ranks_arg(atoms, n, "n_atoms");
    if (h.has_st) same_length(h.st.size(), n, "settings", "the batch");
    fp64_only(h.f64, A.mixed || h.has_st);
    std::vector<int64_t> T(n);
    for (size_t k = 0; k < n; ++k) {
        T[k] = snmf_stft_num_frames(&h.sp, n_samples[k]);
        if (T[k] < 1) mexErrMsgIdAndTxt("snmf:dim", "the training signal of problem %d is shorter than one analysis frame", (int)k + 1);
    }
    const double* ix = packed(idx, "sample_idx", sum(A.v));
    std::vector<int64_t> i0((size_t)sum(A.v));
    for (size_t k = 0, at = 0; k < n; ++k)
        for (int64_t j = 0; j < A.v[k]; ++j, ++at) {
            if (!whole(ix[at], 1.0, (double)T[k]))  // randsample is 1-based (:81)
                mexErrMsgIdAndTxt("snmf:dim", "sample_idx of problem %d: %g is not a frame index in 1..%lld", (int)k + 1, ix[at], (long long)T[k]);
            i0[at] = (int64_t)ix[at] - 1;
        }
    const double* H0 = (h.exemplar || mxIsEmpty(H0a)) ? nullptr : packed(H0a, "H0", dot(A.v, T));
    const bool draw = !h.exemplar && !H0;
    const std::vector<uint64_t> seeds(n, device_seed(p, draw));  // every problem from the same key: the reference re-seeds per call
    h.q.r = (int32_t)largest(A.v);
    const int64_t F = h.q.F, FM = (int64_t)h.K * h.M;
    const std::vector<int64_t> hsz = times(A.v, T), bsz = times(A.v, F), msz = times(A.v, FM);
    const std::vector<const int64_t*> pix = table((const int64_t*)i0.data(), A.v);
    const std::vector<const double*> pH0 = H0 ? table(H0, hsz) : std::vector<const double*>();
    const std::vector<int32_t> a32 = narrow(A.v);
    std::vector<float> sf, melf;
    std::vector<double> meld;
    if (h.f64) meld = mel_rows<double>(melmat, h.nb);
    else melf = mel_rows<float>(melmat, h.nb);
    if (s && !h.f64) sf = as_elem<float>(s, (size_t)sum(n_samples));

    need_ctx();
    mxArray *BD = mxCreateDoubleMatrix((mwSize)F, (mwSize)sum(A.v), mxREAL), *BM = mxCreateDoubleMatrix((mwSize)FM, (mwSize)sum(A.v), mxREAL);
    mxArray *AD = h.exemplar ? mxCreateDoubleScalar(0.0) : packed_out(A.v, T), *AM = h.exemplar ? mxCreateDoubleScalar(0.0) : packed_out(A.v, T);  // :93-96
    const std::vector<double*> pBD = table(mxGetDoubles(BD), bsz), pBM = table(mxGetDoubles(BM), msz);
    const std::vector<double*> pAD = h.exemplar ? std::vector<double*>() : table(mxGetDoubles(AD), hsz);
    const std::vector<double*> pAM = h.exemplar ? std::vector<double*>() : table(mxGetDoubles(AM), hsz);
    std::vector<int32_t> n_iter(2 * n, 0);
    const int32_t ex = h.exemplar ? 1 : 0, N = (int32_t)n;
    const double* const* ph = H0 ? pH0.data() : nullptr;
    const uint64_t* sd = draw ? seeds.data() : nullptr;
    double* const* pad = h.exemplar ? nullptr : pAD.data();
    double* const* pam = h.exemplar ? nullptr : pAM.data();
    const int32_t* pa = A.mixed ? a32.data() : nullptr;  // (NULL: p->r atoms for every problem, the settings entries only)
    int rc;
    if (!s) {
        if (h.has_st)
            rc = snmf_run_basis_train_signals_batch_settings_fp64(g_ctx, &h.q, &h.sp, h.dd, meld.data(), h.M, sig, pa, pix.data(), ex, ph, sd, pBD.data(), pad, pBM.data(),
                                                                  pam, n_iter.data(), h.st.data());
        else if (A.mixed)
            rc = snmf_run_basis_train_signals_batch_ranks_fp64(g_ctx, &h.q, &h.sp, h.dd, meld.data(), h.M, sig, a32.data(), pix.data(), ex, ph, sd, pBD.data(), pad,
                                                               pBM.data(), pam, n_iter.data());
        else if (h.f64)
            rc = snmf_run_basis_train_signals_batch_fp64(g_ctx, &h.q, &h.sp, h.dd, meld.data(), h.M, sig, pix.data(), ex, ph, sd, pBD.data(), pad, pBM.data(), pam,
                                                         n_iter.data());
        else
            rc = snmf_run_basis_train_signals_batch_f64(g_ctx, &h.q, &h.sp, h.dd, melf.data(), h.M, sig, pix.data(), ex, ph, sd, pBD.data(), pad, pBM.data(), pam,
                                                        n_iter.data());
    } else if (h.f64) {
        const std::vector<const double*> ps = table(s, n_samples);
        if (h.has_st)
            rc = snmf_run_basis_train_audio_batch_settings_fp64(g_ctx, &h.q, &h.sp, h.dd, meld.data(), h.M, N, ps.data(), n_samples.data(), pa, pix.data(), ex, ph, sd,
                                                                pBD.data(), pad, pBM.data(), pam, n_iter.data(), h.st.data());
        else if (A.mixed)
            rc = snmf_run_basis_train_audio_batch_ranks_fp64(g_ctx, &h.q, &h.sp, h.dd, meld.data(), h.M, N, ps.data(), n_samples.data(), a32.data(), pix.data(), ex, ph,
                                                             sd, pBD.data(), pad, pBM.data(), pam, n_iter.data());
        else
            rc = snmf_run_basis_train_audio_batch_fp64(g_ctx, &h.q, &h.sp, h.dd, meld.data(), h.M, N, ps.data(), n_samples.data(), pix.data(), ex, ph, sd, pBD.data(),
                                                       pad, pBM.data(), pam, n_iter.data());
    } else {
        const std::vector<const float*> ps = table((const float*)sf.data(), n_samples);
        rc = snmf_run_basis_train_audio_batch_f64(g_ctx, &h.q, &h.sp, h.dd, melf.data(), h.M, N, ps.data(), n_samples.data(), pix.data(), ex, ph, sd, pBD.data(), pad,
                                                  pBM.data(), pam, n_iter.data());
    }
    if (rc != SNMF_OK) failed(id);
    put(nlhs, plhs, 0, BD);
    put(nlhs, plhs, 1, BM);
    put(nlhs, plhs, 2, AD);
    put(nlhs, plhs, 3, AM);
    put(nlhs, plhs, 4, counts_out(n_iter, n, 2));
}

// ---- 'assemble' --------------------------------------------------------------------------------------------------------------
// an integer-valued setting such as 0.05 * fs samples: the integer, or snmf:field
static int64_t whole_setting(double x, const char* what) {
    const double r = std::floor(x + 0.5);
    if (!(std::fabs(x - r) <= 1e-9 * (std::fabs(x) > 1.0 ? std::fabs(x) : 1.0)) || !(std::fabs(r) <= kI53))
        mexErrMsgIdAndTxt("snmf:field", "%s = %g is not a whole number of samples", what, x);
    return (int64_t)r;
}

static void do_assemble(mxArray* plhs[], const mxArray* prhs[]) {
    const mxArray* p = prhs[6];
    need_struct(p, "p");
    const std::vector<int64_t> clip_len = counts(prhs[2], "clip_len", 1.0, kI53), n_clips = counts(prhs[3], "n_clips", 1.0, kI32);
    const std::vector<int64_t> mode = counts(prhs[4], "mode", 0.0, 2.0);
    const size_t n = n_clips.size(), nc = clip_len.size();
    same_length(mode.size(), n, "mode", "n_clips");
    if (sum(n_clips) != (int64_t)nc) mexErrMsgIdAndTxt("snmf:dim", "n_clips sums to %lld clips, clip_len has %d entries", (long long)sum(n_clips), (int)nc);
    const double* clips = packed(prhs[1], "clips", sum(clip_len));
    need_double(prhs[5], "range");
    const double* rg = mxIsEmpty(prhs[5]) ? nullptr : packed(prhs[5], "range", 2 * (int64_t)nc);
    const double fs = field(p, "fs");
    snmf_assemble_params ap;
    std::memset(&ap, 0, sizeof ap);
    const int64_t frame_len = whole_setting(0.02 * fs, "frame_len = 0.02 * p.fs"), bg_len = whole_setting(0.05 * fs, "bg_len = 0.05 * p.fs");
    if (frame_len < 2 || frame_len % 2 || frame_len > (int64_t)kI32 || bg_len < 1 || bg_len > (int64_t)kI32)
        mexErrMsgIdAndTxt("snmf:field", "p.fs = %g: frame_len = 0.02 * fs must be even and at least 2, bg_len = 0.05 * fs at least 1", fs);
    ap.frame_len = (int32_t)frame_len;
    ap.bg_len = (int32_t)bg_len;
    ap.thr = 0.7;  // run_basis_train.m:35
    ap.seq_len_max = whole_setting(field(p, "train_seq_len_max"), "p.train_seq_len_max");
    ap.file_len_max = whole_setting(field(p, "train_file_len_max"), "p.train_file_len_max");
    if (ap.seq_len_max < 0) mexErrMsgIdAndTxt("snmf:field", "p.train_seq_len_max is negative");
    std::vector<int64_t> range(2 * nc);
    for (size_t k = 0, c = 0; k < n; ++k)
        for (int64_t i = 0; i < n_clips[k]; ++i, ++c) {
            range[2 * c] = 1;  // (read for the clips of mode-2 classes only)
            range[2 * c + 1] = clip_len[c];
            if (mode[k] == 1 && clip_len[c] < bg_len)
                mexErrMsgIdAndTxt("snmf:dim", "clip %d of class %d has %lld samples, fewer than bg_len = %lld", (int)i + 1, (int)k + 1, (long long)clip_len[c], (long long)bg_len);
            if (mode[k] != 2) continue;
            if (!rg) mexErrMsgIdAndTxt("snmf:dim", "class %d has mode 2: range must be 2 x clips", (int)k + 1);
            if (!whole(rg[2 * c], 1.0, (double)clip_len[c]) || !whole(rg[2 * c + 1], rg[2 * c], (double)clip_len[c]))
                mexErrMsgIdAndTxt("snmf:dim", "the range [%g, %g] of clip %d of class %d is not inside [1, %lld]", rg[2 * c], rg[2 * c + 1], (int)i + 1, (int)k + 1, (long long)clip_len[c]);
            range[2 * c] = (int64_t)rg[2 * c];
            range[2 * c + 1] = (int64_t)rg[2 * c + 1];
        }
    const std::vector<const double*> pc = table(clips, clip_len);
    const std::vector<int32_t> nc32 = narrow(n_clips), m32 = narrow(mode);

    need_ctx();
    signals_handle h;
    h.s = nullptr;
    if (snmf_train_signals_assemble_f64(g_ctx, &ap, (int32_t)n, nc32.data(), pc.data(), clip_len.data(), m32.data(), range.data(), &h.s) != SNMF_OK) failed("snmf:assemble");
    h.len.assign(n, 0);
    if (snmf_train_signals_info(h.s, nullptr, h.len.data(), nullptr) != SNMF_OK) {
        snmf_train_signals_destroy(h.s);
        failed("snmf:assemble");
    }
    g_signals.push_back(h);
    plhs[0] = mxCreateDoubleScalar((double)g_signals.size());
}

struct command {
    const char* name;
    int max_out;
};
static const command kCommands[] = {{"solve", 5},        {"dnmf", 3},        {"dnmf_audio", 3},    {"train", 5},          {"assemble", 1},
                                    {"signals_info", 2}, {"signals_get", 1}, {"train_signals", 5}, {"signals_destroy", 0}};

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (snmf_abi_version() != SNMF_ABI_VERSION)  // a stale libsnmf_hip.so must not be driven through newer prototypes
        mexErrMsgIdAndTxt("snmf:abi", "libsnmf_hip.so has ABI version %d, this MEX file was built against %d", snmf_abi_version(), SNMF_ABI_VERSION);
    if (nrhs < 1 || !mxIsChar(prhs[0]))
        mexErrMsgIdAndTxt("snmf:usage", "first argument: 'solve' | 'dnmf' | 'dnmf_audio' | 'train' | 'assemble' | 'signals_info' | 'signals_get' | 'train_signals' | 'signals_destroy'");
    char cmd[24];
    mxGetString(prhs[0], cmd, sizeof cmd);
    const command* known = nullptr;
    for (const command& c : kCommands)
        if (!std::strcmp(cmd, c.name)) known = &c;
    if (!known) mexErrMsgIdAndTxt("snmf:usage", "unknown command '%s'", cmd);
    if (nlhs > known->max_out) mexErrMsgIdAndTxt("snmf:nargout", "'%s' has at most %d outputs", cmd, known->max_out);
    if (!strcmp(cmd, "solve")) {
        if (nrhs != 7) mexErrMsgIdAndTxt("snmf:usage", "solve: V, T, W0, H0, p, settings");
        do_solve(nlhs, plhs, prhs);
    } else if (!strcmp(cmd, "dnmf")) {
        if (nrhs != 9) mexErrMsgIdAndTxt("snmf:usage", "dnmf: Y, X, D, T, B, H0, p, settings");
        do_dnmf(nlhs, plhs, prhs);
    } else if (!strcmp(cmd, "dnmf_audio")) {
        if (nrhs != 10) mexErrMsgIdAndTxt("snmf:usage", "dnmf_audio: x, n_x, d, n_d, B, H0, p, melmat, settings");
        do_dnmf_audio(nlhs, plhs, prhs);
    } else if (!strcmp(cmd, "train")) {
        if (nrhs != 10) mexErrMsgIdAndTxt("snmf:usage", "train: s, n_samples, sample_idx, n_atoms, H0, p, melmat, DC_bin, settings");
        const std::vector<int64_t> n_samples = counts(prhs[2], "n_samples", 1.0, kI53);
        const double* s = packed(prhs[1], "s", sum(n_samples));
        train_head h;
        train_head_of(h, prhs[3], prhs[4], prhs[5], prhs[6], prhs[7], prhs[8], prhs[9], n_samples.size());
        do_train(nlhs, plhs, h, "snmf:train", n_samples, s, nullptr, prhs[3], prhs[4], prhs[5], prhs[6], prhs[7]);
    } else if (!strcmp(cmd, "assemble")) {
        if (nrhs != 7) mexErrMsgIdAndTxt("snmf:usage", "assemble: clips, clip_len, n_clips, mode, range, p");
        do_assemble(plhs, prhs);
    } else if (!strcmp(cmd, "signals_info")) {
        if (nrhs != 2) mexErrMsgIdAndTxt("snmf:usage", "signals_info: handle");
        const signals_handle& h = g_signals[signals_index(prhs[1])];
        const size_t n = h.len.size();
        std::vector<int64_t> len(n);
        std::vector<int32_t> used(n);
        if (snmf_train_signals_info(h.s, nullptr, len.data(), used.data()) != SNMF_OK) failed("snmf:signals_info");
        mxArray *L = mxCreateDoubleMatrix((mwSize)n, 1, mxREAL), *U = counts_out(used, n, 1);
        for (size_t k = 0; k < n; ++k) mxGetDoubles(L)[k] = (double)len[k];
        put(nlhs, plhs, 0, L);
        put(nlhs, plhs, 1, U);
    } else if (!strcmp(cmd, "signals_get")) {
        if (nrhs != 3) mexErrMsgIdAndTxt("snmf:usage", "signals_get: handle, k");
        const double k = scalar_arg(prhs[2], "k");
        const signals_handle& h = g_signals[signals_index(prhs[1])];
        if (!whole(k, 1.0, (double)h.len.size())) mexErrMsgIdAndTxt("snmf:dim", "class %g outside 1..%d", k, (int)h.len.size());
        const int32_t k0 = (int32_t)k - 1;
        plhs[0] = mxCreateDoubleMatrix((mwSize)h.len[(size_t)k0], 1, mxREAL);  // the library writes n_samples[k] doubles
        if (snmf_train_signals_get_f64(h.s, k0, mxGetDoubles(plhs[0])) != SNMF_OK) failed("snmf:signals_get");
    } else if (!strcmp(cmd, "train_signals")) {
        if (nrhs != 9) mexErrMsgIdAndTxt("snmf:usage", "train_signals: handle, sample_idx, n_atoms, H0, p, melmat, DC_bin, settings");
        train_head h;
        train_head_of(h, prhs[2], prhs[3], prhs[4], prhs[5], prhs[6], prhs[7], prhs[8], 0);
        const ranks A = ranks_arg(prhs[3], 0, "n_atoms");  // what the counts decide without the handle
        if (A.v.size() > 1) packed(prhs[2], "sample_idx", sum(A.v));
        const signals_handle& sh = g_signals[signals_index(prhs[1])];
        do_train(nlhs, plhs, h, "snmf:train_signals", sh.len, nullptr, sh.s, prhs[2], prhs[3], prhs[4], prhs[5], prhs[6]);
    } else if (!strcmp(cmd, "signals_destroy")) {
        if (nrhs != 2) mexErrMsgIdAndTxt("snmf:usage", "signals_destroy: handle");
        signals_handle& h = g_signals[signals_index(prhs[1])];
        snmf_train_signals_destroy(h.s);
        h.s = nullptr;
    }
}
