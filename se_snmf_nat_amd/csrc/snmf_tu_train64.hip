// snmf_tu_train64.hip -- the fp64 mode of the front-end and of the two training callers of sparse_nmf, device-resident:
//
//   snmf_stft_features_fp64 / snmf_mel_features_fp64 / snmf_tf_dd_fp64      kernels in snmf_frontend64.h
//   snmf_run_basis_dnmf_fp64, snmf_run_basis_dnmf_audio_fp64                run_basis_DNMF.m:1-55, run_basis_DNMF_Mel.m:1-95
//   snmf_run_basis_train_audio_fp64                                         run_basis_train.m:58-91 for one event class
//
// Audio goes in as doubles and double dictionaries come out.  Everything in between -- y = x + d, the features, the Mel
// projection, the exemplar columns, A_hat between the solves -- stays in HBM, tight and column-major, and every solve is
// solve64_core (snmf_tu_solve64.hip) on those buffers with ONE workspace sized for the largest of them.  The solves run
// the kernels of snmf_sparse_nmf_fp64 in its order on the same numbers, so the loop gives the bits of three separate calls.
// A translation unit of its own: nothing of the fp32 callers (snmf_tu_dnmf.hip) is touched.
#include "snmf_internal.h"
#include "snmf_frontend64.h"
#include "snmf_solve64_core.h"
#include "snmf_host64.h"

namespace {

// every device block of one call; freed on every way out (a failed allocation leaks nothing)
struct Dev64 {
    std::vector<void*> ptrs;
    hipStream_t st = nullptr;
    ~Dev64() {
        if (st) hipStreamSynchronize(st);
        for (void* q : ptrs) hipFree(q);
    }
    template <typename T>
    int get(T** p, size_t n) {
        *p = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        hipError_t e = hipMalloc((void**)p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(SNMF_ERR_NOMEM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
        ptrs.push_back(*p);
        return SNMF_OK;
    }
};

// a column-major rows x cols matrix between the host (leading dimension ld) and a tight device buffer
int up2d(hipStream_t st, double* dst, const double* src, int64_t ld, int64_t rows, int64_t cols) {
    if (ld == rows || cols == 1) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)rows * cols * 8, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpy2DAsync(dst, (size_t)rows * 8, src, (size_t)ld * 8, (size_t)rows * 8, (size_t)cols, hipMemcpyHostToDevice, st));
    return SNMF_OK;
}
int down2d(hipStream_t st, double* dst, int64_t ld, const double* src, int64_t rows, int64_t cols) {
    if (ld == rows || cols == 1) HIP_TRY(hipMemcpyAsync(dst, src, (size_t)rows * cols * 8, hipMemcpyDeviceToHost, st));
    else HIP_TRY(hipMemcpy2DAsync(dst, (size_t)ld * 8, src, (size_t)rows * 8, (size_t)rows * 8, (size_t)cols, hipMemcpyDeviceToHost, st));
    return SNMF_OK;
}

template <int LOGN>
int launch_stft64(snmf_ctx* ctx, const Stft64Args& a) {
    const size_t lds = (size_t)2 * (1 << LOGN) * sizeof(double2);
    SN_TRY(ensure_dyn_lds(ctx->device, (const void*)k_stft64<LOGN>, lds));
    hipLaunchKernelGGL(k_stft64<LOGN>, dim3((unsigned)a.n_frames), dim3(256), lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// features of the device samples d_s into dst (column t at dst + t * ld); window, twiddles and the unspliced magnitudes
// live in `mem` until the call ends
int stft64_to_device(snmf_ctx* ctx, Dev64& mem, const snmf_stft_params* sp, const double* d_s, double* dst, int64_t ld, int64_t n_frames) {
    hipStream_t st = ctx->stream;
    const int N = sp->fftlength, K = N / 2 + 1, S = sp->splice;
    std::vector<double2> htw(N / 2);
    for (int q = 0; q < N / 2; ++q) {
        const double ang = -2.0 * M_PI * (double)q / (double)N;
        htw[q] = make_double2(cos(ang), sin(ang));
    }
    double *d_win = nullptr, *d_tmp = nullptr;
    double2* d_tw = nullptr;
    SN_TRY(mem.get(&d_win, (size_t)sp->framelength));
    SN_TRY(mem.get(&d_tw, htw.size()));
    HIP_TRY(hipMemcpyAsync(d_win, sp->window, (size_t)sp->framelength * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tw, htw.data(), htw.size() * sizeof(double2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (htw is a local)
    Stft64Args a{};
    a.s = d_s;
    a.sz = sp->framelength, a.shift = sp->frameshift, a.dcbin = sp->dcbin;
    a.preemph = sp->preemph;
    a.win = d_win, a.tw = d_tw;
    a.powv = sp->pow;
    a.n_frames = (int)n_frames;
    if (S == 0) {
        a.floorv = sp->nonzerofloor, a.out = dst, a.ld = ld;
    } else {
        SN_TRY(mem.get(&d_tmp, (size_t)K * n_frames));
        a.floorv = 0.0, a.out = d_tmp, a.ld = K;
    }
    switch (N) {
        case 64: SN_TRY(launch_stft64<6>(ctx, a)); break;
        case 128: SN_TRY(launch_stft64<7>(ctx, a)); break;
        case 256: SN_TRY(launch_stft64<8>(ctx, a)); break;
        case 512: SN_TRY(launch_stft64<9>(ctx, a)); break;
        case 1024: SN_TRY(launch_stft64<10>(ctx, a)); break;
        case 2048: SN_TRY(launch_stft64<11>(ctx, a)); break;
        default: SN_TRY(launch_stft64<12>(ctx, a)); break;
    }
    if (S > 0) {
        hipLaunchKernelGGL(k_splice64, dim3(grid64((long long)(2 * S + 1) * K * n_frames)), dim3(256), 0, st, (const double*)d_tmp, (int64_t)K, K,
                           (int)n_frames, S, sp->nonzerofloor, dst, ld);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

// the ABI's Mel table (M x n row-major, host) as k_mel64 reads it: n x M on the device
int upload_mel64(Dev64& mem, hipStream_t st, const double* mel, int M, int n, double** d_melT) {
    std::vector<double> t((size_t)M * n);
    for (int m = 0; m < M; ++m)
        for (int f = 0; f < n; ++f) t[(size_t)f * M + m] = mel[(size_t)m * n + f];
    SN_TRY(mem.get(d_melT, t.size()));
    HIP_TRY(hipMemcpyAsync(*d_melT, t.data(), t.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (t is a local)
    return SNMF_OK;
}

int mel64_on_device(hipStream_t st, const double* d_mel, int M, int n, int K, const double* d_v, int64_t ldv, int T, double* d_o, int64_t ldo) {
    hipLaunchKernelGGL(k_mel64, dim3(grid64((long long)K * M * T)), dim3(256), 0, st, d_mel, M, n, K, d_v, ldv, T, d_o, ldo);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

int tfdd64_on_device(hipStream_t st, double a, int F, int T, const double* d_x, int64_t ldx, double* d_o, int64_t ldo, double* d_carry) {
    const int nch = (T + kDd64Chunk - 1) / kDd64Chunk;
    const dim3 g(nch, (F + 255) / 256);
    hipLaunchKernelGGL(k_tfdd64_carry, g, dim3(256), 0, st, d_x, ldx, F, T, a, d_carry);
    hipLaunchKernelGGL(k_tfdd64_state, dim3((F + 255) / 256), dim3(256), 0, st, d_x, F, T, a, d_carry);
    hipLaunchKernelGGL(k_tfdd64_apply, g, dim3(256), 0, st, d_x, ldx, F, T, a, (const double*)d_carry, d_o, ldo);
    HIP_TRY(hipGetLastError());
    return SNMF_OK;
}

// an initial H the caller supplies (host, tight r x T) or the Philox draw of snmf_plan_set_h_random as doubles
int init_h64(hipStream_t st, double* dH, const double* H0, int r, int64_t T, uint64_t seed) {
    const uint64_t n = (uint64_t)r * (uint64_t)T;
    if (H0) HIP_TRY(hipMemcpyAsync(dH, H0, (size_t)n * 8, hipMemcpyHostToDevice, st));
    else {
        hipLaunchKernelGGL(k_rand64, dim3(grid64((long long)((n + 3) / 4))), dim3(256), 0, st, dH, n, seed);
        HIP_TRY(hipGetLastError());
    }
    return SNMF_OK;
}

// what every DNMF entry refuses before it touches the device (as loop3_create of snmf_tu_dnmf.hip does)
int dnmf64_check(const snmf_params* p, int R_x, int R_d) {
    if (R_x < 1 || R_d < 1 || p->r != R_x + R_d) return fail(SNMF_ERR_DIM, "params->r = %d must equal R_x + R_d = %d + %d", p->r, R_x, R_d);
    if (p->sparsity_kind != SNMF_SPARSITY_SCALAR)
        // an r x 1 or r x n p.sparsity has R_x + R_d rows: solves 2 / 3 (R_x, R_d rows) are a MATLAB dimension error (src/sparse_nmf.m:192)
        return fail(SNMF_ERR_DIM, "run_basis_DNMF needs a scalar p.sparsity (its W-only solves have R_x / R_d rows)");
    return SNMF_OK;
}

// run_basis_DNMF.m:36-55 on resident features: dY, dX, dD F x T (each floored in place by its solve), dB F x r (read
// only), dA r x T = the initial H of solve 1, A_hat afterwards.  B_hat and (if asked for) A_hat go to the host.
int dnmf64_loop(snmf_ctx* ctx, Dev64& mem, const snmf_params* p, int R_x, int R_d, double* dY, double* dX, double* dD, const double* dB,
                double* dA, double* B_hat, int64_t ldBh, double* A_hat, int64_t ldA, int32_t* n_iter3) {
    hipStream_t st = ctx->stream;
    const int F = p->F, T = p->T, r = p->r;
    std::vector<uint8_t> on(r, 1), off(r, 0);
    snmf_params q1 = *p, q2 = *p, q3 = *p;
    q1.w_update_ind = off.data(), q1.h_update_ind = on.data();   // :37-38
    q2.r = R_x, q2.w_update_ind = on.data(), q2.h_update_ind = off.data();  // :43-44
    q3.r = R_d, q3.w_update_ind = on.data(), q3.h_update_ind = off.data();  // :49-50
    size_t b1 = 0, b2 = 0, b3 = 0;
    SN_TRY(solve64_ws_bytes(&q1, &b1));
    SN_TRY(solve64_ws_bytes(&q2, &b2));
    SN_TRY(solve64_ws_bytes(&q3, &b3));
    const size_t ws_bytes = std::max(b1, std::max(b2, b3));
    char* ws = nullptr;
    double *dW = nullptr, *dHs = nullptr;
    SN_TRY(mem.get(&ws, ws_bytes));
    SN_TRY(mem.get(&dW, (size_t)F * r));
    SN_TRY(mem.get(&dHs, (size_t)std::max(R_x, R_d) * T));
    int32_t n1 = 0, n2 = 0, n3 = 0;
    HIP_TRY(hipMemcpyAsync(dW, dB, (size_t)F * r * 8, hipMemcpyDeviceToDevice, st));  // p.init_w = B   (:39)
    SN_TRY(solve64_core(ctx, &q1, dY, dW, dA, nullptr, ws, ws_bytes, nullptr, nullptr, &n1));  // [~, A_hat] = sparse_nmf(Y, p)   (:40)
    if (A_hat) SN_TRY(down2d(st, A_hat, ldA, dA, r, T));
    // init_w = B(:,1:R_x) / B(:,R_x+1:end) (:45, :51): column blocks of one tight copy of B, which then IS B_hat (:55)
    HIP_TRY(hipMemcpyAsync(dW, dB, (size_t)F * r * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_rows64, dim3(grid64((long long)R_x * T)), dim3(256), 0, st, (const double*)dA, (int64_t)r, R_x, (int64_t)T, dHs, (int64_t)R_x);  // :46
    HIP_TRY(hipGetLastError());
    SN_TRY(solve64_core(ctx, &q2, dX, dW, dHs, nullptr, ws, ws_bytes, nullptr, nullptr, &n2));  // [B_hat_x, ~] = sparse_nmf(X, p)  (:47)
    hipLaunchKernelGGL(k_rows64, dim3(grid64((long long)R_d * T)), dim3(256), 0, st, (const double*)dA + R_x, (int64_t)r, R_d, (int64_t)T, dHs, (int64_t)R_d);  // :52
    HIP_TRY(hipGetLastError());
    SN_TRY(solve64_core(ctx, &q3, dD, dW + (size_t)F * R_x, dHs, nullptr, ws, ws_bytes, nullptr, nullptr, &n3));  // [B_hat_d, ~] = sparse_nmf(D, p)  (:53)
    SN_TRY(down2d(st, B_hat, ldBh, dW, F, r));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_iter3) n_iter3[0] = n1, n_iter3[1] = n2, n_iter3[2] = n3;
    return SNMF_OK;
}

}  // namespace

// ---- the front-end entries ----------------------------------------------------------------------------------------------
extern "C" int snmf_stft_features_fp64(snmf_ctx* ctx, const snmf_stft_params* sp, const double* samples, int64_t n_samples,
                                       int samples_on_device, double* V_out, int64_t ld, int out_on_device, int32_t* n_frames_out) {
    if (!ctx || !samples || !V_out) return fail(SNMF_ERR_INVALID, "NULL argument");
    SN_TRY(validate_stft(sp));
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t nfr = snmf_stft_num_frames(sp, n_samples);
    const int64_t F = (int64_t)(2 * sp->splice + 1) * (sp->fftlength / 2 + 1);
    if (n_frames_out) *n_frames_out = (int32_t)nfr;
    if (nfr <= 0) return SNMF_OK;
    if (ld < F) return fail(SNMF_ERR_INVALID, "ld < feature rows %lld", (long long)F);
    hipStream_t st = ctx->stream;
    Dev64 mem;
    mem.st = st;
    const double* d_s = samples;
    if (!samples_on_device) {
        double* q = nullptr;
        SN_TRY(mem.get(&q, (size_t)n_samples));
        HIP_TRY(hipMemcpyAsync(q, samples, (size_t)n_samples * 8, hipMemcpyHostToDevice, st));
        d_s = q;
    }
    if (out_on_device) {
        SN_TRY(stft64_to_device(ctx, mem, sp, d_s, V_out, ld, nfr));
        HIP_TRY(hipStreamSynchronize(st));
        return SNMF_OK;
    }
    double* d_out = nullptr;
    SN_TRY(mem.get(&d_out, (size_t)F * nfr));
    SN_TRY(stft64_to_device(ctx, mem, sp, d_s, d_out, F, nfr));
    SN_TRY(down2d(st, V_out, ld, d_out, F, nfr));
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

extern "C" int snmf_mel_features_fp64(snmf_ctx* ctx, const double* mel, int32_t M, int32_t n, int32_t K, const double* V, int64_t ldv,
                                      int32_t T, double* out, int64_t ldo, int on_device) {
    if (!ctx || !mel || !V || !out) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (M < 1 || n < 1 || K < 1 || T < 1 || ldv < (int64_t)K * n || ldo < (int64_t)K * M) return fail(SNMF_ERR_INVALID, "bad Mel projection sizes");
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Dev64 mem;
    mem.st = st;
    double* d_mel = nullptr;
    SN_TRY(upload_mel64(mem, st, mel, M, n, &d_mel));
    if (on_device) {
        SN_TRY(mel64_on_device(st, d_mel, M, n, K, V, ldv, T, out, ldo));
    } else {  // tight on the device, the caller's leading dimensions on the host
        double *d_v = nullptr, *d_o = nullptr;
        const int64_t rv = (int64_t)K * n, ro = (int64_t)K * M;
        SN_TRY(mem.get(&d_v, (size_t)rv * T));
        SN_TRY(mem.get(&d_o, (size_t)ro * T));
        SN_TRY(up2d(st, d_v, V, ldv, rv, T));
        SN_TRY(mel64_on_device(st, d_mel, M, n, K, d_v, rv, T, d_o, ro));
        SN_TRY(down2d(st, out, ldo, d_o, ro, T));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

// TF_DD (src/TF_DD.m, run_basis_train.m:64-67) in double.  X / out: F x T column-major, host or device (both the same
// side); out may alias X.
extern "C" int snmf_tf_dd_fp64(snmf_ctx* ctx, double alpha_eta, int32_t F, int32_t T, const double* X, int64_t ldx, double* out, int64_t ldo,
                               int on_device) {
    if (!ctx || !X || !out) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (F < 1 || T < 1 || ldx < F || ldo < F) return fail(SNMF_ERR_INVALID, "bad TF_DD sizes");
    if (!(alpha_eta == alpha_eta)) return fail(SNMF_ERR_INVALID, "alpha_eta is NaN");
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Dev64 mem;
    mem.st = st;
    double* d_c = nullptr;
    SN_TRY(mem.get(&d_c, (size_t)((T + kDd64Chunk - 1) / kDd64Chunk) * F));
    if (on_device) {
        SN_TRY(tfdd64_on_device(st, alpha_eta, F, T, X, ldx, out, ldo, d_c));
    } else {
        double* d_x = nullptr;
        SN_TRY(mem.get(&d_x, (size_t)F * T));
        SN_TRY(up2d(st, d_x, X, ldx, F, T));
        SN_TRY(tfdd64_on_device(st, alpha_eta, F, T, d_x, F, d_x, F, d_c));
        SN_TRY(down2d(st, out, ldo, d_x, F, T));  // (rows F .. ldo-1 of the caller's out are padding: left untouched)
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SNMF_OK;
}

// ---- run_basis_DNMF on formed features ----------------------------------------------------------------------------------
extern "C" int snmf_run_basis_dnmf_fp64(snmf_ctx* ctx, const snmf_params* p, int32_t R_x, int32_t R_d, const double* Y, int64_t ldY,
                                        const double* X, int64_t ldX, const double* D, int64_t ldD, const double* B, int64_t ldB,
                                        const double* H0, uint64_t seed, double* B_hat, int64_t ldBh, double* A_hat, int64_t ldA,
                                        int32_t* n_iter_out) {
    if (!ctx || !p) return fail(SNMF_ERR_INVALID, "NULL argument");
    if (!Y || !X || !D || !B || !B_hat) return fail(SNMF_ERR_INVALID, "Y, X, D, B and B_hat must be non-NULL");
    SN_TRY(validate_params(p));
    SN_TRY(dnmf64_check(p, R_x, R_d));
    const int F = p->F, T = p->T, r = p->r;
    if (ldY < F || ldX < F || ldD < F) return fail(SNMF_ERR_INVALID, "leading dimension of Y, X or D < F");
    if (ldB < F) return fail(SNMF_ERR_INVALID, "leading dimension of B < F");
    if (ldBh < F) return fail(SNMF_ERR_INVALID, "leading dimension of B_hat < F");
    if (A_hat && ldA < r) return fail(SNMF_ERR_INVALID, "leading dimension of A_hat < R_x + R_d");
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Dev64 mem;
    mem.st = st;
    double *dY, *dX, *dD, *dB, *dA;
    SN_TRY(mem.get(&dY, (size_t)F * T));
    SN_TRY(mem.get(&dX, (size_t)F * T));
    SN_TRY(mem.get(&dD, (size_t)F * T));
    SN_TRY(mem.get(&dB, (size_t)F * r));
    SN_TRY(mem.get(&dA, (size_t)r * T));
    SN_TRY(up2d(st, dY, Y, ldY, F, T));  // each of the three feature sets crosses once
    SN_TRY(up2d(st, dX, X, ldX, F, T));
    SN_TRY(up2d(st, dD, D, ldD, F, T));
    SN_TRY(up2d(st, dB, B, ldB, F, r));
    SN_TRY(init_h64(st, dA, H0, r, T, seed));
    return dnmf64_loop(ctx, mem, p, R_x, R_d, dY, dX, dD, dB, dA, B_hat, ldBh, A_hat, ldA, n_iter_out);
}

// B_hat = run_basis_DNMF(x, d, B, p) from the two WAVEFORMS in double: the truncation to equal length (:5-9), y = x + d (:10),
// the three spectrogram feature sets (:13-34) and the loop (:36-55) on the device; with `mel` the Mel twin run_basis_DNMF_Mel.m.
extern "C" int snmf_run_basis_dnmf_audio_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, int32_t R_x, int32_t R_d,
                                              const double* x, int64_t n_x, const double* d, int64_t n_d, const double* mel, int32_t mel_M,
                                              const double* B, int64_t ldB, const double* H0, uint64_t seed, double* B_hat, int64_t ldBh,
                                              double* A_hat, int64_t ldA, int32_t* n_iter_out) {
    if (!ctx || !p || !x || !d || !B || !B_hat) return fail(SNMF_ERR_INVALID, "NULL argument");
    SN_TRY(validate_stft(sp));
    SN_TRY(validate_params(p));
    (void)hipGetLastError();
    const int64_t n = std::min(n_x, n_d);  // :5-9
    const int64_t T = snmf_stft_num_frames(sp, n);
    const int nb = sp->fftlength / 2 + 1, K = 2 * sp->splice + 1;
    const int64_t Fd = (int64_t)K * nb, F = mel ? (int64_t)K * mel_M : Fd;
    if (T < 1) return fail(SNMF_ERR_INVALID, "the signals are shorter than one analysis frame");
    if (F != p->F || T != p->T)
        return fail(SNMF_ERR_DIM, "the signals give %lld x %lld features, params say %d x %d", (long long)F, (long long)T, p->F, p->T);
    if (mel && mel_M < 1) return fail(SNMF_ERR_INVALID, "mel_M must be positive");
    SN_TRY(dnmf64_check(p, R_x, R_d));
    const int r = p->r;
    if (ldB < F) return fail(SNMF_ERR_INVALID, "leading dimension of B < F");
    if (ldBh < F) return fail(SNMF_ERR_INVALID, "leading dimension of B_hat < F");
    if (A_hat && ldA < r) return fail(SNMF_ERR_INVALID, "leading dimension of A_hat < R_x + R_d");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Dev64 mem;
    mem.st = st;
    double *dx, *dd, *dy, *dV[3], *dB, *dA, *d_mel = nullptr, *scr = nullptr;
    SN_TRY(mem.get(&dx, (size_t)n));
    SN_TRY(mem.get(&dd, (size_t)n));
    SN_TRY(mem.get(&dy, (size_t)n));
    for (int i = 0; i < 3; ++i) SN_TRY(mem.get(&dV[i], (size_t)F * T));
    SN_TRY(mem.get(&dB, (size_t)F * r));
    SN_TRY(mem.get(&dA, (size_t)r * T));
    if (mel) {
        SN_TRY(upload_mel64(mem, st, mel, mel_M, nb, &d_mel));
        SN_TRY(mem.get(&scr, (size_t)Fd * T));
    }
    HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dd, d, (size_t)n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_add64, dim3(grid64(n)), dim3(256), 0, st, (const double*)dx, (const double*)dd, dy, n);
    HIP_TRY(hipGetLastError());
    const double* sig[3] = {dy, dx, dd};
    for (int i = 0; i < 3; ++i) {
        if (!mel) SN_TRY(stft64_to_device(ctx, mem, sp, sig[i], dV[i], F, T));
        else {
            SN_TRY(stft64_to_device(ctx, mem, sp, sig[i], scr, Fd, T));
            SN_TRY(mel64_on_device(st, d_mel, mel_M, nb, K, scr, Fd, (int)T, dV[i], F));
        }
    }
    SN_TRY(up2d(st, dB, B, ldB, F, r));
    SN_TRY(init_h64(st, dA, H0, r, T, seed));
    return dnmf64_loop(ctx, mem, p, R_x, R_d, dV[0], dV[1], dV[2], dB, dA, B_hat, ldBh, A_hat, ldA, n_iter_out);
}

// [B_DFT_init, A_DFT_init] and [B_Mel_init, A_Mel_init] of run_basis_train.m:58-91 for one event class from its training
// signal, in double: TF_mag (:60-63) with the optional TF_DD (:64-67), TF_Mel (:70-78), the exemplar columns (:82-83) and
// the two full-update solves (:84-91).  mel == NULL (with B_Mel == NULL): the DFT solve only.
extern "C" int snmf_run_basis_train_audio_fp64(snmf_ctx* ctx, const snmf_params* p, const snmf_stft_params* sp, double alpha_eta_dd,
                                               const double* mel, int32_t mel_M, const double* s_full, int64_t n_samples,
                                               const int64_t* sample_idx, int32_t train_exemplar, const double* H0, uint64_t seed,
                                               double* B_DFT, double* A_DFT, double* B_Mel, double* A_Mel, int32_t* n_iter_out) {
    if (!ctx || !p || !s_full || !sample_idx || !B_DFT) return fail(SNMF_ERR_INVALID, "NULL argument");
    SN_TRY(validate_stft(sp));
    SN_TRY(validate_params(p));
    (void)hipGetLastError();
    const int nb = sp->fftlength / 2 + 1, K = 2 * sp->splice + 1;
    const int64_t T = snmf_stft_num_frames(sp, n_samples), F = (int64_t)K * nb, Fm = (int64_t)K * mel_M;
    const int r = p->r;
    if (T < 1) return fail(SNMF_ERR_INVALID, "the signal is shorter than one analysis frame");
    if (F != p->F || T != p->T)
        return fail(SNMF_ERR_DIM, "the signal gives %lld x %lld features, params say %d x %d", (long long)F, (long long)T, p->F, p->T);
    if ((mel != nullptr) != (B_Mel != nullptr)) return fail(SNMF_ERR_INVALID, "mel and B_Mel must be given together");
    if (mel && mel_M < 1) return fail(SNMF_ERR_INVALID, "mel_M must be positive");
    if (p->sparsity_kind != SNMF_SPARSITY_SCALAR)
        return fail(SNMF_ERR_UNSUPPORTED, "a sparsity vector or matrix is not supported by the training entry (it takes the scalar of p)");
    for (int j = 0; j < r; ++j)
        if (sample_idx[j] < 0 || sample_idx[j] >= T) return fail(SNMF_ERR_INVALID, "sample_idx[%d] = %lld outside [0, %lld)", j, (long long)sample_idx[j], (long long)T);
    snmf_params qa = *p, qb = *p;
    qa.w_update_ind = qa.h_update_ind = qb.w_update_ind = qb.h_update_ind = nullptr;  // :85-86 all true
    qb.F = (int32_t)Fm;
    size_t ws_bytes = 0;
    if (!train_exemplar) {
        size_t ba = 0, bb = 0;
        SN_TRY(solve64_ws_bytes(&qa, &ba));
        if (mel) SN_TRY(solve64_ws_bytes(&qb, &bb));
        ws_bytes = std::max(ba, bb);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Dev64 mem;
    mem.st = st;
    double *ds, *dV, *ex, *dVm = nullptr, *exm = nullptr, *d_mel = nullptr, *dH = nullptr, *d_c = nullptr;
    char* ws = nullptr;
    int64_t* didx;
    SN_TRY(mem.get(&ds, (size_t)n_samples));
    SN_TRY(mem.get(&didx, (size_t)r));
    SN_TRY(mem.get(&dV, (size_t)F * T));
    SN_TRY(mem.get(&ex, (size_t)F * r));
    if (mel) {
        SN_TRY(upload_mel64(mem, st, mel, mel_M, nb, &d_mel));
        SN_TRY(mem.get(&dVm, (size_t)Fm * T));
        SN_TRY(mem.get(&exm, (size_t)Fm * r));
    }
    if (!train_exemplar) {
        SN_TRY(mem.get(&dH, (size_t)r * T));
        SN_TRY(mem.get(&ws, ws_bytes));
    }
    HIP_TRY(hipMemcpyAsync(ds, s_full, (size_t)n_samples * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(didx, sample_idx, (size_t)r * 8, hipMemcpyHostToDevice, st));
    SN_TRY(stft64_to_device(ctx, mem, sp, ds, dV, F, T));  // TF_mag   (:60-63)
    if (alpha_eta_dd >= 0.0) {  // :64-67
        SN_TRY(mem.get(&d_c, (size_t)((T + kDd64Chunk - 1) / kDd64Chunk) * F));
        SN_TRY(tfdd64_on_device(st, alpha_eta_dd, (int)F, (int)T, dV, F, dV, F, d_c));
    }
    hipLaunchKernelGGL(k_gather64, dim3(grid64((long long)F * r)), dim3(256), 0, st, (const double*)dV, F, (int)F, (const int64_t*)didx, r, ex);  // :82
    HIP_TRY(hipGetLastError());
    if (mel) {  // :70-78, from the unfloored TF_mag like the reference (the solver's own floor comes last)
        SN_TRY(mel64_on_device(st, d_mel, mel_M, nb, K, dV, F, (int)T, dVm, Fm));
        hipLaunchKernelGGL(k_gather64, dim3(grid64((long long)Fm * r)), dim3(256), 0, st, (const double*)dVm, Fm, (int)Fm, (const int64_t*)didx, r, exm);  // :83
        HIP_TRY(hipGetLastError());
    }
    int32_t nit[2] = {0, 0};
    // the exemplars are init_w (:87, :90) and, updated in place, the dictionary; in exemplar mode they ARE the dictionary (:84, :95-96)
    auto solve = [&](const snmf_params* q, double* V, double* w, int64_t rows, double* Bo, double* Ao, int32_t* ni) -> int {
        if (!train_exemplar) {
            SN_TRY(init_h64(st, dH, H0, r, T, seed));  // the reference re-seeds per call (:112-114): both solves start from the SAME h
            SN_TRY(solve64_core(ctx, q, V, w, dH, nullptr, ws, ws_bytes, nullptr, nullptr, ni));
            if (Ao) HIP_TRY(hipMemcpyAsync(Ao, dH, (size_t)r * T * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(Bo, w, (size_t)rows * r * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SNMF_OK;
    };
    SN_TRY(solve(&qa, dV, ex, F, B_DFT, A_DFT, &nit[0]));               // :88
    if (mel) SN_TRY(solve(&qb, dVm, exm, Fm, B_Mel, A_Mel, &nit[1]));   // :91
    if (n_iter_out) n_iter_out[0] = nit[0], n_iter_out[1] = nit[1];
    return SNMF_OK;
}
