// snmf_frontend64.h -- the spectrogram front-end in double: the counterparts of snmf_frontend.h for the fp64 mode of the
// training callers (snmf_tu_train64.hip).
//   src/stft_fft.m:15-37        framing, pre-emphasis, window, zero-padded FFT, |.|, DC-bin value       k_stft64
//   run_basis_train.m:60-63     splice, .^pow + nonzerofloor                                            k_splice64
//   run_basis_train.m:70-78     Mel projection                                                          k_mel64
//   src/TF_DD.m                 recursive average along the frames                                      k_tfdd64_*
//   run_basis_train.m:81-83     exemplar columns V(:, sample_idx)                                       k_gather64
//   run_basis_DNMF.m:10         y = x + d                                                               k_add64
// Every matrix is tight column-major with a leading dimension of the caller's (the fp64 solve takes ld = rows): nothing is
// padded, every kernel checks its bounds.  The FFT is fft_lds<LOGN, double> (snmf_online_common.h) on host-computed fp64
// twiddles; its two buffers are dynamic LDS (2 N double2 = 128 KB at N = 4096 cannot be static).  Every sum has a fixed
// order (the butterflies, the sequential Mel dot product, the chunked recursion), so two runs give the same bits.
#pragma once
#include "snmf_online_common.h"
#include "snmf_philox.h"

namespace snmf {

struct Stft64Args {
    const double* s;     // samples (device)
    int sz, shift, dcbin;
    double preemph;
    const double* win;   // [sz]
    const double2* tw;   // [N/2] exp(-2*pi*i*q/N)
    double powv, floorv; // floorv is added here only when there is no splicing pass
    double* out;         // column t at out + t*ld
    int64_t ld;
    int n_frames;
};

template <int LOGN>
__global__ __launch_bounds__(256) void k_stft64(Stft64Args a) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __attribute__((aligned(16))) double2 fbuf64[];
    const int t = blockIdx.x;
    if (t >= a.n_frames) return;
    double2* bufA = fbuf64;
    const double* s = a.s + (int64_t)t * a.shift;  // 0-based first sample of frame t (size_crnt - 1)
    for (int n = threadIdx.x; n < N; n += 256) {
        double x = 0.0;
        if (n < a.sz) {
            const double cur = s[n];
            const double prev = n > 0 ? s[n - 1] : 0.0;  // filter([1 -preemph],1,.) with zero state
            x = (cur - a.preemph * prev) * a.win[n];
        }
        bufA[n] = make_double2(x, 0.0);
    }
    __syncthreads();
    const double2* X = fft_lds<LOGN, double>(bufA, fbuf64 + N, a.tw);
    double* o = a.out + (int64_t)t * a.ld;
    for (int f = threadIdx.x; f <= N / 2; f += 256) {
        const double2 c = X[f];
        double mag = hypot(c.x, c.y);       // abs(S_frame), src/stft_fft.m:27
        if (f < a.dcbin) mag = 0.000001;    // :31
        double v;
        if (a.powv == 2.0) v = mag * mag;
        else if (a.powv == 1.0) v = mag;
        else v = pow(mag, a.powv);
        o[f] = v + a.floorv;  // run_basis_train.m:63
    }
}

// src/frame_splice.m:8-23 on the powered magnitudes, then + nonzerofloor (run_basis_train.m:62-63):
// out[(S+s)*K + f, t] = src[f, t+s],  out[(S-s)*K + f, t] = src[f, t-s]  (zero outside 1..T)
static __global__ __launch_bounds__(256) void k_splice64(const double* __restrict__ src, int64_t ld_src, int K, int T, int S, double floorv,
                                                         double* __restrict__ out, int64_t ld_out) {
    const int rows = (2 * S + 1) * K;
    const int64_t n = (int64_t)rows * T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i % rows);
        const int t = (int)(i / rows);
        const int blk = row / K, f = row - blk * K;
        const int ts = t + (blk - S);
        double v = 0.0;
        if (ts >= 0 && ts < T) v = src[(int64_t)ts * ld_src + f];
        out[(int64_t)t * ld_out + row] = v + floorv;
    }
}

// run_basis_train.m:70-78: out[k*M + m, t] = sum_f mel[m, f] * V[k*n + f, t]; one thread per output, f ascending.  The table
// comes TRANSPOSED (melT[f * M + m], the host turns the ABI's row-major M x n round before the upload): the threads of a wave
// differ in m, so each step reads 64 consecutive doubles of the table and one broadcast element of V.
static __global__ __launch_bounds__(256) void k_mel64(const double* __restrict__ melT /*[n][M]*/, int M, int n, int K,
                                                      const double* __restrict__ V, int64_t ldv, int T, double* __restrict__ out, int64_t ldo) {
    const int rows = K * M;
    const int64_t tot = (int64_t)rows * T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i % rows);
        const int t = (int)(i / rows);
        const int k = row / M, m = row - k * M;
        const double* mc = melT + m;
        const double* vc = V + (int64_t)t * ldv + (int64_t)k * n;
        double s = 0.0;
        for (int f = 0; f < n; ++f) s = fma(mc[(int64_t)f * M], vc[f], s);
        out[(int64_t)t * ldo + row] = s;
    }
}

// (v = max(v, flr) of src/sparse_nmf.m:169, k_floor_real in the fp32 front-end, is the solve's own k_s64_floor here: a tight
// matrix has no pad rows to step over)

// ---- TF_DD (src/TF_DD.m:1-9): X_DD(:,1) = X(:,1);  X_DD(:,l) = a X_DD(:,l-1) + (1-a) X(:,l), rows independent, the frame
// axis cut into chunks of kDd64Chunk frames as in snmf_frontend.h.  The recursion starts at column 2 from the state
// X(:,1), which is stored as it is: the first column comes out bit for bit (a x + (1-a) x need not round to x).
//   k_tfdd64_carry : every (chunk, row) runs its chunk from state 0 -> its carry c
//   k_tfdd64_state : per row, the states at the chunk starts: S_{j+1} = a^len_j S_j + c_j (sequential over the chunks)
//   k_tfdd64_apply : every (chunk, row) re-runs its chunk from the true start state and writes the result
constexpr int kDd64Chunk = 256;
__device__ __forceinline__ int tfdd64_first(int j) { return j == 0 ? 1 : j * kDd64Chunk; }  // column 1 is no recursion step
static __global__ __launch_bounds__(256) void k_tfdd64_carry(const double* __restrict__ X, int64_t ld, int F, int T, double a,
                                                             double* __restrict__ carry) {
    const int f = blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
    if (f >= F) return;
    const int t1 = min(T, (j + 1) * kDd64Chunk);
    double s = 0.0;
    for (int t = tfdd64_first(j); t < t1; ++t) s = a * s + (1.0 - a) * X[(int64_t)t * ld + f];
    carry[(int64_t)j * F + f] = s;
}
static __global__ __launch_bounds__(256) void k_tfdd64_state(const double* __restrict__ X, int F, int T, double a,
                                                             double* __restrict__ carry /* in: carries, out: start states */) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int nch = (T + kDd64Chunk - 1) / kDd64Chunk;
    double s = X[f];  // the state after column 1
    for (int j = 0; j < nch; ++j) {
        const int len = min(T, (j + 1) * kDd64Chunk) - tfdd64_first(j);
        const double c = carry[(int64_t)j * F + f];
        carry[(int64_t)j * F + f] = s;
        s = pow(a, (double)len) * s + c;
    }
}
static __global__ __launch_bounds__(256) void k_tfdd64_apply(const double* X, int64_t ld, int F, int T, double a,
                                                             const double* __restrict__ state, double* out, int64_t ldo) {
    const int f = blockIdx.y * 256 + threadIdx.x, j = blockIdx.x;
    if (f >= F) return;
    const int t1 = min(T, (j + 1) * kDd64Chunk);
    double s = state[(int64_t)j * F + f];
    if (j == 0) out[f] = s;  // X_DD(:,1) = X(:,1)
    for (int t = tfdd64_first(j); t < t1; ++t) {  // (out may alias X: every element is read before it is written, by this thread)
        s = a * s + (1.0 - a) * X[(int64_t)t * ld + f];
        out[(int64_t)t * ldo + f] = s;
    }
}

// out[j * rows + f] = V[idx[j] * ld + f]: the exemplar columns TF_mag(:, sample_idx) of run_basis_train.m:82-83
static __global__ __launch_bounds__(256) void k_gather64(const double* __restrict__ V, int64_t ld, int rows, const int64_t* __restrict__ idx,
                                                         int n, double* __restrict__ out) {
    const int64_t tot = (int64_t)rows * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
        const int64_t j = i / rows, f = i - j * rows;
        out[i] = V[idx[j] * ld + f];
    }
}

// y = x + d (run_basis_DNMF.m:10)
static __global__ __launch_bounds__(256) void k_add64(const double* __restrict__ x, const double* __restrict__ d, double* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] + d[i];
}

// dst[j * ld_dst + k] = src[j * ld_src + k], k < rows, j < cols: init_h = A_hat(1:R_x,:) / A_hat(R_x+1:end,:) as a copy
// (the solve rescales its init_h in place, src/sparse_nmf.m:157-159)
static __global__ __launch_bounds__(256) void k_rows64(const double* __restrict__ src, int64_t ld_src, int rows, int64_t cols,
                                                       double* __restrict__ dst, int64_t ld_dst) {
    const int64_t tot = (int64_t)rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
        const int64_t j = i / rows, k = i - j * rows;
        dst[j * ld_dst + k] = src[j * ld_src + k];
    }
}

// H[e] = u(e), e < n column-major: the Philox-4x32-10 stream of snmf_plan_set_h_random (snmf_tu_dnmf.hip) as doubles.
// ((x >> 9) + 0.5) * 2^-23 holds 24 significant bits: exact in fp32 and in fp64, so both modes start from the same numbers.
static __global__ __launch_bounds__(256) void k_rand64(double* __restrict__ H, uint64_t n, uint64_t seed) {
    const uint64_t n4 = (n + 3) / 4;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (uint64_t)gridDim.x * 256) {
        uint32_t o[4];
        philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t e = 4 * q + j;
            if (e < n) H[e] = ((double)(o[j] >> 9) + 0.5) * (1.0 / 8388608.0);
        }
    }
}

}  // namespace snmf
