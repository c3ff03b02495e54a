// snmf_frontend_batch.h -- the spectrogram front-end GROUPED over the signals of a batch, in float and in double
// (snmf_tu_frontend_batch.hip: snmf_stft_features_batch_*, snmf_run_basis_dnmf_audio_batch_*, snmf_run_basis_train_audio_batch_*).
//   src/stft_fft.m:15-37        framing, pre-emphasis, window, zero-padded FFT, |.|, DC-bin value   k_stft_grp / k_stft64_grp
//   run_basis_train.m:60-63     splice, .^pow + nonzerofloor                                        k_splice_grp
//   run_basis_train.m:70-78     Mel projection                                                      k_mel_grp
//   run_basis_train.m:64-67     TF_DD, in place                                                     k_tfdd_carry_grp / _state_grp / _apply_grp
//   run_basis_DNMF.m:10         y = x + d, over the whole sample slab                               k_add_grp
// The single front-end (snmf_frontend.h, snmf_frontend64.h) launches per signal and per matrix: k_stft<LOGN> runs one workgroup
// per frame of ONE signal, k_splice / k_mel one matrix.  Here one launch covers every signal of the batch, so the number of
// launches of a call does not depend on the number of signals.  A device table has one FeSig per signal:
//   k_stft*_grp   grid = the frames of all signals; a workgroup finds its signal by a binary search of the frame prefix sums
//                 (FeSig::f0: uniform loads, log2 n steps), then is that signal's frame blockIdx.x - f0
//   element-wise  grid (workgroups, signal): blockIdx.y is the signal, its elements are spread over gridDim.x workgroups
// Offsets into the sample slab and into the matrices are 64-bit.
// Bits.  A frame, a spliced element and a Mel output are formed by the expressions of the single kernels, restated here operation
// for operation -- the Stockham butterflies (the fp64 form calls the same fft_lds), the epilogue, the sequential Mel dot product
// with f ascending (float: s += mel[m][f] * v[f] on the row-major table; double: fma on the transposed table) -- and none of
// them depends on the workgroup that forms it or on the leading dimension it is stored with.  So every feature column is bit
// for bit what snmf_stft_features_* (+ snmf_mel_features_*) give for that signal alone.  The single kernels are left untouched.
// Every kernel checks its bounds; nothing is padded; no atomics.
#pragma once
#include "snmf_online_common.h"

namespace snmf {

struct FeSig {
    int64_t s0;       // k_stft*_grp: the signal's first sample in the sample slab
    int64_t f0;       // k_stft*_grp: frames of the signals before it
    const void* src;  // element-wise passes: the signal's first input column
    void* dst;        // the signal's first output column
    int64_t ld_src, ld_dst;
    int T;            // frames (at least 1: a signal without a frame has no entry)
};

// the entry whose frames hold frame g of the launch: the last one with f0 <= g (g < f0 + T of the last entry)
__device__ __forceinline__ FeSig fe_find(const FeSig* __restrict__ sig, int n, int64_t g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (sig[mid].f0 <= g) lo = mid;
        else hi = mid;
    }
    return sig[lo];
}

struct StftGrpArgs {
    const float* slab;   // the samples of every signal
    const FeSig* sig;
    int n_sig;
    int sz, shift, dcbin;
    float preemph;
    const float* win;    // [sz]
    const float2* tw;    // [N/2] exp(-2*pi*i*q/N)
    float powv, floorv;  // floorv is added here only when there is no splicing pass
};

// k_stft<LOGN> (snmf_frontend.h) for every (signal, frame) of the batch: the frame body restated
template <int LOGN>
__global__ __launch_bounds__(256) void k_stft_grp(StftGrpArgs a) {
    constexpr int N = 1 << LOGN;
    __shared__ float2 bufA[N];
    __shared__ float2 bufB[N];
    const FeSig e = fe_find(a.sig, a.n_sig, (int64_t)blockIdx.x);
    const int t = (int)((int64_t)blockIdx.x - e.f0);
    if (t >= e.T) return;
    const float* __restrict__ s = a.slab + e.s0 + (int64_t)t * a.shift;  // 0-based first sample of frame t
    for (int n = threadIdx.x; n < N; n += 256) {
        float x = 0.f;
        if (n < a.sz) {
            const float cur = s[n];
            const float prev = n > 0 ? s[n - 1] : 0.f;  // filter([1 -preemph],1,.) with zero state
            x = (cur - a.preemph * prev) * a.win[n];
        }
        bufA[n] = make_float2(x, 0.f);
    }
    __syncthreads();
    float2* x = bufA;
    float2* y = bufB;
    // Stockham autosort, decimation in frequency: result in natural order after LOGN stages
    for (int l = N / 2, m = 1; l >= 1; l >>= 1, m <<= 1) {
        const int tstep = N / (2 * l);
        for (int idx = threadIdx.x; idx < N / 2; idx += 256) {
            const int j = idx / m, k = idx - j * m;
            const float2 c0 = x[k + j * m];
            const float2 c1 = x[k + j * m + l * m];
            const float2 w = a.tw[j * tstep];
            const float2 d = make_float2(c0.x - c1.x, c0.y - c1.y);
            y[k + 2 * j * m] = make_float2(c0.x + c1.x, c0.y + c1.y);
            y[k + 2 * j * m + m] = make_float2(w.x * d.x - w.y * d.y, w.x * d.y + w.y * d.x);
        }
        __syncthreads();
        float2* tmp = x;
        x = y;
        y = tmp;
    }
    float* o = (float*)e.dst + (int64_t)t * e.ld_dst;
    for (int f = threadIdx.x; f <= N / 2; f += 256) {
        const float2 c = x[f];
        float mag = sqrtf(c.x * c.x + c.y * c.y);  // abs(S_frame), src/stft_fft.m:27
        if (f < a.dcbin) mag = 0.000001f;          // :31
        float v;
        if (a.powv == 2.f) v = mag * mag;
        else if (a.powv == 1.f) v = mag;
        else v = powf(mag, a.powv);
        o[f] = v + a.floorv;  // run_basis_train.m:63
    }
}

struct Stft64GrpArgs {
    const double* slab;
    const FeSig* sig;
    int n_sig;
    int sz, shift, dcbin;
    double preemph;
    const double* win;
    const double2* tw;
    double powv, floorv;
};

// k_stft64<LOGN> (snmf_frontend64.h) for every (signal, frame) of the batch.  The two FFT buffers are dynamic LDS, 2 N double2:
// 128 KB at N = 4096, which needs the function attribute the single kernel sets (ensure_dyn_lds) and leaves one workgroup per CU.
template <int LOGN>
__global__ __launch_bounds__(256) void k_stft64_grp(Stft64GrpArgs a) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __attribute__((aligned(16))) double2 fbuf64g[];
    const FeSig e = fe_find(a.sig, a.n_sig, (int64_t)blockIdx.x);
    const int t = (int)((int64_t)blockIdx.x - e.f0);
    if (t >= e.T) return;
    double2* bufA = fbuf64g;
    const double* s = a.slab + e.s0 + (int64_t)t * a.shift;  // 0-based first sample of frame t
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
    const double2* X = fft_lds<LOGN, double>(bufA, fbuf64g + N, a.tw);
    double* o = (double*)e.dst + (int64_t)t * e.ld_dst;
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

// k_splice / k_splice64 per signal: out[(S+s)*K + f, t] = src[f, t+s], zero outside the signal's own frames, then + nonzerofloor
template <typename T>
__global__ __launch_bounds__(256) void k_splice_grp(const FeSig* __restrict__ sig, int K, int S, T floorv) {
    const FeSig e = sig[blockIdx.y];
    const T* __restrict__ src = (const T*)e.src;
    T* __restrict__ out = (T*)e.dst;
    const int rows = (2 * S + 1) * K;
    const int64_t n = (int64_t)rows * e.T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i % rows);
        const int t = (int)(i / rows);
        const int blk = row / K, f = row - blk * K;
        const int ts = t + (blk - S);
        T v = T(0);
        if (ts >= 0 && ts < e.T) v = src[(int64_t)ts * e.ld_src + f];
        out[(int64_t)t * e.ld_dst + row] = v + floorv;
    }
}

// k_mel / k_mel64 per signal: out[k*M + m, t] = sum_f mel[m, f] * V[k*n + f, t], one thread per output, f ascending.
// float: `mel` is the ABI's row-major M x n table and the sum is k_mel's s += mel[m][f] * v[f]; double: `mel` is the table
// transposed (n x M, as k_mel64 reads it) and the sum is its fma chain.
template <typename T>
__global__ __launch_bounds__(256) void k_mel_grp(const FeSig* __restrict__ sig, const T* __restrict__ mel, int M, int n, int K) {
    const FeSig e = sig[blockIdx.y];
    const T* __restrict__ V = (const T*)e.src;
    T* __restrict__ out = (T*)e.dst;
    const int rows = K * M;
    const int64_t tot = (int64_t)rows * e.T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i % rows);
        const int t = (int)(i / rows);
        const int k = row / M, m = row - k * M;
        const T* vc = V + (int64_t)t * e.ld_src + (int64_t)k * n;
        T s = T(0);
        if constexpr (sizeof(T) == 4) {
            const T* mr = mel + (int64_t)m * n;
            for (int f = 0; f < n; ++f) s += mr[f] * vc[f];
        } else {
            const T* mc = mel + m;
            for (int f = 0; f < n; ++f) s = fma(mc[(int64_t)f * M], vc[f], s);
        }
        out[(int64_t)t * e.ld_dst + row] = s;
    }
}

// ---- TF_DD (src/TF_DD.m, run_basis_train.m:64-67) of every signal of the batch, IN PLACE on the signal's feature block (FeSig::dst,
// ld_dst): the chunked recursion of snmf_frontend.h (float: k_tfdd_carry / _state / _apply) and snmf_frontend64.h (double:
// k_tfdd64_*) restated operation for operation -- fp64 state and coefficients, chunks of 256 frames, the same expressions in the
// same order -- so every column is bit for bit what snmf_tf_dd_f32 / _fp64 give for that signal alone.  The two differ where
// the single kernels differ: in double the recursion starts at column 2 from the state X(:,1), which is stored as it is; in
// float column 1 goes through the recursion from the state X(:,1) like every other.
// The table has one FeSig per signal with f0 = the CHUNKS of the signals before it, so fe_find maps a workgroup of the carry and
// apply passes to (signal, chunk); the state pass has the signal in blockIdx.y.  carry: [chunks of the batch][F] doubles.
constexpr int kDdGrpChunk = 256;  // kDdChunk and kDd64Chunk: the chunk length is part of the bits
template <typename T>
__device__ __forceinline__ int tfdd_grp_first(int j) {  // first column a chunk's recursion steps over
    return (sizeof(T) == 8 && j == 0) ? 1 : j * kDdGrpChunk;
}
// grid (chunks of the batch, ceil(F / 256)): every (signal, chunk, row) runs its chunk from state 0 -> its carry
template <typename T>
__global__ __launch_bounds__(256) void k_tfdd_carry_grp(const FeSig* __restrict__ sig, int n_sig, int F, double a, double* __restrict__ carry) {
    const FeSig e = fe_find(sig, n_sig, (int64_t)blockIdx.x);
    const int f = blockIdx.y * 256 + threadIdx.x, j = (int)((int64_t)blockIdx.x - e.f0);
    if (f >= F || (int64_t)j * kDdGrpChunk >= e.T) return;
    const T* X = (const T*)e.dst;
    const int64_t ld = e.ld_dst;
    const int t1 = min(e.T, (j + 1) * kDdGrpChunk);
    double s = 0.0;
    for (int t = tfdd_grp_first<T>(j); t < t1; ++t) s = a * s + (1.0 - a) * (double)X[(int64_t)t * ld + f];
    carry[(int64_t)blockIdx.x * F + f] = s;
}
// grid (ceil(F / 256), signals): per row, the states at the chunk starts, S_{j+1} = a^len_j S_j + c_j, sequential over the
// signal's chunks; carry in, start states out
template <typename T>
__global__ __launch_bounds__(256) void k_tfdd_state_grp(const FeSig* __restrict__ sig, int F, double a, double* __restrict__ carry) {
    const FeSig e = sig[blockIdx.y];
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const T* X = (const T*)e.dst;
    double* c = carry + e.f0 * F;
    const int nch = (e.T + kDdGrpChunk - 1) / kDdGrpChunk;
    double s = (double)X[f];  // float: the state "before" column 1 (a x + (1-a) x); double: the state after column 1
    for (int j = 0; j < nch; ++j) {
        const int len = min(e.T, (j + 1) * kDdGrpChunk) - tfdd_grp_first<T>(j);
        const double cj = c[(int64_t)j * F + f];
        c[(int64_t)j * F + f] = s;
        s = pow(a, (double)len) * s + cj;
    }
}
// grid as the carry pass: every (signal, chunk, row) re-runs its chunk from the true start state and writes the result over its
// input (every element is read before it is written, by this thread)
template <typename T>
__global__ __launch_bounds__(256) void k_tfdd_apply_grp(const FeSig* __restrict__ sig, int n_sig, int F, double a, const double* __restrict__ state) {
    const FeSig e = fe_find(sig, n_sig, (int64_t)blockIdx.x);
    const int f = blockIdx.y * 256 + threadIdx.x, j = (int)((int64_t)blockIdx.x - e.f0);
    if (f >= F || (int64_t)j * kDdGrpChunk >= e.T) return;
    T* X = (T*)e.dst;
    const int64_t ld = e.ld_dst;
    const int t1 = min(e.T, (j + 1) * kDdGrpChunk);
    double s = state[(int64_t)blockIdx.x * F + f];
    if (sizeof(T) == 8 && j == 0) X[f] = (T)s;  // X_DD(:,1) = X(:,1)
    for (int t = tfdd_grp_first<T>(j); t < t1; ++t) {
        s = a * s + (1.0 - a) * (double)X[(int64_t)t * ld + f];
        X[(int64_t)t * ld + f] = (T)s;
    }
}

// y = x + d (run_basis_DNMF.m:10) over the sample slab of the whole batch: signal k sits at one offset in x, d and y, and the
// sum is taken in the sample type
template <typename T>
__global__ __launch_bounds__(256) void k_add_grp(const T* __restrict__ x, const T* __restrict__ d, T* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] + d[i];
}

}  // namespace snmf
