// snmf_online_common.h -- the per-frame arithmetic of the online separators, ONE body per reference step, shared by the
// fp32 single-stream separator (snmf_online.h), its fp64 mode (snmf_online_f64.h) and the batched separator
// (snmf_online_batch.h).  Reference (shipped configuration: blk_len_sep = 1, Splice = 0):
//   src/bnmf_sep_event_RT_IS16.m:65-81     frame STFT: |Y|^pow with DC bins zeroed + floor, phase
//   src/bnmf_sep_event_RT_IS16.m:106-120   Mel features of a frame
//   src/bnmf_sep_event_RT_IS16.m:158-202   reconstructions  Xm_hat = B_x*A_x,  Dm_hat = B_d*A_d
//   src/blk_sparse.m:1-37                  Hoyer block sparsity Q
//   src/bnmf_sep_event_RT_IS16.m:220-261   adaptive beta, smoothed noise PSD, Wiener / MMSE gain
//   src/bnmf_sep_event_RT_IS16.m:263-347   noise-reference rings, r_up, dictionary re-assembly
//   src/synth_ifft_buff.m:1-32             inverse STFT of a frame
//   src/NTF_sep_event_RT.m:104-124         overlap-add, int16 output
// The steps are templates on the real type T (float or double); the kernels that launch them are thin: they own the
// indexing (frame, stream, class) and the LDS policy.  Where the two precisions differ ON PURPOSE the difference is an
// overload or a constexpr on T below, marked "deliberate": each is today's behaviour of one of the separators and decides
// bits.  Everything here is a template or __device__ __forceinline__, so every translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_cooperative_groups.h>
#include <stdint.h>
#include <type_traits>
#include "snmf_kernels.h"

namespace snmf {

struct OnlineStatus {  // written once per frame, read back by the host
    int trig, do_solve, n_up, n_iter;
    float beta, A_x_mag, A_d_mag, Q_control;  // diagnostics: float in every precision (deliberate)
};

struct OnlineDev {     // device-resident scalar state of the loop
    int n_push;        // pushes into the noise-reference rings (lambda_d_blk / Ad_blk)
    int update_switch; // src/init_buff.m:42
    int pad0, pad1;
};

// ---- what depends on the precision ----------------------------------------------------------------------------------
template <typename T> struct OPrec;
template <> struct OPrec<float> {
    using cplx = float2;
    using iters = DevState;  // the engine's frame solve leaves its iteration count in its DevState
};
template <> struct OPrec<double> {
    using cplx = double2;
    using iters = int;       // k_hsolve64 writes a plain int per frame
};
template <typename T> using ocplx = typename OPrec<T>::cplx;
__device__ __forceinline__ float2 omake(float x, float y) { return make_float2(x, y); }
__device__ __forceinline__ double2 omake(double x, double y) { return make_double2(x, y); }
// |x + iy|: the plain form in fp32, hypot in fp64 (deliberate)
__device__ __forceinline__ float omag(float x, float y) { return sqrtf(x * x + y * y); }
__device__ __forceinline__ double omag(double x, double y) { return hypot(x, y); }
__device__ __forceinline__ int oiters(const DevState* s) { return s->n_iter; }
__device__ __forceinline__ int oiters(const int* s) { return *s; }
static_assert((float)0.1 == 0.1f && (float)0.0031 == 0.0031f, "T(0.1) / T(0.0031) are the fp32 separator's 0.1f / 0.0031f");

// radix-2 Stockham autosort FFT of N = 2^LOGN points held in LDS; returns the buffer with the result
template <int LOGN, typename T>
__device__ __forceinline__ ocplx<T>* fft_lds(ocplx<T>* x, ocplx<T>* y, const ocplx<T>* __restrict__ tw) {
    constexpr int N = 1 << LOGN;
    for (int l = N / 2, m = 1; l >= 1; l >>= 1, m <<= 1) {
        const int tstep = N / (2 * l);
        for (int idx = threadIdx.x; idx < N / 2; idx += blockDim.x) {
            const int j = idx / m, k = idx - j * m;
            const ocplx<T> c0 = x[k + j * m];
            const ocplx<T> c1 = x[k + j * m + l * m];
            const ocplx<T> w = tw[j * tstep];
            const ocplx<T> d = omake(c0.x - c1.x, c0.y - c1.y);
            y[k + 2 * j * m] = omake(c0.x + c1.x, c0.y + c1.y);
            y[k + 2 * j * m + m] = omake(w.x * d.x - w.y * d.y, w.x * d.y + w.y * d.x);
        }
        __syncthreads();
        ocplx<T>* t = x;
        x = y;
        y = t;
    }
    return x;
}

template <typename T>
struct OStftArgsT {
    const T* sig;      // [(sz - hop) history | n_frames * hop new samples]; frame i starts at i*hop
    int sz, hop, dcbin;
    T preemph;
    const T* win;
    const ocplx<T>* tw;  // twiddles, computed by the host in T
    T powv, floorv;
    T* Ym;             // column i at Ym + i*ld
    ocplx<T>* Yph;     // exp(i*angle(Y)) per bin, same layout
    int64_t ld;
    int n_frames;
};
using OStftArgs = OStftArgsT<float>;

// src/bnmf_sep_event_RT_IS16.m:65-81 for the frame whose samples start at s; magnitude / phase columns om / op.
// bufA / bufB: N complex each, the caller's LDS (256 threads)
template <int LOGN, typename T>
__device__ __forceinline__ void ostft_frame(const OStftArgsT<T>& a, const T* s, T* om, ocplx<T>* op, ocplx<T>* bufA, ocplx<T>* bufB) {
    constexpr int N = 1 << LOGN;
    for (int n = threadIdx.x; n < N; n += 256) {
        T x = T(0);
        if (n < a.sz) {
            const T cur = s[n];
            const T prev = n > 0 ? s[n - 1] : T(0);  // filter([1 -preemph],1,y), zero state (:66)
            x = (cur - a.preemph * prev) * a.win[n];  // :67
        }
        bufA[n] = omake(x, T(0));
    }
    __syncthreads();
    const ocplx<T>* X = fft_lds<LOGN, T>(bufA, bufB, a.tw);
    for (int f = threadIdx.x; f <= N / 2; f += 256) {
        const ocplx<T> c = X[f];
        const T mag = omag(c.x, c.y);
        T v;
        if (a.powv == T(2)) v = mag * mag;
        else if (a.powv == T(1)) v = mag;
        else v = pow(mag, a.powv);
        if (f < a.dcbin) v = T(0);                       // :74
        om[f] = v + a.floorv;                            // :77
        op[f] = mag > T(0) ? omake(c.x / mag, c.y / mag) : omake(T(1), T(0));  // angle(0) = 0
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// fixed-order block sum, result in every thread; red holds one double per wave
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    return s;
}
// block maximum, result in every thread (fmax skips NaN, as MATLAB's max)
template <typename T>
__device__ __forceinline__ T block_max(T v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)v;
    __syncthreads();
    T s = (T)red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) s = fmax(s, (T)red[i]);
    return s;
}

template <typename T>
struct OPostArgsT {
    const T* A;           // [r] activations of this frame (fp32: the solver's H buffer, first r of rp)
    const typename OPrec<T>::iters* hst;  // the frame solve's iteration count (oiters)
    const T* B;           // [F x r] column-major, current [B_DFT_x | B_DFT_d] (fp32 with recon == NULL only)
    const T* recon;       // [2][recon_len] per frame: B_x*A_x and B_d*A_d from the frame solve (fp32: NULL = computed here from B)
    const T* Ym;          // [F]
    T* lambda_dav;        // [F] state
    T* Xm_tilde;          // [F] state
    T* r_blk;             // [Pl][F] ring of SNR_local columns
    T* ldblk;             // [ma][F] ring  lambda_d_blk
    T* adblk;             // [ma][Ra] ring Ad_blk
    uint8_t* rup;         // [Ra]
    OnlineDev* dev;
    OnlineStatus* status;
    T* Xt_out;            // [F] G .* Ym of this frame
    T* Xh_out;            // [F] Xm_hat_sum (may be NULL)
    T* Dh_out;            // [F] Dm_hat_sum (may be NULL)
    int F, Rx, Rd, Ra, ma, Pl, Pk, dcbin, gap;
    int l;                // 1-based frame index
    int blk_sparse, adapt, wiener, init_N_len, switch_at;
    T alpha_p, alpha_eta, alpha_d, beta0, beta_max, Ar_up, flr;
    // B_sep_mode = 'Mel' (:106-120): the solve ran on Mel features (fp32 only: the fp64 separator has no Mel mode)
    const T* melmat;      // [n1][F] row-major (g.melmat)
    const T* Ymel;        // [n1] this frame's normalised Mel features
    const T* Bmf;         // [n1 x r] fp32 mirror of [B_Mel_x | B_Mel_d] (reconstruction fallback)
    int mel, mel_conv, n1;
    int recon_len;        // rows of one reconstruction in `recon` (F, or n1 with MelConv)
    int n;                // frames handled by this launch, one after the other (> 1 only without adaptation)
    int a_stride;         // distance between the activation vectors of consecutive frames
};
using OPostArgs = OPostArgsT<float>;

// Everything between the frame solve and the inverse STFT, src/bnmf_sep_event_RT_IS16.m:158-292, for one frame.
// sm: (r + 7 F + 3 n1) floats resp. (r + 6 F) doubles of LDS; red: 16 doubles.
template <typename T>
__device__ __forceinline__ void opost_frame(const OPostArgsT<T>& a, T* sm, double* red) {
    constexpr bool kF32 = std::is_same<T, float>::value;
    const int F = a.F, r = a.Rx + a.Rd;
    T* sA = sm;
    T* Xs = sA + r;
    T* Ds = Xs + F;
    T* Q = Ds + F;
    T* rs1 = Q + F;
    T* rs2 = rs1 + F;
    T* Gs = rs2 + F;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n_push0 = a.dev->n_push, sw0 = a.dev->update_switch;
    for (int k = tid; k < r; k += nt) sA[k] = a.A[k];
    __syncthreads();
    // A_x_mag, A_d_mag (:228-229)
    double sx = 0.0, sd = 0.0;
    for (int k = tid; k < r; k += nt) {
        if (k < a.Rx) sx += (double)sA[k];
        else sd += (double)sA[k];
    }
    sx = block_sum_d(sx, red);
    sd = block_sum_d(sd, red);
    const T A_x_mag = (T)(sx / a.Rx), A_d_mag = (T)(sd / a.Rd);
    // Xm_hat_sum = B_x*A_x, Dm_hat_sum = B_d*A_d (:158-202; any class partition sums to these)
    T* Ymd = Gs + F;  // fp32 only: [F] Ym_Mel_DFT (first frame only), then [3*n1] Mel-domain vectors
    if constexpr (kF32) {  // the Mel branches and recon == NULL exist in fp32 only (deliberate: k_opost64 does not grow)
        if (a.mel && a.mel_conv) {
            // :165-171,:185-192: reconstructions in the Mel domain, mapped back with melmat'; :205-211 Ym_Mel_DFT
            float* Xm = Ymd + F;
            float* Dm = Xm + a.n1;
            float* Ym1 = Dm + a.n1;
            for (int m = tid; m < a.n1; m += nt) {
                float x, d;
                if (a.recon) {
                    x = a.recon[m];
                    d = a.recon[a.recon_len + m];
                } else {
                    x = 0.f;
                    d = 0.f;
                    const float* b = a.Bmf + m;
                    for (int k = 0; k < a.Rx; ++k) x = fmaf(b[(size_t)k * a.n1], sA[k], x);
                    b += (size_t)a.Rx * a.n1;
                    for (int k = 0; k < a.Rd; ++k) d = fmaf(b[(size_t)k * a.n1], sA[a.Rx + k], d);
                }
                Xm[m] = x;
                Dm[m] = d;
                Ym1[m] = a.Ymel[m];
            }
            __syncthreads();
            for (int f = tid; f < F; f += nt) {
                float x = 0.f, d = 0.f, y = 0.f;
                for (int m = 0; m < a.n1; ++m) {
                    const float mm = a.melmat[(size_t)m * F + f];
                    x = fmaf(mm, Xm[m], x);
                    d = fmaf(mm, Dm[m], d);
                    y = fmaf(mm, Ym1[m], y);
                }
                Xs[f] = x;
                Ds[f] = d;
                Ymd[f] = y;
            }
        } else if (a.recon) {
            for (int f = tid; f < F; f += nt) {
                Xs[f] = a.recon[f];
                Ds[f] = a.recon[a.recon_len + f];
                Ymd[f] = a.Ym[f];
            }
        } else {
            for (int f = tid; f < F; f += nt) {
                const float* b = a.B + f;
                float x = 0.f, d = 0.f;
                for (int k = 0; k < a.Rx; ++k) x = fmaf(b[(size_t)k * F], sA[k], x);
                b += (size_t)a.Rx * F;
                for (int k = 0; k < a.Rd; ++k) d = fmaf(b[(size_t)k * F], sA[a.Rx + k], d);
                Xs[f] = x;
                Ds[f] = d;
                Ymd[f] = a.Ym[f];
            }
        }
    } else {
        for (int f = tid; f < F; f += nt) {
            Xs[f] = a.recon[f];
            Ds[f] = a.recon[a.recon_len + f];
        }
    }
    __syncthreads();
    // ---- src/blk_sparse.m ----
    if (a.blk_sparse) {
        // the maximum starts at 0 in fp32 and at -inf in fp64 (deliberate; the quotients are never negative, so the start is
        // not known to be reachable)
        T mx = kF32 ? T(0) : T(-INFINITY);
        for (int f = tid; f < F; f += nt) {
            const T s = Xs[f] / fmax(Ds[f], a.flr);  // :10
            rs1[f] = s;
            mx = fmax(mx, s);
        }
        mx = block_max<T>(mx, red);
        T* col = a.r_blk + (size_t)((a.l - 1) % a.Pl) * F;  // newest column of the ring (:14)
        for (int f = tid; f < F; f += nt) {
            col[f] = rs1[f] / mx;                                // :12
            Q[f] = f < a.dcbin ? T(0) : T(0.1);                  // :16
        }
        __syncthreads();
        if (a.l > a.Pl) {
            for (int f = tid; f < F; f += nt) {
                T s1 = T(0), s2 = T(0);
                for (int c = 0; c < a.Pl; ++c) {
                    const T v = a.r_blk[(size_t)c * F + f];
                    s1 += v;
                    s2 = fma(v, v, s2);
                }
                rs1[f] = s1;
                rs2[f] = s2;
            }
            __syncthreads();
            const int k2 = a.Pk / 2, gN2 = (a.gap - 1) / 2;
            const int kfirst = k2 + a.dcbin, klast = F - k2;  // 1-based, :20
            const int nwin = klast >= kfirst ? (klast - kfirst) / a.gap + 1 : 0;
            const double sqn = sqrt((double)a.Pl * (double)a.Pk);
            for (int j = tid; j < nwin; j += nt) {
                const int k = kfirst + j * a.gap;
                double l1 = 0.0, l2 = 0.0;
                for (int row = k - k2; row < k + k2; ++row) {  // 1-based rows k-k2+1 .. k+k2
                    l1 += (double)rs1[row];
                    l2 += (double)rs2[row];
                }
                Gs[j] = (T)((sqn - l1 / sqrt(l2)) / (sqn - 1.0));  // :26
            }
            __syncthreads();
            if (gN2 >= 1) {
                // blk_gap >= 3: window k reads Q(k-1), which no other window writes (window k-gap ends at
                // k-gap+gN2 < k-1), so the recursion of :28 sees the initial value and windows are independent
                for (int j = tid; j < nwin; j += nt) {
                    const int k = kfirst + j * a.gap;
                    const T qprev = (k - 2) < a.dcbin ? T(0) : T(0.1);
                    const T pv = a.alpha_p * qprev + (T(1) - a.alpha_p) * Gs[j];
                    for (int i = k - gN2 - 1; i <= k + gN2 - 1; ++i) Q[i] = pv;  // :29-30
                }
            } else if (tid == 0) {
                // blk_gap = 1: a genuine first-order recursion along frequency
                for (int j = 0; j < nwin; ++j) {
                    const int k = kfirst + j;
                    Q[k - 1] = a.alpha_p * Q[k - 2] + (T(1) - a.alpha_p) * Gs[j];
                }
            }
            __syncthreads();
            const T qv = Q[a.Pk + a.dcbin - 1];
            __syncthreads();
            for (int f = tid; f < a.Pk - 1; f += nt) Q[f] = qv;  // :32
            __syncthreads();
        }
        for (int f = tid; f < a.dcbin; f += nt) Q[f] = T(0);     // :36
    } else {
        for (int f = tid; f < F; f += nt) Q[f] = T(1);           // :217
    }
    __syncthreads();
    double qs = 0.0;
    for (int f = tid; f < F; f += nt) qs += (double)Q[f];
    qs = block_sum_d(qs, red);
    const T meanQ = (T)(qs / F);
    // ---- gain (:221-261) ----
    // :230-231: the dB value is formed in double and rounded to T BEFORE the product with beta0 (deliberate: fp32's order)
    T beta = (T)(20.0 * log10((double)A_d_mag / (double)A_x_mag)) * a.beta0;
    if (beta < a.beta0) beta = a.beta0;
    else if (beta >= a.beta_max) beta = a.beta_max;
    const bool init = a.l <= a.init_N_len;
    for (int f = tid; f < F; f += nt) {
        const T ym = a.Ym[f];
        // :223-225: frame 1 starts from Ym_Mel_DFT in fp32 (= Ym outside Mel mode), from Ym in fp64 (deliberate)
        T ld;
        if constexpr (kF32) ld = a.l == 1 ? Ymd[f] : a.lambda_dav[f];
        else ld = a.l == 1 ? ym : a.lambda_dav[f];
        ld = a.alpha_d * ld + (T(1) - a.alpha_d) * Ds[f] * beta;          // :241
        a.lambda_dav[f] = ld;
        T G;
        if (a.wiener) {
            G = Xs[f] / (Xs[f] + Ds[f]);                                  // :245
        } else {
            T eta = (a.alpha_eta * a.Xm_tilde[f] + (T(1) - a.alpha_eta) * Xs[f] * Q[f]) / fmax(ld, a.flr);  // :247
            eta = fmax(T(0.0031), eta);                                   // :251
            G = eta / (eta + T(1));
        }
        G = fmin(G, T(1));                                                // :254 (min ignores NaN, as MATLAB's)
        if (init) G = a.flr;                                              // :256-258
        Gs[f] = G;
        const T xt = G * ym;                                              // :260
        a.Xm_tilde[f] = xt;
        a.Xt_out[f] = xt;
        if (a.Xh_out) a.Xh_out[f] = Xs[f];
        if (a.Dh_out) a.Dh_out[f] = Ds[f];
    }
    const T A_x_eff = init ? a.flr : A_x_mag;                             // :258
    const T Q_control = (T(1) - meanQ) * a.Ar_up;                         // :264
    const bool trig = a.adapt && (Q_control * A_d_mag > A_x_eff);         // :266
    int do_solve = 0, n_up = 0;
    __syncthreads();
    if (trig) {
        const int head = n_push0 % a.ma;  // overwrites the oldest column == shift + append (:282,:285)
        for (int f = tid; f < F; f += nt) {
            const T ym = a.Ym[f];
            const T mref = f < a.dcbin ? a.flr : T(1) - Gs[f];            // :271-272
            a.ldblk[(size_t)head * F + f] = init ? ym : ym * mref;        // :268-274
        }
        for (int k = tid; k < a.Ra; k += nt) a.adblk[(size_t)head * a.Ra + k] = sA[a.Rx + k];
        __syncthreads();
        int cnt = 0;
        for (int k = tid; k < a.Ra; k += nt) {
            // the ring mean in double: slots in slot order in fp32, oldest first in fp64 (deliberate: the order decides
            // bits that feed the > of :288)
            double s = 0.0;
            for (int c = 0; c < a.ma; ++c) s += (double)a.adblk[(size_t)(kF32 ? c : (head + 1 + c) % a.ma) * a.Ra + k];
            const bool up = (double)Q_control * (s / a.ma) > (double)A_x_eff;  // :288
            a.rup[k] = up ? 1 : 0;
            cnt += up;
        }
        n_up = (int)(block_sum_d((double)cnt, red) + 0.5);
        do_solve = sw0 == a.switch_at;                                    // :294
        if (tid == 0) {
            a.dev->n_push = n_push0 + 1;
            a.dev->update_switch = do_solve ? 1 : sw0 + 1;                // :343-345
        }
    }
    if (tid == 0) {
        OnlineStatus s;
        s.trig = trig;
        s.do_solve = do_solve;
        s.n_up = n_up;
        s.n_iter = oiters(a.hst);
        s.beta = (float)beta;
        s.A_x_mag = (float)A_x_eff;
        s.A_d_mag = (float)A_d_mag;
        s.Q_control = (float)Q_control;
        *a.status = s;
    }
}

// Inputs of the adaptation solve (:296-335) in time order: V = lambda_d_blk, H = Ad_blk with the
// rows not flagged by r_up zeroed (the reference drops those rows/columns; a zero activation row
// contributes nothing to Lam, G or the cost, so the flagged columns see the same problem), and
// the solve's W-update mask = r_up.  Element i of the F*ma + Ra*ma + Ra outputs (the kernels walk them grid-stride); oldest =
// n_push % ma, the ring slot of the oldest column.
template <typename T>
__device__ __forceinline__ void oprep_elem(size_t i, int oldest, const T* __restrict__ ldblk, const T* __restrict__ adblk,
                                           const uint8_t* __restrict__ rup, int F, int Ra, int ma, T* __restrict__ Vad,
                                           T* __restrict__ Had, uint8_t* __restrict__ w_ind) {
    const size_t nv = (size_t)F * ma, nh = (size_t)Ra * ma;
    if (i < nv) {
        const int c = (int)(i / F), f = (int)(i - (size_t)c * F);
        Vad[i] = ldblk[(size_t)((oldest + c) % ma) * F + f];
    } else if (i < nv + nh) {
        const size_t j = i - nv;
        const int c = (int)(j / Ra), k = (int)(j - (size_t)c * Ra);
        Had[j] = rup[k] ? adblk[(size_t)((oldest + c) % ma) * Ra + k] : T(0);
    } else {
        const int k = (int)(i - nv - nh);
        w_ind[k] = rup[k];
    }
}

// B_DFT_d = [B_d_rem, B_d_tmp, B_d_fix] (:336): kept columns first, then the re-trained ones (the columns beyond R_a come
// from the original dictionary, :328: the caller's).  For the new column j < Ra: the old column it copies, and whether that
// is a column of the adaptation solve's result (*retrained) or of the dictionary as it was.
__device__ __forceinline__ int oassemble_col(const uint8_t* __restrict__ rup, int Ra, int j, bool* retrained) {
    int n_rem = 0;
    for (int k = 0; k < Ra; ++k) n_rem += rup[k] ? 0 : 1;
    const bool want_up = j >= n_rem;
    int need = want_up ? j - n_rem : j, k = 0;
    for (; k < Ra; ++k) {
        if ((rup[k] != 0) == want_up) {
            if (need == 0) break;
            --need;
        }
    }
    *retrained = want_up;
    return k;
}

template <typename T>
struct OIstftArgsT {
    const T* mag;      // column i at mag + i*ld  (magnitude^pow domain)
    const ocplx<T>* ph;
    int64_t ld;
    int n_frames, sz, dcb;
    T powv, scale, preemph;  // scale = overlapscale / N
    const T* win;
    const ocplx<T>* tw;
    T* syn;            // frame i at syn + i*sz
};
using OIstftArgs = OIstftArgsT<float>;

// src/synth_ifft_buff.m:10-28 (+ the overlapscale of src/bnmf_sep_event_RT_IS16.m:363): magnitude / phase columns mg / ph
// -> the windowed frame o.  bufA / bufB: N complex each, the caller's LDS (256 threads)
template <int LOGN, typename T>
__device__ __forceinline__ void oistft_frame(const OIstftArgsT<T>& a, const T* mg, const ocplx<T>* ph, T* o, ocplx<T>* bufA,
                                             ocplx<T>* bufB) {
    constexpr int N = 1 << LOGN;
    // real(ifft(X)) = real(fft(conj(X)))/N with X(N-k) = conj(X(k)) for k = 1..N/2-1 (:16-18)
    for (int k = threadIdx.x; k < N; k += 256) {
        const int kk = k <= N / 2 ? k : N - k;
        T m = kk < a.dcb ? T(0) : mg[kk];                       // :10
        if (a.powv == T(2)) m = sqrt(m);                        // :11
        else if (a.powv != T(1)) m = pow(m, T(1) / a.powv);
        const ocplx<T> p = ph[kk];
        bufA[k] = omake(m * p.x, k <= N / 2 ? -m * p.y : m * p.y);
    }
    __syncthreads();
    ocplx<T>* X = fft_lds<LOGN, T>(bufA, bufB, a.tw);
    if (a.preemph == T(0)) {
        for (int n = threadIdx.x; n < a.sz; n += 256) o[n] = X[n].x * a.scale * a.win[n];  // :19-24
    } else {
        for (int n = threadIdx.x; n < a.sz; n += 256) X[n].y = X[n].x * a.scale * a.win[n];
        __syncthreads();
        if (threadIdx.x == 0) {  // filter(1, [1 -preemph], .) (:26)
            T acc = T(0);
            for (int n = 0; n < a.sz; ++n) {
                acc = X[n].y + a.preemph * acc;
                o[n] = acc;
            }
        }
    }
}

// Overlap-add of src/NTF_sep_event_RT.m:104-124 in closed form, one output sample: sample s of the hop written at frame
// l = l0 + i is the sum over the frames l-q (q = nov-1 .. 0, oldest first, only frames > delay were ever accumulated) of
// their samples q*hop + s.  syn holds nov-1 frames of the previous call, then the new ones (i counts the new ones).
// The sum goes to outf[o] and, rounded as fwrite(..,'int16') does -- half away from zero, saturated, NaN -> 0 as MATLAB's
// integer conversion -- to out16[o] (either may be NULL).
template <typename T>
__device__ __forceinline__ void oola_sample(const T* __restrict__ syn, int i, int s, int l0, int delay, int sz, int hop, int nov,
                                            T* __restrict__ outf, int16_t* __restrict__ out16, size_t o) {
    T acc = T(0);
    for (int q = nov - 1; q >= 0; --q) {
        const int lq = l0 + i - q, off = q * hop + s;
        if (lq > delay && lq >= 1 && off < sz) acc += syn[(size_t)(i - q + nov - 1) * sz + off];
    }
    if (outf) outf[o] = acc;
    if (out16) {
        T rr = copysign(floor(fabs(acc) + T(0.5)), acc);
        rr = fmin(fmax(rr, T(-32768)), T(32767));
        if (!(acc == acc)) rr = T(0);
        out16[o] = (int16_t)rr;
    }
}

// :106-120 for one frame: Ym_Mel = melmat*Ym, normalised to unit norm (+1e-9) and scaled to ||Ym||; feature m goes to
// store(m, value).  One workgroup of 256 threads, one wave per group of outputs; sm: n1 floats, part: 4 floats of LDS.
template <typename Store>
__device__ __forceinline__ void omel_features(const float* __restrict__ y, const float* __restrict__ melmat, int F, int n1, float* sm,
                                              float* part, Store&& store) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float tn2 = 0.f;
    for (int f = tid; f < F; f += 256) tn2 = fmaf(y[f], y[f], tn2);
    tn2 = wave_sum_f(tn2);
    if (lane == 0) part[w] = tn2;
    for (int m = w; m < n1; m += 4) {
        float s = 0.f;
        for (int f = lane; f < F; f += 64) s = fmaf(melmat[(size_t)m * F + f], y[f], s);
        s = wave_sum_f(s);
        if (lane == 0) sm[m] = s;
    }
    __syncthreads();
    const float tn = sqrtf(part[0] + part[1] + part[2] + part[3]);
    float vn2 = 0.f;
    for (int m = tid; m < n1; m += 256) vn2 = fmaf(sm[m], sm[m], vn2);
    vn2 = wave_sum_f(vn2);
    __syncthreads();
    if (lane == 0) part[w] = vn2;
    __syncthreads();
    const float vn = sqrtf(part[0] + part[1] + part[2] + part[3]);
    for (int m = tid; m < n1; m += 256) store(m, (sm[m] / vn + 1e-9f) * tn);
}

// Mel mode's V of the adaptation solve (:298-303): out = melmat * col for one ring column of lambda_d_blk.  One workgroup
// of 256 threads, one wave per group of outputs.
__device__ __forceinline__ void omel_project(const float* __restrict__ col, const float* __restrict__ melmat, int F, int n1,
                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int m = w; m < n1; m += 4) {
        float s = 0.f;
        for (int f = lane; f < F; f += 64) s = fmaf(melmat[(size_t)m * F + f], col[f], s);
        s = wave_sum_f(s);
        if (lane == 0) out[m] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// Per-class reconstructions (src/bnmf_sep_event_RT_IS16.m:158-202): p.EVENT_RANK / p.NOISE_RANK cut [B_x | B_d] into
// classes of consecutive columns, class c = columns cls[c] .. cls[c+1]-1 (0-based over the r columns; event classes
// first, cls[n_cls] = r).  Xm_hat(c) = B(:, R_c) * A(R_c) from the frame's activations and the dictionary the frame solve
// saw, so the launch sits between the frame solve and the adaptation.  With p.pow = 2 the synthesis takes a square root
// (src/synth_ifft_buff.m:11): the class signals cannot be had from the sums afterwards.
// One thread per bin f (rows coalesced along f), the columns walked once in order for all classes; the class of column k
// does not depend on the thread, so the boundaries are uniform branches and the activations scalar loads.  Each class
// is one fma chain in fp64 over values of the output precision TO: a class of 30 columns out of 200 has none of the sum's
// averaging, and the fp64 chain keeps its rounding to the one final conversion.  TB: how the dictionary is stored (the
// batched separator keeps fp64 masters only; their fp32 rounding IS the single-stream separator's mirror).
// ---------------------------------------------------------------------------------------------
constexpr int kOClassMax = 32;  // classes per side (snmf_online_set_classes refuses more)

template <typename TO, typename TB, typename TA>
__device__ __forceinline__ void oclass_dft(const TB* __restrict__ B, const TA* __restrict__ A, const int* __restrict__ cls, int n_cls,
                                           int F, TO* __restrict__ out, int64_t cstride) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    for (int c = 0; c < n_cls; ++c) {
        const int k1 = cls[c + 1];
        double acc = 0.0;
#pragma unroll 4
        for (int k = cls[c]; k < k1; ++k) acc = fma((double)(TO)B[(size_t)k * F + f], (double)A[k], acc);
        out[(size_t)c * cstride + f] = (TO)acc;
    }
}

// 'Mel' with MelConv = 1 (:165-171, :187-195): melmat' * (B_Mel(:, R_c) * A(R_c)).  The n1 x n_cls Mel products first (P, LDS,
// [n_cls][n1]; every workgroup of a frame forms them), then melmat' on them for this workgroup's bins.
template <typename TB>
__device__ __forceinline__ void oclass_mel(const TB* __restrict__ Bm, const float* __restrict__ A, const int* __restrict__ cls,
                                           int n_cls, int n1, const float* __restrict__ melmat, int F, float* __restrict__ out,
                                           int64_t cstride, float* P) {
    for (int i = threadIdx.x; i < n_cls * n1; i += blockDim.x) {
        const int c = i / n1, m = i - c * n1, k1 = cls[c + 1];
        double acc = 0.0;
        for (int k = cls[c]; k < k1; ++k) acc = fma((double)(float)Bm[(size_t)k * n1 + m], (double)A[k], acc);
        P[i] = (float)acc;
    }
    __syncthreads();
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    for (int c = 0; c < n_cls; ++c) {
        double acc = 0.0;
#pragma unroll 4
        for (int m = 0; m < n1; ++m) acc = fma((double)melmat[(size_t)m * F + f], (double)P[c * n1 + m], acc);
        out[(size_t)c * cstride + f] = (float)acc;
    }
}

// ---------------------------------------------------------------------------------------------
// The exchange of the cooperative adaptation solves (k_wadapt, k_wadapt64): sc1 stores / loads, a fixed-order
// cross-workgroup sum and a bounded-spin grid barrier.
// ---------------------------------------------------------------------------------------------

// exchange accesses: agent-scope relaxed atomics = sc1 write-through stores / coherent loads (see grid_bar)
__device__ __forceinline__ void xstore(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double xload(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Cross-workgroup sum of `ncol` (<= 2*RP+1) column quantities, part[q*stride + c], q < nwg, into out[c]
// (LDS).  After the barrier's acquire these loads come from memory, ~2 us each: every thread issues all of
// its loads before the first add (4 thread groups x 64 columns, <= kWaQ workgroups per group), then the
// sums are combined in a fixed order (bit-reproducible).
constexpr int kWaQ = 40;  // workgroups per thread group: covers nwg <= 80
__device__ __forceinline__ void cross_sum(const double* __restrict__ part, int stride, int ncol, int nwg, double* scratch /*[2][128]*/,
                                          double* out /*[128]*/) {
    const int g = threadIdx.x >> 7, c = threadIdx.x & 127;
    if (threadIdx.x < 256) {  // (a workgroup may have more threads than the exchange needs)
        const int per = (nwg + 1) / 2, q0 = g * per;
        double v[kWaQ];
#pragma unroll
        for (int i = 0; i < kWaQ; ++i) {
            const int q = q0 + i;
            v[i] = (i < per && q < nwg && c < ncol) ? xload(part + (size_t)q * stride + c) : 0.0;
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < kWaQ; ++i) s += v[i];
        scratch[g * 128 + c] = s;
    }
    __syncthreads();
    if (threadIdx.x < 128 && threadIdx.x < ncol) out[threadIdx.x] = scratch[c] + scratch[128 + c];
    __syncthreads();
}

// Grid barrier on a monotonic device counter (zeroed before the launch).  cooperative_groups' grid.sync()
// measured ~20 us per call here, and an agent-scope release/acquire pair costs a write-back plus an
// invalidate of the XCD's whole L2 on every workgroup.  Instead, everything the workgroups exchange goes
// through agent-scope (sc1, write-through / coherent) relaxed atomic stores and loads (xstore / xload):
// __syncthreads() waits for those stores to be acknowledged by the coherence point, one relaxed agent-scope
// add publishes the arrival, and the readers' sc1 loads cannot hit a stale line.  The kernel is launched
// cooperatively, so every workgroup is resident; the spin is bounded all the same so that a lost workgroup
// ends in wrong numbers (flagged through n_iter_out = -1), never in a hung GPU.
// (Tried: no barrier at all, every thread re-loading the partial rows until a sentinel value is gone -- "the data
// is the flag".  Correct, but 256 pollers per workgroup flood the coherent path: 2090 instead of 2790 frames/s.
// Tried: 16 / 32 rows per workgroup: the exchange does not get cheaper with fewer workgroups, the products do
// get slower: 2650 / 2400 frames/s.)
// `ok_sp`: one int of the caller's DYNAMIC LDS.  (A static __shared__ here preceded the dynamic region and shifted its base
// by 4 bytes: every 8- / 16-byte LDS access of the kernel was then off its natural alignment and replayed at 64 cycles per
// wave-instruction: statics totalling != 0 (mod 16) shift the base.)
__device__ __forceinline__ bool grid_bar(unsigned* ctr, unsigned nwg, unsigned& gen, int* ok_sp) {
    int& ok_s = *ok_sp;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's exchange stores are acknowledged ...
    __syncthreads();                                   // ... and so are everybody's in the workgroup
    ++gen;
    if (threadIdx.x < 64) stress_jitter();  // (-DSNMF_STRESS builds only: snmf_kernels.h)
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = gen * nwg;
        unsigned spins = 0;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && ++spins < (1u << 24))
            __builtin_amdgcn_s_sleep(1);
        ok_s = spins < (1u << 24);
    }
    __syncthreads();
    return ok_s != 0;
}

}  // namespace snmf
