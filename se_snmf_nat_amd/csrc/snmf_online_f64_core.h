// snmf_online_f64_core.h -- the fp64 frame solve and the dictionary images of the online separators' fp64 modes, as
// __device__ bodies: the single-stream kernels (snmf_online_f64.h: k_hsolve64, k_wnorm64) and the batched ones
// (snmf_online_batch_f64.h: k_obhsolve64, k_obrefresh64) launch the same arithmetic, the kernels own the indexing.
#pragma once
#include "snmf_online_common.h"

namespace snmf {

// src/sparse_nmf.m:157-159 for column k of [B_DFT_x | B_DFT_d] (b, F rows): wn = sqrt(sum(w.^2)), w ./ wn column-major and
// transposed, and the column sum of the normalised w (:192).  One workgroup of 256 threads; red: 4 doubles of LDS.  `keep`
// (may be NULL) also receives the column as it was read.
__device__ __forceinline__ void wnorm64_col(const double* __restrict__ b, double* __restrict__ keep, int F, int r, int k,
                                            double* __restrict__ Wn, double* __restrict__ WnT, double* __restrict__ wn,
                                            double* __restrict__ csum, double* red) {
    double s2 = 0.0;
    for (int f = threadIdx.x; f < F; f += 256) s2 += b[f] * b[f];
    s2 = block_sum_d(s2, red);
    const double nrm = sqrt(s2);
    double s1 = 0.0;
    for (int f = threadIdx.x; f < F; f += 256) {
        const double w = b[f] / nrm;
        if (keep) keep[f] = b[f];
        Wn[(size_t)k * F + f] = w;
        WnT[(size_t)f * r + k] = w;
        s1 += w;
    }
    s1 = block_sum_d(s1, red);
    if (threadIdx.x == 0) {
        wn[k] = nrm;
        csum[k] = s1;
    }
}

// divergence of one element, src/sparse_nmf.m:248-258 (generic beta: the numerator; the caller divides the SUM by
// beta*(beta-1), as the reference does)
__device__ __forceinline__ double div_term_d(double v, double lam, double beta) {
    if (beta == 1.0) return v * log(v / lam) - v + lam;
    if (beta == 2.0) return (v - lam) * (v - lam);
    if (beta == 0.0) {
        const double q = v / lam;
        return q - log(q) - 1.0;
    }
    return pow(v, beta) + (beta - 1.0) * pow(lam, beta) - beta * v * pow(lam, beta - 1.0);
}
__device__ __forceinline__ double div_scale_d(double s, double beta) {
    return (beta == 1.0 || beta == 2.0 || beta == 0.0) ? s : s / (beta * (beta - 1.0));
}

struct HSolve64Args {
    const double* Wn;    // [r][F]  normalised dictionary, column-major
    const double* WnT;   // [F][r]  its transpose
    const double* wn;    // [r]     column norms of the dictionary
    const double* csum;  // [r]     column sums of Wn
    const double* H0;    // [r]     init_h (the same vector every frame)
    const double* V;     // [n][F]  Ym of the frames
    double* A;           // [n][r]  activations
    double* recon;       // [n][2][F]  B_x*A_x | B_d*A_d
    int* n_iter;         // [n]
    int F, r, Rx, max_iter, cost_check, n;
    double beta, sparsity, conv_eps, flr;
};

// The whole H-only loop of src/sparse_nmf.m:157-286 for one frame per workgroup (h_update_ind all true, w_update_ind all
// false), in the reference's sequence: h .* wn', Lam = max(w*h, flr); per iteration the H step, Lam again, the objective,
// the stop test.  16 waves: a wave takes columns of W (lanes along the rows, coalesced in Wn) for the contractions over
// rows, and rows of W (lanes along the columns, coalesced in WnT) for W*h.  Dynamic LDS = (4 F + 3 r + 32) doubles.
__device__ __forceinline__ void hsolve64_frame(const HSolve64Args& a, int fr, double* sm64) {
    const int F = a.F, r = a.r, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nwv = nt >> 6;
    double* vs = sm64;        // [F] max(v, flr)
    double* lam = vs + F;     // [F]
    double* p1 = lam + F;     // [F] numerator weights   v .* lam.^(beta-2)
    double* p2 = p1 + F;      // [F] denominator weights lam.^(beta-1)
    double* h = p2 + F;       // [r]
    double* num = h + r;      // [r]
    double* den = num + r;    // [r]
    double* red = den + r;    // [32]
    const double beta = a.beta;
    const bool kl = beta == 1.0, ed = beta == 2.0;
    const double* v = a.V + (size_t)fr * F;
    for (int f = tid; f < F; f += nt) vs[f] = fmax(v[f], a.flr);          // :169
    for (int k = tid; k < r; k += nt) h[k] = a.H0[k] * a.wn[k];           // :160
    __syncthreads();
    // Lam = max(w*h, flr) and, with it, the weights of the next H step
    auto lam_pass = [&]() {
        for (int f = wv; f < F; f += nwv) {
            const double* wr = a.WnT + (size_t)f * r;
            double s = 0.0;
            for (int k = lane; k < r; k += 64) s = fma(wr[k], h[k], s);
            s = wave_sum_d(s);
            if (lane == 0) {
                const double l = fmax(s, a.flr);
                lam[f] = l;
                if (kl) {
                    p1[f] = vs[f] / l;
                } else if (ed) {
                    p1[f] = vs[f];
                    p2[f] = l;
                } else {
                    p1[f] = vs[f] * pow(l, beta - 2.0);
                    p2[f] = pow(l, beta - 1.0);
                }
            }
        }
        __syncthreads();
    };
    lam_pass();                                                           // :167
    double last_cost = 0.0;
    int n_iter = a.max_iter;
    for (int it = 1; it <= a.max_iter; ++it) {
        // ---- H step (:189-206) ----
        for (int k = wv; k < r; k += nwv) {
            const double* wc = a.Wn + (size_t)k * F;
            double sn = 0.0, sd = 0.0;
            if (kl) {
                for (int f = lane; f < F; f += 64) sn = fma(wc[f], p1[f], sn);
            } else {
                for (int f = lane; f < F; f += 64) {
                    const double w = wc[f];
                    sn = fma(w, p1[f], sn);
                    sd = fma(w, p2[f], sd);
                }
            }
            sn = wave_sum_d(sn);
            if (!kl) sd = wave_sum_d(sd);
            if (lane == 0) {
                num[k] = sn;
                den[k] = fmax((kl ? a.csum[k] : sd) + a.sparsity, a.flr);  // :192-193 / :197-198 / :202-203
            }
        }
        __syncthreads();
        for (int k = tid; k < r; k += nt) h[k] = h[k] * num[k] / den[k];   // :195
        __syncthreads();
        lam_pass();                                                       // :207
        // ---- objective (:248-261) and stop test (:273-284) ----
        double d = 0.0;
        for (int f = tid; f < F; f += nt) d += div_term_d(vs[f], lam[f], beta);
        d = div_scale_d(block_sum_d(d, red), beta);
        if (a.cost_check) {
            double sh = 0.0;
            for (int k = tid; k < r; k += nt) sh += a.sparsity * h[k];
            const double cost = d + block_sum_d(sh, red);
            if (it > 1 && a.conv_eps > 0.0 && fabs(cost - last_cost) / last_cost < a.conv_eps) {  // (NaN < eps is false, as MATLAB's)
                n_iter = it;
                break;
            }
            last_cost = cost;
        }
    }
    __syncthreads();
    // activations and the reconstructions B_x*A_x, B_d*A_d (src/bnmf_sep_event_RT_IS16.m:158-202): B = Wn * diag(wn)
    for (int k = tid; k < r; k += nt) {
        a.A[(size_t)fr * r + k] = h[k];
        num[k] = h[k] * a.wn[k];
    }
    __syncthreads();
    double* rx = a.recon + (size_t)fr * 2 * F;
    for (int f = wv; f < F; f += nwv) {
        const double* wr = a.WnT + (size_t)f * r;
        double x = 0.0, dd = 0.0;
        for (int k = lane; k < r; k += 64) {
            const double t = wr[k] * num[k];
            if (k < a.Rx) x += t;
            else dd += t;
        }
        x = wave_sum_d(x);
        dd = wave_sum_d(dd);
        if (lane == 0) {
            rx[f] = x;
            rx[F + f] = dd;
        }
    }
    if (tid == 0) a.n_iter[fr] = n_iter;
}

}  // namespace snmf
