// snmf_online_batch.h -- kernels of the batched online separator (include/snmf.h: snmf_online_batch_*): S independent
// streams of src/bnmf_sep_event_RT_IS16.m, one set of settings, each stream with its own PCM, noise dictionary and
// state g (src/init_buff.m:17-42).  The per-frame arithmetic is that of snmf_online_common.h; here every launch covers all streams:
//   k_obstft      framing + STFT of the S x n frames of a chunk (one workgroup per (frame, stream))
//   k_obmel       B_sep_mode = 'Mel': the normalised Mel features of every (frame, stream), the solve's input
//   k_hsolve_frame<..., BATCH = true> (snmf_kernels.h) the frame solves, one workgroup per (frame, stream)
//   k_obpost      the post-filter, one workgroup per stream walking its frames in order
//   k_obclass     the per-class reconstructions of a frame step (snmf_online_batch_set_classes), behind the solves and
//                 before the adaptation
//   k_obprep_mel  Mel mode: melmat * lambda_d_blk of every stream whose adaptation is due (k_wadapt_batch's V)
//   k_wadapt_batch the W-only adaptation solve of :296-336, one workgroup per stream, gated on the device
//   k_obassemble / k_obrefresh  the re-assembly of :336 and the next frame solve's dictionary images, gated
//   k_obistft<LOGN, float> / k_obtail<float> / k_obola<float>  inverse STFT and overlap-add of src/NTF_sep_event_RT.m:104-124
//   k_obrestart   the state of the listed streams back to init_buff (a new recording; creation restarts all streams)
// The synthesis kernels and the restart of the arrays both modes hold are written once over the element type in
// snmf_online_batch_common.h, and this unit instantiates them with float; the re-assembly's body (all doubles) is there too.
// Frame-indexed buffers are frame-major: the slot of frame i of stream s is i * S + s.  A stream's own state sits at a
// fixed stride per stream.  Nothing is shared between the streams' workgroups, so a stream's bits do not depend on
// the other streams of its batch.
// In Mel mode (snmf_online_batch_set_mel) the frame solve, the adaptation and the re-assembly run at F_order rows on the
// per-stream fp64 Mel master [B_Mel_x | B_Mel_d]; B_DFT_d is set on restart and never adapted (src/bnmf_sep_event_RT_IS16.m).
// Included by snmf_tu_online_batch.hip only.
#pragma once
#include "snmf_online_common.h"
#include "snmf_online_batch_common.h"

namespace snmf {

// src/bnmf_sep_event_RT_IS16.m:65-81 for every (frame, stream); PACK (DFT mode) also writes the floored solve input (k_pack's
// floor) -- in Mel mode k_obmel writes it, at F_order rows
template <int LOGN, bool PACK = true>
__global__ __launch_bounds__(256) void k_obstft(OStftArgs a, OBatchFrames b, float* __restrict__ Vp, int Fp) {
    constexpr int N = 1 << LOGN;
    __shared__ float2 bufA[N];
    __shared__ float2 bufB[N];
    const int i = blockIdx.x, s = blockIdx.y;
    if (i >= b.nfr[s]) return;
    const float* src = a.sig + (i < b.nreal[s] ? b.off[s] + (int64_t)i * a.hop : b.zoff[s]);
    const size_t slot = (size_t)i * b.S + s;
    float* om = a.Ym + slot * a.ld;
    ostft_frame<LOGN, float>(a, src, om, a.Yph + slot * a.ld, bufA, bufB);
    if (!PACK) return;
    __syncthreads();
    float* vp = Vp + slot * Fp;
    for (int f = threadIdx.x; f < (int)a.ld; f += 256) {
        const float v = om[f];
        vp[f] = v > kFlr ? v : kFlr;
    }
}

// :106-120 for every (frame, stream) (omel_features, so a stream's features are the single-stream separator's bits) into Ymel
// (the post-filter's, MelConv = 1) and, floored, into the solve input Vp at the plan's Fp stride.  Grid (C, S), 256 threads.
__global__ __launch_bounds__(256) void k_obmel(const float* __restrict__ Ym, const float* __restrict__ melmat, const int* nfr, int S,
                                               int F, int n1, float* __restrict__ Ymel, float* __restrict__ Vp, int Fp) {
    extern __shared__ float sm[];  // [n1]
    __shared__ float part[4];
    const int i = blockIdx.x, s = blockIdx.y;
    if (i >= nfr[s]) return;
    const size_t slot = (size_t)i * S + s;
    omel_features(Ym + slot * F, melmat, F, n1, sm, part, [&](int m, float v) {
        Ymel[slot * n1 + m] = v;
        Vp[slot * Fp + m] = v > kFlr ? v : kFlr;
    });
}

// per-stream strides of the post-filter state (OPostArgs holds stream 0's pointers)
struct OBatchPost {
    OBatchFrames fr;
    int step;           // >= 0: frame `step` of every stream that has it; < 0: all frames of the chunk in order
    int rp;             // stride of the activation vectors
    int64_t sB;         // B stride: the fp32 [B_DFT_x | B_DFT_d] of Mel mode without MelConv (unused when the reconstructions
                        // come from the frame solve)
};

// One workgroup per stream: opost_frame on that stream's state, its frames one after the other.
__global__ __launch_bounds__(1024) void k_obpost(OPostArgs a0, OBatchPost b) {
    extern __shared__ float sm[];
    __shared__ double red[16];
    const int s = blockIdx.x, S = b.fr.S, n = b.fr.nfr[s];
    const int F = a0.F, Pl = a0.Pl, ma = a0.ma, Ra = a0.Ra;
    OPostArgs as = a0;
    as.lambda_dav += (size_t)s * F;
    as.Xm_tilde += (size_t)s * F;
    as.r_blk += (size_t)s * F * Pl;
    as.ldblk += (size_t)s * F * ma;
    as.adblk += (size_t)s * Ra * ma;
    as.rup += (size_t)s * Ra;
    as.dev += s;
    as.B += (size_t)s * b.sB;
    const int i0 = b.step >= 0 ? b.step : 0, i1 = b.step >= 0 ? b.step + 1 : n;
    for (int i = i0; i < i1 && i < n; ++i) {
        const size_t slot = (size_t)i * S + s;
        OPostArgs a = as;
        a.A = a0.A + slot * b.rp;
        a.hst = a0.hst + slot;
        if (a.recon) a.recon = a0.recon + slot * 2 * a0.recon_len;
        if (a.Ymel) a.Ymel = a0.Ymel + slot * a0.n1;
        a.Ym = a0.Ym + slot * F;
        a.Xt_out = a0.Xt_out + slot * F;
        if (a.Xh_out) a.Xh_out = a0.Xh_out + slot * F;
        if (a.Dh_out) a.Dh_out = a0.Dh_out + slot * F;
        a.status = a0.status + slot;
        a.l = b.fr.l0[s] + i;
        opost_frame<float>(a, sm, red);
        __syncthreads();  // state written by this frame (global + LDS scratch) is visible to the next
    }
}

// The class spectra (oclass_dft / oclass_mel, as k_oclass) for every stream of a frame step: Xm_hat(c) = B(:, R_c) * A(R_c) (src/bnmf_sep_event_RT_IS16.m:158-202;
// MelConv = 1: melmat' * (B_Mel(:, R_c) * A(R_c))) from the stream's fp64 master, rounded to fp32 as the single-stream
// separator's mirror is, so a stream's class spectra are that separator's.  Slot q's class c goes to out + c*cstride + q*F.
struct OBatchClassArgs {
    const double* B;      // [S][r][F] the masters [B_DFT_x | B_DFT_d]; MelConv = 1: [S][r][n1] the Mel masters
    const float* A;       // activations of slot q at A + q*rp
    const int* cls;       // [n_cls + 1] column ranges
    const float* melmat;  // [n1][F] (MelConv = 1)
    float* out;
    int64_t cstride;
    int n_cls, F, n1, mel_conv, rp, r;
};

// Grid (ceil(F / 256), S, frames): step >= 0: frame `step` of every stream that has it (grid z = 1); step < 0: frame
// blockIdx.z.  Streams without that frame leave (nfr, as their neighbours).  Dynamic LDS: n_cls * n1 floats with MelConv = 1.
__global__ __launch_bounds__(256) void k_obclass(OBatchClassArgs a, OBatchFrames fr, int step) {
    extern __shared__ float sm[];
    const int s = blockIdx.y, i = step >= 0 ? step : (int)blockIdx.z;
    if (i >= fr.nfr[s]) return;  // (uniform over the workgroup)
    const size_t slot = (size_t)i * fr.S + s;
    const float* A = a.A + slot * a.rp;
    float* out = a.out + slot * a.F;
    if (a.mel_conv) oclass_mel<double>(a.B + (size_t)s * a.r * a.n1, A, a.cls, a.n_cls, a.n1, a.melmat, a.F, out, a.cstride, sm);
    else oclass_dft<float, double, float>(a.B + (size_t)s * a.r * a.F, A, a.cls, a.n_cls, a.F, out, a.cstride);
}

// Mel mode's V of the adaptation solve (:298-303): melmat * lambda_d_blk (omel_project), column c of stream s's ring into
// column c of Vm (ring order: k_wadapt_batch reads it as it reads the ring, at F_order rows) for every stream whose
// adaptation is due.  Grid (m_a, S), 256 threads.
__global__ __launch_bounds__(256) void k_obprep_mel(const OnlineStatus* status, const int* nfr, int step, int S, const float* __restrict__ ldblk,
                                                    const float* __restrict__ melmat, int F, int n1, int ma, float* __restrict__ Vm) {
    const int c = blockIdx.x, s = blockIdx.y;
    if (!ob_due(status, nfr, step, S, s)) return;
    omel_project(ldblk + ((size_t)s * ma + c) * F, melmat, F, n1, Vm + ((size_t)s * ma + c) * n1);
}

// ---------------------------------------------------------------------------------------------
// k_wadapt_batch: the W-only adaptation solve (src/bnmf_sep_event_RT_IS16.m:296-336 -> src/sparse_nmf.m:157-286 with
// h_update_ind all false) for every stream whose status says it is due, ONE workgroup per stream: no grid barrier, no
// cooperative launch, and the decomposition does not depend on S.  Any beta (BM).
// Geometry: 16 waves; wave w takes the blocks of 4 rows of W b = w, w + 16, ...; within a block lane t (t + 64) forms
// Lam' and the ratio of its frames, then lane k (k + 64) the statistics of its columns.  H (both orientations) and the
// per-wave operand images live in LDS.  The fp64 master of W, the statistics G / P and the time-ordered V live in
// per-stream global scratch, and every element of that scratch is written and read by the SAME thread, so the
// workgroup never exchanges data through global memory; the cross-row column sums (colsum(G.*W), the norms) are
// per-wave partials added in LDS in wave order (bit-reproducible).
// ---------------------------------------------------------------------------------------------
constexpr int kWbNW = 16, kWbNT = kWbNW * 64, kWbRB = 4;  // waves, threads, rows per block

struct WBatchArgs {
    const OnlineStatus* status;
    const int* nfr;
    int step, S;
    const float* ldblk;    // [S][ma][F] lambda_d_blk rings
    const float* adblk;    // [S][ma][Ra] Ad_blk rings
    const uint8_t* rup;    // [S][Ra]
    const OnlineDev* dev;  // [S]
    const double* B;       // [S][r][F] dictionaries: init_w = the first R_a noise columns
    double* Wu;            // [S][Ra][F] the solve's W (result: normalised)
    float* G;              // [S][Fb][RA2] numerator statistics
    float* P;              // [S][Fb][RA2] denominator statistics (beta != 1)
    float* Vt;             // [S][Fb / 4][ma][4] V in time order, floored
    int* iters;            // [chunk slots] iterations of the solve
    int F, r, Rx, Ra, ma, max_iter, cost_check, RA2;  // RA2 = Ra rounded up to 64
    float sparsity, flr, beta, inv_bb1;
    double conv_eps;
};

// dynamic LDS of k_wadapt_batch in bytes
__host__ __device__ inline size_t wbatch_lds(int Ra, int ma, int RA2, int BMKL) {
    const size_t doubles = (size_t)5 * RA2 + (size_t)kWbNW * 2 * RA2 + 2 * kWbNW;  // nrm cs cq cp sk(float) | wave partials
    const size_t floats = (size_t)((Ra * ma + 3) & ~3) + (size_t)ma * RA2 + (size_t)kWbNW * (kWbRB * Ra + kWbRB * ma * (BMKL ? 1 : 2));
    return doubles * 8 + floats * 4;
}

template <int BM>
__global__ __launch_bounds__(kWbNT) void k_wadapt_batch(WBatchArgs a) {
    constexpr int NW = kWbNW, RB = kWbRB;
    constexpr bool KL = BM == BM_KL;
    const int s = blockIdx.x;
    if (!ob_due(a.status, a.nfr, a.step, a.S, s)) return;  // (uniform over the workgroup)
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const int F = a.F, Ra = a.Ra, ma = a.ma, RA2 = a.RA2, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Fb = (F + RB - 1) / RB * RB, nblk = Fb / RB;
    double* nrm = wsm;                   // [RA2]
    double* cs = nrm + RA2;              // [RA2] colsum of the normalised W
    double* cq = cs + RA2;               // [RA2] colsum(G .* W)
    double* cp = cq + RA2;               // [RA2] colsum(P .* W)
    float* sk = reinterpret_cast<float*>(cp + RA2);  // [RA2] rowsum(H)  (RA2 doubles reserved)
    double* wpart = cp + 2 * RA2;        // [NW][2][RA2]
    double* dpart = wpart + NW * 2 * RA2;  // [2 * NW]
    float* Hs = reinterpret_cast<float*>(dpart + 2 * NW);  // [Ra][ma]
    float* HT = Hs + ((Ra * ma + 3) & ~3);  // [ma][RA2] (16-byte aligned, as the per-wave images behind it)
    float* wv = HT + ma * RA2;           // per wave: Wt [Ra][RB], Rt [ma][RB] (, Dt [ma][RB])
    const int wstride = RB * Ra + RB * ma * (KL ? 1 : 2);
    float* Wt = wv + w * wstride;
    float* Rt = Wt + RB * Ra;
    float* Dt = Rt + RB * ma;

    const float* ld = a.ldblk + (size_t)s * ma * F;
    const float* ad = a.adblk + (size_t)s * ma * Ra;
    const uint8_t* rup = a.rup + (size_t)s * Ra;
    const double* W0 = a.B + (size_t)s * a.r * F + (size_t)a.Rx * F;
    double* Wu = a.Wu + (size_t)s * Ra * F;
    float* G = a.G + (size_t)s * Fb * RA2;
    float* P = a.P + (size_t)s * Fb * RA2;
    float* Vt = a.Vt + (size_t)s * Fb * ma;
    const int oldest = a.dev[s].n_push % ma;

    // ---- load (oprep_elem's inputs: rings in time order, rows not in r_up zeroed) + src/sparse_nmf.m:157-169 ----------
    for (int i = tid; i < Ra * ma; i += kWbNT) {
        const int k = i / ma, t = i - k * ma;
        Hs[i] = rup[k] ? ad[(size_t)((oldest + t) % ma) * Ra + k] : 0.f;
    }
    // this thread's V (lane <-> frame t, rows of its blocks) and W (lane <-> column k) entries, and the column sums of W
    double s2[2] = {0.0, 0.0}, s1[2] = {0.0, 0.0};
    for (int b = w; b < nblk; b += NW) {
        const int f0 = b * RB;
        for (int t = lane; t < ma; t += 64) {
            const float* col = ld + (size_t)((oldest + t) % ma) * F;
#pragma unroll
            for (int j = 0; j < RB; ++j) Vt[((size_t)b * ma + t) * RB + j] = f0 + j < F ? fmaxf(col[f0 + j], a.flr) : 0.f;  // :169
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int k = lane + 64 * c;
            if (k < Ra) {
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    if (f0 + j >= F) continue;  // (the last block's pad rows: Wu holds F rows per column)
                    const double x = W0[(size_t)k * F + f0 + j];
                    Wu[(size_t)k * F + f0 + j] = x;
                    s2[c] += x * x;
                    s1[c] += x;
                }
            }
        }
    }
    auto colsums = [&](const double (&q0)[2], const double (&q1)[2], double* out0, double* out1) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int k = lane + 64 * c;
            if (k < RA2) {
                wpart[(w * 2) * RA2 + k] = q0[c];
                wpart[(w * 2 + 1) * RA2 + k] = q1[c];
            }
        }
        __syncthreads();
        for (int k = tid; k < RA2; k += kWbNT) {
            double x0 = 0.0, x1 = 0.0;
            for (int q = 0; q < NW; ++q) {
                x0 += wpart[(q * 2) * RA2 + k];
                x1 += wpart[(q * 2 + 1) * RA2 + k];
            }
            out0[k] = x0;
            out1[k] = x1;
        }
        __syncthreads();
    };
    colsums(s2, s1, cq, cs);
    for (int k = tid; k < RA2; k += kWbNT) {
        const double wn = k < Ra ? sqrt(cq[k]) : 1.0;  // wn
        nrm[k] = wn;
        cs[k] = cs[k] / wn;
    }
    __syncthreads();
    for (int i = tid; i < Ra * ma; i += kWbNT) Hs[i] = (float)((double)Hs[i] * nrm[i / ma]);  // h = h .* wn' (:160)
    __syncthreads();
    for (int i = tid; i < ma * RA2; i += kWbNT) {
        const int t = i / RA2, k = i - t * RA2;
        HT[i] = k < Ra ? Hs[k * ma + t] : 0.f;
    }
    for (int k = tid; k < RA2; k += kWbNT) {
        float x = 0.f;
        if (k < Ra)
            for (int t = 0; t < ma; ++t) x += Hs[k * ma + t];
        sk[k] = x;  // sum(h, 2)
    }
    __syncthreads();
    double sh_const = 0.0;  // sum(sum(sparsity .* h)) (:261): H is fixed
    for (int k = 0; k < Ra; ++k) sh_const += (double)a.sparsity * (double)sk[k];

    double last_cost = 0.0;
    int n_rec = 0;
    bool stopped = false;
    for (int j = 1; j <= a.max_iter + 1; ++j) {
        if (j > a.max_iter && !a.cost_check) break;
        // ---- Lam' = max(W*H, flr), ratio, divergence; G = ratio * H' (and P) ----------------------------------------
        double q0[2] = {0.0, 0.0}, q1[2] = {0.0, 0.0};
        float dterm = 0.f;
        for (int b = w; b < nblk; b += NW) {
            const int f0 = b * RB;
            // w = w ./ wn (in fp64; the products take its fp32 image, the column sums below the fp64 value again)
            auto wnorm = [&](int k, int jj) -> double { return (k < Ra && f0 + jj < F) ? Wu[(size_t)k * F + f0 + jj] / nrm[k] : 0.0; };
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int k = lane + 64 * c;
                if (k < Ra)
#pragma unroll
                    for (int jj = 0; jj < RB; ++jj) Wt[k * RB + jj] = (float)wnorm(k, jj);
            }
            __builtin_amdgcn_wave_barrier();
            float acc[2][RB];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) acc[c][jj] = 0.f;
            const bool t1 = lane + 64 < ma;
            for (int k = 0; k < Ra; ++k) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(Wt + k * RB);
                const float h0 = lane < ma ? Hs[k * ma + lane] : 0.f;
                const float h1 = t1 ? Hs[k * ma + lane + 64] : 0.f;
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) {
                    acc[0][jj] = fmaf(w4[jj], h0, acc[0][jj]);
                    acc[1][jj] = fmaf(w4[jj], h1, acc[1][jj]);
                }
            }
            if (KL) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int t = lane + 64 * c;
                    if (t < ma) {
#pragma unroll
                        for (int jj = 0; jj < RB; ++jj) {
                            const bool real = f0 + jj < F;
                            const float lam = fmaxf(acc[c][jj], a.flr), v = Vt[((size_t)b * ma + t) * RB + jj];
                            if (real) dterm += div_term<BM>(v, lam, a.beta, a.inv_bb1);
                            Rt[t * RB + jj] = real ? v * fast_rcp(lam) : 0.f;
                        }
                    }
                }
            } else {
                // Lam' through this lane's own LDS slots first, then one entry at a time: the powers (OCML powf) unrolled
                // over all eight entries spilled
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int t = lane + 64 * c;
                    if (t < ma)
#pragma unroll
                        for (int jj = 0; jj < RB; ++jj) Rt[t * RB + jj] = fmaxf(acc[c][jj], a.flr);
                }
#pragma unroll 1
                for (int e = 0; e < 2 * RB; ++e) {
                    const int t = lane + 64 * (e / RB), jj = e % RB;
                    if (t >= ma) continue;
                    const bool real = f0 + jj < F;
                    const float lam = Rt[t * RB + jj], v = Vt[((size_t)b * ma + t) * RB + jj];
                    if (real) dterm += div_term<BM>(v, lam, a.beta, a.inv_bb1);
                    const float den = den_of_lam<BM>(lam, a.beta);
                    float lf = 1.f;  // lam^(beta-2) from den, as the frame solve
                    if (BM != BM_EUC) lf = (a.beta == 0.f) ? den * den : fast_pow(den, (a.beta - 2.f) / (a.beta - 1.f));
                    Rt[t * RB + jj] = real ? v * lf : 0.f;
                    Dt[t * RB + jj] = real ? den : 0.f;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // G = ratio * H' (KL) resp. num * H', then P = den * H' (beta != 1): one product at a time (two sets of
            // accumulators at once spilled)
            const bool k1 = lane + 64 < Ra;
            for (int pass = 0; pass < (KL ? 1 : 2); ++pass) {
                const float* img = pass ? Dt : Rt;
                float g[2][RB];
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int jj = 0; jj < RB; ++jj) g[c][jj] = 0.f;
                for (int t = 0; t < ma; ++t) {
                    const f32x4 r4 = *reinterpret_cast<const f32x4*>(img + t * RB);
                    const float x0 = HT[t * RA2 + lane];
                    const float x1 = k1 ? HT[t * RA2 + lane + 64] : 0.f;
#pragma unroll
                    for (int jj = 0; jj < RB; ++jj) {
                        g[0][jj] = fmaf(r4[jj], x0, g[0][jj]);
                        g[1][jj] = fmaf(r4[jj], x1, g[1][jj]);
                    }
                }
                float* dst = pass ? P : G;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int k = lane + 64 * c;
                    if (k < Ra) {
#pragma unroll
                        for (int jj = 0; jj < RB; ++jj) {
                            dst[(size_t)(f0 + jj) * RA2 + k] = g[c][jj];
                            const double x = (double)g[c][jj] * wnorm(k, jj);  // colsum(G .* W) (:217), colsum(P .* W)
                            if (pass) q1[c] += x;
                            else q0[c] += x;
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();  // (Wt / Rt of the next block)
        }
        {
            const float dw = wave_sum_f(dterm);
            if (lane == 0) dpart[w] = (double)dw;
        }
        stress_jitter();  // (-DSNMF_STRESS builds only: the waves reach the exchange in a random order)
        colsums(q0, q1, cq, cp);
        double div = 0.0;
        for (int q = 0; q < NW; ++q) div += dpart[q];
        if (a.cost_check && j > 1) {  // cost of iterate j-1 (:260-284)
            const double cost = div + sh_const;
            const int it = j - 1;
            bool stopnow = false;
            if (it > 1 && a.conv_eps > 0.0) stopnow = fabs(cost - last_cost) / last_cost < a.conv_eps;
            n_rec = it;
            last_cost = cost;
            if (stopnow) {
                stopped = true;
                break;
            }
        }
        if (j > a.max_iter) break;
        // ---- W update (:215-222) on this thread's entries, then the norms -------------------------------------------
#pragma unroll
        for (int c = 0; c < 2; ++c) s2[c] = s1[c] = 0.0;
        for (int b = w; b < nblk; b += NW) {
            const int f0 = b * RB;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int k = lane + 64 * c;
                if (k >= Ra) continue;
                const bool up = rup[k] != 0;
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) {
                    if (f0 + jj >= F) continue;
                    double wv0 = Wu[(size_t)k * F + f0 + jj] / nrm[k];
                    if (up) {
                        const double gq = (double)G[(size_t)(f0 + jj) * RA2 + k];
                        const double pv = KL ? (double)sk[k] : (double)P[(size_t)(f0 + jj) * RA2 + k];
                        double dpw = pv + wv0 * cq[k];
                        dpw = dpw > (double)a.flr ? dpw : (double)a.flr;
                        wv0 = wv0 * (gq + wv0 * (KL ? pv * cs[k] : cp[k])) / dpw;
                    }
                    Wu[(size_t)k * F + f0 + jj] = wv0;
                    s2[c] += wv0 * wv0;
                    s1[c] += wv0;
                }
            }
        }
        stress_jitter();
        colsums(s2, s1, cq, cs);
        for (int k = tid; k < RA2; k += kWbNT) {
            const double nr = k < Ra ? sqrt(cq[k]) : 1.0;
            nrm[k] = nr;
            cs[k] = cs[k] / nr;  // colsum of the normalised W (:242 normalises ALL columns)
        }
        __syncthreads();
    }
    // the result, normalised, by the threads that own the entries
    for (int b = w; b < nblk; b += NW) {
        const int f0 = b * RB;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int k = lane + 64 * c;
            if (k >= Ra) continue;
#pragma unroll
            for (int jj = 0; jj < RB; ++jj)
                if (f0 + jj < F) Wu[(size_t)k * F + f0 + jj] = Wu[(size_t)k * F + f0 + jj] / nrm[k];
        }
    }
    if (tid == 0) a.iters[(size_t)a.step * a.S + s] = stopped ? n_rec : a.max_iter;
}

// the re-assembly of every stream whose adaptation ran (oassemble_cols, snmf_online_batch_common.h); grid (Rd, S)
__global__ __launch_bounds__(256) void k_obassemble(const OnlineStatus* status, const int* nfr, int step, int S, const double* B,
                                                    const double* Wu, const double* Bfix, int64_t sfix, const uint8_t* rupa, int F,
                                                    int r, int Rx, int Ra, int Rd, double* Btmp) {
    oassemble_cols(status, nfr, step, S, B, Wu, Bfix, sfix, rupa, F, r, Rx, Ra, Rd, Btmp);
}

// ---------------------------------------------------------------------------------------------
// k_obrestart: the restart of the listed streams (snmf_online_batch_common.h: grid (listed stream, array, part), the shared
// arrays through orestart_common) with the fp32 mode's own arrays behind the shared ones: the frame solve's images and, in
// Mel mode, the Mel masters and the fp32 DFT dictionary.  k_obrefresh (slot list form) follows.
// ---------------------------------------------------------------------------------------------
enum : int { kRsWcf = kRsShared, kRsBmx, kRsBmd, kRsBdf, kRsImg, kRsN };

struct ORestartArgs {
    ORestartCommon<float> c;
    float *Wcf, *wx, *dphv, *Hin;
    double* wn;
    // Mel mode (NULL otherwise)
    const double* Bmx;      // [Rx][n1] the shared B_Mel_x
    const double* Bmd;      // [n][Rd][n1] new B_Mel_d, or NULL = keep each stream's (carry)
    double* Bm;             // [S][r][n1] the fp64 Mel masters [B_Mel_x | B_Mel_d]: the solve's dictionary
    float* Bdf;             // [S][r][F] fp32 [B_DFT_x | B_DFT_d] (MelConv = 0: the post-filter's DFT bases)
    int rp, Fp, adapt, n1;
};

__global__ __launch_bounds__(256) void k_obrestart(ORestartArgs a) {
    const int i = blockIdx.x, arr = blockIdx.y, s = a.c.slots[i];
    if (arr < kRsShared) return orestart_common(a.c, arr, a.adapt != 0);
    const size_t F = a.c.F, nX = (size_t)a.c.Rx, nD = (size_t)a.c.Rd, r = a.c.r;
    switch (arr) {
        case kRsWcf: ors_fill(a.Wcf + (size_t)s * a.rp * a.Fp, 0.f, (size_t)a.rp * a.Fp); break;  // rows >= F stay zero
        case kRsBmx:
            if (a.Bm) ors_copy(a.Bm + s * r * a.n1, a.Bmx, nX * a.n1);
            break;
        case kRsBmd:
            if (a.Bm && a.Bmd) ors_copy(a.Bm + s * r * a.n1 + nX * a.n1, a.Bmd + i * nD * a.n1, nD * a.n1);
            break;
        case kRsBdf:  // the fp32 image of the DFT dictionary this restart leaves (kRsBd writes B only when a new one is given)
            if (a.Bdf) {
                float* d = a.Bdf + s * r * F;
                ors_copy(d, a.c.Bx + s * a.c.sBx, nX * F);
                ors_copy(d + nX * F, a.c.Bd ? a.c.Bd + i * nD * F : a.c.B + s * r * F + nX * F, nD * F);
            }
            break;
        default: {  // kRsImg: k_obrefresh writes the r real columns of these; pads: dphv 1.0f (r < 8 * KB must divide by
                    // something finite: 0 * 0 / 0 was NaN in every pad activation and cost), the rest 0
            const size_t o = (size_t)s * a.rp;
            ors_fill(a.wx + o, 0.f, (size_t)a.rp);
            ors_fill(a.dphv + o, 1.f, (size_t)a.rp);
            ors_fill(a.Hin + o, 0.f, (size_t)a.rp);
            ors_fill(a.wn + o, 0.0, (size_t)a.rp);
        }
    }
}

struct ORefreshArgs {
    const OnlineStatus* status;  // NULL: every listed stream, every column from k0 (restart)
    const int* nfr;
    const int* slots;            // NULL: stream blockIdx.y; else stream slots[blockIdx.y]
    int step, S;
    const double* Btmp;  // [S][Rd][F] (status != NULL: the re-assembled noise columns)
    double* B;           // [S][r][F]
    float* Wcf;          // [S][rp][Fp] W ./ wn in fp32 (rows >= F stay zero)
    float* wx;           // [S][rp] row F-1 of Wcf when the frame kernel keeps it outside its register block
    float* dphv;         // [S][rp] KL: max(colsum + lambda, flr)
    double* wn;          // [S][rp]
    float* Hin;          // [S][rp] h .* wn (:160), the frame solve's start
    const float* H0;     // [S][r]
    const float* lamk;   // [rp] the frame plan's sparsity
    int F, r, Rx, rp, Fp, xr, k0;  // columns k0 + blockIdx.x
};

// The next frame solve's images of the dictionary (set_w + k_wapply's init mode, src/sparse_nmf.m:157-160): per
// column the norm, W ./ wn in fp32, its column sum, and H0 .* wn.  One workgroup (256 threads) per (column, stream).
__global__ __launch_bounds__(256) void k_obrefresh(ORefreshArgs a) {
    const int s = a.slots ? a.slots[blockIdx.y] : blockIdx.y, k = a.k0 + blockIdx.x, tid = threadIdx.x;
    if (k >= a.r) return;
    if (a.status && !ob_due(a.status, a.nfr, a.step, a.S, s)) return;
    __shared__ double red[256];
    double* col = a.B + (size_t)s * a.r * a.F + (size_t)k * a.F;
    const double* src = a.status ? a.Btmp + (size_t)s * (a.r - a.Rx) * a.F + (size_t)(k - a.Rx) * a.F : col;
    auto bsum = [&](double v) -> double {  // fixed-order workgroup sum
        red[tid] = v;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        const double x = red[0];
        __syncthreads();
        return x;
    };
    double ssq = 0.0;
    for (int f = tid; f < a.F; f += 256) {
        const double v = src[f];
        ssq += v * v;
    }
    const double nr = sqrt(bsum(ssq));
    double cw = 0.0;
    float* wc = a.Wcf + (size_t)s * a.rp * a.Fp + (size_t)k * a.Fp;
    for (int f = tid; f < a.F; f += 256) {
        const double v = src[f];
        if (a.status) col[f] = v;
        const float wf = (float)(v / nr);
        wc[f] = wf;
        cw += (double)wf;
        if (a.xr && f == a.F - 1) a.wx[(size_t)s * a.rp + k] = wf;
    }
    cw = bsum(cw);
    if (tid == 0) {
        const size_t i = (size_t)s * a.rp + k;
        a.dphv[i] = fmaxf((float)cw + a.lamk[k], kFlr);
        a.wn[i] = nr;
        a.Hin[i] = (float)((double)a.H0[(size_t)s * a.r + k] * nr);
    }
}

// The listed streams' state g into (k_obstate_get) / out of (k_obstate_put) a slab of records (ostate_xfer,
// snmf_online_batch_common.h); grid (listed stream, kStN, kStParts).  k_obrefresh (slot list form) follows a put.
__global__ __launch_bounds__(256) void k_obstate_get(OStateArgs<float> a) { ostate_xfer<float, false>(a); }
__global__ __launch_bounds__(256) void k_obstate_put(OStateArgs<float> a) { ostate_xfer<float, true>(a); }

}  // namespace snmf
