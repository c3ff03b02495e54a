// snmf_online_batch_f64.h -- kernels of the fp64 mode of the batched online separator (snmf_online_batch_create_f64,
// include/snmf.h): S independent streams, every step from PCM to the fed-back dictionary in double, as the single-stream
// fp64 mode (snmf_online_f64.h) has it for one stream.  The per-frame arithmetic is the double instantiation of
// snmf_online_common.h and the frame solve of snmf_online_f64_core.h; the launch structure is the fp32 batch's
// (snmf_online_batch.h): every launch covers all streams, frame-indexed buffers are frame-major (the slot of frame i of
// stream s is i * S + s), a stream's own state sits at a fixed stride per stream, and nothing is shared between the
// streams' workgroups, so a stream's bits do not depend on the other streams of its batch.
//   k_obstft64     framing + STFT of the S x n frames of a chunk (one workgroup per (frame, stream))
//   k_obhsolve64   the frame solves (hsolve64_frame), one workgroup per (frame, stream), each stream on its own images
//   k_obpost64     the post-filter, one workgroup per stream walking its frames in order
//   k_obclass64    the per-class reconstructions of a frame step, behind the solves and before the adaptation
//   k_wadapt_batch64  the W-only adaptation solve of :296-336, ONE workgroup per due stream, gated on the device
//   k_obassemble64 / k_obrefresh64  the re-assembly of :336 and the next frame solve's dictionary images, gated
//   k_obistft<LOGN, double> / k_obtail<double> / k_obola<double>  inverse STFT and overlap-add of src/NTF_sep_event_RT.m:104-124
//   k_obrestart64  the state of the listed streams back to init_buff, each from its own event dictionary
// The synthesis kernels and the restart's body are written once over the element type in snmf_online_batch_common.h, and this
// unit instantiates them with double; the re-assembly's body (all doubles) is there too.
// Every stream has its own settings (OStreamSettings, a device table indexed by the stream) and its own B_DFT_x; the
// geometry is the batch's.  DFT mode and the supervised frame solve only, as the single-stream fp64 mode.
// Included by snmf_tu_online_batch_f64.hip only.
#pragma once
#include "snmf_online_batch_common.h"
#include "snmf_online_f64_core.h"

namespace snmf {

// Entry s of the per-stream settings table (device, [S], next to the per-stream state): what the frame solve, the
// post-filter, the adaptation and the restart read per stream instead of per launch.  The geometry (transform, windows,
// ranks, ring sizes, cost_check, class partition) stays in the launch arguments: it is the batch's.  Written by the host
// with hipMemcpyAsync from its mirror, read with ordinary loads; s is uniform over a workgroup, so the loads are scalar.
struct OStreamSettings {
    double beta_div, sparsity, conv_eps;               // the frame and adaptation solves (src/sparse_nmf.m)
    double alpha_eta, alpha_d, beta, beta_max;         // the enhancement filter (:221-261)
    double alpha_p, Ar_up;                             // src/blk_sparse.m:28, :264
    int max_iter, enhance_method, init_N_len;
    int blk_sparse, P_len_k, blk_gap;
    int adapt_train_N, switch_at;                      // switch_at = floor(overlap_m_a * m_a) (:294)
};

// src/bnmf_sep_event_RT_IS16.m:65-81 for every (frame, stream); dynamic LDS = 2 N double2 (as k_ostft64)
template <int LOGN>
__global__ __launch_bounds__(256) void k_obstft64(OStftArgsT<double> a, OBatchFrames b) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __attribute__((aligned(16))) double2 fbuf[];
    const int i = blockIdx.x, s = blockIdx.y;
    if (i >= b.nfr[s]) return;
    const double* src = a.sig + (i < b.nreal[s] ? b.off[s] + (int64_t)i * a.hop : b.zoff[s]);
    const size_t slot = (size_t)i * b.S + s;
    ostft_frame<LOGN, double>(a, src, a.Ym + slot * a.ld, a.Yph + slot * a.ld, fbuf, fbuf + N);
}

// The frame solves: `a` holds stream 0's images and H0 and the chunk's slot-indexed buffers; grid (frames, S).  step >= 0:
// frame `step` of every stream that has it (grid x = 1); step < 0: frame blockIdx.x.  Dynamic LDS as k_hsolve64.  The
// divergence, the sparsity weight and the stop rule are entry s of `set`.
__global__ __launch_bounds__(1024) void k_obhsolve64(HSolve64Args a, const OStreamSettings* __restrict__ set, OBatchFrames fr, int step) {
    extern __shared__ __attribute__((aligned(16))) double sm64[];
    const int s = blockIdx.y, i = step >= 0 ? step : (int)blockIdx.x;
    if (i >= fr.nfr[s]) return;  // (uniform over the workgroup)
    const OStreamSettings& q = set[s];
    a.beta = q.beta_div;
    a.sparsity = q.sparsity;
    a.conv_eps = q.conv_eps;
    a.max_iter = q.max_iter;
    const size_t img = (size_t)a.F * a.r;
    a.Wn += (size_t)s * img;
    a.WnT += (size_t)s * img;
    a.wn += (size_t)s * a.r;
    a.csum += (size_t)s * a.r;
    a.H0 += (size_t)s * a.r;
    hsolve64_frame(a, (int)((size_t)i * fr.S + s), sm64);
}

// One workgroup per stream: opost_frame<double> on that stream's state, its frames one after the other (k_obpost's
// indexing).  step >= 0: frame `step` of every stream that has it; < 0: all frames of the chunk in order.  Dynamic LDS =
// (r + 6 F) doubles.  The filter's and the trigger's settings are re-based like the pointers: entry s of `set`.
__global__ __launch_bounds__(1024) void k_obpost64(OPostArgsT<double> a0, const OStreamSettings* __restrict__ set, OBatchFrames fr, int step) {
    extern __shared__ __attribute__((aligned(16))) double sm64[];
    __shared__ double red[16];
    const int s = blockIdx.x, S = fr.S, n = fr.nfr[s];
    const int F = a0.F, r = a0.Rx + a0.Rd;
    OPostArgsT<double> as = a0;
    as.lambda_dav += (size_t)s * F;
    as.Xm_tilde += (size_t)s * F;
    as.r_blk += (size_t)s * F * a0.Pl;
    as.ldblk += (size_t)s * F * a0.ma;
    as.adblk += (size_t)s * a0.Ra * a0.ma;
    as.rup += (size_t)s * a0.Ra;
    as.dev += s;
    {
        const OStreamSettings& q = set[s];
        as.blk_sparse = q.blk_sparse; as.Pk = q.P_len_k; as.gap = q.blk_gap; as.alpha_p = q.alpha_p;
        as.adapt = q.adapt_train_N; as.switch_at = q.switch_at; as.Ar_up = q.Ar_up;
        as.wiener = q.enhance_method == 0; as.init_N_len = q.init_N_len;
        as.alpha_eta = q.alpha_eta; as.alpha_d = q.alpha_d; as.beta0 = q.beta; as.beta_max = q.beta_max;
    }
    const int i0 = step >= 0 ? step : 0, i1 = step >= 0 ? step + 1 : n;
    for (int i = i0; i < i1 && i < n; ++i) {
        const size_t slot = (size_t)i * S + s;
        OPostArgsT<double> a = as;
        a.A = a0.A + slot * r;
        a.hst = a0.hst + slot;
        a.recon = a0.recon + slot * 2 * F;
        a.Ym = a0.Ym + slot * F;
        a.Xt_out = a0.Xt_out + slot * F;
        if (a.Xh_out) a.Xh_out = a0.Xh_out + slot * F;
        if (a.Dh_out) a.Dh_out = a0.Dh_out + slot * F;
        a.status = a0.status + slot;
        a.l = fr.l0[s] + i;
        opost_frame<double>(a, sm64, red);
        __threadfence_block();  // (as k_opost64)
        __syncthreads();  // state written by this frame (global + LDS scratch) is visible to the next
    }
}

// The class spectra (oclass_dft, as k_oclass64) of every stream from its fp64 dictionary [S][r][F]: slot q's class c goes
// to out + c*cstride + q*F.  Grid (ceil(F / 256), S, frames); step as k_obhsolve64 (step < 0: frame blockIdx.z).
__global__ __launch_bounds__(256) void k_obclass64(const double* __restrict__ B, const double* __restrict__ A, const int* __restrict__ cls,
                                                   int n_cls, int F, int r, double* __restrict__ out, int64_t cstride, OBatchFrames fr,
                                                   int step) {
    const int s = blockIdx.y, i = step >= 0 ? step : (int)blockIdx.z;
    if (i >= fr.nfr[s]) return;
    const size_t slot = (size_t)i * fr.S + s;
    oclass_dft<double, double, double>(B + (size_t)s * r * F, A + slot * r, cls, n_cls, F, out + slot * F, cstride);
}

// ---------------------------------------------------------------------------------------------
// k_wadapt_batch64: the W-only adaptation solve (src/bnmf_sep_event_RT_IS16.m:296-336 -> src/sparse_nmf.m:157-286 with
// h_update_ind all false) in fp64 for every stream whose status says it is due, ONE workgroup per stream: no grid barrier,
// no cooperative launch, no wait on another workgroup, and the decomposition does not depend on S.  The arithmetic is
// k_wadapt64's (snmf_online_f64.h): with P = lam.^(beta-1) * h', Q = (v .* lam.^(beta-2)) * h' the update of :215-239 is
//   w .* (Q + colsum(P.*w) .* w) ./ max(P + colsum(Q.*w) .* w, flr)        (beta = 1: P = sum(h,2)', Q = (v./lam) * h').
// Geometry (k_wadapt_batch's, re-budgeted for 8-byte elements): 8 waves; wave w takes the blocks of 4 rows of W
// b = w, w + 8, ...; within a block lane t (and t + 64) forms Lam and the weights of its frames, then lane k the
// statistics of its column (R_a <= 64: one column per lane).  LDS holds ONE orientation of H, [R_a][m_a | 1]: the odd row
// length lets lanes walk it along t (Lam, consecutive doubles) and along k (the statistics, odd stride) without bank
// conflicts, where the fp32 kernel keeps H and its transpose; and per wave the operand images of one row block.
// W, the statistics P / Q and the time-ordered V live in per-stream global scratch, and every element of that scratch is
// written and read by the SAME thread, so the workgroup never exchanges data through global memory; the cross-row column
// sums (colsum(Q.*w), colsum(P.*w), the norms) are per-wave partials added in LDS in wave order, and the divergence is
// summed over the waves in wave order: a stream's bits depend on nothing but its own inputs.
// ---------------------------------------------------------------------------------------------
constexpr int kWb64NW = 8, kWb64NT = kWb64NW * 64, kWb64RB = 4, kWb64RP = 64;  // waves, threads, rows per block, column lanes
constexpr int kWb64MaxMa = 128;  // two frames per lane

struct WBatch64Args {
    const OnlineStatus* status;
    const int* nfr;
    int step, S;
    const double* ldblk;   // [S][ma][F] lambda_d_blk rings
    const double* adblk;   // [S][ma][Ra] Ad_blk rings
    const uint8_t* rup;    // [S][Ra]
    const OnlineDev* dev;  // [S]
    const double* B;       // [S][r][F] dictionaries: init_w = the first R_a noise columns
    double* Wu;            // [S][Ra][F] result, normalised
    double* Wm;            // [S][Fb][RP] the solve's W, row-major
    double* Q;             // [S][Fb][RP] numerator statistics
    double* P;             // [S][Fb][RP] denominator statistics (beta != 1)
    double* Vt;            // [S][Fb / 4][ma][4] V in time order, floored
    int* iters;            // [chunk slots] iterations of the solve
    const OStreamSettings* set;  // [S] beta_div, sparsity, max_iter, conv_eps, adapt_train_N of each stream
    int F, r, Rx, Ra, ma, cost_check;
    double flr;
};

// dynamic LDS of k_wadapt_batch64 in bytes (kl: beta == 1 keeps no denominator image).  R_a <= 64 and m_a <= 128 fit the
// 160 KB of a compute unit for every beta: 159120 bytes at the edge (the shipped 50 x 100 ring, beta = 1: 93536).
__host__ __device__ inline size_t wbatch64_lds(int Ra, int ma, int kl) {
    const size_t small = (size_t)5 * kWb64RP + (size_t)kWb64NW * 2 * kWb64RP + 2 * kWb64NW + kWb64RP / 2 + 2;  // nrm cq cp sk | partials | dpart | act
    const size_t hs = ((size_t)Ra * (ma | 1) + 1) & ~(size_t)1;  // one orientation of H, rows of odd length
    const size_t wave = (size_t)kWb64RB * kWb64RP + (size_t)kWb64RB * ma * (kl ? 1 : 2);
    return (small + hs + kWb64NW * wave) * 8;
}

enum : int { kWb64KL = 0, kWb64ED = 1, kWb64GEN = 2 };
// the instantiation of k_wadapt_batch64 that serves a divergence
__host__ __device__ inline int wbatch64_class(double beta_div) { return beta_div == 1.0 ? kWb64KL : beta_div == 2.0 ? kWb64ED : kWb64GEN; }

// One launch per divergence class present among the adapting streams, each over all S streams with its own dynamic LDS: a
// workgroup whose stream does not adapt, or whose divergence is another instantiation's, returns before it touches LDS or
// scratch.
template <int BM>
__global__ __launch_bounds__(kWb64NT) void k_wadapt_batch64(WBatch64Args a) {
    constexpr int NW = kWb64NW, RB = kWb64RB, RP = kWb64RP, NT = kWb64NT;
    constexpr bool KL = BM == kWb64KL;
    const int s = blockIdx.x;
    const OStreamSettings& set = a.set[s];
    if (!set.adapt_train_N || wbatch64_class(set.beta_div) != BM) return;  // (uniform over the workgroup)
    if (!ob_due(a.status, a.nfr, a.step, a.S, s)) return;
    const int max_iter = set.max_iter;
    const double sparsity = set.sparsity, conv_eps = set.conv_eps;
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const int F = a.F, Ra = a.Ra, ma = a.ma, ma1 = ma | 1, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Fb = (F + RB - 1) / RB * RB, nblk = Fb / RB;
    double* nrm = wsm;                     // [RP]
    double* cq = nrm + RP;                 // [RP] colsum(Q .* w)
    double* cp = cq + RP;                  // [RP] colsum(P .* w)
    double* sk = cp + RP;                  // [RP] rowsum(H)
    double* tmp = sk + RP;                 // [RP]
    double* wpart = tmp + RP;              // [NW][2][RP]
    double* dpart = wpart + NW * 2 * RP;   // [2 NW]
    int* act = reinterpret_cast<int*>(dpart + 2 * NW);  // [1 + RP] number and list of the flagged columns (RP / 2 + 2 doubles)
    double* Hs = dpart + 2 * NW + RP / 2 + 2;            // [Ra][ma1]
    double* wv = Hs + (((size_t)Ra * ma1 + 1) & ~(size_t)1);  // per wave: Wt [RP][RB], Bt [ma][RB] (, At [ma][RB]); 16-byte aligned
    const int wstride = RB * RP + RB * ma * (KL ? 1 : 2);
    double* Wt = wv + (size_t)w * wstride;
    double* Bt = Wt + RB * RP;             // v .* lam.^(beta-2)   (Lam itself on the way)
    double* At = Bt + RB * ma;             // lam.^(beta-1)

    const double* ld = a.ldblk + (size_t)s * ma * F;
    const double* ad = a.adblk + (size_t)s * ma * Ra;
    const uint8_t* rup = a.rup + (size_t)s * Ra;
    const double* W0 = a.B + (size_t)s * a.r * F + (size_t)a.Rx * F;
    double* Wu = a.Wu + (size_t)s * Ra * F;
    double* Wm = a.Wm + (size_t)s * Fb * RP;
    double* Q = a.Q + (size_t)s * Fb * RP;
    double* P = KL ? nullptr : a.P + (size_t)s * Fb * RP;  // (beta = 1 keeps no denominator statistics)
    double* Vt = a.Vt + (size_t)s * Fb * ma;
    const int oldest = a.dev[s].n_push % ma;
    const double beta = set.beta_div;
    const bool kact = lane < Ra;           // this lane owns column `lane`
    const bool up = kact && rup[kact ? lane : 0] != 0;

    // ---- load (oprep_elem's inputs: rings in time order, rows not in r_up zeroed) + src/sparse_nmf.m:157-169 ----------
    for (int i = tid; i < Ra * ma; i += NT) {
        const int k = i / ma, t = i - k * ma;
        Hs[k * ma1 + t] = rup[k] ? ad[(size_t)((oldest + t) % ma) * Ra + k] : 0.0;
    }
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < Ra; ++k)
            if (rup[k]) act[1 + n++] = k;
        act[0] = n;
    }
    // this thread's V (lane <-> frame t, rows of its blocks) and W (lane <-> column k) entries, and the column norms of W
    double s2 = 0.0;
    for (int b = w; b < nblk; b += NW) {
        const int f0 = b * RB;
        for (int t = lane; t < ma; t += 64) {
            const double* col = ld + (size_t)((oldest + t) % ma) * F;
#pragma unroll
            for (int j = 0; j < RB; ++j) Vt[((size_t)b * ma + t) * RB + j] = f0 + j < F ? fmax(col[f0 + j], a.flr) : 0.0;  // :169
        }
        if (kact) {
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const double x = f0 + j < F ? W0[(size_t)lane * F + f0 + j] : 0.0;
                Wm[(size_t)(f0 + j) * RP + lane] = x;
                s2 += x * x;
            }
        }
    }
    // cross-wave column sums of two per-thread quantities, in wave order
    auto colsums = [&](double q0, double q1, double* out0, double* out1) {
        wpart[(w * 2) * RP + lane] = q0;
        wpart[(w * 2 + 1) * RP + lane] = q1;
        __syncthreads();
        if (tid < RP) {
            double x0 = 0.0, x1 = 0.0;
            for (int q = 0; q < NW; ++q) {
                x0 += wpart[(q * 2) * RP + tid];
                x1 += wpart[(q * 2 + 1) * RP + tid];
            }
            out0[tid] = x0;
            out1[tid] = x1;
        }
        __syncthreads();
    };
    // w = w ./ wn on this thread's entries (:158 / :242, ALL columns)
    auto normalise = [&]() {
        if (!kact) return;
        const double wn = nrm[lane];
        for (int b = w; b < nblk; b += NW)
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const size_t e = (size_t)(b * RB + j) * RP + lane;
                Wm[e] = Wm[e] / wn;
            }
    };
    colsums(s2, 0.0, tmp, cp);
    if (tid < RP) nrm[tid] = tid < Ra ? sqrt(tmp[tid]) : 1.0;  // wn
    __syncthreads();
    normalise();
    for (int i = tid; i < Ra * ma; i += NT) {
        const int k = i / ma, t = i - k * ma;
        Hs[k * ma1 + t] = Hs[k * ma1 + t] * nrm[k];            // h = h .* wn'  (:160)
    }
    __syncthreads();
    if (tid < RP) {
        double x = 0.0;
        if (tid < Ra)
            for (int t = 0; t < ma; ++t) x += Hs[tid * ma1 + t];
        sk[tid] = x;                                           // sum(h,2)
    }
    __syncthreads();
    const int nact = act[0];
    double sh_const = 0.0;                                     // sum(sum(sparsity .* h)) (:261), constant: H is fixed
    for (int k = 0; k < Ra; ++k) sh_const += sparsity * sk[k];

    double last_cost = 0.0;
    int n_rec = 0;
    bool stopped = false;
    const bool t1 = lane + 64 < ma;
    const double* hk = Hs + (size_t)(kact ? lane : 0) * ma1;   // this lane's row of H (column k of the statistics)
    for (int j = 1; j <= max_iter + 1; ++j) {
        if (j > max_iter && !a.cost_check) break;
        // ---- Lam = max(w*h, flr) of iterate j-1, its divergence, the weights; P and Q on this wave's row blocks --------
        double q0 = 0.0, q1 = 0.0, dterm = 0.0;
        for (int b = w; b < nblk; b += NW) {
            const int f0 = b * RB;
            double wown[RB];  // this lane's column of the block
#pragma unroll
            for (int jj = 0; jj < RB; ++jj) {
                wown[jj] = kact ? Wm[(size_t)(f0 + jj) * RP + lane] : 0.0;
                Wt[lane * RB + jj] = wown[jj];
            }
            __builtin_amdgcn_wave_barrier();
            double acc[2][RB];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) acc[c][jj] = 0.0;
            for (int q = 0; q < nact; ++q) {
                const int k = act[1 + q];
                const double2 wa = *reinterpret_cast<const double2*>(Wt + k * RB);
                const double2 wb = *reinterpret_cast<const double2*>(Wt + k * RB + 2);
                const double w4[RB] = {wa.x, wa.y, wb.x, wb.y};
                const double h0 = lane < ma ? Hs[k * ma1 + lane] : 0.0;
                const double h1 = t1 ? Hs[k * ma1 + lane + 64] : 0.0;
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) {
                    acc[0][jj] = fma(w4[jj], h0, acc[0][jj]);
                    acc[1][jj] = fma(w4[jj], h1, acc[1][jj]);
                }
            }
            // Lam through this lane's own LDS slots first, then one entry at a time (the fp64 pow / log unrolled over all
            // eight entries would hold eight sets of their temporaries)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int t = lane + 64 * c;
                if (t < ma)
#pragma unroll
                    for (int jj = 0; jj < RB; ++jj) Bt[t * RB + jj] = fmax(acc[c][jj], a.flr);
            }
#pragma unroll 1
            for (int e = 0; e < 2 * RB; ++e) {
                const int t = lane + 64 * (e / RB), jj = e % RB;
                if (t >= ma) continue;
                const bool real = f0 + jj < F;
                const double lam = Bt[t * RB + jj], v = Vt[((size_t)b * ma + t) * RB + jj];
                if (real) dterm += div_term_d(v, lam, beta);
                double pa, pb;
                if (BM == kWb64KL) {
                    pa = 1.0;
                    pb = v / lam;
                } else if (BM == kWb64ED) {
                    pa = lam;
                    pb = v;
                } else {
                    pa = pow(lam, beta - 1.0);
                    pb = v * pow(lam, beta - 2.0);
                }
                Bt[t * RB + jj] = real ? pb : 0.0;
                if (!KL) At[t * RB + jj] = real ? pa : 0.0;
            }
            __builtin_amdgcn_wave_barrier();
            // Q = (v .* lam.^(beta-2)) * h', then P = lam.^(beta-1) * h' (beta != 1), column `lane`, one product at a time
            for (int pass = 0; pass < (KL ? 1 : 2); ++pass) {
                const double* img = pass ? At : Bt;
                double g[RB];
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) g[jj] = 0.0;
                for (int t = 0; t < ma; ++t) {
                    const double2 ra = *reinterpret_cast<const double2*>(img + t * RB);
                    const double2 rb = *reinterpret_cast<const double2*>(img + t * RB + 2);
                    const double x = hk[t];
                    g[0] = fma(ra.x, x, g[0]);
                    g[1] = fma(ra.y, x, g[1]);
                    g[2] = fma(rb.x, x, g[2]);
                    g[3] = fma(rb.y, x, g[3]);
                }
                if (kact) {
                    double* dst = pass ? P : Q;
                    double sum = 0.0;
#pragma unroll
                    for (int jj = 0; jj < RB; ++jj) {
                        dst[(size_t)(f0 + jj) * RP + lane] = g[jj];
                        sum += g[jj] * wown[jj];               // colsum(Q .* w) (:217), colsum(P .* w)
                    }
                    if (pass) q1 += sum;
                    else q0 += sum;
                }
            }
            if (KL)                                            // P = sum(h,2)' on every row: colsum(P .* w) = sum(sk .* w)
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) q1 += sk[lane] * wown[jj];
            __builtin_amdgcn_wave_barrier();  // (Wt / Bt / At of the next block)
        }
        {
            const double dw = wave_sum_d(dterm);
            if (lane == 0) dpart[w] = dw;
        }
        stress_jitter();  // (-DSNMF_STRESS builds only: the waves reach the exchange in a random order)
        colsums(q0, q1, cq, cp);
        double div = 0.0;
        for (int q = 0; q < NW; ++q) div += dpart[q];
        div = div_scale_d(div, beta);
        if (a.cost_check && j > 1) {                           // cost of iterate j-1 (:260-284)
            const double cost = div + sh_const;
            const int it = j - 1;
            bool stopnow = false;
            if (it > 1 && conv_eps > 0.0) stopnow = fabs(cost - last_cost) / last_cost < conv_eps;
            n_rec = it;
            last_cost = cost;
            if (stopnow) {
                stopped = true;
                break;
            }
        }
        if (j > max_iter) break;
        // ---- W update (:215-239) on this thread's entries, then the norms ------------------------------------------------
        s2 = 0.0;
        if (kact) {
            const double cqk = cq[lane], cpk = cp[lane], skk = sk[lane];
            for (int b = w; b < nblk; b += NW) {
#pragma unroll
                for (int jj = 0; jj < RB; ++jj) {
                    const int f = b * RB + jj;
                    if (f >= F) continue;                      // (the pad rows stay zero)
                    const size_t e = (size_t)f * RP + lane;
                    double x = Wm[e];
                    if (up) {
                        const double pe = KL ? skk : P[e];
                        const double dpw = fmax(pe + cqk * x, a.flr);
                        const double dmw = Q[e] + cpk * x;
                        x = x * dmw / dpw;
                        Wm[e] = x;
                    }
                    s2 += x * x;
                }
            }
        }
        stress_jitter();
        colsums(s2, 0.0, tmp, cp);                             // (cp: free until the next statistics)
        if (tid < RP) nrm[tid] = tid < Ra ? sqrt(tmp[tid]) : 1.0;
        __syncthreads();
        normalise();
    }
    // the result (normalised), column-major for the re-assembly, by the threads that own the entries
    if (kact)
        for (int b = w; b < nblk; b += NW)
#pragma unroll
            for (int jj = 0; jj < RB; ++jj) {
                const int f = b * RB + jj;
                if (f < F) Wu[(size_t)lane * F + f] = Wm[(size_t)f * RP + lane];
            }
    if (tid == 0) a.iters[(size_t)a.step * a.S + s] = stopped ? n_rec : max_iter;
}

// the re-assembly of every stream whose adaptation ran (oassemble_cols, snmf_online_batch_common.h): the fixed columns are
// the dictionary each stream started with, [S][Rd][F]; grid (Rd, S)
__global__ __launch_bounds__(256) void k_obassemble64(const OnlineStatus* status, const int* nfr, int step, int S, const double* B,
                                                      const double* Wu, const double* Bfix, const uint8_t* rupa, int F, int r, int Rx,
                                                      int Ra, int Rd, double* Btmp) {
    oassemble_cols(status, nfr, step, S, B, Wu, Bfix, (int64_t)Rd * F, rupa, F, r, Rx, Ra, Rd, Btmp);
}

struct ORefresh64Args {
    const OnlineStatus* status;  // NULL: every listed stream, every column (restart)
    const int* nfr;
    const int* slots;            // status == NULL: stream slots[blockIdx.y]; else stream blockIdx.y
    int step, S;
    const double* Btmp;          // [S][Rd][F] (status != NULL: the re-assembled noise columns, copied into B)
    double* B;                   // [S][r][F]
    double *Wn, *WnT, *wn, *csum;  // [S][r][F], [S][F][r], [S][r], [S][r]
    int F, r, Rx, k0;            // columns k0 + blockIdx.x
};

// The next frame solve's images of the dictionary (wnorm64_col, as k_wnorm64) per stream, gated on "this stream's dictionary
// changed".  One workgroup (256 threads) per (column, stream).
__global__ __launch_bounds__(256) void k_obrefresh64(ORefresh64Args a) {
    __shared__ double red[4];
    const int s = a.status ? (int)blockIdx.y : a.slots[blockIdx.y], k = a.k0 + blockIdx.x;
    if (k >= a.r) return;
    if (a.status && !ob_due(a.status, a.nfr, a.step, a.S, s)) return;
    const size_t img = (size_t)a.F * a.r;
    double* col = a.B + (size_t)s * img + (size_t)k * a.F;
    const double* src = a.status ? a.Btmp + ((size_t)s * (a.r - a.Rx) + (k - a.Rx)) * a.F : col;
    wnorm64_col(src, a.status ? col : nullptr, a.F, a.r, k, a.Wn + (size_t)s * img, a.WnT + (size_t)s * img, a.wn + (size_t)s * a.r,
                a.csum + (size_t)s * a.r, red);
}

// k_obrestart64: the restart of the listed streams (orestart_common, snmf_online_batch_common.h; grid (listed stream,
// kRsShared, kRsParts)): every stream from its own event dictionary, its Ad_blk by its own adapt_train_N.  k_obrefresh64
// (slot list form) follows.
__global__ __launch_bounds__(256) void k_obrestart64(ORestartCommon<double> a, const OStreamSettings* __restrict__ set) {
    orestart_common(a, blockIdx.y, set[a.slots[blockIdx.x]].adapt_train_N != 0);
}

// The listed streams' state g into (k_obstate_get64) / out of (k_obstate_put64) a slab of records (ostate_xfer,
// snmf_online_batch_common.h); grid (listed stream, kStN, kStParts).  k_obrefresh64 (slot list form) follows a put.
__global__ __launch_bounds__(256) void k_obstate_get64(OStateArgs<double> a) { ostate_xfer<double, false>(a); }
__global__ __launch_bounds__(256) void k_obstate_put64(OStateArgs<double> a) { ostate_xfer<double, true>(a); }

}  // namespace snmf
