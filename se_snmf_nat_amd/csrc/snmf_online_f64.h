// snmf_online_f64.h -- the kernels of the fp64 mode of the single-stream online separator (snmf_online_create_f64,
// include/snmf.h).
// The online loop is a feedback system (activations -> adapted noise dictionary -> next activations) that amplifies a
// perturbation about tenfold per 100 frames (docs/WIDENING.md, "Parity horizon"): a path that carries fp32-sized errors
// leaves the fp64 reference's trajectory after a few hundred frames.  Here every step from PCM to the fed-back state is
// double: the transforms, the frame solve, the post-filter state, the adaptation solve, the synthesis.  No float sits on
// that path; float appears only in the diagnostic fields of the 32-byte status.
//
// The transforms, the post-filter, the ring preparation, the re-assembly and the overlap-add are the double instantiations
// of the per-frame steps in snmf_online_common.h (same launch structure as the fp32 kernels of snmf_online.h).  The frame
// solve is this mode's own: an fp64 dictionary of 513 x 200 (820 KB) fits neither a CU's LDS nor its registers, so k_hsolve64
// streams the L2-resident normalised dictionary -- and a transposed image of it -- through the two matrix-vector products
// of an iteration, with every vector in LDS.
//
// Host side (snmf_tu_online_f64.hip): an OnlineF64 object behind the snmf_online handle (snmf_online_f64_host.h).
// Included by snmf_tu_online_f64.hip only.
#pragma once
#include "snmf_online_common.h"
#include "snmf_online_batch_common.h"  // ostate_xfer: the state record's gather / scatter
#include "snmf_online_f64_core.h"

namespace snmf {

// src/bnmf_sep_event_RT_IS16.m:65-81.  fp64 transforms keep their two buffers in dynamic LDS = 2 N double2 behind
// ensure_dyn_lds (deliberate: 128 KB at N = 4096 cannot be static)
template <int LOGN>
__global__ __launch_bounds__(256) void k_ostft64(OStftArgsT<double> a) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __attribute__((aligned(16))) double2 fbuf[];
    const int t = blockIdx.x;
    if (t >= a.n_frames) return;
    ostft_frame<LOGN, double>(a, a.sig + (int64_t)t * a.hop, a.Ym + (int64_t)t * a.ld, a.Yph + (int64_t)t * a.ld, fbuf, fbuf + N);
}

// ---- dictionary images of the frame solve ---------------------------------------------------------------------------
// wnorm64_col (snmf_online_f64_core.h) for [B_DFT_x | B_DFT_d].  One workgroup per column; launched at creation and after
// every adaptation.
__global__ __launch_bounds__(256) void k_wnorm64(const double* __restrict__ B, int F, int r, double* __restrict__ Wn,
                                                 double* __restrict__ WnT, double* __restrict__ wn, double* __restrict__ csum) {
    __shared__ double red[4];
    const int k = blockIdx.x;
    if (k >= r) return;
    wnorm64_col(B + (size_t)k * F, nullptr, F, r, k, Wn, WnT, wn, csum, red);
}

// The frame solve (hsolve64_frame, snmf_online_f64_core.h), one workgroup of 16 waves per frame.  Dynamic LDS =
// (4 F + 3 r + 32) doubles.
__global__ __launch_bounds__(1024) void k_hsolve64(HSolve64Args a) {
    extern __shared__ __attribute__((aligned(16))) double sm64[];
    const int fr = blockIdx.x;
    if (fr >= a.n) return;
    hsolve64_frame(a, fr, sm64);
}

// ---- post-filter -----------------------------------------------------------------------------------------------------
// One workgroup; dynamic LDS = (r + 6 F) doubles.  Walks the n frames of a launch in order, as k_opost does.
__global__ __launch_bounds__(1024) void k_opost64(OPostArgsT<double> a0) {
    extern __shared__ __attribute__((aligned(16))) double sm64[];
    __shared__ double red[16];
    for (int i = 0; i < a0.n; ++i) {
        OPostArgsT<double> a = a0;
        a.A += (size_t)i * a0.a_stride;
        a.recon += (size_t)i * 2 * a0.recon_len;
        a.hst += i;
        a.Ym += (size_t)i * a0.F;
        a.Xt_out += (size_t)i * a0.F;
        if (a.Xh_out) a.Xh_out += (size_t)i * a0.F;
        if (a.Dh_out) a.Dh_out += (size_t)i * a0.F;
        a.status += i;
        a.l += i;
        opost_frame<double>(a, sm64, red);
        __threadfence_block();  // (deliberate: this kernel has it, k_opost and k_obpost do not)
        __syncthreads();  // state written by this frame (global + LDS scratch) is visible to the next
    }
}

// ---- adaptation ------------------------------------------------------------------------------------------------------
// The inputs of the adaptation solve (oprep_elem)
__global__ void k_oprep64(const double* __restrict__ ldblk, const double* __restrict__ adblk, const uint8_t* __restrict__ rup,
                          const OnlineDev* dev, int F, int Ra, int ma, double* __restrict__ Vad, double* __restrict__ Had,
                          uint8_t* __restrict__ w_ind) {
    const int oldest = dev->n_push % ma;
    const size_t n = (size_t)F * ma + (size_t)Ra * ma + Ra;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        oprep_elem<double>(i, oldest, ldblk, adblk, rup, F, Ra, ma, Vad, Had, w_ind);
}

// The re-assembly of :336 (oassemble_col); this separator keeps no fp32 mirror.  One workgroup per column.
__global__ void k_oassemble64(const double* __restrict__ Bd_old, const double* __restrict__ Wc, int Fp,
                              const double* __restrict__ Bfix, const uint8_t* __restrict__ rup, int F, int Ra, int Rd,
                              double* __restrict__ Bd_new) {
    const int j = blockIdx.x;
    if (j >= Rd) return;
    const double* src;
    if (j >= Ra) {
        src = Bfix + (size_t)j * F;
    } else {
        bool retrained;
        const int k = oassemble_col(rup, Ra, j, &retrained);
        src = retrained ? Wc + (size_t)k * Fp : Bd_old + (size_t)k * F;
    }
    for (int f = threadIdx.x; f < F; f += blockDim.x) Bd_new[(size_t)j * F + f] = src[f];
}

struct WAdapt64Args {
    const double* V;       // [ma][F]  lambda_d_blk in time order
    const double* H;       // [ma][Ra] Ad_blk in time order, rows not in r_up zeroed
    const double* W0;      // [Ra][F]  init_w (first R_a columns of B_DFT_d)
    const uint8_t* w_ind;  // [Ra]     r_up
    double* Wout;          // [Ra][F]  result
    double* part1;         // [nwg][2 RP + 1]  colsum(Q.*W) | colsum(P.*W) | divergence partials
    double* part2;         // [nwg][RP]        squared-norm partials
    int* n_iter_out;
    unsigned* bar;         // grid-barrier counter, zero at launch
    int F, Ra, ma, max_iter, cost_check;
    double beta, sparsity, flr, conv_eps;
};

constexpr int kWa64RB = 8, kWa64RP = 64, kWa64LPR = 32, kWa64NT = kWa64RB * kWa64LPR;
// doubles of dynamic LDS
__host__ __device__ constexpr size_t wadapt64_lds_doubles(int Ra, int ma) {
    return (size_t)kWa64RB * kWa64RP * 3 + 2 * kWa64RP + 32 + 256 + 2 * kWa64RP + kWa64RP + 3 * (size_t)kWa64RB * ma + (size_t)Ra * ma +
           (size_t)ma * (kWa64RP + 1) + kWa64RP;
}

// The whole W-only adaptation solve (src/bnmf_sep_event_RT_IS16.m:330-335 -> src/sparse_nmf.m:157-286 with h_update_ind all
// false) in ONE cooperative launch, every beta: k_wadapt's design in fp64.  V and H never change, so a workgroup keeps H
// (both orientations) and its 8 rows of V and W in LDS for the whole solve; an iteration is two small products per row
// block and two grid barriers (the column sums of the update, then the column norms), through k_wadapt's bounded-spin
// barrier and its sc1 exchanges.  The stop test runs identically in every workgroup on the same reduced numbers.
// With P = lam.^(beta-1) * h', Q = (v .* lam.^(beta-2)) * h' the update of :215-239 is, for every beta,
//   w .* (Q + colsum(P.*w) .* w) ./ max(P + colsum(Q.*w) .* w, flr)        (beta = 1: P = sum(h,2)', Q = (v./lam) * h').
// Grid = ceil(F / 8) workgroups of 256 threads.
__global__ __launch_bounds__(kWa64NT) void k_wadapt64(WAdapt64Args a) {
    constexpr int RB = kWa64RB, RP = kWa64RP, NT = kWa64NT, NWV = kWa64NT / 64, LPR = kWa64LPR;
    unsigned gen = 0;
    bool bar_ok = true;
    extern __shared__ __attribute__((aligned(16))) double sm64[];
    const int F = a.F, Ra = a.Ra, ma = a.ma, tid = threadIdx.x, nwg = gridDim.x, wg = blockIdx.x;
    const int f0 = wg * RB;
    double* Wd = sm64;                     // [RB][RP]
    double* Ps = Wd + RB * RP;             // [RB][RP]
    double* Qs = Ps + RB * RP;             // [RB][RP]
    double* cq = Qs + RB * RP;             // [2 RP] reduced column quantities
    double* red = cq + 2 * RP;             // [32] (the last one holds the grid barrier's verdict)
    int* oks = reinterpret_cast<int*>(red + 31);
    double* scr = red + 32;                // [2][128] cross_sum scratch
    double* tmp = scr + 256;               // [2 RP] reduced quantities of one exchange
    double* sk = tmp + 2 * RP;             // [RP] rowsum(H)
    double* Vs = sk + RP;                  // [RB][ma]
    double* As = Vs + RB * ma;             // [RB][ma] lam.^(beta-1)
    double* Bs = As + RB * ma;             // [RB][ma] v .* lam.^(beta-2)
    double* Hs = Bs + RB * ma;             // [Ra][ma]
    double* HT = Hs + Ra * ma;             // [ma][RP + 1]
    int* act = reinterpret_cast<int*>(HT + ma * (RP + 1));  // [1 + RP] number and list of the flagged columns
    const double beta = a.beta;
    const bool kl = beta == 1.0, ed = beta == 2.0;
    const int f = tid / LPR, l32 = tid % LPR;
    const bool row_ok = f0 + f < F;

    // ---- load + src/sparse_nmf.m:157-169 ----
    for (int i = tid; i < RB * RP; i += NT) {
        const int k = i / RB, ff = i - k * RB;
        Wd[ff * RP + k] = (k < Ra && f0 + ff < F) ? a.W0[(size_t)k * F + f0 + ff] : 0.0;
    }
    for (int i = tid; i < RB * ma; i += NT) {
        const int t = i / RB, ff = i - t * RB;
        Vs[ff * ma + t] = (f0 + ff < F) ? fmax(a.V[(size_t)t * F + f0 + ff], a.flr) : 0.0;   // :169
    }
    for (int i = tid; i < Ra * ma; i += NT) {
        const int t = i / Ra, k = i - t * Ra;
        Hs[k * ma + t] = a.H[i];
    }
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < Ra; ++k)
            if (a.w_ind[k]) act[1 + n++] = k;
        act[0] = n;
    }
    __syncthreads();
    const int nact = act[0];
    if (tid < RP) {
        double s2 = 0.0;
        for (int ff = 0; ff < RB; ++ff) {
            const double w = Wd[ff * RP + tid];
            s2 += w * w;
        }
        xstore(a.part2 + (size_t)wg * RP + tid, s2);
    }
    bar_ok &= grid_bar(a.bar, (unsigned)nwg, gen, oks);
    cross_sum(a.part2, RP, RP, nwg, scr, tmp);
    if (tid < RP) cq[tid] = tid < Ra ? sqrt(tmp[tid]) : 1.0;  // wn
    __syncthreads();
    for (int i = tid; i < RB * RP; i += NT) {
        const int k = i % RP;
        Wd[i] = k < Ra ? Wd[i] / cq[k] : 0.0;                 // w = w ./ wn
    }
    for (int i = tid; i < Ra * ma; i += NT) Hs[i] = Hs[i] * cq[i / ma];   // h = h .* wn'  (:160)
    __syncthreads();
    for (int i = tid; i < ma * (RP + 1); i += NT) {
        const int t = i / (RP + 1), k = i - t * (RP + 1);
        HT[i] = k < Ra ? Hs[k * ma + t] : 0.0;
    }
    if (tid < RP) {
        double s = 0.0;
        if (tid < Ra)
            for (int t = 0; t < ma; ++t) s += Hs[tid * ma + t];
        sk[tid] = s;                                          // sum(h,2)
    }
    __syncthreads();
    double sh_const = 0.0;                                    // sum(sum(sparsity .* h)) (:261), constant: H is fixed
    for (int k = 0; k < Ra; ++k) sh_const += a.sparsity * sk[k];

    double last_cost = 0.0;
    int n_rec = 0;
    bool stopped = false;
    for (int j = 1; j <= a.max_iter + 1; ++j) {
        if (j > a.max_iter && !a.cost_check) break;
        // ---- Lam = max(w*h, flr) of iterate j-1, its divergence, the weights of the update ----
        double dterm = 0.0;
        for (int t = l32; t < ma; t += LPR) {
            double acc = 0.0;
            for (int q = 0; q < nact; ++q) {
                const int k = act[1 + q];
                acc = fma(Wd[f * RP + k], Hs[k * ma + t], acc);
            }
            const double lam = fmax(acc, a.flr), v = Vs[f * ma + t];
            double pa, pb;
            if (kl) {
                pa = 1.0;
                pb = v / lam;
            } else if (ed) {
                pa = lam;
                pb = v;
            } else {
                pa = pow(lam, beta - 1.0);
                pb = v * pow(lam, beta - 2.0);
            }
            As[f * ma + t] = row_ok ? pa : 0.0;
            Bs[f * ma + t] = row_ok ? pb : 0.0;
            if (row_ok) dterm += div_term_d(v, lam, beta);
        }
        __syncthreads();
        // ---- P = lam.^(beta-1) * h', Q = (v .* lam.^(beta-2)) * h' on this block's rows ----
        {
            double gp[2] = {0.0, 0.0}, gq[2] = {0.0, 0.0};
            const double* ar = As + f * ma;
            const double* br = Bs + f * ma;
            const double* hc = HT + l32;
            if (kl) {
                for (int t = 0; t < ma; ++t) {
                    const double b = br[t];
                    gq[0] = fma(b, hc[t * (RP + 1)], gq[0]);
                    gq[1] = fma(b, hc[t * (RP + 1) + LPR], gq[1]);
                }
                gp[0] = row_ok ? sk[l32] : 0.0;
                gp[1] = row_ok ? sk[l32 + LPR] : 0.0;
            } else {
                for (int t = 0; t < ma; ++t) {
                    const double av = ar[t], b = br[t], h0 = hc[t * (RP + 1)], h1 = hc[t * (RP + 1) + LPR];
                    gp[0] = fma(av, h0, gp[0]);
                    gp[1] = fma(av, h1, gp[1]);
                    gq[0] = fma(b, h0, gq[0]);
                    gq[1] = fma(b, h1, gq[1]);
                }
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int k = l32 + LPR * c;
                Ps[f * RP + k] = k < Ra ? gp[c] : 0.0;
                Qs[f * RP + k] = k < Ra ? gq[c] : 0.0;
            }
        }
        const double dw = wave_sum_d(dterm);
        if ((tid & 63) == 0) red[tid >> 6] = dw;
        __syncthreads();
        if (tid < 2 * RP) {
            const int k = tid & (RP - 1);
            const double* src = tid < RP ? Qs : Ps;
            double s = 0.0;
            for (int ff = 0; ff < RB; ++ff) s += src[ff * RP + k] * Wd[ff * RP + k];
            xstore(a.part1 + (size_t)wg * (2 * RP + 1) + tid, s);   // colsum(Q .* w) | colsum(P .* w) partials
        }
        if (tid == 2 * RP) {
            double dsum = 0.0;
#pragma unroll
            for (int q = 0; q < NWV; ++q) dsum += red[q];
            xstore(a.part1 + (size_t)wg * (2 * RP + 1) + 2 * RP, dsum);
        }
        bar_ok &= grid_bar(a.bar, (unsigned)nwg, gen, oks);
        const double dpart = tid < nwg ? xload(a.part1 + (size_t)tid * (2 * RP + 1) + 2 * RP) : 0.0;
        cross_sum(a.part1, 2 * RP + 1, 2 * RP, nwg, scr, tmp);
        const double div = div_scale_d(block_sum_d(dpart, red), beta);   // fixed order: the same number in every workgroup
        if (tid < 2 * RP) cq[tid] = tmp[tid];
        __syncthreads();
        if (a.cost_check && j > 1) {                          // cost of iterate j-1 (:260-284)
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
        // ---- W update (:215-239) on this block's rows, then the norms ----
        for (int i = tid; i < RB * RP; i += NT) {
            const int k = i % RP;
            double wv = Wd[i];
            if (k < Ra && a.w_ind[k]) {
                const double dpw = fmax(Ps[i] + cq[k] * wv, a.flr);
                const double dmw = Qs[i] + cq[RP + k] * wv;
                wv = wv * dmw / dpw;
            }
            Wd[i] = wv;
        }
        __syncthreads();
        if (tid < RP) {
            double s2 = 0.0;
            for (int ff = 0; ff < RB; ++ff) {
                const double w = Wd[ff * RP + tid];
                s2 += w * w;
            }
            xstore(a.part2 + (size_t)wg * RP + tid, s2);
        }
        bar_ok &= grid_bar(a.bar, (unsigned)nwg, gen, oks);
        cross_sum(a.part2, RP, RP, nwg, scr, tmp);
        if (tid < RP) cq[tid] = tid < Ra ? sqrt(tmp[tid]) : 1.0;
        __syncthreads();
        for (int i = tid; i < RB * RP; i += NT) {
            const int k = i % RP;
            Wd[i] = k < Ra ? Wd[i] / cq[k] : 0.0;             // :242, ALL columns
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < RB * RP; i += NT) {
        const int k = i / RB, ff = i - k * RB;
        if (k < Ra && f0 + ff < F) a.Wout[(size_t)k * F + f0 + ff] = Wd[ff * RP + k];
    }
    if (wg == 0 && tid == 0) *a.n_iter_out = !bar_ok ? -1 : (stopped ? n_rec : a.max_iter);
}

// ---- per-class reconstructions ---------------------------------------------------------------------------------------
// k_oclass of snmf_online.h on the fp64 dictionary (DFT mode; this separator has no Mel mode): Xm_hat(c) = B(:, R_c) * A(R_c)
// (src/bnmf_sep_event_RT_IS16.m:158-202) of frame i = blockIdx.y into out + c*cstride + i*F.  Grid (ceil(F / 256), n frames).
__global__ __launch_bounds__(256) void k_oclass64(const double* __restrict__ B, const double* __restrict__ A, int a_stride,
                                                  const int* __restrict__ cls, int n_cls, int F, int n, double* __restrict__ out,
                                                  int64_t cstride) {
    const int i = blockIdx.y;
    if (i >= n) return;
    oclass_dft<double, double, double>(B, A + (size_t)i * a_stride, cls, n_cls, F, out + (size_t)i * F, cstride);
}

// ---- synthesis -------------------------------------------------------------------------------------------------------
// src/synth_ifft_buff.m:10-28 (+ the overlapscale of src/bnmf_sep_event_RT_IS16.m:363); dynamic LDS = 2 N double2
template <int LOGN>
__global__ __launch_bounds__(256) void k_oistft64(OIstftArgsT<double> a) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __attribute__((aligned(16))) double2 fbuf[];
    const int t = blockIdx.x;
    if (t >= a.n_frames) return;
    oistft_frame<LOGN, double>(a, a.mag + (int64_t)t * a.ld, a.ph + (int64_t)t * a.ld, a.syn + (int64_t)t * a.sz, fbuf, fbuf + N);
}

// Overlap-add (oola_sample); the int16 stream is the fp64 value rounded
__global__ void k_oola64(const double* __restrict__ syn, int n_new, int l0, int delay, int sz, int hop, int nov, int i_first,
                         int n_out, double* __restrict__ outf, int16_t* __restrict__ out16) {
    const size_t n = (size_t)n_out * hop;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / hop), s = (int)(e - (size_t)j * hop);
        oola_sample<double>(syn, i_first + j, s, l0, delay, sz, hop, nov, outf, out16, e);  // global frame l = l0 + i_first + j
    }
}

// The separator's state g into (k_ostate_get64) / out of (k_ostate_put64) one staging record: the batched separator's
// ostate_xfer on the single-stream arrays (S = 1, slot list {0}), as k_ostate_get / _put in snmf_online.h.
__global__ __launch_bounds__(256) void k_ostate_get64(OStateArgs<double> a, int64_t l) {
    const int slot0 = 0;
    const int64_t l0 = l;
    a.slots = &slot0;
    a.l = &l0;
    ostate_xfer<double, false>(a);
}
__global__ __launch_bounds__(256) void k_ostate_put64(OStateArgs<double> a) {
    const int slot0 = 0;
    a.slots = &slot0;
    a.l = nullptr;
    ostate_xfer<double, true>(a);
}

}  // namespace snmf
