// snmf_online.h -- the kernels of the fp32 single-stream online separator (BASELINE config 3), kept on
// the device.  Reference (shipped configuration: blk_len_sep = 1, Splice = 0): src/bnmf_sep_event_RT_IS16.m,
// src/blk_sparse.m, src/synth_ifft_buff.m, src/NTF_sep_event_RT.m:104-124 -- the per-frame arithmetic itself is in
// snmf_online_common.h, shared with the fp64 mode and the batched separator; the kernels here own the indexing and the LDS.
// Everything is vector work on F ~ 513 bins per frame: latency-bound, one workgroup per
// frame for the transforms and ONE workgroup for the sequential post-solve step.  The solves
// themselves are the engine's kernels (k_hsolve_small for the frame, k_wstats/k_wapply for the
// adaptation).  Included by snmf_tu_online.hip only.
#pragma once
#include "snmf_online_common.h"
#include "snmf_online_batch_common.h"  // ostate_xfer: the state record's gather / scatter

namespace snmf {

// fp32 transforms keep their two buffers in static LDS (deliberate: 64 KB at N = 4096 fits; the fp64 ones cannot)
template <int LOGN>
__global__ __launch_bounds__(256) void k_ostft(OStftArgs a) {
    constexpr int N = 1 << LOGN;
    __shared__ float2 bufA[N];
    __shared__ float2 bufB[N];
    const int t = blockIdx.x;
    if (t >= a.n_frames) return;
    ostft_frame<LOGN, float>(a, a.sig + (int64_t)t * a.hop, a.Ym + (int64_t)t * a.ld, a.Yph + (int64_t)t * a.ld, bufA, bufB);
}

// One workgroup; dynamic LDS = (r + 7*F + 3*n1) floats.  The post-filter recurrences (smoothed noise PSD, the
// previous frame's G.*Y, the SNR ring) make the frames sequential, but when the dictionary is fixed
// (no adaptation) nothing the host must decide sits between them: the frame solves of a whole batch run
// in parallel first and this kernel then walks the batch in ONE launch.
__global__ __launch_bounds__(1024) void k_opost(OPostArgs a0) {
    extern __shared__ float sm[];
    __shared__ double red[16];
    for (int i = 0; i < a0.n; ++i) {
        OPostArgs a = a0;
        a.A += (size_t)i * a0.a_stride;
        if (a.recon) a.recon += (size_t)i * 2 * a0.recon_len;
        if (a.Ymel) a.Ymel += (size_t)i * a0.n1;
        a.hst += i;
        a.Ym += (size_t)i * a0.F;
        a.Xt_out += (size_t)i * a0.F;
        if (a.Xh_out) a.Xh_out += (size_t)i * a0.F;
        if (a.Dh_out) a.Dh_out += (size_t)i * a0.F;
        a.status += i;
        a.l += i;
        opost_frame<float>(a, sm, red);
        __syncthreads();  // state written by this frame (global + LDS scratch) is visible to the next
    }
}

// The inputs of the adaptation solve (oprep_elem)
__global__ void k_oprep(const float* __restrict__ ldblk, const float* __restrict__ adblk, const uint8_t* __restrict__ rup,
                        const OnlineDev* dev, int F, int Ra, int ma, float* __restrict__ Vad, float* __restrict__ Had,
                        uint8_t* __restrict__ w_ind) {
    const int oldest = dev->n_push % ma;
    const size_t n = (size_t)F * ma + (size_t)Ra * ma + Ra;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        oprep_elem<float>(i, oldest, ldblk, adblk, rup, F, Ra, ma, Vad, Had, w_ind);
}

// :106-120 for a batch of frames (omel_features).  One workgroup per frame.
__global__ __launch_bounds__(256) void k_omel_frame(const float* __restrict__ Ym, const float* __restrict__ melmat, int F, int n1,
                                                    int n_frames, float* __restrict__ Ymel) {
    extern __shared__ float sm[];  // [n1] + 2
    __shared__ float part[4];
    const int t = blockIdx.x;
    if (t >= n_frames) return;
    omel_features(Ym + (size_t)t * F, melmat, F, n1, sm, part, [&](int m, float v) { Ymel[(size_t)t * n1 + m] = v; });
}

// Mel-mode inputs of the adaptation solve (:298-313): lambda_d_blk_Mel = melmat * lambda_d_blk in time order,
// Ad_blk rows masked by r_up, the update mask.  One workgroup per ring column.
__global__ __launch_bounds__(256) void k_oprep_mel(const float* __restrict__ ldblk, const float* __restrict__ adblk,
                                                   const uint8_t* __restrict__ rup, const OnlineDev* dev,
                                                   const float* __restrict__ melmat, int F, int n1, int Ra, int ma,
                                                   float* __restrict__ Vad, float* __restrict__ Had, uint8_t* __restrict__ w_ind) {
    const int c = blockIdx.x, tid = threadIdx.x;
    const int oldest = dev->n_push % ma;
    omel_project(ldblk + (size_t)((oldest + c) % ma) * F, melmat, F, n1, Vad + (size_t)c * n1);
    for (int k = tid; k < Ra; k += 256) {
        Had[(size_t)c * Ra + k] = rup[k] ? adblk[(size_t)((oldest + c) % ma) * Ra + k] : 0.f;
        if (c == 0) w_ind[k] = rup[k];
    }
}

// The re-assembly of :336 (oassemble_col) into the fp64 master and its fp32 mirror.  One workgroup per column.
__global__ void k_oassemble(const double* __restrict__ Bd_old, const double* __restrict__ Wc, int Fp,
                            const double* __restrict__ Bfix, const uint8_t* __restrict__ rup, int F, int Ra, int Rd,
                            double* __restrict__ Bd_new, float* __restrict__ Bd_f32) {
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
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        const double v = src[f];
        Bd_new[(size_t)j * F + f] = v;
        Bd_f32[(size_t)j * F + f] = (float)v;
    }
}

template <int LOGN>
__global__ __launch_bounds__(256) void k_oistft(OIstftArgs a) {
    constexpr int N = 1 << LOGN;
    __shared__ float2 bufA[N];
    __shared__ float2 bufB[N];
    const int t = blockIdx.x;
    if (t >= a.n_frames) return;
    oistft_frame<LOGN, float>(a, a.mag + (int64_t)t * a.ld, a.ph + (int64_t)t * a.ld, a.syn + (int64_t)t * a.sz, bufA, bufB);
}

// Overlap-add and int16 output (oola_sample) of the n_out hops from new frame i_first on
__global__ void k_oola(const float* __restrict__ syn, int n_new, int l0, int delay, int sz, int hop, int nov, int i_first,
                       int n_out, float* __restrict__ outf, int16_t* __restrict__ out16) {
    const size_t n = (size_t)n_out * hop;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / hop), s = (int)(e - (size_t)j * hop);
        oola_sample<float>(syn, i_first + j, s, l0, delay, sz, hop, nov, outf, out16, e);  // global frame l = l0 + i_first + j
    }
}

// k_oistft over a class-major stack (snmf_online_set_classes): class c's frame t at mag + c*mag_cstride + t*ld, every class
// with the frame's phase, into syn + c*syn_cstride + t*sz.  Grid (n_frames, classes): ONE launch for all class signals.
template <int LOGN>
__global__ __launch_bounds__(256) void k_oistft_cls(OIstftArgs a, int64_t mag_cstride, int64_t syn_cstride) {
    constexpr int N = 1 << LOGN;
    __shared__ float2 bufA[N];
    __shared__ float2 bufB[N];
    const int t = blockIdx.x, c = blockIdx.y;
    if (t >= a.n_frames) return;
    oistft_frame<LOGN, float>(a, a.mag + (int64_t)c * mag_cstride + (int64_t)t * a.ld, a.ph + (int64_t)t * a.ld,
                       a.syn + (int64_t)c * syn_cstride + (int64_t)t * a.sz, bufA, bufB);
}

struct OClassArgs {
    const float* B;       // [r][F] fp32 [B_DFT_x | B_DFT_d] (Bf); MelConv = 1: [r][n1] [B_Mel_x | B_Mel_d] (Bmf)
    const float* A;       // activations of frame i at A + i*a_stride
    const int* cls;       // [n_cls + 1] column ranges
    const float* melmat;  // [n1][F] (MelConv = 1)
    float* out;           // class c, frame i at out + c*cstride + i*F
    int64_t cstride;
    int n_cls, F, n1, mel_conv, n, a_stride;
};

// Grid (ceil(F / 256), n frames): one launch per frame step, or one for the n frames of a fixed-dictionary batch.
// Dynamic LDS: n_cls * n1 floats with MelConv = 1, none otherwise.
__global__ __launch_bounds__(256) void k_oclass(OClassArgs a) {
    extern __shared__ float sm[];
    const int i = blockIdx.y;
    if (i >= a.n) return;
    const float* A = a.A + (size_t)i * a.a_stride;
    float* out = a.out + (size_t)i * a.F;
    if (a.mel_conv) oclass_mel<float>(a.B, A, a.cls, a.n_cls, a.n1, a.melmat, a.F, out, a.cstride, sm);
    else oclass_dft<float, float, float>(a.B, A, a.cls, a.n_cls, a.F, out, a.cstride);
}

// ---------------------------------------------------------------------------------------------
// k_wadapt: the whole W-only adaptation solve (src/bnmf_sep_event_RT_IS16.m:330-335 ->
// src/sparse_nmf.m:157-286 with h_update_ind all false, KL) in ONE cooperative launch.
// The problem is tiny (513 x 100, rank <= 64) and the generic path costs three launches per
// iteration (~30 us); here V and H never change, so every workgroup keeps H (both orientations) and its
// RB = 8 rows of V and W in LDS for the whole solve and an iteration is two small products per row block
// plus two grid barriers for the column sums (colsum(G.*W), then the column norms).  The convergence
// test runs identically in every workgroup on the same reduced numbers.  Master copy of W in fp64
// (see k_wapply).  Grid = ceil(F / 8) workgroups of 256 threads, launched cooperatively.
// ---------------------------------------------------------------------------------------------

struct WAdaptArgs {
    const float* V;        // [ma][F]  lambda_d_blk in time order
    const float* H;        // [ma][Ra] Ad_blk in time order, rows not in r_up zeroed
    const double* W0;      // [Ra][F]  init_w (first R_a columns of B_DFT_d)
    const uint8_t* w_ind;  // [Ra]     r_up
    double* Wout;          // [Ra][F]  result
    double* part1;         // [nwg][RP + 1]  colsum(G.*W) partials + divergence partial
    double* part2;         // [nwg][2][RP]   squared-norm and column-sum partials
    double* costh;         // [max_iter]
    int* n_iter_out;
    unsigned* bar;         // grid-barrier counter, zero at launch
    int F, Ra, ma, max_iter, cost_check;
    float sparsity, flr;
    double conv_eps;
};

constexpr int kWaRB = 8, kWaRP = 64;    // rows of W per workgroup (32 threads each), padded rank (32 rows x 1024 threads: 2261 instead of 2743 frames/s)
constexpr int kWaLPR = 32;                // threads per row of W (64 -- a wave per row, eight waves per workgroup -- made the products no
                                          // faster and both exchanges slower: 3434 against 3620 frames/s)
constexpr int kWaNT = kWaRB * kWaLPR;     // threads per workgroup

#ifdef SNMF_PROF_WA  // diagnostic builds only: cycles of workgroup 0 by phase, summed over the solves of a run
__device__ unsigned long long g_wa_prof[10];
#define WA_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    atomicAdd(&g_wa_prof[i], t_ - wa_t_); wa_t_ = t_; } } while (0)
#else
#define WA_STAMP(i)
#endif
__global__ __launch_bounds__(kWaNT) void k_wadapt(WAdaptArgs a) {
#ifdef SNMF_PROF_WA
    unsigned long long wa_t_ = __builtin_amdgcn_s_memtime();
#endif
    constexpr int RB = kWaRB, RP = kWaRP, NT = kWaNT, NWV = kWaNT / 64;
    unsigned gen = 0;
    bool bar_ok = true;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int F = a.F, Ra = a.Ra, ma = a.ma, tid = threadIdx.x, nwg = gridDim.x, wg = blockIdx.x;
    const int f0 = wg * RB;
    double* Wd = reinterpret_cast<double*>(sm);          // [RB][RP]
    double* cq = Wd + RB * RP;                            // [RP] reduced column quantities
    double* cs = cq + RP;                                 // [RP] colsum(W)
    double* red = cs + RP;                                // [NWV + 1] (padded to 32)
    int* oks = reinterpret_cast<int*>(red + 31);          // the grid barrier's verdict (red is padded to 32 doubles)
    double* scr = red + 32;                               // [2][128] cross_sum scratch
    double* tmp = scr + 256;                              // [2*RP] reduced quantities of one exchange
    float* Wf = reinterpret_cast<float*>(tmp + 2 * RP);   // [RB][RP]
    float* Gs = Wf + RB * RP;                             // [RB][RP]
    float* sk = Gs + RB * RP;                             // [RP] rowsum(H)
    float* Vs = sk + RP;                                  // [RB][ma]
    float* Rs = Vs + RB * ma;                             // [RB][ma]
    float* Hs = Rs + RB * ma;                             // [Ra][ma]
    float* HT = Hs + Ra * ma;                             // [ma][RP + 1]
    // the operand images of the two products: what ONE lane needs for one k (its four frames l, l + 32, l + 64, l + 96) resp.
    // one frame (its two columns l, l + 32) side by side, so that it is ONE wide read instead of four / two (ma <= 128)
    float* Hp = HT + ma * (RP + 1);                       // [Ra][128]: Hp[k][4 l + j] = h[k][l + 32 j]  (0 past ma)
    float* HTp = Hp + Ra * 128;                           // [ma][RP]:  HTp[t][2 l + c] = h[l + 32 c][t] (0 past Ra)
    static_assert(kWaLPR == 32 && RP == 64, "operand images of k_wadapt's products");
    const bool wide = a.ma <= 128 && (a.ma & 3) == 0;    // (16-byte reads of rows of ma floats)
    const int f = tid / kWaLPR, l32 = tid % kWaLPR;       // row of the block, lane within the row's threads
    static_assert(RP % kWaLPR == 0 && 128 % kWaLPR == 0, "whole columns of G / frames per lane");
    const bool row_ok = f0 + f < F;

    // ---- load + src/sparse_nmf.m:157-169 ------------------------------------------------------
    // (consecutive threads take consecutive ROWS of one column / frame: the block's 8 rows are one 64- / 32-byte piece of memory)
    for (int i = tid; i < RB * RP; i += NT) {
        const int k = i / RB, ff = i - k * RB;
        Wd[ff * RP + k] = (k < Ra && f0 + ff < F) ? a.W0[(size_t)k * F + f0 + ff] : 0.0;
    }
    for (int i = tid; i < RB * ma; i += NT) {
        const int t = i / RB, ff = i - t * RB;
        Vs[ff * ma + t] = (f0 + ff < F) ? fmaxf(a.V[(size_t)t * F + f0 + ff], a.flr) : 0.f;   // :169
    }
    for (int i = tid; i < Ra * ma; i += NT) {
        const int t = i / Ra, k = i - t * Ra;
        Hs[k * ma + t] = a.H[i];
    }
    __syncthreads();
    // wn = sqrt(sum(w.^2)) and colsum(w): partials over this block's rows, ONE exchange (the column sums of the normalised
    // W are colsum(w) ./ wn, as after every update below)
    if (tid < RP) {
        double s2 = 0.0, s1 = 0.0;
        for (int ff = 0; ff < RB; ++ff) {
            const double w = Wd[ff * RP + tid];
            s2 += w * w;
            s1 += w;
        }
        xstore(a.part2 + (size_t)wg * 2 * RP + tid, s2);
        xstore(a.part2 + (size_t)wg * 2 * RP + RP + tid, s1);
    }
    bar_ok &= grid_bar(a.bar, (unsigned)nwg, gen, oks);
    cross_sum(a.part2, 2 * RP, 2 * RP, nwg, scr, tmp);
    if (tid < RP) {
        cq[tid] = tid < Ra ? sqrt(tmp[tid]) : 1.0;  // wn
        cs[tid] = tmp[RP + tid] / cq[tid];
    }
    __syncthreads();
    for (int i = tid; i < RB * RP; i += NT) {
        const int k = i % RP;
        const double w = k < Ra ? Wd[i] / cq[k] : 0.0;   // w = w ./ wn
        Wd[i] = w;
        Wf[i] = (float)w;
    }
    for (int i = tid; i < Ra * ma; i += NT) {
        const int k = i / ma;
        Hs[i] = (float)((double)Hs[i] * cq[k]);          // h = h .* wn'  (:160)
    }
    __syncthreads();
    for (int i = tid; i < ma * (RP + 1); i += NT) {
        const int t = i / (RP + 1), k = i - t * (RP + 1);
        HT[i] = k < Ra ? Hs[k * ma + t] : 0.f;
    }
    if (wide) {
        for (int i = tid; i < Ra * 128; i += NT) {
            const int k = i >> 7, l = (i & 127) >> 2, j = i & 3, t = l + 32 * j;
            Hp[i] = t < ma ? Hs[k * ma + t] : 0.f;
        }
        for (int i = tid; i < ma * RP; i += NT) {
            const int t = i / RP, l = (i % RP) >> 1, c = i & 1, k = l + 32 * c;
            HTp[i] = k < Ra ? Hs[k * ma + t] : 0.f;
        }
    }
    if (tid < RP) {
        float s = 0.f;
        if (tid < Ra)
            for (int t = 0; t < ma; ++t) s += Hs[tid * ma + t];
        sk[tid] = s;                                     // sum(h,2)
    }
    __syncthreads();
    double sh_const = 0.0;                               // sum(sum(sparsity .* h)) (:261), constant: H is fixed
    for (int k = 0; k < Ra; ++k) sh_const += (double)a.sparsity * (double)sk[k];
    WA_STAMP(0);

    double last_cost = 0.0;
    int n_rec = 0;
    bool stopped = false;
    for (int j = 1; j <= a.max_iter + 1; ++j) {
        if (j > a.max_iter && !a.cost_check) break;
        // ---- Lam' = max(W*H, flr), ratio, divergence of iterate j-1 ------------------------------
        // Both products keep the summation order of the plain loops (one fma chain per output element, k resp. t ascending), but
        // as written before -- one output at a time, its LDS operands read inside the chain, the result stored into the same
        // LDS array the next chain reads from -- every fma waited for an LDS round trip (18 k cycles per product on a wave that
        // has its SIMD to itself: 115 cycles per fma; phase stamps of the diagnostic build).  Here a thread's outputs (four
        // frames, two columns) advance together and nothing is stored inside the loops, so the reads pipeline.
        float dterm = 0.f;
        if (wide) {
            constexpr int NJ = 4;
            f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
            const float* wr = Wf + f * RP;        // (columns k >= Ra of Wf are zero)
            const float* hp = Hp + 4 * l32;
            // four k per step: one 16-byte read of the W row + four 16-byte reads of the lane's frames; the chains are the plain
            // loop's (per frame, k ascending; a padded k adds fma(0, h, acc) = acc)
            const int n4 = (Ra + 3) >> 2;
            for (int g = 0; g < n4; ++g) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + 4 * g);
                f32x4 h4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = 4 * g + u < Ra ? 4 * g + u : Ra - 1;  // (w = 0 there)
                    h4[u] = *reinterpret_cast<const f32x4*>(hp + k * 128);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) a4[jj] = fmaf(w4[u], h4[u][jj], a4[jj]);
            }
            float ac[NJ] = {a4[0], a4[1], a4[2], a4[3]};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int t = l32 + kWaLPR * j;
                if (t < ma) {
                    const float lam = fmaxf(ac[j], a.flr), v = Vs[f * ma + t];
                    Rs[f * ma + t] = row_ok ? v * fast_rcp(lam) : 0.f;
                    if (row_ok) dterm += div_term<BM_KL>(v, lam, 1.f, 0.f);
                }
            }
        } else {
            for (int t = l32; t < ma; t += kWaLPR) {
                float acc = 0.f;
                for (int k = 0; k < Ra; ++k) acc = fmaf(Wf[f * RP + k], Hs[k * ma + t], acc);
                const float lam = fmaxf(acc, a.flr), v = Vs[f * ma + t];
                Rs[f * ma + t] = row_ok ? v * fast_rcp(lam) : 0.f;
                if (row_ok) dterm += div_term<BM_KL>(v, lam, 1.f, 0.f);
            }
        }
        __syncthreads();
        WA_STAMP(1);
        // ---- G = (V./Lam') * H' -----------------------------------------------------------------
        {
            constexpr int NC = RP / kWaLPR;  // columns l32 + kWaLPR * c of this lane (HT's columns k >= Ra are zero)
            float g[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) g[c] = 0.f;
            const float* rr = Rs + f * ma;
            if (wide) {
                // four frames per step: one 16-byte read of the ratio row + four 8-byte reads of the lane's two columns
                typedef float f32x2 __attribute__((ext_vector_type(2)));
                const float* xp = HTp + 2 * l32;
                const int m4 = ma >> 2;
                for (int q = 0; q < m4; ++q) {
                    const f32x4 r4 = *reinterpret_cast<const f32x4*>(rr + 4 * q);
                    f32x2 x2[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x2[u] = *reinterpret_cast<const f32x2*>(xp + (4 * q + u) * RP);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        g[0] = fmaf(r4[u], x2[u][0], g[0]);
                        g[1] = fmaf(r4[u], x2[u][1], g[1]);
                    }
                }
                for (int t = 4 * m4; t < ma; ++t) {
                    const float r = rr[t];
                    g[0] = fmaf(r, xp[t * RP], g[0]);
                    g[1] = fmaf(r, xp[t * RP + 1], g[1]);
                }
            } else {
                const float* hc = HT + l32;
                for (int t = 0; t < ma; ++t) {
                    const float r = rr[t];
#pragma unroll
                    for (int c = 0; c < NC; ++c) g[c] = fmaf(r, hc[t * (RP + 1) + kWaLPR * c], g[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) Gs[f * RP + l32 + kWaLPR * c] = l32 + kWaLPR * c < Ra ? g[c] : 0.f;
        }
        const float dw = wave_sum_f(dterm);
        if ((tid & 63) == 0) red[tid >> 6] = (double)dw;
        __syncthreads();
        if (tid < RP) {
            double s = 0.0;
            for (int ff = 0; ff < RB; ++ff) s += (double)Gs[ff * RP + tid] * Wd[ff * RP + tid];
            xstore(a.part1 + (size_t)wg * (RP + 1) + tid, s);  // colsum(G .* W) partial (:217)
        }
        if (tid == RP) {
            double dsum = 0.0;
#pragma unroll
            for (int q = 0; q < NWV; ++q) dsum += red[q];
            xstore(a.part1 + (size_t)wg * (RP + 1) + RP, dsum);
        }
        WA_STAMP(2);
        bar_ok &= grid_bar(a.bar, (unsigned)nwg, gen, oks);
        cross_sum(a.part1, RP + 1, RP + 1, nwg, scr, tmp);     // colsum(G .* W) | div
        if (tid < RP) cq[tid] = tmp[tid];
        if (tid == RP) red[NWV] = tmp[RP];
        __syncthreads();
        WA_STAMP(3);
        if (a.cost_check && j > 1) {                      // cost of iterate j-1 (:260-284)
            const double cost = red[NWV] + sh_const;
            const int it = j - 1;
            bool stopnow = false;
            if (it > 1 && a.conv_eps > 0.0) stopnow = fabs(cost - last_cost) / last_cost < a.conv_eps;
            if (wg == 0 && tid == 0) a.costh[it - 1] = cost;
            n_rec = it;
            last_cost = cost;
            if (stopnow) {
                stopped = true;
                break;
            }
        }
        if (j > a.max_iter) break;
        // ---- W update (:215-222) on this block's rows, then the norms ------------------------------
        for (int i = tid; i < RB * RP; i += NT) {
            const int k = i % RP;
            double wv = Wd[i];
            if (k < Ra && a.w_ind[k]) {
                const double s = (double)sk[k];
                double dpw = s + wv * cq[k];
                dpw = dpw > (double)a.flr ? dpw : (double)a.flr;
                wv = wv * ((double)Gs[i] + wv * (s * cs[k])) / dpw;
            }
            Wd[i] = wv;
        }
        __syncthreads();
        if (tid < RP) {
            double s2 = 0.0, s1 = 0.0;
            for (int ff = 0; ff < RB; ++ff) {
                const double w = Wd[ff * RP + tid];
                s2 += w * w;
                s1 += w;
            }
            xstore(a.part2 + (size_t)wg * 2 * RP + tid, s2);
            xstore(a.part2 + (size_t)wg * 2 * RP + RP + tid, s1);
        }
        WA_STAMP(4);
        bar_ok &= grid_bar(a.bar, (unsigned)nwg, gen, oks);
        cross_sum(a.part2, 2 * RP, 2 * RP, nwg, scr, tmp);
        if (tid < RP) {
            const double nrm = tid < Ra ? sqrt(tmp[tid]) : 1.0;
            cq[tid] = nrm;
            cs[tid] = tmp[RP + tid] / nrm;               // colsum of the normalised W
        }
        __syncthreads();
        WA_STAMP(5);
        for (int i = tid; i < RB * RP; i += NT) {
            const int k = i % RP;
            const double w = k < Ra ? Wd[i] / cq[k] : 0.0;   // :242, ALL columns
            Wd[i] = w;
            Wf[i] = (float)w;
        }
        __syncthreads();
        WA_STAMP(6);
#ifdef SNMF_PROF_WA
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_wa_prof[8], 1ull);
#endif
    }
    __syncthreads();
    for (int i = tid; i < RB * RP; i += NT) {
        const int k = i / RB, ff = i - k * RB;
        if (k < Ra && f0 + ff < F) a.Wout[(size_t)k * F + f0 + ff] = Wd[ff * RP + k];
    }
    if (wg == 0 && tid == 0) *a.n_iter_out = !bar_ok ? -1 : (stopped ? n_rec : a.max_iter);
    WA_STAMP(7);
#ifdef SNMF_PROF_WA
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_wa_prof[9], 1ull);
#endif
}

// The separator's state g into (k_ostate_get) / out of (k_ostate_put) one staging record: the batched separator's ostate_xfer
// on the single-stream arrays, which are the batch's with S = 1 and the slot list {0}.  Grid (1, kStN, kStParts).  `l`: the
// 1-based index of the next frame (a put reads it from the record).  In Mel mode a.Bm is the Mel master; a.Bdf stays NULL,
// the fp32 mirrors are rebuilt by k_omirror behind a put.
__global__ __launch_bounds__(256) void k_ostate_get(OStateArgs<float> a, int64_t l) {
    const int slot0 = 0;
    const int64_t l0 = l;
    a.slots = &slot0;
    a.l = &l0;
    ostate_xfer<float, false>(a);
}
__global__ __launch_bounds__(256) void k_ostate_put(OStateArgs<float> a) {
    const int slot0 = 0;
    a.slots = &slot0;
    a.l = nullptr;
    ostate_xfer<float, true>(a);
}

// the fp32 mirror of n fp64 dictionary entries, rounded as k_oassemble rounds a re-assembled column
__global__ __launch_bounds__(256) void k_omirror(const double* __restrict__ src, float* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}

}  // namespace snmf
