// snmf_batch.h -- device code of the batched offline solver: B independent problems V_b ~ W_b * H_b (one F, one r, one
// settings struct, a frame count T_b of their own) advance through the iteration of src/sparse_nmf.m:186-286 in SHARED
// launches.  The arithmetic is the fp32 solver's (f32 MFMA 32x32x2 products, fp64 statistics, fp64 master copy of W); what
// is new is the geometry: a workgroup is handed a (problem, piece) pair by a device table instead of a piece of one problem.
//
//   k_bh    : H step of one (problem, 32-frame tile): Lam = W*H -> ratio image(s) in LDS -> W'*ratio -> H <- H .* dmh ./ dph,
//             and the divergence / sum(sparsity .* H) partials of the iterate it READS (one pair of doubles per tile)
//   k_bw    : W statistics of one (problem, chunk of kBChunkTiles tiles, row group, column group): Lam' = W*H ->
//             ratio image(s) -> G += ratio * H' in registers over the chunk, written once as an fp32 slab
//   k_bfin  : one (problem, column): folds the problem's objective partials and runs its stop test (:272-284), adds the
//             chunk slabs in chunk order in fp64, the F x r epilogue of :215-244 for its column (the update and the
//             renormalisation are column-local), and the column's entries of the W images of the next H step
//   k_bfold : the objective fold + stop test alone (loops that do not update W, and the last iterate of a run)
//   k_btake_h : one (problem, tile): the initial H of this batch from rows of the result H of another batch (the batched DNMF loop)
//   k_bfloor_v, k_brand_h : grid (workgroups, problem): the V floor on a V that was written on the device, and an initial H drawn
//             on the device (the batched DNMF loop from waveforms)
//   k_btake_w : grid (workgroups, problem): the initial W of every problem from columns of its own V (batched basis training)
//
// Layouts: the engine's (snmf_kernels.h, StepArgs): V [Ttot][Fp], H [Ttot][rp], Wt4 / Wk4 per problem; the frames of
// problem b start at tile prob[b].tile0, so a tile never spans two problems.  A problem's last tile is partial when T_b is
// no multiple of 32: its missing frames are masked where the ratio image is written and where H is written (they hold
// zeros everywhere), so nothing of them reaches a sum.
//
// Independence.  Every workgroup touches one problem only, the tables fix which tiles / chunks a problem has from T_b alone,
// and every sum has a fixed order (lanes, waves, tiles, chunks): the bits of a problem depend on its inputs and the
// settings, not on the batch around it.  Kernel boundaries are the only ordering between workgroups; there are no waits.
// A problem whose stop test fired is frozen: BState::stop is read at the top of every workgroup of that problem.
#pragma once
#include "snmf_kernels.h"
#include "snmf_philox.h"

namespace snmf {

constexpr int kBW = 8;            // waves per workgroup of k_bh / k_bw
constexpr int kBThr = 64 * kBW;
constexpr int kBChunkTiles = 2;   // 32-frame tiles per W-statistics chunk (64 frames: the longest fp32 chain over frames; DESIGN.md, "How the
                                  // batch kernels are judged", has why)
constexpr int kBMaxF = 513;       // envelope: 16 row tiles (+ the extra row of F = 32n+1)
constexpr int kBMaxR = 200;       //           7 column tiles

struct BProb {
    int T;         // frames
    int tile0;     // first 32-frame tile (frame offset 32 * tile0)
    int n_tiles;
    int chunk0;    // first W-statistics chunk
    int n_chunks;
};
struct BState {
    int stop;    // the stop test fired (src/sparse_nmf.m:275-281): the problem is frozen
    int n_iter;  // iterate whose objective was recorded last (= the stop index once stop is set)
    int n_rec;   // objectives recorded
    int hsel;    // buffer that holds the H of the stop iterate
};
struct BTile {
    int b, l;    // problem, tile / chunk inside the problem
};

struct BatchArgs {
    const float* V;
    float* H[2];
    float* Wt4;
    float* Wk4;
    double* Wc;           // fp64 master copy of W, [rp][Fp] per problem
    const double* Wraw;   // k_bfin, init: the initial W as uploaded, [rp][Fp]
    float* wx;            // [B][rp] extra row of W
    float* colsum;        // [B][rp] column sums of W
    double* wn0;          // [B][rp] column norms of the initial W (:157-160: H is rescaled by them)
    const float* lamk;    // [rp] sparsity per row of H
    const uint8_t* w_ind; // [r]
    float* slabs;         // [chunks][n_mat][rp][Fp]
    float* spart;         // [chunks][rp] row sums of H (KL)
    double* part;         // [tiles][2] (div, sum sparsity .* H) of the iterate the last objective pass read
    double* divh;         // [B][max_iter]
    double* costh;
    const BProb* prob;
    const BTile* tiles;
    const BTile* chunks;
    BState* st;
    int* n_stopped;
    long long sWt, sWk, sWc;  // per-problem strides of Wt4, Wk4, Wc (elements)
    int F, r, Fp, rp, nf, nk, nqk, Fm, Fq, xr;
    int ldh, ldr, ldrw;   // LDS leading dimensions: H tile, ratio image of k_bh / of k_bw
    int cf;               // k_bh: row tiles per pass over the ratio image (all of them for KL)
    int S;                // k_bh: ways W'*ratio is cut over the contraction (8 / nk)
    int nfg, nkg;         // k_bw: row tiles / column tiles per workgroup
    int n_mat;            // 1: KL (ratio), 2: ratio and denominator images
    int max_iter, cost_check;
    float beta, inv_bb1;
    double conv_eps;
};

__device__ __forceinline__ double b_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Lam tile (32 rows of W) x (32 frames): wt -> this lane's f32x4 of the tile's first 8-deep block (Wt4), hrow -> Hs + fl*ldh + 4h
__device__ __forceinline__ f32x16 b_lam_tile(const f32x4* __restrict__ wt, const float* hrow, int nqk) {
    f32x16 acc = zero16();
    f32x4 wv = wt[0];
    for (int q = 0; q < nqk; ++q) {
        const f32x4 wn = wt[min(q + 1, nqk - 1) * 64];  // the next block's fragment is in flight under this block's MFMAs
        const f32x4 hv = *reinterpret_cast<const f32x4*>(hrow + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = mfma32(wv[e], hv[e], acc);
        wv = wn;
    }
    return acc;
}

// Lam tile -> ratio image (KL: V ./ Lam; else V .* Lam^(beta-2) and the denominator image Lam^(beta-1)), rows f0 + 8g + j of
// frame fl; entries outside F x T_b are written as zeros.  obj: the tile's divergence terms (:248-258) into dsum.
template <int BM>
__device__ __forceinline__ void b_ratio_tile(const f32x16& acc, const float* __restrict__ vcol, float* rrow, float* drw, int f0, int F,
                                             bool tvalid, bool obj, float beta, float inv_bb1, double& dsum) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(vcol + 8 * g);
        f32x4 o, d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lam = fmaxf(acc[4 * g + j], kFlr);
            const bool ok = tvalid && (f0 + 8 * g + j < F);
            if (obj && ok) dsum += (double)div_term<BM>(v[j], lam, beta, inv_bb1);
            if (BM == BM_KL) {
                o[j] = ok ? v[j] * fast_rcp(lam) : 0.f;
            } else {
                o[j] = ok ? v[j] * numfac_of_lam<BM>(lam, beta) : 0.f;
                d[j] = ok ? den_of_lam<BM>(lam, beta) : 0.f;
            }
        }
        *reinterpret_cast<f32x4*>(rrow + 8 * g) = o;
        if (BM != BM_KL) *reinterpret_cast<f32x4*>(drw + 8 * g) = d;
    }
}

// The extra row (F = 32 nf + 1) of a tile: Lam[Fm][t] as a dot product on the VALU, 16 lanes per frame (fixed order), its
// ratio entries into column `col` of the image(s) and zeros into the seven columns behind it (the rest of the 8-deep block).
template <int BM>
__device__ __forceinline__ void b_extra_row(const BatchArgs& a, const float* __restrict__ wx, const float* Hs, const float* __restrict__ Vt,
                                            float* Rs, float* Ds, int ld, int col, int Tl, bool obj, double& dsum) {
    const int t = threadIdx.x >> 4, sub = threadIdx.x & 15;
    float s = 0.f;
    for (int k = sub; k < a.r; k += 16) s += wx[k] * Hs[t * a.ldh + k];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (sub == 0) {
        const float lam = fmaxf(s, kFlr), v = Vt[(long long)t * a.Fp + a.Fm];
        const bool ok = t < Tl;
        if (obj && ok) dsum += (double)div_term<BM>(v, lam, a.beta, a.inv_bb1);
        if (BM == BM_KL) {
            Rs[t * ld + col] = ok ? v * fast_rcp(lam) : 0.f;
        } else {
            Rs[t * ld + col] = ok ? v * numfac_of_lam<BM>(lam, a.beta) : 0.f;
            Ds[t * ld + col] = ok ? den_of_lam<BM>(lam, a.beta) : 0.f;
        }
    } else if (sub < 8) {
        Rs[t * ld + col + sub] = 0.f;
        if (BM != BM_KL) Ds[t * ld + col + sub] = 0.f;
    }
}

// H tile [32][rp] of the problem -> LDS [32][ldh]; obj: this thread's share of sum(sparsity .* H) into shsum
__device__ __forceinline__ void b_load_h(const BatchArgs& a, const float* __restrict__ Ht, float* Hs, bool obj, double& shsum) {
    const int rp4 = a.rp >> 2;
    for (int i = threadIdx.x; i < 32 * rp4; i += kBThr) {
        const int t = i / rp4, c = (i - t * rp4) * 4;
        const f32x4 hv = *reinterpret_cast<const f32x4*>(Ht + (long long)t * a.rp + c);
        *reinterpret_cast<f32x4*>(Hs + t * a.ldh + c) = hv;
        if (obj) {
            const f32x4 lk = *reinterpret_cast<const f32x4*>(a.lamk + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) shsum += (double)lk[j] * (double)hv[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// H step.  LDS: [16 doubles][Hs 32 x ldh][image region]; the image region holds the ratio image(s) [32][ldr] of one pass
// and, after the last pass, the partial numerators of the waves (S ways over the contraction, added in part order).
// cur: buffer of the iterate read; upd: write the updated H to the other buffer; obj: write the objective partials.
// ------------------------------------------------------------------------------------------------------------------
template <int BM>
__global__ __launch_bounds__(kBThr) void k_bh(BatchArgs a, int cur, int upd, int obj) {
    extern __shared__ double b_lds[];
    const BTile tt = a.tiles[blockIdx.x];
    const int b = tt.b;
    if (a.st[b].stop) return;
    const BProb pb = a.prob[b];
    const int tg = pb.tile0 + tt.l;
    const long long fr0 = 32LL * tg;
    const int Tl = min(32, pb.T - 32 * tt.l);
    constexpr int NM = BM == BM_KL ? 1 : 2;
    double* red = b_lds;
    float* Hs = reinterpret_cast<float*>(b_lds + 16);
    float* Rs = Hs + 32 * a.ldh;
    float* Ds = Rs + 32 * a.ldr;
    const int tid = threadIdx.x, w = wave_index(), lane = tid & 63, fl = lane & 31, h = lane >> 5;
    const float* Wt = a.Wt4 + (long long)b * a.sWt;
    const float* Wk = a.Wk4 + (long long)b * a.sWk;
    const float* Vt = a.V + fr0 * a.Fp;
    double dsum = 0.0, shsum = 0.0;

    b_load_h(a, a.H[cur] + fr0 * a.rp, Hs, obj != 0, shsum);
    __syncthreads();

    const int nk = a.nk, S = a.S;
    const int kap = w % nk, part = w / nk;
    const bool p2 = w < nk * S;
    f32x16 accn = zero16(), accd = zero16();
    const int n_fc = (a.nf + a.cf - 1) / a.cf;
    for (int c = 0; c < n_fc; ++c) {
        const int phi0 = c * a.cf, ntc = min(a.cf, a.nf - phi0);
        const bool last = c == n_fc - 1;
        for (int phi = phi0 + w; phi < phi0 + ntc; phi += kBW) {
            const f32x4* wt = reinterpret_cast<const f32x4*>(Wt) + (long long)phi * (a.rp >> 3) * 64 + h * 32 + fl;
            const f32x16 acc = b_lam_tile(wt, Hs + fl * a.ldh + 4 * h, a.nqk);
            const int off = fl * a.ldr + 32 * (phi - phi0) + 4 * h;
            b_ratio_tile<BM>(acc, Vt + (long long)fl * a.Fp + 32 * phi + 4 * h, Rs + off, Ds + off, 32 * phi + 4 * h, a.F, fl < Tl,
                             obj != 0, a.beta, a.inv_bb1, dsum);
        }
        if (a.xr && last) b_extra_row<BM>(a, a.wx + (long long)b * a.rp, Hs, Vt, Rs, Ds, a.ldr, 32 * ntc, Tl, obj != 0, dsum);
        __syncthreads();
        if (upd && p2) {
            const int qa = phi0 * 4, qb = (phi0 + ntc) * 4 + ((a.xr && last) ? 1 : 0);
            const f32x4* wk = reinterpret_cast<const f32x4*>(Wk) + (long long)kap * (a.Fq >> 3) * 64 + h * 32 + fl;
            const float* rr = Rs + fl * a.ldr + 4 * h;
            const float* dr = Ds + fl * a.ldr + 4 * h;
            f32x4 wv = wk[min(qa + part, qb - 1) * 64];
            for (int q = qa + part; q < qb; q += S) {
                const f32x4 wn = wk[min(q + S, qb - 1) * 64];
                const f32x4 rv = *reinterpret_cast<const f32x4*>(rr + 8 * (q - qa));
#pragma unroll
                for (int e = 0; e < 4; ++e) accn = mfma32(wv[e], rv[e], accn);
                if (NM == 2) {
                    const f32x4 dv = *reinterpret_cast<const f32x4*>(dr + 8 * (q - qa));
#pragma unroll
                    for (int e = 0; e < 4; ++e) accd = mfma32(wv[e], dv[e], accd);
                }
                wv = wn;
            }
        }
        __syncthreads();
    }
    if (obj) {
        dsum = b_wave_sum(dsum);
        shsum = b_wave_sum(shsum);
        if (lane == 0) {
            red[2 * w] = dsum;
            red[2 * w + 1] = shsum;
        }
    }
    f32x4* Ps = reinterpret_cast<f32x4*>(Rs);  // [wave][NM][4][64]
    if (upd && p2) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 x;
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = accn[4 * g + j];
            Ps[((w * NM + 0) * 4 + g) * 64 + lane] = x;
            if (NM == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = accd[4 * g + j];
                Ps[((w * NM + 1) * 4 + g) * 64 + lane] = x;
            }
        }
    }
    __syncthreads();
    if (obj && tid == 0) {
        double d = 0.0, s = 0.0;
        for (int i = 0; i < kBW; ++i) {
            d += red[2 * i];
            s += red[2 * i + 1];
        }
        a.part[2LL * tg] = d;
        a.part[2LL * tg + 1] = s;
    }
    if (!upd) return;
    float* Ho = a.H[cur ^ 1] + fr0 * a.rp;
    const float* cs = a.colsum + (long long)b * a.rp;
    for (int e = tid; e < nk * 256; e += kBThr) {
        const int kp = e >> 8, g = (e >> 6) & 3, ln = e & 63, t = ln & 31, k0 = 32 * kp + 8 * g + 4 * (ln >> 5);
        f32x4 num = Ps[(((0 * nk + kp) * NM + 0) * 4 + g) * 64 + ln], den;
        for (int p = 1; p < S; ++p) num += Ps[(((p * nk + kp) * NM + 0) * 4 + g) * 64 + ln];
        if (NM == 2) {
            den = Ps[(((0 * nk + kp) * NM + 1) * 4 + g) * 64 + ln];
            for (int p = 1; p < S; ++p) den += Ps[(((p * nk + kp) * NM + 1) * 4 + g) * 64 + ln];
        }
        const f32x4 ho = *reinterpret_cast<const f32x4*>(Hs + t * a.ldh + k0);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j;
            const float dp = fmaxf((NM == 2 ? den[j] : cs[k]) + a.lamk[k], kFlr);  // :192-193, :197-198, :202-203
            o[j] = (k < a.r && t < Tl) ? ho[j] * num[j] / dp : 0.f;
        }
        *reinterpret_cast<f32x4*>(Ho + (long long)t * a.rp + k0) = o;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// W statistics.  grid (chunks, row groups, column groups).  LDS: [Hs 32 x ldh][image(s) 32 x ldrw].  The workgroup's
// nfg x nkg output tiles are dealt to the waves (tile id = wave + 8 j), NA accumulators (x n_mat) per wave.
// hn: the buffer that holds the iterate the H step of this iteration produced.
// ------------------------------------------------------------------------------------------------------------------
template <int BM, int NA>
__global__ __launch_bounds__(kBThr) void k_bw(BatchArgs a, int hn) {
    extern __shared__ double b_lds[];
    const BTile cc = a.chunks[blockIdx.x];
    const int b = cc.b;
    if (a.st[b].stop) return;
    const BProb pb = a.prob[b];
    constexpr int NM = BM == BM_KL ? 1 : 2;
    float* Hs = reinterpret_cast<float*>(b_lds);
    float* Rs = Hs + 32 * a.ldh;
    float* Ds = Rs + 32 * a.ldrw;
    const int tid = threadIdx.x, w = wave_index(), lane = tid & 63, fl = lane & 31, h = lane >> 5;
    const int phi0 = blockIdx.y * a.nfg, ntf = min(a.nfg, a.nf - phi0);
    const bool lastfg = blockIdx.y == gridDim.y - 1, xrow = a.xr && lastfg;
    const int kap0 = blockIdx.z * a.nkg, ntk = min(a.nkg, a.nk - kap0);
    const int n_out = ntf * ntk;
    const float* Wt = a.Wt4 + (long long)b * a.sWt;
    f32x16 acc[NM][NA];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int j = 0; j < NA; ++j) acc[m][j] = zero16();
    float hs = 0.f, gxq = 0.f, gxp = 0.f;
    double dummy = 0.0;
    const int lt0 = cc.l * kBChunkTiles, lt1 = min(pb.n_tiles, lt0 + kBChunkTiles);
    for (int lt = lt0; lt < lt1; ++lt) {
        const long long fr0 = 32LL * (pb.tile0 + lt);
        const int Tl = min(32, pb.T - 32 * lt);
        const float* Vt = a.V + fr0 * a.Fp;
        b_load_h(a, a.H[hn] + fr0 * a.rp, Hs, false, dummy);
        __syncthreads();
        if (w < ntf) {
            const int phi = phi0 + w;
            const f32x4* wt = reinterpret_cast<const f32x4*>(Wt) + (long long)phi * (a.rp >> 3) * 64 + h * 32 + fl;
            const f32x16 lam = b_lam_tile(wt, Hs + fl * a.ldh + 4 * h, a.nqk);
            const int off = fl * a.ldrw + 32 * w + 4 * h;
            b_ratio_tile<BM>(lam, Vt + (long long)fl * a.Fp + 32 * phi + 4 * h, Rs + off, Ds + off, 32 * phi + 4 * h, a.F, fl < Tl, false,
                             a.beta, a.inv_bb1, dummy);
        }
        if (xrow) b_extra_row<BM>(a, a.wx + (long long)b * a.rp, Hs, Vt, Rs, Ds, a.ldrw, 32 * ntf, Tl, false, dummy);
        __syncthreads();
        const int nq = (Tl + 7) >> 3;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int id = w + kBW * j;
            if (id < n_out) {
                const int kal = id / ntf, phl = id - kal * ntf;
                const float* ra = Rs + 4 * h * a.ldrw + 32 * phl + fl;
                const float* da = Ds + 4 * h * a.ldrw + 32 * phl + fl;
                const float* hb = Hs + 4 * h * a.ldh + 32 * (kap0 + kal) + fl;
                for (int q = 0; q < nq; ++q) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float hv = hb[(8 * q + e) * a.ldh];
                        acc[0][j] = mfma32(ra[(8 * q + e) * a.ldrw], hv, acc[0][j]);
                        if (NM == 2) acc[1][j] = mfma32(da[(8 * q + e) * a.ldrw], hv, acc[1][j]);
                    }
                }
            }
        }
        if (tid < 32 * ntk) {  // row sums of H (KL: the "P" of every row) and the extra row of the statistics
            const int k = 32 * kap0 + tid;
            for (int t = 0; t < Tl; ++t) {
                const float hv = Hs[t * a.ldh + k];
                hs += hv;
                if (xrow) {
                    gxq += Rs[t * a.ldrw + 32 * ntf] * hv;
                    if (NM == 2) gxp += Ds[t * a.ldrw + 32 * ntf] * hv;
                }
            }
        }
        __syncthreads();
    }
    const long long cg = pb.chunk0 + cc.l, nW = (long long)a.rp * a.Fp;
    float* slab = a.slabs + cg * NM * nW;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int id = w + kBW * j;
        if (id < n_out) {
            const int kal = id / ntf, phl = id - kal * ntf;
            const long long base = (long long)(32 * (kap0 + kal) + fl) * a.Fp + 32 * (phi0 + phl) + 4 * h;
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 x;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) x[jj] = acc[m][j][4 * g + jj];
                    *reinterpret_cast<f32x4*>(slab + m * nW + base + 8 * g) = x;
                }
        }
    }
    if (tid < 32 * ntk) {
        const int k = 32 * kap0 + tid;
        if (xrow) {
            slab[(long long)k * a.Fp + a.Fm] = gxq;
            if (NM == 2) slab[nW + (long long)k * a.Fp + a.Fm] = gxp;
        }
        if (BM == BM_KL && blockIdx.y == 0) a.spart[cg * a.rp + k] = hs;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Objective fold + stop test of iterate j for problem b (src/sparse_nmf.m:260-285), by a workgroup of 256 threads.
// Every workgroup of the problem in a launch evaluates it identically from data earlier launches wrote (the partials, the
// cost of iterate j - 1); `recorder` (one of them) writes the history and the state.  Returns true when the problem is
// frozen (stopped before, or stopping now).  cur: the buffer that holds H of iterate j.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool b_fold(const BatchArgs& a, int b, int j, int cur, bool recorder, double* red /*[512]*/) {
    const int tid = threadIdx.x;
    // one read per workgroup (a concurrent recorder of this launch can turn the word from 0 into 1 -- the 1 the test below
    // gives as well -- and the threads of a workgroup must not disagree in front of a barrier)
    if (tid == 0) red[0] = (double)a.st[b].stop;
    __syncthreads();
    const bool was = red[0] != 0.0;
    __syncthreads();
    if (was) return true;
    const BProb pb = a.prob[b];
    double d = 0.0, s = 0.0;
    for (int i = tid; i < pb.n_tiles; i += 256) {
        d += a.part[2LL * (pb.tile0 + i)];
        s += a.part[2LL * (pb.tile0 + i) + 1];
    }
    red[tid] = d;
    red[256 + tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o];
            red[256 + tid] += red[256 + tid + o];
        }
        __syncthreads();
    }
    const double div = red[0], cost = red[0] + red[256];
    __syncthreads();
    bool stopnow = false;
    double* ch = a.costh + (long long)b * a.max_iter;
    if (j > 1 && a.conv_eps > 0.0) {
        const double last = ch[j - 2];
        stopnow = fabs(cost - last) / last < a.conv_eps;
    }
    if (recorder && tid == 0) {
        a.divh[(long long)b * a.max_iter + j - 1] = div;
        ch[j - 1] = cost;
        BState* st = a.st + b;
        st->n_rec = j;
        st->n_iter = j;
        if (stopnow) {
            st->hsel = cur;
            st->stop = 1;
            atomicAdd(a.n_stopped, 1);
        }
    }
    return stopnow;
}

__global__ __launch_bounds__(256) void k_bfold(BatchArgs a, int j, int cur) {
    __shared__ double red[512];
    b_fold(a, blockIdx.x, j, cur, true, red);
}

// sums of two values over the workgroup (256 threads), every thread gets both
__device__ __forceinline__ void b_block_sum2(double& x, double& y, double* red) {
    const int tid = threadIdx.x;
    red[tid] = x;
    red[256 + tid] = y;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o];
            red[256 + tid] += red[256 + tid + o];
        }
        __syncthreads();
    }
    x = red[0];
    y = red[256];
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------
// Finish: grid (r, problems), 256 threads, column k = blockIdx.x of problem b0 + blockIdx.y.
//   init = 1: W <- Wraw with unit columns (:157-158), wn0 <- the norms; nothing is folded.
//   init = 0: iteration `it`: fold = 1 folds the objective of iterate it - 1 and tests; then the W update of :215-244.
// ------------------------------------------------------------------------------------------------------------------
template <int BM>
__global__ __launch_bounds__(256) void k_bfin(BatchArgs a, int b0, int init, int it, int fold, int cur) {
    __shared__ double red[512];
    const int k = blockIdx.x, b = b0 + blockIdx.y, tid = threadIdx.x;
    if (!init) {
        const bool frozen = fold ? b_fold(a, b, it - 1, cur, k == 0, red) : a.st[b].stop != 0;
        if (frozen) return;
    }
    const BProb pb = a.prob[b];
    constexpr int NE = (kBMaxF + 255) / 256;
    const long long nW = (long long)a.rp * a.Fp;
    double* Wc = a.Wc + (long long)b * a.sWc + (long long)k * a.Fp;
    const double* src = init ? a.Wraw + (long long)k * a.Fp : Wc;
    double wv[NE], qv[NE], pv[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int f = tid + 256 * i;
        wv[i] = f < a.F ? src[f] : 0.0;
        qv[i] = pv[i] = 0.0;
    }
    if (!init && a.w_ind[k]) {
        double s = 0.0;
        for (int c = 0; c < pb.n_chunks; ++c) {  // chunk order, fp64
            const float* slab = a.slabs + (long long)(pb.chunk0 + c) * a.n_mat * nW + (long long)k * a.Fp;
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int f = tid + 256 * i;
                if (f < a.F) {
                    qv[i] += (double)slab[f];
                    if (BM != BM_KL) pv[i] += (double)slab[nW + f];
                }
            }
            if (BM == BM_KL) s += (double)a.spart[(long long)(pb.chunk0 + c) * a.rp + k];
        }
        double x = 0.0, y = 0.0;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            x += qv[i] * wv[i];                            // sum(Q .* w)          (:216, :224, :231)
            y += BM == BM_KL ? wv[i] : pv[i] * wv[i];      // sum(P .* w), KL: P = s (:220, :228, :236)
        }
        b_block_sum2(x, y, red);
        if (BM == BM_KL) y *= s;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const double P = BM == BM_KL ? s : pv[i];
            const double dpw = fmax(P + x * wv[i], 1e-9), dmw = qv[i] + y * wv[i];
            if (tid + 256 * i < a.F) wv[i] = wv[i] * dmw / dpw;  // :222, :229, :239
        }
    }
    double n2 = 0.0, cs = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) n2 += wv[i] * wv[i];
    b_block_sum2(n2, cs, red);
    const double nrm = sqrt(n2);
    cs = 0.0;
    double zz = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        if (tid + 256 * i < a.F) wv[i] = wv[i] / nrm;  // :158, :242 (every column)
        cs += wv[i];
    }
    b_block_sum2(cs, zz, red);
    float* Wt = a.Wt4 + (long long)b * a.sWt;
    float* Wk = a.Wk4 + (long long)b * a.sWk;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int f = tid + 256 * i;
        if (f < a.F) {
            Wc[f] = wv[i];
            const float wf = (float)wv[i];
            if (f < a.Fm)
                Wt[((((long long)(f >> 5) * (a.rp >> 3) + (k >> 3)) * 2 + ((k >> 2) & 1)) * 32 + (f & 31)) * 4 + (k & 3)] = wf;
            else
                a.wx[(long long)b * a.rp + k] = wf;
            Wk[((((long long)(k >> 5) * (a.Fq >> 3) + (f >> 3)) * 2 + ((f >> 2) & 1)) * 32 + (k & 31)) * 4 + (f & 3)] = wf;
        }
    }
    if (tid == 0) {
        a.colsum[(long long)b * a.rp + k] = (float)cs;
        if (init) a.wn0[(long long)b * a.rp + k] = nrm;
    }
}

// h <- h .* wn (:159) on the frames of problem b, in buffer 0
static __global__ __launch_bounds__(256) void k_bscale(BatchArgs a, int b) {
    const BProb pb = a.prob[b];
    float* H = a.H[0] + 32LL * pb.tile0 * a.rp;
    const double* wn = a.wn0 + (long long)b * a.rp;
    const long long n = (long long)pb.T * a.rp;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int k = (int)(i % a.rp);
        if (k < a.r) H[i] = (float)((double)H[i] * wn[k]);
    }
}

// H0 of every problem of batch `a` from rows [row0, row0 + a.r) of the result H of another batch with the same frame counts (and
// so the same tile table): grid = a's tiles, one (problem, 32-frame tile) each.  s0 / s1: the other batch's two H buffers,
// [frame][srp]; sst: its states; scur: the buffer its unstopped problems ended in.  A problem's source is the buffer of its
// stop iterate (BState::hsel) once it has stopped -- the choice the host makes when it reads H back.  Lanes run along k, the
// contiguous direction on both sides.  Pad rows (k >= a.r) and pad frames (t >= T_b) are written as zeros.
static __global__ __launch_bounds__(256) void k_btake_h(BatchArgs a, const float* __restrict__ s0, const float* __restrict__ s1,
                                                        const BState* __restrict__ sst, int scur, int srp, int row0) {
    const BTile tt = a.tiles[blockIdx.x];
    const BProb pb = a.prob[tt.b];
    const BState ss = sst[tt.b];
    const float* __restrict__ S = (ss.stop ? ss.hsel : scur) ? s1 : s0;
    const long long fr0 = 32LL * (pb.tile0 + tt.l);
    const int Tl = min(32, pb.T - 32 * tt.l);
    float* __restrict__ H = a.H[0];
    for (int i = threadIdx.x; i < 32 * a.rp; i += 256) {
        const int t = i / a.rp, k = i - t * a.rp;
        const long long fr = fr0 + t;
        H[fr * a.rp + k] = (k < a.r && t < Tl) ? S[fr * srp + row0 + k] : 0.f;
    }
}

// grid (workgroups, problems): init_w of problem b = V_b(:, idx[b * r + k]), k < r (run_basis_train.m:82-83) -- the columns of
// the problem's own V block, widened into the fp64 [rp][Fp] layout k_bfin's init pass reads, at W + b * stride.  idx: 0-based,
// on the device; an index outside [0, T_b) (the host refuses it) gives a zero column, never a read outside the block.  Lanes run
// along f, the contiguous direction on both sides.  Pad rows and pad columns are not written.
static __global__ __launch_bounds__(256) void k_btake_w(BatchArgs a, const int64_t* __restrict__ idx, double* __restrict__ W, long long stride) {
    const int b = blockIdx.y;
    const BProb pb = a.prob[b];
    const float* __restrict__ Vb = a.V + 32LL * pb.tile0 * a.Fp;
    double* __restrict__ Wb = W + (long long)b * stride;
    const int n = a.F * a.r;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int k = i / a.F, f = i - k * a.F;
        const long long t = idx[(long long)b * a.r + k];
        Wb[(long long)k * a.Fp + f] = (t >= 0 && t < pb.T) ? (double)Vb[t * a.Fp + f] : 0.0;
    }
}

// v = max(v, flr) (src/sparse_nmf.m:169) on the real F x T_b entries of problem blockIdx.y: what k_pack does on the way in, for a
// V that the grouped front-end wrote into the [frame][Fp] layout.  Pad rows and pad frames are not touched (they hold zeros).
static __global__ __launch_bounds__(256) void k_bfloor_v(BatchArgs a, float* __restrict__ V) {
    const BProb pb = a.prob[blockIdx.y];
    float* __restrict__ Vb = V + 32LL * pb.tile0 * a.Fp;
    const long long n = (long long)pb.T * a.Fp;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if ((int)(i % a.Fp) >= a.F) continue;
        const float v = Vb[i];
        Vb[i] = v > kFlr ? v : kFlr;
    }
}

// H0 of problem blockIdx.y drawn on the device, in buffer 0: H[t][k] = u(k + r * t), the Philox stream of snmf_plan_set_h_random
// (k_rand_h, snmf_tu_dnmf.hip) keyed by seed[b] -- element index in the column-major r x T_b matrix, counter = index / 4.  Every
// entry of the problem's tiles is written: pad rows and pad frames as zeros.  draw[b] == 0: the problem's H0 came from the host.
static __global__ __launch_bounds__(256) void k_brand_h(BatchArgs a, const uint64_t* __restrict__ seed, const uint8_t* __restrict__ draw) {
    const int b = blockIdx.y;
    if (!draw[b]) return;
    const BProb pb = a.prob[b];
    const uint64_t sd = seed[b];
    float* __restrict__ H = a.H[0] + 32LL * pb.tile0 * a.rp;
    const long long n = 32LL * pb.n_tiles * a.rp;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long t = i / a.rp;
        const int k = (int)(i - t * a.rp);
        float v = 0.f;
        if (k < a.r && t < pb.T) {
            const uint64_t e = (uint64_t)k + (uint64_t)a.r * (uint64_t)t, q = e >> 2;
            uint32_t o[4];
            philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), o);
            const int j = (int)(e & 3);
            const uint32_t x = j == 0 ? o[0] : (j == 1 ? o[1] : (j == 2 ? o[2] : o[3]));  // (no indexed array: no scratch)
            v = ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f);
        }
        H[i] = v;
    }
}

}  // namespace snmf
