// ============================================================================================
// The fp64 solve mode (snmf_sparse_nmf_fp64): src/sparse_nmf.m:157-286 with fp64 storage and the contractions on the
// f64 MFMA (v_mfma_f64_16x16x4_f64).  The structure is the out-of-envelope path's (snmf_generic.h): every intermediate
// lives in HBM, one strided split-K GEMM kernel forms all five products of an iteration
//     Lam = W*H,   num = W'*R,   den = W'*D,   Q = R*H',   P = D*H'
// and a few element-wise passes do the rest.  Nothing is padded: V, Lam, R, D are F x T, H / num / den r x T, W / Q / P
// F x r, all column-major and tight, every kernel checks its bounds, so no pad row or column can reach the objective
// (0 * log 0 = NaN) or a sum.  Offsets are 64-bit throughout.
// Every reduction has a fixed order -- the k-loop of a GEMM chunk, the chunk partials (added in chunk order by
// k_s64_sumz), the workgroup trees of the objective and the column sums -- so two runs give the same bits.
// Every per-iteration kernel returns at once when the device-side stop word is set: after a convergence stop
// (src/sparse_nmf.m:272-282) W and H keep the values of the stop iteration without a host round trip.
// ============================================================================================
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snmf {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kS64Blocks = 1024;     // workgroups of the objective pass = its partial slots
constexpr int kS64ChunkK = 2048;     // L: contraction indices per split of a GEMM (each split writes a partial of its own)
constexpr int kS64RowChunk = 256;    // frames per split of the row sums of H
constexpr double kS64Flr = 1e-9;     // src/sparse_nmf.m:166
enum { S64_KL = 0, S64_ED = 1, S64_IS = 2, S64_GEN = 3 };

struct Solve64State {
    int stop;          // 1 once the convergence test of :273-282 has fired
    int n_iter;        // the iteration it fired at
    double last_cost;  // :168, :284
};

// C[z](m, n) = sum_{k in split z} A(m, k) * B(k, n); element (i, j) of X at X[i * rsX + j * csX]; split z covers
// k in [z * kchunk, min(K, (z + 1) * kchunk)) and writes C + z * zC.  do_floor: C = max(C, 1e-9) (one split only).
struct Gemm64Args {
    const double* A;
    const double* B;
    double* C;
    int M, N, K, kchunk;
    long long rsA, csA, rsB, csB, rsC, csC, zC;
    int do_floor;
    const int* stop;
};

// 64 x 64 x 16 LDS tiles, four waves, a 32 x 32 quadrant each as 2 x 2 MFMA tiles of 16 x 16 x 4.  Operand map of the
// f64 MFMA: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result register g of lane l is
// D[row = (l >> 4) + 4 g][col = l & 15] -- NOT the f32 map.  The 16 lanes of a result register run along n, so the
// stores are contiguous (128 bytes) when C's unit stride runs along n: the host hands a product whose C has its unit
// stride along m over as C^T = B^T * A^T (s64_gemm_plan below), a relabelling of the strides.
// Tile bx of a split takes row tile bx % tiles_m and column tile bx / tiles_m.
// This is the tile body: k_s64_gemm (blockIdx.x = bx -- the one grid dimension that holds 2^31 tiles --, blockIdx.y = the
// split z) and the grouped kernel of the batched solve (k_b64_gemm in snmf_batch64.h: bx and z from a table) both call it,
// so a product has one summation order whichever kernel forms it.
__device__ __forceinline__ void s64_gemm_tile(const Gemm64Args& g, unsigned bx, int z, double (*As)[64 + 2], double (*Bs)[64 + 2]) {
    constexpr int BM = 64, BN = 64, BK = 16;
    const int tid = threadIdx.x;
    const int tiles_m = (g.M + BM - 1) / BM;
    const int m0 = (int)(bx % tiles_m) * BM, n0 = (int)(bx / tiles_m) * BN;
    const int k_lo = z * g.kchunk, k_hi = min(g.K, k_lo + g.kchunk);
    const int w = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
    const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    // the faster-running index of each operand picks how a tile is read (coalesced along the unit stride)
    const bool a_m_fast = g.rsA == 1, b_n_fast = g.csB == 1;
    for (int k0 = k_lo; k0 < k_hi; k0 += BK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = tid + 256 * e;  // 1024 elements of each tile
            {
                const int mm = a_m_fast ? (i & 63) : (i >> 4), kk = a_m_fast ? (i >> 6) : (i & 15);
                const int m = m0 + mm, k = k0 + kk;
                As[kk][mm] = (m < g.M && k < k_hi) ? g.A[(long long)m * g.rsA + (long long)k * g.csA] : 0.0;
            }
            {
                const int nn = b_n_fast ? (i & 63) : (i >> 4), kk = b_n_fast ? (i >> 6) : (i & 15);
                const int n = n0 + nn, k = k0 + kk;
                Bs[kk][nn] = (n < g.N && k < k_hi) ? g.B[(long long)k * g.rsB + (long long)n * g.csB] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const double a0 = As[kk + q][wm + l15], a1 = As[kk + q][wm + 16 + l15];
            const double b0 = Bs[kk + q][wn + l15], b1 = Bs[kk + q][wn + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    double* C = g.C + (long long)z * g.zC;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                // rows of D come from the first MFMA operand, columns from the second
                const int m = m0 + wm + 16 * i + q + 4 * reg, n = n0 + wn + 16 * j + l15;
                double v = acc[i][j][reg];
                if (g.do_floor) v = fmax(v, kS64Flr);
                if (m < g.M && n < g.N) C[(long long)m * g.rsC + (long long)n * g.csC] = v;
            }
}

static __global__ __launch_bounds__(256) void k_s64_gemm(Gemm64Args g) {
    if (*g.stop) return;
    __shared__ double As[16][64 + 2];
    __shared__ double Bs[16][64 + 2];
    s64_gemm_tile(g, blockIdx.x, (int)blockIdx.y, As, Bs);
}

// Host side: the kernel arguments of C = A * B with the contraction cut into splits of kS64ChunkK.  One split stores straight
// into C; several write tight column-major partials at zbuf, which k_s64_sumz adds in split order.  The kernel's stores run
// along n: a C whose smaller stride runs along m is formed as C^T = B^T * A^T, which only relabels the strides.  Returns the
// number of splits.  The single solve (gemm64 in snmf_tu_solve64.hip) and the batched solve's tables both come from here.
inline int s64_gemm_plan(Gemm64Args* out, const double* A, long long rsA, long long csA, const double* B, long long rsB, long long csB,
                         double* C, long long rsC, long long csC, int M, int N, int K, bool do_floor, double* zbuf, const int* stop) {
    const int nz = (K + kS64ChunkK - 1) / kS64ChunkK;
    Gemm64Args g;
    g.K = K, g.kchunk = kS64ChunkK, g.stop = stop;
    const bool direct = nz == 1;
    // the partials of a split product are tight and column-major (unit stride along m)
    const long long rs = direct ? rsC : 1, cs = direct ? csC : M;
    if (rs < cs) {  // transposed problem
        g.A = B, g.rsA = csB, g.csA = rsB;
        g.B = A, g.rsB = csA, g.csB = rsA;
        g.M = N, g.N = M, g.rsC = cs, g.csC = rs;
    } else {
        g.A = A, g.rsA = rsA, g.csA = csA;
        g.B = B, g.rsB = rsB, g.csB = csB;
        g.M = M, g.N = N, g.rsC = rs, g.csC = cs;
    }
    g.C = direct ? C : zbuf;
    g.zC = direct ? 0 : (long long)M * N;
    g.do_floor = direct && do_floor;
    *out = g;
    return nz;
}
inline long long s64_gemm_tiles(const Gemm64Args& g) { return (long long)((g.M + 63) / 64) * ((g.N + 63) / 64); }

// C(m, n) = sum over the splits z, in split order, of part[z][m + M * n] (the partials are tight and column-major)
// (Every pass below is a __device__ body -- workgroup bx of gx, or one column -- and a kernel of the single solve around it;
// the batched solve's grouped kernels in snmf_batch64.h call the same bodies, one problem per grid row, so an element has ONE
// expression and one summation order in both and the compiler cannot contract the two differently.)
__device__ __forceinline__ void s64_sumz_span(const double* __restrict__ part, int nz, long long n, int M, double* __restrict__ C,
                                              long long rsC, long long csC, int do_floor, unsigned bx, unsigned gx) {
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n; i += (long long)gx * 256) {
        double s = 0.0;
        for (int z = 0; z < nz; ++z) s += part[(long long)z * n + i];
        if (do_floor) s = fmax(s, kS64Flr);
        const long long col = i / M, row = i - col * M;
        C[row * rsC + col * csC] = s;
    }
}
static __global__ __launch_bounds__(256) void k_s64_sumz(const double* __restrict__ part, int nz, long long n, int M, double* __restrict__ C,
                                                         long long rsC, long long csC, int do_floor, const int* stop) {
    if (*stop) return;
    s64_sumz_span(part, nz, n, M, C, rsC, csC, do_floor, blockIdx.x, gridDim.x);
}

// workgroup sum of one double per thread (256 threads), fixed tree; the result in every thread
__device__ __forceinline__ double s64_block_sum(double v, double* red /*[256]*/) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// R = V .* Lam^(beta-2) (KL: V ./ Lam) and D = Lam^(beta-1) (src/sparse_nmf.m:194, :202-204, :217, :231-236); the
// Euclidean case needs neither (R = V, D = Lam are used where they lie).
template <int MODE>
__device__ __forceinline__ void s64_ratio_span(const double* __restrict__ V, const double* __restrict__ Lam, double* __restrict__ R,
                                               double* __restrict__ D, long long n, double beta, unsigned bx, unsigned gx) {
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n; i += (long long)gx * 256) {
        const double v = V[i], lam = Lam[i];
        if (MODE == S64_KL) {
            R[i] = v / lam;
        } else if (MODE == S64_IS) {
            R[i] = v / (lam * lam);
            D[i] = 1.0 / lam;
        } else {
            R[i] = v * pow(lam, beta - 2.0);
            D[i] = pow(lam, beta - 1.0);
        }
    }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_s64_ratio(const double* __restrict__ V, const double* __restrict__ Lam, double* __restrict__ R,
                                                   double* __restrict__ D, long long n, double beta, const int* stop) {
    if (*stop) return;
    s64_ratio_span<MODE>(V, Lam, R, D, n, beta, blockIdx.x, gridDim.x);
}

__device__ __forceinline__ double s64_sparsity(int kind, double scalar, const double* __restrict__ S, long long i, int k) {
    return kind == 0 ? scalar : (kind == 1 ? S[k] : S[i]);
}

// H <- H .* num ./ max(den + sparsity, flr) (src/sparse_nmf.m:192-205); KL: den = colsum(W)
template <bool KL>
__device__ __forceinline__ void s64_hupd_span(double* __restrict__ H, const double* __restrict__ Num, const double* __restrict__ Den,
                                              const double* __restrict__ colsum, int kind, double scalar, const double* __restrict__ S,
                                              int r, long long n, unsigned bx, unsigned gx) {
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n; i += (long long)gx * 256) {
        const int k = (int)(i % r);
        const double sp = s64_sparsity(kind, scalar, S, i, k);
        const double den = fmax((KL ? colsum[k] : Den[i]) + sp, kS64Flr);
        H[i] = H[i] * Num[i] / den;
    }
}
template <bool KL>
__global__ __launch_bounds__(256) void k_s64_hupd(double* __restrict__ H, const double* __restrict__ Num, const double* __restrict__ Den,
                                                  const double* __restrict__ colsum, int kind, double scalar,
                                                  const double* __restrict__ S, int r, long long n, const int* stop) {
    if (*stop) return;
    s64_hupd_span<KL>(H, Num, Den, colsum, kind, scalar, S, r, n, blockIdx.x, gridDim.x);
}

// colsum[k] = sum_f W[f, k] (:192), one workgroup per column
__device__ __forceinline__ void s64_colsum_col(const double* __restrict__ W, int F, double* __restrict__ colsum, int k, double* red) {
    const double* col = W + (long long)k * F;
    double s = 0.0;
    for (int f = threadIdx.x; f < F; f += 256) s += col[f];
    s = s64_block_sum(s, red);
    if (threadIdx.x == 0) colsum[k] = s;
}
static __global__ __launch_bounds__(256) void k_s64_colsum(const double* __restrict__ W, int F, double* __restrict__ colsum, const int* stop) {
    if (*stop) return;
    __shared__ double red[256];
    s64_colsum_col(W, F, colsum, (int)blockIdx.x, red);
}

// spart[z][k] = sum over the frames of split z of H[k, t] (:215, the row sums of H; the splits are added by k_s64_sumz)
__device__ __forceinline__ void s64_rowsum_chunk(const double* __restrict__ H, int r, int T, int chunk, double* __restrict__ spart, int z,
                                                 unsigned bx, unsigned gx) {
    const int t_lo = z * chunk, t_hi = min(T, t_lo + chunk);
    for (int k = bx * 256 + threadIdx.x; k < r; k += gx * 256) {
        double s = 0.0;
        for (int t = t_lo; t < t_hi; ++t) s += H[(long long)t * r + k];
        spart[(long long)z * r + k] = s;
    }
}
static __global__ __launch_bounds__(256) void k_s64_rowsum(const double* __restrict__ H, int r, int T, int chunk, double* __restrict__ spart,
                                                           const int* stop) {
    if (*stop) return;
    s64_rowsum_chunk(H, r, T, chunk, spart, (int)blockIdx.y, blockIdx.x, gridDim.x);
}

// The F x r epilogue of the W step (src/sparse_nmf.m:215-244), one workgroup per column k:
//   a = sum_f Q[f,k] w[f,k], b = sum_f P[f,k] w[f,k] (KL: P[f,k] = hsum[k] for every f)
//   w <- w .* (Q + b w) ./ max(P + a w, flr)      for the columns of w_update_ind
//   w <- w / sqrt(sum w^2)                         for ALL columns (:242)
// UPD = false: only the normalisation, and wn[k] = the norm (the initial scaling of :157-160).
template <bool KL, bool UPD>
__device__ __forceinline__ void s64_wupd_col(double* __restrict__ W, const double* __restrict__ Q, const double* __restrict__ P,
                                             const double* __restrict__ hsum, const uint8_t* __restrict__ w_ind, int F,
                                             double* __restrict__ wn, int k, double* red) {
    const long long o = (long long)k * F;
    double* col = W + o;
    if (UPD && w_ind[k]) {
        const double hs = KL ? hsum[k] : 0.0;
        double a = 0.0, b = 0.0;
        for (int f = threadIdx.x; f < F; f += 256) {
            const double w = col[f];
            a += Q[o + f] * w;
            b += (KL ? hs : P[o + f]) * w;
        }
        a = s64_block_sum(a, red);
        b = s64_block_sum(b, red);
        for (int f = threadIdx.x; f < F; f += 256) {
            const double w = col[f];
            const double dpw = fmax((KL ? hs : P[o + f]) + a * w, kS64Flr);
            const double dmw = Q[o + f] + b * w;
            col[f] = w * dmw / dpw;
        }
    }
    double s = 0.0;
    for (int f = threadIdx.x; f < F; f += 256) s += col[f] * col[f];  // (each thread re-reads what it wrote itself)
    const double nrm = sqrt(s64_block_sum(s, red));
    for (int f = threadIdx.x; f < F; f += 256) col[f] = col[f] / nrm;
    if (!UPD && threadIdx.x == 0) wn[k] = nrm;
}
template <bool KL, bool UPD>
__global__ __launch_bounds__(256) void k_s64_wupd(double* __restrict__ W, const double* __restrict__ Q, const double* __restrict__ P,
                                                  const double* __restrict__ hsum, const uint8_t* __restrict__ w_ind, int F,
                                                  double* __restrict__ wn, const int* stop) {
    if (UPD && *stop) return;
    __shared__ double red[256];
    s64_wupd_col<KL, UPD>(W, Q, P, hsum, w_ind, F, wn, (int)blockIdx.x, red);
}

// h = bsxfun(@times, h, wn') (:160)
static __global__ __launch_bounds__(256) void k_s64_hscale(double* __restrict__ H, const double* __restrict__ wn, int r, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) H[i] = H[i] * wn[i % r];
}  // (the batched solve launches this kernel and k_s64_floor as they are, once per problem when the problem is set)

// v = max(v, flr) (:169)
static __global__ __launch_bounds__(256) void k_s64_floor(double* __restrict__ X, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) X[i] = fmax(X[i], kS64Flr);
}

// d + one element's divergence term (src/sparse_nmf.m:248-258); the one expression of k_s64_obj and k_s64_mdi_obj
template <int MODE>
__device__ __forceinline__ double s64_div_add(double d, double v, double lam, double beta) {
    if (MODE == S64_KL) {
        d += v * log(v / lam) - v + lam;
    } else if (MODE == S64_ED) {
        d += (v - lam) * (v - lam);
    } else if (MODE == S64_IS) {
        const double qq = v / lam;
        d += qq - log(qq) - 1.0;
    } else {
        d += pow(v, beta) + (beta - 1.0) * pow(lam, beta) - beta * v * pow(lam, beta - 1.0);
    }
    return d;
}

// sum(sparsity .* h) of :261 over the elements of workgroup b, then both workgroup sums into part[2 b] and part[2 b + 1]
__device__ __forceinline__ void s64_obj_tail(double d, const double* __restrict__ H, int kind, double scalar, const double* __restrict__ S,
                                             int r, long long n_h, double* __restrict__ part, double* red, unsigned bx, unsigned gx) {
    double sh = 0.0;
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n_h; i += (long long)gx * 256)
        sh += s64_sparsity(kind, scalar, S, i, (int)(i % r)) * H[i];
    d = s64_block_sum(d, red);
    sh = s64_block_sum(sh, red);
    if (threadIdx.x == 0) {
        part[2 * bx] = d;
        part[2 * bx + 1] = sh;
    }
}

// The divergence terms of src/sparse_nmf.m:248-258 and sum(sparsity .* h) of :261: workgroup b sums its elements (a fixed
// assignment: grid-stride from b) into part[2 b] and part[2 b + 1].
template <int MODE>
__device__ __forceinline__ void s64_obj_block(const double* __restrict__ V, const double* __restrict__ Lam, long long n_v, double beta,
                                              const double* __restrict__ H, int kind, double scalar, const double* __restrict__ S, int r,
                                              long long n_h, double* __restrict__ part, double* red, unsigned bx, unsigned gx) {
    double d = 0.0;
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n_v; i += (long long)gx * 256)
        d = s64_div_add<MODE>(d, V[i], Lam[i], beta);
    s64_obj_tail(d, H, kind, scalar, S, r, n_h, part, red, bx, gx);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_s64_obj(const double* __restrict__ V, const double* __restrict__ Lam, long long n_v, double beta,
                                                 const double* __restrict__ H, int kind, double scalar, const double* __restrict__ S,
                                                 int r, long long n_h, double* __restrict__ part, const int* stop) {
    if (*stop) return;
    __shared__ double red[256];
    s64_obj_block<MODE>(V, Lam, n_v, beta, H, kind, scalar, S, r, n_h, part, red, blockIdx.x, gridDim.x);
}

// ---- the missing-data steps (src/snmf_mdi.m / src/snmf_mdi_Sm.m; M is F x T, 1 = observed, soft masks lie in [0, 1]) ----
// the masked start v = max(v .* M, flr) (src/snmf_mdi.m:175), in the place of k_s64_floor
static __global__ __launch_bounds__(256) void k_s64_mdi_start(double* __restrict__ V, const double* __restrict__ M, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) V[i] = fmax(V[i] * M[i], kS64Flr);
}

// one element of the re-imputation v = max(v .* M + lam .* (1 - M), flr) (:251-254 / snmf_mdi_Sm.m:251-260); M = 1 gives v
// and M = 0 gives lam, both exactly
__device__ __forceinline__ double s64_impute(double v, double m, double lam) { return fmax(v * m + lam * (1.0 - m), kS64Flr); }

// The re-imputation of every iteration fused with the objective of the imputed v (:257-268): V is read once and written
// once, and the partials have the element assignment, the workgroup tree and the slots of k_s64_obj -- with M = 1 the
// objective is the plain solve's bit for bit.  Lam is the max(w * h, flr) the last product left: the reference's v_est.
// (The body of workgroup bx of gx, as every pass above: k_s64_mdi_obj and the batched solve's k_b64_mdi_obj call it.)
template <int MODE>
__device__ __forceinline__ void s64_mdi_obj_block(double* __restrict__ V, const double* __restrict__ M, const double* __restrict__ Lam,
                                                  long long n_v, double beta, const double* __restrict__ H, int kind, double scalar,
                                                  const double* __restrict__ S, int r, long long n_h, double* __restrict__ part,
                                                  double* red, unsigned bx, unsigned gx) {
    double d = 0.0;
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n_v; i += (long long)gx * 256) {
        const double lam = Lam[i], v = s64_impute(V[i], M[i], lam);
        V[i] = v;
        d = s64_div_add<MODE>(d, v, lam, beta);
    }
    s64_obj_tail(d, H, kind, scalar, S, r, n_h, part, red, bx, gx);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_s64_mdi_obj(double* __restrict__ V, const double* __restrict__ M, const double* __restrict__ Lam,
                                                     long long n_v, double beta, const double* __restrict__ H, int kind, double scalar,
                                                     const double* __restrict__ S, int r, long long n_h, double* __restrict__ part,
                                                     const int* stop) {
    if (*stop) return;
    __shared__ double red[256];
    s64_mdi_obj_block<MODE>(V, M, Lam, n_v, beta, H, kind, scalar, S, r, n_h, part, red, blockIdx.x, gridDim.x);
}

// cost_check = 0: the re-imputation alone
__device__ __forceinline__ void s64_mdi_impute_span(double* __restrict__ V, const double* __restrict__ M, const double* __restrict__ Lam,
                                                    long long n, unsigned bx, unsigned gx) {
    for (long long i = (long long)bx * 256 + threadIdx.x; i < n; i += (long long)gx * 256) V[i] = s64_impute(V[i], M[i], Lam[i]);
}
static __global__ __launch_bounds__(256) void k_s64_mdi_impute(double* __restrict__ V, const double* __restrict__ M,
                                                               const double* __restrict__ Lam, long long n, const int* stop) {
    if (*stop) return;
    s64_mdi_impute_span(V, M, Lam, n, blockIdx.x, gridDim.x);
}

// The gain-matched final imputation (:296-306 / snmf_mdi_Sm.m:302-309), one wave per frame t (four frames a workgroup):
//   a = sum_f v .* M, b = sum_f lam .* M, Nt = a / max(b, flr),   v_mdi = max(v .* M + Nt .* lam .* (1 - M), flr)
// Lane l sums the rows l, l + 64, ... in row order and the 64 lane sums meet in a fixed butterfly, so the result depends on
// neither the grid nor the timing; the second pass finds the frame in the cache.  Runs after the loop: no stop test.
// Vm may be V itself (every element is read and then written by the same lane).
// (The batched solve launches this kernel and k_s64_mdi_start as they are, on one problem's arrays.)
static __global__ __launch_bounds__(256) void k_s64_mdi_final(const double* V, const double* __restrict__ M, const double* __restrict__ Lam,
                                                              int F, long long T, double* Vm) {
    const int lane = threadIdx.x & 63;
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += (long long)gridDim.x * 4) {  // (wave-uniform)
        const long long o = t * F;
        double a = 0.0, b = 0.0;
        for (int f = lane; f < F; f += 64) {
            const double m = M[o + f];
            a += V[o + f] * m;
            b += Lam[o + f] * m;
        }
        for (int s = 32; s > 0; s >>= 1) {
            a += __shfl_xor(a, s, 64);
            b += __shfl_xor(b, s, 64);
        }
        const double nt = a / fmax(b, kS64Flr);
        for (int f = lane; f < F; f += 64) {
            const double m = M[o + f];
            Vm[o + f] = fmax(V[o + f] * m + nt * Lam[o + f] * (1.0 - m), kS64Flr);
        }
    }
}

// One workgroup: div and cost of iteration `it` from the block partials (fixed order), the objective vectors (:263-264)
// and the convergence test of :272-284 -- on the device, so that the host need not wait for every iteration.
// s64_stop_test returns true in thread 0 when the test fired.
__device__ __forceinline__ bool s64_stop_test(const double* __restrict__ part, int n_part, int it, double conv_eps, double div_scale,
                                              double* __restrict__ divh, double* __restrict__ costh, Solve64State* st, double* red) {
    double d = 0.0, sh = 0.0;
    for (int b = threadIdx.x; b < n_part; b += 256) {
        d += part[2 * b];
        sh += part[2 * b + 1];
    }
    d = s64_block_sum(d, red);
    sh = s64_block_sum(sh, red);
    if (threadIdx.x == 0) {
        const double div = d / div_scale;  // beta (beta - 1) for the generic divergence (:257), else 1
        const double cost = div + sh;
        divh[it - 1] = div;
        costh[it - 1] = cost;
        bool fired = false;
        if (it > 1 && conv_eps > 0.0) {
            const double e = fabs(cost - st->last_cost) / st->last_cost;  // :274 (NaN compares false, as in MATLAB)
            fired = e < conv_eps;
        }
        if (fired) {
            st->n_iter = it;
            st->stop = 1;
        } else {
            st->last_cost = cost;
        }
        return fired;
    }
    return false;
}
static __global__ __launch_bounds__(256) void k_s64_stop(const double* __restrict__ part, int n_part, int it, double conv_eps, double div_scale,
                                                         double* __restrict__ divh, double* __restrict__ costh, Solve64State* st) {
    if (st->stop) return;
    __shared__ double red[256];
    (void)s64_stop_test(part, n_part, it, conv_eps, div_scale, divh, costh, st, red);
}

}  // namespace snmf
