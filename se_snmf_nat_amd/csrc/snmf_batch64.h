// ============================================================================================
// The batched offline solve in the fp64 mode (snmf_batch_create_fp64, snmf_batch_create_ranks_fp64): B independent problems of
// one F, each with a frame count T_b and a rank r_b of its own (one r for all on a handle made without
// ranks), each the fp64 solve of snmf_solve64.h, in SHARED launches.  The arrays of a problem are the single solve's -- tight,
// column-major, nothing padded, 64-bit offsets -- and the problems lie one behind the other: V, Lam, R, D are F x sum(T_b);
// H, Num, Den are the r_b x T_b matrices packed at sum(r_j T_j); W, Q, P the F x r_b matrices packed at F sum(r_j); the column
// norms, column sums and row sums r_b entries at sum(r_j); and every problem has its own row-sum partials, objective partials,
// objective history and Solve64State.  The offsets are prefix sums kept per problem (B64Prob): no kernel multiplies by "the" r.
// Every kernel here is a grid of the single solve's workgroups with one more index, the problem: it finds the problem's
// arrays and calls the __device__ body the single solve's kernel calls (snmf_solve64.h), with the workgroup index and the
// grid size that kernel would have had.  So every element, every partial sum and every tree is formed by the same
// expression in the same order, and a problem's bits are those of snmf_sparse_nmf_fp64 on it alone.
// A workgroup returns at once when its problem's stop word is set.
// The settings of a solve -- divergence, sparsity weight, stop threshold, iteration limit -- are entries of B64Prob too
// (snmf_batch_create_settings_fp64 gives every problem its own; otherwise they are filled from the one settings struct, and the
// expressions and operands are the same).  A pass that is compiled per divergence is launched once per divergence present, and
// a workgroup returns at once when its problem's mode is not the launch's: the pattern of the stop word.
// ============================================================================================
#pragma once

#include "snmf_philox.h"
#include "snmf_solve64.h"

namespace snmf {

struct B64Prob {
    int T;          // frames of this problem
    int n_rowz;     // its row-sum chunks of kS64RowChunk frames
    int r;          // its rank
    long long fr0;  // frames of the problems before it
    long long rz0;  // row-sum chunks of the problems before it
    long long h0;   // H elements of the problems before it: sum r_j T_j
    long long w0;   // W columns of the problems before it: sum r_j
    long long sp0;  // row-sum partials of the problems before it: sum r_j n_rowz_j
    // its settings (those of the one settings struct on a handle made without settings per problem)
    int mode;          // S64_KL / S64_ED / S64_IS / S64_GEN: a pass compiled per mode is launched once per mode present
    int max_iter;      // its iteration limit (B64Args.max_iter is the largest: the stride of the histories)
    double beta, div_scale, sparsity, conv_eps;
};

// one workgroup of a grouped product: problem, 64 x 64 tile of that problem's product, split
struct B64Tile {
    int prob, tile, z;
};

// one split product (or one problem's row sums) whose partials k_b64_sumz adds in split order
struct B64Sum {
    const double* part;
    double* C;
    long long n, rsC, csC;
    int nz, M, do_floor;
    const int* stop;
};

struct B64Args {
    int F, r, kind, max_iter;  // r: the largest rank (the rank, on a uniform batch); max_iter: the largest limit
    int own_limit;             // settings per problem: a problem is stopped and counted when it reaches its own max_iter
    const B64Prob* prob;
    const double* S;  // r-vector sparsity (kind 1)
    double *V, *Lam, *R, *D, *H, *Num, *Den, *W, *Q, *P;
    const double* M;  // the masks of a missing-data batch (F x sum(T_b), at V's frame offsets); nullptr on a plain batch
    double *cs, *hs, *sp, *wn, *part, *divh, *costh;
    const uint8_t* w_ind;
    Solve64State* st;
    int* n_stopped;
};

// The grouped f64-MFMA GEMM: workgroup b takes entry b of a table built from the frame counts when the batch is made --
// the problem, the 64 x 64 tile within that problem's product and the split -- and that problem's Gemm64Args, which are
// the ones gemm64() makes for the problem alone (s64_gemm_plan).  Problems with one split (a direct store, floored there)
// and problems with several (tight partials for k_b64_sumz) share the launch.
static __global__ __launch_bounds__(256) void k_b64_gemm(const Gemm64Args* __restrict__ args, const B64Tile* __restrict__ tiles) {
    const B64Tile t = tiles[blockIdx.x];
    const Gemm64Args g = args[t.prob];
    if (*g.stop) return;
    __shared__ double As[16][64 + 2];
    __shared__ double Bs[16][64 + 2];
    s64_gemm_tile(g, (unsigned)t.tile, t.z, As, Bs);
}

// blockIdx.y: the entry; the elements of an entry are spread over gridDim.x workgroups (each sum is one thread's, in split order)
static __global__ __launch_bounds__(256) void k_b64_sumz(const B64Sum* __restrict__ e) {
    const B64Sum s = e[blockIdx.y];
    if (*s.stop) return;
    s64_sumz_span(s.part, s.nz, s.n, s.M, s.C, s.rsC, s.csC, s.do_floor, blockIdx.x, gridDim.x);
}

// ---- element-wise passes: grid (workgroups, problem); an element's value does not depend on the workgroup that forms it
template <int MODE>
__global__ __launch_bounds__(256) void k_b64_ratio(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    const B64Prob p = a.prob[b];
    if (p.mode != MODE) return;  // (another launch's problem)
    const long long o = p.fr0 * a.F;
    s64_ratio_span<MODE>(a.V + o, a.Lam + o, a.R ? a.R + o : nullptr, a.D ? a.D + o : nullptr, (long long)a.F * p.T, p.beta, blockIdx.x,
                         gridDim.x);
}

// grid (workgroups, B): H0 of problem b of batch `a` (tight a.r x T_b) from rows [row0, row0 + a.r) of the H of another batch with
// the same frame counts (tight r_src x T_b at the same frame offset); consecutive lanes run along k within a frame.  Both batches
// have one rank for all problems (the host refuses the call on a batch with ranks), so h0 = fr0 * r in each.
static __global__ __launch_bounds__(256) void k_b64_take_h(B64Args a, const double* __restrict__ Hsrc, int r_src, int row0) {
    const B64Prob p = a.prob[blockIdx.y];
    const double* __restrict__ S = Hsrc + p.fr0 * r_src + row0;
    double* __restrict__ H = a.H + p.fr0 * a.r;
    const long long n = (long long)a.r * p.T;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long t = i / a.r;
        const int k = (int)(i - t * a.r);
        H[i] = S[t * r_src + k];
    }
}

// grid (workgroups, B): the same hand-over between two batches whose problems have ranks of their own.  H0 of problem b of batch
// `a` (tight r_b x T_b at its own B64Prob::h0) from rows [row0[b], row0[b] + r_b) of problem b's H in the source batch (tight
// rs_b x T_b at the source's own h0): `src` is the source's table of problems, Hsrc its H, row0 a device array with one entry per
// problem.  A flat index over the r_b T_b elements, consecutive lanes along k within a frame, so that a problem of rank one
// keeps every lane busy.  The host has checked equal frame counts and 0 <= row0[b], row0[b] + r_b <= rs_b.  A copy: no
// arithmetic, nothing shared between workgroups.
static __global__ __launch_bounds__(256) void k_b64_take_h_rows(B64Args a, const B64Prob* __restrict__ src, const double* __restrict__ Hsrc,
                                                                const int32_t* __restrict__ row0) {
    const int b = blockIdx.y;
    const B64Prob p = a.prob[b];
    const B64Prob q = src[b];
    const int r = p.r, rs = q.r;
    const double* __restrict__ S = Hsrc + q.h0 + row0[b];
    double* __restrict__ H = a.H + p.h0;
    const long long n = (long long)r * p.T;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long t = i / r;
        const int k = (int)(i - t * r);
        H[i] = S[t * rs + k];
    }
}

// grid (workgroups, B): init_w of problem b = V_b(:, idx[w0_b + k]), k < r_b (run_basis_train.m:82-83; k_gather64 per problem):
// columns of the problem's own tight V block into its tight F x r_b W.  idx: 0-based, on the device, the problems' r_b entries
// packed one behind the other; an index outside [0, T_b) (the host refuses it) gives a zero column, never a read outside the block.
static __global__ __launch_bounds__(256) void k_b64_take_w(B64Args a, const int64_t* __restrict__ idx) {
    const int b = blockIdx.y;
    const B64Prob p = a.prob[b];
    const double* __restrict__ V = a.V + p.fr0 * a.F;
    double* __restrict__ W = a.W + p.w0 * a.F;
    const long long n = (long long)a.F * p.r;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long k = i / a.F, f = i - k * a.F;
        const long long t = idx[p.w0 + k];
        W[i] = (t >= 0 && t < p.T) ? V[t * a.F + f] : 0.0;
    }
}

// grid (workgroups, B): H0 of problem b drawn on the device: H[e] = u(e), e the element index in the tight column-major r_b x T_b
// matrix -- k_rand64 (snmf_frontend64.h) per problem, keyed by seed[b].  draw[b] == 0: the problem's H0 came from the host.
static __global__ __launch_bounds__(256) void k_b64_rand_h(B64Args a, const uint64_t* __restrict__ seed, const uint8_t* __restrict__ draw) {
    const int b = blockIdx.y;
    if (!draw[b]) return;
    const B64Prob p = a.prob[b];
    const uint64_t sd = seed[b], n = (uint64_t)p.r * (uint64_t)p.T, n4 = (n + 3) / 4;
    double* __restrict__ H = a.H + p.h0;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (uint64_t)gridDim.x * 256) {
        uint32_t o[4];
        philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t e = 4 * q + j;
            if (e < n) H[e] = ((double)(o[j] >> 9) + 0.5) * (1.0 / 8388608.0);
        }
    }
}

template <bool KL>
__global__ __launch_bounds__(256) void k_b64_hupd(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    const B64Prob p = a.prob[b];
    if ((p.mode == S64_KL) != KL) return;
    const long long o = p.h0;
    s64_hupd_span<KL>(a.H + o, a.Num + o, KL ? nullptr : a.Den + o, KL ? a.cs + p.w0 : nullptr, a.kind, p.sparsity, a.S, p.r,
                      (long long)p.r * p.T, blockIdx.x, gridDim.x);
}

// ---- reductions: the single solve's partition per problem
// grid (the largest r, B): column sums of W_b; the workgroups past the problem's own r_b columns return
static __global__ __launch_bounds__(256) void k_b64_colsum(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    const B64Prob p = a.prob[b];
    if (p.mode != S64_KL || (int)blockIdx.x >= p.r) return;
    __shared__ double red[256];
    s64_colsum_col(a.W + p.w0 * a.F, a.F, a.cs + p.w0, (int)blockIdx.x, red);
}

// grid (ceil(the largest r / 256), the largest chunk count, B): the row-sum partials of H_b; k_b64_sumz adds them
static __global__ __launch_bounds__(256) void k_b64_rowsum(B64Args a) {
    const int b = blockIdx.z;
    if (a.st[b].stop) return;
    const B64Prob p = a.prob[b];
    if (p.mode != S64_KL || (int)blockIdx.y >= p.n_rowz) return;
    s64_rowsum_chunk(a.H + p.h0, p.r, p.T, kS64RowChunk, a.sp + p.sp0, (int)blockIdx.y, blockIdx.x, gridDim.x);
}

// grid (the largest r, B): the W epilogue of problem b, column k < r_b (w_ind: one mask for all problems; with ranks it is uniform)
template <bool KL>
__global__ __launch_bounds__(256) void k_b64_wupd(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    const B64Prob p = a.prob[b];
    if ((p.mode == S64_KL) != KL || (int)blockIdx.x >= p.r) return;
    __shared__ double red[256];
    const long long o = p.w0 * a.F;
    s64_wupd_col<KL, true>(a.W + o, a.Q + o, KL ? nullptr : a.P + o, KL ? a.hs + p.w0 : nullptr, a.w_ind, a.F, nullptr,
                           (int)blockIdx.x, red);
}

// grid (kS64Blocks, B): the objective partials of problem b, the single solve's kS64Blocks slots and element assignment
template <int MODE>
__global__ __launch_bounds__(256) void k_b64_obj(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    __shared__ double red[256];
    const B64Prob p = a.prob[b];
    if (p.mode != MODE) return;  // (uniform over the workgroup, before any barrier)
    const long long o = p.fr0 * a.F;
    s64_obj_block<MODE>(a.V + o, a.Lam + o, (long long)a.F * p.T, p.beta, a.H + p.h0, a.kind, p.sparsity, a.S, p.r,
                        (long long)p.r * p.T, a.part + (long long)b * 2 * kS64Blocks, red, blockIdx.x, gridDim.x);
}

// ---- the missing-data steps of a masked batch (snmf_batch_create_mdi_fp64): the bodies of k_s64_mdi_impute / k_s64_mdi_obj
// grid (workgroups, B): the re-imputation alone (cost_check = 0).  V and Lam of a stopped problem stay those of its stop iterate.
static __global__ __launch_bounds__(256) void k_b64_mdi_impute(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    const B64Prob p = a.prob[b];
    const long long o = p.fr0 * a.F;
    s64_mdi_impute_span(a.V + o, a.M + o, a.Lam + o, (long long)a.F * p.T, blockIdx.x, gridDim.x);
}

// grid (kS64Blocks, B): the re-imputation fused with the objective of the imputed v, in the place of k_b64_obj
template <int MODE>
__global__ __launch_bounds__(256) void k_b64_mdi_obj(B64Args a) {
    const int b = blockIdx.y;
    if (a.st[b].stop) return;
    __shared__ double red[256];
    const B64Prob p = a.prob[b];
    if (p.mode != MODE) return;
    const long long o = p.fr0 * a.F;
    s64_mdi_obj_block<MODE>(a.V + o, a.M + o, a.Lam + o, (long long)a.F * p.T, p.beta, a.H + p.h0, a.kind, p.sparsity, a.S, p.r,
                            (long long)p.r * p.T, a.part + (long long)b * 2 * kS64Blocks, red, blockIdx.x, gridDim.x);
}

// grid (B): the fixed tree over problem b's partials, its objective vectors and its stop test (src/sparse_nmf.m:272-284);
// a problem that stops counts itself in n_stopped, which is all the host polls.  With settings per problem (own_limit) a problem
// whose test has not fired at its own max_iter is stopped there too, after its objective is recorded: n_iter = max_iter_b, the
// value the single solve reports at the end of its loop.  (Thread 0 alone holds `fired` and writes the state.)
static __global__ __launch_bounds__(256) void k_b64_stop(B64Args a, int it) {
    const int b = blockIdx.x;
    if (a.st[b].stop) return;
    __shared__ double red[256];
    const B64Prob p = a.prob[b];
    bool fired = s64_stop_test(a.part + (long long)b * 2 * kS64Blocks, kS64Blocks, it, p.conv_eps, p.div_scale,
                               a.divh + (long long)b * a.max_iter, a.costh + (long long)b * a.max_iter, a.st + b, red);
    if (threadIdx.x == 0 && !fired && a.own_limit && it == p.max_iter) {
        a.st[b].n_iter = it;
        a.st[b].stop = 1;
        fired = true;
    }
    if (fired) atomicAdd(a.n_stopped, 1);
}

// grid (ceil(B / 256)): the iteration limit of its own without the objective (cost_check = 0, settings per problem): thread b
// stops problem b after iteration it == max_iter_b and counts it.  An integer counter, and nobody waits on anybody.
static __global__ __launch_bounds__(256) void k_b64_limit(B64Args a, int n_problems, int it) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_problems || a.st[b].stop || a.prob[b].max_iter != it) return;
    a.st[b].n_iter = it;
    a.st[b].stop = 1;
    atomicAdd(a.n_stopped, 1);
}

}  // namespace snmf
