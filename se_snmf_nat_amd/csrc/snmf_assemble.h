// snmf_assemble.h -- the training signal of every class assembled on the device from the clips as they come off disk
// (snmf_tu_assemble.hip: snmf_train_signals_*; snmf_tu_frontend_batch.hip: snmf_run_basis_train_signals_batch_*).
//   run_basis_train.m:26-27     s = wavread(.) * 32767 (int16 PCM: pcm / 32768 * 32767, exact in double)   AsmIn<int16_t>
//   src/vadenergy_simple.m:11   bg_mean = mean(|s(1:bg_len)|)                                                k_asm_bg
//   src/vadenergy_simple.m:19-32  half-overlapping frames, (mean - bg_mean) / mean > thr                    k_asm_frames
//   run_basis_train.m:37        nonzeros(s .* vad)                                    } the keep predicate  k_asm_keep
//   run_basis_train.m:40, :42   s(v_start:v_end), s(1:train_file_len_max)             }                      (and k_asm_dev, k_asm_write)
//   run_basis_train.m:44        var(s): two passes, N - 1                                                    k_asm_keep (sums), k_asm_sum, k_asm_dev
//   run_basis_train.m:45        max(|s|)                                                                     k_asm_dev
//   run_basis_train.m:46-57     append, cut at train_seq_len_max, stop                                       k_asm_place
//   run_basis_train.m:44-45     s / sqrt(var) / max|.| * 30000, into s_full                                  k_asm_write
// Every kernel is driven by device tables: AsmClip per clip (where it lies in the input slab, its mode and range, its first work
// block and first VAD frame) and AsmClass per class.  A work block is kAsmSpan samples of one clip; a workgroup finds its clip by
// a binary search of the block prefix sums (uniform loads, log2 n steps), as k_stft_grp finds its signal.  The whole assembly is
// ten launches, whatever the number of classes and clips.
// The kept samples are not stored: k_asm_keep, k_asm_dev and k_asm_write each recompute the predicate from the clip and the frame
// flags (asm_load_keep), k_asm_keep counts them per block, k_asm_scan_* turn the counts into offsets (block sums, a scan of the
// sums, apply: no workgroup waits on another), and k_asm_write ranks its own samples with a scan inside the workgroup.
// Sums.  Per thread in sample order, then the wave's shuffle tree, then the waves in order (block_sum_d); the blocks of a clip
// strided over a workgroup's threads in block order, then the same tree.  No floating-point atomics: the signals are the same
// bits from run to run.  The summation order is not MATLAB's (nor NumPy's); DESIGN.md says what that can move.
// The kernels that are no templates are static: the header is included by two translation units.
// Loads.  A thread reads kAsmVec = 8 consecutive samples at an index that is a multiple of 8 in the INPUT SLAB (16 bytes of
// int16, aligned), so a block starts at the clip's first sample rounded down to 8; samples of the neighbouring clip in the
// vector are masked.  The slab is allocated 8 samples beyond its end rounded up to 8.  Sample indices are 64-bit throughout.
#pragma once
#include "snmf_online_common.h"

#include <vector>

namespace snmf {

constexpr int kAsmVec = 8;               // samples of a thread
constexpr int kAsmSpan = 256 * kAsmVec;  // samples of a work block (one workgroup)
constexpr int kAsmScan = 1024;           // work blocks of a scan group (256 threads x 4)

struct AsmClip {
    int64_t in0;     // first sample in the input slab
    int64_t len;     // samples
    int64_t lo, hi;  // modes 0 and 2: the samples [lo, hi) are kept (0-based); mode 1: [0, len)
    int64_t blk0;    // work blocks of the clips before it
    int64_t fr0;     // VAD frames of the clips before it
    int32_t cls, mode;
    int32_t nfr;     // VAD frames (mode 1: max(0, floor(len / shift) - 1), else 0)
    int32_t pad_;
};
struct AsmClass {
    int64_t out0;  // first sample of the class's segment of the signal slab
    int32_t clip0, n_clips;
};

struct AsmArgs {
    const void* in;       // the clips one behind the other, int16 or double
    const AsmClip* clip;  // [n_clips + 1]: the last entry holds the totals (blk0, fr0)
    const AsmClass* cls;
    int n_clips, n_classes;
    int shift, bg_len;    // frame_len = 2 * shift
    double thr;
    int64_t seq_max;
    int64_t n_blocks, n_frames, n_groups;
    uint8_t* flag;                   // [n_frames]
    int32_t* bcnt;                   // [n_groups * kAsmScan] kept samples per work block (zero beyond n_blocks)
    int64_t* bscan;                  // [n_groups * kAsmScan] their exclusive scan over ALL blocks
    int64_t* gsum;                   // [n_groups]
    double *bsum, *bdev, *bmax;      // [n_blocks]
    double *bg, *mean, *sd, *pk;     // [n_clips]
    int64_t *kept, *dst;             // [n_clips]; dst: where the clip starts in its class, -1: nothing of it is written
    int64_t* clen;                   // [n_classes]
    int32_t *used, *bad;             // [n_classes]; bad: the first clip (within the class) without a positive finite variance, or -1
    double* out;                     // the signal slab
};

template <typename T>
struct AsmIn;
template <>
struct AsmIn<int16_t> {
    static __device__ __forceinline__ double one(const void* in, int64_t i) { return (double)((const int16_t*)in)[i] / 32768.0 * 32767.0; }
    static __device__ __forceinline__ void vec(const void* in, int64_t i8, double* v) {
        const uint4 q = *(const uint4*)((const int16_t*)in + i8);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = (double)(int16_t)(w[e] & 0xffffu) / 32768.0 * 32767.0;
            v[2 * e + 1] = (double)(int16_t)(w[e] >> 16) / 32768.0 * 32767.0;
        }
    }
};
template <>
struct AsmIn<double> {
    static __device__ __forceinline__ double one(const void* in, int64_t i) { return ((const double*)in)[i]; }
    static __device__ __forceinline__ void vec(const void* in, int64_t i8, double* v) {
        const double2* p = (const double2*)((const double*)in + i8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double2 d = p[e];
            v[2 * e] = d.x, v[2 * e + 1] = d.y;
        }
    }
};

// the clip whose work blocks (BLOCKS) or VAD frames hold number g of the launch: the last one with blk0 / fr0 <= g
template <bool BLOCKS>
__device__ __forceinline__ int asm_find(const AsmClip* __restrict__ clip, int n, int64_t g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((BLOCKS ? clip[mid].blk0 : clip[mid].fr0) <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The 8 samples of this thread in work block lb of clip c, and which of them are kept (bit e: v[e]).
template <typename T>
__device__ __forceinline__ unsigned asm_load_keep(const AsmArgs& a, const AsmClip& c, int64_t lb, double* v) {
    const int64_t i8 = (c.in0 & ~(int64_t)7) + lb * kAsmSpan + (int64_t)threadIdx.x * kAsmVec;
    const int64_t rel = i8 - c.in0;  // >= -7
    if (rel >= c.len) return 0u;
    AsmIn<T>::vec(a.in, i8, v);
    unsigned m = 0u;
    if (c.mode == 1) {  // voiced in either covering frame (hop j: frames j - 1 and j), and not exactly zero
        const uint8_t* __restrict__ fl = a.flag + c.fr0;
        const int64_t q = rel > 0 ? rel : 0;
        int64_t j = q / a.shift;
        int r = (int)(q - j * a.shift);
        bool fa = j >= 1 && j - 1 < c.nfr && fl[j - 1], fb = j < c.nfr && fl[j];
#pragma unroll
        for (int e = 0; e < kAsmVec; ++e) {
            const int64_t i = rel + e;
            if (i < 0 || i >= c.len) continue;
            if ((fa || fb) && v[e] != 0.0) m |= 1u << e;
            if (++r == a.shift) {
                r = 0, ++j;
                fa = fb, fb = j < c.nfr && fl[j];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < kAsmVec; ++e) {
            const int64_t i = rel + e;
            if (i >= c.lo && i < c.hi) m |= 1u << e;
        }
    }
    return m;
}

__device__ __forceinline__ int64_t asm_block_sum_i(int64_t v, int64_t* red /*[4]*/) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
// exclusive prefix of v over the 256 threads of the workgroup
__device__ __forceinline__ int64_t asm_block_excl(int64_t v, int64_t* red /*[4]*/) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int64_t base = 0;
    for (int i = 0; i < w; ++i) base += red[i];
    return base + inc - v;
}

// src/vadenergy_simple.m:11 -- one workgroup per clip
template <typename T>
__global__ __launch_bounds__(256) void k_asm_bg(AsmArgs a) {
    __shared__ double red[4];
    const int ci = blockIdx.x;
    if (ci >= a.n_clips) return;
    const AsmClip c = a.clip[ci];
    if (c.mode != 1) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < a.bg_len; i += 256) s += fabs(AsmIn<T>::one(a.in, c.in0 + i));  // (bg_len <= len: checked on the host)
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) a.bg[ci] = s / (double)a.bg_len;
}

// src/vadenergy_simple.m:24-32 -- one wave per frame: frame k of a clip covers its samples [k * shift, k * shift + 2 * shift)
template <typename T>
__global__ __launch_bounds__(256) void k_asm_frames(AsmArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.n_frames) return;
    const int ci = asm_find<false>(a.clip, a.n_clips, g);
    const AsmClip c = a.clip[ci];
    const int64_t k = g - c.fr0;
    if (k >= c.nfr) return;
    const int64_t s0 = c.in0 + k * a.shift;  // (k + 2) * shift <= len: nfr = floor(len / shift) - 1
    const int fl = 2 * a.shift;
    double s = 0.0;
    for (int i = threadIdx.x & 63; i < fl; i += 64) s += fabs(AsmIn<T>::one(a.in, s0 + i));
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) {
        const double m = s / (double)fl;
        a.flag[g] = ((m - a.bg[ci]) / m > a.thr) ? 1 : 0;  // 0/0 and -inf compare false (:27)
    }
}

// the keep predicate: kept samples and their sum per work block
template <typename T>
__global__ __launch_bounds__(256) void k_asm_keep(AsmArgs a) {
    __shared__ double red[4];
    __shared__ int64_t redi[4];
    const int64_t b = blockIdx.x;
    if (b >= a.n_blocks) return;
    const int ci = asm_find<true>(a.clip, a.n_clips, b);
    const AsmClip c = a.clip[ci];
    double v[kAsmVec];
    const unsigned m = asm_load_keep<T>(a, c, b - c.blk0, v);
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < kAsmVec; ++e)
        if (m >> e & 1u) s += v[e];
    const int64_t n = asm_block_sum_i((int64_t)__popc(m), redi);
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) a.bcnt[b] = (int32_t)n, a.bsum[b] = s;
}

// exclusive scan of bcnt over all work blocks in three launches: the sum of every group of kAsmScan blocks ...
static __global__ __launch_bounds__(256) void k_asm_scan_sums(AsmArgs a) {
    __shared__ int64_t redi[4];
    const int64_t g = blockIdx.x;
    if (g >= a.n_groups) return;
    const int32_t* p = a.bcnt + g * kAsmScan + threadIdx.x * 4;
    const int64_t s = asm_block_sum_i((int64_t)p[0] + p[1] + p[2] + p[3], redi);
    if (threadIdx.x == 0) a.gsum[g] = s;
}
// ... the exclusive scan of those sums, in place, by one workgroup (a slice per thread) ...
static __global__ __launch_bounds__(256) void k_asm_scan_top(AsmArgs a) {
    __shared__ int64_t part[256];
    const int64_t per = (a.n_groups + 255) / 256;
    const int64_t lo = per * threadIdx.x < a.n_groups ? per * threadIdx.x : a.n_groups, hi = lo + per < a.n_groups ? lo + per : a.n_groups;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += a.gsum[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t x = part[i];
            part[i] = run, run += x;
        }
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t x = a.gsum[i];
        a.gsum[i] = run, run += x;
    }
}
// ... and every group scans its own blocks behind its base
static __global__ __launch_bounds__(256) void k_asm_scan_apply(AsmArgs a) {
    __shared__ int64_t redi[4];
    const int64_t g = blockIdx.x;
    if (g >= a.n_groups) return;
    const int64_t i0 = g * kAsmScan + threadIdx.x * 4;
    const int32_t* p = a.bcnt + i0;
    const int64_t c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3];
    int64_t run = a.gsum[g] + asm_block_excl(c0 + c1 + c2 + c3, redi);
    a.bscan[i0] = run, run += c0;
    a.bscan[i0 + 1] = run, run += c1;
    a.bscan[i0 + 2] = run, run += c2;
    a.bscan[i0 + 3] = run;
}

// the blocks of a clip in block order, strided over the threads: sum (MAX: maximum) of x[b0 .. b1), in every thread
template <bool MAX>
__device__ __forceinline__ double asm_fold(const double* __restrict__ x, int64_t b0, int64_t b1, double* red) {
    double s = 0.0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) s = MAX ? fmax(s, x[i]) : s + x[i];
    return MAX ? block_max<double>(s, red) : block_sum_d(s, red);
}

// kept samples and mean of every clip -- one workgroup per clip
static __global__ __launch_bounds__(256) void k_asm_sum(AsmArgs a) {
    __shared__ double red[4];
    const int ci = blockIdx.x;
    if (ci >= a.n_clips) return;
    const int64_t b0 = a.clip[ci].blk0, b1 = a.clip[ci + 1].blk0;
    const int64_t n = a.bscan[b1] - a.bscan[b0];
    const double s = asm_fold<false>(a.bsum, b0, b1, red);
    if (threadIdx.x == 0) a.kept[ci] = n, a.mean[ci] = n > 0 ? s / (double)n : 0.0;
}

// squared deviations from the clip's mean and max|s| per work block
template <typename T>
__global__ __launch_bounds__(256) void k_asm_dev(AsmArgs a) {
    __shared__ double red[4];
    const int64_t b = blockIdx.x;
    if (b >= a.n_blocks) return;
    const int ci = asm_find<true>(a.clip, a.n_clips, b);
    const AsmClip c = a.clip[ci];
    const double mu = a.mean[ci];
    double v[kAsmVec];
    const unsigned m = asm_load_keep<T>(a, c, b - c.blk0, v);
    double s = 0.0, mx = 0.0;
#pragma unroll
    for (int e = 0; e < kAsmVec; ++e)
        if (m >> e & 1u) {
            const double d = v[e] - mu;
            s += d * d;
            mx = fmax(mx, fabs(v[e]));
        }
    s = block_sum_d(s, red);
    mx = block_max<double>(mx, red);
    if (threadIdx.x == 0) a.bdev[b] = s, a.bmax[b] = mx;
}

// run_basis_train.m:44-57 per class -- one workgroup per class walks its clips in order: standard deviation and peak of the clip,
// where it goes, the cut at seq_max and the stop.  Every thread computes the same values, so the loop is uniform.
static __global__ __launch_bounds__(256) void k_asm_place(AsmArgs a) {
    __shared__ double red[4];
    const int k = blockIdx.x;
    if (k >= a.n_classes) return;
    const AsmClass cl = a.cls[k];
    int64_t L = 0;
    int32_t used = 0, bad = -1;
    for (int i = 0; i < cl.n_clips; ++i) {
        const int ci = cl.clip0 + i;
        const int64_t n = a.kept[ci];
        used = i + 1;
        if (n == 0) continue;  // an empty vector is appended (:47)
        const int64_t b0 = a.clip[ci].blk0, b1 = a.clip[ci + 1].blk0;
        const double var = asm_fold<false>(a.bdev, b0, b1, red) / (double)(n - 1);  // (n = 1: 0/0)
        const double mx = asm_fold<true>(a.bmax, b0, b1, red);
        if (!(var > 0.0) || isinf(var)) {
            bad = i;
            break;
        }
        const double sd = sqrt(var);
        if (threadIdx.x == 0) a.sd[ci] = sd, a.pk[ci] = mx / sd, a.dst[ci] = L;  // max|s / sd| = fl(max|s| / sd): both monotone
        L += n;
        if (L > a.seq_max) {  // :50-53
            L = a.seq_max;
            break;
        }
    }
    if (threadIdx.x == 0) a.clen[k] = L, a.used[k] = used, a.bad[k] = bad;
}

// run_basis_train.m:44-47 -- normalise the kept samples and put them where they belong, up to the class's cut
template <typename T>
__global__ __launch_bounds__(256) void k_asm_write(AsmArgs a) {
    __shared__ int64_t redi[4];
    const int64_t b = blockIdx.x;
    if (b >= a.n_blocks) return;
    const int ci = asm_find<true>(a.clip, a.n_clips, b);
    const AsmClip c = a.clip[ci];
    const int64_t d0 = a.dst[ci];
    if (d0 < 0) return;
    const int64_t L = a.clen[c.cls];
    const int64_t at = d0 + (a.bscan[b] - a.bscan[c.blk0]);
    if (at >= L) return;
    double v[kAsmVec];
    const unsigned m = asm_load_keep<T>(a, c, b - c.blk0, v);
    int64_t d = at + asm_block_excl((int64_t)__popc(m), redi);
    const double sd = a.sd[ci], pk = a.pk[ci];
    double* __restrict__ o = a.out + a.cls[c.cls].out0;
#pragma unroll
    for (int e = 0; e < kAsmVec; ++e)
        if (m >> e & 1u) {
            if (d < L) o[d] = v[e] / sd / pk * 30000.0;
            ++d;
        }
}

// The resident signals into the grouped front-end's sample slab: a copy for double, round to nearest for float.
struct SigCopy {
    int64_t src0, dst0, n;
};
template <typename S>
__global__ __launch_bounds__(256) void k_sig_fill(const double* __restrict__ src, const SigCopy* __restrict__ tab, S* __restrict__ dst) {
    const SigCopy t = tab[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (int64_t)gridDim.x * 256) dst[t.dst0 + i] = (S)src[t.src0 + i];
}

}  // namespace snmf

// the handle of include/snmf.h: the signal slab in HBM and what the host knows about it
struct snmf_train_signals {
    snmf_ctx* ctx = nullptr;
    int device = 0;  // (the context's: destroy does not look at the context)
    double* slab = nullptr;
    std::vector<int64_t> out0, len;  // per class: first sample in the slab, samples
    std::vector<int32_t> used;       // per class: clips_used
};
