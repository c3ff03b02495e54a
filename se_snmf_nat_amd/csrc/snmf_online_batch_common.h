// snmf_online_batch_common.h -- what the batched online separator's two precisions share on the device, each written
// once over the mode's element type T (float / double): the per-chunk framing of the streams and the gate of the adaptation
// launches, the restart of the listed streams' shared arrays (orestart_common), the re-assembly (oassemble_cols), the
// synthesis (k_obtail<T>, k_obistft<LOGN, T>, k_obola<T>) and get-state / set-state (ostate_xfer).  A kernel template is
// instantiated by the one translation unit that launches it with its T, so no symbol is emitted from both units.
// Included by snmf_online_batch.h (fp32) and snmf_online_batch_f64.h (fp64).
#pragma once
#include "snmf_online_common.h"

namespace snmf {

// per-stream, per-chunk framing (host-computed, uploaded once per chunk)
struct OBatchFrames {
    const int* nfr;        // [S] frames of stream s in this chunk
    const int* nreal;      // [S] of which the first nreal come from PCM (the rest are the all-zero flush frames)
    const int64_t* off;    // [S] sample offset of stream s's [history | hops] in the signal buffer
    const int64_t* zoff;   // [S] offset of sz zero samples (the flush frames, src/NTF_sep_event_RT.m:69-76)
    const int* l0;         // [S] 1-based index of stream s's first frame of the chunk
    int S;
};

// the adaptation of stream s is due at frame `step`: the post-filter said so (:294, sum(r_up) > 0)
__device__ __forceinline__ bool ob_due(const OnlineStatus* status, const int* nfr, int step, int S, int s) {
    if (step >= nfr[s]) return false;
    const OnlineStatus& st = status[(size_t)step * S + s];
    return st.do_solve && st.n_up > 0;
}

// ---------------------------------------------------------------------------------------------
// Get-state / set-state (snmf_online_batch_get_state / _set_state): the listed streams' arrays gathered into / scattered
// from one staging slab of records (include/snmf.h: snmf_online_state_field gives the layout).  Grid (listed stream, array,
// part) as the restart: each workgroup moves one part of one array of one listed stream with plain loads and stores, and
// no workgroup reads what another writes.  The rings cross in time order: column c of lambda_d_blk / Ad_blk lives in slot
// (n_push + c) % ma, column c of r_blk in slot (l - 1 + c) % Pl (snmf_online_common.h: the post-filter writes the newest
// column over the oldest), so a put leaves every column in the slot it had.
// ---------------------------------------------------------------------------------------------
enum : int {
    kStXm, kStLam, kStRblk, kStLdblk, kStAdblk, kStBd, kStBfix, kStBmd, kStH0, kStAd0, kStTail, kStTailX, kStTailD, kStTailC,
    kStDev, kStBdf, kStN
};
constexpr int kStParts = 8;  // workgroups per (stream, array)

template <typename T>
struct OStateArgs {
    const int* slots;       // [n] the listed streams (distinct, in range: checked on the host)
    const int64_t* l;       // [n] 1-based index of each listed stream's next frame (get); NULL: read from the record (put)
    unsigned char* slab;    // [n] records, `stride` bytes each (a multiple of 8)
    int64_t stride;
    int64_t off[kStN];      // byte offset of each array in a record (kStDev: n_push, update_switch behind it)
    int64_t off_l;          // of the record's l
    T *Xm_tilde, *lambda_dav, *r_blk, *ldblk, *adblk, *H0, *Ad0, *tail, *tail_x, *tail_d, *tail_c;  // tail_x / _d / _c may be NULL
    double *B, *Bfix;       // [S][r][F], [S][Rd][F]
    double* Bm;             // Mel mode: [S][r][n1], else NULL
    float* Bdf;             // Mel mode with MelConv = 0: [S][r][F] fp32, else NULL
    OnlineDev* dev;
    int S, F, r, Rx, Rd, Ra, ma, Pl, n1, n_cls;
    int64_t ntail;
};

template <typename T, bool PUT>
__device__ __forceinline__ void ostate_xfer(const OStateArgs<T>& a) {
    const int i = blockIdx.x, arr = blockIdx.y, s = a.slots[i];
    const size_t F = a.F, q0 = (size_t)blockIdx.z * 256 + threadIdx.x, qs = (size_t)kStParts * 256;
    unsigned char* rec = a.slab + (size_t)i * a.stride;
    // dev[e] <-> record element e
    auto lin = [&](auto* dev, int k, size_t n) {
        auto* p = reinterpret_cast<std::remove_reference_t<decltype(dev)>>(rec + a.off[k]);
        for (size_t e = q0; e < n; e += qs) {
            if (PUT) dev[e] = p[e];
            else p[e] = dev[e];
        }
    };
    // a ring of `cols` columns of `rows`: record column c <-> device slot (first + c) % cols
    auto ring = [&](T* dev, int k, size_t rows, int cols, int first) {
        T* p = reinterpret_cast<T*>(rec + a.off[k]);
        for (size_t e = q0; e < rows * cols; e += qs) {
            const int c = (int)(e / rows);
            const size_t f = e - (size_t)c * rows, d = (size_t)((first + c) % cols) * rows + f;
            if (PUT) dev[d] = p[e];
            else p[e] = dev[d];
        }
    };
    int* rdev = reinterpret_cast<int*>(rec + a.off[kStDev]);
    const size_t nA = (size_t)a.Ra * a.ma;
    switch (arr) {
        case kStXm: lin(a.Xm_tilde + s * F, kStXm, F); break;
        case kStLam: lin(a.lambda_dav + s * F, kStLam, F); break;
        case kStRblk: {
            const int64_t l = a.l ? a.l[i] : *reinterpret_cast<const int64_t*>(rec + a.off_l);
            ring(a.r_blk + s * F * a.Pl, kStRblk, F, a.Pl, (int)((l - 1) % a.Pl));
            break;
        }
        case kStLdblk: ring(a.ldblk + s * F * a.ma, kStLdblk, F, a.ma, (PUT ? rdev[0] : a.dev[s].n_push) % a.ma); break;
        case kStAdblk: ring(a.adblk + s * nA, kStAdblk, (size_t)a.Ra, a.ma, (PUT ? rdev[0] : a.dev[s].n_push) % a.ma); break;
        case kStBd: lin(a.B + (size_t)s * a.r * F + (size_t)a.Rx * F, kStBd, (size_t)a.Rd * F); break;
        case kStBfix: lin(a.Bfix + (size_t)s * a.Rd * F, kStBfix, (size_t)a.Rd * F); break;
        case kStBmd:
            if (a.Bm) lin(a.Bm + (size_t)s * a.r * a.n1 + (size_t)a.Rx * a.n1, kStBmd, (size_t)a.Rd * a.n1);
            break;
        case kStH0: lin(a.H0 + (size_t)s * a.r, kStH0, (size_t)a.r); break;
        case kStAd0: lin(a.Ad0 + s * nA, kStAd0, nA); break;
        case kStTail: lin(a.tail + s * a.ntail, kStTail, (size_t)a.ntail); break;
        case kStTailX:
            if (a.tail_x) lin(a.tail_x + s * a.ntail, kStTailX, (size_t)a.ntail);
            break;
        case kStTailD:
            if (a.tail_d) lin(a.tail_d + s * a.ntail, kStTailD, (size_t)a.ntail);
            break;
        case kStTailC:  // [n_cls][S][ntail] on the device, [n_cls][ntail] in the record
            if (a.tail_c) {
                T* p = reinterpret_cast<T*>(rec + a.off[kStTailC]);
                for (size_t e = q0; e < (size_t)a.n_cls * a.ntail; e += qs) {
                    const size_t c = e / (size_t)a.ntail, d = (c * a.S + s) * a.ntail + (e - c * a.ntail);
                    if (PUT) a.tail_c[d] = p[e];
                    else p[e] = a.tail_c[d];
                }
            }
            break;
        case kStDev:
            if (q0 == 0) {
                if (PUT) {
                    a.dev[s] = OnlineDev{rdev[0], rdev[1], 0, 0};
                } else {
                    rdev[0] = a.dev[s].n_push;
                    rdev[1] = a.dev[s].update_switch;
                }
            }
            break;
        default:  // kStBdf: the fp32 image of the record's B_DFT_d, as k_obrestart's kRsBdf rounds a new dictionary
            if (PUT && a.Bdf) {
                const double* p = reinterpret_cast<const double*>(rec + a.off[kStBd]);
                float* d = a.Bdf + (size_t)s * a.r * F + (size_t)a.Rx * F;
                for (size_t e = q0; e < (size_t)a.Rd * F; e += qs) d[e] = (float)p[e];
            }
    }
}

// ---------------------------------------------------------------------------------------------
// Restart: src/NTF_sep_event_RT.m:27-38 + src/init_buff.m:17-42 for the listed streams -- the one initialisation path
// (creation restarts every stream through it).  Grid (listed stream, array, part): each workgroup resets one part of one
// per-stream array of one listed stream.  No array is both read and written by the launch except through disjoint
// (stream, array) pairs, so the workgroups are independent.  The arrays both modes hold are listed here and reset by
// orestart_common; a mode's own arrays (k_obrestart: the fp32 images and the Mel masters) follow from kRsShared.
// ---------------------------------------------------------------------------------------------
enum : int {
    kRsBx, kRsBd, kRsBfix, kRsH0, kRsAd0, kRsAdblk, kRsLdblk, kRsRup, kRsLam, kRsXm, kRsRblk, kRsTail, kRsTailX, kRsTailD,
    kRsDev, kRsShared
};
constexpr int kRsParts = 8;  // workgroups per (stream, array)

template <typename T>
struct ORestartCommon {
    const int* slots;       // [n] the streams to restart (distinct, in range: checked on the host)
    const double* Bx;       // the event dictionary [Rx][F]: stream s's at Bx + s * sBx (sBx = 0: one for all)
    int64_t sBx;
    const double* Bd;       // [n][Rd][F] new noise dictionaries, or NULL = keep each stream's (carry; Bfix untouched)
    const T* H0n;           // [n][r] or NULL = keep
    const T* Adn;           // [n][Ra][ma] or NULL = the values the stream last started with (Ad0)
    double *B, *Bfix;       // [S][r][F], [S][Rd][F]
    T *H0, *Ad0, *adblk, *ldblk, *lambda_dav, *Xm_tilde, *r_blk, *tail, *tail_x, *tail_d;
    uint8_t* rup;
    OnlineDev* dev;
    int F, r, Rx, Rd, Ra, ma, Pl;
    int64_t ntail;
};

// this workgroup's part of n elements: dst[e] = src[e] / dst[e] = v
template <typename D, typename S>
__device__ __forceinline__ void ors_copy(D* dst, const S* src, size_t n) {
    for (size_t e = (size_t)blockIdx.z * 256 + threadIdx.x; e < n; e += (size_t)kRsParts * 256) dst[e] = (D)src[e];
}
template <typename D>
__device__ __forceinline__ void ors_fill(D* dst, D v, size_t n) {
    for (size_t e = (size_t)blockIdx.z * 256 + threadIdx.x; e < n; e += (size_t)kRsParts * 256) dst[e] = v;
}

// array `arr` (< kRsShared) of listed stream blockIdx.x; adapts: this stream runs the noise-dictionary adaptation
template <typename T>
__device__ __forceinline__ void orestart_common(const ORestartCommon<T>& a, int arr, bool adapts) {
    const int i = blockIdx.x, s = a.slots[i];
    const size_t F = a.F, nA = (size_t)a.Ra * a.ma, nD = (size_t)a.Rd * F;
    switch (arr) {
        case kRsBx: ors_copy(a.B + (size_t)s * a.r * F, a.Bx + (size_t)s * a.sBx, (size_t)a.Rx * F); break;
        case kRsBd:
            if (a.Bd) ors_copy(a.B + (size_t)s * a.r * F + (size_t)a.Rx * F, a.Bd + i * nD, nD);
            break;
        case kRsBfix:  // B_Mel_d in DFT mode (:328): set with a new dictionary, never adapted (:392)
            if (a.Bd) ors_copy(a.Bfix + s * nD, a.Bd + i * nD, nD);
            break;
        case kRsH0:
            if (a.H0n) ors_copy(a.H0 + (size_t)s * a.r, a.H0n + (size_t)i * a.r, (size_t)a.r);
            break;
        case kRsAd0:
            if (a.Adn) ors_copy(a.Ad0 + s * nA, a.Adn + i * nA, nA);
            break;
        case kRsAdblk:  // rand(R_a, m_a) (src/init_buff.m:39); zeros without adaptation
            if (!adapts) ors_fill(a.adblk + s * nA, T(0), nA);
            else ors_copy(a.adblk + s * nA, a.Adn ? a.Adn + i * nA : a.Ad0 + s * nA, nA);
            break;
        case kRsLdblk: ors_fill(a.ldblk + s * F * a.ma, T(0), F * a.ma); break;
        case kRsRup: ors_fill(a.rup + (size_t)s * a.Ra, (uint8_t)0, (size_t)a.Ra); break;
        case kRsLam: ors_fill(a.lambda_dav + s * F, T(0), F); break;
        case kRsXm: ors_fill(a.Xm_tilde + s * F, T(0), F); break;
        case kRsRblk: ors_fill(a.r_blk + s * F * a.Pl, T(0), F * a.Pl); break;
        case kRsTail: ors_fill(a.tail + s * a.ntail, T(0), (size_t)a.ntail); break;
        case kRsTailX:
            if (a.tail_x) ors_fill(a.tail_x + s * a.ntail, T(0), (size_t)a.ntail);
            break;
        case kRsTailD:
            if (a.tail_d) ors_fill(a.tail_d + s * a.ntail, T(0), (size_t)a.ntail);
            break;
        default:  // kRsDev
            if (blockIdx.z == 0 && threadIdx.x == 0) a.dev[s] = OnlineDev{0, 1, 0, 0};  // update_switch = 1 (src/init_buff.m:42)
    }
}

// B_DFT_d = [B_d_rem, B_d_tmp, B_d_fix] (:336), resp. B_Mel_d (:318), of every stream whose adaptation ran: one workgroup per
// (column, stream), into Btmp (the kept columns are read from the dictionary the refresh overwrites).  Stream s's fixed
// columns are at Bfix + s * sfix (DFT: the dictionary it started with, :328; Mel: its own B_Mel_d, :309).  The dictionaries
// are doubles in both modes, so the body is no template; k_obassemble (fp32: sfix from the host) and k_obassemble64 (sfix =
// Rd * F) wrap it, one kernel per unit.
__device__ __forceinline__ void oassemble_cols(const OnlineStatus* status, const int* nfr, int step, int S, const double* B, const double* Wu,
                                               const double* Bfix, int64_t sfix, const uint8_t* rupa, int F, int r, int Rx, int Ra, int Rd,
                                               double* Btmp) {
    const int j = blockIdx.x, s = blockIdx.y;
    if (j >= Rd || !ob_due(status, nfr, step, S, s)) return;
    const double* Bd_old = B + (size_t)s * r * F + (size_t)Rx * F;
    const uint8_t* rup = rupa + (size_t)s * Ra;
    const double* src;
    if (j >= Ra) {
        src = Bfix + (size_t)s * sfix + (size_t)j * F;
    } else {
        bool retrained;
        const int k = oassemble_col(rup, Ra, j, &retrained);
        src = retrained ? Wu + (size_t)s * Ra * F + (size_t)k * F : Bd_old + (size_t)k * F;
    }
    double* dst = Btmp + (size_t)s * Rd * F + (size_t)j * F;
    for (int f = threadIdx.x; f < F; f += blockDim.x) dst[f] = src[f];
}

// inverse STFT of every (frame, stream): stream s's frames go behind the nov-1 frames kept from its previous chunk.  The two
// FFT buffers are static LDS in fp32 and dynamic LDS (2 N double2) in fp64, where 2^12 points exceed the static limit.
template <int LOGN, typename T>
__global__ __launch_bounds__(256) void k_obistft(OIstftArgsT<T> a, const int* nfr, int S, int64_t syn_stride, int nov) {
    constexpr int N = 1 << LOGN;
    const int i = blockIdx.x, s = blockIdx.y;
    if (i >= nfr[s]) return;
    const size_t slot = (size_t)i * S + s;
    const T* mag = a.mag + slot * a.ld;
    const ocplx<T>* ph = a.ph + slot * a.ld;
    T* o = a.syn + (size_t)s * syn_stride + (size_t)(nov - 1 + i) * a.sz;
    if constexpr (sizeof(T) == 4) {
        __shared__ ocplx<T> bufA[N];
        __shared__ ocplx<T> bufB[N];
        oistft_frame<LOGN, T>(a, mag, ph, o, bufA, bufB);
    } else {
        extern __shared__ __attribute__((aligned(16))) ocplx<T> fbuf[];
        oistft_frame<LOGN, T>(a, mag, ph, o, fbuf, fbuf + N);
    }
}

// the nov-1 synthesis frames carried between chunks: into (dir 0) / out of (dir 1) each stream's synthesis buffer
template <typename T>
__global__ __launch_bounds__(256) void k_obtail(T* syn, T* tail, const int* nfr, int64_t syn_stride, int nov, int sz, int dir) {
    const int s = blockIdx.x;
    const size_t n = (size_t)(nov - 1) * sz;
    T* sy = syn + (size_t)s * syn_stride + (dir ? (size_t)nfr[s] * sz : 0);
    T* tl = tail + (size_t)s * n;
    for (size_t e = threadIdx.x; e < n; e += 256) {
        if (dir) tl[e] = sy[e];
        else sy[e] = tl[e];
    }
}

// Overlap-add and int16 output (oola_sample: the int16 stream is the value rounded half away from zero) per stream: grid
// (blocks, S); stream s writes its n_out[s] hops at out_off[s]
template <typename T>
__global__ __launch_bounds__(256) void k_obola(const T* __restrict__ syn, int64_t syn_stride, OBatchFrames b, const int* i_first,
                                               const int* n_out, const int64_t* out_off, int delay, int sz, int hop, int nov,
                                               T* __restrict__ outf, int16_t* __restrict__ out16) {
    const int s = blockIdx.y;
    const size_t n = (size_t)n_out[s] * hop;
    const T* sy = syn + (size_t)s * syn_stride;
    const int l0 = b.l0[s], i0 = i_first[s];
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / hop), q0 = (int)(e - (size_t)j * hop);
        oola_sample<T>(sy, i0 + j, q0, l0, delay, sz, hop, nov, outf, out16, (size_t)out_off[s] + e);
    }
}

}  // namespace snmf
