// snmf_online_batch_common.h -- what the batched online separator's two precisions share on the device: the per-chunk
// framing of the streams and the gate of the adaptation launches.  Included by snmf_online_batch.h (fp32) and
// snmf_online_batch_f64.h (fp64).
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
// part) as k_obrestart: each workgroup moves one part of one array of one listed stream with plain loads and stores, and
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

}  // namespace snmf
