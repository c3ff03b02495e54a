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

}  // namespace snmf
