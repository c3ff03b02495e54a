// snmf_online_batch_chains.h -- the chain driver of the batched online separator (snmf_online_batch_run_chains_f32 / _f64):
// a queue of chains of recordings over the S slots of one batch, the per-target loop of Do_MultiBatch_IS16_20160324.m:183-205
// around run_ntf_sep_RT.m:10-41.  Host code only, beside snmf_online_batch_host.h: it decides nothing about a frame.  It
// reaches the batch through three calls of the mode (Ops), which are the public restart / process / get-basis entries, so a
// file's bits are those of the same calls made by hand -- and of se_snmf_nat_amd/online.py's ntf_sep_event_rt_chains, whose
// schedule this restates.
//   int ops.restart(n, slots, Bd, Bmd, H0, Ad)         all arrays NULL: the carry; else a new chain's dictionary and draws
//   int ops.process(pcm, n, flush, xt, x16, cap, n_out)  one process call over all S streams
//   int ops.basis(k, dst)                               stream k's fp64 master, tight (Mel batch: of B_Mel_d)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "snmf.h"

// Of snmf_internal.h, which the library's translation units include first; restated so that this header also compiles on its
// own in a host-only program (tests/chains_host/chains_sim_main.cpp drives the scheduler against a simulated batch).
int fail(int code, const char* fmt, ...);
#ifndef SN_TRY
#define SN_TRY(expr)              \
    do {                          \
        int s_ = (expr);          \
        if (s_ != SNMF_OK) return s_; \
    } while (0)
#endif

// what the driver reads of the batch: slots, hop, delay, and one chain's array lengths (nBm: 0 outside Mel mode; nA: 0
// when the batch does not adapt); step0 = hops per call when chunk_hops is 0
struct OChainsGeom {
    int S = 0, hop = 1, delay = 0;
    size_t nB = 0, nBm = 0, r = 0, nA = 0;
    int64_t step0 = 1;
};

template <typename T>
struct OChainsArgs {
    int32_t n_chains;
    const int32_t* n_files;
    const T* const* pcm;
    const int64_t* n_samples;
    const double *Bd, *Bmd;
    const T *H0, *Ad;
    int32_t chunk_hops;
    int16_t* const* x16;
    T* const* xf;
    const int64_t* cap;
    int64_t* n_out;
    double* const* B_out;
};

// The counts and arrays of a run, before the handle's state is looked at.  n_total: files in all.
template <typename T>
int ochains_check_args(const OChainsGeom& g, const OChainsArgs<T>& a, int64_t* n_total) {
    *n_total = 0;
    if (a.n_chains < 0) return fail(SNMF_ERR_INVALID, "n_chains = %d", a.n_chains);
    if (a.chunk_hops < 0) return fail(SNMF_ERR_INVALID, "chunk_hops = %d (0: one device chunk)", a.chunk_hops);
    if (a.n_chains > 0 && !a.n_files) return fail(SNMF_ERR_INVALID, "n_files is NULL");
    int64_t nf = 0;
    for (int c = 0; c < a.n_chains; ++c) {
        if (a.n_files[c] < 0) return fail(SNMF_ERR_INVALID, "chain %d has %d files", c, a.n_files[c]);
        nf += a.n_files[c];
    }
    if (nf == 0) return SNMF_OK;
    if (!a.pcm || !a.n_samples) return fail(SNMF_ERR_INVALID, "pcm / n_samples is NULL");
    if (!a.Bd || !a.H0) return fail(SNMF_ERR_INVALID, "B_DFT_d / H0 is NULL");
    if (g.nA && !a.Ad) return fail(SNMF_ERR_INVALID, "Ad_blk0 is required when adapt_train_N is set");
    if (g.nBm && !a.Bmd) return fail(SNMF_ERR_INVALID, "a Mel batch needs every chain's start B_Mel_d");
    const bool any_out = a.x16 || a.xf;
    if (any_out && !a.cap) return fail(SNMF_ERR_INVALID, "cap is NULL");
    for (int64_t i = 0; i < nf; ++i) {
        if (a.n_samples[i] < 0 || (a.n_samples[i] > 0 && !a.pcm[i])) return fail(SNMF_ERR_INVALID, "file %lld: pcm is NULL", (long long)i);
        const int64_t need = (a.n_samples[i] / g.hop + g.delay + 1) * g.hop;
        if (((a.x16 && a.x16[i]) || (a.xf && a.xf[i])) && a.cap[i] < need)
            return fail(SNMF_ERR_INVALID, "file %lld: output capacity %lld < %lld samples", (long long)i, (long long)a.cap[i], (long long)need);
    }
    *n_total = nf;
    return SNMF_OK;
}

// The run itself, on a batch whose streams are all idle (checked by the caller).  Every call feeds each busy slot `step`
// hops of its file, the last piece with the flush; a slot whose file ended takes the next file of its chain (carry) or the
// next chain of the queue (its dictionary and draws) in the restart calls that open the next round.
template <typename T, class Ops>
int ochains_run(const OChainsGeom& g, const OChainsArgs<T>& a, Ops& ops) {
    const int S = g.S;
    const int64_t hop = g.hop;
    int64_t nf = 0, longest = 0;
    for (int c = 0; c < a.n_chains; ++c) nf += a.n_files[c];
    for (int64_t i = 0; i < nf; ++i) longest = std::max(longest, a.n_samples[i] / hop);
    // no call can feed a slot more than its whole file: a larger chunk_hops asks for the same calls, and must not size the scratch
    const int64_t step = std::min<int64_t>(a.chunk_hops > 0 ? a.chunk_hops : g.step0, longest + 1);
    std::vector<int64_t> first(a.n_chains + 1, 0);  // chain c's files are first[c] .. first[c + 1]
    std::vector<int> queue;                          // the chains that have files, in chain order
    for (int c = 0; c < a.n_chains; ++c) {
        first[c + 1] = first[c] + a.n_files[c];
        if (a.n_files[c] > 0) queue.push_back(c);
    }
    size_t next = 0;
    struct Slot { int chain = -1, file = 0; int64_t fed = 0, written = 0; };
    std::vector<Slot> slot(S);
    std::vector<int32_t> carry, fresh;
    int busy = 0;
    for (int k = 0; k < S && next < queue.size(); ++k, ++busy) {
        slot[k].chain = queue[next++];
        fresh.push_back(k);
    }
    // one call's outputs of every slot: step hops, the hop a remainder completes and the flush frames
    const int64_t cap_s = (step + g.delay + 3) * hop;
    std::vector<T> sf((size_t)S * cap_s);
    std::vector<int16_t> s16((size_t)S * cap_s);
    std::vector<const T*> pcm(S);
    std::vector<T*> xf(S);
    std::vector<int16_t*> x16(S);
    std::vector<int64_t> n(S), cap(S, cap_s), n_out(S);
    std::vector<int32_t> flush(S);
    for (int k = 0; k < S; ++k) {
        xf[k] = sf.data() + (size_t)k * cap_s;
        x16[k] = s16.data() + (size_t)k * cap_s;
    }
    const T dummy = T(0);
    std::vector<double> Bd, Bmd;
    std::vector<T> H0, Ad;
    while (busy > 0) {
        if (!carry.empty()) SN_TRY(ops.restart((int)carry.size(), carry.data(), nullptr, nullptr, nullptr, nullptr));
        if (!fresh.empty()) {
            Bd.clear(); Bmd.clear(); H0.clear(); Ad.clear();
            for (int32_t k : fresh) {
                const size_t c = (size_t)slot[k].chain;
                Bd.insert(Bd.end(), a.Bd + c * g.nB, a.Bd + (c + 1) * g.nB);
                if (g.nBm) Bmd.insert(Bmd.end(), a.Bmd + c * g.nBm, a.Bmd + (c + 1) * g.nBm);
                H0.insert(H0.end(), a.H0 + c * g.r, a.H0 + (c + 1) * g.r);
                if (g.nA) Ad.insert(Ad.end(), a.Ad + c * g.nA, a.Ad + (c + 1) * g.nA);
            }
            SN_TRY(ops.restart((int)fresh.size(), fresh.data(), Bd.data(), g.nBm ? Bmd.data() : nullptr, H0.data(), g.nA ? Ad.data() : nullptr));
        }
        carry.clear();
        fresh.clear();
        for (int k = 0; k < S; ++k) {
            pcm[k] = &dummy;
            n[k] = 0;
            flush[k] = 0;
            if (slot[k].chain < 0) continue;
            const int64_t i = first[slot[k].chain] + slot[k].file;
            n[k] = std::min<int64_t>(step * hop, a.n_samples[i] - slot[k].fed);
            if (n[k] > 0) pcm[k] = a.pcm[i] + slot[k].fed;
            slot[k].fed += n[k];
            flush[k] = slot[k].fed >= a.n_samples[i];
        }
        SN_TRY(ops.process(pcm.data(), n.data(), flush.data(), xf.data(), x16.data(), cap.data(), n_out.data()));
        for (int k = 0; k < S; ++k) {
            Slot& q = slot[k];
            if (q.chain < 0) continue;
            const int c = q.chain;
            const int64_t i = first[c] + q.file;
            if (a.x16 && a.x16[i]) std::memcpy(a.x16[i] + q.written, x16[k], (size_t)n_out[k] * 2);
            if (a.xf && a.xf[i]) std::memcpy(a.xf[i] + q.written, xf[k], (size_t)n_out[k] * sizeof(T));
            q.written += n_out[k];
            if (!flush[k]) continue;
            if (a.n_out) a.n_out[i] = q.written;
            if (a.B_out && a.B_out[i]) SN_TRY(ops.basis(k, a.B_out[i]));
            q.fed = q.written = 0;
            if (q.file + 1 < a.n_files[c]) {
                ++q.file;
                carry.push_back(k);
            } else if (next < queue.size()) {
                q.chain = queue[next++];
                q.file = 0;
                fresh.push_back(k);
            } else {
                q.chain = -1;
                --busy;
            }
        }
    }
    return SNMF_OK;
}
