// snmf_tu_assemble.hip -- run_basis_train.m:16-57 on the device: the clips of every class go up as they come off disk (int16 PCM,
// or doubles already scaled), the ten launches of snmf_assemble.h form every class's s_full in one signal slab in HBM, and the
// handle keeps it there for snmf_run_basis_train_signals_batch_* (snmf_tu_frontend_batch.hip).
//
//   snmf_train_signals_assemble_i16 / _f64    clips in, handle out
//   snmf_train_signals_info / _get_f64        lengths and clips_used; one class's signal to the host
//   snmf_train_signals_destroy
//
// Everything the entries refuse is refused before the device is touched, except a clip without a positive finite variance, which
// only the device knows: then nothing is returned, every block is freed and the context stays usable.
#include "snmf_internal.h"
#include "snmf_assemble.h"

namespace {

constexpr int64_t kMaxGrid = 0x7fffffffLL;

template <typename T>
int assemble(const char* entry, snmf_ctx* ctx, const snmf_assemble_params* ap, int32_t n_classes, const int32_t* n_clips, const T* const* clips,
             const int64_t* clip_len, const int32_t* mode, const int64_t* range, snmf_train_signals** out) {
    if (out) *out = nullptr;
    if (!ctx || !ap || !n_clips || !clips || !clip_len || !mode || !out) return fail(SNMF_ERR_INVALID, "%s: NULL argument", entry);
    if (n_classes < 1) return fail(SNMF_ERR_INVALID, "%s: n_classes must be at least 1 (got %d)", entry, n_classes);
    if (ap->frame_len < 2 || (ap->frame_len & 1)) return fail(SNMF_ERR_INVALID, "%s: frame_len must be even and at least 2 (got %d)", entry, ap->frame_len);
    if (ap->bg_len < 1) return fail(SNMF_ERR_INVALID, "%s: bg_len must be at least 1 (got %d)", entry, ap->bg_len);
    if (ap->seq_len_max < 0) return fail(SNMF_ERR_INVALID, "%s: seq_len_max is negative", entry);
    const int shift = ap->frame_len / 2;
    int64_t total_clips = 0;
    for (int k = 0; k < n_classes; ++k) {
        if (n_clips[k] < 1) return fail(SNMF_ERR_INVALID, "%s: class %d has no clip", entry, k);
        if (mode[k] < 0 || mode[k] > 2) return fail(SNMF_ERR_INVALID, "%s: class %d has mode %d (0: cut, 1: VAD, 2: range)", entry, k, mode[k]);
        if (mode[k] == 2 && !range) return fail(SNMF_ERR_INVALID, "%s: class %d is cut to ranges and range is NULL", entry, k);
        total_clips += n_clips[k];
    }
    if (total_clips > kMaxGrid) return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld clips", entry, (long long)total_clips);
    const int nc = (int)total_clips;
    std::vector<AsmClip> h_clip((size_t)nc + 1);
    std::vector<AsmClass> h_cls(n_classes);
    std::vector<int64_t> len(nc);
    int64_t in0 = 0, blk0 = 0, fr0 = 0, out0 = 0;
    for (int k = 0, ci = 0; k < n_classes; ++k) {
        h_cls[k].clip0 = ci, h_cls[k].n_clips = n_clips[k], h_cls[k].out0 = out0;
        int64_t cap = 0;
        for (int i = 0; i < n_clips[k]; ++i, ++ci) {
            const int64_t L = clip_len[ci];
            if (!clips[ci]) return fail(SNMF_ERR_INVALID, "%s: clip %d of class %d is NULL", entry, i, k);
            if (L < 1) return fail(SNMF_ERR_DIM, "%s: clip %d of class %d has %lld samples", entry, i, k, (long long)L);
            AsmClip c{};
            c.in0 = in0, c.len = L, c.lo = 0, c.hi = L, c.blk0 = blk0, c.fr0 = fr0, c.cls = k, c.mode = mode[k];
            if (mode[k] == 1) {
                if (L < ap->bg_len)
                    return fail(SNMF_ERR_DIM, "%s: clip %d of class %d has %lld samples, fewer than bg_len = %d", entry, i, k, (long long)L, ap->bg_len);
                const int64_t nfr = std::max<int64_t>(0, L / shift - 1);  // src/vadenergy_simple.m:21, :24
                if (nfr > kMaxGrid) return fail(SNMF_ERR_UNSUPPORTED, "%s: clip %d of class %d has %lld VAD frames", entry, i, k, (long long)nfr);
                c.nfr = (int32_t)nfr;
            } else if (mode[k] == 2) {
                const int64_t a = range[2 * (size_t)ci], b = range[2 * (size_t)ci + 1];
                if (a < 1 || b > L || a > b)
                    return fail(SNMF_ERR_DIM, "%s: the range [%lld, %lld] of clip %d of class %d is not inside [1, %lld]", entry, (long long)a,
                                (long long)b, i, k, (long long)L);
                c.lo = a - 1, c.hi = b;
            } else if (ap->file_len_max > 0 && L > ap->file_len_max) {
                c.hi = ap->file_len_max;
            }
            h_clip[ci] = c;
            len[ci] = L;
            cap += c.hi - c.lo;
            blk0 += (L + (in0 & 7) + kAsmSpan - 1) / kAsmSpan;
            fr0 += c.nfr;
            in0 += L;
        }
        out0 += std::min(cap, ap->seq_len_max);
    }
    h_clip[nc] = AsmClip{};
    h_clip[nc].in0 = in0, h_clip[nc].blk0 = blk0, h_clip[nc].fr0 = fr0;
    if (blk0 > kMaxGrid || (fr0 + 3) / 4 > kMaxGrid)
        return fail(SNMF_ERR_UNSUPPORTED, "%s: %lld work blocks and %lld VAD frames are above a launch grid's limit", entry, (long long)blk0, (long long)fr0);

    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevMem mem;
    mem.st = st;
    AsmArgs a{};
    a.n_clips = nc, a.n_classes = n_classes, a.shift = shift, a.bg_len = ap->bg_len, a.thr = ap->thr, a.seq_max = ap->seq_len_max;
    a.n_blocks = blk0, a.n_frames = fr0, a.n_groups = (blk0 + 1 + kAsmScan - 1) / kAsmScan;  // (one entry beyond the last block: the total)
    T* in = nullptr;
    AsmClip* d_clip = nullptr;
    AsmClass* d_cls = nullptr;
    SN_TRY(mem.get(&in, (size_t)((in0 + 7) / 8 * 8 + 8)));  // (a thread's 8-sample vector may end beyond the last clip)
    SN_TRY(mem.get(&d_clip, h_clip.size()));
    SN_TRY(mem.get(&d_cls, h_cls.size()));
    SN_TRY(mem.get(&a.flag, (size_t)fr0));
    SN_TRY(mem.get(&a.bcnt, (size_t)a.n_groups * kAsmScan));
    SN_TRY(mem.get(&a.bscan, (size_t)a.n_groups * kAsmScan));
    SN_TRY(mem.get(&a.gsum, (size_t)a.n_groups));
    SN_TRY(mem.get(&a.bsum, (size_t)blk0));
    SN_TRY(mem.get(&a.bdev, (size_t)blk0));
    SN_TRY(mem.get(&a.bmax, (size_t)blk0));
    SN_TRY(mem.get(&a.bg, (size_t)nc));
    SN_TRY(mem.get(&a.mean, (size_t)nc));
    SN_TRY(mem.get(&a.sd, (size_t)nc));
    SN_TRY(mem.get(&a.pk, (size_t)nc));
    SN_TRY(mem.get(&a.kept, (size_t)nc));
    SN_TRY(mem.get(&a.dst, (size_t)nc));
    SN_TRY(mem.get(&a.clen, (size_t)n_classes));
    SN_TRY(mem.get(&a.used, (size_t)n_classes));
    SN_TRY(mem.get(&a.bad, (size_t)n_classes));
    snmf_train_signals* ts = new snmf_train_signals();
    struct Guard {  // the handle and its slab, until the call has succeeded
        snmf_train_signals* ts;
        ~Guard() {
            if (!ts) return;
            hipStreamSynchronize(ts->ctx->stream);
            if (ts->slab) hipFree(ts->slab);
            delete ts;
        }
    } guard{ts};
    ts->ctx = ctx, ts->device = ctx->device;
    SN_TRY(mem.get(&ts->slab, (size_t)out0, true));
    a.in = in, a.clip = d_clip, a.cls = d_cls, a.out = ts->slab;
    SN_TRY(xfer_gather_in<T>(ctx, nc, clips, len.data(), in));
    HIP_TRY(hipMemcpyAsync(d_clip, h_clip.data(), h_clip.size() * sizeof(AsmClip), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_cls, h_cls.data(), h_cls.size() * sizeof(AsmClass), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.bcnt, 0, (size_t)a.n_groups * kAsmScan * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(a.dst, 0xff, (size_t)nc * sizeof(int64_t), st));  // -1: nothing of the clip is written
    {
        ScopedTimer tm(ctx, FAM_ASSEMBLE);
        const dim3 tb(256);
        const unsigned gb = (unsigned)blk0, gg = (unsigned)a.n_groups;
        if (fr0 > 0) {
            hipLaunchKernelGGL(k_asm_bg<T>, dim3((unsigned)nc), tb, 0, st, a);
            hipLaunchKernelGGL(k_asm_frames<T>, dim3((unsigned)((fr0 + 3) / 4)), tb, 0, st, a);
        }
        hipLaunchKernelGGL(k_asm_keep<T>, dim3(gb), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_scan_sums, dim3(gg), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_scan_top, dim3(1), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_scan_apply, dim3(gg), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_sum, dim3((unsigned)nc), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_dev<T>, dim3(gb), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_place, dim3((unsigned)n_classes), tb, 0, st, a);
        hipLaunchKernelGGL(k_asm_write<T>, dim3(gb), tb, 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    ts->out0.resize(n_classes), ts->len.resize(n_classes), ts->used.resize(n_classes);
    std::vector<int32_t> bad(n_classes);
    HIP_TRY(hipMemcpyAsync(ts->len.data(), a.clen, sizeof(int64_t) * (size_t)n_classes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ts->used.data(), a.used, sizeof(int32_t) * (size_t)n_classes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bad.data(), a.bad, sizeof(int32_t) * (size_t)n_classes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < n_classes; ++k) {
        ts->out0[k] = h_cls[k].out0;
        if (bad[k] >= 0)
            return fail(SNMF_ERR_INVALID, "%s: clip %d of class %d has no positive finite variance (one kept sample, or a constant clip): "
                        "run_basis_train.m:44 would write NaN", entry, bad[k], k);
    }
    guard.ts = nullptr;
    *out = ts;
    return SNMF_OK;
}

}  // namespace

extern "C" int snmf_train_signals_assemble_i16(snmf_ctx* ctx, const snmf_assemble_params* ap, int32_t n_classes, const int32_t* n_clips,
                                               const int16_t* const* clips, const int64_t* clip_len, const int32_t* mode, const int64_t* range,
                                               snmf_train_signals** out) {
    return assemble<int16_t>("snmf_train_signals_assemble_i16", ctx, ap, n_classes, n_clips, clips, clip_len, mode, range, out);
}
extern "C" int snmf_train_signals_assemble_f64(snmf_ctx* ctx, const snmf_assemble_params* ap, int32_t n_classes, const int32_t* n_clips,
                                               const double* const* clips, const int64_t* clip_len, const int32_t* mode, const int64_t* range,
                                               snmf_train_signals** out) {
    return assemble<double>("snmf_train_signals_assemble_f64", ctx, ap, n_classes, n_clips, clips, clip_len, mode, range, out);
}

extern "C" int snmf_train_signals_info(const snmf_train_signals* ts, int32_t* n_classes, int64_t* n_samples, int32_t* clips_used) {
    if (!ts) return fail(SNMF_ERR_INVALID, "snmf_train_signals_info: the handle is NULL");
    if (n_classes) *n_classes = (int32_t)ts->len.size();
    if (n_samples) std::copy(ts->len.begin(), ts->len.end(), n_samples);
    if (clips_used) std::copy(ts->used.begin(), ts->used.end(), clips_used);
    return SNMF_OK;
}

extern "C" int snmf_train_signals_get_f64(const snmf_train_signals* ts, int32_t k, double* s_full) {
    if (!ts || !s_full) return fail(SNMF_ERR_INVALID, "snmf_train_signals_get_f64: NULL argument");
    if (k < 0 || k >= (int32_t)ts->len.size()) return fail(SNMF_ERR_DIM, "snmf_train_signals_get_f64: class %d of %d", k, (int)ts->len.size());
    if (ts->len[k] == 0) return SNMF_OK;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(ts->ctx->device));
    HIP_TRY(hipMemcpyAsync(s_full, ts->slab + ts->out0[k], sizeof(double) * (size_t)ts->len[k], hipMemcpyDeviceToHost, ts->ctx->stream));
    HIP_TRY(hipStreamSynchronize(ts->ctx->stream));
    return SNMF_OK;
}

extern "C" int snmf_train_signals_destroy(snmf_train_signals* ts) {
    if (!ts) return SNMF_OK;
    if (ts->slab) {
        hipSetDevice(ts->device);
        hipDeviceSynchronize();  // (whatever still reads the slab; the context may be gone)
        hipFree(ts->slab);
    }
    delete ts;
    return SNMF_OK;
}
