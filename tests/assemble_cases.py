"""The NumPy restatement of the training-signal assembly (run_basis_train.m:16-57, src/vadenergy_simple.m:1-32) and the clips of
its tests (test_assemble_api.py, test_gpu_assemble.py, test_gpu_train_clips.py).  A helper, not a test.

The restatement follows the reference line by line in float64; only its sums are NumPy's (pairwise) where MATLAB's are
sequential.  A different summation order moves a frame quotient q = (mean - bg_mean) / mean by about 1e-16 relative, so the
device's voiced / unvoiced decisions are the restatement's as long as no finite q of a case lies within 1e-9 of thr
(test_assemble_api.py asserts it for every mode-1 clip of the GPU cases).

The GPU cases use fs = 1000: frame_len 20, frame_shift 10, bg_len 50, so that clips of a few thousand samples cross several
2048-sample work blocks of the keep / deviation / write kernels.  SPAN, FOLD and SCAN restate the kernels' per-workgroup spans
(csrc/snmf_assemble.h: kAsmSpan; 256 work blocks per pass of a clip's fold; kAsmScan work blocks per scan group).
"""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THR = 0.7          # run_basis_train.m:35
PEAK = 30000.0     # run_basis_train.m:45
SPAN = 2048        # samples of a work block
FOLD = 256         # work blocks per pass of a clip's fold
SCAN = 1024        # work blocks per scan group
TOL = 1e-12 * PEAK  # per sample: tree-ordered fp64 sums of <= 2^24 terms move sd by ~1e-14 relative; a wrong index makes >= 1e-4


def pcm_to_double(c):
    """run_basis_train.m:26-27: wavread(.) .* 32767 of 16-bit PCM, exact in double."""
    c = np.asarray(c)
    return c.astype(np.float64) / 32768 * 32767 if c.dtype == np.int16 else np.asarray(c, dtype=np.float64)


def vad_settings(fs):
    """-> (bg_len, frame_len): run_basis_train.m:32, src/vadenergy_simple.m:19."""
    return int(round(0.05 * fs)), int(round(0.02 * fs))


def vad_frames(s, bg_len, frame_len):
    """src/vadenergy_simple.m:11, :19-27 -> (q per frame, first 0-based sample per frame): frames k = 1 .. floor(len / shift) - 1
    of frame_len samples, half overlapping."""
    x = np.abs(s)
    bg_mean = x[:bg_len].mean()                                   # :11
    shift = frame_len // 2                                        # :20
    frame_num = len(s) // shift                                   # :21
    starts = np.arange(max(frame_num - 1, 0)) * shift             # :23-24, :31 (0-based)
    if len(starts) == 0:
        return np.zeros(0), starts
    m = np.lib.stride_tricks.sliding_window_view(x, frame_len)[starts].mean(axis=1)   # :25
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (m - bg_mean) / m                                     # :27
    return q, starts


def vadenergy_simple(s, bg_len, frame_len, thr=THR):
    """src/vadenergy_simple.m:1-32 -> vad (0 / 1 per sample)."""
    q, starts = vad_frames(s, bg_len, frame_len)
    vad = np.zeros(len(s))
    for i in starts[q > thr]:                                     # :27-29 (NaN and -inf compare false)
        vad[i:i + frame_len] = 1
    return vad


def vad_margin(s, bg_len, frame_len, thr=THR):
    """The smallest |q - thr| over the finite frame quotients of a clip (inf when there is none)."""
    q, _ = vad_frames(s, bg_len, frame_len)
    q = q[np.isfinite(q)]
    return float(np.abs(q - thr).min()) if q.size else float("inf")


def treat_clip(c, mode, rng, fs, file_len_max):
    """run_basis_train.m:26-43 -> the clip's samples after its class's treatment (before the normalisation)."""
    s = pcm_to_double(c)                                          # :26-27
    if mode == 1:
        bg_len, frame_len = vad_settings(fs)                      # :32-35
        vad = vadenergy_simple(s, bg_len, frame_len)              # :36
        s = s * vad
        return s[s != 0]                                          # :37 nonzeros
    if mode == 2:
        a, b = rng
        a, b = (1 if a == 0 else a), min(b, len(s))               # src/load_anot.m:9-15
        return s[a - 1:b]                                         # :40
    if file_len_max > 0 and len(s) > file_len_max:                # :41
        return s[:file_len_max]                                   # :42
    return s


def normalise(s):
    """run_basis_train.m:44-45."""
    s = s / np.sqrt(np.var(s, ddof=1))
    return s / np.max(np.abs(s)) * PEAK


def assemble_class(clips, mode, ranges, fs, seq_len_max, file_len_max):
    """run_basis_train.m:19-57 for one class -> (s_full, clips_used, [(start, stop) of every used clip's part of s_full]).
    A clip with no kept sample appends nothing and counts as used."""
    parts, seg, cnt, used = [], [], 0, 0
    for i, c in enumerate(clips):
        used = i + 1
        s = treat_clip(c, mode, ranges[i] if ranges is not None else None, fs, file_len_max)
        if len(s):
            s = normalise(s)                                      # :44-45
        parts.append(s)                                           # :47
        seg.append((cnt, min(cnt + len(s), seq_len_max)))
        cnt += len(s)                                             # :49
        if cnt > seq_len_max:                                     # :50
            break
    s_full = np.concatenate(parts)[:seq_len_max] if parts else np.zeros(0)   # :51, :55-57
    return s_full, used, seg


def assemble(case):
    """-> [(s_full, clips_used, segments)] per class of a case (a dict as CASES holds them)."""
    p = case["p"]
    return [assemble_class(cl, m, r, p["fs"], p["train_seq_len_max"], p["train_file_len_max"])
            for cl, m, r in zip(case["classes"], modes(case), case["ranges"])]


def modes(case):
    return [1 if v else (2 if r is not None else 0) for v, r in zip(case["vad"], case["ranges"])]


# ---- generators -----------------------------------------------------------------------------------------------------------------
def vad_clip(rs, n, silent=False):
    """int16: a background in +-12 with loud bursts in +-9000 of 15-120 samples, and two exact zeros planted inside the longer
    bursts (what nonzeros drops inside voiced stretches)."""
    c = rs.randint(-12, 13, size=n).astype(np.int16)
    if silent:
        return c
    if n <= 64:  # a clip barely longer than bg_len: loud behind the background stretch, so its LAST frame decides what is kept
        c[50:] = rs.randint(4000, 9001, size=max(n - 50, 0))
        return c
    at = 60 + rs.randint(0, 30)
    while at + 15 < n:
        L = min(int(rs.randint(15, 121)), n - at)
        c[at:at + L] = rs.randint(-9000, 9001, size=L)
        if L >= 40:
            c[at + L // 3] = 0
            c[at + 2 * L // 3] = 0
        at += L + int(rs.randint(40, 200))
    return c


def plain_clip(rs, n):
    """int16 in +-9000 with a few exact zeros (kept by modes 0 and 2)."""
    c = rs.randint(-9000, 9001, size=n).astype(np.int16)
    if n >= 8:
        c[rs.randint(0, n, size=max(1, n // 50))] = 0
        c[0], c[-1] = 1234, -4321  # (never a constant clip, whatever the draw)
    return c


P1000 = dict(fs=1000, train_seq_len_max=6000, train_file_len_max=1500)


@functools.lru_cache(maxsize=None)
def case_mixed():
    """All three modes in one call at fs = 1000 (bg_len 50, frame 20, shift 10), seq 6000, file 1500.
    class 0  VAD: bg_len, bg_len + 1, the frame-count edge floor(len / shift) - 1 at 59 / 60, a silent clip, one below / at /
             one above a work block
    class 1  VAD: one clip over more than three work blocks; the class stops in the middle of a clip
    class 2  cut: 3 * shift - 1, 3 * shift, clips at, one over and far over train_file_len_max; the length is EXACTLY the limit
             after clip 6 ('>' does not stop), so clip 7 is still read and cut away whole
    class 3  cut: stops in the middle of a clip; a clip behind the stop is not used
    class 4  ranges: two samples, a range across a work-block edge, v_start = 0 and v_end beyond the clip (clamped), a whole
             clip; never reaches the limit
    class 5  cut: more clips (300) than a workgroup has threads; never reaches the limit
    class 6  range: one clip over more than 256 work blocks (a second pass of the clip's fold), stops inside it"""
    rs = np.random.RandomState(20160324)
    c0 = [vad_clip(rs, n) for n in (50, 51, 59, 60)] + [vad_clip(rs, 700, silent=True)] + [vad_clip(rs, n) for n in (SPAN - 1, SPAN, SPAN + 1)]
    c1 = [vad_clip(rs, 900), vad_clip(rs, 3 * SPAN + 77), vad_clip(rs, 3001), vad_clip(rs, 3001), vad_clip(rs, 3001), vad_clip(rs, 3001)]
    c2 = [plain_clip(rs, n) for n in (29, 30, 1500, 1501, 2 * SPAN + 5, 1441, 100, 64)]
    c3 = [plain_clip(rs, n) for n in (1500, 1700, 1500, 1499, 700, 90)]
    c4 = [plain_clip(rs, n) for n in (40, 2 * SPAN + 4, 300, 200, 77)]
    r4 = [(7, 8), (SPAN - 8, SPAN + 12), (0, 120), (150, 999), (1, 77)]
    c5 = [plain_clip(rs, int(n)) for n in rs.randint(8, 28, size=300)]
    c6 = [plain_clip(rs, 10), plain_clip(rs, (FOLD + 1) * SPAN + 5)]
    r6 = [(1, 10), (3, (FOLD + 1) * SPAN + 1)]
    return dict(p=P1000, classes=[c0, c1, c2, c3, c4, c5, c6], vad=[True, True, False, False, False, False, False],
                ranges=[None, None, None, None, r4, None, r6])


@functools.lru_cache(maxsize=None)
def case_nocut():
    """train_file_len_max <= 0 (no cut) and a limit nothing reaches: a mode-0 clip longer than any cut of the other case, and a
    VAD clip over more than one scan group of work blocks (SCAN * SPAN samples), written whole."""
    rs = np.random.RandomState(7)
    return dict(p=dict(fs=1000, train_seq_len_max=4_000_000, train_file_len_max=0),
                classes=[[plain_clip(rs, 2 * SPAN + 100), plain_clip(rs, 33)], [vad_clip(rs, (SCAN + 3) * SPAN + 19), vad_clip(rs, 50)]],
                vad=[False, True], ranges=[None, None])


@functools.lru_cache(maxsize=None)
def case_recordings():
    """The two committed input recordings at 16 kHz with the shipped limits' proportions: one VAD class, one cut class."""
    d = np.load(os.path.join(GOLD, "refwav_pairs.npz"))
    a, b = d["m03_in"], d["lm_in"]
    return dict(p=dict(fs=16000, train_seq_len_max=200_000, train_file_len_max=60_000), classes=[[a, b], [b, a]], vad=[True, False],
                ranges=[None, None])


@functools.lru_cache(maxsize=None)
def case_blocks(n_blocks):
    """One VAD clip of exactly n_blocks work blocks, written whole: one below, at and one above the FOLD work blocks a workgroup
    folds per pass, and the SCAN work blocks of a scan group (the scan covers one entry more than there are blocks: the total)."""
    rs = np.random.RandomState(1000 + n_blocks)
    return dict(p=dict(fs=1000, train_seq_len_max=10_000_000, train_file_len_max=0), classes=[[vad_clip(rs, n_blocks * SPAN)]], vad=[True],
                ranges=[None])


CASES = {"mixed": case_mixed, "nocut": case_nocut, "recordings": case_recordings}
CASES.update({f"blocks{n}": functools.partial(case_blocks, n) for n in (FOLD - 1, FOLD, FOLD + 1, SCAN - 2, SCAN - 1, SCAN, SCAN + 1)})


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result for a case, computed once and read only."""
    out = assemble(CASES[name]())
    for s, _, _ in out:
        s.setflags(write=False)
    return out


def mode1_clips(case):
    return [(k, i, c) for k, (cl, v) in enumerate(zip(case["classes"], case["vad"])) if v for i, c in enumerate(cl)]
