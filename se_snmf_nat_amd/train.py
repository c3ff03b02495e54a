"""Host mirror of the basis-training caller, run_basis_train.m:58-136, for ONE event class whose
training signal has already been assembled, and of the assembly itself (:16-57) for the clips of many
classes at once (reading and shuffling the wav files stays with the caller).  Everything numeric runs
on the GPU: the assembly, features (frontend.py), both sparse_nmf solves (api.py); this module only
sequences them like the reference does.

    out = run_basis_train_signal(s_full, R, p)        # B_DFT_sub, B_Mel_sub, A_DFT_sub, A_Mel_sub
    [out_k] = run_basis_train_signal_batch(signals, R, p)      # the same for a list of signals (one per class), solved together
    ts = assemble_training_signals(classes, p, vad=...)        # run_basis_train.m:16-57: every class's s_full from its clips, in HBM
    [out_k] = run_basis_train_assembled_batch(ts, R, p)        # run_basis_train_signal_batch on those resident signals
    [out_k] = run_basis_train_clips_batch(classes, R, p)       # both steps: clips in, dictionaries out
    save_basis_mat(path, out)                         # R_<R>.mat with the reference's variable names
    B_hat = run_basis_DNMF(x, d, B, p)                # run_basis_DNMF.m:1      (waveforms in, like the reference)
    B_hat = run_basis_DNMF_Mel(x, d, B, p)            # run_basis_DNMF_Mel.m:1
    [(B_hat, A_hat)] = run_basis_DNMF_batch(xs, ds, B, p)      # the same for a list of waveform pairs, solved together
    [(B_hat, A_hat)] = run_basis_DNMF_Mel_batch(xs, ds, B, p)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, frontend
from .api import SnmfError, _check_precision, _fp64_rules, _make_params, _ptr, _solver_scalars, default_context
from .batch import (_dnmf_rank_inputs, _dnmf_rank_pairs, _dnmf_rank_params, _ints_per_problem, _problem_settings, _ptr_or_null, _ptrs,
                    _settings_array)


def run_basis_train_signal(s_full, R, p, *, DC_bin=None, sample_idx=None, ctx=None, h0="host", precision="fp32", info=None):
    """run_basis_train.m:58-136.  `p`: the reference's settings fields (front-end fields of
    frontend.default_params() plus cf/sparsity/max_iter/conv_eps/cost_check, cluster_buff,
    train_Exemplar).  sample_idx: the exemplar columns (1-based like randsample, :81); default = a
    seeded numpy draw standing in for MATLAB's rng(1); randsample(...).  cluster_buff > 1: the dictionary is trained
    with cluster_buff*R atoms and reduced to R by kmeans.reduce_rank (:118-127; p["kmeans_seed"] seeds its draws).

    ONE call across the C ABI (include/snmf.h: snmf_run_basis_train_audio_f64): TF_mag, TF_DD, TF_Mel, the exemplar columns and
    both solves stay in HBM -- only the audio goes in and the dictionaries (and activations) come out.
    h0: "host" = the rand(r, n) both sparse_nmf calls draw after re-seeding (src/sparse_nmf.m:112-114,:133-134; RandomState
    stand-in) is drawn here and uploaded; "device" = drawn on the device (api.philox_uniform).
    precision: "fp32" (default) = float samples, fp32 features and solves; "fp64" = snmf_run_basis_train_audio_fp64: the signal
    crosses as float64 and features, Mel projection, exemplars and both solves are computed in double.  Any other string is a
    ValueError.  The returned arrays are float64 in both.  info: a dict that receives info["n_iter"] = [n_dft, n_mel]."""
    _check_precision(precision)
    f64 = precision == "fp64"
    sdt = np.float64 if f64 else np.float32
    p = dict(p)
    cluster_buff = int(p.get("cluster_buff", 1))
    exemplar = bool(p.get("train_Exemplar", 0))
    if cluster_buff > 1 and exemplar:
        # :125-126 index the activation matrices, which :95-96 set to the scalar 0 in exemplar mode: MATLAB stops there too
        raise SnmfError(3, "cluster_buff > 1 needs train_Exemplar = 0 (run_basis_train.m:125-126 index A_*_init, a scalar otherwise)")
    fp = dict(p)
    if DC_bin is not None:
        fp["DCbin"] = int(DC_bin)
    s = np.ascontiguousarray(np.asarray(s_full, dtype=sdt).reshape(-1))
    sp, _win = frontend._params(fp)
    lib = _lib.load()
    T = int(lib.snmf_stft_num_frames(C.byref(sp), s.size))
    K = 2 * sp.splice + 1
    F, M = K * (sp.fftlength // 2 + 1), int(p["F_order"])
    n_ex = cluster_buff * int(R)
    if T < 1:
        raise SnmfError(3, "the training signal is shorter than one analysis frame")
    if sample_idx is None:
        sample_idx = np.random.RandomState(1).choice(T, size=n_ex, replace=False) + 1  # :80-81 stand-in
    idx0 = np.ascontiguousarray(np.asarray(sample_idx, dtype=np.int64).reshape(-1) - 1)
    if idx0.size != n_ex or idx0.min() < 0 or idx0.max() >= T:
        raise SnmfError(3, "sample_idx must hold cluster_buff*R valid 1-based column indices")
    if exemplar:
        beta, max_iter, conv_eps, cost_check, lam = 1.0, 1, 0.0, 0, 0.0
    else:
        beta, max_iter, conv_eps, cost_check, lam = _solver_scalars(p)
    q = _make_params(F, T, n_ex, beta, max_iter, conv_eps, cost_check, True, 0, lam, None, None)
    seed = int(p.get("random_seed", 1))
    H0 = None
    if h0 == "host" and not exemplar:
        H0 = np.asfortranarray(np.random.RandomState(seed if seed > 0 else None).random_sample((n_ex, T)))
    mel = np.ascontiguousarray(frontend.mel_matrix(p["fs"], M, p["fftlength"], 1.0, p["fs"] / 2).T, dtype=sdt)
    B_DFT = np.empty((F, n_ex), order="F")
    B_Mel = np.empty((K * M, n_ex), order="F")
    A_DFT = A_Mel = 0  # :95-96
    if not exemplar:
        A_DFT = np.empty((n_ex, T), order="F")
        A_Mel = np.empty((n_ex, T), order="F")
    nit = np.zeros(2, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else None
    ctx = ctx or default_context()
    fn = lib.snmf_run_basis_train_audio_fp64 if f64 else lib.snmf_run_basis_train_audio_f64
    _lib.check(fn(
        ctx._h, C.byref(q), C.byref(sp), float(p["alpha_eta"]) if p.get("domain_DD", 0) else -1.0, ptr(mel), M, ptr(s), s.size,
        ptr(idx0), 1 if exemplar else 0, ptr(H0), seed, ptr(B_DFT), ptr(A_DFT), ptr(B_Mel), ptr(A_Mel), ptr(nit)))
    if info is not None:
        info["n_iter"] = [int(v) for v in nit]
    B_DFT = B_DFT / np.sqrt((B_DFT ** 2).sum(0)) + 1e-9  # :113-114
    B_Mel = B_Mel / np.sqrt((B_Mel ** 2).sum(0)) + 1e-9  # :115-116
    if cluster_buff > 1:  # :118-127: keep one basis vector per cluster of the Mel dictionary (host logic, as in the reference)
        from .kmeans import reduce_rank
        B_Mel, B_DFT, A_DFT, A_Mel, _ = reduce_rank(B_Mel, B_DFT, A_DFT, A_Mel, int(R), seed=int(p.get("kmeans_seed", 1)))
    return {"B_DFT_sub": B_DFT, "B_Mel_sub": B_Mel, "A_DFT_sub": A_DFT, "A_Mel_sub": A_Mel}  # :130-134


def run_basis_train_signal_batch(signals, R, p, *, DC_bin=None, sample_idx=None, ctx=None, h0="host", precision="fp32", info=None,
                                 settings=None):
    """[run_basis_train_signal(s_k, R, p, ...) for s_k in signals], solved together: the loop l = 1:length(DB_path_list) of
    run_basis_train.m, one training signal per event class or noise type, in ONE call across the C ABI
    (snmf_run_basis_train_audio_batch_f64; precision="fp64": _fp64).  The signals (any lengths) go up as one slab, TF_mag, TF_DD and
    TF_Mel of all of them are formed in HBM by shared launches, the exemplar columns are gathered there, and the DFT and the Mel
    solves are two resident batches.  p and DC_bin are shared.  Returns a list of the dicts run_basis_train_signal returns.
    R: one dictionary size for every problem, or a sequence with one per problem (the reference trains events with R_x and noise
    with R_d, Do_MultiBatch_IS16_20160324.m:107,135).  Equal entries are the scalar call in both precisions; differing ones need
    precision="fp64" (snmf_run_basis_train_audio_batch_ranks_fp64; SnmfError status 8 in fp32).  Problem k then has
    n_ex_k = cluster_buff * R_k exemplar columns in its default sample_idx, its H0 and its results, and the host epilogue
    (renormalise + 1e-9, reduce_rank to R_k when cluster_buff > 1) runs with its own R_k.
    settings: None, or a list with one dict per problem with keys among cf, beta, sparsity, max_iter, conv_eps (a missing key takes
    p's value): both solves of problem k run with its own settings (snmf_run_basis_train_audio_batch_settings_fp64), bit for bit
    run_basis_train_signal(s_k, R_k, dict(p, **settings[k]), precision="fp64") alone.  precision="fp64" only (status 8 in fp32);
    a list of another length is status 3, an unknown key status 1, a vector sparsity status 8.  The host epilogue is unchanged.

    sample_idx: None = every problem gets the single call's own stand-in draw, RandomState(1).choice(T_k, cluster_buff*R,
    replace=False) + 1 (the reference re-seeds per class, :80-81); else a list of 1-based index arrays, one per problem.
    h0: "host" = every problem gets the draw the single call makes, RandomState(random_seed).random_sample((n_ex, T_k)) -- the same
    seed for every problem, since the reference re-seeds inside every sparse_nmf call; "device" = drawn on the device from
    random_seed, for every problem.  Both solves of a problem start from the same H0, as in the single call.
    precision="fp64": problem k is bit for bit run_basis_train_signal(s_k, R_k, p, precision="fp64", ...) alone.
    precision="fp32": the fp32 batch engine (F <= 513, cluster_buff*R <= 200): bit for bit sparse_nmf_batch(precision="fp32") on
    the fp32 features stft_features (then tf_dd, then mel_features on that) give for s_k, with init_w their columns sample_idx_k.
    Any other string is a ValueError.  info["T"] receives the frame counts, info["n_iter"] a list of [n_dft, n_mel].
    Every argument error is raised before the library is loaded."""
    return _train_batch(signals, None, R, p, DC_bin=DC_bin, sample_idx=sample_idx, ctx=ctx, h0=h0, precision=precision, info=info,
                        settings=settings)


def _train_settings(settings, n, p, precision):
    """settings of the batched training calls -> None, or the list of (beta, sparsity, max_iter, conv_eps) per problem
    (batch._problem_settings with p's values as the shared ones).  fp64 only: SnmfError status 8 in fp32."""
    if settings is None:
        return None
    if precision != "fp64":
        raise SnmfError(8, "settings per problem need precision='fp64': the fp32 batch engine has one settings struct for all problems")
    beta, max_iter, conv_eps, _cc, lam = _solver_scalars(p)
    return _problem_settings(settings, n, dict(beta=beta, sparsity=lam, max_iter=max_iter, conv_eps=conv_eps))


def _train_ranks(R, n, precision):
    """R of the batched training calls: an int (one dictionary size for every problem) -> None; a sequence with one entry per
    problem -> the list when the entries differ (fp64 only: SnmfError status 8 in fp32), None when they are equal (the scalar
    call).  Its own errors: a length that is not n (3), an entry below 1 (1)."""
    Rs = _ints_per_problem(R, n, "R")
    if Rs is None or len(set(Rs)) == 1:
        return None
    if precision != "fp64":
        raise SnmfError(8, "differing R need precision='fp64': the fp32 batch engine has one rank for all problems")
    return Rs


def _train_batch(signals, ts, R, p, *, DC_bin, sample_idx, ctx, h0, precision, info, settings=None):
    """run_basis_train_signal_batch (ts None: host signals through snmf_run_basis_train_audio_batch_*) and
    run_basis_train_assembled_batch (ts: a TrainSignals, through snmf_run_basis_train_signals_batch_*): the same checks, draws,
    call and host epilogue; only where the samples come from differs."""
    _check_precision(precision)
    f64 = precision == "fp64"
    sdt = np.float64 if f64 else np.float32
    p = dict(p)
    cluster_buff = int(p.get("cluster_buff", 1))
    exemplar = bool(p.get("train_Exemplar", 0))
    if cluster_buff > 1 and exemplar:
        raise SnmfError(3, "cluster_buff > 1 needs train_Exemplar = 0 (run_basis_train.m:125-126 index A_*_init, a scalar otherwise)")
    fp = dict(p)
    if DC_bin is not None:
        fp["DCbin"] = int(DC_bin)
    if ts is None:
        sigs = [np.ascontiguousarray(np.asarray(s, dtype=sdt).reshape(-1)) for s in signals]
        sizes = [s.size for s in sigs]
    else:
        sizes = [int(v) for v in ts.lengths]
    n = len(sizes)
    if n == 0:
        raise SnmfError(1, "the batch is empty: signals must hold at least one waveform")
    if not isinstance(h0, str) or h0 not in ("host", "device"):
        raise SnmfError(3, "h0 must be 'host' or 'device'")
    K = 2 * int(fp.get("Splice", 0)) + 1
    F, M = K * (int(fp["fftlength"]) // 2 + 1), int(p["F_order"])
    Rk = _train_ranks(R, n, precision)  # a list only when the problems' R differ
    st = None if exemplar else _train_settings(settings, n, p, precision)  # (the exemplars are the dictionaries: nothing is solved)
    Rs = Rk if Rk is not None else [int(np.asarray(R).reshape(-1)[0])] * n
    n_exs = [cluster_buff * r for r in Rs]
    Ts = [frontend.num_frames_host(size, fp) for size in sizes]
    for k, (T, n_ex) in enumerate(zip(Ts, n_exs)):
        if T < 1:
            raise SnmfError(3, f"the training signal of problem {k} is shorter than one analysis frame")
        if n_ex > T:
            raise SnmfError(3, f"problem {k} has {T} frames, fewer than cluster_buff*R = {n_ex} exemplar columns")
    if sample_idx is None:  # :80-81 stand-in, per class
        sample_idx = [np.random.RandomState(1).choice(T, size=n_ex, replace=False) + 1 for T, n_ex in zip(Ts, n_exs)]
    elif len(sample_idx) != n:
        raise SnmfError(3, f"sample_idx is a list of {len(sample_idx)}, the batch has {n} problems")
    idx0 = [np.ascontiguousarray(np.asarray(ix, dtype=np.int64).reshape(-1) - 1) for ix in sample_idx]
    for k, (ix, T) in enumerate(zip(idx0, Ts)):
        if ix.size != n_exs[k] or ix.min() < 0 or ix.max() >= T:
            raise SnmfError(3, f"sample_idx of problem {k} must hold cluster_buff*R valid 1-based column indices")
    if exemplar:
        beta, max_iter, conv_eps, cost_check, lam = 1.0, 1, 0.0, 0, 0.0
    else:
        beta, max_iter, conv_eps, cost_check, lam = _solver_scalars(p)
    if st is not None:
        max_iter = max(s[2] for s in st)  # the handles': the largest
    q = _make_params(F, 1, max(n_exs), beta, max_iter, conv_eps, cost_check, True, 0, lam, None, None)
    seed = int(p.get("random_seed", 1))
    H0s = seeds = None
    if not exemplar:
        if h0 == "host":
            H0s = [np.asfortranarray(np.random.RandomState(seed if seed > 0 else None).random_sample((n_ex, T))) for T, n_ex in zip(Ts, n_exs)]
        else:
            seeds = np.full(n, seed, np.uint64)
    mel = frontend._mel_table(p, sdt)
    sp, _win = frontend._params(fp)

    lib = _lib.load()
    ctx = ts._ctx if ts is not None else (ctx or default_context())
    B_DFT = [np.empty((F, n_ex), order="F") for n_ex in n_exs]
    B_Mel = [np.empty((K * M, n_ex), order="F") for n_ex in n_exs]
    A_DFT = A_Mel = None
    if not exemplar:
        A_DFT = [np.empty((n_ex, T), order="F") for T, n_ex in zip(Ts, n_exs)]
        A_Mel = [np.empty((n_ex, T), order="F") for T, n_ex in zip(Ts, n_exs)]
    n_iter = np.zeros(2 * n, np.int32)
    alpha = float(p["alpha_eta"]) if p.get("domain_DD", 0) else -1.0
    atoms, lens = np.array(n_exs, np.int32), np.array(sizes, np.int64)
    # the entry: where the samples come from, then the form; its arguments: the source's head, n_atoms where the form has it
    # (NULL for one size), the shared tail, the settings where the form has them
    form = "settings_fp64" if st is not None else "ranks_fp64" if Rk is not None else "fp64" if f64 else "f64"
    args = (n, _ptrs(sigs), _ptr(lens)) if ts is None else (ts._handle(),)
    if st is not None or Rk is not None:
        args += (_ptr(atoms) if Rk is not None else None,)
    args += (_ptrs(idx0), 1 if exemplar else 0, _ptrs(H0s), _ptr_or_null(seeds), _ptrs(B_DFT), _ptrs(A_DFT), _ptrs(B_Mel), _ptrs(A_Mel),
             _ptr(n_iter))
    if st is not None:
        args += (_settings_array(st),)
    entry = getattr(lib, f"snmf_run_basis_train_{'audio' if ts is None else 'signals'}_batch_{form}")
    _lib.check(entry(ctx._h, C.byref(q), C.byref(sp), alpha, _ptr(mel), M, *args))
    if info is not None:
        info["T"] = list(Ts)
        info["n_iter"] = [[int(v) for v in n_iter[2 * k:2 * k + 2]] for k in range(n)]
    out = []
    for k in range(n):  # the host epilogue of the single call, per problem
        bd = B_DFT[k] / np.sqrt((B_DFT[k] ** 2).sum(0)) + 1e-9  # :113-114
        bm = B_Mel[k] / np.sqrt((B_Mel[k] ** 2).sum(0)) + 1e-9  # :115-116
        ad, am = (0, 0) if exemplar else (A_DFT[k], A_Mel[k])  # :95-96
        if cluster_buff > 1:  # :118-127
            from .kmeans import reduce_rank
            bm, bd, ad, am, _ = reduce_rank(bm, bd, ad, am, Rs[k], seed=int(p.get("kmeans_seed", 1)))
        out.append({"B_DFT_sub": bd, "B_Mel_sub": bm, "A_DFT_sub": ad, "A_Mel_sub": am})  # :130-134
    return out


class TrainSignals:
    """The training signals of every class, assembled and resident on the device (snmf_train_signals of include/snmf.h).
    .lengths / .clips_used: per class, samples of s_full and clips consumed (run_basis_train.m:46-57); .signal(k): s_full of class
    k as float64 (:96 writes it ./ 32767 as the class's wav); .close() gives the device memory back (also a context manager)."""

    def __init__(self, handle, ctx, lengths, clips_used):
        self._h, self._ctx = handle, ctx
        self.lengths, self.clips_used = list(lengths), list(clips_used)

    def _handle(self):
        if self._h is None:
            raise SnmfError(7, "the training signals have been closed")
        return self._h

    def signal(self, k):
        k = int(k)
        if not 0 <= k < len(self.lengths):
            raise SnmfError(3, f"class {k} of {len(self.lengths)}")
        s = np.empty(self.lengths[k], np.float64)
        _lib.check(_lib.load().snmf_train_signals_get_f64(self._handle(), k, C.c_void_p(s.ctypes.data)))
        return s

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            _lib.load().snmf_train_signals_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _whole(x, what):
    """An integer-valued setting (0.05 * fs samples): the integer, or SnmfError."""
    r = round(float(x))
    if abs(float(x) - r) > 1e-9 * max(1.0, abs(float(x))):
        raise SnmfError(1, f"{what} = {x} is not a whole number of samples")
    return int(r)


def assemble_training_signals(classes, p, *, vad=None, ranges=None, ctx=None):
    """run_basis_train.m:16-57 for every class at once, on the device (snmf_train_signals_assemble_*): -> TrainSignals.
    classes: a list (one entry per event class or noise type) of lists of 1-D arrays, the clips in the order they are consumed --
    the caller applies randperm and clip_subsample (:17, :21).  int16 clips are PCM (s = pcm / 32768 * 32767, what wavread(.) *
    32767 gives, :26-27) and cross as 2 bytes per sample; any other dtype is taken as doubles already scaled like that (a mix
    crosses as doubles).  p: fs, train_seq_len_max, train_file_len_max (samples; <= 0: no cut).
    vad: one bool per class (VAD_set, default all False): silence is removed by vadenergy_simple with bg_len = 0.05 * fs,
    frame_len = 0.02 * fs, thr = 0.7 (:32-36) and nonzeros(s .* vad) (:37).  ranges: per class None, or one (v_start, v_end) per
    clip (1-based, inclusive, what load_anot returns for p.train_ANOT, :38-40; v_start = 0 becomes 1 and v_end is clamped to the
    clip, src/load_anot.m:9-15).  A class with neither is cut to train_file_len_max per clip (:41-43).
    Every clip is then scaled to unit variance and a peak of 30000 (:44-45) and appended until the length exceeds
    train_seq_len_max (:46-57).  Where the reference would produce NaN -- a consumed clip with one kept sample or no variance --
    the call fails (SnmfError status 1, naming class and clip).  Every argument error is raised before the library is loaded."""
    p = dict(p)
    if not isinstance(classes, (list, tuple)) or len(classes) == 0:
        raise SnmfError(1, "classes must be a list with at least one class")
    n = len(classes)
    fs = float(p["fs"])
    bg_len, frame_len = _whole(0.05 * fs, "bg_len = 0.05 * fs"), _whole(0.02 * fs, "frame_len = 0.02 * fs")
    if frame_len < 2 or frame_len % 2:
        raise SnmfError(1, f"frame_len = 0.02 * fs = {frame_len} must be even and at least 2 (frame_shift = frame_len / 2)")
    if bg_len < 1:
        raise SnmfError(1, f"bg_len = 0.05 * fs = {bg_len} must be at least 1")
    seq_max, file_max = int(p["train_seq_len_max"]), int(p["train_file_len_max"])
    if seq_max < 0:
        raise SnmfError(1, "train_seq_len_max is negative")
    vad = [False] * n if vad is None else [bool(v) for v in vad]
    if len(vad) != n:
        raise SnmfError(1, f"vad has {len(vad)} entries, there are {n} classes")
    ranges = [None] * n if ranges is None else list(ranges)
    if len(ranges) != n:
        raise SnmfError(1, f"ranges has {len(ranges)} entries, there are {n} classes")
    clips, modes, rng = [], [], []
    for k, cl in enumerate(classes):
        if not isinstance(cl, (list, tuple)) or len(cl) == 0:
            raise SnmfError(1, f"class {k} has no clip")
        mode = 1 if vad[k] else (2 if ranges[k] is not None else 0)
        if mode == 2 and len(ranges[k]) != len(cl):
            raise SnmfError(1, f"class {k} has {len(cl)} clips and {len(ranges[k])} ranges")
        modes.append(mode)
        for i, c in enumerate(cl):
            c = np.asarray(c)
            if c.ndim != 1:
                raise SnmfError(3, f"clip {i} of class {k} is not a vector")
            if c.size < 1:
                raise SnmfError(3, f"clip {i} of class {k} has no sample")
            if mode == 1 and c.size < bg_len:
                raise SnmfError(3, f"clip {i} of class {k} has {c.size} samples, fewer than bg_len = {bg_len}")
            a, b = 1, c.size
            if mode == 2:
                a, b = (int(v) for v in ranges[k][i])
                a, b = (1 if a == 0 else a), min(b, c.size)  # src/load_anot.m:9-15
                if a < 1 or a > b:
                    raise SnmfError(3, f"the range {tuple(ranges[k][i])} of clip {i} of class {k} is not inside [1, {c.size}]")
            clips.append(c)
            rng += [a, b]
    pcm = all(c.dtype == np.int16 for c in clips)
    if pcm:
        clips = [np.ascontiguousarray(c) for c in clips]
    else:  # (an int16 clip among doubles: its exact double values)
        clips = [np.ascontiguousarray(c.astype(np.float64) / 32768 * 32767 if c.dtype == np.int16 else np.asarray(c, dtype=np.float64))
                 for c in clips]
    ap = _lib.SnmfAssembleParams(frame_len, bg_len, 0.7, seq_max, file_max)
    n_clips = np.array([len(cl) for cl in classes], np.int32)
    lens = np.array([c.size for c in clips], np.int64)
    modes = np.array(modes, np.int32)
    rng = np.array(rng, np.int64)

    lib = _lib.load()
    ctx = ctx or default_context()
    h = C.c_void_p()
    cp = (C.c_void_p * len(clips))(*[c.ctypes.data for c in clips])
    fn = lib.snmf_train_signals_assemble_i16 if pcm else lib.snmf_train_signals_assemble_f64
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.check(fn(ctx._h, C.byref(ap), n, vp(n_clips), cp, vp(lens), vp(modes), vp(rng), C.byref(h)))
    length, used = np.zeros(n, np.int64), np.zeros(n, np.int32)
    _lib.check(lib.snmf_train_signals_info(h, None, vp(length), vp(used)))
    return TrainSignals(h, ctx, [int(v) for v in length], [int(v) for v in used])


def run_basis_train_assembled_batch(ts, R, p, *, DC_bin=None, sample_idx=None, h0="host", precision="fp32", info=None, settings=None):
    """run_basis_train_signal_batch([ts.signal(k) for k ...], R, p, ...) without the signals leaving the device
    (snmf_run_basis_train_signals_batch_*): same arguments, same draws (T_k comes from ts.lengths, so the default sample_idx and the
    host H0 are that call's own), same returned list, bit for bit -- in fp32 the resident doubles are rounded to float on the
    device as np.float32 rounds them.  It runs on the context the signals were assembled on.  settings: as in that call
    (snmf_run_basis_train_signals_batch_settings_fp64)."""
    if not isinstance(ts, TrainSignals):
        raise SnmfError(1, "ts must be the TrainSignals assemble_training_signals returns")
    ts._handle()
    return _train_batch(None, ts, R, p, DC_bin=DC_bin, sample_idx=sample_idx, ctx=None, h0=h0, precision=precision, info=info,
                        settings=settings)


def run_basis_train_clips_batch(classes, R, p, *, vad=None, ranges=None, DC_bin=None, sample_idx=None, ctx=None, h0="host", precision="fp32",
                                info=None, settings=None):
    """assemble_training_signals, run_basis_train_assembled_batch, close: the clips of every class in, the dictionaries out.
    info also receives info["lengths"] and info["clips_used"].  The argument errors of either step that do not need the assembled
    lengths are raised before the library is loaded; those that do (sample_idx, R against T_k) after the assembly.
    settings: as in run_basis_train_signal_batch."""
    _check_precision(precision)
    if not isinstance(h0, str) or h0 not in ("host", "device"):
        raise SnmfError(3, "h0 must be 'host' or 'device'")
    if int(p.get("cluster_buff", 1)) > 1 and p.get("train_Exemplar", 0):
        raise SnmfError(3, "cluster_buff > 1 needs train_Exemplar = 0 (run_basis_train.m:125-126 index A_*_init, a scalar otherwise)")
    if not p.get("train_Exemplar", 0):
        _solver_scalars(p)
    if isinstance(classes, (list, tuple)):
        _train_ranks(R, len(classes), precision)
        if not p.get("train_Exemplar", 0):
            _train_settings(settings, len(classes), p, precision)
    frontend._params(p if DC_bin is None else dict(p, DCbin=int(DC_bin)))
    with assemble_training_signals(classes, p, vad=vad, ranges=ranges, ctx=ctx) as ts:
        if info is not None:
            info["lengths"], info["clips_used"] = list(ts.lengths), list(ts.clips_used)
        return run_basis_train_assembled_batch(ts, R, p, DC_bin=DC_bin, sample_idx=sample_idx, h0=h0, precision=precision, info=info,
                                               settings=settings)


def save_basis_mat(path, out, v73=True):
    """run_basis_train.m:136: `save(..., 'B_DFT_sub', 'B_Mel_sub', 'A_DFT_sub', 'A_Mel_sub', '-v7.3')` -- an HDF5-based MAT-file
    (se_snmf_nat_amd/mat73.py); v73=False writes MAT-5 like the three .mat files the reference ships (basis/*/R_100.mat, B_D_u.mat).
    MATLAB's `load` reads either."""
    vars_ = {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}
    if v73:
        from .mat73 import save_mat73
        save_mat73(path, vars_)
    else:
        import scipy.io as sio
        sio.savemat(path, vars_, do_compression=True)


def load_basis_mat(path):
    """run_basis_train.m:138 / src/NTF_sep_event_RT.m:28-38: `load` of a dictionary file, MAT-5 or -v7.3 (what the reference's own
    run_basis_train.m:136 writes)."""
    from .mat73 import is_mat73, load_mat73
    if is_mat73(path):
        return load_mat73(path)
    import scipy.io as sio
    m = sio.loadmat(path)
    return {k: v for k, v in m.items() if not k.startswith("__")}


def _dnmf_features(x, d, p, ctx):
    """run_basis_DNMF.m:3-34: equal lengths, y = x + d (waveform sum), three spectrogram feature sets on the GPU
    (returned to the host: the resident entry below forms them in HBM instead)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    n = min(len(x), len(d))  # :5-9
    x, d = x[:n], d[:n]
    y = x + d  # :10
    return tuple(frontend.stft_features(sig, p, ctx=ctx) for sig in (y, x, d))  # :13-34


def _run_basis_dnmf_audio(x, d, B, p, *, ctx, mel, h0, want_a=False, precision="fp32", dtype=None, info=None):
    """ONE call across the C ABI (snmf_run_basis_dnmf_audio_f64; precision="fp64": snmf_run_basis_dnmf_audio_fp64, waveforms and
    Mel table as float64): the waveforms go in, B_hat comes out; features, A_hat and all three V matrices stay in HBM.
    h0: "host", "device", or the r x T array itself; info["n_iter"] receives [n1, n2, n3]."""
    f64 = precision == "fp64"
    sdt = np.float64 if f64 else np.float32
    x = np.ascontiguousarray(np.asarray(x, dtype=sdt).reshape(-1))
    d = np.ascontiguousarray(np.asarray(d, dtype=sdt).reshape(-1))
    sp, _win = frontend._params(p)
    lib = _lib.load()
    R_x, R_d = int(p["R_x"]), int(p["R_d"])
    r = R_x + R_d
    T = int(lib.snmf_stft_num_frames(C.byref(sp), min(x.size, d.size)))
    K = 2 * sp.splice + 1
    M = int(p["F_order"]) if mel else 0
    F = K * M if mel else K * (sp.fftlength // 2 + 1)
    if T < 1:
        raise SnmfError(3, "the signals are shorter than one analysis frame")
    B = np.asfortranarray(B, dtype=np.float64)
    if B.shape != (F, r):
        raise SnmfError(3, f"B is {B.shape}, expected ({F}, {r})")
    beta, max_iter, conv_eps, cost_check, lam = _solver_scalars(p)
    q = _make_params(F, T, r, beta, max_iter, conv_eps, cost_check, True, 0, lam, None, None)
    if f64:  # (after the reference's own errors, before any device work)
        _fp64_rules(dtype, None, "the fp64 DNMF caller")
    seed = int(p.get("random_seed", 1))
    H0 = None
    if not isinstance(h0, str):
        H0 = np.asfortranarray(h0, dtype=np.float64)
        if H0.shape != (r, T):
            raise SnmfError(3, f"init_h is {H0.shape}, expected ({r}, {T})")
    elif h0 == "host":
        H0 = np.asfortranarray(np.random.RandomState(seed if seed > 0 else None).random_sample((r, T)))
    melm = np.ascontiguousarray(frontend.mel_matrix(p["fs"], M, p["fftlength"], 1.0, p["fs"] / 2).T, dtype=sdt) if mel else None
    B_hat = np.empty((F, r), order="F")
    A_hat = np.empty((r, T), order="F") if want_a else None
    nit = np.zeros(3, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    ctx = ctx or default_context()
    fn = lib.snmf_run_basis_dnmf_audio_fp64 if f64 else lib.snmf_run_basis_dnmf_audio_f64
    _lib.check(fn(ctx._h, C.byref(q), C.byref(sp), R_x, R_d, ptr(x), x.size, ptr(d), d.size, ptr(melm), M,
                  ptr(B), F, ptr(H0), seed, ptr(B_hat), F, ptr(A_hat), r, ptr(nit)))
    if info is not None:
        info["n_iter"] = [int(v) for v in nit]
    return (B_hat, A_hat) if want_a else B_hat


def _check_dtype(dtype):
    """`dtype` of the callers below: accepted for callers written against the round-3 signature.  The entry they go through takes
    the waveforms as fp32 (the device front-end's sample type: y = x + d of run_basis_DNMF.m:10 is formed in fp32 on the device,
    INTEGRATION.md) and returns fp64; any other request is an error rather than silently something else."""
    if dtype is not None and np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise SnmfError(1, "dtype must be float64 or float32")


def run_basis_DNMF(x, d, B, p, *, ctx=None, h0="host", dtype=None, precision="fp32"):
    """B_hat = run_basis_DNMF(x, d, B, p) -- run_basis_DNMF.m:1: clean and noise waveforms, exemplar basis
    B = [B_x, B_d] (F x (R_x+R_d)); p carries the front-end fields, R_x, R_d and the solver fields.
    precision="fp64": the waveforms cross as float64 and y = x + d, the features and the three solves are computed in double
    (dtype=np.float32 is then SnmfError status 1); any other string than "fp32" / "fp64" is a ValueError."""
    _check_precision(precision)
    _check_dtype(dtype)
    return _run_basis_dnmf_audio(x, d, B, p, ctx=ctx, mel=False, h0=h0, precision=precision, dtype=dtype)  # :1-55


def run_basis_DNMF_Mel(x, d, B, p, *, ctx=None, h0="host", dtype=None, precision="fp32"):
    """B_hat = run_basis_DNMF_Mel(x, d, B, p) -- run_basis_DNMF_Mel.m:1: the same loop on the Mel projections of
    the three feature sets (:21-69); B is the Mel exemplar basis (F_order*(2*Splice+1) rows).  precision: as in run_basis_DNMF."""
    _check_precision(precision)
    _check_dtype(dtype)
    return _run_basis_dnmf_audio(x, d, B, p, ctx=ctx, mel=True, h0=h0, precision=precision, dtype=dtype)  # :1-95


def _run_basis_dnmf_audio_batch(xs, ds, B, p, *, ctx, mel, h0, precision, dtype, info, settings=None):
    """ONE call across the C ABI (snmf_run_basis_dnmf_audio_batch_f64; precision="fp64": _fp64) for every waveform pair: the
    waveforms go up as one slab, the three feature sets of all problems are formed in HBM by shared launches, and the three
    solves are three resident batches.  Every error that needs no device is raised before the library is loaded.
    A sequence for p["R_x"] / p["R_d"] or settings per problem: snmf_run_basis_dnmf_audio_batch_ranks_fp64 (fp64 only).  One body
    for both: the uniform call is a rank pair n times (batch._dnmf_rank_inputs, _dnmf_rank_params), and only the entry and the
    head of its argument list differ.  The host draw is rand(r_k, T_k) per problem in list order from one generator; the device
    draw of problem k is philox_uniform(random_seed + k, r_k, T_k)."""
    _check_precision(precision)
    _check_dtype(dtype)
    f64 = precision == "fp64"
    sdt = np.float64 if f64 else np.float32
    p = dict(p)
    xs = [np.ascontiguousarray(np.asarray(x, dtype=sdt).reshape(-1)) for x in xs]
    ds = [np.ascontiguousarray(np.asarray(d, dtype=sdt).reshape(-1)) for d in ds]
    n = len(xs)
    if n == 0:
        raise SnmfError(1, "the batch is empty: xs must hold at least one waveform")
    if len(ds) != n:
        raise SnmfError(1, f"{n} clean and {len(ds)} noise waveforms: one of each per problem")
    pairs = _dnmf_rank_pairs(p["R_x"], p["R_d"], n, settings, precision)  # None: two scalars, the uniform entry
    Rxs, Rds = pairs or ([int(p["R_x"])] * n, [int(p["R_d"])] * n)
    rs = [a + b for a, b in zip(Rxs, Rds)]
    K = 2 * int(p.get("Splice", 0)) + 1
    M = int(p["F_order"]) if mel else 0
    F = K * M if mel else K * (int(p["fftlength"]) // 2 + 1)
    Ts = [frontend.num_frames_host(min(x.size, d.size), p) for x, d in zip(xs, ds)]  # run_basis_DNMF.m:5-9
    for k, T in enumerate(Ts):
        if T < 1:
            raise SnmfError(3, f"the signals of problem {k} are shorter than one analysis frame")
    seed = int(p.get("random_seed", 1))
    Bs, H0s = _dnmf_rank_inputs(B, h0, rs, F, Ts, ("host", "device"), p)  # "host": in list order from one generator
    q, sarr = _dnmf_rank_params(p, settings, n, F, max(rs))
    if f64:  # (after the reference's own errors, before any device work)
        _fp64_rules(dtype, None, "the fp64 DNMF batch")
    seeds = np.array([seed + k for k in range(n)], np.uint64) if H0s is None else None  # "device": philox_uniform(seed + k, r_k, T_k)
    melm = frontend._mel_table(p, sdt) if mel else None
    sp, _win = frontend._params(p)

    lib = _lib.load()
    ctx = ctx or default_context()
    B_hat = [np.empty((F, r), order="F") for r in rs]
    A_hat = [np.empty((r, T), order="F") for r, T in zip(rs, Ts)]
    n_iter = np.zeros(3 * n, np.int32)
    n_x, n_d = (np.array([a.size for a in v], np.int64) for v in (xs, ds))
    rx, rd = np.array(Rxs, np.int32), np.array(Rds, np.int32)
    if pairs is not None:
        entry, head = lib.snmf_run_basis_dnmf_audio_batch_ranks_fp64, (_ptr(rx), _ptr(rd), sarr)
    else:
        entry = lib.snmf_run_basis_dnmf_audio_batch_fp64 if f64 else lib.snmf_run_basis_dnmf_audio_batch_f64
        head = (Rxs[0], Rds[0])
    _lib.check(entry(ctx._h, C.byref(q), C.byref(sp), *head, n, _ptrs(xs), _ptr(n_x), _ptrs(ds), _ptr(n_d),
                     _ptr_or_null(melm), M, _ptrs(Bs), _ptrs(H0s), _ptr_or_null(seeds), _ptrs(B_hat), _ptrs(A_hat), _ptr(n_iter)))
    if info is not None:
        info["n_iter"] = [[int(v) for v in n_iter[3 * k:3 * k + 3]] for k in range(n)]
        info["T"] = list(Ts)
    return list(zip(B_hat, A_hat))


def run_basis_DNMF_batch(xs, ds, B, p, *, ctx=None, h0="host", precision="fp32", info=None, dtype=None, settings=None):
    """[(B_hat_k, A_hat_k)] = run_basis_DNMF(x_k, d_k, B_k, p) for every pair of the two lists of waveforms, solved together
    (snmf_run_basis_dnmf_audio_batch_*).  B: one F x (R_x + R_d) array for every problem, or a list of them; p: as for
    run_basis_DNMF, shared.  h0: "host" = rand(r, T_k) of solve 1 drawn per problem, in list order, from one
    RandomState(p["random_seed"]) (as run_basis_dnmf_batch); "device" = drawn on the device, problem k from
    philox_uniform(random_seed + k, r, T_k); or a list of r x T_k arrays.
    precision="fp32": float waveforms, fp32 features, the fp32 batch engine (F <= 513, R_x + R_d <= 200): bit for bit
    run_basis_dnmf_batch on the features stft_features gives for y_k = float32(x_k) + float32(d_k), x_k and d_k.
    precision="fp64": everything in double; problem k is bit for bit run_basis_DNMF(x_k, d_k, B_k, p, precision="fp64") alone
    with the same H0 (dtype=np.float32 is then SnmfError status 1).
    A rank pair per problem (precision="fp64" only, snmf_run_basis_dnmf_audio_batch_ranks_fp64): p["R_x"] and p["R_d"] may each be
    a sequence of len(xs) ints, as p["r"] may be for sparse_nmf_batch_fp64.  B is then a list of F x (R_x[k] + R_d[k]) arrays (one
    array only when every pair is the same); with r_k = R_x[k] + R_d[k], h0="host" draws rand(r_k, T_k) per problem in list order
    from the one RandomState, h0="device" draws problem k from philox_uniform(random_seed + k, r_k, T_k), and a list holds
    r_k x T_k arrays.  settings: one dict per problem with keys among cf, beta, sparsity, max_iter, conv_eps (a missing key takes
    p's value), held in all three solves of the problem.  Problem k stays bit for bit run_basis_DNMF alone with its own ranks and
    settings.  A sequence or settings with precision="fp32" is SnmfError status 8.
    info["n_iter"] receives a list of [n1, n2, n3], info["T"] the frame counts.  Returns a list of (B_hat, A_hat)."""
    return _run_basis_dnmf_audio_batch(xs, ds, B, p, ctx=ctx, mel=False, h0=h0, precision=precision, dtype=dtype, info=info,
                                       settings=settings)


def run_basis_DNMF_Mel_batch(xs, ds, B, p, *, ctx=None, h0="host", precision="fp32", info=None, dtype=None, settings=None):
    """run_basis_DNMF_batch on the Mel projections of the three feature sets (run_basis_DNMF_Mel.m:21-69); B: the Mel exemplar
    bases (F_order * (2 * Splice + 1) rows)."""
    return _run_basis_dnmf_audio_batch(xs, ds, B, p, ctx=ctx, mel=True, h0=h0, precision=precision, dtype=dtype, info=info,
                                       settings=settings)
