"""GPU tests of run_basis_train_signal_batch (snmf_run_basis_train_audio_batch_*): basis training for the signals of many classes
in one call -- the grouped front-end with TF_DD and both feature sets resident, the exemplar gather on the device (take_w0) and
the two batch engines.

The contracts are bit equalities with what is already shipped (np.array_equal throughout):
    fp64   problem k is run_basis_train_signal(s_k, R, p, sample_idx=idx_k, precision="fp64", h0=...) alone: the four arrays and
           both iteration counts;
    fp32   B and A of problem k are sparse_nmf_batch(precision="fp32") on the single front-end's fp32 features (stft_features, then
           tf_dd when on, and mel_features on that), widened to double, with init_w their columns idx_k and init_h the same H0,
           once for the DFT set and once for the Mel set, followed by the host epilogue of the single call.
Signals and settings: tests/train_batch_cases.py.  Against the oracle the bounds are the project's own: REL_SOLVE of
tests/test_gpu_train_f64.py in fp64 and the 2e-4 of tests/test_frontend.py::test_basis_training_caller_end_to_end in fp32, on the
waveform, settings and exemplar columns of those tests.

Measured on an MI355X (the tests print their own figures before they assert):
    [n_dft, n_mel] per problem, both modes   [20, 4] [20, 4] [18, 4] [10, 4] [19, 4] [10, 4]: the oracle's (tests/test_train_batch_api.py)
    problem 0 of a batch of two against the oracle, all four arrays   fp64 <= 9.4e-16 (bound 1e-11)   fp32 <= 1.9e-7 (bound 2e-4)
"""
import ctypes as C

import numpy as np
import pytest

import frontend_envelope as env
import train_batch_cases as tc
from test_gpu_train_f64 import IDX, REL_SOLVE, TRAIN_BASE, samples

pytestmark = pytest.mark.gpu
MODES = ["fp32", "fp64"]
REL_F32_END_TO_END = 2e-4  # tests/test_frontend.py::test_basis_training_caller_end_to_end
KEYS = ("B_DFT_sub", "B_Mel_sub", "A_DFT_sub", "A_Mel_sub")
VARIANTS = {
    "plain": (tc.R, tc.P_STOP),
    "domain_dd": (tc.R, dict(tc.P_STOP, domain_DD=1, alpha_eta=0.4)),
    "splice1_pow07_preemph": (tc.R, dict(tc.P_STOP, Splice=1, pow=0.7, preemph=0.92)),
    "ed": (tc.R, dict(tc.P_STOP, cf="ed")),
    "b05": (tc.R, dict(tc.P_STOP, cf="beta", beta=0.5)),
    "exemplar": (tc.R, dict(tc.P_STOP, train_Exemplar=1)),
    "cluster2": (3, dict(tc.P_STOP, cluster_buff=2, kmeans_seed=3)),
}


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def unit_columns(b):
    """run_basis_train.m:113-116 as the callers write it, on a Fortran-ordered double array like theirs (NumPy's column sums
    depend on the memory order of what they sum)."""
    b = np.asfortranarray(b, dtype=np.float64)
    return b / np.sqrt((b ** 2).sum(0)) + 1e-9


def run_batch(ctx, mode, name="plain", order=None, h0="host"):
    """-> [(out, [n_dft, n_mel])] of one call on the problems `order` of the cases (default: all, in order)."""
    from se_snmf_nat_amd import train
    R, p = VARIANTS[name]
    order = list(range(len(tc.TS))) if order is None else order
    info = {}
    out = train.run_basis_train_signal_batch([tc.signals()[k] for k in order], R, p, sample_idx=[tc.sample_idx()[k] for k in order], ctx=ctx,
                                             h0=h0, precision=mode, info=info)
    assert info["T"] == [tc.TS[k] for k in order]
    return list(zip(out, info["n_iter"]))


def same_bits(res, ref):
    assert len(res) == len(ref)
    for k, ((o, n), (orf, nr)) in enumerate(zip(res, ref)):
        assert list(n) == list(nr), (k, n, nr)
        for key in KEYS:
            g, w = o[key], orf[key]
            if np.isscalar(w):  # run_basis_train.m:95-96: the activations of the exemplar mode are the scalar 0
                assert np.isscalar(g) and g == w == 0, (k, key)
                continue
            assert g.dtype == w.dtype == np.float64 and g.shape == w.shape, (k, key, g.shape, w.shape)
            assert np.array_equal(g, w), (k, key, float(np.abs(g - w).max()))


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        for o, _ in _cache[key]:
            for v in o.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _cache[key]


def alone_fp64(ctx, name, h0="host"):
    """run_basis_train_signal(..., precision="fp64") per problem: the fp64 contract's reference."""
    from se_snmf_nat_amd import train
    R, p = VARIANTS[name]

    def make():
        out = []
        for s, ix in zip(tc.signals(), tc.sample_idx()):
            info = {}
            o = train.run_basis_train_signal(s, R, p, sample_idx=ix, ctx=ctx, h0=h0, precision="fp64", info=info)
            out.append((o, info["n_iter"]))
        return out
    return cached(("alone", name, h0), make)


def matrix_batch_fp32(ctx, name, h0="host"):
    """sparse_nmf_batch(precision="fp32") on the single front-end's fp32 features, DFT set and Mel set, then the host epilogue of the
    single call: the fp32 contract's reference."""
    from se_snmf_nat_amd import frontend as fe, sparse_nmf_batch
    from se_snmf_nat_amd.api import philox_uniform
    from se_snmf_nat_amd.kmeans import reduce_rank
    R, p = VARIANTS[name]
    n_ex = int(p["cluster_buff"]) * R

    def make():
        Vd, Vm, H0s = [], [], []
        for s, T in zip(tc.signals(), tc.TS):
            V = fe.stft_features(s, p, ctx=ctx)
            if p.get("domain_DD", 0):
                V = fe.tf_dd(V, p, ctx=ctx)
            Vd.append(V.astype(np.float64))
            Vm.append(fe.mel_features(V, p, ctx=ctx).astype(np.float64))
            H0s.append(tc.host_h0(T, p, n_ex) if h0 == "host" else philox_uniform(p["random_seed"], n_ex, T).astype(np.float64))
        W0d = [V[:, ix - 1] for V, ix in zip(Vd, tc.sample_idx())]
        W0m = [V[:, ix - 1] for V, ix in zip(Vm, tc.sample_idx())]
        if p["train_Exemplar"]:
            sol = [[(w, 0, {"n_iter": 0}) for w in W0] for W0 in (W0d, W0m)]
        else:
            q = {k: p[k] for k in ("cf", "beta", "sparsity", "max_iter", "conv_eps", "cost_check") if k in p}
            sol = [sparse_nmf_batch(Vs, dict(q, init_w=W0, init_h=H0s), ctx=ctx, precision="fp32") for Vs, W0 in ((Vd, W0d), (Vm, W0m))]
        out = []
        for (bd, ad, od), (bm, am, om) in zip(*sol):
            bd, bm = unit_columns(bd), unit_columns(bm)
            if p["cluster_buff"] > 1:
                bm, bd, ad, am, _ = reduce_rank(bm, bd, ad, am, R, seed=p["kmeans_seed"])
            out.append(({"B_DFT_sub": bd, "B_Mel_sub": bm, "A_DFT_sub": ad, "A_Mel_sub": am}, [od["n_iter"], om["n_iter"]]))
        return out
    return cached(("matrix", name, h0), make)


def reference(ctx, mode, name, **kw):
    return alone_fp64(ctx, name, **kw) if mode == "fp64" else matrix_batch_fp32(ctx, name, **kw)


def batch_of_all(ctx, mode, name="plain"):
    return cached(("batch", mode, name), lambda: run_batch(ctx, mode, name))


# ---- 1. / 2. the contracts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_the_shipped_paths_bit_for_bit(gpu_ctx, mode):
    res = batch_of_all(gpu_ctx, mode)
    n_dft = [n[0] for _, n in res]
    print(f"{mode}: [n_dft, n_mel] per problem {[n for _, n in res]}")
    same_bits(res, reference(gpu_ctx, mode, "plain"))
    assert tc.stops_are_spread(n_dft, tc.P_STOP["max_iter"]), n_dft  # (problems of one batch end at different iterations, as on the oracle)
    for o, _ in res:
        assert all(np.isfinite(o[k]).all() for k in KEYS)
        assert o["B_DFT_sub"].shape == (tc.F, tc.R) and o["B_Mel_sub"].shape == (tc.F_MEL, tc.R)


@pytest.mark.parametrize("mode", MODES)
def test_h0_drawn_on_the_device(gpu_ctx, mode):
    """fp64: the single call's own device draw with the same seed; fp32: philox_uniform(random_seed, n_ex, T_k) through the matrix form."""
    res = run_batch(gpu_ctx, mode, h0="device")
    same_bits(res, reference(gpu_ctx, mode, "plain", h0="device"))
    assert not np.array_equal(res[5][0]["A_DFT_sub"], batch_of_all(gpu_ctx, mode)[5][0]["A_DFT_sub"])  # (another start, another result)


@pytest.mark.parametrize("mode", MODES)
def test_a_problem_does_not_depend_on_the_batch_around_it(gpu_ctx, mode):
    res = batch_of_all(gpu_ctx, mode)
    order = list(range(len(tc.TS)))[::-1]
    same_bits(run_batch(gpu_ctx, mode, order=order)[::-1], res)
    for k in (0, 2, 5):  # every column an exemplar, a partial tile, several tiles
        same_bits(run_batch(gpu_ctx, mode, order=[k]), [res[k]])


# ---- 3. variants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["domain_dd", "splice1_pow07_preemph", "ed", "b05", "exemplar", "cluster2"])
@pytest.mark.parametrize("mode", MODES)
def test_variants_equal_the_shipped_paths_bit_for_bit(gpu_ctx, mode, name):
    res = batch_of_all(gpu_ctx, mode, name)
    same_bits(res, reference(gpu_ctx, mode, name))
    R, p = VARIANTS[name]
    K = 2 * p["Splice"] + 1
    assert res[0][0]["B_DFT_sub"].shape == (K * tc.F, R) and res[0][0]["B_Mel_sub"].shape == (K * tc.F_MEL, R)
    if name != "exemplar":
        assert res[0][0]["A_DFT_sub"].shape == (R, tc.TS[0])
    if name == "domain_dd":  # (and TF_DD is applied: another result than the plain one)
        assert not np.array_equal(res[5][0]["B_DFT_sub"], batch_of_all(gpu_ctx, mode)[5][0]["B_DFT_sub"])
    if name == "exemplar":  # in both modes the arrays of the single call, whose exemplars are its own front-end's columns
        from se_snmf_nat_amd import train
        for (o, n), s, ix in zip(res, tc.signals(), tc.sample_idx()):
            one = train.run_basis_train_signal(s, R, p, sample_idx=ix, ctx=gpu_ctx, precision=mode)
            same_bits([(o, n)], [(one, [0, 0])])


# ---- 4. the grouped TF_DD alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_grouped_tf_dd_columns_are_the_single_tf_dds(gpu_ctx, mode):
    """No feature-level entry takes domain_DD, so the columns are read through the exemplar mode, whose dictionaries are the
    gathered columns after the host epilogue: T = 1 (X_DD = X), 2, 33, 70, and 257 and 600 frames, which cross the 256-frame
    chunks of the recursion (first and last column of a chunk, the last column of the signal)."""
    from se_snmf_nat_amd import frontend as fe, train
    p = dict(tc.P_STOP, train_Exemplar=1, domain_DD=1, alpha_eta=0.4)
    Ts = [1, 2, 33, 70, 257, 600]
    sigs = [env.signal(tc.n_samples(T), 400 + T) for T in Ts]
    cols = {1: [1], 2: [1, 2], 33: [1, 2, 17, 33], 70: [1, 32, 33, 70], 257: [1, 2, 255, 256, 257], 600: [1, 256, 257, 258, 512, 513, 514, 600]}
    for i, T in enumerate(Ts):
        ix = np.array(cols[T])
        # a batch of two: the signal behind a longer or shorter one, so that its chunks are not the first of the launch
        other = sigs[(i + 3) % len(Ts)]
        oix = np.arange(1, len(ix) + 1) if Ts[(i + 3) % len(Ts)] >= len(ix) else None
        if oix is None:
            out = train.run_basis_train_signal_batch([sigs[i]], len(ix), p, sample_idx=[ix], ctx=gpu_ctx, precision=mode)[0]
        else:
            out = train.run_basis_train_signal_batch([other, sigs[i]], len(ix), p, sample_idx=[oix, ix], ctx=gpu_ctx, precision=mode)[1]
        X = fe.stft_features(sigs[i], p, ctx=gpu_ctx, precision=mode)
        V = fe.tf_dd(X, p, ctx=gpu_ctx, precision=mode)
        assert V.shape == (tc.F, T)
        want_d = unit_columns(V[:, ix - 1])
        want_m = unit_columns(fe.mel_features(V, p, ctx=gpu_ctx, precision=mode)[:, ix - 1])
        assert np.array_equal(out["B_DFT_sub"], want_d), (T, float(np.abs(out["B_DFT_sub"] - want_d).max()))
        assert np.array_equal(out["B_Mel_sub"], want_m), (T, float(np.abs(out["B_Mel_sub"] - want_m).max()))
        if T == 1 and mode == "fp64":  # (in double the first column is the input's, bit for bit)
            assert np.array_equal(out["B_DFT_sub"], unit_columns(X))


# ---- 5. one anchor to the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_problem_against_the_oracle(gpu_ctx, mode):
    """The waveform, settings and exemplar columns of tests/test_gpu_train_f64.py::test_basis_training_in_fp64 ("plain", also those
    of tests/test_frontend.py::test_basis_training_caller_end_to_end) as problem 0 of a batch of two."""
    import oracle.frontend_oracle as fo
    from se_snmf_nat_amd import train
    p = dict(TRAIN_BASE)
    s2 = samples()[2000:9000]
    idx2 = np.random.RandomState(6).choice(train.frontend.num_frames_host(s2.size, p), size=16, replace=False) + 1
    ref = fo.run_basis_train_signal(samples(), 16, p, IDX)
    out = train.run_basis_train_signal_batch([samples(), s2], 16, p, sample_idx=[IDX, idx2], ctx=gpu_ctx, precision=mode)[0]
    errs = {k: rel(out[k], ref[k]) for k in KEYS}
    print(f"{mode} batch problem 0 against the oracle: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k in KEYS:
        assert out[k].shape == ref[k].shape
        assert errs[k] < (REL_SOLVE if mode == "fp64" else REL_F32_END_TO_END), k
    assert out["B_DFT_sub"].shape == (513, 16) and out["B_Mel_sub"].shape == (64, 16)


# ---- 6. refusals through ctypes ----------------------------------------------------------------------------------------------
def test_c_entries_refuse_with_the_documented_status_and_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    sp, _win = fe._params(tc.TINY)
    T = 33
    L = tc.n_samples(T)

    def call(ty, *, F=tc.F, r=tc.R, n=2, L=(L, L), kind=0, null=None, null_entry=None, ctx=gpu_ctx._h, sp=sp, mel_M=tc.F_MEL, bad_idx=None,
             exemplar=0):
        sdt = np.float32 if ty == "f64" else np.float64
        q = _make_params(F, 1, r, 1.0, 3, 0.0, 1, True, kind, 0.1, None, None)
        m = max(n, 1)
        Tm = 40
        idx = [np.arange(r, dtype=np.int64) % T for _ in range(m)]
        if bad_idx is not None:
            idx[m - 1][r - 1] = bad_idx
        keep = dict(s=[env.signal(Lk, 1 + i).astype(sdt) for i, Lk in zip(range(m), L)], idx=idx,
                    H0=[np.full((r, Tm), 0.5, order="F") for _ in range(m)],
                    B_DFT=[np.ones((F, r), order="F") for _ in range(m)], A_DFT=[np.ones((r, Tm), order="F") for _ in range(m)],
                    B_Mel=[np.ones((max(mel_M, 1), r), order="F") for _ in range(m)], A_Mel=[np.ones((r, Tm), order="F") for _ in range(m)])
        ptr = {k: (C.c_void_p * m)(*[a.ctypes.data for a in v]) for k, v in keep.items()}
        if null_entry:
            ptr[null_entry][m - 1] = None
        a = {k: (None if null == k else ptr[k]) for k in keep}
        lens = np.array([v.size for v in keep["s"]], np.int64)
        seed = np.arange(1, m + 1, dtype=np.uint64)
        n_iter = np.zeros(2 * m, np.int32)
        mel = np.ones((mel_M, tc.F), dtype=sdt) if mel_M else None
        vp = lambda v: None if v is None else C.c_void_p(v.ctypes.data)  # noqa: E731
        return getattr(lib, f"snmf_run_basis_train_audio_batch_{ty}")(
            ctx, None if null == "p" else C.byref(q), None if null == "sp" else C.byref(sp), -1.0, None if null == "mel" else vp(mel),
            mel_M, n, a["s"], None if null == "lens" else vp(lens), a["idx"], exemplar, a["H0"], None if null == "seed" else vp(seed),
            a["B_DFT"], a["A_DFT"], a["B_Mel"], a["A_Mel"], vp(n_iter))

    before = {m: batch_of_all(gpu_ctx, m) for m in MODES}
    for ty in ("f64", "fp64"):
        assert call(ty) == 0
        assert call(ty, ctx=None) == 1
        for nm in ("p", "sp", "s", "lens", "idx", "B_DFT"):
            assert call(ty, null=nm) == 1, (ty, nm)
        for nm in ("s", "idx", "B_DFT", "B_Mel"):
            assert call(ty, null_entry=nm) == 1, (ty, nm)
        assert call(ty, null="mel") == 1 and call(ty, null="B_Mel") == 1  # mel and B_Mel go together
        assert call(ty, n=0) == 1
        assert call(ty, L=(L, tc.N + 1)) == 1  # a signal without a frame
        assert call(ty, null_entry="H0", null="seed") == 1 and call(ty, null="H0") == 0 and call(ty, null_entry="H0") == 0
        assert call(ty, null="H0", null_entry=None, exemplar=1) == 0 and call(ty, null_entry="H0", null="seed", exemplar=1) == 0
        assert call(ty, null="A_DFT") == 0 and call(ty, null_entry="A_Mel") == 0  # the activations are optional, whole or per problem
        assert call(ty, F=tc.F + 1) == 3                          # p->F is not the feature rows
        assert call(ty, bad_idx=T) == 3 and call(ty, bad_idx=-1) == 3 and call(ty, bad_idx=T - 1) == 0
        assert call(ty, kind=1) == 8 and call(ty, kind=2) == 8    # an r-vector and an r x n sparsity
        bad = fe._params(dict(tc.TINY, fftlength=96, framelength=40))[0]
        assert call(ty, sp=bad) == 8  # validate_stft: not a power of two
    assert call("f64", r=300) == 8 and b"limit of 200 components" in lib.snmf_last_error()  # the fp32 batch's envelope
    assert call("fp64", r=300) == 0  # (no such limit in the fp64 mode)
    for m in MODES:  # a valid batch afterwards still gives the earlier bits
        same_bits(run_batch(gpu_ctx, m), before[m])
