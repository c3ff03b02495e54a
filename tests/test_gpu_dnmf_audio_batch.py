"""GPU tests of the batched front-end and of run_basis_DNMF_batch / run_basis_DNMF_Mel_batch (snmf_stft_features_batch_*,
snmf_run_basis_dnmf_audio_batch_*): the front-end grouped over the signals of a batch, and the batched DNMF re-training fed by it.

The contracts are bit equalities with what is already shipped (np.array_equal throughout):
    features   every column is what stft_features (+ mel_features) give for that signal alone, in both precisions;
    fp64       problem k is run_basis_DNMF(x_k, d_k, B_k, p, precision="fp64") alone, with the same H0_k or the same seed;
    fp32       the batch is run_basis_dnmf_batch(precision="fp32") on the single front-end's features of
               y_k = float32(x_k) + float32(d_k), x_k and d_k, widened to double, and H0_k or philox_uniform(seed_k, r, T_k).
Waveforms and settings: tests/dnmf_audio_batch_cases.py.  Against the oracle the bounds are imported from the single tests:
AB_STFT of tests/test_gpu_frontend_envelope.py, REL_SOLVE of tests/test_gpu_train_f64.py and the 1e-4 of
tests/test_frontend.py::test_dnmf_callers_from_waveforms, on that test's own waveforms.
"""
import ctypes as C
import os

import numpy as np
import pytest

import dnmf_audio_batch_cases as ac
import frontend_envelope as env
from test_gpu_frontend_envelope import AB_STFT, judge
from test_gpu_train_f64 import REL_SOLVE

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = ["fp32", "fp64"]
REL_F32_WAVEFORMS = 1e-4  # tests/test_frontend.py::test_dnmf_callers_from_waveforms
SETTINGS = {"kl": ac.P_STOP, "ed": dict(ac.P_STOP, cf="ed"), "b05": dict(ac.P_STOP, cf="beta", beta=0.5)}
FEATURE_VARIANTS = {"plain": {}, "splice1": dict(Splice=1), "splice2": dict(Splice=2), "pow1": dict(pow=1), "pow07": dict(pow=0.7),
                    "preemph": dict(preemph=0.92), "splice1_pow07_preemph": dict(Splice=1, pow=0.7, preemph=0.92)}


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def single_features(ctx, s, p, mode, mel):
    """What the single front-end gives for one signal: stft_features, then mel_features on its output."""
    from se_snmf_nat_amd import frontend as fe
    V = fe.stft_features(s, p, ctx=ctx, precision=mode)
    if mel and V.shape[1]:
        V = fe.mel_features(V, p, ctx=ctx, precision=mode)
    elif mel:
        V = np.zeros((int(p["F_order"]) * (2 * int(p.get("Splice", 0)) + 1), 0), dtype=V.dtype, order="F")
    return V


def same_matrices(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (k, float(np.abs(g.astype(np.float64) - w).max()))


# ---- 1. the grouped front-end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(FEATURE_VARIANTS) + ["mel", "mel_splice1"])
@pytest.mark.parametrize("mode", MODES)
def test_features_are_the_single_front_ends_bit_for_bit(gpu_ctx, mode, variant):
    """T = 1, 2, 31, 32, 33, 70 and a signal without a frame; the list, the list reversed, and every signal as a batch of one.
    With Splice = 1 / 2 the signals of T <= Splice have every neighbour block outside the signal."""
    from se_snmf_nat_amd import frontend as fe
    mel = variant.startswith("mel")
    p = dict(ac.TINY, **(dict(Splice=1) if variant == "mel_splice1" else FEATURE_VARIANTS.get(variant, {})))
    sigs = list(ac.signals())
    want = [single_features(gpu_ctx, s, p, mode, mel) for s in sigs]
    rows = (2 * p["Splice"] + 1) * (p["F_order"] if mel else ac.F)
    assert [w.shape for w in want] == [(rows, T) for T in ac.TS + [0]]
    got = fe.stft_features_batch(sigs, p, mel=mel, precision=mode, ctx=gpu_ctx)
    same_matrices(got, want)
    same_matrices(fe.stft_features_batch(sigs[::-1], p, mel=mel, precision=mode, ctx=gpu_ctx)[::-1], want)
    for s, w in zip(sigs, want):
        same_matrices(fe.stft_features_batch([s], p, mel=mel, precision=mode, ctx=gpu_ctx), [w])
    assert all(np.isfinite(g).all() and (g > 0).all() for g in got)


@pytest.mark.parametrize("mode", MODES)
def test_features_at_fftlength_4096(gpu_ctx, mode):
    """The LDS edge: 64 KB static (float), 128 KB dynamic (double) per workgroup; T = 2 and T = 1 in one launch."""
    from se_snmf_nat_amd import frontend as fe
    p = dict(ac.TINY, fftlength=4096, framelength=2051, frameshift=513, DCbin=5, preemph=0.92, pow=0.5,
             win_STFT=env.window(2051))
    sigs = [env.signal(ac.n_samples(2, 513, 4096), 7), env.signal(ac.n_samples(1, 513, 4096) + 3, 8)]
    want = [single_features(gpu_ctx, s, p, mode, False) for s in sigs]
    assert [w.shape for w in want] == [(2049, 2), (2049, 1)]
    same_matrices(fe.stft_features_batch(sigs, p, precision=mode, ctx=gpu_ctx), want)


@pytest.mark.parametrize("name", ["n64_full_shift9_pow2", "n512_pow05_splice2_T5"])
@pytest.mark.parametrize("mode", MODES)
def test_features_against_the_oracle(gpu_ctx, mode, name):
    """A case of tests/frontend_envelope.py as one signal of a batch of three, judged against its fp64 oracle reference at the
    bounds of the single front-end's test: the chain of bit equalities above is anchored to the oracle, not only to the engine."""
    from se_snmf_nat_amd import frontend as fe
    p, s, ref = env.STFT_CASES[name], env.case_signal(name), env.case_reference(name)
    others = [env.signal(env.n_samples(p, 3), 91), env.signal(env.n_samples(p, 1), 92)]
    got = fe.stft_features_batch([others[0], s, others[1]], p, precision=mode, ctx=gpu_ctx)
    assert [g.shape[1] for g in got] == [3, p["T"], 1]
    judge(f"stft batch {mode} {name}", got[1], ref, env.colmax(ref, p), AB_STFT["f32" if mode == "fp32" else "fp64"])


# ---- 2. / 3. the batched loop ------------------------------------------------------------------------------------------------
def run_batch(ctx, mode, p, order=None, B=None, h0="given", mel=False):
    """-> [(B_hat, A_hat, [n1, n2, n3])] of one call on the problems `order` of the cases (default: all, in order)."""
    from se_snmf_nat_amd import train
    order = list(range(len(ac.TS))) if order is None else order
    bases = ac.bases(p["F_order"] if mel else ac.F)
    info = {}
    fn = train.run_basis_DNMF_Mel_batch if mel else train.run_basis_DNMF_batch
    out = fn([ac.waves()[k][0] for k in order], [ac.waves()[k][1] for k in order], [bases[k] for k in order] if B is None else B, p,
             ctx=ctx, h0=[ac.given_h0()[k] for k in order] if h0 == "given" else h0, precision=mode, info=info)
    assert info["T"] == [ac.TS[k] for k in order]
    return [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]


def same_bits(res, ref):
    assert len(res) == len(ref)
    for k, ((b, a, n), (br, ar, nr)) in enumerate(zip(res, ref)):
        assert list(n) == list(nr), (k, n, nr)
        assert b.dtype == br.dtype == np.float64 and b.shape == br.shape and a.shape == ar.shape
        assert np.array_equal(b, br), (k, "B_hat", float(np.abs(b - br).max()))
        assert np.array_equal(a, ar), (k, "A_hat", float(np.abs(a - ar).max()))


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        for b, a, _ in _cache[key]:
            b.setflags(write=False)
            a.setflags(write=False)
    return _cache[key]


def alone_fp64(ctx, p, h0="given", mel=False):
    """run_basis_DNMF(..., precision="fp64") per problem: the fp64 contract's reference."""
    from se_snmf_nat_amd import train

    def make():
        out = []
        bases = ac.bases(p["F_order"] if mel else ac.F)
        for k, (x, d) in enumerate(ac.waves()):
            info = {}
            q = p if h0 == "given" else dict(p, random_seed=p["random_seed"] + k)
            b, a = train._run_basis_dnmf_audio(x, d, bases[k], q, ctx=ctx, mel=mel, h0=ac.given_h0()[k] if h0 == "given" else "device",
                                               want_a=True, precision="fp64", info=info)
            out.append((b, a, info["n_iter"]))
        return out
    return cached(("alone", p["cf"], h0, mel), make)


def matrix_batch_fp32(ctx, p, h0="given", mel=False):
    """run_basis_dnmf_batch(precision="fp32") on the single front-end's fp32 features: the fp32 contract's reference."""
    from se_snmf_nat_amd import run_basis_dnmf_batch
    from se_snmf_nat_amd.api import philox_uniform

    def make():
        r = ac.R_X + ac.R_D
        Ys, Xs, Ds, H0s = [], [], [], []
        for k, (x, d) in enumerate(ac.waves()):
            n = min(len(x), len(d))
            xf, df = x[:n].astype(np.float32), d[:n].astype(np.float32)
            for lst, s in ((Ys, xf + df), (Xs, xf), (Ds, df)):  # (the sum of two float32 arrays is taken in float32)
                lst.append(single_features(ctx, s, p, "fp32", mel).astype(np.float64))
            H0s.append(ac.given_h0()[k] if h0 == "given" else philox_uniform(p["random_seed"] + k, r, ac.TS[k]).astype(np.float64))
        info = {}
        out = run_basis_dnmf_batch(Ys, Xs, Ds, list(ac.bases(p["F_order"] if mel else ac.F)), ac.R_X, ac.R_D, p, ctx=ctx, h0=H0s,
                                   precision="fp32", info=info)
        return [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]
    return cached(("matrix", p["cf"], h0, mel), make)


def reference(ctx, mode, p, **kw):
    return alone_fp64(ctx, p, **kw) if mode == "fp64" else matrix_batch_fp32(ctx, p, **kw)


def batch_of_all(ctx, mode, setting="kl"):
    return cached(("batch", mode, setting), lambda: run_batch(ctx, mode, SETTINGS[setting]))


@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_the_shipped_paths_bit_for_bit(gpu_ctx, mode):
    res = batch_of_all(gpu_ctx, mode)
    print(f"{mode}: n_iter per problem {[n for _, _, n in res]}")
    same_bits(res, reference(gpu_ctx, mode, ac.P_STOP))
    n1 = [n[0] for _, _, n in res]
    assert max(n1) == ac.P_STOP["max_iter"] and len(set(n1)) > 2, n1  # one problem runs to max_iter, the others stop on their own
    for b, a, _ in res:
        assert np.isfinite(b).all() and np.isfinite(a).all()


@pytest.mark.parametrize("mode", MODES)
def test_h0_drawn_on_the_device(gpu_ctx, mode):
    """fp64: the single call's own device draw with the seed random_seed + k; fp32: philox_uniform through the matrix form."""
    res = run_batch(gpu_ctx, mode, ac.P_STOP, h0="device")
    same_bits(res, reference(gpu_ctx, mode, ac.P_STOP, h0="device"))
    assert not np.array_equal(res[5][1], batch_of_all(gpu_ctx, mode)[5][1])  # (another start, another A_hat)


@pytest.mark.parametrize("mode", MODES)
def test_a_problem_does_not_depend_on_the_batch_around_it(gpu_ctx, mode):
    res = batch_of_all(gpu_ctx, mode)
    order = list(range(len(ac.TS)))[::-1]
    same_bits(run_batch(gpu_ctx, mode, ac.P_STOP, order=order)[::-1], res)
    for k in (0, 2, 5):  # one frame, a partial tile, several tiles
        same_bits(run_batch(gpu_ctx, mode, ac.P_STOP, order=[k]), [res[k]])


@pytest.mark.parametrize("mode", MODES)
def test_one_basis_equals_a_list_of_equal_bases(gpu_ctx, mode):
    B0 = ac.bases()[0]
    one = run_batch(gpu_ctx, mode, ac.P_STOP, B=B0)
    same_bits(one, run_batch(gpu_ctx, mode, ac.P_STOP, B=[B0.copy() for _ in ac.TS]))
    assert not np.array_equal(one[1][0], batch_of_all(gpu_ctx, mode)[1][0])  # (and B is read: another basis, another result)


@pytest.mark.parametrize("setting", ["ed", "b05"])
@pytest.mark.parametrize("mode", MODES)
def test_two_image_modes_equal_the_shipped_paths_bit_for_bit(gpu_ctx, mode, setting):
    same_bits(batch_of_all(gpu_ctx, mode, setting), reference(gpu_ctx, mode, SETTINGS[setting]))


@pytest.mark.parametrize("mode", MODES)
def test_mel_twin_equals_the_shipped_paths_bit_for_bit(gpu_ctx, mode):
    same_bits(run_batch(gpu_ctx, mode, ac.P_STOP, mel=True), reference(gpu_ctx, mode, ac.P_STOP, mel=True))


def test_every_stage_of_the_grouped_front_end_in_one_fp64_call(gpu_ctx):
    """Pre-emphasis, pow = 0.7, Splice = 1 and the Mel projection together, H0 drawn on the device: STFT -> splice -> Mel."""
    from se_snmf_nat_amd import train
    p = dict(ac.P_STOP, Splice=1, pow=0.7, preemph=0.92)
    B = np.random.RandomState(4).rand(3 * p["F_order"], ac.R_X + ac.R_D) + 0.05
    ks = [4, 1]
    info = {}
    out = train.run_basis_DNMF_Mel_batch([ac.waves()[k][0] for k in ks], [ac.waves()[k][1] for k in ks], B, p, ctx=gpu_ctx, h0="device",
                                         precision="fp64", info=info)
    for i, k in enumerate(ks):
        one = {}
        b, a = train._run_basis_dnmf_audio(*ac.waves()[k], B, dict(p, random_seed=p["random_seed"] + i), ctx=gpu_ctx, mel=True, h0="device",
                                           want_a=True, precision="fp64", info=one)
        same_bits([(out[i][0], out[i][1], info["n_iter"][i])], [(b, a, one["n_iter"])])


# ---- 4. one anchor to the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_problem_against_the_oracle_loop(gpu_ctx, mode):
    """The waveforms, settings and bounds of the single callers' tests (tests/test_frontend.py and tests/test_gpu_train_f64.py:
    test_dnmf_callers_from_waveforms*) as problem 0 of a batch of two; h0="host" gives problem 0 the oracle's own draw."""
    import oracle.frontend_oracle as fo
    from se_snmf_nat_amd import train
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    x, d = s[:9000], s[9000:19000][::-1].copy()
    p = dict(fo.default_params(), cf="kl", sparsity=5, max_iter=12, conv_eps=1e-3, cost_check=1, random_seed=1, R_x=10, R_d=12)
    B = np.random.RandomState(5).rand(513, 22) + 0.05
    ref = fo.run_basis_DNMF(x, d, B, p)
    out = train.run_basis_DNMF_batch([x, s[2000:6000]], [d, s[12000:17000]], B, p, ctx=gpu_ctx, precision=mode)
    dev = out[0][0]
    print(f"{mode} batch problem 0 against the oracle: relB = {rel(dev, ref):.2e}")
    assert dev.shape == ref.shape == (513, 22)
    assert rel(dev, ref) < (REL_SOLVE if mode == "fp64" else REL_F32_WAVEFORMS)


# ---- 5. refusals through ctypes ----------------------------------------------------------------------------------------------
def test_c_entries_refuse_with_the_documented_status_and_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    sp, _win = fe._params(ac.TINY)
    T = 33
    L = ac.n_samples(T)

    def call(ty, *, F=ac.F, Rx=ac.R_X, Rd=ac.R_D, r=None, n=2, L=(L, L), kind=0, null=None, null_entry=None, ctx=gpu_ctx._h, sp=sp,
             mel_M=None):
        sdt = np.float32 if ty == "f64" else np.float64
        r = Rx + Rd if r is None else r
        q = _make_params(F, 1, r, 1.0, 3, 0.0, 1, True, kind, 0.1, None, None)
        m = max(n, 1)
        rr, Tm = max(r, 1), 40
        keep = dict(x=[env.signal(Lk, 1 + i).astype(sdt) for i, Lk in zip(range(m), L)],
                    d=[env.signal(Lk + 3, 9 + i).astype(sdt) for i, Lk in zip(range(m), L)],
                    B=[np.ones((F, rr), order="F") for _ in range(m)], H0=[np.full((rr, Tm), 0.5, order="F") for _ in range(m)],
                    B_hat=[np.ones((F, rr), order="F") for _ in range(m)], A_hat=[np.ones((rr, Tm), order="F") for _ in range(m)])
        ptr = {k: (C.c_void_p * m)(*[a.ctypes.data for a in v]) for k, v in keep.items()}
        if null_entry:
            ptr[null_entry][m - 1] = None
        a = {k: (None if null == k else ptr[k]) for k in keep}
        n_x = np.array([v.size for v in keep["x"]], np.int64)
        n_d = np.array([v.size for v in keep["d"]], np.int64)
        seed = np.arange(1, m + 1, dtype=np.uint64)
        n_iter = np.zeros(3 * m, np.int32)
        mel = np.ones((mel_M, ac.F), dtype=sdt) if mel_M else None
        vp = lambda v: None if v is None else C.c_void_p(v.ctypes.data)  # noqa: E731
        return getattr(lib, f"snmf_run_basis_dnmf_audio_batch_{ty}")(
            ctx, None if null == "p" else C.byref(q), None if null == "sp" else C.byref(sp), Rx, Rd, n, a["x"],
            None if null == "n_x" else vp(n_x), a["d"], None if null == "n_d" else vp(n_d), vp(mel), mel_M or 0, a["B"], a["H0"],
            None if null == "seed" else vp(seed), a["B_hat"], a["A_hat"], vp(n_iter))

    before = {m: batch_of_all(gpu_ctx, m) for m in MODES}
    for ty in ("f64", "fp64"):
        assert call(ty) == 0
        assert call(ty, ctx=None) == 1
        for nm in ("p", "sp", "x", "n_x", "d", "n_d", "B", "B_hat"):
            assert call(ty, null=nm) == 1, (ty, nm)
        for nm in ("x", "d", "B", "B_hat"):
            assert call(ty, null_entry=nm) == 1, (ty, nm)
        assert call(ty, n=0) == 1
        assert call(ty, L=(L, ac.N + 1)) == 1  # a problem shorter than one analysis frame
        assert call(ty, null_entry="H0", null="seed") == 1 and call(ty, null="H0") == 0 and call(ty, null_entry="H0") == 0
        assert call(ty, null="A_hat") == 0 and call(ty, null_entry="A_hat") == 0  # A_hat is optional, whole or per problem
        assert call(ty, F=ac.F + 1) == 3                 # p->F is not the feature rows
        assert call(ty, F=ac.F, mel_M=8) == 3 and call(ty, F=8, mel_M=8) == 0
        assert call(ty, Rx=0, r=ac.R_D) == 3 and call(ty, Rd=0, r=ac.R_X) == 3 and call(ty, r=ac.R_X + ac.R_D + 1) == 3
        assert call(ty, kind=1) == 3 and call(ty, kind=2) == 3  # an r-vector and an r x n sparsity
        bad = fe._params(dict(ac.TINY, fftlength=96, framelength=40))[0]
        assert call(ty, sp=bad) == 8  # validate_stft: not a power of two
    assert call("f64", Rx=150, Rd=150) == 8 and b"limit of 200 components" in lib.snmf_last_error()  # the fp32 batch's envelope
    assert call("fp64", Rx=150, Rd=150) == 0  # (no such limit in the fp64 mode)
    for ty in ("f32", "fp64"):  # the feature entries
        fn = getattr(lib, f"snmf_stft_features_batch_{ty}")
        dt = np.float32 if ty == "f32" else np.float64
        s = env.signal(L, 3).astype(dt)
        out = np.zeros((ac.F, T), dtype=dt, order="F")
        ps, po = (C.c_void_p * 1)(s.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
        ln, nf = np.array([L], np.int64), np.zeros(1, np.int32)
        vp = lambda v: C.c_void_p(v.ctypes.data)  # noqa: E731
        assert fn(gpu_ctx._h, C.byref(sp), 1, None, vp(ln), None, 0, po, vp(nf)) == 1
        assert fn(gpu_ctx._h, C.byref(sp), 1, ps, None, None, 0, po, vp(nf)) == 1
        assert fn(gpu_ctx._h, C.byref(sp), 1, ps, vp(ln), None, 0, None, vp(nf)) == 1
        assert fn(gpu_ctx._h, C.byref(sp), 0, ps, vp(ln), None, 0, po, vp(nf)) == 1
        assert fn(gpu_ctx._h, None, 1, ps, vp(ln), None, 0, po, vp(nf)) == 1
        mel = np.ones((8, ac.F), dtype=dt)
        assert fn(gpu_ctx._h, C.byref(sp), 1, ps, vp(ln), vp(mel), 0, po, vp(nf)) == 1
        assert fn(gpu_ctx._h, C.byref(sp), 1, ps, vp(ln), None, 0, po, None) == 0 and (out > 0).all()
    for m in MODES:  # a valid batch afterwards still gives the earlier bits
        same_bits(run_batch(gpu_ctx, m, ac.P_STOP), before[m])
