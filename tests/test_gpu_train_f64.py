"""The fp64 mode of the front-end, the DNMF loop and the basis-training caller (precision="fp64" -> the snmf_*_fp64 entries of
include/snmf.h: double from the samples to the dictionaries, resident in HBM) against the fp64 oracle.

Bounds.  None is read off the device: each is the ORACLE's own response to a relative perturbation eps = 1e-12 of its inputs
(samples and B multiplied by 1 + eps N(0,1); scripts/train_f64_sensitivity.py -> profiles/train_f64_sensitivity.md; the
response is linear in eps).  The figures the bounds were set from:
    B_hat of run_basis_DNMF 4.1e-12, of run_basis_DNMF_Mel 3.8e-12; training outputs (plain, domain_DD, early stop) <= 1.2e-12
    STFT features: max error over the column maximum <= 5.4e-12 (pow=1, preemph=0.92), Frobenius-relative 2.6e-12
    Mel features: per element relative <= 9.6e-11
    TF_DD (its input perturbed): per element relative 2.7e-12 .. 4.6e-12, over the row maximum 1.2e-12 .. 3.9e-12 on the four
    shapes below; the smallest of each is taken
So
    REL_SOLVE = 1e-11    relative Frobenius error of every solve output (the bound of tests/test_gpu_solve_f64.py)
    features             |err| <= a |ref| + b colmax, (a, b) = (2.6e-12, 5.4e-12) STFT, (9.6e-11, 5.4e-12) Mel,
                         (2.7e-12, 1.2e-12) TF_DD with the row maximum as its scale
The fp32 mode sits near 1e-6 on the same cases: a fall-back to it cannot pass.

Shapes of the bit-for-bit cases: 33 x 2100 crosses one split of the R * H' contraction (L = 2048, kS64ChunkK), its ranks
3 / 5 / 8 are no tile multiples and T is no multiple of 64; 64 x 70 is Euclidean with an early stop; 17 x 15 has rank 1 + 1.

Measured on an MI355X (every test prints its own figures before it asserts):
    STFT features (4 cases)   error <= 8.8e-16 of the column maximum = 1.1e-4 of the bound; relative Frobenius <= 2.7e-16
    Mel features              <= 1.7e-6 of the bound, relative Frobenius 2.4e-18
    TF_DD (4 shapes)          error <= 7.8e-16 of the row maximum = 2.4e-4 of the bound; first column equal in all
    DNMF loop (4 shapes)      relB <= 9.7e-15  relA <= 2.7e-15  n_iter equal in all  | ||column|| - 1 | <= 2.2e-16
                              resident == three calls bit for bit (B_hat, A_hat, n_iter) on all three shapes
    from waveforms            relB = 1.3e-15 (run_basis_DNMF), 7.1e-16 (run_basis_DNMF_Mel); the fp32 mode: 1.4e-6, 3.8e-7
    basis training (4 cases)  all outputs <= 1.1e-15
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import frontend_oracle as fo
from oracle.sparse_nmf_oracle import run_basis_dnmf_solves, sparse_nmf as oracle_nmf, synth_problem

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL_SOLVE = 1e-11
AB_STFT = (2.6e-12, 5.4e-12)
AB_MEL = (9.6e-11, 5.4e-12)
AB_TFDD = (2.7e-12, 1.2e-12)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def judge_features(name, got, ref, scale, ab):
    """|err| <= a |ref| + b scale, element-wise; prints the error in units of the bound first."""
    a, b = ab
    assert got.dtype == np.float64 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    err = np.abs(got - ref)
    bound = a * np.abs(ref) + b * scale
    print(f"fp64 front-end {name}: max err/bound = {float((err / bound).max()):.2e}  max err/scale = {float((err / scale).max()):.2e}  "
          f"relFro = {rel(got, ref):.2e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), float((err / bound).max())


@functools.lru_cache(maxsize=None)
def samples():
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    s.setflags(write=False)
    return s


def stft_colmax(ref, p):
    K = p["fftlength"] // 2 + 1
    cm = ref.reshape(-1, K, ref.shape[1]).max(axis=(0, 1)) if p.get("Splice", 0) else ref.max(0)
    return np.maximum(cm, ref.max() * 1e-3)[None, :]  # (as tests/test_frontend.py: spliced neighbours may dominate a column)


TINY = dict(fftlength=64, framelength=40, frameshift=10, DCbin=1, win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(40) / 40)))
STFT_CASES = {"shipped": {}, "splice1": dict(Splice=1), "pow1_preemph": dict(pow=1, preemph=0.92), "tiny_64_40_10": TINY}


# ---- 1. the front-end against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STFT_CASES))
def test_stft_features_in_fp64(gpu_ctx, name):
    from se_snmf_nat_amd import frontend as fe
    p = dict(fo.default_params(), **STFT_CASES[name])
    s = samples()[:4000] if name.startswith("tiny") else samples()
    ref = fo.dft_features(s, p)
    got = fe.stft_features(s, p, ctx=gpu_ctx, precision="fp64")
    assert fe.num_frames(len(s), p) == ref.shape[1] > 1
    judge_features(name, got, ref, stft_colmax(ref, p), AB_STFT)
    assert rel(fe.stft_features(s, p, ctx=gpu_ctx).astype(np.float64), ref) > 1e-9  # the two modes are two computations


def test_mel_features_in_fp64(gpu_ctx):
    from se_snmf_nat_amd import frontend as fe
    p = fo.default_params()
    V = fo.dft_features(samples(), p)
    ref = fo.mel_features(V, p)
    judge_features("mel", fe.mel_features(V, p, ctx=gpu_ctx, precision="fp64"), ref, ref.max(0)[None, :], AB_MEL)
    p1 = dict(p, Splice=1)
    V1 = fo.dft_features(samples(), p1)
    ref1 = fo.mel_features(V1, p1)
    judge_features("mel, Splice=1", fe.mel_features(V1, p1, ctx=gpu_ctx, precision="fp64"), ref1, ref1.max(0)[None, :], AB_MEL)


@pytest.mark.parametrize("shape,alpha", [((513, 3000), 0.4), ((1, 1000), 0.7), ((700, 1), 0.4), ((64, 257), 0.95)])
def test_tf_dd_in_fp64(gpu_ctx, shape, alpha):
    """Chunk boundaries (256 frames a chunk), one row, one frame; the first column is the input's, bit for bit."""
    from se_snmf_nat_amd import frontend as fe
    rs = np.random.RandomState(shape[0] + shape[1])
    X = rs.gamma(0.5, 1.0, shape) * 10.0 ** rs.uniform(-3, 3, (shape[0], 1))
    ref = fo.tf_dd(X, {"alpha_eta": alpha})
    got = fe.tf_dd(X, {"alpha_eta": alpha}, ctx=gpu_ctx, precision="fp64")
    judge_features(f"tf_dd {shape}", got, ref, np.abs(ref).max(axis=1, keepdims=True), AB_TFDD)
    np.testing.assert_array_equal(got[:, 0], X[:, 0])


# ---- 2. / 3. the DNMF loop -----------------------------------------------------------------------------------------------
KL = dict(cf="kl", sparsity=5, cost_check=1, random_seed=1)
DNMF_CASES = {
    "kl_33x2100_r3_5": ((33, 2100), 3, 5, dict(KL, max_iter=12, conv_eps=0)),
    "ed_64x70_r10_12_stop": ((64, 70), 10, 12, dict(cf="ed", sparsity=2, cost_check=1, random_seed=1, max_iter=100, conv_eps=1e-3)),
    "kl_17x15_r1_1": ((17, 15), 1, 1, dict(KL, max_iter=10, conv_eps=0)),
    "kl_513x64_r20_20": ((513, 64), 20, 20, dict(KL, max_iter=15, conv_eps=0)),
}
BITWISE = ["kl_33x2100_r3_5", "ed_64x70_r10_12_stop", "kl_17x15_r1_1"]


@functools.lru_cache(maxsize=None)
def dnmf_problem(name):
    (F, T), R_x, R_d, p = DNMF_CASES[name]
    X = synth_problem(F, T, R_x + 2, seed_data=11)[0]
    D = synth_problem(F, T, R_d + 2, seed_data=12)[0]
    Y = X + D
    B = np.random.RandomState(5).rand(F, R_x + R_d) + 0.05
    for a in (Y, X, D, B):
        a.setflags(write=False)
    return Y, X, D, B


@functools.lru_cache(maxsize=None)
def dnmf_oracle(name):
    """run_basis_dnmf_solves, and the same three calls restated for their iteration counts (which it does not return)."""
    _, R_x, R_d, p = DNMF_CASES[name]
    Y, X, D, B = dnmf_problem(name)
    B_hat, A_hat = run_basis_dnmf_solves(Y, X, D, B, R_x, R_d, p)
    r = R_x + R_d
    _, A, o1 = oracle_nmf(Y, dict(p, w_update_ind=np.zeros(r, bool), h_update_ind=np.ones(r, bool), init_w=B))
    bx, _, o2 = oracle_nmf(X, dict(p, w_update_ind=np.ones(R_x, bool), h_update_ind=np.zeros(R_x, bool), init_w=B[:, :R_x], init_h=A[:R_x]))
    bd, _, o3 = oracle_nmf(D, dict(p, w_update_ind=np.ones(R_d, bool), h_update_ind=np.zeros(R_d, bool), init_w=B[:, R_x:], init_h=A[R_x:]))
    assert np.array_equal(np.concatenate([bx, bd], axis=1), B_hat) and np.array_equal(A, A_hat)  # the restatement IS the oracle's loop
    return B_hat, A_hat, [o1["n_iter"], o2["n_iter"], o3["n_iter"]]


def dnmf_device(name, ctx, **kw):
    from se_snmf_nat_amd import run_basis_dnmf
    _, R_x, R_d, p = DNMF_CASES[name]
    Y, X, D, B = dnmf_problem(name)
    info = {}
    B_hat, A_hat = run_basis_dnmf(Y, X, D, B, R_x, R_d, p, ctx=ctx, precision="fp64", info=info, **kw)
    return B_hat, A_hat, info["n_iter"]


@pytest.mark.parametrize("name", BITWISE)
def test_resident_dnmf_equals_three_calls_bit_for_bit(gpu_ctx, name):
    b1, a1, n1 = dnmf_device(name, gpu_ctx)
    b3, a3, n3 = dnmf_device(name, gpu_ctx, resident=False)
    print(f"fp64 DNMF {name}: n_iter resident {n1}, three calls {n3}")
    assert b1.dtype == a1.dtype == np.float64
    assert n1 == n3
    assert b1.tobytes() == b3.tobytes() and a1.tobytes() == a3.tobytes()


@pytest.mark.parametrize("name", sorted(DNMF_CASES))
def test_dnmf_loop_against_oracle(gpu_ctx, name):
    b, a, n = dnmf_device(name, gpu_ctx)
    br, ar, nr = dnmf_oracle(name)
    nrm = np.sqrt((b ** 2).sum(0))
    print(f"fp64 DNMF {name}: n_iter {n} (oracle {nr}) relB={rel(b, br):.2e} relA={rel(a, ar):.2e} max|norm-1|={float(np.abs(nrm - 1).max()):.1e}")
    assert n == nr
    assert rel(b, br) < REL_SOLVE and rel(a, ar) < REL_SOLVE
    np.testing.assert_allclose(nrm, 1.0, rtol=1e-14)
    if name == "ed_64x70_r10_12_stop":
        assert min(nr) < 100  # (the early stop is exercised)


@pytest.mark.parametrize("mel", [False, True], ids=["run_basis_DNMF", "run_basis_DNMF_Mel"])
def test_dnmf_callers_from_waveforms_in_fp64(gpu_ctx, mel):
    """The waveforms of tests/test_frontend.py::test_dnmf_callers_from_waveforms: unequal lengths, y = x + d in double."""
    from se_snmf_nat_amd import train
    s = samples()
    x, d = s[:9000], s[9000:19000][::-1].copy()
    p = dict(fo.default_params(), cf="kl", sparsity=5, max_iter=12, conv_eps=1e-3, cost_check=1, random_seed=1, R_x=10, R_d=12)
    F = 64 if mel else 513
    B = np.random.RandomState(5).rand(F, 22) + 0.05
    ref = fo.run_basis_DNMF(x, d, B, p, mel=mel)
    fn = train.run_basis_DNMF_Mel if mel else train.run_basis_DNMF
    dev = fn(x, d, B, p, ctx=gpu_ctx, precision="fp64")
    nrm = np.sqrt((dev ** 2).sum(0))
    print(f"fp64 {fn.__name__}: relB={rel(dev, ref):.2e} max|norm-1|={float(np.abs(nrm - 1).max()):.1e}; "
          f"fp32 mode relB={rel(fn(x, d, B, p, ctx=gpu_ctx), ref):.2e}")
    assert dev.dtype == np.float64 and dev.shape == ref.shape == (F, 22)
    assert rel(dev, ref) < REL_SOLVE
    np.testing.assert_allclose(nrm, 1.0, rtol=1e-14)


# ---- 4. basis training ---------------------------------------------------------------------------------------------------
TRAIN_BASE = dict(fo.default_params(), cf="kl", sparsity=5, max_iter=20, conv_eps=0, cost_check=1, cluster_buff=1, train_Exemplar=0)
TRAIN_CASES = {"plain": {}, "domain_dd": dict(domain_DD=1, alpha_eta=0.4), "early_stop": dict(conv_eps=1e-3, max_iter=40),
               "exemplar": dict(train_Exemplar=1)}
IDX = np.random.RandomState(5).choice(114, size=16, replace=False) + 1


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_basis_training_in_fp64(gpu_ctx, name):
    from se_snmf_nat_amd import train
    p = dict(TRAIN_BASE, **TRAIN_CASES[name])
    out = train.run_basis_train_signal(samples(), 16, p, sample_idx=IDX, ctx=gpu_ctx, precision="fp64")
    if name == "exemplar":  # run_basis_train.m:84, :95-96: the exemplar columns are the dictionaries, the activations the scalar 0
        V = fo.dft_features(samples(), p)
        ref = {"B_DFT_sub": V[:, IDX - 1], "B_Mel_sub": fo.mel_features(V, p)[:, IDX - 1]}
        ref = {k: v / np.sqrt((v ** 2).sum(0)) + 1e-9 for k, v in ref.items()}
        assert np.isscalar(out["A_DFT_sub"]) and out["A_DFT_sub"] == 0 and out["A_Mel_sub"] == 0
    else:
        ref = fo.run_basis_train_signal(samples(), 16, p, IDX)
    errs = {k: rel(out[k], ref[k]) for k in ref}
    print(f"fp64 training {name}: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k in ref:
        assert out[k].dtype == np.float64 and out[k].shape == ref[k].shape
        assert errs[k] < REL_SOLVE, k
    assert out["B_DFT_sub"].shape == (513, 16) and out["B_Mel_sub"].shape == (64, 16)


def test_basis_training_with_kmeans_rank_reduction_in_fp64(gpu_ctx):
    """cluster_buff = 2: every kept atom is one of the trained ones and the nearest to its cluster's centroid.  No index
    equality: a two-member cluster has both members equidistant from their median, in the oracle too."""
    from oracle import kmeans_oracle
    from se_snmf_nat_amd import train
    base = dict(TRAIN_BASE, max_iter=15)
    full = train.run_basis_train_signal(samples(), 16, dict(base, cluster_buff=1), sample_idx=IDX, ctx=gpu_ctx, precision="fp64")
    red = train.run_basis_train_signal(samples(), 8, dict(base, cluster_buff=2, kmeans_seed=3), sample_idx=IDX, ctx=gpu_ctx, precision="fp64")
    _, _, D = kmeans_oracle.kmeans_cityblock(full["B_Mel_sub"].T, 8, seed=3)
    assert red["B_DFT_sub"].shape == (513, 8) and red["B_Mel_sub"].shape == (64, 8) and red["A_DFT_sub"].shape[0] == 8
    keep = np.array([int(np.flatnonzero((full["B_Mel_sub"] == red["B_Mel_sub"][:, [j]]).all(0))[0]) for j in range(8)])
    np.testing.assert_allclose(D[keep, np.arange(8)], D.min(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(red["B_DFT_sub"], full["B_DFT_sub"][:, keep])
    np.testing.assert_array_equal(red["A_DFT_sub"], full["A_DFT_sub"][keep])
    np.testing.assert_array_equal(red["A_Mel_sub"], full["A_Mel_sub"][keep])


# ---- 5. the device's own draw ---------------------------------------------------------------------------------------------
def test_device_h0_is_the_philox_stream_as_doubles(gpu_ctx):
    from se_snmf_nat_amd.api import philox_uniform
    name = "kl_33x2100_r3_5"
    _, R_x, R_d, p = DNMF_CASES[name]
    h0 = philox_uniform(p["random_seed"], R_x + R_d, 2100).astype(np.float64)
    b1, a1, n1 = dnmf_device(name, gpu_ctx, h0="device")
    b2, a2, n2 = dnmf_device(name, gpu_ctx, h0=h0)
    b3, a3, n3 = dnmf_device(name, gpu_ctx, h0="device", resident=False)
    assert n1 == n2 == n3
    assert b1.tobytes() == b2.tobytes() == b3.tobytes() and a1.tobytes() == a2.tobytes() == a3.tobytes()
    assert b1.tobytes() != dnmf_device(name, gpu_ctx)[0].tobytes()  # (and it is another start than the host's draw)


# ---- 6. reproducibility ---------------------------------------------------------------------------------------------------
def test_two_fp64_runs_give_the_same_bits(gpu_ctx):
    from se_snmf_nat_amd import frontend as fe, train
    for name in ("kl_33x2100_r3_5", "ed_64x70_r10_12_stop"):
        r1, r2 = dnmf_device(name, gpu_ctx), dnmf_device(name, gpu_ctx)
        assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes() and r1[2] == r2[2]
    p = dict(TRAIN_BASE, domain_DD=1, alpha_eta=0.4)
    o1 = train.run_basis_train_signal(samples(), 16, p, sample_idx=IDX, ctx=gpu_ctx, precision="fp64", h0="device")
    o2 = train.run_basis_train_signal(samples(), 16, p, sample_idx=IDX, ctx=gpu_ctx, precision="fp64", h0="device")
    for k in o1:
        assert o1[k].tobytes() == o2[k].tobytes(), k
    q = dict(fo.default_params(), Splice=1)
    assert fe.stft_features(samples(), q, ctx=gpu_ctx, precision="fp64").tobytes() == fe.stft_features(samples(), q, ctx=gpu_ctx, precision="fp64").tobytes()


# ---- 7. the default path ----------------------------------------------------------------------------------------------------
def test_default_precision_is_the_fp32_path_bit_for_bit(gpu_ctx):
    """Without the keyword and with precision="fp32": the same bits, also around fp64 calls on the same context."""
    from se_snmf_nat_amd import frontend as fe, run_basis_dnmf, train
    s, p = samples(), fo.default_params()
    _, R_x, R_d, pd = DNMF_CASES["kl_513x64_r20_20"]
    Y, X, D, B = dnmf_problem("kl_513x64_r20_20")
    x, d = s[:9000], s[9000:19000][::-1].copy()
    pw = dict(p, cf="kl", sparsity=5, max_iter=6, conv_eps=0, cost_check=1, random_seed=1, R_x=10, R_d=12)
    Bw = np.random.RandomState(5).rand(513, 22) + 0.05
    Xdd = np.random.RandomState(0).gamma(0.5, 1.0, (64, 300))

    def all_calls(**kw):
        V = fe.stft_features(s, p, ctx=gpu_ctx, **kw)
        tr = train.run_basis_train_signal(s, 16, dict(TRAIN_BASE, max_iter=6), sample_idx=IDX, ctx=gpu_ctx, **kw)
        return [V, fe.mel_features(V, p, ctx=gpu_ctx, **kw), fe.tf_dd(Xdd, {"alpha_eta": 0.4}, ctx=gpu_ctx, **kw),
                *run_basis_dnmf(Y, X, D, B, R_x, R_d, pd, ctx=gpu_ctx, **kw), train.run_basis_DNMF(x, d, Bw, pw, ctx=gpu_ctx, **kw),
                tr["B_DFT_sub"], tr["A_Mel_sub"]]

    first = all_calls()
    dnmf_device("kl_17x15_r1_1", gpu_ctx)
    fe.tf_dd(Xdd, {"alpha_eta": 0.4}, ctx=gpu_ctx, precision="fp64")
    second = all_calls(precision="fp32")
    assert first[0].dtype == np.float32 and first[2].dtype == np.float32
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_a_refused_fp64_call_leaves_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    name = "kl_17x15_r1_1"
    before = dnmf_device(name, gpu_ctx)
    Y, X, D, B = (np.asfortranarray(a) for a in dnmf_problem(name))
    out = np.empty((17, 2), order="F")
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def dnmf(q):
        return lib.snmf_run_basis_dnmf_fp64(gpu_ctx._h, C.byref(q), 1, 1, ptr(Y), 17, ptr(X), 17, ptr(D), 17, ptr(B), 17, None, 1, ptr(out), 17,
                                            None, 2, None)

    assert dnmf(_make_params(17, 15, 2, 1.0, 10, 0.0, 1, True, 2, 0.0, None, None)) == 3       # a FULL sparsity matrix: SNMF_ERR_DIM here
    assert dnmf(_make_params(17, 15, 3, 1.0, 10, 0.0, 1, True, 0, 5.0, None, None)) == 3       # r != R_x + R_d
    s = np.ascontiguousarray(samples())
    p = fo.default_params()
    sp, _win = fe._params(p)
    T = fe.num_frames(s.size, p)
    idx = np.arange(4, dtype=np.int64)
    bd, bm = np.empty((513, 4), order="F"), np.empty((64, 4), order="F")
    mel = np.ascontiguousarray(fe.mel_matrix(p["fs"], 64, p["fftlength"], 1.0, p["fs"] / 2).T)

    def train_entry(q):
        return lib.snmf_run_basis_train_audio_fp64(gpu_ctx._h, C.byref(q), C.byref(sp), -1.0, ptr(mel), 64, ptr(s), s.size, ptr(idx), 0, None, 1,
                                                   ptr(bd), None, ptr(bm), None, None)

    assert train_entry(_make_params(513, T, 4, 1.0, 3, 0.0, 1, True, 2, 0.0, None, None)) == 8     # FULL sparsity: SNMF_ERR_UNSUPPORTED
    assert train_entry(_make_params(513, T + 1, 4, 1.0, 3, 0.0, 1, True, 0, 5.0, None, None)) == 3  # p->T is not the frame count
    assert train_entry(_make_params(512, T, 4, 1.0, 3, 0.0, 1, True, 0, 5.0, None, None)) == 3      # p->F is not the feature rows
    x = np.ascontiguousarray(s[:9000])
    q = _make_params(513, fe.num_frames(9000, p) + 2, 2, 1.0, 3, 0.0, 1, True, 0, 5.0, None, None)
    Bw = np.ones((513, 2), order="F")
    assert lib.snmf_run_basis_dnmf_audio_fp64(gpu_ctx._h, C.byref(q), C.byref(sp), 1, 1, ptr(x), x.size, ptr(x), x.size, None, 0, ptr(Bw), 513,
                                              None, 1, ptr(bd), 513, None, 2, None) == 3
    assert train_entry(_make_params(513, T, 4, 1.0, 3, 0.0, 1, True, 0, 5.0, None, None)) == 0      # and the valid call goes through
    after = dnmf_device(name, gpu_ctx)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
