"""The MEX shims (integration/*_mex.cpp) executed on the device under the test host (tests/mexhost.py, tests/mexhost/):
what a MATLAB caller gets through them.

Two judgements per case.
  1. Against the Python binding, BIT FOR BIT: shim and binding make the same C entry call with the same values on the same
     device, and runs are bitwise reproducible (tests/test_gpu_parity.py::test_runs_are_bitwise_reproducible).  Where the
     binding post-processes (truncated objective vectors, normalised dictionaries, a Mel table of its own) the C entry is
     called through _lib with the shim's values instead.
  2. Against the fp64 oracle, with the bounds the existing modules hold that entry to (imported, none added): REL_WH /
     REL_COST of tests/test_gpu_parity.py for the fp32 solves and the fp32 DNMF loop, REL_WH / REL_COST of
     tests/test_gpu_solve_f64.py for 'fp64' (REL_SOLVE of tests/test_gpu_train_f64.py, the same 1e-11, for the fp64 callers),
     REL / REL_COST of tests/test_mdi.py, AB_STFT / EPS of tests/test_gpu_frontend_envelope.py (the bound of
     tests/test_frontend.py), REL_OUT and _check_trace of tests/test_online.py.  Two bounds are literals in their modules and
     restated here under a name: REL_TRAIN_F32 = 2e-4 (tests/test_frontend.py::test_basis_training_caller_end_to_end) and
     the 1 LSB / 1e-3 of the int16 stream and the adapted dictionary (tests/test_online.py).  This judgement is what
     catches a mistake the shim and the binding share.
Every call also runs under the host's checks (guard zones round every array, input checksums, lifetimes): a recorded
host error fails the call.  Shapes are small with pairwise different dimensions that are no multiples of one another
(F = 65, T = 300, r = 20; F = 33, R_x = 5, R_d = 4; Mel 7 x 33), so a transposition or a swapped leading dimension
cannot pass.

No case is exempt from the bit-for-bit comparison, and none is judged by the oracle alone.  Where the second judgement is
indirect:
  * snmf_online_mex returns the int16 stream and the dictionary; the float signal and the per-frame trace are not exposed
    to MATLAB.  REL_OUT and _check_trace are therefore applied to the binding's run of the same call, whose int16 stream
    and dictionary the shim's must equal bit for bit; the shim's own int16 stream is held to the oracle's within 1 LSB and
    its dictionary within 1e-3, as tests/test_online.py holds the binding's.
  * 'train' returns the raw dictionaries; run_basis_train.m:113-116 (column norm + 1e-9) is the wrapper's part and is
    applied here before the comparison with the oracle, which returns the stored form.

Defects found while writing these tests and fixed with them (integration/snmf_online_mex.cpp, all in
test_online_wrong_sizes_are_refused): 'basis' sized its output by the F and R_d the CALLER stated, while
snmf_online_get_basis_* copies the handle's R_d columns at the leading dimension it is given -- a smaller stated R_d was
written past the end of the matrix, a larger stated F gave a matrix with rows of zeros between the columns; 'set_mel' read
melmat without a type check and all three matrices without a size check; 'process' took a pcm matrix of any shape.

Measured on an MI355X (every test prints its figures before it asserts): all bit-for-bit comparisons equal; against the
oracle fp32 solves relW <= 2.7e-7, relH <= 6.4e-7; 'fp64' <= 2.1e-15; MDI <= 7.5e-7; STFT <= 0.035 of the bound (fp32),
<= 0.0041 (fp64); Mel <= 0.11 of the bound; DNMF relB <= 1.2e-7 (fp32), <= 4.9e-16 (fp64); training <= 1.9e-7 / 5.2e-16;
online relOut 1.1e-7 (fp32), 3.4e-16 (fp64), int16 streams equal to the oracle's; every decision trace equal.  The module
runs in under 5 s.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import frontend_envelope as env
from mexhost import MexError, mex_shims  # noqa: F401  (session fixture)
from oracle import frontend_oracle as fo
from oracle.mdi_oracle import snmf_mdi as oracle_mdi
from oracle.online_oracle import default_params as online_defaults, ntf_sep_event_rt as oracle_rt
from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem
from test_gpu_frontend_envelope import AB_STFT, EPS, judge as judge_features
from test_gpu_parity import REL_WH, check, rel
from test_gpu_solve_f64 import REL_COST as REL_COST_F64, REL_WH as REL_WH_F64, relmax
from test_gpu_train_f64 import REL_SOLVE
from test_mdi import REL as REL_MDI, REL_COST as REL_COST_MDI
from test_online import GEOMETRIES, REL_OUT, _check_trace, _random_setup

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL_TRAIN_F32 = 2e-4   # tests/test_frontend.py::test_basis_training_caller_end_to_end (a literal there)
LSB_I16, REL_BASIS = 1, 1e-3  # tests/test_online.py::test_device_other_geometries_match_the_oracle (literals there)

F, T, R = 65, 300, 20
V, W0, H0 = synth_problem(F, T, R)
bits = lambda a: np.ascontiguousarray(a).tobytes()  # noqa: E731
ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert bits(np.asfortranarray(a)) == bits(np.asfortranarray(b)), f"{what}: shim and binding differ (max |d| = {np.abs(a - b).max():.3e})"


# ---- sparse_nmf_mex ------------------------------------------------------------------------------------------------------
_rs = np.random.RandomState(3)
SEMI = np.arange(R) >= 7        # the first 7 atoms are a fixed dictionary, the rest are learnt (semi-supervised)
NONE, ALL = np.zeros(R, bool), np.ones(R, bool)
KL = dict(cf="kl", sparsity=5, max_iter=25, conv_eps=0, cost_check=1)
# name -> (binding / oracle p, what the shim's opts add, keyword arguments of the binding)
SOLVES = {
    "sparsity-scalar": (KL, {}, {}),
    "sparsity-rx1": (dict(KL, sparsity=np.linspace(0, 9, R).reshape(-1, 1)), {}, {}),
    "sparsity-rxT": (dict(KL, sparsity=np.abs(_rs.randn(R, T)) * 4), {}, {}),
    "semi-logical": (dict(KL, w_update_ind=SEMI), dict(w_update_ind=SEMI), {}),
    "semi-double": (dict(KL, w_update_ind=SEMI), dict(w_update_ind=SEMI * 1.0), {}),
    "h-only-logical": (dict(KL, w_update_ind=NONE), dict(w_update_ind=NONE, h_update_ind=ALL), {}),
    "h-only-double": (dict(KL, w_update_ind=NONE), dict(w_update_ind=NONE * 1.0, h_update_ind=ALL.reshape(1, -1) * 1.0), {}),
    "w-only-logical": (dict(KL, h_update_ind=NONE), dict(h_update_ind=NONE), {}),
    "w-only-double": (dict(KL, h_update_ind=NONE), dict(h_update_ind=NONE * 1.0), {}),
    "beta0": (dict(KL, cf="is", sparsity=0.1, max_iter=15), {}, {}),
    "beta05": (dict(KL, cf="beta", beta=0.5, sparsity=1, max_iter=15), {}, {}),
    "beta1": (dict(KL, max_iter=15), {}, {}),
    "beta2": (dict(KL, cf="ed", sparsity=0.5, max_iter=15), {}, {}),
    "floor_v0": (KL, dict(floor_v=0.0), dict(gpu_variant=True)),
    "cost_check0": (dict(KL, cost_check=0), {}, {}),
    "early-stop": (dict(KL, conv_eps=2e-3, max_iter=200), {}, {}),
    "fp64": (KL, dict(precision="fp64"), dict(precision="fp64")),
    "fp64-early-stop-rx1": (dict(KL, conv_eps=2e-3, max_iter=200, sparsity=np.linspace(0, 9, R).reshape(-1, 1)), dict(precision="fp64"),
                            dict(precision="fp64")),
    "devices00": (KL, dict(devices=[0.0, 0.0]), dict(devices=[0, 0])),
}


def beta_of(p):
    return {"is": 0.0, "kl": 1.0, "ed": 2.0}.get(p["cf"], p.get("beta", 1.0))


def shim_opts(p, extra):
    o = dict(beta=beta_of(p), max_iter=float(p["max_iter"]), conv_eps=float(p["conv_eps"]), cost_check=float(p["cost_check"]), floor_v=1.0,
             device=0.0)
    o.update(extra)
    return o


@functools.lru_cache(maxsize=None)
def solve_reference(name):
    p, _, kw = SOLVES[name]
    return oracle_nmf(V, dict(p, init_w=W0, init_h=H0), gpu_variant=bool(kw.get("gpu_variant")))


def binding_solve(name, ctx):
    from se_snmf_nat_amd import sparse_nmf, sparse_nmf_GPU
    p, _, kw = SOLVES[name]
    kw = dict(kw)
    fn = sparse_nmf_GPU if kw.pop("gpu_variant", False) else sparse_nmf
    if "devices" not in kw:
        kw["ctx"] = ctx
    return fn(V, dict(p, init_w=W0, init_h=H0), **kw)


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_sparse_nmf_mex(mex_shims, gpu_ctx, name):
    p, extra, kw = SOLVES[name]
    m = mex_shims["sparse_nmf_mex"]
    w, h, div, cost, nit = m(5, V, W0, H0, p["sparsity"], shim_opts(p, extra))
    mi = p["max_iter"]
    assert (w.shape, h.shape, div.shape, cost.shape, nit.shape) == ((F, R), (R, T), (1, mi), (1, mi), (1, 1))
    n = int(nit[0, 0])
    wb, hb, ob = binding_solve(name, gpu_ctx)
    same_bits(w, wb, "w")
    same_bits(h, hb, "h")
    assert n == ob["n_iter"]
    gpu_variant = bool(kw.get("gpu_variant"))
    if p["cost_check"] and not gpu_variant:  # the binding cuts the vectors at an early stop, as integration/sparse_nmf.m does
        k = len(ob["cost"])
        assert k == (n if n < mi else mi)
        same_bits(div[0, :k], ob["div"], "div")
        same_bits(cost[0, :k], ob["cost"], "cost")
        assert not div[0, k:].any() and not cost[0, k:].any()
    wr, hr, orf = solve_reference(name)
    if name == "early-stop" or name.startswith("fp64-early"):
        assert orf["n_iter"] < mi, "the case must stop early"
    if "precision" in extra:
        ew, eh = rel(w, wr), rel(h, hr)
        ed, ec = relmax(div[0, :n], orf["div"]), relmax(cost[0, :n], orf["cost"])
        print(f"sparse_nmf_mex {name}: n_iter {n} (oracle {orf['n_iter']}) relW={ew:.2e} relH={eh:.2e} reldiv={ed:.2e} relcost={ec:.2e}")
        assert n == orf["n_iter"] and ew < REL_WH_F64 and eh < REL_WH_F64 and ed < REL_COST_F64 and ec < REL_COST_F64
    else:
        k = n if n < mi else mi
        o = {"n_iter": n, "div": div[0, :k], "cost": cost[0, :k]}
        print(f"sparse_nmf_mex {name}: n_iter {n} (oracle {orf['n_iter']}) relW={rel(w, wr):.2e} relH={rel(h, hr):.2e}")
        check((w, h, o), (wr, hr, orf), cost=bool(p["cost_check"]) and not gpu_variant, vsum=float(V.sum()))
        if not p["cost_check"] or gpu_variant:
            assert gpu_variant or (not div.any() and not cost.any())


@pytest.mark.parametrize("nlhs", [0, 1, 2, 5])
def test_sparse_nmf_mex_output_counts(mex_shims, gpu_ctx, nlhs):
    p, extra, _ = SOLVES["sparsity-scalar"]
    full = mex_shims["sparse_nmf_mex"](5, V, W0, H0, p["sparsity"], shim_opts(p, extra))
    out = mex_shims["sparse_nmf_mex"](nlhs, V, W0, H0, p["sparsity"], shim_opts(p, extra))
    assert len(out) == max(nlhs, 1)
    for a, b in zip(out, full):
        same_bits(a, b, f"output of nlhs={nlhs}")


def test_sparse_nmf_mex_cached_context_and_reload(mex_shims, gpu_ctx):
    """Two calls in a row reuse the locked context and give the same bits; after the exit function (MATLAB exit / clear of
    an unlocked MEX file) a third call makes a new context and gives them again."""
    m = mex_shims["sparse_nmf_mex"]
    p, extra, _ = SOLVES["semi-logical"]
    args = (V, W0, H0, p["sparsity"], shim_opts(p, extra))
    a = m(5, *args)
    locks = m.lock_count()
    assert locks >= 1 and m.has_exit_fcn()
    b = m(5, *args)
    assert m.lock_count() == locks, "the second call must reuse the context"
    m.unload()
    assert m.lock_count() == 0 and not m.has_exit_fcn()
    c = m(5, *args)
    assert m.lock_count() == 1 and m.has_exit_fcn()
    for x, y, z in zip(a, b, c):
        same_bits(x, y, "second call")
        same_bits(x, z, "call after the exit function")


# ---- snmf_mdi_mex --------------------------------------------------------------------------------------------------------
_rm = np.random.RandomState(0)
MASK_BIN = (_rm.rand(F, T) > 0.3).astype(np.float64)
MASK_SOFT = np.clip(MASK_BIN * 0.8 + _rm.rand(F, T) * 0.2, 0, 1)
MDI_P = dict(cf="kl", sparsity_mdi=0.5, conv_eps_mdi=1e-4, max_iter=40, cost_check=1)


@pytest.mark.parametrize("nlhs", [1, 6])
@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
def test_snmf_mdi_mex(mex_shims, gpu_ctx, soft, nlhs):
    from se_snmf_nat_amd import Plan, snmf_mdi, snmf_mdi_Sm
    M = MASK_SOFT if soft else MASK_BIN
    p = dict(MDI_P, init_w=W0, init_h=H0)
    opts = dict(beta=1.0, max_iter=40.0, conv_eps=1e-4, cost_check=1.0, device=0.0)
    out = mex_shims["snmf_mdi_mex"](nlhs, V, M, W0, H0, 0.5, opts)
    assert len(out) == nlhs
    v_b, h_b, o_b = (snmf_mdi_Sm if soft else snmf_mdi)(V, M, p, ctx=gpu_ctx)
    v_r, h_r, o_r = oracle_mdi(V, M, p)
    same_bits(out[0], v_b, "v_mdi")
    assert out[0].shape == (F, T)
    print(f"snmf_mdi_mex soft={soft}: relV={rel(out[0], v_r):.2e}")
    assert rel(out[0], v_r) < REL_MDI
    if nlhs == 6:
        v, w, h, div, cost, nit = out
        assert (w.shape, h.shape, div.shape, cost.shape, nit.shape) == ((F, R), (R, T), (1, 40), (1, 40), (1, 1))
        n = int(nit[0, 0])
        same_bits(h, h_b, "h")
        assert n == o_b["n_iter"] == o_r["n_iter"]
        k = len(o_b["cost"])
        same_bits(cost[0, :k], o_b["cost"], "cost")
        same_bits(div[0, :k], o_b["div"], "div")
        # w is not returned by the binding: the same plan calls, made here
        pl = Plan(gpu_ctx, F, T, R, beta=1.0, max_iter=40, conv_eps=1e-4, cost_check=True, floor_v=True, sparsity=0.5, w_update_ind=ALL,
                  h_update_ind=ALL)
        pl.set_mask(M); pl.set_v(V); pl.set_w(W0); pl.set_h(H0); pl.init(); pl.run()  # noqa: E702
        same_bits(w, pl.get_w(), "w")
        pl.close()
        print(f"snmf_mdi_mex soft={soft}: n_iter {n} relH={rel(h, h_r):.2e} relW={rel(w, o_r['w']):.2e}")
        assert rel(h, h_r) < REL_MDI and rel(w, o_r["w"]) < REL_MDI
        assert len(o_r["cost"]) == k
        np.testing.assert_allclose(cost[0, :k], o_r["cost"], rtol=REL_COST_MDI, atol=2e-7 * V.sum())
        if not soft:  # observed entries are the input's (tests/test_mdi.py)
            obs = M == 1
            assert np.array_equal(v[obs].astype(np.float32), np.maximum(V, 1e-9)[obs].astype(np.float32))


# ---- snmf_frontend_mex ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def audio():
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    s.setflags(write=False)
    return s


STFT_GEOS = {"n64": (64, 64, 16, 2800, 1), "n1024": (1024, 640, 160, 4000, 5)}  # fftlength, framelength, frameshift, samples, DC_bin


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("splice", [0, 1])
@pytest.mark.parametrize("geo", sorted(STFT_GEOS))
def test_frontend_mex_stft(mex_shims, gpu_ctx, geo, splice, prec):
    from se_snmf_nat_amd import frontend as fe
    N, fl, fs, L, dc = STFT_GEOS[geo]
    p = env.case(N, fl, fs, dc, 0.92, 1, splice, None)
    s = audio()[1000:1000 + L]
    mp = {k: (float(v) if np.isscalar(v) else v) for k, v in p.items() if k not in ("T", "fs", "DCbin")}
    if prec == "fp64":
        mp["snmf_precision"] = "fp64"
    (tf,) = mex_shims["snmf_frontend_mex"](1, "stft", s, mp, float(dc))
    nfr = fe.num_frames(L, p)
    assert tf.shape == ((2 * splice + 1) * (N // 2 + 1), nfr) and nfr > 2 * splice + 1
    got_b = fe.stft_features(s, p, ctx=gpu_ctx, precision=prec)
    same_bits(tf, got_b.astype(np.float64), "TF_mag")
    mode = "f32" if prec == "fp32" else "fp64"
    ref = env.features(s.astype(np.float32).astype(np.float64) if prec == "fp32" else s, p)
    judge_features(f"snmf_frontend_mex stft {geo} Splice={splice} {prec}", tf, ref, env.colmax(ref, p), AB_STFT[mode])


MELMAT = np.random.RandomState(11).rand(7, 33) * (np.random.RandomState(12).rand(7, 33) > 0.3)  # 7 x 33, non-negative, not square


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("K", [1, 3])
def test_frontend_mex_mel(mex_shims, gpu_ctx, lib, K, prec):
    """'mel' with a non-square table: against the C entry called with the row-major table (the binding builds its own square-ish
    table from p) and against blockdiag(melmat) @ V in NumPy fp64, (w + 1) eps per element (non-negative terms)."""
    Tm = 41
    rs = np.random.RandomState(K)
    dt, mode = (np.float32, "f32") if prec == "fp32" else (np.float64, "fp64")
    Vm = (rs.gamma(0.5, 1.0, (K * 33, Tm)) * 10.0 ** rs.uniform(-2, 2, (K * 33, 1))).astype(dt).astype(np.float64)
    (mel,) = mex_shims["snmf_frontend_mex"](1, "mel", Vm, MELMAT, float(K), *(["fp64"] if prec == "fp64" else []))
    assert mel.shape == (K * 7, Tm)
    table = np.ascontiguousarray(MELMAT, dtype=dt)  # row-major 7 x 33
    vin, out = np.asfortranarray(Vm, dtype=dt), np.zeros((K * 7, Tm), dtype=dt, order="F")
    assert getattr(lib, "snmf_mel_features_" + mode)(gpu_ctx._h, ptr(table), 7, 33, K, ptr(vin), K * 33, Tm, ptr(out), K * 7, 0) == 0
    same_bits(mel, out.astype(np.float64), "TF_Mel")
    ref = np.kron(np.eye(K), MELMAT) @ Vm
    w = int((MELMAT != 0).sum(1).max())
    err, bound = np.abs(mel - ref), (w + 1) * EPS[mode] * ref
    print(f"snmf_frontend_mex mel K={K} {prec}: max err/bound = {float((err[bound > 0] / bound[bound > 0]).max()):.2e}")
    assert ref.max() > 0 and (err <= bound).all()


# ---- snmf_dnmf_mex -------------------------------------------------------------------------------------------------------
N_FFT, NB, L_X, L_D, RX, RD = 64, 33, 3000, 2900, 5, 4
WIN = env.window(64)
DP = dict(fs=16000, framelength=64, frameshift=16, fftlength=64, DCbin=1, Splice=0, preemph=0.0, pow=2, nonzerofloor=1e-9, win_STFT=WIN,
          F_order=7, R_x=RX, R_d=RD, cf="kl", sparsity=5, max_iter=8, conv_eps=0, cost_check=1, random_seed=3)


def mex_p(p, **over):
    q = {k: (float(v) if isinstance(v, (int, float)) else v) for k, v in p.items() if k != "fs"}
    q.update(over)
    return q


def melmat_of(p):
    from se_snmf_nat_amd import frontend as fe
    return np.ascontiguousarray(fe.mel_matrix(p["fs"], p["F_order"], p["fftlength"], 1.0, p["fs"] / 2).T)  # F_order x (fftlength/2+1)


def dnmf_oracle(x, d, B, p, mel, h0):
    """run_basis_DNMF.m:36-55 on the oracle's features with a given first H (fo.run_basis_DNMF draws its own): B_hat, n_iter."""
    n = min(len(x), len(d))
    feats = [fo.dft_features(sig, p) for sig in (x[:n] + d[:n], x[:n], d[:n])]
    if mel:
        feats = [fo.mel_features(M, p) for M in feats]
    Y, X, D = feats
    q = {k: p[k] for k in ("cf", "sparsity", "max_iter", "conv_eps", "cost_check")}
    r = RX + RD
    _, A, o1 = oracle_nmf(Y, dict(q, w_update_ind=np.zeros(r, bool), h_update_ind=np.ones(r, bool), init_w=B, init_h=h0))
    bx, _, o2 = oracle_nmf(X, dict(q, w_update_ind=np.ones(RX, bool), h_update_ind=np.zeros(RX, bool), init_w=B[:, :RX], init_h=A[:RX]))
    bd, _, o3 = oracle_nmf(D, dict(q, w_update_ind=np.ones(RD, bool), h_update_ind=np.zeros(RD, bool), init_w=B[:, RX:], init_h=A[RX:]))
    return np.concatenate([bx, bd], axis=1), [o1["n_iter"], o2["n_iter"], o3["n_iter"]]


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("h0", ["given", "device"])
@pytest.mark.parametrize("mel", [False, True], ids=["DFT", "Mel"])
def test_dnmf_mex_dnmf(mex_shims, gpu_ctx, mel, h0, prec):
    from se_snmf_nat_amd import frontend as fe, train
    from se_snmf_nat_amd.api import philox_uniform
    x, d = audio()[:L_X].copy(), audio()[5000:5000 + L_D][::-1].copy()  # unequal lengths: cut to the shorter one
    Fd = 7 if mel else NB
    B = np.random.RandomState(5).rand(Fd, RX + RD) + 0.05
    Td = fe.num_frames(min(L_X, L_D), DP)
    seed = DP["random_seed"]
    H_host = np.asfortranarray(np.random.RandomState(seed).random_sample((RX + RD, Td)))
    melmat = melmat_of(DP) if mel else None
    assert melmat is None or (melmat.shape == (7, NB) and (melmat.sum(1) > 0).all())
    mp = mex_p(DP, **({"snmf_precision": "fp64"} if prec == "fp64" else {}))
    b_hat, nit = mex_shims["snmf_dnmf_mex"](2, "dnmf", x, d, B, H_host if h0 == "given" else None, mp, melmat)
    assert b_hat.shape == (Fd, RX + RD) and nit.shape == (1, 3)
    # the binding's own call: h0="host" draws RandomState(seed), the H0 given above; "device" is the Philox draw
    fn = train._run_basis_dnmf_audio
    bb = fn(x, d, B, DP, ctx=gpu_ctx, mel=mel, h0="host" if h0 == "given" else "device", precision=prec)
    same_bits(b_hat, bb, "B_hat")
    first = H_host if h0 == "given" else philox_uniform(seed, RX + RD, Td).astype(np.float64)
    xr, dr = (x, d) if prec == "fp64" else (x.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64))
    br, nr = dnmf_oracle(xr, dr, B, DP, mel, first)
    tol = REL_SOLVE if prec == "fp64" else REL_WH
    print(f"snmf_dnmf_mex dnmf mel={mel} h0={h0} {prec}: n_iter {nit[0].tolist()} (oracle {nr}) relB={rel(b_hat, br):.2e}")
    assert nit[0].tolist() == nr
    assert rel(b_hat, br) < tol


def test_dnmf_mex_dnmf_multi(mex_shims, gpu_ctx):
    """'dnmf_multi' over [0 0]: formed features, two ranks on the one device, against run_basis_dnmf(devices=[0, 0])."""
    from se_snmf_nat_amd import run_basis_dnmf
    Fm, Tm = 33, 230
    X = synth_problem(Fm, Tm, RX + 2, seed_data=11)[0]
    D = synth_problem(Fm, Tm, RD + 2, seed_data=12)[0]
    Y = X + D
    B = np.random.RandomState(5).rand(Fm, RX + RD) + 0.05
    H = np.asfortranarray(np.random.RandomState(3).random_sample((RX + RD, Tm)))
    p = {k: DP[k] for k in ("cf", "sparsity", "max_iter", "conv_eps", "cost_check", "random_seed")}
    mp = mex_p(dict(p, R_x=RX, R_d=RD))
    b_hat, nit = mex_shims["snmf_dnmf_mex"](2, "dnmf_multi", Y, X, D, B, H, mp, [0.0, 0.0])
    info = {}
    bb, _ = run_basis_dnmf(Y, X, D, B, RX, RD, p, devices=[0, 0], h0=H, info=info)
    assert b_hat.shape == (Fm, RX + RD) and nit.shape == (1, 3)
    same_bits(b_hat, bb, "B_hat")
    assert nit[0].tolist() == info["n_iter"]
    q = {k: p[k] for k in ("cf", "sparsity", "max_iter", "conv_eps", "cost_check")}
    r = RX + RD
    _, A, o1 = oracle_nmf(Y, dict(q, w_update_ind=np.zeros(r, bool), init_w=B, init_h=H))
    bx, _, o2 = oracle_nmf(X, dict(q, h_update_ind=np.zeros(RX, bool), init_w=B[:, :RX], init_h=A[:RX]))
    bd, _, o3 = oracle_nmf(D, dict(q, h_update_ind=np.zeros(RD, bool), init_w=B[:, RX:], init_h=A[RX:]))
    print(f"snmf_dnmf_mex dnmf_multi: relB={rel(b_hat, np.concatenate([bx, bd], axis=1)):.2e}")
    assert nit[0].tolist() == [o1["n_iter"], o2["n_iter"], o3["n_iter"]]
    assert rel(b_hat, np.concatenate([bx, bd], axis=1)) < REL_WH


TRAIN_IDX = np.array([9, 151, 2, 77, 40, 123], dtype=np.float64)  # 1-based frame indices (randsample), R = 6


def train_entry(lib, ctx, s, p, idx0, h0, prec, exemplar, Tt):
    """snmf_run_basis_train_audio_* through _lib with the shim's values: the indices minus one."""
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    f64 = prec == "fp64"
    sdt = np.float64 if f64 else np.float32
    sp, _win = fe._params(p)
    r = len(idx0)
    if exemplar:
        q = _make_params(NB, Tt, r, 1.0, 1, 0.0, 0, True, 0, 0.0, None, None)
    else:
        q = _make_params(NB, Tt, r, 1.0, p["max_iter"], p["conv_eps"], p["cost_check"], True, 0, p["sparsity"], None, None)
    sv = np.ascontiguousarray(s, dtype=sdt)
    mel = np.ascontiguousarray(melmat_of(p), dtype=sdt)
    bd, bm = np.zeros((NB, r), order="F"), np.zeros((7, r), order="F")
    ad = am = None
    if not exemplar:
        ad, am = np.zeros((r, Tt), order="F"), np.zeros((r, Tt), order="F")
    nit = np.zeros(2, np.int32)
    fn = lib.snmf_run_basis_train_audio_fp64 if f64 else lib.snmf_run_basis_train_audio_f64
    dd = float(p["alpha_eta"]) if p.get("domain_DD", 0) else -1.0
    seed = 1 if (h0 is not None or exemplar) else int(p["random_seed"])
    assert fn(ctx._h, C.byref(q), C.byref(sp), dd, ptr(mel), 7, ptr(sv), sv.size, ptr(idx0), 1 if exemplar else 0, ptr(h0), seed,
              ptr(bd), ptr(ad), ptr(bm), ptr(am), ptr(nit)) == 0
    return bd, bm, ad, am, nit


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("dd", [0, 1], ids=["plain", "domain_DD"])
@pytest.mark.parametrize("exemplar", [0, 1], ids=["solve", "train_Exemplar"])
def test_dnmf_mex_train(mex_shims, gpu_ctx, lib, exemplar, dd, prec):
    from se_snmf_nat_amd import frontend as fe
    s = audio()[2000:2000 + L_X].copy()
    p = dict(DP, train_Exemplar=exemplar, domain_DD=dd, alpha_eta=0.4, random_seed=1)
    Tt = fe.num_frames(L_X, p)
    assert Tt > TRAIN_IDX.max()
    r = len(TRAIN_IDX)
    H = None if exemplar else np.asfortranarray(np.random.RandomState(1).random_sample((r, Tt)))  # the oracle's draw of both solves
    mp = mex_p(p, **({"snmf_precision": "fp64"} if prec == "fp64" else {}))
    bd, bm, ad, am, nit = mex_shims["snmf_dnmf_mex"](5, "train", s, TRAIN_IDX, H, mp, melmat_of(p), 1.0)
    idx0 = np.ascontiguousarray(TRAIN_IDX, dtype=np.int64) - 1
    bd_b, bm_b, ad_b, am_b, nit_b = train_entry(lib, gpu_ctx, s, p, idx0, H, prec, exemplar, Tt)
    assert (bd.shape, bm.shape, nit.shape) == ((NB, r), (7, r), (1, 2))
    same_bits(bd, bd_b, "B_DFT")
    same_bits(bm, bm_b, "B_Mel")
    assert nit[0].tolist() == nit_b.tolist()
    sr = s if prec == "fp64" else s.astype(np.float32).astype(np.float64)
    norm = lambda M: M / np.sqrt((M ** 2).sum(0)) + 1e-9  # noqa: E731  run_basis_train.m:113-116, the wrapper's part
    tol = REL_SOLVE if prec == "fp64" else REL_TRAIN_F32
    if exemplar:  # run_basis_train.m:84, :95-96: the exemplar columns, the activations the scalar 0
        assert ad.shape == am.shape == (1, 1) and ad[0, 0] == 0 and am[0, 0] == 0
        Vr = fo.dft_features(sr, p)
        if dd:
            Vr = fo.tf_dd(Vr, p)
        ref = {"B_DFT_sub": norm(Vr[:, idx0]), "B_Mel_sub": norm(fo.mel_features(Vr, p)[:, idx0])}
        got = {"B_DFT_sub": norm(bd), "B_Mel_sub": norm(bm)}
    else:
        assert ad.shape == am.shape == (r, Tt)
        same_bits(ad, ad_b, "A_DFT")
        same_bits(am, am_b, "A_Mel")
        ref = fo.run_basis_train_signal(sr, r, p, TRAIN_IDX)
        got = {"B_DFT_sub": norm(bd), "B_Mel_sub": norm(bm), "A_DFT_sub": ad, "A_Mel_sub": am}
        assert nit[0].tolist() == [p["max_iter"]] * 2
    errs = {k: rel(got[k], ref[k]) for k in ref}
    print(f"snmf_dnmf_mex train exemplar={exemplar} domain_DD={dd} {prec}: " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k in ref:
        assert got[k].shape == ref[k].shape and errs[k] < tol, (k, errs[k])
    # the 1-based -> 0-based move, seen directly: column j of the raw exemplar dictionary is feature column sample_idx(j) - 1
    if exemplar and not dd:
        tf = fe.stft_features(s, p, ctx=gpu_ctx, precision=prec).astype(np.float64)
        same_bits(bd, np.asfortranarray(tf[:, idx0]), "B_DFT = TF_mag(:, sample_idx)")


# ---- snmf_online_mex -----------------------------------------------------------------------------------------------------
GEO = min(GEOMETRIES, key=lambda g: (g[0], g[3] + g[4]))  # fft 64, frame 64, hop 16, R 8 + 12
assert GEO[:5] == (64, 64, 16, 8, 12)
N_HOPS = 44


@functools.lru_cache(maxsize=None)
def online_setup():
    fft, sz, hop, R_x, R_d, over = GEO
    Bx, Bd, win = _random_setup(fft, fft, sz, hop, R_x, R_d)
    p = dict(online_defaults(), fftlength=fft, framelength=sz, frameshift=hop, win_STFT=win, win_ISTFT=win.copy(), overlapscale=2 * hop / sz)
    p.update(over)
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"][:hop * N_HOPS].astype(np.float64)
    rs = np.random.RandomState(7)
    H0o, Ad0 = rs.random_sample(R_x + R_d), rs.random_sample((p["R_a"], p["m_a"]))
    return Bx, Bd, p, s, H0o, Ad0


def online_mex_p(p, **over):
    from se_snmf_nat_amd.online import default_settings
    q = {k: (float(v) if isinstance(v, (int, float)) else v) for k, v in p.items() if k in default_settings() and k not in ("EVENT_RANK", "NOISE_RANK")}
    q.update(over)
    return q


def binding_settings(p):
    from se_snmf_nat_amd.online import default_settings
    return dict(default_settings(), **{k: v for k, v in p.items() if k in default_settings()})


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_online_mex_create_process_basis_destroy(mex_shims, gpu_ctx, prec):
    from se_snmf_nat_amd.online import OnlineSeparator
    Bx, Bd, p, s, H0o, Ad0 = online_setup()
    m = mex_shims["snmf_online_mex"]
    (h,) = m(1, "create", Bx, Bd, H0o, Ad0, online_mex_p(p, **({"precision": "fp64"} if prec == "fp64" else {})))
    assert h.shape == (1, 1) and h[0, 0] >= 1
    (x16,) = m(1, "process", h, s, 1.0)
    (Bn,) = m(1, "basis", h, 33.0, 12.0)
    m(0, "destroy", h)
    with pytest.raises(MexError) as e:
        m(1, "process", h, s, 1.0)
    assert e.value.id == "snmf:handle"
    assert x16.dtype == np.int16 and x16.shape[1] == 1 and Bn.shape == (33, 12) and Bn.dtype == np.float64
    sep = OnlineSeparator(Bx, Bd, binding_settings(p), H0=H0o, Ad_blk0=Ad0, ctx=gpu_ctx, precision=prec)
    out = sep.process(s, flush=True)
    tr, Bb = sep.trace(), sep.basis()
    sep.close()
    assert np.array_equal(x16[:, 0], out["x_tilde"]), "the int16 stream of shim and binding must be equal"
    same_bits(Bn, Bb, "B_DFT_d")
    o16, of, Bdn, tro = oracle_rt(s, Bx, Bd, p, H0o, Ad0, return_trace=True)
    _check_trace(tr, [t["n_iter"] for t in tro], [t["trig"] for t in tro], [t["n_up"] for t in tro], [t["adapt_iters"] for t in tro])
    ok = np.isfinite(of)
    e_out = np.linalg.norm(out["x_tilde_f"][ok] - of[ok]) / np.linalg.norm(of[ok])
    print(f"snmf_online_mex {prec}: relOut={e_out:.2e} max int16 diff={np.abs(x16[:, 0].astype(int) - o16.astype(int)).max()} relB={rel(Bn, Bdn):.2e}")
    assert e_out < REL_OUT
    assert len(x16) == len(o16) == (N_HOPS + 1) * 16 and np.abs(x16[:, 0].astype(int) - o16.astype(int)).max() <= LSB_I16
    assert rel(Bn, Bdn) < REL_BASIS
    assert sum(t["solved"] for t in tr) > 0


@pytest.mark.parametrize("melconv", [1, 0], ids=["MelConv1", "MelConv0"])
def test_online_mex_set_mel(mex_shims, gpu_ctx, melconv):
    """'set_mel' with a 12 x 33 table: against OnlineSeparator in Mel mode (which builds the same table) and the oracle."""
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.online import OnlineSeparator
    Bx, Bd, p, s, H0o, Ad0 = online_setup()
    p = dict(p, B_sep_mode="Mel", MelConv=melconv, F_order=12)
    melmat = np.ascontiguousarray(fe.mel_matrix(p["fs"], 12, 64, 1.0, p["fs"] / 2).T)
    assert melmat.shape == (12, 33) and (melmat.sum(1) > 0).all()
    BM = melmat @ np.concatenate([Bx, Bd], axis=1)
    BM = BM / np.sqrt((BM ** 2).sum(0)) + 1e-9
    BMx, BMd = np.asfortranarray(BM[:, :8]), np.asfortranarray(BM[:, 8:])
    m = mex_shims["snmf_online_mex"]
    (h,) = m(1, "create", Bx, Bd, H0o, Ad0, online_mex_p(p))
    m(0, "set_mel", h, melmat, BMx, BMd, float(melconv))
    (x16,) = m(1, "process", h, s, 1.0)
    (Bn,) = m(1, "basis", h, 33.0, 12.0)
    m(0, "destroy", h)
    sep = OnlineSeparator(Bx, Bd, binding_settings(p), H0=H0o, Ad_blk0=Ad0, ctx=gpu_ctx, B_Mel_x=BMx, B_Mel_d=BMd)
    out = sep.process(s, flush=True)
    tr, Bb = sep.trace(), sep.basis()
    sep.close()
    assert np.array_equal(x16[:, 0], out["x_tilde"])
    same_bits(Bn, Bb, "B_DFT_d")
    o16, of, _, tro = oracle_rt(s, Bx, Bd, p, H0o, Ad0, return_trace=True, mel=dict(B_Mel_x=BMx, B_Mel_d=BMd, melmat=melmat))
    _check_trace(tr, [t["n_iter"] for t in tro], [t["trig"] for t in tro], [t["n_up"] for t in tro], [t["adapt_iters"] for t in tro])
    ok = np.isfinite(of)
    e_out = np.linalg.norm(out["x_tilde_f"][ok] - of[ok]) / np.linalg.norm(of[ok])
    print(f"snmf_online_mex set_mel MelConv={melconv}: relOut={e_out:.2e} max int16 diff={np.abs(x16[:, 0].astype(int) - o16.astype(int)).max()}")
    assert e_out < REL_OUT and np.abs(x16[:, 0].astype(int) - o16.astype(int)).max() <= LSB_I16
    assert np.array_equal(Bn.astype(np.float32), Bd.astype(np.float32))  # B_DFT_d is not adapted in Mel mode (tests/test_online.py)


def test_online_mex_two_process_calls_equal_one(mex_shims, gpu_ctx):
    Bx, Bd, p, s, H0o, Ad0 = online_setup()
    m = mex_shims["snmf_online_mex"]
    mp = online_mex_p(p)
    (h1,) = m(1, "create", Bx, Bd, H0o, Ad0, mp)
    (one,) = m(1, "process", h1, s, 1.0)
    m(0, "destroy", h1)
    (h2,) = m(1, "create", Bx, Bd, H0o, Ad0, mp)
    cut = 16 * 17 + 5  # inside a hop
    (a,) = m(1, "process", h2, s[:cut], 0.0)
    (b,) = m(1, "process", h2, s[cut:].reshape(1, -1), 1.0)  # (a row vector is a vector too)
    m(0, "destroy", h2)
    assert a.shape[1] == b.shape[1] == 1 and a.dtype == b.dtype == np.int16
    assert np.array_equal(np.concatenate([a[:, 0], b[:, 0]]), one[:, 0])


def test_online_mex_two_handles_interleaved(mex_shims, gpu_ctx):
    """Two separators alive at once, fed in turns; one is destroyed mid-way and the other's remaining output is what it
    gives alone.  'process' on the destroyed handle, on 0 and on 99: snmf:handle."""
    Bx, Bd, p, s, H0o, Ad0 = online_setup()
    m = mex_shims["snmf_online_mex"]
    mp = online_mex_p(p)
    (h0,) = m(1, "create", Bx, Bd, H0o, Ad0, mp)
    (alone,) = m(1, "process", h0, s, 1.0)
    m(0, "destroy", h0)
    (ha,) = m(1, "create", Bx, Bd, H0o, Ad0, mp)
    (hb,) = m(1, "create", Bx, Bd[:, ::-1].copy(), H0o, Ad0, mp)
    assert ha[0, 0] != hb[0, 0]
    half = 16 * 20
    (a1,) = m(1, "process", ha, s[:half], 0.0)
    (b1,) = m(1, "process", hb, s[:half], 0.0)
    m(0, "destroy", hb)
    for bad in (hb, 0.0, 99.0):
        with pytest.raises(MexError) as e:
            m(1, "process", bad, s[half:], 1.0)
        assert e.value.id == "snmf:handle"
    (a2,) = m(1, "process", ha, s[half:], 1.0)
    m(0, "destroy", ha)
    assert not np.array_equal(a1, b1), "the two separators must be different streams"
    assert np.array_equal(np.concatenate([a1[:, 0], a2[:, 0]]), alone[:, 0])


def test_online_wrong_sizes_are_refused(mex_shims, gpu_ctx):
    """What needs a live handle to be decided: 'basis' with another F or R_d than the handle's (the library copies the handle's
    R_d columns: before the check, a smaller R_d stated by the caller was overrun), 'set_mel' with a table or dictionaries
    of the wrong size or type, 'process' with pcm that is not a real double vector.  All snmf:dim / snmf:type, and the handle
    works afterwards."""
    Bx, Bd, p, s, H0o, Ad0 = online_setup()
    m = mex_shims["snmf_online_mex"]
    (h,) = m(1, "create", Bx, Bd, H0o, Ad0, online_mex_p(p))
    mel, bx, bd = np.ones((12, 33)), np.ones((12, 8)), np.ones((12, 12))
    cases = [("snmf:dim", ("basis", h, 32.0, 12.0)), ("snmf:dim", ("basis", h, 33.0, 11.0)), ("snmf:dim", ("basis", h, 12.0, 33.0)),
             ("snmf:dim", ("basis", h, None, 12.0)),
             ("snmf:dim", ("set_mel", h, mel.T, bx, bd, 1.0)), ("snmf:dim", ("set_mel", h, mel[:, :-1], bx, bd, 1.0)),
             ("snmf:dim", ("set_mel", h, mel, bx[:-1], bd, 1.0)), ("snmf:dim", ("set_mel", h, mel, bx, bd[:, :-1], 1.0)),
             ("snmf:dim", ("set_mel", h, mel, bd, bx, 1.0)), ("snmf:dim", ("set_mel", h, mel, bx, bd, None)),
             ("snmf:type", ("set_mel", h, mel.astype(np.float32), bx, bd, 1.0)), ("snmf:type", ("set_mel", h, mel, bx > 0, bd, 1.0)),
             ("snmf:type", ("process", h, s.astype(np.int16), 1.0)), ("snmf:type", ("process", h, s.astype(np.float32), 1.0)),
             ("snmf:dim", ("process", h, s[:32].reshape(2, 16), 1.0)), ("snmf:dim", ("process", h, s, None))]
    for want, args in cases:
        with pytest.raises(MexError) as e:
            m(1, *args)
        assert e.value.id == want, (args[0], e.value.id, e.value.msg)
    (x16,) = m(1, "process", h, s, 1.0)
    assert len(x16) == (N_HOPS + 1) * 16
    m(0, "destroy", h)
