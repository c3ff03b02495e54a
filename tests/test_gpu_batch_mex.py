"""GPU tests of integration/snmf_batch_mex.cpp: every command on the device through the test host (tests/mexhost.py), every
output compared with np.array_equal against the Python binding called on the same inputs in the same process.  The binding and
the shim hand the same bytes to the same C entry, so equality of bits is the criterion; no tolerance is involved.  Where the
binding applies its host epilogue (B / sqrt(sum(B^2)) + 1e-9, run_basis_train.m:113-116) the same NumPy expression is applied to
the shim's raw output.  A HostError (guard zone, modified input, lifetime) fails the test that makes the call.

The shapes are the smallest at which the marshalling can go wrong: problems of pairwise different T (a wrong offset lands in a
neighbour's data), T_k = n_atoms, signal lengths that are no multiple of the hop, F_order = 8 != F = 33 (a transposed Mel table
shows), pairwise different ranks and settings that mix divergences and iteration limits in fp64."""
import numpy as np
import pytest

import assemble_cases as ac
import batch_ranks_cases as brc
import batch_settings_cases as bsc
import dnmf_audio_batch_cases as dac
import dnmf_batch_cases as dc
import dnmf_batch_ranks_cases as dbr
import mexhost
import train_batch_cases as tc
from batch_mex_cases import NAME, col, long, pack, settings_matrix, short, side, unpack
from mexhost import MexError
from oracle.sparse_nmf_oracle import synth_problem

pytestmark = pytest.mark.gpu
eq = np.array_equal
MODES = ("fp32", "fp64")


@pytest.fixture(scope="module")
def shim(tmp_path_factory, gpu_ctx):
    m = mexhost.Mex(mexhost.build_shim(NAME, tmp_path_factory.mktemp("batch_mex_gpu")))
    yield m
    m.unload()


def prec(p, mode):
    return dict(p, snmf_precision=mode)


def mel_table(p):
    from se_snmf_nat_amd import frontend
    return np.asfortranarray(frontend.mel_matrix(p["fs"], int(p["F_order"]), p["fftlength"], 1.0, p["fs"] / 2).T)  # = mel_matrix(...)'


def resolved(settings, shared):
    """Settings dicts -> (beta, sparsity, max_iter, conv_eps) per problem, as the binding resolves them."""
    from se_snmf_nat_amd.batch import _problem_settings
    from se_snmf_nat_amd.api import _solver_scalars
    beta, max_iter, conv_eps, _cc, lam = _solver_scalars(shared)
    return _problem_settings(settings, len(settings), dict(beta=beta, sparsity=lam, max_iter=max_iter, conv_eps=conv_eps))


# ---- 'solve' ---------------------------------------------------------------------------------------------------------------------
S_TS, S_R, S_F = [31, 70, 45, 33], 6, 33
P_SOLVE = dict(cf="kl", sparsity=5, max_iter=25, conv_eps=1e-2, cost_check=1)  # the oracle stops these four at 9, 13, 10 and 5


def solve_problems():
    return [synth_problem(S_F, T, S_R, seed_data=70 + b, seed_init=80 + b, r_true=3) for b, T in enumerate(S_TS)]


def check_solve(out, ref, ranks, Ts, F, max_iters):
    W, H, div, cost, n_iter = out
    Ws, Hs = unpack(W, [(F, r) for r in ranks]), unpack(H, [(r, T) for r, T in zip(ranks, Ts)])
    assert W.shape == (F, sum(ranks)) and div.shape == cost.shape == (max(max_iters), len(Ts)) and n_iter.shape == (len(Ts), 1)
    for k, (w, h, obj) in enumerate(ref):
        assert eq(Ws[k], w) and eq(Hs[k], h), k
        assert int(n_iter[k, 0]) == obj["n_iter"], k
        n = len(obj["div"])  # the binding cuts at an early stop, as the wrapper does; past it the shim's columns are zero
        assert n == min(obj["n_iter"], max_iters[k])
        assert eq(div[:n, k], obj["div"]) and eq(cost[:n, k], obj["cost"]) and not div[n:, k].any() and not cost[n:, k].any(), k


@pytest.mark.parametrize("mode", MODES)
def test_solve_one_rank(shim, gpu_ctx, mode):
    from se_snmf_nat_amd import batch
    pr = solve_problems()
    vs, w0, h0 = ([q[i] for q in pr] for i in range(3))
    fn = batch.sparse_nmf_batch if mode == "fp32" else batch.sparse_nmf_batch_fp64
    ref = fn(vs, dict(P_SOLVE, init_w=w0, init_h=h0), ctx=gpu_ctx)
    out = shim(5, "solve", side(vs), col(S_TS), side(w0), side(h0), prec(dict(P_SOLVE, r=S_R), mode), None)
    check_solve(out, ref, [S_R] * 4, S_TS, S_F, [25] * 4)
    stops = [int(v) for v in out[4][:, 0]]
    print(mode, "n_iter", stops)
    assert len(set(stops)) >= 3 and max(stops) < 25, "the problems stop at different iterations"
    assert out[1].shape == (S_R, sum(S_TS))  # one rank: H side by side


def test_solve_rvec_sparsity_and_masks(shim, gpu_ctx):
    from se_snmf_nat_amd import batch
    pr = solve_problems()[:3]
    vs, w0, h0 = ([q[i] for q in pr] for i in range(3))
    p = dict(P_SOLVE, sparsity=np.linspace(0.5, 5, S_R), w_update_ind=np.array([1, 0, 1, 1, 0, 1], bool), max_iter=6)
    ref = batch.sparse_nmf_batch(vs, dict(p, init_w=w0, init_h=h0), ctx=gpu_ctx)
    out = shim(5, "solve", side(vs), col(S_TS[:3]), side(w0), side(h0), dict(p, r=float(S_R)), None)  # (the mask crosses as a logical array)
    check_solve(out, ref, [S_R] * 3, S_TS[:3], S_F, [6] * 3)


def test_solve_a_rank_per_problem(shim, gpu_ctx):
    from se_snmf_nat_amd import batch
    pr = bsc.problems()
    vs, w0, h0 = ([np.array(q[i]) for q in pr] for i in range(3))
    p = dict(cf="kl", sparsity=5, max_iter=12, conv_eps=1e-2, cost_check=1)
    ref = batch.sparse_nmf_batch_fp64(vs, dict(p, r=list(bsc.RANKS), init_w=w0, init_h=h0), ctx=gpu_ctx)
    out = shim(5, "solve", side(vs), col(bsc.TS), pack(w0), pack(h0), prec(dict(p, r=col(bsc.RANKS)), "fp64"), None)
    check_solve(out, ref, bsc.RANKS, bsc.TS, bsc.F, [12] * 6)
    assert out[1].shape == (sum(r * t for r, t in zip(bsc.RANKS, bsc.TS)), 1)  # ranks differ: H as a column


@pytest.mark.parametrize("ranks", ["ranks", "one-rank"])
def test_solve_settings_per_problem(shim, gpu_ctx, ranks):
    """Divergences, sparsity weights, thresholds and iteration limits of their own: the oracle stops these at 4, 7, 26, 20, 17, 12."""
    from se_snmf_nat_amd import batch
    rs = bsc.RANKS if ranks == "ranks" else (5,) * 6
    pr = bsc.problems(ranks=rs)
    vs, w0, h0 = ([np.array(q[i]) for q in pr] for i in range(3))
    st = bsc.sweep_settings()
    ref = batch.sparse_nmf_batch_fp64(vs, [dict(s, init_w=w, init_h=h) for s, w, h in zip(st, w0, h0)], ctx=gpu_ctx)
    from se_snmf_nat_amd.api import _cf_to_beta
    S = settings_matrix([(_cf_to_beta(s), s["sparsity"], s["max_iter"], s["conv_eps"]) for s in st])
    out = shim(5, "solve", side(vs), col(bsc.TS), pack(w0), pack(h0), dict(r=col(rs), cost_check=1, snmf_precision="fp64"), S)
    check_solve(out, ref, rs, bsc.TS, bsc.F, list(bsc.MAX_ITER))
    stops = [int(v) for v in out[4][:, 0]]
    print(ranks, "n_iter", stops)
    if ranks == "ranks":
        assert len(set(stops)) >= 4


# ---- 'dnmf' ----------------------------------------------------------------------------------------------------------------------
def check_dnmf(out, ref, info, rs, Ts, F, widen=False):
    Bh, Ah, n_iter = out
    Bs, As = unpack(Bh, [(F, r) for r in rs]), unpack(Ah, [(r, T) for r, T in zip(rs, Ts)])
    assert Bh.shape == (F, sum(rs)) and n_iter.shape == (len(Ts), 3)
    for k, (b, a) in enumerate(ref):
        if widen:
            b, a = b.astype(np.float64), a.astype(np.float64)
        assert eq(Bs[k], b) and eq(As[k], a), k
    assert n_iter.astype(int).tolist() == info["n_iter"]


@pytest.mark.parametrize("form", ["fp32", "fp32-single", "fp64"])
def test_dnmf_matrices(shim, gpu_ctx, form):
    from se_snmf_nat_amd import batch
    E = dc.edges()
    Y, X, D, B, H0 = ([e[i] for e in E] for i in range(5))
    p = dict(dc.P_EDGES, R_x=dc.R_X, R_d=dc.R_D)
    info = {}
    dt = np.float32 if form == "fp32-single" else np.float64
    ref = batch.run_basis_dnmf_batch(Y, X, D, B, dc.R_X, dc.R_D, p, ctx=gpu_ctx, dtype=dt, h0=H0, precision=form[:4], info=info)
    q = prec(p, form[:4])
    if form == "fp32-single":
        q["snmf_single"] = 1.0
    out = shim(3, "dnmf", side(Y), side(X), side(D), col(dc.TS), side(B), side(H0), q, None)
    print(form, "n_iter", info["n_iter"])
    check_dnmf(out, ref, info, [dc.R_X + dc.R_D] * 6, dc.TS, dc.F, widen=form == "fp32-single")
    assert len({n[0] for n in info["n_iter"]}) >= 3


@pytest.mark.parametrize("with_settings", [False, True])
def test_dnmf_matrices_rank_pairs(shim, gpu_ctx, with_settings):
    from se_snmf_nat_amd import batch
    Q = dbr.problems()
    Y, X, D, B, H0 = ([q[i] for q in Q] for i in range(5))
    rx, rd = [a for a, _ in dbr.PAIRS], [b for _, b in dbr.PAIRS]
    rs = [a + b for a, b in dbr.PAIRS]
    st = dbr.SETTINGS if with_settings else None
    info = {}
    ref = batch.run_basis_dnmf_batch(Y, X, D, list(B), rx, rd, dbr.P_EDGES, ctx=gpu_ctx, h0=list(H0), precision="fp64", info=info, settings=st)
    S = settings_matrix(resolved(st, dbr.P_EDGES)) if with_settings else None
    out = shim(3, "dnmf", side(Y), side(X), side(D), col(dbr.TS), pack(B), pack(H0), dict(dbr.P_EDGES, R_x=col(rx), R_d=col(rd), snmf_precision="fp64"), S)
    print("settings" if with_settings else "shared", "n_iter", info["n_iter"])
    check_dnmf(out, ref, info, rs, dbr.TS, dbr.F)


# ---- 'dnmf_audio' ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mel", [False, True], ids=["dft", "mel"])
@pytest.mark.parametrize("h0", ["given", "device"])
def test_dnmf_waveforms(shim, gpu_ctx, mode, mel, h0):
    from se_snmf_nat_amd import train
    W = dac.waves()
    xs, ds = [w[0] for w in W], [w[1] for w in W]
    rows = dac.TINY["F_order"] if mel else dac.F
    B = dac.bases(rows)
    fn = train.run_basis_DNMF_Mel_batch if mel else train.run_basis_DNMF_batch
    info = {}
    ref = fn(xs, ds, list(B), dac.P_STOP, ctx=gpu_ctx, h0=list(dac.given_h0()) if h0 == "given" else "device", precision=mode, info=info)
    assert info["T"] == dac.TS and all(x.size != d.size for x, d in W)
    out = shim(3, "dnmf_audio", pack(xs), col([x.size for x in xs]), pack(ds), col([d.size for d in ds]), side(B),
               pack(dac.given_h0()) if h0 == "given" else None, prec(dac.P_STOP, mode), mel_table(dac.TINY) if mel else None, None)
    check_dnmf(out, ref, info, [dac.R_X + dac.R_D] * 6, dac.TS, rows)


@pytest.mark.parametrize("h0", ["given", "device"])
def test_dnmf_waveforms_rank_pairs_and_settings(shim, gpu_ctx, h0):
    from se_snmf_nat_amd import train
    W = dac.waves()
    xs, ds = [w[0] for w in W], [w[1] for w in W]
    rx, rd = [a for a, _ in dbr.PAIRS], [b for _, b in dbr.PAIRS]
    rs = [a + b for a, b in dbr.PAIRS]
    rng = np.random.RandomState(9)
    B = [rng.rand(dac.F, r) + 0.05 for r in rs]
    H0 = [rng.rand(r, T) for r, T in zip(rs, dac.TS)]
    p = dict(dac.P_STOP, R_x=rx, R_d=rd)
    info = {}
    ref = train.run_basis_DNMF_batch(xs, ds, B, p, ctx=gpu_ctx, h0=H0 if h0 == "given" else "device", precision="fp64", info=info, settings=dbr.SETTINGS)
    S = settings_matrix(resolved(dbr.SETTINGS, dac.P_STOP))
    out = shim(3, "dnmf_audio", pack(xs), col([x.size for x in xs]), pack(ds), col([d.size for d in ds]), pack(B), pack(H0) if h0 == "given" else None,
               dict(dac.P_STOP, R_x=col(rx), R_d=col(rd), snmf_precision="fp64"), None, S)
    check_dnmf(out, ref, info, rs, dac.TS, dac.F)


# ---- 'train' ---------------------------------------------------------------------------------------------------------------------
def epilogue(B):
    return B / np.sqrt((B ** 2).sum(0)) + 1e-9  # run_basis_train.m:113-116, as the binding applies it


def check_train(out, ref, info, atoms, Ts, p, exemplar=False):
    BD, BM, AD, AM, n_iter = out
    F, FM = tc.F, tc.F_MEL
    assert BD.shape == (F, sum(atoms)) and BM.shape == (FM, sum(atoms)) and n_iter.shape == (len(Ts), 2)
    bd, bm = unpack(BD, [(F, a) for a in atoms]), unpack(BM, [(FM, a) for a in atoms])
    if exemplar:
        assert AD.shape == AM.shape == (1, 1) and AD[0, 0] == 0 and AM[0, 0] == 0
    else:
        ad, am = (unpack(A, [(a, T) for a, T in zip(atoms, Ts)]) for A in (AD, AM))
    for k, r in enumerate(ref):
        assert eq(epilogue(bd[k]), r["B_DFT_sub"]) and eq(epilogue(bm[k]), r["B_Mel_sub"]), k
        if exemplar:
            assert r["A_DFT_sub"] == 0 and r["A_Mel_sub"] == 0
        else:
            assert eq(ad[k], r["A_DFT_sub"]) and eq(am[k], r["A_Mel_sub"]), k
    assert n_iter.astype(int).tolist() == info["n_iter"] and info["T"] == list(Ts)


TRAIN_VARIANTS = {
    "host_h0": (tc.P_STOP, "host"),
    "device_h0": (tc.P_STOP, "device"),
    "exemplar": (dict(tc.P_STOP, train_Exemplar=1), "host"),
    "dd": (dict(tc.P_STOP, domain_DD=1, alpha_eta=0.4), "host"),
}


def train_args(sigs, idx, atoms, H0, p, settings=None):
    return ("train", pack(sigs), col([s.size for s in sigs]), pack(idx), atoms, H0, p, mel_table(tc.TINY), 1.0, settings)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TRAIN_VARIANTS))
def test_train_from_signals(shim, gpu_ctx, mode, name):
    from se_snmf_nat_amd import train
    p, h0 = TRAIN_VARIANTS[name]
    sigs, idx = tc.signals(), tc.sample_idx()
    assert tc.TS[0] == tc.R and all(s.size % tc.TINY["frameshift"] for s in sigs)  # T_0 = n_atoms; no length is a multiple of the hop
    info = {}
    ref = train.run_basis_train_signal_batch(sigs, tc.R, p, DC_bin=1, sample_idx=list(idx), ctx=gpu_ctx, h0=h0, precision=mode, info=info)
    H0 = pack([tc.host_h0(T) for T in tc.TS]) if (h0 == "host" and name != "exemplar") else None
    out = shim(5, *train_args(sigs, idx, float(tc.R), H0, prec(p, mode)))
    print(mode, name, "n_iter", info["n_iter"])
    check_train(out, ref, info, [tc.R] * 6, tc.TS, p, exemplar=name == "exemplar")


@pytest.mark.parametrize("with_settings", [False, True])
def test_train_from_signals_atoms_and_settings_per_problem(shim, gpu_ctx, with_settings):
    from se_snmf_nat_amd import train
    sigs, idx = tc.signals(), brc.sample_idx()
    st = [dict(m, conv_eps=e, max_iter=mi) for m, e, mi in zip(bsc.MODES, bsc.CONV_EPS, bsc.MAX_ITER_NO_CC)] if with_settings else None
    info = {}
    ref = train.run_basis_train_signal_batch(sigs, brc.RANKS, tc.P_STOP, DC_bin=1, sample_idx=list(idx), ctx=gpu_ctx, h0="host", precision="fp64", info=info,
                                             settings=st)
    H0 = pack([tc.host_h0(T, n_ex=r) for T, r in zip(tc.TS, brc.RANKS)])
    S = settings_matrix(resolved(st, tc.P_STOP)) if with_settings else None
    out = shim(5, *train_args(sigs, idx, col(brc.RANKS), H0, prec(tc.P_STOP, "fp64"), S))
    check_train(out, ref, info, brc.RANKS, tc.TS, tc.P_STOP)


def test_train_settings_with_one_dictionary_size(shim, gpu_ctx):
    from se_snmf_nat_amd import train
    sigs, idx = tc.signals(), tc.sample_idx()
    st = [dict(m, conv_eps=e, max_iter=mi) for m, e, mi in zip(bsc.MODES, bsc.CONV_EPS, bsc.MAX_ITER_NO_CC)]
    info = {}
    ref = train.run_basis_train_signal_batch(sigs, tc.R, tc.P_STOP, DC_bin=1, sample_idx=list(idx), ctx=gpu_ctx, h0="device", precision="fp64", info=info,
                                             settings=st)
    out = shim(5, *train_args(sigs, idx, float(tc.R), None, prec(tc.P_STOP, "fp64"), settings_matrix(resolved(st, tc.P_STOP))))
    check_train(out, ref, info, [tc.R] * 6, tc.TS, tc.P_STOP)


# ---- 'assemble', 'signals_info', 'signals_get', 'train_signals', 'signals_destroy' -------------------------------------------------
def mixed_inputs():
    """tests/assemble_cases.py::case_mixed as the shim takes it: the clips as doubles wavread(.) * 32767, the ranges as
    load_anot returns them (src/load_anot.m:9-15: v_start = 0 becomes 1, v_end is clamped), [1; len] elsewhere."""
    c = ac.case_mixed()
    classes = [[ac.pcm_to_double(x) for x in cl] for cl in c["classes"]]
    rng = []
    for cl, r in zip(classes, c["ranges"]):
        for i, x in enumerate(cl):
            a, b = (1, x.size) if r is None else (max(int(r[i][0]), 1), min(int(r[i][1]), x.size))
            rng.append((a, b))
    return c, classes, np.asfortranarray(np.array(rng, dtype=np.float64).T)


P_ASM = dict(ac.P1000)


@pytest.fixture(scope="module")
def assembled(shim, gpu_ctx):
    from se_snmf_nat_amd import assemble_training_signals
    c, classes, rng = mixed_inputs()
    assert sorted(set(ac.modes(c))) == [0, 1, 2]
    flat = [x for cl in classes for x in cl]
    h = shim(1, "assemble", pack(flat), col([x.size for x in flat]), col([len(cl) for cl in classes]), col(ac.modes(c)), rng, P_ASM)[0]
    with assemble_training_signals(classes, P_ASM, vad=c["vad"], ranges=c["ranges"], ctx=gpu_ctx) as ts:
        yield h, ts
    shim(0, "signals_destroy", h)


def test_assembled_signals(shim, assembled):
    h, ts = assembled
    assert h.shape == (1, 1) and h[0, 0] >= 1
    n_samples, used = shim(2, "signals_info", h)
    assert n_samples.shape == used.shape == (7, 1)
    assert n_samples[:, 0].astype(np.int64).tolist() == ts.lengths and used[:, 0].astype(int).tolist() == ts.clips_used
    for k in range(7):
        s = shim(1, "signals_get", h, float(k + 1))[0]
        assert s.shape == (ts.lengths[k], 1) and eq(s[:, 0], ts.signal(k)), k
    for k in (0.0, 8.0, 1.5):
        with pytest.raises(MexError) as e:
            shim(1, "signals_get", h, k)
        assert e.value.id == "snmf:dim"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h0", ["host", "device"])
def test_train_on_assembled_signals(shim, gpu_ctx, assembled, mode, h0):
    from se_snmf_nat_amd import frontend, run_basis_train_assembled_batch
    h, ts = assembled
    Ts = [frontend.num_frames_host(n, dict(tc.TINY, DCbin=1)) for n in ts.lengths]
    idx = [np.random.RandomState(60 + k).choice(T, size=tc.R, replace=False) + 1 for k, T in enumerate(Ts)]
    idx[0][0] = Ts[0]  # the 1-based upper edge
    idx[0][1:] = np.arange(1, tc.R)
    info = {}
    ref = run_basis_train_assembled_batch(ts, tc.R, tc.P_STOP, DC_bin=1, sample_idx=idx, h0=h0, precision=mode, info=info)
    H0 = pack([tc.host_h0(T) for T in Ts]) if h0 == "host" else None
    out = shim(5, "train_signals", h, pack(idx), float(tc.R), H0, prec(tc.P_STOP, mode), mel_table(tc.TINY), 1.0, None)
    check_train(out, ref, info, [tc.R] * 7, Ts, tc.P_STOP)


def test_train_on_assembled_signals_atoms_and_settings_per_problem(shim, gpu_ctx, assembled):
    from se_snmf_nat_amd import frontend, run_basis_train_assembled_batch
    h, ts = assembled
    atoms = brc.RANKS + [4]
    Ts = [frontend.num_frames_host(n, dict(tc.TINY, DCbin=1)) for n in ts.lengths]
    idx = [np.random.RandomState(60 + k).choice(T, size=a, replace=False) + 1 for k, (T, a) in enumerate(zip(Ts, atoms))]
    st = [dict(m, conv_eps=e, max_iter=mi) for m, e, mi in zip(bsc.MODES + (dict(cf="kl", sparsity=1.0),), bsc.CONV_EPS + (0.0,), bsc.MAX_ITER_NO_CC + (4,))]
    info = {}
    ref = run_basis_train_assembled_batch(ts, atoms, tc.P_STOP, DC_bin=1, sample_idx=idx, h0="host", precision="fp64", info=info, settings=st)
    H0 = pack([tc.host_h0(T, n_ex=a) for T, a in zip(Ts, atoms)])
    out = shim(5, "train_signals", h, pack(idx), col(atoms), H0, prec(tc.P_STOP, "fp64"), mel_table(tc.TINY), 1.0, settings_matrix(resolved(st, tc.P_STOP)))
    check_train(out, ref, info, atoms, Ts, tc.P_STOP)


def test_sizes_the_handle_fixes_are_refused(shim, assembled):
    from se_snmf_nat_amd import frontend
    h, ts = assembled
    Ts = [frontend.num_frames_host(n, dict(tc.TINY, DCbin=1)) for n in ts.lengths]
    idx = pack([np.arange(1, tc.R + 1)] * 7)
    H0 = pack([tc.host_h0(T) for T in Ts])
    good = ("train_signals", h, idx, float(tc.R), H0, tc.P_STOP, mel_table(tc.TINY), 1.0, None)
    beyond = idx.copy()
    beyond[tc.R * 4] = Ts[4] + 1
    for what, i, v in (("H0 short", 4, short(H0)), ("H0 long", 4, long(H0)), ("sample_idx short", 2, short(idx)), ("sample_idx long", 2, long(idx)),
                       ("sample_idx = T_k + 1", 2, beyond), ("n_atoms of another length", 3, col([tc.R] * 6)),
                       ("settings of another length", 8, np.ones((6, 4)))):
        with pytest.raises(MexError) as e:
            shim(5, *(good[:i] + (v,) + good[i + 1:]))
        assert e.value.id == "snmf:dim", (what, e.value.id, e.value.msg)
    with pytest.raises(MexError) as e:
        shim(5, *(good[:5] + (dict(tc.P_STOP, snmf_precision="fp32"),) + good[6:8] + (np.ones((7, 4)),)))
    assert e.value.id == "snmf:unsupported"
    assert shim.live_arrays() == 0


def test_a_destroyed_handle_is_refused_and_unload_releases_a_live_one(tmp_path, gpu_ctx):
    """On a shim of its own: 'signals_destroy', then every command on the dead handle is snmf:handle; a second handle is left
    live and unload() -- what `clear mex` does -- destroys it and then the context, without a host error."""
    m = mexhost.Mex(mexhost.build_shim(NAME, tmp_path))
    rs = np.random.RandomState(3)
    clips = [rs.randn(300) * 2000, rs.randn(240) * 2000]
    args = ("assemble", pack(clips), col([300, 240]), col([1, 1]), col([0, 0]), None, dict(fs=1000, train_seq_len_max=1000, train_file_len_max=250))
    h1 = m(1, *args)[0]
    h2 = m(1, *args)[0]
    assert (h1[0, 0], h2[0, 0]) == (1.0, 2.0) and m.has_exit_fcn() and m.lock_count() == 1
    assert m(2, "signals_info", h1)[0][:, 0].tolist() == [250.0, 240.0]
    m(0, "signals_destroy", h1)
    for call in (("signals_info", h1), ("signals_get", h1, 1.0), ("signals_destroy", h1),
                 ("train_signals", h1, pack([np.arange(1, 7)] * 2), 6.0, None, tc.P_STOP, mel_table(tc.TINY), 1.0, None)):
        with pytest.raises(MexError) as e:
            m(1 if call[0] != "signals_destroy" else 0, *call)
        assert e.value.id == "snmf:handle", call[0]
    assert eq(m(1, "signals_get", h2, 2.0)[0][:, 0], m(1, "signals_get", h2, 2.0)[0][:, 0])
    assert m.live_arrays() == 0
    m.unload()  # h2 is still live
    assert m.live_arrays() == 0
