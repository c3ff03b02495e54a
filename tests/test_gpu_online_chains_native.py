"""The chain driver behind the C ABI (snmf_online_batch_run_chains_f32 / _f64, OnlineBatchSeparator.run_chains) and the MEX
shim integration/snmf_online_batch_mex.cpp on the device.

The yardstick is the Python driver ntf_sep_event_rt_chains (se_snmf_nat_amd/online.py), which tests/test_online_batch*.py
hold to the single-stream separator and the oracle: every file's int16 signal, float signal and final dictionary must
equal it BIT FOR BIT, in fp32 DFT, fp32 Mel and fp64, for every number of slots and every chunk length.  The shim is held
to the binding in the same way (int16 exactly, doubles as bits), through 'chains' and through its commands driven by hand.

Geometry: the one tests/test_gpu_mex.py uses for snmf_online_mex (its helpers are imported): fftlength 64, F = 33, hop 16,
the dictionaries of its online_setup() (R_x = 8, R_d = 12), Mel 12 x 33.  Corpus: 2 slots; 5 chains of 1 to 3 files and
an empty one; files of 3 to 40 hops, one of them 5 samples past a hop; R_a = 3, m_a = 4, overlap_m_a = 0.5 (a dictionary
update at every second triggered frame), init_N_len = 2, so that every chain adapts within its first file.  Every test
that completes a run asserts it from the streams' traces (adapt_iters > 0) and from every chain's first final dictionary,
which differs from its start: a corpus that never adapts would pass vacuously.

All of this fails on a tree without the feature: the symbols and the shim do not exist there."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import mexhost
from mexhost import MexError
from test_gpu_mex import GOLD, binding_settings, online_mex_p, online_setup, same_bits

pytestmark = pytest.mark.gpu

HOP, F, R_X, R_D, N1 = 16, 33, 8, 12, 12
R_A, M_A = 3, 4
# files per chain, in hops (+ samples): 5 chains of 1 to 3 files, one empty chain, 3 to 40 hops, one length off the hop
CORPUS = [[(40, 0), (3, 0), (21, 0)], [], [(36, 0)], [(38, 0), (12, 5)], [(33, 0), (9, 0), (27, 0)], [(30, 0), (40, 0)]]
MODES = ("fp32-DFT", "fp32-Mel", "fp64")


@functools.lru_cache(maxsize=None)
def setup(mode):
    """(chains, B_DFT_x, per-chain B_DFT_d, p, per-chain H0, per-chain Ad_blk0, B_Mel_x, per-chain B_Mel_d, precision)"""
    from se_snmf_nat_amd import frontend as fe
    Bx, Bd, p, _, _, _ = online_setup()
    assert Bx.shape == (F, R_X) and Bd.shape == (F, R_D) and p["frameshift"] == HOP
    p = dict(binding_settings(p), R_a=R_A, m_a=M_A, overlap_m_a=0.5, init_N_len=2)
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    chains, at = [], 0
    for c in CORPUS:
        files = []
        for hops, extra in c:
            n = hops * HOP + extra
            files.append(s[at:at + n].copy())
            at += n + 37
        chains.append(files)
    assert at < s.size
    nc = len(chains)
    rs = np.random.RandomState(11)
    Bds = [np.asfortranarray(Bd * (1 + 0.2 * rs.random_sample(Bd.shape))) for _ in range(nc)]
    H0s = [rs.random_sample(R_X + R_D) for _ in range(nc)]
    Ads = [rs.random_sample((R_A, M_A)) for _ in range(nc)]
    BMx = BMds = None
    if mode == "fp32-Mel":
        p = dict(p, B_sep_mode="Mel", MelConv=1, F_order=N1)
        melmat = np.ascontiguousarray(fe.mel_matrix(p["fs"], N1, 64, 1.0, p["fs"] / 2).T)
        norm = lambda B: B / np.sqrt((B ** 2).sum(0)) + 1e-9  # noqa: E731
        BMx = np.asfortranarray(norm(melmat @ Bx))
        BMds = [np.asfortranarray(norm(melmat @ B)) for B in Bds]
    return chains, Bx, Bds, p, H0s, Ads, BMx, BMds, ("fp64" if mode == "fp64" else "fp32")


def make_sep(mode, S, ctx, **kw):
    """A batch of S slots; what it is created with does not matter to a run over chains (every used slot is restarted)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    return OnlineBatchSeparator(Bx, Bds[0], p, S, ctx=ctx, B_Mel_x=BMx, B_Mel_d=BMds[0] if BMds else None, precision=prec, **kw)


def run(sep, mode, chunk_hops=None, masters=False):
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    return sep.run_chains(chains, Bds, H0=H0s, Ad_blk0=Ads, B_Mel_d=BMds, chunk_hops=chunk_hops, masters=masters)


_REF = {}


def reference(mode, ctx):
    """ntf_sep_event_rt_chains on the corpus, computed once per mode and never changed."""
    if mode not in _REF:
        from se_snmf_nat_amd.online import ntf_sep_event_rt_chains
        chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
        _REF[mode] = ntf_sep_event_rt_chains(chains, Bx, Bds, p, n_streams=2, H0=H0s, Ad_blk0=Ads, ctx=ctx, B_Mel_x=BMx, B_Mel_d=BMds,
                                             precision=prec)
    return _REF[mode]


def assert_same_results(got, want, what):
    assert [len(c) for c in got] == [len(c) for c in want] == [len(c) for c in CORPUS], what
    for c, (gc, wc) in enumerate(zip(got, want)):
        for i, (g, w) in enumerate(zip(gc, wc)):
            tag = f"{what}: chain {c} file {i}"
            assert g[0].dtype == w[0].dtype == np.int16 and np.array_equal(g[0], w[0]), tag + " int16"
            same_bits(g[1], w[1], tag + " float")
            same_bits(g[2], w[2], tag + " dictionary")


def assert_adapted(sep, results, mode, S):
    """The corpus adapts: from the traces of the slots' last files, and from every chain's first final dictionary."""
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    used = min(S, sum(1 for c in CORPUS if c))
    iters = [sum(t["adapt_iters"] for t in sep.trace(k)) for k in range(used)]
    print(f"{mode} S={S}: adapt_iters of the slots' last files {iters}")
    assert all(n > 0 for n in iters), iters
    start = BMds if mode == "fp32-Mel" else Bds
    for c, res in enumerate(results):
        if res:
            first = np.asarray(start[c], dtype=np.float64 if prec == "fp64" else np.float32).astype(np.float64)
            assert res[0][2].shape == first.shape and not np.array_equal(res[0][2], first), f"chain {c} did not adapt within its first file"


# ---- bit equality with the Python driver -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("mode", MODES)
def test_run_chains_equals_the_python_driver(gpu_ctx, mode, S):
    want = reference(mode, gpu_ctx)
    sep = make_sep(mode, S, gpu_ctx)
    try:
        for chunk_hops in (1, 7, None):
            got = run(sep, mode, chunk_hops)  # (the same handle again and again: every run leaves it idle)
            assert_same_results(got, want, f"{mode} S={S} chunk_hops={chunk_hops}")
            assert_adapted(sep, got, mode, S)
            for c, files in zip(got, setup(mode)[0]):
                for (x16, xf, B), x in zip(c, files):
                    assert len(x16) == len(xf) <= sep.out_capacity(len(x))
    finally:
        sep.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_chunk_far_longer_than_any_file_is_whole_files_per_call(gpu_ctx, mode):
    """chunk_hops = 0 is the default; 10^6 and INT32_MAX mean whole files per call: the same bits, and no buffer of that size."""
    want = reference(mode, gpu_ctx)
    sep = make_sep(mode, 2, gpu_ctx)
    try:
        for chunk_hops in (0, 10 ** 6, 2 ** 31 - 1):
            got = run(sep, mode, chunk_hops)
            assert_same_results(got, want, f"{mode} chunk_hops={chunk_hops}")
            assert_adapted(sep, got, mode, 2)
    finally:
        sep.close()


@pytest.mark.parametrize("mode", MODES)
def test_default_draws_are_the_python_drivers(gpu_ctx, mode):
    """H0 / Ad_blk0 left out: RandomState(random_seed + c) per chain, as ntf_sep_event_rt_chains draws them."""
    from se_snmf_nat_amd.online import ntf_sep_event_rt_chains
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    want = ntf_sep_event_rt_chains(chains, Bx, Bds, p, n_streams=2, ctx=gpu_ctx, B_Mel_x=BMx, B_Mel_d=BMds, precision=prec)
    sep = make_sep(mode, 2, gpu_ctx)
    try:
        got = sep.run_chains(chains, Bds, B_Mel_d=BMds)
        assert_adapted(sep, got, mode, 2)  # (under these draws too)
    finally:
        sep.close()
    assert_same_results(got, want, f"{mode} default draws")
    assert not np.array_equal(got[0][0][1], reference(mode, gpu_ctx)[0][0][1]), "the draws must matter"


@pytest.mark.parametrize("mode", MODES)
def test_a_second_run_on_the_handle_equals_the_first_on_a_fresh_one(gpu_ctx, mode):
    sep = make_sep(mode, 2, gpu_ctx)
    try:
        run(sep, mode)
        second = run(sep, mode)
        assert_adapted(sep, second, mode, 2)
    finally:
        sep.close()
    fresh = make_sep(mode, 2, gpu_ctx)
    try:
        first = run(fresh, mode)
        assert_adapted(fresh, first, mode, 2)
    finally:
        fresh.close()
    assert_same_results(second, first, f"{mode} reuse")
    assert_same_results(first, reference(mode, gpu_ctx), f"{mode} fresh")


def test_masters_are_the_fp64_dictionaries(gpu_ctx):
    """masters=True: the fp64 masters; the default on an fp32 batch is their fp32 image, as basis(k) of the Python driver."""
    sep = make_sep("fp32-DFT", 2, gpu_ctx)
    try:
        m = run(sep, "fp32-DFT", masters=True)
        assert_adapted(sep, m, "fp32-DFT", 2)
        d = run(sep, "fp32-DFT")
        assert_adapted(sep, d, "fp32-DFT", 2)
    finally:
        sep.close()
    rounded = [[(a, b, B.astype(np.float32).astype(np.float64)) for a, b, B in c] for c in m]
    assert_same_results(rounded, d, "masters rounded")
    assert any(not np.array_equal(x[2], y[2]) for cm, cd in zip(m, d) for x, y in zip(cm, cd)), "an adapted fp64 master is no fp32 value"


# ---- status codes ----------------------------------------------------------------------------------------------------------------
def c_run(sep, files, Bd, H0, Ad, n_out_fill=99):
    """One chain of `files` through the C entry itself: (status, n_out)."""
    from se_snmf_nat_amd import _lib
    lib = _lib.load()
    dt = sep._dt
    xs = [np.ascontiguousarray(x, dtype=dt) for x in files]
    nf = len(xs)
    P = C.c_void_p * nf
    n_files = np.array([nf], np.int32)
    ns = np.array([x.size for x in xs], np.int64)
    caps = np.array([sep.out_capacity(x.size) for x in xs], np.int64)
    o16 = [np.zeros(c, np.int16) for c in caps]
    n_out = np.full(nf, n_out_fill, np.int64)
    Bd = np.asfortranarray(Bd, dtype=np.float64)
    H0, Ad = np.ascontiguousarray(H0, dtype=dt), np.ascontiguousarray(np.asarray(Ad, dtype=dt).ravel(order="F"))
    fn = lib.snmf_online_batch_run_chains_f64 if sep.precision == "fp64" else lib.snmf_online_batch_run_chains_f32
    st = fn(sep._h, 1, n_files.ctypes.data, P(*[x.ctypes.data for x in xs]), ns.ctypes.data, Bd.ctypes.data, None, H0.ctypes.data,
            Ad.ctypes.data, 0, P(*[a.ctypes.data for a in o16]), None, caps.ctypes.data, n_out.ctypes.data, None)
    return st, n_out, [a[:max(0, m)] for a, m in zip(o16, n_out)]


@pytest.mark.parametrize("mode", ["fp32-DFT", "fp64"])
def test_a_stream_in_the_middle_of_a_recording_is_refused(gpu_ctx, mode):
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    files = chains[0][:2]
    sep = make_sep(mode, 2, gpu_ctx)
    try:
        st, n_out, want = c_run(sep, files, Bds[0], H0s[0], Ads[0])
        assert st == 0 and (n_out > 0).all()
        adapted = lambda: sum(t["adapt_iters"] for t in sep.trace(0))  # noqa: E731  (one chain: slot 0, its last file)
        assert adapted() > 0
        dt = sep._dt
        sep.process([np.zeros(0, dt), chains[2][0][:5 * HOP]], flush=False)  # stream 1 is now in the middle of a recording
        st, n_out, _ = c_run(sep, files, Bds[0], H0s[0], Ads[0])
        assert st == 7 and not n_out.any(), (st, n_out)  # SNMF_ERR_STATE, every n_out zeroed
        from se_snmf_nat_amd import SnmfError
        with pytest.raises(SnmfError) as e:
            run(sep, mode)
        assert e.value.status == 7
        sep.process([np.zeros(0, dt), np.zeros(0, dt)], flush=[False, True])  # flushed: the handle is usable again
        st, n_out, got = c_run(sep, files, Bds[0], H0s[0], Ads[0])
        assert st == 0 and adapted() > 0
        for g, w in zip(got, want):
            assert np.array_equal(g, w), "the same bits after the refusal"
    finally:
        sep.close()


def test_the_entry_of_the_other_precision_is_refused(gpu_ctx):
    from se_snmf_nat_amd import _lib
    lib = _lib.load()
    for mode, other in (("fp32-DFT", lib.snmf_online_batch_run_chains_f64), ("fp64", lib.snmf_online_batch_run_chains_f32)):
        chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
        sep = make_sep(mode, 2, gpu_ctx)
        try:
            x = np.zeros(4 * HOP, np.float64)  # (8 bytes per sample: enough for either entry; it is never read)
            P = C.c_void_p * 1
            n_files, ns, n_out = np.array([1], np.int32), np.array([x.size], np.int64), np.array([5], np.int64)
            Bd, H0, Ad = np.asfortranarray(Bds[0]), np.zeros(R_X + R_D), np.zeros(R_A * M_A)
            st = other(sep._h, 1, n_files.ctypes.data, P(x.ctypes.data), ns.ctypes.data, Bd.ctypes.data, None, H0.ctypes.data, Ad.ctypes.data, 0,
                       None, None, None, n_out.ctypes.data, None)
            assert st == 7 and n_out[0] == 0
            got = run(sep, mode)
            assert_same_results(got, reference(mode, gpu_ctx), f"{mode} after the refusal")
            assert_adapted(sep, got, mode, 2)
        finally:
            sep.close()


def test_a_batch_with_settings_per_stream_is_unsupported_and_stays_usable(gpu_ctx):
    from se_snmf_nat_amd import SnmfError
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup("fp64")
    sep = make_sep("fp64", 2, gpu_ctx, settings=[{}, {"sparsity": 3.0}])
    try:
        with pytest.raises(SnmfError) as e:
            run(sep, "fp64")
        assert e.value.status == 8  # SNMF_ERR_UNSUPPORTED
        outs = sep.process([chains[0][0], chains[2][0]], flush=True)
        assert all(len(o["x_tilde"]) > 0 for o in outs)
    finally:
        sep.close()


def test_out_capacity_is_the_python_rule(gpu_ctx):
    sep = make_sep("fp32-DFT", 2, gpu_ctx)
    try:
        for n in (0, 1, HOP - 1, HOP, 10 * HOP + 3):
            assert sep.out_capacity(n) == (n // sep.hop + sep.delay + 3) * sep.hop
        got = run(sep, "fp32-DFT")
        assert_adapted(sep, got, "fp32-DFT", 2)
    finally:
        sep.close()
    chains = setup("fp32-DFT")[0]
    for c, files in zip(got, chains):
        for (x16, xf, B), x in zip(c, files):
            assert 0 < len(x16) <= (len(x) // HOP + sep.delay + 3) * HOP


# ---- the MEX shim ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory, lib):
    m = mexhost.Mex(mexhost.build_shim("snmf_online_batch_mex", tmp_path_factory.mktemp("batch_mex")))
    yield m
    m.unload()


def mex_create(shim, mode, S, Bd, H0, Ad, BMd=None):
    from se_snmf_nat_amd import frontend as fe
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    mp = online_mex_p(p, **({"precision": "fp64"} if prec == "fp64" else {}))
    (h,) = shim(1, "create", Bx, Bd, H0, Ad, mp, float(S))
    if mode == "fp32-Mel":
        melmat = np.ascontiguousarray(fe.mel_matrix(p["fs"], N1, 64, 1.0, p["fs"] / 2).T)
        shim(0, "set_mel", h, melmat, BMx, BMds[0] if BMd is None else BMd, 1.0)
    return h


@pytest.mark.parametrize("mode", MODES)
def test_mex_chains_equals_run_chains(shim, gpu_ctx, mode):
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    sep = make_sep(mode, 2, gpu_ctx)
    try:
        want = run(sep, mode, masters=True)
        assert_adapted(sep, want, mode, 2)
    finally:
        sep.close()
    files = [x for c in chains for x in c]
    args = [np.concatenate(files), [float(x.size) for x in files], [float(len(c)) for c in chains], np.hstack(Bds),
            np.stack(H0s, axis=1), np.hstack(Ads)]
    mel = [np.hstack(BMds)] if mode == "fp32-Mel" else []
    h = mex_create(shim, mode, 2, Bds[0], H0s[0].reshape(-1, 1), Ads[0])
    for chunk_hops in (0.0, 5.0, 2147483647.0):
        x, n_out, B_out, xf = shim(4, "chains", h, *args, chunk_hops, *mel)
        assert x.dtype == np.int16 and x.shape == xf.shape and x.shape[1] == 1 and n_out.shape == (len(files), 1)
        rows = N1 if mode == "fp32-Mel" else F
        assert B_out.shape == (rows, R_D * len(files)) and B_out.dtype == np.float64
        flat = [t for c in want for t in c]
        assert [int(v) for v in n_out[:, 0]] == [len(t[0]) for t in flat]
        assert np.array_equal(x[:, 0], np.concatenate([t[0] for t in flat])), "int16"
        same_bits(xf[:, 0], np.concatenate([t[1] for t in flat]), "float signal")
        same_bits(B_out, np.asfortranarray(np.hstack([t[2] for t in flat])), "dictionaries")
    # sizes the handle fixes, refused before the library is called
    for bad, what in (([args[0], args[1], args[2], args[3][:, :-1], args[4], args[5], 0.0, *mel], "B_DFT_d columns"),
                      ([args[0], args[1], args[2], args[3], args[4][:-1], args[5], 0.0, *mel], "H0 rows"),
                      ([args[0], args[1], args[2], args[3], args[4], args[5][:, 1:], 0.0, *mel], "Ad_blk0 columns")):
        with pytest.raises(MexError) as e:
            shim(3, "chains", h, *bad)
        assert e.value.id == "snmf:dim", what
    with pytest.raises(MexError) as e:  # the Mel dictionaries go with a Mel batch, and only with one
        shim(3, "chains", h, *args, 0.0, *([] if mel else [np.hstack(Bds)[:N1]]))
    assert e.value.id == "snmf:usage"
    shim(0, "destroy", h)
    with pytest.raises(MexError) as e:
        shim(3, "chains", h, *args, 0.0, *mel)
    assert e.value.id == "snmf:handle"


@pytest.mark.parametrize("mode", MODES)
def test_mex_by_hand_equals_the_binding(shim, gpu_ctx, mode):
    """create / process / restart / basis / mel_basis driven by hand against the same sequence on OnlineBatchSeparator."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    chains, Bx, Bds, p, H0s, Ads, BMx, BMds, prec = setup(mode)
    is_mel = mode == "fp32-Mel"
    a, b, c, d = chains[0][0], chains[2][0], chains[3][1], chains[4][2]  # 40, 36, 12 + 5 samples, 27 hops
    sep = OnlineBatchSeparator(Bx, Bds[:2], p, 2, H0=H0s[:2], Ad_blk0=Ads[:2], ctx=gpu_ctx, B_Mel_x=BMx, B_Mel_d=BMds[:2] if is_mel else None,
                               precision=prec)
    master = (lambda k: sep.mel_basis_f64(k)) if is_mel else (lambda k: sep.basis_f64(k))
    h = None
    try:
        # the binding
        want = []
        want.append(sep.process([a[:20 * HOP], b], flush=[False, True]))
        want.append(sep.process([a[20 * HOP:], b[:0]], flush=[True, False]))
        B1 = [master(0), master(1), sep.basis_f64(0)]
        sep.restart([1])  # carry
        sep.restart([0], Bds[3], H0s[3], Ads[3], B_Mel_d=BMds[3] if is_mel else None)
        want.append(sep.process([c, d], flush=True))
        B2 = [master(0), master(1)]
        assert any(t["adapt_iters"] > 0 for k in (0, 1) for t in sep.trace(k)), "the sequence must adapt"
        # the shim
        h = mex_create(shim, mode, 2, np.hstack(Bds[:2]), np.stack(H0s[:2], axis=1), np.hstack(Ads[:2]), np.hstack(BMds[:2]) if is_mel else None)
        got = []
        got.append(shim(3, "process", h, np.concatenate([a[:20 * HOP], b]), [20.0 * HOP, float(b.size)], [0.0, 1.0]))
        got.append(shim(3, "process", h, a[20 * HOP:], [float(a.size - 20 * HOP), 0.0], [1.0, 0.0]))
        basis = "mel_basis" if is_mel else "basis"
        G1 = [shim(1, basis, h, 1.0)[0], shim(1, basis, h, 2.0)[0], shim(1, "basis", h, 1.0)[0]]
        shim(0, "restart", h, [2.0], None, None, None)
        shim(0, "restart", h, [1.0], Bds[3], H0s[3].reshape(-1, 1), Ads[3], *([BMds[3]] if is_mel else []))
        got.append(shim(3, "process", h, np.concatenate([c, d]), [float(c.size), float(d.size)], [1.0, 1.0]))
        G2 = [shim(1, basis, h, 1.0)[0], shim(1, basis, h, 2.0)[0]]
        for step, ((x, n_out, xf), outs) in enumerate(zip(got, want)):
            assert [int(v) for v in n_out[:, 0]] == [len(o["x_tilde"]) for o in outs], step
            assert x.dtype == np.int16 and np.array_equal(x[:, 0], np.concatenate([o["x_tilde"] for o in outs])), f"call {step}: int16"
            same_bits(xf[:, 0], np.concatenate([o["x_tilde_f"] for o in outs]).astype(np.float64), f"call {step}: float signal")
        for g, w in zip(G1 + G2, B1 + B2):
            same_bits(g, w, "fp64 master")
        shim(0, "destroy", float(h[0, 0]) + 0.5)  # no such handle: nothing is destroyed
        same_bits(shim(1, basis, h, 1.0)[0], G2[0], "the handle after a destroy of h + 0.5")
        # sizes the handle fixes
        for args, what in ((("process", h, a, [float(a.size)], [1.0]), "n of one entry on two streams"),
                           (("restart", h, [3.0], None, None, None), "slot 3 of 2"),
                           (("restart", h, [1.0, 1.0], None, None, None), "a slot twice"),
                           (("restart", h, [1.0], Bds[0][:, :-1], None, None), "B_DFT_d columns"),
                           (("restart", h, [1.0, 2.0], None, H0s[0].reshape(-1, 1), None), "one H0 for two slots"),
                           (("basis", h, 3.0), "stream 3 of 2"), (("basis", h, 0.0), "stream 0")):
            with pytest.raises(MexError) as e:
                shim(3 if args[0] == "process" else 1, *args)
            assert e.value.id == "snmf:dim", what
        if not is_mel:
            for args in (("mel_basis", h, 1.0), ("restart", h, [1.0], None, None, None, BMx)):
                with pytest.raises(MexError) as e:
                    shim(1, *args)
                assert e.value.id == "snmf:usage"
    finally:
        sep.close()
        if h is not None:
            shim(0, "destroy", h)
