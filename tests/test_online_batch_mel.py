"""Mel mode of the batched online separator (snmf_online_batch_set_mel / _restart_mel / _get_mel_basis_* in
include/snmf.h; OnlineBatchSeparator(..., B_Mel_x, B_Mel_d), ntf_sep_event_rt_batch / _chains in Mel mode).  With
B_sep_mode = 'Mel' the frame solve and the adaptation run on F_order Mel bands (src/bnmf_sep_event_RT_IS16.m:106-120,
:165-171, :205-211, :298-318), for every stream in shared launches.  Every stream must match its own fp64 oracle run
(oracle/online_oracle.py, mel=...) with the bounds of tests/test_online.py's Mel test, and its bits must depend neither
on its batch-mates nor on how it is fed or restarted."""
import os

import numpy as np
import pytest

from oracle.online_oracle import default_params, ntf_sep_event_rt
from test_online_batch import REL_OUT, _decisions, _fixture, _settings, _streams
from test_online_batch_restart import REL_OUT_CHAIN, _f32, _noisy, _uneven_chains

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N1 = 64


def _melmat(p, n1=N1):
    from oracle.frontend_oracle import mel_matrix
    return mel_matrix(p["fs"], n1, p["fftlength"], 1.0, p["fs"] / 2).T


def _mel_dict(melmat, B):
    """The stored form of a Mel dictionary (run_basis_train.m:115-116): melmat * B, unit columns, + 1e-9; fp32 values."""
    BM = melmat @ B
    return _f32(BM / np.sqrt((BM ** 2).sum(0)) + 1e-9)


def _mel_params(melconv=1, **kw):
    return dict(default_params(), B_sep_mode="Mel", MelConv=melconv, F_order=N1, **kw)


def _mel_streams(n_hops, S=5, seed=11, p=None):
    """test_online_batch._streams plus each stream's own start B_Mel_d (from its own B_DFT_d) and the shared B_Mel_x."""
    pcms, Bx, Bds, H0s, Ads = _streams(n_hops, S=S, seed=seed)
    mm = _melmat(p or _mel_params())
    return pcms, Bx, Bds, H0s, Ads, _mel_dict(mm, Bx), [_mel_dict(mm, B) for B in Bds]


def _run(ctx, pcms, Bx, Bds, p, H0s, Ads, BMx, BMds, class_outputs=False, feed=None):
    """Like test_online_batch._run_batch, Mel mode: per stream (outputs, trace, B_Mel_d fp64 master, B_DFT_d fp64)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    S = len(pcms)
    sep = OnlineBatchSeparator(Bx, Bds, _settings(p), S, H0=H0s, Ad_blk0=Ads, ctx=ctx, class_outputs=class_outputs, B_Mel_x=BMx,
                               B_Mel_d=BMds)
    keys = ["x_tilde", "x_tilde_f"] + (["x_hat", "d_hat"] if class_outputs else [])
    acc = [{k: [] for k in keys} for _ in range(S)]
    for chunk_list, flush in (feed or [(pcms, True)]):
        for a, o in zip(acc, sep.process(chunk_list, flush=flush)):
            for k in keys:
                a[k].append(o[k])
    res = [({key: np.concatenate(acc[k][key]) for key in keys}, sep.trace(k), sep.mel_basis_f64(k), sep.basis_f64(k)) for k in range(S)]
    assert all(np.array_equal(sep.mel_basis(k), res[k][2].astype(np.float32).astype(np.float64)) for k in range(S))
    sep.close()
    return res


def _same(a, b):
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]), key
    assert a[1] == b[1]
    assert all(np.array_equal(u, v) for u, v in zip(a[2:], b[2:]))


def _oracle(x, Bx, Bd, p, H0, Ad, BMx, BMd, cls=False):
    return ntf_sep_event_rt(x, Bx, Bd, p, H0, Ad, return_trace=True, class_outputs=cls,
                            mel=dict(B_Mel_x=BMx, B_Mel_d=BMd, melmat=_melmat(p, p["F_order"])))


def _check(res, ref, cls=False, tol=REL_OUT):
    out, trd, BMn = res[:3]
    o16, of, BMo, tr = ref[:4]
    assert _decisions(trd) == _decisions(tr)
    pairs = [(out["x_tilde_f"], of)] + ([(out["x_hat"], ref[4]), (out["d_hat"], ref[5])] if cls else [])
    for dev, rf in pairs:
        assert len(dev) == len(rf) and np.isfinite(dev).all()
        assert np.linalg.norm(dev - rf) / np.linalg.norm(rf) < tol
    assert np.abs(out["x_tilde"].astype(int) - o16.astype(int)).max(initial=0) <= 1
    assert np.linalg.norm(BMn - BMo) / np.linalg.norm(BMo) < 1e-3


# ---------------------------------------------------------------- CPU ----------------------------------------------
def test_mel_argument_checks_raise_before_any_device_call(monkeypatch):
    """Mel shapes, list lengths and F_order are checked in Python before the library is loaded or a context is made;
    Mel mode without the Mel dictionaries stays SNMF_ERR_UNSUPPORTED."""
    from se_snmf_nat_amd import _lib, online
    from se_snmf_nat_amd.online import OnlineBatchSeparator, ntf_sep_event_rt_chains

    def no_device(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(online, "default_context", no_device)
    _, Bx, Bd = _fixture()
    p = _settings(_mel_params())
    BMx, BMd = np.ones((N1, 100)), np.ones((N1, 100))
    for kw in (dict(B_Mel_x=np.ones((N1 - 1, 100))),
               dict(B_Mel_x=np.ones((N1, 99))),
               dict(B_Mel_d=[BMd, BMd, BMd]),
               dict(B_Mel_d=np.ones((N1, 100, 3))),
               dict(B_Mel_d=[BMd, np.ones((N1, 50))]),
               dict(p=dict(p, F_order=514), B_Mel_x=np.ones((514, 100)), B_Mel_d=np.ones((514, 100))),
               dict(p=dict(p, F_order=1), B_Mel_x=np.ones((1, 100)), B_Mel_d=np.ones((1, 100)))):
        args = dict(p=p, B_Mel_x=BMx, B_Mel_d=BMd)
        args.update(kw)
        with pytest.raises(_lib.SnmfError) as e:
            OnlineBatchSeparator(Bx, Bd, args.pop("p"), 2, **args)
        assert e.value.status == 1, kw  # SNMF_ERR_INVALID
    for kw in (dict(), dict(B_Mel_x=BMx), dict(B_Mel_d=BMd)):
        with pytest.raises(_lib.SnmfError) as e:
            OnlineBatchSeparator(Bx, Bd, p, 2, **kw)
        assert e.value.status == 8  # SNMF_ERR_UNSUPPORTED
    with pytest.raises(_lib.SnmfError) as e:
        ntf_sep_event_rt_chains([[np.zeros(1600)]], Bx, Bd, p, B_Mel_x=BMx)
    assert e.value.status == 8
    with pytest.raises(_lib.SnmfError) as e:
        ntf_sep_event_rt_chains([[np.zeros(1600)], [np.zeros(1600)]], Bx, Bd, p, B_Mel_x=BMx, B_Mel_d=[BMd, BMd[:, :50]])
    assert e.value.status == 1


# ---------------------------------------------------------------- GPU ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("melconv,cls", [(1, False), (0, False), (1, True)], ids=["MelConv1", "MelConv0-coupled", "MelConv1-class"])
def test_mel_heterogeneous_batch_matches_the_oracle_per_stream(gpu_ctx, melconv, cls):
    """Five streams that differ in signal, length, H0 / Ad_blk0 and start B_Mel_d / B_DFT_d, adaptation on: each stream
    against its own oracle run, and its B_DFT_d comes back as it started (Mel mode never adapts it)."""
    p = _mel_params(melconv)
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(40, p=p)
    res = _run(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, BMx, BMds, class_outputs=cls)
    for k in range(len(pcms)):
        _check(res[k], _oracle(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], BMx, BMds[k], cls=cls), cls=cls)
        assert np.array_equal(res[k][3], _f32(Bds[k]))
    assert sum(t["solved"] for t in res[0][1]) > 5


def _imcra():
    """settings/bak_IS16_results/initial_setting_IMCRA.m:47-113 on the shipped dictionaries (R_x = R_d = 50 columns of
    B_DFT_sub / B_Mel_sub: speech from the TIMIT file, noise from the CHiME3 one)."""
    from se_snmf_nat_amd.train import load_basis_mat
    sp = load_basis_mat(os.path.join(GOLD, "ref_basis", "R_100_Clean_train_TIMIT_test.mat"))
    nz = load_basis_mat(os.path.join(GOLD, "ref_basis", "R_100_CHiME3_bgn_ch6.mat"))
    p = dict(default_params(), B_sep_mode="Mel", MelConv=1, F_order=64, adapt_train_N=0, init_N_len=10, m_a=40, overlap_m_a=0.5,
             blk_sparse=0, P_len_k=50, P_len_l=3, max_iter=25, conv_eps=1e-3, sparsity=5, cf="kl", ENHANCE_METHOD="MMSE",
             DCbin=10, DCbin_back=10)
    f = lambda m, key: _f32(np.asarray(m[key], dtype=np.float64)[:, :50])  # noqa: E731
    return p, f(sp, "B_DFT_sub"), f(nz, "B_DFT_sub"), f(sp, "B_Mel_sub"), f(nz, "B_Mel_sub")


@pytest.mark.gpu
def test_mel_imcra_setting_matches_the_oracle_and_the_single_stream_separator(gpu_ctx):
    """The reference's Mel configuration (MelConv = 1, F_order = 64, R_x = R_d = 50, adaptation off, max_iter = 25) on the
    shipped B_Mel_sub / B_DFT_sub: every stream against the oracle, and against OnlineSeparator in Mel mode with equal
    decisions and x_tilde_f within 1e-6 (test_online_batch.py's batch-vs-single-stream bound: another reduction order)."""
    from se_snmf_nat_amd.online import OnlineSeparator
    p, Bx, Bd, BMx, BMd = _imcra()
    pcms, _, _, _, _ = _streams(40, S=4, seed=13)
    rs = np.random.RandomState(14)
    H0s = [rs.random_sample(100) for _ in pcms]
    Ad0 = rs.random_sample((p["R_a"], p["m_a"]))  # (the oracle's init_buff draws it whether or not it adapts)
    res = _run(gpu_ctx, pcms, Bx, Bd, p, H0s, None, BMx, BMd)
    for k, x in enumerate(pcms):
        _check(res[k], _oracle(x, Bx, Bd, p, H0s[k], Ad0, BMx, BMd))
        sep = OnlineSeparator(Bx, Bd, _settings(p), H0=H0s[k], ctx=gpu_ctx, B_Mel_x=BMx, B_Mel_d=BMd)
        out = sep.process(x, flush=True)
        tr = sep.trace()
        sep.close()
        assert _decisions(res[k][1]) == _decisions(tr)
        a, b = res[k][0]["x_tilde_f"], out["x_tilde_f"]
        assert len(a) == len(b) and np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-6


@pytest.mark.gpu
def test_mel_bits_do_not_depend_on_the_company(gpu_ctx):
    """S = 1 vs S = 5 vs a permuted order vs S = 300 replicas, MelConv 1 with adaptation: every stream's bits identical."""
    p = _mel_params()
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(24)
    pick = lambda idx: ([pcms[i] for i in idx], Bx, [Bds[i] for i in idx], p, [H0s[i] for i in idx], [Ads[i] for i in idx], BMx,  # noqa: E731
                        [BMds[i] for i in idx])
    full = _run(gpu_ctx, *pick(range(5)))
    for k in range(5):
        _same(_run(gpu_ctx, *pick([k]))[0], full[k])
    order = [3, 1, 4, 0, 2]
    for j, r in enumerate(_run(gpu_ctx, *pick(order))):
        _same(r, full[order[j]])
    big = _run(gpu_ctx, *pick([k % 5 for k in range(300)]))
    for k in range(300):
        _same(big[k], full[k % 5])
    assert sum(t["solved"] for r in full for t in r[1]) > 0


@pytest.mark.gpu
def test_mel_bits_do_not_depend_on_how_the_streams_are_fed(gpu_ctx):
    """Uneven chunks, empty feeds and flushes in different calls give the bits of one call, MelConv 0 and 1."""
    for melconv in (1, 0):
        p = _mel_params(melconv)
        pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(30, S=3, p=p)
        whole = _run(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, BMx, BMds)
        sizes, pos, feed, rnd = [160, 1000, 57], [0, 0, 0], [], 0
        while any(pos[k] < len(pcms[k]) for k in range(3)):
            chunk = []
            for k in range(3):
                if (rnd + k) % 4 == 3:  # some streams get nothing in some calls
                    chunk.append(pcms[k][:0])
                    continue
                chunk.append(pcms[k][pos[k]:pos[k] + sizes[k]])
                pos[k] += sizes[k]
            feed.append((chunk, False))
            rnd += 1
        feed.append(([x[:0] for x in pcms], [False, True, False]))
        feed.append(([x[:0] for x in pcms], [True, False, True]))
        for a, b in zip(whole, _run(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, BMx, BMds, feed=feed)):
            _same(a, b)


def _file(sep, k, x):
    """Stream k of `sep` runs the whole recording x (the other streams get nothing)."""
    pcms, flush = [np.zeros(0)] * sep.S, [False] * sep.S
    pcms[k], flush[k] = x, True
    out = sep.process(pcms, flush)[k]
    return out, sep.trace(k), sep.mel_basis_f64(k), sep.basis_f64(k)


@pytest.mark.gpu
def test_mel_restart(gpu_ctx):
    """A restart with new dictionaries equals a fresh separator bit for bit; a carry keeps the fp64 Mel master (and
    B_DFT_d) exactly, and restarting with that master passed in explicitly gives the same bits; batch-mates fed across
    the restarts do not notice."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = _mel_params()
    ps = _settings(p)
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(30, S=3, seed=31, p=p)
    x2, x3 = _noisy(28, 5, 0.7, 90.0), _noisy(26, 6, 1.2, 60.0)
    rs = np.random.RandomState(32)
    Bn, Hn, An = _f32(Bds[2] * (1 + 0.1 * rs.random_sample(Bds[2].shape))), rs.random_sample(200), rs.random_sample((50, 100))
    BMn = _mel_dict(_melmat(p), Bn)
    mk = lambda: OnlineBatchSeparator(Bx, Bds, ps, 3, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx, B_Mel_x=BMx, B_Mel_d=BMds)  # noqa: E731
    ref0 = _run(gpu_ctx, pcms[:1], Bx, Bds[:1], p, H0s[:1], Ads[:1], BMx, BMds[:1])[0]
    sep = mk()
    e, cut = np.zeros(0), 2000
    acc0 = [sep.process([pcms[0][:cut], pcms[1], e], [False, True, False])[0]["x_tilde_f"]]
    m1, d1 = sep.mel_basis_f64(1), sep.basis_f64(1)
    assert np.array_equal(d1, _f32(Bds[1]))
    sep.restart(1)  # carry
    assert np.array_equal(sep.mel_basis_f64(1), m1) and np.array_equal(sep.basis_f64(1), d1)
    acc0.append(sep.process([pcms[0][cut:cut + 1500], x2, e], [False, True, False])[0]["x_tilde_f"])
    carry = (None, sep.trace(1), sep.mel_basis_f64(1), sep.basis_f64(1))
    sep.restart([1], B_DFT_d=Bn, H0=Hn, Ad_blk0=An, B_Mel_d=BMn)  # new dictionaries
    assert np.array_equal(sep.mel_basis_f64(1), BMn) and np.array_equal(sep.basis_f64(1), Bn)
    outs = sep.process([pcms[0][cut + 1500:], x3, e], [True, True, False])
    acc0.append(outs[0]["x_tilde_f"])
    new = (outs[1], sep.trace(1), sep.mel_basis_f64(1), sep.basis_f64(1))
    assert np.array_equal(np.concatenate(acc0), ref0[0]["x_tilde_f"]) and sep.trace(0) == ref0[1]
    assert np.array_equal(sep.mel_basis_f64(0), ref0[2])
    assert sep.trace(2) == [] and np.array_equal(sep.mel_basis_f64(2), BMds[2])
    sep.close()
    fresh = _run(gpu_ctx, [x3], Bx, [Bn], p, [Hn], [An], BMx, [BMn])[0]
    _same(new, fresh)
    # the same carry with the master passed in explicitly
    sep = mk()
    _file(sep, 1, pcms[1])
    sep.restart(1, B_DFT_d=d1, B_Mel_d=m1)
    expl = _file(sep, 1, x2)
    sep.close()
    assert carry[1] == expl[1] and np.array_equal(carry[2], expl[2]) and np.array_equal(carry[3], expl[3])
    assert sum(t["solved"] for t in carry[1]) > 0


def _mel_chain_vs_oracle(ctx, p):
    """tests/test_online_batch_restart.py's _chain_vs_oracle in Mel mode: a 3-file chain on slot 0 of a batch of 2, both
    dictionaries carried on the device.  Per file, against the oracle started from the device's carried fp64 B_Mel_d
    ("file") and the chain the oracle carries itself ("chain")."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(40, S=2, seed=24, p=p)
    files = [pcms[0], _noisy(38, 7, 0.6, 80.0), _noisy(36, 8, 1.1, 120.0)]
    sep = OnlineBatchSeparator(Bx, Bds, _settings(p), 2, H0=H0s, Ad_blk0=Ads, ctx=ctx, B_Mel_x=BMx, B_Mel_d=BMds)
    sep.process([np.zeros(0), pcms[1]], [False, True])  # company that finished
    B_dev, B_orc = BMds[0], BMds[0]
    rows, solved = [], 0
    for i, x in enumerate(files):
        if i:
            sep.restart(0)
        out, tr, BMn, Bdn = _file(sep, 0, x)
        assert np.array_equal(Bdn, _f32(Bds[0]))
        solved += sum(t["solved"] for t in tr)
        chain = None
        for kind, B0 in (("file", B_dev), ("chain", B_orc)):
            o16, of, BMo, rtr = _oracle(x, Bx, Bds[0], p, H0s[0], Ads[0], BMx, B0)
            dd, dr = _decisions(tr), _decisions(rtr)
            dev = out["x_tilde_f"]
            assert len(dev) == len(of) and np.isfinite(dev).all()
            rows.append(dict(file=i, kind=kind, same=dd == dr, rel_out=np.linalg.norm(dev - of) / np.linalg.norm(of),
                             rel_B=np.linalg.norm(BMn - BMo) / np.linalg.norm(BMo),
                             i16=int(np.abs(out["x_tilde"].astype(int) - o16.astype(int)).max(initial=0))))
            if kind == "chain":
                chain = BMo
        B_dev, B_orc = BMn, chain
    sep.close()
    assert solved > 0
    return rows


@pytest.mark.gpu
def test_mel_chain_matches_the_oracle(gpu_ctx):
    """A 3-file Mel chain (MelConv 1, adaptation on): every file within REL_OUT of the oracle started from the device's
    carried B_Mel_d, the first two within REL_OUT_CHAIN of the oracle's own chain, with equal decision traces."""
    for r in _mel_chain_vs_oracle(gpu_ctx, _mel_params()):
        if r["kind"] == "chain" and r["file"] >= 2:
            continue
        bound = REL_OUT if r["kind"] == "file" else REL_OUT_CHAIN
        assert r["same"] and r["rel_out"] < bound and r["rel_B"] < 10 * bound, r
        if r["kind"] == "file":
            assert r["i16"] <= 1, r


@pytest.mark.gpu
def test_mel_chain_driver_does_not_depend_on_scheduling(gpu_ctx):
    """Five uneven Mel chains (one with an empty file), each with its own B_DFT_d and B_Mel_d: identical bits for
    n_streams 1, 2, 5 and two chunk_hops values; one-file chains equal ntf_sep_event_rt_batch bit for bit."""
    from se_snmf_nat_amd.online import ntf_sep_event_rt_batch, ntf_sep_event_rt_chains
    p = _settings(_mel_params(0))
    _, Bx, Bds, _, _, BMx, BMds = _mel_streams(10, S=5, seed=26)
    chains = _uneven_chains()
    kw = dict(B_Mel_x=BMx, B_Mel_d=BMds, ctx=gpu_ctx)
    base = ntf_sep_event_rt_chains(chains, Bx, Bds, p, **kw)
    assert [len(r) for r in base] == [len(c) for c in chains]
    assert base[0][0][2].shape == (N1, 100)
    for n_streams in (1, 2, 5):
        for hops in (None, 7):
            if n_streams == 5 and hops is None:
                continue
            got = ntf_sep_event_rt_chains(chains, Bx, Bds, p, n_streams=n_streams, chunk_hops=hops, **kw)
            for rc, gc in zip(base, got):
                for a, b in zip(rc, gc):
                    assert all(np.array_equal(u, v) for u, v in zip(a, b)), (n_streams, hops)
    pcms = [c[0] for c in chains]
    one = ntf_sep_event_rt_chains([[x] for x in pcms], Bx, Bds, p, n_streams=len(pcms), **kw)
    bat = ntf_sep_event_rt_batch(pcms, Bx, Bds, p, **kw)
    for (a,), b in zip(one, bat):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.gpu
def test_mel_error_codes(gpu_ctx):
    """At the C entries: set_mel after a process call returns SNMF_ERR_STATE; F_order 1 or above F, or a NULL argument,
    SNMF_ERR_INVALID; get_mel_basis_* and restart_mel with a B_Mel_d on a DFT batch, SNMF_ERR_STATE.  After each refusal
    a valid Mel run -- on the refused handle where it is still fresh -- gives the same bits."""
    from se_snmf_nat_amd import _lib
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    lib = _lib.load()
    p = _mel_params()
    pd = _settings(default_params())
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(12, S=2, seed=41, p=p)
    ref = _run(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, BMx, BMds)
    from se_snmf_nat_amd.frontend import mel_matrix
    mm = np.ascontiguousarray(mel_matrix(p["fs"], N1, p["fftlength"], 1.0, p["fs"] / 2).T, dtype=np.float32)
    bx = np.asfortranarray(BMx, dtype=np.float32)
    bd = np.ascontiguousarray(np.concatenate([np.asarray(B, np.float32).ravel(order="F") for B in BMds]))
    F = p["fftlength"] // 2 + 1

    def dft_batch():
        return OnlineBatchSeparator(Bx, Bds, pd, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)

    def mel_run(sep):
        assert lib.snmf_online_batch_set_mel(sep._h, N1, 1, mm.ctypes.data, bx.ctypes.data, bd.ctypes.data) == 0
        sep.mel, sep.n1 = True, N1
        outs = sep.process(pcms, flush=True)
        for k in range(2):
            _same((outs[k], sep.trace(k), sep.mel_basis_f64(k), sep.basis_f64(k)), ref[k])
        sep.close()

    sep = dft_batch()
    sep.process([pcms[0][:800], np.zeros(0)])
    assert lib.snmf_online_batch_set_mel(sep._h, N1, 1, mm.ctypes.data, bx.ctypes.data, bd.ctypes.data) == 7
    sep.close()
    for n1, ptrs in ((1, None), (F + 1, None), (N1, (None, bx.ctypes.data, bd.ctypes.data)), (N1, (mm.ctypes.data, None, bd.ctypes.data)),
                     (N1, (mm.ctypes.data, bx.ctypes.data, None))):
        sep = dft_batch()
        args = ptrs or (mm.ctypes.data, bx.ctypes.data, bd.ctypes.data)
        assert lib.snmf_online_batch_set_mel(sep._h, n1, 1, *args) == 1
        mel_run(sep)
    sep = dft_batch()
    buf, buf32 = np.zeros((N1, 100)), np.zeros((N1, 100), np.float32)
    assert lib.snmf_online_batch_get_mel_basis_f32(sep._h, 0, buf32.ctypes.data, N1) == 7
    assert lib.snmf_online_batch_get_mel_basis_f64(sep._h, 0, buf.ctypes.data, N1) == 7
    sl = np.array([0], np.int32)
    assert lib.snmf_online_batch_restart_mel(sep._h, 1, sl.ctypes.data, None, buf.ctypes.data, None, None) == 7
    assert lib.snmf_online_batch_restart_mel(sep._h, 1, sl.ctypes.data, None, None, None, None) == 0  # = restart
    with pytest.raises(_lib.SnmfError) as e:
        sep.restart(0, B_Mel_d=buf)
    assert e.value.status == 7
    mel_run(sep)
