"""Batched online separation (snmf_online_batch_* in include/snmf.h, OnlineBatchSeparator): S independent streams of the
per-frame loop in shared launches.  Every stream must match its own fp64 oracle run (oracle/online_oracle.py) with the
tolerances of tests/test_online.py, and its bits must not depend on the other streams of its batch or on how the
streams are fed."""
import os

import numpy as np
import pytest

from oracle.online_oracle import default_params, ntf_sep_event_rt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_OUT = 1e-4
REL_OUT_ED_ADAPT = 2e-3  # tests/test_online.py: the Euclidean variant with adaptation carries its own bound
# beta = 0.5 / 1.5 with 30 un-stopped frame iterations: the third stream of the beta = 0.5 variant measured 1.1e-4 (every
# decision equal); the generic update's fp32 pow (lam^(beta-2) through den) leaves a little more per frame than KL's ratio
REL_OUT_GEN = 3e-4


def _fixture():
    B = np.load(os.path.join(GOLD, "ref_data.npz"))["B"].astype(np.float64)
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    return s, B[:, :100], B[:, 100:]


def _streams(n_hops, S=5, seed=11):
    """S streams that differ in signal (offset, scale, seeded noise), length, H0 / Ad_blk0 and initial B_DFT_d."""
    s, Bx, Bd = _fixture()
    rs = np.random.RandomState(seed)
    pcms, Bds, H0s, Ads = [], [], [], []
    lens = [n_hops * 160, 2 * 160, n_hops * 160 + 57, (n_hops - 7) * 160, (n_hops - 3) * 160 + 100][:S]
    while len(lens) < S:
        lens.append(n_hops * 160)
    for k in range(S):
        off = (k * 1733) % (len(s) - lens[k])
        x = s[off:off + lens[k]] * (0.5 + 0.25 * k) + rs.randn(lens[k]) * 30.0 * k
        pcms.append(np.round(x))
        if k % 2:
            Bk = Bd[:, rs.permutation(Bd.shape[1])]
        else:
            Bk = Bd * (1.0 + 0.05 * rs.random_sample(Bd.shape)) if k else Bd.copy()
        Bds.append(Bk)
        H0s.append(rs.random_sample(200))
        Ads.append(rs.random_sample((50, 100)))
    return pcms, Bx, Bds, H0s, Ads


def _settings(p):
    from se_snmf_nat_amd.online import default_settings
    ps = default_settings()
    ps.update({k: v for k, v in p.items() if k in ps or k == "beta_div"})  # (beta_div: the divergence of cf = 'x')
    return ps


def _run_batch(ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=False, feed=None):
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    S = len(pcms)
    sep = OnlineBatchSeparator(Bx, Bds, _settings(p), S, H0=H0s, Ad_blk0=Ads, ctx=ctx, class_outputs=class_outputs)
    keys = ["x_tilde", "x_tilde_f"] + (["x_hat", "d_hat"] if class_outputs else [])
    acc = [{k: [] for k in keys} for _ in range(S)]
    if feed is None:
        outs = sep.process(pcms, flush=True)
        for a, o in zip(acc, outs):
            for k in keys:
                a[k].append(o[k])
    else:
        for chunk_list, flush in feed:
            outs = sep.process(chunk_list, flush=flush)
            for a, o in zip(acc, outs):
                for k in keys:
                    a[k].append(o[k])
    res = []
    for k in range(S):
        o = {key: np.concatenate(acc[k][key]) for key in keys}
        res.append((o, sep.trace(k), sep.basis(k)))
    sep.close()
    return res


def _decisions(tr):
    return ([t["n_iter"] for t in tr], [int(t["trig"]) for t in tr], [t["n_up"] for t in tr], [t["adapt_iters"] for t in tr])


def _check_vs_oracle(out, trd, Bn, ref, tol=REL_OUT, cls=False):
    o16, of, Bdn, tr = ref[:4]
    assert _decisions(trd) == _decisions(tr)
    pairs = [(out["x_tilde_f"], of)]
    if cls:
        pairs += [(out["x_hat"], ref[4]), (out["d_hat"], ref[5])]
    for dev, rf in pairs:
        assert len(dev) == len(rf)
        ok = np.isfinite(rf)
        assert np.array_equal(np.isfinite(dev), ok)
        if ok.any() and np.linalg.norm(rf[ok]) > 0:
            assert np.linalg.norm(dev[ok] - rf[ok]) / np.linalg.norm(rf[ok]) < tol
    if tol == REL_OUT:
        assert np.abs(out["x_tilde"].astype(int) - o16.astype(int)).max(initial=0) <= 1
    assert np.linalg.norm(Bn - Bdn) / np.linalg.norm(Bdn) < 10 * tol


# ---------------------------------------------------------------- CPU ----------------------------------------------
def test_argument_checks_raise_before_any_device_call(monkeypatch):
    """Shapes and list lengths are checked in Python before the library is loaded or a context is made."""
    from se_snmf_nat_amd import _lib, online
    from se_snmf_nat_amd.online import OnlineBatchSeparator

    def no_device(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(online, "default_context", no_device)
    _, Bx, Bd = _fixture()
    p = _settings(default_params())
    for kw in (dict(n_streams=0),
               dict(n_streams=3, B_DFT_d=[Bd, Bd]),
               dict(n_streams=2, B_DFT_d=Bd[:-1]),
               dict(n_streams=2, B_DFT_d=[Bd, Bd[:, :50]]),
               dict(n_streams=2, H0=[np.ones(200)]),
               dict(n_streams=2, H0=np.ones(199)),
               dict(n_streams=2, Ad_blk0=[np.ones((50, 100)), np.ones((50, 99))])):
        args = dict(B_DFT_d=Bd)
        args.update(kw)
        with pytest.raises(_lib.SnmfError) as e:
            OnlineBatchSeparator(Bx, args.pop("B_DFT_d"), p, args.pop("n_streams"), **args)
        assert e.value.status == 1  # SNMF_ERR_INVALID
    with pytest.raises(_lib.SnmfError) as e:
        OnlineBatchSeparator(Bx, Bd, dict(p, B_sep_mode="Mel"), 2)
    assert e.value.status == 8  # SNMF_ERR_UNSUPPORTED


# ---------------------------------------------------------------- GPU ----------------------------------------------
@pytest.mark.gpu
def test_heterogeneous_batch_matches_the_oracle_per_stream(gpu_ctx):
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams(40)
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads)
    for k in range(len(pcms)):
        ref = ntf_sep_event_rt(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], return_trace=True)
        _check_vs_oracle(*res[k], ref)
    assert sum(t["solved"] for t in res[0][1]) > 0


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_company(gpu_ctx):
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams(30)
    alone = _run_batch(gpu_ctx, pcms[:1], Bx, Bds[:1], p, H0s[:1], Ads[:1])[0]
    full = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads)
    order = [3, 1, 4, 0, 2]
    perm = _run_batch(gpu_ctx, [pcms[i] for i in order], Bx, [Bds[i] for i in order], p, [H0s[i] for i in order],
                      [Ads[i] for i in order])
    for other in (full[0], perm[order.index(0)]):
        for key in ("x_tilde_f", "x_tilde"):
            assert np.array_equal(alone[0][key], other[0][key])
        assert alone[1] == other[1]
        assert np.array_equal(alone[2], other[2])
    for j, i in enumerate(order):  # every stream, not only the first
        assert np.array_equal(perm[j][0]["x_tilde_f"], full[i][0]["x_tilde_f"]) and perm[j][1] == full[i][1]


@pytest.mark.gpu
def test_bits_do_not_depend_on_how_the_streams_are_fed(gpu_ctx):
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams(30, S=3)
    whole = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads)
    sizes = [160, 1000, 57]
    pos = [0, 0, 0]
    feed = []
    rnd = 0
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
    # streams flush in different calls: 1 first, then 0 and 2 together
    feed.append(([pcms[k][:0] for k in range(3)], [False, True, False]))
    feed.append(([pcms[k][:0] for k in range(3)], [True, False, True]))
    fed = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, feed=feed)
    for a, b in zip(whole, fed):
        assert np.array_equal(a[0]["x_tilde_f"], b[0]["x_tilde_f"]) and np.array_equal(a[0]["x_tilde"], b[0]["x_tilde"])
        assert a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_golden_run_inside_a_batch(gpu_ctx):
    g = np.load(os.path.join(GOLD, "online_is16_124frames.npz"))
    s, Bx, Bd = _fixture()
    rs = np.random.RandomState(1)
    H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
    pcms, _, Bds, H0s, Ads = _streams(40, S=3, seed=5)
    pcms[1], Bds[1], H0s[1], Ads[1] = s, Bd, H0, Ad0
    out, tr, Bn = _run_batch(gpu_ctx, pcms, Bx, Bds, default_params(), H0s, Ads)[1]
    assert _decisions(tr) == (list(g["n_iter"]), [int(x) for x in g["trig"]], list(g["n_up"]), list(g["adapt_iters"]))
    ref = g["x_tilde_f"].astype(np.float64)
    assert len(out["x_tilde"]) == len(ref)
    assert np.linalg.norm(out["x_tilde_f"] - ref) / np.linalg.norm(ref) < REL_OUT
    assert np.abs(out["x_tilde"].astype(int) - g["x_tilde_i16"].astype(int)).max() <= 1
    assert np.linalg.norm(Bn[::4] - g["B_DFT_d_sub"]) / np.linalg.norm(g["B_DFT_d_sub"]) < 1e-3
    np.testing.assert_allclose([t["beta"] for t in tr], g["beta"], rtol=1e-3)


@pytest.mark.gpu
def test_reference_held_recordings_as_one_batch(gpu_ctx):
    """tests/test_refwav.py's pin (exact length, lag 0, corr >= 0.99, SNR >= 20 / 19.5 dB), both recordings -- of
    different lengths -- in one batch of 2."""
    from se_snmf_nat_amd.online import default_settings, ntf_sep_event_rt_batch
    from tests.test_refwav import _check, _inputs
    keys = ["m03", "lm"]
    ins = [_inputs(k) for k in keys]
    Bx, Bd = ins[0][2], ins[0][3]
    res = ntf_sep_event_rt_batch([x[0].astype(np.float64) for x in ins], Bx, Bd, default_settings(), H0=[x[4] for x in ins],
                                 Ad_blk0=[x[5] for x in ins], ctx=gpu_ctx)
    for k, x, (o16, of, _) in zip(keys, ins, res):
        _check(k, of, o16, x[1])


VARIANTS = [
    dict(ENHANCE_METHOD="Wiener"),
    dict(blk_sparse=0),
    dict(adapt_train_N=0),
    dict(preemph=0.92, pow=1),
    dict(cf="ed", sparsity=50.0),
    dict(conv_eps=0.0, max_iter=12),
    # generic beta: k_hsolve_frame<BM_GEN, RECON, BATCH> (tests/test_online.py's VARIANTS).  beta = 1.5 runs in WADAPT_CASES
    # instead: here the 2-hop stream's class outputs decay to ~1e-65 under it (fp64), below fp32's range
    dict(cf="x", beta_div=0.5, adapt_train_N=0, conv_eps=0.0, max_iter=30),
    dict(cf="is", adapt_train_N=0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(f"{k}={v[k]}" for k in v))
def test_variants_match_the_oracle(gpu_ctx, var):
    p = dict(default_params(), **var)
    pcms, Bx, Bds, H0s, Ads = _streams(36, S=3, seed=3)
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=True)
    tol = REL_OUT_ED_ADAPT if (var.get("cf") == "ed" and p.get("adapt_train_N", 1)) else REL_OUT
    if var.get("cf") == "x":
        tol = REL_OUT_GEN
    for k in range(3):
        ref = ntf_sep_event_rt(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], return_trace=True, class_outputs=True)
        _check_vs_oracle(*res[k], ref, tol=tol, cls=True)


KB = 1024


def wbatch_lds(Ra, ma, beta_div):
    """Dynamic LDS of k_wadapt_batch in bytes: wbatch_lds() of snmf_online_batch.h with kWbNW = 16 waves, kWbRB = 4 rows per
    block and RA2 = R_a rounded up to 64 (the lane layout: a second column per lane when R_a > 64)."""
    NW, RB, RA2 = 16, 4, (Ra + 63) // 64 * 64
    doubles = 5 * RA2 + NW * 2 * RA2 + 2 * NW
    floats = ((Ra * ma + 3) & ~3) + ma * RA2 + NW * (RB * Ra + RB * ma * (1 if beta_div == 1.0 else 2))
    return doubles * 8 + floats * 4


def _geo_streams(geo, n_hops, S=3, seed=11):
    """_streams for another geometry (tests/test_online.py's GEOMETRIES form): S streams with different signals (offset,
    scale, noise), lengths, H0 / Ad_blk0 and initial noise dictionaries."""
    from test_online import _random_setup
    fft, sz, hop, R_x, R_d, over = geo
    Bx, Bd, win = _random_setup(fft, fft, sz, hop, R_x, R_d)
    p = dict(default_params(), fftlength=fft, framelength=sz, frameshift=hop, win_STFT=win, win_ISTFT=win.copy(),
             overlapscale=2 * hop / sz)
    p.update(over)
    s, _, _ = _fixture()
    rs = np.random.RandomState(seed)
    lens = [n_hops * hop, (n_hops - 7) * hop + hop // 3, (n_hops - 3) * hop][:S]
    pcms, Bds, H0s, Ads = [], [], [], []
    for k in range(S):
        off = (k * 1733) % (len(s) - lens[k])
        pcms.append(np.round(s[off:off + lens[k]] * (0.5 + 0.25 * k) + rs.randn(lens[k]) * 30.0 * k))
        Bds.append(Bd[:, rs.permutation(R_d)] if k % 2 else (Bd * (1.0 + 0.05 * rs.random_sample(Bd.shape)) if k else Bd.copy()))
        H0s.append(rs.random_sample(R_x + R_d))
        Ads.append(rs.random_sample((p["R_a"], p["m_a"])))
    return p, pcms, Bx, Bds, H0s, Ads


def _batch_geometries():
    from test_online import GEOMETRIES
    # (the R_a = 80 entry is WADAPT_CASES' first, on a shorter stream)
    return [g for g in GEOMETRIES if g[0] in (64, 128, 256, 512, 1024) and g[3] + g[4] <= 200 and g[5].get("R_a", 50) <= 64]


# k_wadapt_batch off the shipped 50 x 100 ring (R_x = 72, R_d = 128 at the shipped transform): R_a > 64 puts a second
# column on every lane (RA2 = 128), m_a <= 64 takes one trip of the frame loop.  The ring stays at least as long as R_a
# except in the R_a = 128 case, which is short (an under-determined ring lets fp32 rounding move stop decisions,
# tests/test_online.py's geometry docstring).
WADAPT_CASES = [
    (dict(R_a=80, m_a=80), 30),
    (dict(R_a=64, m_a=128), 30),
    (dict(R_a=72, m_a=72, cf="x", beta_div=1.5, conv_eps=0.0, max_iter=30), 30),
    (dict(R_a=128, m_a=40), 14),
    (dict(R_a=40, m_a=48), 30),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("geo", g) for g in _batch_geometries()] + [("wadapt", c) for c in WADAPT_CASES],
                         ids=lambda c: (f"fft{c[1][0]}-sz{c[1][1]}-hop{c[1][2]}-r{c[1][3]}+{c[1][4]}" if c[0] == "geo" else
                                        "wadapt-" + "-".join(f"{k}={v}" for k, v in c[1][0].items())))
def test_heterogeneous_batch_off_the_shipped_geometry(gpu_ctx, case):
    """S = 3 heterogeneous streams per launch at other transforms (k_obstft / k_obistft at LOGN 6..10), dictionary sizes
    (k_hsolve_frame<FB, KB, ..., BATCH = true> at FB = 4 and 8: the per-stream strides rp * Fp with other Fp) and
    adaptation rings (k_wadapt_batch with R_a > 64, m_a = 128, m_a <= 64, generic beta); every stream against its own
    fp64 oracle run (src/NTF_sep_event_RT.m:67-124, src/bnmf_sep_event_RT_IS16.m:65-363).
    Found here: snmf_online_batch_create left the pad entries r..rp-1 of dphv at 0, so whenever r < 8 * KB (r = 20, 36,
    120) every pad activation became 0 * 0 / 0 = NaN and every frame solve ran to max_iter."""
    kind, c = case
    if kind == "geo":
        geo, n_hops = c, 36
    else:
        over, n_hops = c
        geo = (1024, 640, 160, 72, 128, dict(overlap_m_a=0.05, Ar_up=2.0, sparsity=1.0, **over))
        assert wbatch_lds(over["R_a"], over["m_a"], over.get("beta_div", 1.0)) < 160 * KB
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(geo, n_hops)
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=True)
    for k in range(len(pcms)):
        ref = ntf_sep_event_rt(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], return_trace=True, class_outputs=True)
        _check_vs_oracle(*res[k], ref, cls=True)
    if p["adapt_train_N"]:
        assert sum(t["solved"] for t in res[0][1]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(512, 400, 100, 24, 40, dict(P_len_k=30, P_len_l=6, init_N_len=4, DCbin=3, DCbin_back=3)),
                                 (128, 100, 25, 16, 20, dict(P_len_k=12, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2))],
                         ids=["fft512-r24+40", "fft128-r16+20"])
def test_batch_equals_single_stream_without_adaptation(gpu_ctx, geo):
    """With adapt_train_N = 0 a batch stream runs the same per-frame work as OnlineSeparator: identical decision traces
    and x_tilde_f within 1e-6.  (Not bit-identical: the single-stream separator solves each frame through the plan's
    launch_small and its own STFT / post-filter kernels, the batch through the BATCH forms with another reduction order.)"""
    from se_snmf_nat_amd.online import OnlineSeparator
    fft, sz, hop, R_x, R_d, over = geo
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams((fft, sz, hop, R_x, R_d, dict(over, adapt_train_N=0, R_a=4, m_a=4)), 30)
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads)
    for k in range(len(pcms)):
        sep = OnlineSeparator(Bx, Bds[k], _settings(p), H0=H0s[k], Ad_blk0=Ads[k], ctx=gpu_ctx)
        out = sep.process(pcms[k], flush=True)
        tr = sep.trace()
        sep.close()
        assert _decisions(res[k][1]) == _decisions(tr)
        a, b = res[k][0]["x_tilde_f"], out["x_tilde_f"]
        assert len(a) == len(b) and np.array_equal(np.isfinite(a), np.isfinite(b))
        ok = np.isfinite(b)
        assert np.linalg.norm(a[ok] - b[ok]) / np.linalg.norm(b[ok]) < 1e-6


@pytest.mark.gpu
def test_more_streams_than_cus(gpu_ctx):
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams(12, S=3, seed=9)
    pcms = [x[:12 * 160] for x in pcms]
    singles = [_run_batch(gpu_ctx, pcms[k:k + 1], Bx, Bds[k:k + 1], p, H0s[k:k + 1], Ads[k:k + 1])[0] for k in range(3)]
    S = 300
    big = _run_batch(gpu_ctx, [pcms[k % 3] for k in range(S)], Bx, [Bds[k % 3] for k in range(S)], p, [H0s[k % 3] for k in range(S)],
                     [Ads[k % 3] for k in range(S)])
    for k in range(S):
        a, b = singles[k % 3], big[k]
        assert np.array_equal(a[0]["x_tilde_f"], b[0]["x_tilde_f"]) and np.array_equal(a[0]["x_tilde"], b[0]["x_tilde"])
        assert a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_error_codes(gpu_ctx):
    import ctypes as C

    from se_snmf_nat_amd import _lib
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    _, Bx, Bd = _fixture()
    p = _settings(default_params())
    lib = _lib.load()
    for over, code in ((dict(B_sep_mode="Mel"), 8), (dict(basis_update_N=1), 8)):
        with pytest.raises(_lib.SnmfError) as e:
            OnlineBatchSeparator(Bx, Bd, dict(p, **over), 2, ctx=gpu_ctx)
        assert e.value.status == code
    rs = np.random.RandomState(0)
    big = rs.random_sample((Bx.shape[0], 150))
    with pytest.raises(_lib.SnmfError) as e:  # r = 300 > the frame kernel's 200
        OnlineBatchSeparator(big, big, p, 2, ctx=gpu_ctx)
    assert e.value.status == 8
    with pytest.raises(_lib.SnmfError) as e:
        OnlineBatchSeparator(Bx, Bd, p, 0, ctx=gpu_ctx)
    assert e.value.status == 1
    with pytest.raises(_lib.SnmfError) as e:
        OnlineBatchSeparator(Bx, [Bd, Bd, Bd], p, 2, ctx=gpu_ctx)
    assert e.value.status == 1
    with pytest.raises(_lib.SnmfError) as e:
        OnlineBatchSeparator(Bx, Bd[:, :50].T, p, 2, ctx=gpu_ctx)
    assert e.value.status == 1
    # outside the batch envelope: the frame kernel's F <= 513 and r <= 200, k_wadapt_batch's LDS (snmf_online_batch.h:
    # wbatch_lds); after each refusal a valid separator is still made and still runs
    from test_online import _random_setup
    s, _, _ = _fixture()
    Bx2, Bd2, win2 = _random_setup(2048, 2048, 1600, 400, 40, 40)
    p2048 = dict(p, fftlength=2048, framelength=1600, frameshift=400, win_STFT=win2, win_ISTFT=win2.copy(), overlapscale=0.5,
                 R_a=24, m_a=30, P_len_k=100)
    refused = [(Bx2, Bd2, p2048), (rs.random_sample((Bx.shape[0], 100)), rs.random_sample((Bx.shape[0], 101)), p)]
    Bx3, Bd3 = rs.random_sample((Bx.shape[0], 72)), rs.random_sample((Bx.shape[0], 128))
    for Ra, ma in ((128, 128), (100, 100)):
        assert wbatch_lds(Ra, ma, 1.0) > 160 * KB
        refused.append((Bx3, Bd3, dict(p, R_a=Ra, m_a=ma)))
    def valid_run():
        ok = OnlineBatchSeparator(Bx, Bd, p, 2, ctx=gpu_ctx)
        outs = ok.process([s[:1600], s[800:2400]], flush=True)
        ok.close()
        return [o["x_tilde_f"] for o in outs]
    before = valid_run()
    for bx, bd, q in refused:
        with pytest.raises(_lib.SnmfError) as e:
            OnlineBatchSeparator(bx, bd, q, 2, ctx=gpu_ctx, Ad_blk0=[np.ones((q["R_a"], q["m_a"]))] * 2)
        assert e.value.status == 8
        after = valid_run()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    # the C entry itself: S = 0 is INVALID
    sep = OnlineBatchSeparator(Bx, Bd, p, 2, ctx=gpu_ctx)
    h = C.c_void_p()
    rc = lib.snmf_online_batch_create(gpu_ctx._h, C.byref(sep._q), 0, Bx.ctypes.data, Bd.ctypes.data, Bd.ctypes.data, Bd.ctypes.data,
                                      Bd.ctypes.data, Bd.ctypes.data, C.byref(h))
    assert rc == 1
    s, _, _ = _fixture()
    with pytest.raises(_lib.SnmfError) as e:
        sep.process([s[:800], s[:800], s[:1]])  # list length
    assert e.value.status == 1
    sep.process([s[:800], s[:800]], flush=[True, False])
    with pytest.raises(_lib.SnmfError) as e:
        sep.process([s[:160], s[:0]])  # feeding the flushed stream
    assert e.value.status == 7
    sep.process([s[:0], s[:800]], flush=[False, True])
    sep.close()
