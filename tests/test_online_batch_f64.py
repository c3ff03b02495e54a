"""The fp64 mode of the batched online separator: OnlineBatchSeparator(..., precision="fp64"),
snmf_online_batch_create_f64 / _process_f64 (csrc/snmf_online_batch_f64.h).

Every stream of a batch must hold its own fp64 oracle run (oracle/online_oracle.py) as the single-stream fp64 separator holds
it, and its bits must depend neither on the other streams of its batch, nor on its slot, nor on how the streams are fed.

Bounds: the fp64 mode's own, tests/test_online_f64.py (derived there from the oracle's response to input perturbation, not
from the device): every decision (n_iter, trig, n_up, adapt_iters) equal; signal and x_hat / d_hat within 1e-9 overall;
final B_DFT_d within 1e-8; int16 at most 2 samples by 1 LSB.  Every test prints its figures before it asserts (pytest -s).

Measured on an MI355X (all 17 GPU tests pass; every decision of every stream equal, 0 int16 samples differ anywhere):
  heterogeneous batch (124 / 6 / 94 frames, 86 / 2 / 51 solves): signal <= 5.7e-15, x_hat / d_hat <= 2.8e-14, B_DFT_d <= 4.4e-14;
  variants: Wiener, no adaptation, no stop test <= 4.2e-14 (B_DFT_d <= 3.4e-13); ED signal 9.3e-12, d_hat 1.0e-11, B_DFT_d 1.8e-11;
    beta = 1.5 with the stop test (the largest of all): signal 7.1e-11, d_hat 1.5e-10, B_DFT_d 7.7e-10 on the 60-hop stream;
  geometries: F = 65 with the 8 x 12 ring <= 1.5e-14; the 64 x 128 ring at F = 513 <= 2.0e-13 (B_DFT_d <= 2e-15);
  against the single-stream fp64 separator: signal <= 4.5e-15, B_DFT_d <= 1.6e-14;
  chains: signal <= 1.6e-12 and B_DFT_d <= 1.8e-11 on the carried files; class partitions <= 6.8e-15;
  one slot's first / carried / fresh (restart_f64 with a new dictionary and draws) file: signal 4.2e-15 / 1.8e-13 / 9.8e-14,
    B_DFT_d <= 9.3e-13; the refused 80 x 100 and 128 x 40 rings report 117776 / 143376 and 79760 / 90000 bytes (beta 1 / 2).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle.online_oracle import default_params, ntf_sep_event_rt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("n_iter", "trig", "n_up", "adapt_iters")
HOP = 160
FIX_OVERALL, FIX_BASIS, I16_TIES = 1e-9, 1e-8, 2  # tests/test_online_f64.py
KB = 1024


def _fixture():
    B = np.load(os.path.join(GOLD, "ref_data.npz"))["B"].astype(np.float64)
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    return s, B[:, :100], B[:, 100:]


def _streams(lens, seed=11):
    """len(lens) streams built like tests/test_online_batch.py::_streams: they differ in signal (offset, scale, seeded
    noise), length, H0 / Ad_blk0 and initial B_DFT_d; a stream as long as the fixture IS the fixture (the 124-frame run)."""
    s, Bx, Bd = _fixture()
    rs = np.random.RandomState(seed)
    pcms, Bds, H0s, Ads = [], [], [], []
    for k, n in enumerate(lens):
        off = (k * 1733) % max(1, len(s) - n)
        x = s[off:off + n] * (0.5 + 0.25 * k) + rs.randn(n) * 30.0 * k if k else s[:n].copy()
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


def _decisions(tr):
    return {k: np.array([int(t[k]) for t in tr]) for k in KEYS}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _run_batch(ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=False, feed=None, flush=True, precision="fp64"):
    """-> per stream (outputs, trace, basis)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    S = len(pcms)
    sep = OnlineBatchSeparator(Bx, Bds, _settings(p), S, H0=H0s, Ad_blk0=Ads, ctx=ctx, class_outputs=class_outputs, precision=precision)
    keys = ["x_tilde", "x_tilde_f"] + (["x_hat", "d_hat"] if class_outputs else [])
    acc = [{k: [] for k in keys} for _ in range(S)]
    for chunk_list, fl in (feed if feed is not None else [(pcms, flush)]):
        for a, o in zip(acc, sep.process(chunk_list, flush=fl)):
            for k in keys:
                a[k].append(o[k])
    res = [({key: np.concatenate(acc[k][key]) for key in keys}, sep.trace(k), sep.basis(k)) for k in range(S)]
    sep.close()
    return res


def _judge(label, out, tr, Bn, ref, cls=True, n_fr=None):
    """One stream against its oracle run ref = (int16, float, final B_DFT_d, trace[, x_hat, d_hat]); n_fr: compare the
    first n_fr frames only (a stream fed without the flush)."""
    o16, of, Bdn, rtr = ref[:4]
    dec, rdec = _decisions(tr), _decisions(rtr)
    names = [("x_tilde_f", of)] + ([("x_hat", ref[4]), ("d_hat", ref[5])] if cls else [])
    if n_fr is not None:
        n_s = len(out["x_tilde_f"])
        rdec = {k: rdec[k][:n_fr] for k in KEYS}
        o16 = o16[:n_s]
        names = [(nm, rf[:n_s]) for nm, rf in names]
    first = next((i + 1 for i in range(min(len(dec["n_iter"]), len(rdec["n_iter"]))) if any(dec[k][i] != rdec[k][i] for k in KEYS)), None)
    errs = []
    for nm, rf in names:
        dev = out[nm]
        assert dev.dtype == np.float64 and len(dev) == len(rf), nm
        ok = np.isfinite(rf)  # a silent tail can be 0/0 in the reference's own formulas (:230): NaN on both sides
        assert np.array_equal(np.isfinite(dev), ok), nm
        errs.append(_rel(dev[ok], rf[ok]) if ok.any() and np.linalg.norm(rf[ok]) > 0 else 0.0)
    di = np.abs(out["x_tilde"].astype(int) - o16.astype(int))
    basis = _rel(Bn, Bdn)
    print("%s: frames %d, first differing decision %s, solves %d; %s; B_DFT_d %.3g; int16 differing %d (max %d LSB)"
          % (label, len(dec["n_iter"]), first, int((dec["adapt_iters"] > 0).sum()),
             ", ".join("%s %.3g" % (nm, e) for (nm, _), e in zip(names, errs)), basis, int((di > 0).sum()), int(di.max(initial=0))))
    for k in KEYS:
        assert np.array_equal(dec[k], rdec[k]), (label, k, first)
    assert Bn.dtype == np.float64
    assert max(errs) <= FIX_OVERALL, label
    assert di.max(initial=0) <= 1 and int((di > 0).sum()) <= I16_TIES, label
    assert basis <= FIX_BASIS, label


def _oracle(x, Bx, Bd, p, H0, Ad):
    return ntf_sep_event_rt(x, Bx, Bd, p, H0, Ad, return_trace=True, class_outputs=True)


# ---------------------------------------------------------------- CPU ----------------------------------------------
def test_precision_is_a_keyword_of_the_three_entry_points_and_defaults_to_fp32():
    import inspect

    from se_snmf_nat_amd import online
    for fn in (online.OnlineBatchSeparator.__init__, online.ntf_sep_event_rt_batch, online.ntf_sep_event_rt_chains):
        assert inspect.signature(fn).parameters["precision"].default == "fp32"


def test_unknown_precision_is_a_value_error():
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings, ntf_sep_event_rt_batch, ntf_sep_event_rt_chains
    s, Bx, Bd = _fixture()
    p = default_settings()
    with pytest.raises(ValueError, match="precision"):
        OnlineBatchSeparator(Bx, Bd, p, 2, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        ntf_sep_event_rt_batch([s[:HOP]], Bx, Bd, p, precision="double")
    with pytest.raises(ValueError, match="precision"):
        ntf_sep_event_rt_chains([[s[:HOP]]], Bx, Bd, p, precision="double")


def test_fp64_with_mel_is_unsupported_before_any_device_call(monkeypatch):
    from se_snmf_nat_amd import _lib, online
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings, ntf_sep_event_rt_batch, ntf_sep_event_rt_chains

    def no_device(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(online, "default_context", no_device)
    s, Bx, Bd = _fixture()
    p = dict(default_settings(), B_sep_mode="Mel")
    BM = np.ones((64, 100))
    for call in (lambda: OnlineBatchSeparator(Bx, Bd, p, 2, B_Mel_x=BM, B_Mel_d=BM, precision="fp64"),
                 lambda: ntf_sep_event_rt_batch([s[:HOP]], Bx, Bd, p, B_Mel_x=BM, B_Mel_d=BM, precision="fp64"),
                 lambda: ntf_sep_event_rt_chains([[s[:HOP]]], Bx, Bd, p, B_Mel_x=BM, B_Mel_d=BM, precision="fp64")):
        with pytest.raises(_lib.SnmfError) as e:
            call()
        assert e.value.status == 8  # SNMF_ERR_UNSUPPORTED


def test_new_symbols_are_bound_and_create_rejects_null(lib):
    from se_snmf_nat_amd import _lib
    for name in ("snmf_online_batch_create_f64", "snmf_online_batch_process_f64", "snmf_online_batch_process_classes_f64",
                 "snmf_online_batch_restart_f64"):
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes is not None
    h = C.c_void_p()
    assert lib.snmf_online_batch_create_f64(None, None, 2, None, None, None, None, None, None, C.byref(h)) == 1  # SNMF_ERR_INVALID
    assert not h.value


def wbatch64_lds(Ra, ma, beta_div):
    """Dynamic LDS of k_wadapt_batch64 in bytes: wbatch64_lds() of csrc/snmf_online_batch_f64.h with kWb64NW = 8 waves,
    kWb64RB = 4 rows per block, kWb64RP = 64 column lanes and one orientation of H with rows of odd length m_a | 1."""
    NW, RB, RP = 8, 4, 64
    small = 5 * RP + NW * 2 * RP + 2 * NW + RP // 2 + 2
    hs = (Ra * (ma | 1) + 1) & ~1
    wave = RB * RP + RB * ma * (1 if beta_div == 1.0 else 2)
    return (small + hs + NW * wave) * 8


# ---------------------------------------------------------------- GPU ----------------------------------------------
@pytest.mark.gpu
def test_heterogeneous_batch_matches_the_oracle_per_stream(gpu_ctx):
    """S = 3 on the 124-frame fixture at the shipped settings: the fixture itself, a stream of 2 hops, one ending mid-hop."""
    p = default_params()
    s, _, _ = _fixture()
    pcms, Bx, Bds, H0s, Ads = _streams([len(s), 2 * HOP, 90 * HOP + 57])
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=True)
    solved = 0
    for k in range(3):
        ref = _oracle(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k])
        if k == 0:
            assert len(ref[3]) == 124
        assert sum(int(t["adapt_iters"] > 0) for t in ref[3]) == sum(t["solved"] for t in res[k][1])
        solved += sum(int(t["adapt_iters"] > 0) for t in ref[3])
        _judge("heterogeneous stream %d" % k, *res[k], ref)
    assert solved > 0 and sum(t["solved"] for t in res[0][1]) > 0


VARIANTS = [
    dict(ENHANCE_METHOD="Wiener"),
    dict(adapt_train_N=0),
    dict(cf="ed", sparsity=50.0),
    dict(conv_eps=0.0, max_iter=12),
    # generic beta with the stop test: fed WITHOUT the flush and compared on the frames that carry signal, for the reason
    # written at tests/test_online_f64.py:148-156 (on the all-zero flush frames the oracle's stop is decided by pow's residue)
    dict(cf="x", beta_div=1.5),
]


@pytest.mark.gpu
@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(f"{k}={v[k]}" for k in v))
def test_variants_match_the_oracle(gpu_ctx, var):
    p = dict(default_params(), **var)
    s, _, _ = _fixture()
    pcms, Bx, Bds, H0s, Ads = _streams([len(s), 60 * HOP], seed=3)
    signal_only = var.get("cf") == "x" and var.get("conv_eps", 1e-3) > 0
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=True, flush=not signal_only)
    for k in range(2):
        ref = _oracle(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k])
        n_fr = None
        if signal_only:
            n_fr = len(pcms[k]) // HOP
            assert not _decisions(ref[3])["trig"][n_fr:].any()  # the oracle's dictionary after the last signal frame is its final one
            assert len(res[k][0]["x_tilde_f"]) == (n_fr - p["delay"]) * HOP
        _judge("variant %s stream %d" % (var, k), *res[k], ref, n_fr=n_fr)


GEO_CASES = [
    # a small transform (F = 65: 16 row blocks and one row; k_obstft64 / k_obistft<LOGN, double> at LOGN 7) with a short ring: R_a = 8 of
    # 64 column lanes, m_a = 12: one trip of the frame loop
    ((128, 100, 25, 16, 20, dict(P_len_k=12, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2, R_a=8, m_a=12, overlap_m_a=0.1)), 36),
    # the ring at the envelope's edge at the shipped transform (F = 513 = 128 row blocks and one row): R_a = 64 fills the
    # column lanes, m_a = 128: two trips of the frame loop (tests/test_online_batch.py's WADAPT_CASES form)
    ((1024, 640, 160, 72, 128, dict(overlap_m_a=0.05, Ar_up=2.0, sparsity=1.0, R_a=64, m_a=128)), 30),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEO_CASES, ids=["fft128-Ra8-ma12", "fft1024-Ra64-ma128"])
def test_heterogeneous_batch_off_the_shipped_geometry(gpu_ctx, case):
    from test_online_batch import _geo_streams
    geo, n_hops = case
    assert wbatch64_lds(geo[5]["R_a"], geo[5]["m_a"], 1.0) <= 160 * KB
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(geo, n_hops)
    res = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, class_outputs=True)
    solved = 0
    for k in range(len(pcms)):
        ref = _oracle(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k])
        assert np.isfinite(ref[1]).all() and np.isfinite(ref[2]).all()
        solved += sum(int(t["adapt_iters"] > 0) for t in ref[3])
        _judge("geometry %s stream %d" % (geo[:5], k), *res[k], ref)
    assert solved > 0  # the oracle alone runs adaptation solves in this case


def _same(a, b):
    for key in ("x_tilde_f", "x_tilde"):
        assert np.array_equal(a[0][key], b[0][key]), key
    assert a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.fixture(scope="module")
def three(gpu_ctx):
    """S = 3 streams of about 40 hops at the shipped settings, run once as one batch."""
    pcms, Bx, Bds, H0s, Ads = _streams([40 * HOP, 33 * HOP + 57, 37 * HOP], seed=7)
    full = _run_batch(gpu_ctx, pcms, Bx, Bds, default_params(), H0s, Ads)
    assert sum(t["solved"] for r in full for t in r[1]) > 0
    return (pcms, Bx, Bds, H0s, Ads), full


@pytest.mark.gpu
def test_bits_do_not_depend_on_company_slot_or_feeding(gpu_ctx, three):
    (pcms, Bx, Bds, H0s, Ads), full = three
    p = default_params()
    for k in range(3):  # alone
        _same(_run_batch(gpu_ctx, pcms[k:k + 1], Bx, Bds[k:k + 1], p, H0s[k:k + 1], Ads[k:k + 1])[0], full[k])
    order = [2, 0, 1]  # another slot
    perm = _run_batch(gpu_ctx, [pcms[i] for i in order], Bx, [Bds[i] for i in order], p, [H0s[i] for i in order], [Ads[i] for i in order])
    for j, i in enumerate(order):
        _same(perm[j], full[i])
    sizes, pos, feed, rnd = [160, 1000, 57], [0, 0, 0], [], 0  # 160- / 1000- / 57-sample chunks
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
    feed.append(([pcms[k][:0] for k in range(3)], [False, True, False]))
    feed.append(([pcms[k][:0] for k in range(3)], [True, False, True]))
    fed = _run_batch(gpu_ctx, pcms, Bx, Bds, p, H0s, Ads, feed=feed)
    for a, b in zip(fed, full):
        _same(a, b)


@pytest.mark.gpu
def test_more_streams_than_cus(gpu_ctx, three):
    (pcms, Bx, Bds, H0s, Ads), _ = three
    p = default_params()
    short = [x[:3 * HOP] for x in pcms]
    singles = [_run_batch(gpu_ctx, short[k:k + 1], Bx, Bds[k:k + 1], p, H0s[k:k + 1], Ads[k:k + 1])[0] for k in range(3)]
    S = 300
    big = _run_batch(gpu_ctx, [short[k % 3] for k in range(S)], Bx, [Bds[k % 3] for k in range(S)], p, [H0s[k % 3] for k in range(S)],
                     [Ads[k % 3] for k in range(S)])
    for k in range(S):
        _same(singles[k % 3], big[k])


@pytest.mark.gpu
def test_batch_streams_equal_the_single_stream_fp64_separator(gpu_ctx, three):
    """Decisions equal, signal within 1e-9 (not bit-identical: the two adaptation kernels reduce in different orders)."""
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings
    (pcms, Bx, Bds, H0s, Ads), full = three
    for k in range(3):
        sep = OnlineSeparator(Bx, Bds[k], default_settings(), H0=H0s[k], Ad_blk0=Ads[k], ctx=gpu_ctx, precision="fp64")
        out = sep.process(pcms[k], flush=True)
        tr, Bn = sep.trace(), sep.basis()
        sep.close()
        a, b = full[k][0]["x_tilde_f"], out["x_tilde_f"]
        print("batch vs single-stream fp64, stream %d: signal %.3g, B_DFT_d %.3g, solves %d"
              % (k, _rel(a, b), _rel(full[k][2], Bn), sum(t["solved"] for t in tr)))
        for key in KEYS:
            assert np.array_equal(_decisions(full[k][1])[key], _decisions(tr)[key]), key
        assert len(a) == len(b) and _rel(a, b) <= FIX_OVERALL
        assert _rel(full[k][2], Bn) <= FIX_BASIS


@pytest.mark.gpu
def test_chains_match_the_oracle_file_after_file(gpu_ctx):
    """2 chains x 2 files of about 60 hops: every file against the oracle run with the dictionary its predecessor left, and
    the same bits for n_streams = 1 (fresh restarts and carries on one slot) and 2."""
    from se_snmf_nat_amd.online import ntf_sep_event_rt_chains
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams([60 * HOP, 57 * HOP + 31, 62 * HOP, 58 * HOP], seed=5)
    chains = [[pcms[0], pcms[1]], [pcms[2], pcms[3]]]
    runs = [ntf_sep_event_rt_chains(chains, Bx, [Bds[0], Bds[2]], _settings(p), n_streams=n, H0=[H0s[0], H0s[2]], Ad_blk0=[Ads[0], Ads[2]],
                                    ctx=gpu_ctx, precision="fp64") for n in (2, 1)]
    solved = 0
    for c, (B0, H0, Ad) in enumerate(((Bds[0], H0s[0], Ads[0]), (Bds[2], H0s[2], Ads[2]))):
        B = B0
        for i, x in enumerate(chains[c]):
            o16, of, Bdn, tr = ntf_sep_event_rt(x, Bx, B, p, H0, Ad, return_trace=True)
            d16, df, dB = runs[0][c][i]
            di = np.abs(d16.astype(int) - o16.astype(int))
            print("chain %d file %d: signal %.3g, B_DFT_d %.3g, int16 differing %d, oracle solves %d"
                  % (c, i, _rel(df, of), _rel(dB, Bdn), int((di > 0).sum()), sum(int(t["adapt_iters"] > 0) for t in tr)))
            assert df.dtype == np.float64 and dB.dtype == np.float64 and len(df) == len(of)
            assert _rel(df, of) <= FIX_OVERALL and _rel(dB, Bdn) <= FIX_BASIS
            assert di.max(initial=0) <= 1 and int((di > 0).sum()) <= I16_TIES
            solved += sum(int(t["adapt_iters"] > 0) for t in tr)
            B = Bdn  # carried (src/NTF_sep_event_RT.m:27-38, :137-140)
            for a, b in zip(runs[0][c][i], runs[1][c][i]):
                assert np.array_equal(a, b)
    assert solved > 0  # (equal dictionaries after a file with solves: equal decisions in it)


@pytest.mark.gpu
def test_chain_decisions_equal_the_oracles(gpu_ctx):
    """The decisions of every file of a chain run on one slot: a first file, a carried file (restart with the adapted
    dictionary kept) against the oracle started from the oracle's own adapted dictionary, then a NEW chain on the used slot --
    snmf_online_batch_restart_f64 with a new dictionary and new fp64 draws -- against the oracle run of that file."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams([50 * HOP, 50 * HOP, 45 * HOP, 48 * HOP], seed=5)
    sep = OnlineBatchSeparator(Bx, Bds[1:2], _settings(p), 1, H0=H0s[1:2], Ad_blk0=Ads[1:2], ctx=gpu_ctx, precision="fp64")
    B, H0, Ad = Bds[1], H0s[1], Ads[1]
    for i, x in enumerate((pcms[1], pcms[2], pcms[3])):
        if i == 1:
            sep.restart(0)
        if i == 2:
            B, H0, Ad = Bds[3], H0s[3], Ads[3]
            sep.restart(0, B_DFT_d=B, H0=H0, Ad_blk0=Ad)
        out = sep.process([x], flush=True)[0]
        o16, of, B, tr = ntf_sep_event_rt(x, Bx, B, p, H0, Ad, return_trace=True)
        dec, rdec = _decisions(sep.trace(0)), _decisions(tr)
        print("%s file %d: %d frames, %d solves, signal %.3g, B_DFT_d %.3g"
              % (("first", "carried", "fresh")[i], i, len(tr), int((rdec["adapt_iters"] > 0).sum()), _rel(out["x_tilde_f"], of), _rel(sep.basis(0), B)))
        for k in KEYS:
            assert np.array_equal(dec[k], rdec[k]), (i, k)
        assert int((rdec["adapt_iters"] > 0).sum()) > 0
        assert _rel(out["x_tilde_f"], of) <= FIX_OVERALL and _rel(sep.basis(0), B) <= FIX_BASIS
    sep.close()


@pytest.mark.gpu
def test_restart_widens_fp32_draws_as_restart_f64_takes_them(gpu_ctx, lib):
    """snmf_online_batch_restart on an fp64 batch (H0 / Ad_blk0 in fp32, widened) gives the bits of snmf_online_batch_restart_f64
    with the same, fp32-representable, values; a stream count beyond the batch is INVALID before anything is read."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams([20 * HOP, 30 * HOP, 30 * HOP], seed=9)
    H32, A32 = H0s[2].astype(np.float32), np.asfortranarray(Ads[2], dtype=np.float32)
    sl = np.array([1], dtype=np.int32)
    Bn = np.asfortranarray(Bds[2], dtype=np.float64)
    res = []
    for widen in (False, True):
        sep = OnlineBatchSeparator(Bx, Bds[:2], _settings(p), 2, H0=H0s[:2], Ad_blk0=Ads[:2], ctx=gpu_ctx, precision="fp64")
        sep.process(pcms[:2], flush=True)
        if widen:
            assert lib.snmf_online_batch_restart(sep._h, 3, sl.ctypes.data, None, H32.ctypes.data, A32.ctypes.data) == 1  # n > S
            assert lib.snmf_online_batch_restart(sep._h, 1, sl.ctypes.data, Bn.ctypes.data, H32.ctypes.data, A32.ctypes.data) == 0
        else:
            sep.restart(1, B_DFT_d=Bn, H0=H32.astype(np.float64), Ad_blk0=A32.astype(np.float64))
        o = sep.process([pcms[0][:0], pcms[2]], flush=[False, True])[1]
        res.append((o["x_tilde_f"], o["x_tilde"], sep.basis(1), [tuple(t[k] for k in KEYS) for t in sep.trace(1)]))
        sep.close()
    assert sum(t[3] > 0 for t in res[0][3]) > 0  # the adaptation ran on the restarted stream
    assert all(np.array_equal(a, b) for a, b in zip(res[0][:3], res[1][:3])) and res[0][3] == res[1][3]


@pytest.mark.gpu
def test_class_partitions_match_the_oracle(gpu_ctx):
    from online_classes import class_reference
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    ev, nz = [1, 41], [1, 51]
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams([40 * HOP, 40 * HOP, 35 * HOP + 57], seed=7)
    pcms, Bds, H0s, Ads = pcms[1:], Bds[1:], H0s[1:], Ads[1:]
    sep = OnlineBatchSeparator(Bx, Bds, dict(_settings(p), EVENT_NUM=2, EVENT_RANK=ev, NOISE_NUM=2, NOISE_RANK=nz), 2, H0=H0s, Ad_blk0=Ads,
                               ctx=gpu_ctx, class_outputs=True, precision="fp64")
    outs = sep.process(pcms, flush=True)
    sep.close()
    for k in range(2):
        ref = class_reference(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], ev, nz)
        for name in ("x_tilde_f", "x_hat", "d_hat", "x_hat_i", "d_hat_i"):
            dev, rf = outs[k][name], ref[name]
            assert dev.dtype == np.float64 and dev.shape == rf.shape, name
            for c in range(rf.shape[0]) if rf.ndim == 2 else [None]:
                e = _rel(dev if c is None else dev[c], rf if c is None else rf[c])
                print("classes stream %d: %s%s %.3g" % (k, name, "" if c is None else "[%d]" % c, e))
                assert e <= FIX_OVERALL, (name, c)


def _valid_run(gpu_ctx, precision="fp64", **kw):
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings
    pcms, Bx, Bds, H0s, Ads = _streams([30 * HOP, 20 * HOP], seed=2)
    if precision is not None:
        kw["precision"] = precision
    sep = OnlineBatchSeparator(Bx, Bds, default_settings(), 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx, **kw)
    outs = sep.process(pcms, flush=True)
    res = [(o["x_tilde_f"], o["x_tilde"], sep.basis(k)) for k, o in enumerate(outs)]
    sep.close()
    return res


@pytest.mark.gpu
def test_refusals_and_a_valid_batch_afterwards(gpu_ctx, lib):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings
    s, Bx, Bd = _fixture()
    p = default_settings()
    good = _valid_run(gpu_ctx)
    # Mel: the Python mirror, and the Mel entries on an fp64 handle -> SNMF_ERR_UNSUPPORTED (8); the handle stays usable
    with pytest.raises(SnmfError) as e:
        OnlineBatchSeparator(Bx, Bd, dict(p, B_sep_mode="Mel"), 2, ctx=gpu_ctx, precision="fp64", B_Mel_x=np.ones((64, 100)),
                             B_Mel_d=np.ones((64, 100)))
    assert e.value.status == 8
    pcms, _, Bds, H0s, Ads = _streams([30 * HOP, 20 * HOP], seed=2)
    sep = OnlineBatchSeparator(Bx, Bds, p, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx, precision="fp64")
    melmat = np.ones((64, 513), np.float32)
    BM = np.ones((64, 200), np.float32, order="F")
    BM64 = np.ones((64, 100), np.float64, order="F")
    sl = np.zeros(1, np.int32)
    assert lib.snmf_online_batch_set_mel(sep._h, 64, 1, melmat.ctypes.data, BM.ctypes.data, BM.ctypes.data) == 8
    assert b"Mel" in lib.snmf_last_error()
    assert lib.snmf_online_batch_restart_mel(sep._h, 1, sl.ctypes.data, None, BM64.ctypes.data, None, None) == 8
    assert lib.snmf_online_batch_get_mel_basis_f32(sep._h, 0, BM.ctypes.data, 64) == 8
    assert lib.snmf_online_batch_get_mel_basis_f64(sep._h, 0, BM64.ctypes.data, 64) == 8
    # the fp32 process entries on an fp64 batch -> SNMF_ERR_STATE (7), n_out zeroed
    P = C.c_void_p * 2
    x32 = [np.ascontiguousarray(x, dtype=np.float32) for x in pcms]
    n = np.array([x.size for x in x32], dtype=np.int64)
    n_out = np.full(2, -1, dtype=np.int64)
    assert lib.snmf_online_batch_process_f32(sep._h, P(*[x.ctypes.data for x in x32]), n.ctypes.data, None, None, None, None, None, None,
                                             n_out.ctypes.data) == 7
    assert list(n_out) == [0, 0]
    outs = sep.process(pcms, flush=True)  # ... and the batch they were tried on still runs, with the bits of an untouched one
    B32 = np.zeros((513, 100), np.float32, order="F")
    assert lib.snmf_online_batch_get_basis_f32(sep._h, 1, B32.ctypes.data, 513) == 0  # the fp64 dictionary, rounded
    assert np.array_equal(B32, sep.basis(1).astype(np.float32))
    sep.close()
    for k in range(2):
        assert np.array_equal(outs[k]["x_tilde_f"], good[k][0]) and np.array_equal(outs[k]["x_tilde"], good[k][1])
    # the semi-supervised frame solve
    for key in ("basis_update_N", "basis_update_E"):
        with pytest.raises(SnmfError) as e:
            OnlineBatchSeparator(Bx, Bd, dict(p, **{key: 1}), 2, ctx=gpu_ctx, precision="fp64")
        assert e.value.status == 8
    # a ring beyond the envelope (R_a > 64 column lanes; the fp32 batch takes these); the message names the limit
    rs = np.random.RandomState(0)
    Bx3, Bd3 = rs.random_sample((513, 72)) + 1e-3, rs.random_sample((513, 128)) + 1e-3
    for Ra, ma in ((80, 100), (128, 40)):
        for cf, beta in (("kl", 1.0), ("ed", 2.0)):
            with pytest.raises(SnmfError, match="R_a <= 64, m_a <= 128") as e:
                OnlineBatchSeparator(Bx3, Bd3, dict(p, R_a=Ra, m_a=ma, cf=cf), 2, ctx=gpu_ctx, precision="fp64", Ad_blk0=[np.ones((Ra, ma))] * 2)
            assert e.value.status == 8
            # the kernel's own LDS formula (wbatch64_lds of csrc/snmf_online_batch_f64.h) speaks in the message: the mirror above is it
            need, limit = (int(v) for v in re.search(r"(\d+) bytes of LDS <= (\d+)", e.value.message).groups())
            print("refused ring %d x %d, beta %g: %d bytes of LDS (limit %d)" % (Ra, ma, beta, need, limit))
            assert need == wbatch64_lds(Ra, ma, beta) and limit == 160 * KB
    for beta in (0.0, 1.0, 1.5, 2.0):  # ... and by that formula the envelope's edge fits for every beta
        assert wbatch64_lds(64, 128, beta) <= 160 * KB
    # the fp64 process entries on an fp32 batch -> SNMF_ERR_STATE (7), n_out zeroed; the batch is not harmed
    sep32 = OnlineBatchSeparator(Bx, Bds, p, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    n_out[:] = -1
    assert lib.snmf_online_batch_process_f64(sep32._h, P(*[x.ctypes.data for x in pcms]), n.ctypes.data, None, None, None, None, None, None,
                                             n_out.ctypes.data) == 7
    assert list(n_out) == [0, 0]
    assert lib.snmf_online_batch_restart_f64(sep32._h, 1, sl.ctypes.data, None, None, None) == 7
    o32 = sep32.process(pcms, flush=True)
    sep32.close()
    ref32 = _valid_run(gpu_ctx, precision=None)
    assert all(np.array_equal(o32[k]["x_tilde_f"], ref32[k][0]) for k in range(2))
    # after all of them a valid fp64 batch gives the bits it gave before
    again = _valid_run(gpu_ctx)
    for a, b in zip(again, good):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_the_default_precision_is_the_fp32_batch_unchanged(gpu_ctx):
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings
    g = np.load(os.path.join(GOLD, "online_is16_124frames.npz"))
    s, Bx, Bd = _fixture()
    rs = np.random.RandomState(1)
    H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
    outs = []
    for kw in (dict(), dict(precision="fp32")):
        sep = OnlineBatchSeparator(Bx, Bd, default_settings(), 1, H0=[H0], Ad_blk0=[Ad0], ctx=gpu_ctx, **kw)
        o = sep.process([s], flush=True)[0]
        outs.append((o["x_tilde"], o["x_tilde_f"], sep.basis(0), [tuple(t[k] for k in KEYS) for t in sep.trace(0)]))
        sep.close()
    assert outs[0][1].dtype == np.float32
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]
    dec = outs[0][3]
    assert [t[0] for t in dec] == list(g["n_iter"]) and [int(t[1]) for t in dec] == [int(x) for x in g["trig"]]
    assert [t[2] for t in dec] == list(g["n_up"]) and [t[3] for t in dec] == list(g["adapt_iters"])
