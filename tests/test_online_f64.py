"""The fp64 mode of the online separator: OnlineSeparator(..., precision="fp64"), snmf_online_create_f64 / _process_f64.

The online loop is a feedback system (activations -> adapted noise dictionary -> next activations).  The fp32 device path
leaves the fp64 oracle's trajectory after a few hundred frames (tests/test_online.py pins 300); the fp64 mode keeps every
step from PCM to the fed-back dictionary in fp64 and is pinned here over a whole recording: `lm_in` of refwav_pairs.npz,
the reference's own wav/LM_in.wav, 1777 frames / 17.7 s, 913 adaptation solves.

Where the bounds come from (scripts/online_f64_sensitivity.py, profiles/online_f64_sensitivity.md -- the fp64 ORACLE run
against itself with B_DFT_x, B_DFT_d, H0 multiplied by 1 + eps * N(0,1); nothing here is read off the device):
  lm_in: decisions hold for eps <= 1e-11 and the response is linear in eps up to there.  The bounds below are the oracle's
  response to eps = 1e-12 -- one decade inside the range where decisions hold, three to four decades above fp64 unit
  roundoff: signal overall 6e-10, per-hop maximum 1.2e-7, final B_DFT_d 8e-8; int16: at most 2 samples by 1 LSB (.5 ties).
  124-frame fixture: signal within 1e-9 overall; the oracle's response to eps = 1e-13 on it is 1.3e-12 (770 times below).
  The final dictionary of a 124-frame variant is held to 1e-8: ten times the signal bound, because the oracle's dictionary
  response on this fixture is ten times its signal response (1.4e-11 against 1.3e-12 at eps = 1e-13).

Measured on an MI355X (each test prints its figures before it asserts, pytest -s):
  lm_in: every decision of all 1777 frames equal; 0 int16 samples differ; signal overall 1.27e-12, per-hop maximum
  2.96e-10, final B_DFT_d 1.84e-10 -- 470, 400 and 430 times inside the bounds, the oracle's own response to eps ~ 1e-15.
  124-frame variants: decisions equal, 0 int16 samples differ; signal 4e-16 .. 2.2e-13 (largest: ED with adaptation),
  x_hat / d_hat <= 2.9e-13, final B_DFT_d <= 1.0e-12.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.online_oracle import default_params, ntf_sep_event_rt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("n_iter", "trig", "n_up", "adapt_iters")
HOP = 160
# lm_in (see the module docstring)
LM_OVERALL, LM_PER_HOP, LM_BASIS, LM_I16_TIES = 6e-10, 1.2e-7, 8e-8, 2
# 124-frame fixture
FIX_OVERALL, FIX_BASIS = 1e-9, 1e-8


def _dictionaries_and_draws():
    B = np.load(os.path.join(GOLD, "ref_data.npz"))["B"].astype(np.float64)
    rs = np.random.RandomState(1)  # H0 / Ad_blk0 of tests/test_online.py's fixture_inputs()
    H0 = rs.random_sample(200)
    Ad0 = rs.random_sample((50, 100))
    return B[:, :100], B[:, 100:], H0, Ad0


def lm_inputs(n_hops=None):
    s = np.load(os.path.join(GOLD, "refwav_pairs.npz"))["lm_in"]
    if n_hops is not None:
        s = s[:n_hops * HOP]
    return (s,) + _dictionaries_and_draws()


def fixture_inputs():
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"]
    return (s,) + _dictionaries_and_draws()


def _decisions(tr):
    return {k: np.array([int(t[k]) for t in tr]) for k in KEYS}


@pytest.fixture(scope="module")
def lm_oracle():
    """The fp64 oracle on lm_in, once for the module (about 30 s)."""
    s, Bx, Bd, H0, Ad0 = lm_inputs()
    o16, of, Bdn, tr = ntf_sep_event_rt(s, Bx, Bd, default_params(), H0, Ad0, return_trace=True)
    return dict(i16=o16, f=of, B=Bdn, dec=_decisions(tr))


# ---------------------------------------------------------------- CPU ------------------------------
def test_oracle_decisions_on_lm_in_equal_the_committed_fixture(lm_oracle):
    """A drift of the oracle (NumPy / BLAS version, an edit) shows up without a GPU: its 1777 x 4 decisions for lm_in are
    committed (tests/golden/make_golden_online_f64.py)."""
    g = np.load(os.path.join(GOLD, "online_f64", "lm_decisions.npz"))
    assert len(lm_oracle["dec"]["n_iter"]) == 1777 and len(lm_oracle["i16"]) == 283840
    for k in KEYS:
        assert np.array_equal(lm_oracle["dec"][k], g[k].astype(int)), k
    assert int((lm_oracle["dec"]["adapt_iters"] > 0).sum()) > 900  # the recording exercises the adaptation throughout


def test_unknown_precision_is_a_value_error():
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings, ntf_sep_event_rt as dev_rt
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    with pytest.raises(ValueError, match="precision"):
        OnlineSeparator(Bx, Bd, default_settings(), H0=H0, Ad_blk0=Ad0, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        dev_rt(s[:HOP], Bx, Bd, default_settings(), H0=H0, Ad_blk0=Ad0, precision="double")


# ---------------------------------------------------------------- GPU ------------------------------
def _settings(p):
    from se_snmf_nat_amd.online import default_settings
    ps = default_settings()
    ps.update({k: v for k, v in p.items() if k in ps or k == "beta_div"})
    return ps


def _device64(s, Bx, Bd, p, H0, Ad0, **kw):
    from se_snmf_nat_amd.online import OnlineSeparator
    sep = OnlineSeparator(Bx, Bd, _settings(p), H0=H0, Ad_blk0=Ad0, precision="fp64", **kw)
    out = sep.process(s, flush=True)
    tr, Bn = sep.trace(), sep.basis()
    sep.close()
    return out, _decisions(tr), Bn


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.gpu
def test_lm_in_whole_recording_holds_the_oracles_trajectory(gpu_ctx, lm_oracle):
    """The hard pin: every decision of all 1777 frames, the int16 stream, the float signal and the final dictionary."""
    s, Bx, Bd, H0, Ad0 = lm_inputs()
    out, dec, Bn = _device64(s, Bx, Bd, default_params(), H0, Ad0, ctx=gpu_ctx)
    ref = lm_oracle
    xf = out["x_tilde_f"]
    assert xf.dtype == np.float64 and Bn.dtype == np.float64
    assert len(xf) == len(ref["f"]) == 283840 and len(dec["n_iter"]) == 1777
    first = next((i + 1 for i in range(1777) if any(dec[k][i] != ref["dec"][k][i] for k in KEYS)), None)
    d = xf - ref["f"]
    per = np.array([np.linalg.norm(d[j * HOP:(j + 1) * HOP]) / max(np.linalg.norm(ref["f"][j * HOP:(j + 1) * HOP]), 1.0)
                    for j in range(len(xf) // HOP)])
    di = np.abs(out["x_tilde"].astype(int) - ref["i16"].astype(int))
    overall, basis = _rel(xf, ref["f"]), _rel(Bn, ref["B"])
    print("lm_in fp64: first differing decision %s; int16 differing %d (max %d LSB); signal overall %.3g, per-hop max %.3g; "
          "final B_DFT_d %.3g" % (first, int((di > 0).sum()), int(di.max()), overall, per.max(), basis))
    for k in KEYS:
        assert np.array_equal(dec[k], ref["dec"][k]), (k, first)
    assert int((di > 0).sum()) <= LM_I16_TIES and di.max() <= 1
    assert overall <= LM_OVERALL
    assert per.max() <= LM_PER_HOP
    assert basis <= LM_BASIS


VARIANTS = [
    dict(ENHANCE_METHOD="Wiener"),
    dict(blk_sparse=0),
    dict(adapt_train_N=0),
    dict(preemph=0.92, pow=1),
    dict(cf="ed", sparsity=50.0),
    dict(cf="ed", sparsity=50.0, adapt_train_N=0),
    dict(blk_gap=1, P_len_l=4, init_N_len=3),
    dict(conv_eps=0.0, max_iter=12),
    dict(cf="x", beta_div=1.5, adapt_train_N=0, conv_eps=0.0, max_iter=30),  # generic beta (src/sparse_nmf.m:200-205), update only
    # ... and with the stop test, without and with the adaptation solve (the generic branch of the objective in k_hsolve64 and
    # k_wadapt64 decides n_iter / adapt_iters here).  These two are compared on the 120 frames that carry signal, the stream
    # fed WITHOUT the flush: on the delay+1 all-zero flush frames (src/NTF_sep_event_RT.m:69-76) Lam = v = the 1e-9 floor,
    # the divergence is exactly 0, and what the oracle computes for it is the rounding residue of NumPy's pow (-4.3e-27) --
    # its stop at iteration 7 of those frames is the cost turning NEGATIVE (relative change -0.07 < conv_eps), a decision
    # made by that residue alone and not one that fp64 arithmetic defines.  The flush frames trigger no adaptation, so the
    # oracle's final dictionary is the one after frame 120.
    dict(cf="x", beta_div=1.5, adapt_train_N=0),
    dict(cf="x", beta_div=1.5),
]


def _signal_frames_only(var):
    return var.get("cf") == "x" and var.get("conv_eps", 1e-3) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(f"{k}={v[k]}" for k in v))
def test_variants_on_the_124_frame_fixture(gpu_ctx, var):
    """Decisions exact, the signal and both class outputs within 1e-9 overall (the fp32 path: 3e-6, ED 7e-4)."""
    from se_snmf_nat_amd.online import OnlineSeparator
    p = dict(default_params(), **var)
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    o16, of, Bdn, tr, xh, dh = ntf_sep_event_rt(s, Bx, Bd, p, H0, Ad0, return_trace=True, class_outputs=True)
    ref = _decisions(tr)
    assert len(tr) == 124
    if _signal_frames_only(var):
        n_fr = 124 - (p["delay"] + 1)
        assert not ref["trig"][n_fr:].any()  # the oracle's dictionary after frame 120 is its final one
        sep = OnlineSeparator(Bx, Bd, _settings(p), H0=H0, Ad_blk0=Ad0, precision="fp64", ctx=gpu_ctx, class_outputs=True)
        out = sep.process(s, flush=False)
        dec, Bn = _decisions(sep.trace()), sep.basis()
        sep.close()
        n_s = (n_fr - p["delay"]) * HOP
        ref = {k: ref[k][:n_fr] for k in KEYS}
        o16, of, xh, dh = o16[:n_s], of[:n_s], xh[:n_s], dh[:n_s]
        assert len(np.unique(ref["n_iter"])) > 10 and ref["n_iter"].max() <= 100  # the stop test decides these frames
    else:
        out, dec, Bn = _device64(s, Bx, Bd, p, H0, Ad0, ctx=gpu_ctx, class_outputs=True)
    errs = []
    for k in KEYS:
        assert np.array_equal(dec[k], ref[k]), k
    for name, rf in (("x_tilde_f", of), ("x_hat", xh), ("d_hat", dh)):
        dev = out[name]
        assert dev.dtype == np.float64 and len(dev) == len(rf)
        ok = np.isfinite(rf)  # a silent tail can be 0/0 in the reference's own formulas (:230): NaN on both sides
        assert np.array_equal(np.isfinite(dev), ok)
        errs.append(_rel(dev[ok], rf[ok]))
    di = np.abs(out["x_tilde"].astype(int) - o16.astype(int))
    print("variant %s: signal %.3g, x_hat %.3g, d_hat %.3g, B_DFT_d %.3g, int16 differing %d" % (var, *errs, _rel(Bn, Bdn), int((di > 0).sum())))
    assert max(errs) <= FIX_OVERALL
    assert di.max() <= 1 and int((di > 0).sum()) <= LM_I16_TIES
    assert _rel(Bn, Bdn) <= FIX_BASIS


@pytest.mark.gpu
def test_geometries_beyond_the_adaptation_kernel_are_refused(gpu_ctx):
    """With adaptation on, the fp64 adaptation solve is one cooperative launch of at most 80 workgroups with R_a <= 64:
    fftlength > 1024 or R_a > 64 -> SNMF_ERR_UNSUPPORTED (8) with a message, and a valid separator created afterwards
    gives the bits it gave before."""
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings
    good = _run_short(gpu_ctx, precision="fp64")
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    p = default_settings()
    rs = np.random.RandomState(3)
    with pytest.raises(SnmfError, match="adaptation solve") as e:  # R_a = 80 > 64
        OnlineSeparator(Bx, Bd, dict(p, R_a=80), H0=H0, Ad_blk0=rs.random_sample((80, 100)), ctx=gpu_ctx, precision="fp64")
    assert e.value.status == 8
    fft, sz, hop = 2048, 1280, 320  # F = 1025: 129 row blocks > 80
    n = np.arange(sz)
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / sz))
    B2 = rs.random_sample((fft // 2 + 1, 200)) + 1e-3
    q = dict(p, fftlength=fft, framelength=sz, frameshift=hop, win_STFT=win, win_ISTFT=win.copy(), overlapscale=2 * hop / sz)
    with pytest.raises(SnmfError, match="adaptation solve") as e:
        OnlineSeparator(B2[:, :100], B2[:, 100:], q, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64")
    assert e.value.status == 8
    again = _run_short(gpu_ctx, precision="fp64")
    assert np.array_equal(again["x_tilde_f"], good["x_tilde_f"]) and np.array_equal(again["x_tilde"], good["x_tilde"])


@pytest.mark.gpu
def test_class_outputs_match_the_oracle(gpu_ctx):
    """x_hat / d_hat of the shipped settings (the variants above carry them too), and the float outputs' type."""
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    o16, of, Bdn, tr, xh, dh = ntf_sep_event_rt(s, Bx, Bd, default_params(), H0, Ad0, return_trace=True, class_outputs=True)
    out, dec, Bn = _device64(s, Bx, Bd, default_params(), H0, Ad0, ctx=gpu_ctx, class_outputs=True)
    for k in KEYS:
        assert np.array_equal(dec[k], _decisions(tr)[k]), k
    assert np.array_equal(out["x_tilde"], o16)
    for name, rf in (("x_tilde_f", of), ("x_hat", xh), ("d_hat", dh)):
        assert out[name].dtype == np.float64
        print("class outputs: %s %.3g" % (name, _rel(out[name], rf)))
        assert _rel(out[name], rf) <= FIX_OVERALL
    assert _rel(Bn, Bdn) <= FIX_BASIS


@pytest.mark.gpu
def test_feeding_lm_in_in_chunks_gives_the_same_bits(gpu_ctx):
    from se_snmf_nat_amd.online import default_settings, ntf_sep_event_rt as dev_rt
    s, Bx, Bd, H0, Ad0 = lm_inputs(400)
    p = default_settings()
    a16, af, aB = dev_rt(s, Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64")
    assert len(a16) == (400 + p["delay"] + 1 - p["delay"]) * HOP
    for chunk in (160, 1000, 57):
        b16, bf, bB = dev_rt(s, Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, chunk=chunk, precision="fp64")
        assert np.array_equal(a16, b16) and np.array_equal(af, bf) and np.array_equal(aB, bB), chunk


def _run_short(gpu_ctx, **kw):
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    sep = OnlineSeparator(Bx, Bd, default_settings(), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, **kw)
    out = sep.process(s[:30 * HOP], flush=True)
    sep.close()
    return out


@pytest.mark.gpu
def test_refusals_and_a_valid_separator_afterwards(gpu_ctx, lib):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    p = default_settings()
    good = _run_short(gpu_ctx, precision="fp64")
    # Mel mode: the Python mirror and snmf_online_set_mel on an fp64 handle -> SNMF_ERR_UNSUPPORTED (8)
    with pytest.raises(SnmfError) as e:
        OnlineSeparator(Bx, Bd, dict(p, B_sep_mode="Mel"), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64",
                        B_Mel_x=np.ones((64, 100)), B_Mel_d=np.ones((64, 100)))
    assert e.value.status == 8
    sep = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64")
    melmat = np.ones((64, 513), np.float32)
    BM = np.ones((64, 100), np.float32, order="F")
    assert lib.snmf_online_set_mel(sep._h, 64, 1, melmat.ctypes.data, BM.ctypes.data, BM.ctypes.data) == 8
    assert b"Mel" in lib.snmf_last_error()
    # ... and the separator it was tried on still runs, with the bits of an untouched one
    out = sep.process(s[:30 * HOP], flush=True)
    sep.close()
    assert np.array_equal(out["x_tilde_f"], good["x_tilde_f"]) and np.array_equal(out["x_tilde"], good["x_tilde"])
    # semi-supervised frame solve
    with pytest.raises(SnmfError) as e:
        OnlineSeparator(Bx, Bd, dict(p, basis_update_N=1), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64")
    assert e.value.status == 8
    with pytest.raises(SnmfError) as e:
        OnlineSeparator(Bx, Bd, dict(p, basis_update_E=1), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64")
    assert e.value.status == 8
    # snmf_online_process_f64 on an fp32 separator -> SNMF_ERR_STATE (7); the separator is not harmed
    sep32 = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx)
    x = np.ascontiguousarray(s[:30 * HOP], dtype=np.float64)
    of = np.zeros(40 * HOP)
    n = C.c_int64(-1)
    assert lib.snmf_online_process_f64(sep32._h, x.ctypes.data, x.size, 1, of.ctypes.data, None, None, None, of.size, C.byref(n)) == 7
    assert n.value == 0
    out32 = sep32.process(s[:30 * HOP], flush=True)
    B64 = sep32.basis_f64()  # get_basis_f64 works on both kinds: the fp32 separator's fp64 master
    assert np.array_equal(B64.astype(np.float32), sep32.basis().astype(np.float32))
    sep32.close()
    assert np.array_equal(out32["x_tilde_f"], _run_short(gpu_ctx)["x_tilde_f"])
    # after all the refusals a valid fp64 separator gives the same bits as before them
    again = _run_short(gpu_ctx, precision="fp64")
    assert np.array_equal(again["x_tilde_f"], good["x_tilde_f"])


@pytest.mark.gpu
def test_process_f32_on_an_fp64_separator_rounds_the_fp64_outputs(gpu_ctx, lib):
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    good = _run_short(gpu_ctx, precision="fp64")
    sep = OnlineSeparator(Bx, Bd, default_settings(), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64")
    x = np.ascontiguousarray(s[:30 * HOP], dtype=np.float32)
    of = np.zeros(40 * HOP, np.float32)
    o16 = np.zeros(40 * HOP, np.int16)
    n = C.c_int64()
    assert lib.snmf_online_process_f32(sep._h, x.ctypes.data, x.size, 1, of.ctypes.data, o16.ctypes.data, None, None, of.size, C.byref(n)) == 0
    B32 = np.zeros((513, 100), np.float32, order="F")
    assert lib.snmf_online_get_basis_f32(sep._h, B32.ctypes.data, 513) == 0
    B64 = sep.basis()
    sep.close()
    assert n.value == len(good["x_tilde_f"])
    assert np.array_equal(of[:n.value], good["x_tilde_f"].astype(np.float32))
    assert np.array_equal(o16[:n.value], good["x_tilde"])
    assert np.array_equal(B32, B64.astype(np.float32))


@pytest.mark.gpu
def test_the_default_precision_is_the_fp32_path_unchanged(gpu_ctx):
    from se_snmf_nat_amd.online import OnlineSeparator, default_settings
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    outs = []
    for kw in (dict(), dict(precision="fp32")):
        sep = OnlineSeparator(Bx, Bd, default_settings(), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, **kw)
        o = sep.process(s, flush=True)
        outs.append((o["x_tilde"], o["x_tilde_f"], sep.basis(), [tuple(t[k] for k in KEYS) for t in sep.trace()]))
        sep.close()
    assert outs[0][1].dtype == np.float32
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]
    g = np.load(os.path.join(GOLD, "online_is16_124frames.npz"))  # ... and still the golden run's decisions
    assert [t[0] for t in outs[0][3]] == list(g["n_iter"]) and [t[3] for t in outs[0][3]] == list(g["adapt_iters"])
