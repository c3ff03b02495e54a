"""Per-class event / noise outputs of the online separators (p.EVENT_RANK / p.NOISE_RANK; snmf_online_set_classes,
snmf_online_batch_set_classes; x_hat_i / d_hat_i of src/bnmf_sep_event_RT_IS16.m:158-202, :350-361).

Reference: tests/online_classes.py, the oracle's own frame function driven in its own loop with the class spectra formed
from each frame's activations and the dictionary the frame solve saw.  Bounds are the project's: REL_OUT = 1e-4
Frobenius-relative per class with the finite mask equal (tests/test_online.py:184-188) for the fp32 separators,
FIX_OVERALL = 1e-9 for the fp64 one (tests/test_online_f64.py), every per-frame decision exact.  With a full partition the
sums over the classes are x_hat's / d_hat's spectra, so nothing but the new outputs may move: that is checked bit for bit.

The GPU fixture (EVENT_RANK = [1, 41, 71], NOISE_RANK = [1, 51] on the 100 + 100 dictionaries; noise class 1 is exactly
the R_a = 50 adapted columns) on the fp64 oracle over 64 frames: all five class signals finite, each 0.50 .. 1.34 times
||x_hat||; a 5e-5 relative perturbation of every activation (the worst per-atom figure of tests/test_online.py) moves a class
by 1 .. 2e-5.  The GPU tests print the measured per-class errors before they assert (docs/WIDENING.md, "Class outputs",
is where they belong; none has been recorded yet).
"""
import numpy as np
import pytest

from oracle.online_oracle import default_params, ntf_sep_event_rt
from online_classes import class_ranges, class_reference
from test_online import REL_OUT, _check_trace, fixture_inputs

EVENT_RANK, NOISE_RANK = [1, 41, 71], [1, 51]
FIX_OVERALL = 1e-9  # tests/test_online_f64.py


def _settings(p, classes=True):
    from se_snmf_nat_amd.online import default_settings
    ps = default_settings()
    ps.update({k: v for k, v in p.items() if k in ps or k == "beta_div"})
    for k in ("EVENT_NUM", "EVENT_RANK", "NOISE_NUM", "NOISE_RANK"):
        ps.pop(k, None)
    if classes:
        ps.update(EVENT_RANK=EVENT_RANK, NOISE_RANK=NOISE_RANK)
    return ps


# ---------------------------------------------------------------- CPU ------------------------------
def test_class_ranges_follow_the_reference():
    assert class_ranges([1, 41, 71], 100) == [(0, 40), (40, 70), (70, 100)]
    assert class_ranges([1], 100) == [(0, 100)]


def test_trivial_partition_is_the_oracles_x_hat_and_d_hat():
    s, Bx, Bd, H0, Ad0 = fixture_inputs(24)
    p = default_params()
    o16, of, Bdn, tr, xh, dh = ntf_sep_event_rt(s, Bx, Bd, p, H0, Ad0, return_trace=True, class_outputs=True)
    ref = class_reference(s, Bx, Bd, p, H0, Ad0)
    assert ref["x_hat_i"].shape == (1, len(xh)) and ref["d_hat_i"].shape == (1, len(dh))
    assert np.array_equal(ref["x_tilde_f"], of) and np.array_equal(ref["x_hat"], xh) and np.array_equal(ref["d_hat"], dh)
    assert np.array_equal(ref["x_hat_i"][0], xh) and np.array_equal(ref["d_hat_i"][0], dh)
    assert np.array_equal(ref["basis"], Bdn)
    assert [t["n_iter"] for t in ref["trace"]] == [t["n_iter"] for t in tr]


def test_with_pow_1_the_classes_sum_to_the_sides():
    """pow = 1: the synthesis is linear in the spectrum, so each side's class signals sum to x_hat / d_hat."""
    s, Bx, Bd, H0, Ad0 = fixture_inputs(24)
    p = dict(default_params(), pow=1)
    ref = class_reference(s, Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK)
    assert ref["x_hat_i"].shape[0] == 3 and ref["d_hat_i"].shape[0] == 2
    assert sum(t["solved"] for t in ref["trace"]) > 0  # the snapshot before the adaptation matters
    for parts, whole in ((ref["x_hat_i"], ref["x_hat"]), (ref["d_hat_i"], ref["d_hat"])):
        assert np.linalg.norm(parts.sum(0) - whole) / np.linalg.norm(whole) < 1e-12


BAD_PARTITIONS = [
    (dict(EVENT_RANK=[2, 41]), 8),            # first rank above 1
    (dict(NOISE_RANK=[3]), 8),
    (dict(EVENT_RANK=[1, 41, 41]), 1),        # equal
    (dict(EVENT_RANK=[1, 71, 41]), 1),        # descending
    (dict(NOISE_RANK=[1, 60, 51]), 1),
    (dict(EVENT_RANK=[1, 101]), 1),           # a start above R_x
    (dict(NOISE_RANK=[1, 51, 101]), 1),
    (dict(EVENT_RANK=[0, 41]), 1),
    (dict(EVENT_RANK=[1, 41, 71], EVENT_NUM=2), 1),
    (dict(NOISE_RANK=[1, 51], NOISE_NUM=3), 1),
    (dict(EVENT_NUM=2), 1),                   # a count without its ranks
    (dict(EVENT_RANK=list(range(1, 35))), 8),  # more classes than the separators take
]


def test_argument_checks_raise_before_any_device_call(monkeypatch):
    """A bad partition is refused in Python before the library is loaded or a context is made, by all three separators and
    whether or not class outputs were asked for."""
    from se_snmf_nat_amd import _lib, online
    from se_snmf_nat_amd.online import OnlineBatchSeparator, OnlineSeparator

    def no_device(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(online, "default_context", no_device)
    s, Bx, Bd, H0, Ad0 = fixture_inputs(2)
    p = _settings(default_params(), classes=False)
    for over, code in BAD_PARTITIONS:
        for cls in (True, False):
            makers = [lambda q: OnlineSeparator(Bx, Bd, q, H0=H0, Ad_blk0=Ad0, class_outputs=cls),
                      lambda q: OnlineSeparator(Bx, Bd, q, H0=H0, Ad_blk0=Ad0, class_outputs=cls, precision="fp64"),
                      lambda q: OnlineBatchSeparator(Bx, Bd, q, 2, class_outputs=cls)]
            for make in makers:
                with pytest.raises(_lib.SnmfError) as e:
                    make(dict(p, **over))
                assert e.value.status == code, over
    # a valid partition gets as far as the library
    with pytest.raises(AssertionError, match="reached the device"):
        OnlineSeparator(Bx, Bd, dict(p, EVENT_RANK=EVENT_RANK, NOISE_RANK=NOISE_RANK, EVENT_NUM=3, NOISE_NUM=2), class_outputs=True)


def test_default_settings_ship_one_class_per_side():
    from se_snmf_nat_amd.online import _class_partition, default_settings
    p = default_settings()
    assert (p["EVENT_NUM"], p["EVENT_RANK"], p["NOISE_NUM"], p["NOISE_RANK"]) == (1, [1], 1, [1])
    assert _class_partition(p, 100, 100) is None and _class_partition({}, 100, 100) is None
    ev, nz = _class_partition(dict(EVENT_RANK=EVENT_RANK, NOISE_RANK=NOISE_RANK), 100, 100)
    assert list(ev) == EVENT_RANK and list(nz) == NOISE_RANK


# ---------------------------------------------------------------- GPU ------------------------------
def _rel_masked(dev, ref):
    """tests/test_online.py:184-188: equal finite masks, Frobenius-relative error over the finite part."""
    assert dev.shape == ref.shape
    ok = np.isfinite(ref)
    assert np.array_equal(np.isfinite(dev), ok)
    return np.linalg.norm(dev[ok] - ref[ok]) / max(np.linalg.norm(ref[ok]), 1e-30)


def _check_classes(out, ref, tol, label):
    errs = [_rel_masked(np.asarray(out[key][i], dtype=np.float64), ref[key][i])
            for key in ("x_hat_i", "d_hat_i") for i in range(ref[key].shape[0])]
    sums = [_rel_masked(np.asarray(out[key], dtype=np.float64), ref[key]) for key in ("x_tilde_f", "x_hat", "d_hat")]
    print(f"[classes] {label}: per-class rel. error " + " ".join(f"{e:.3e}" for e in errs)
          + " | x_tilde x_hat d_hat " + " ".join(f"{e:.3e}" for e in sums))
    assert out["x_hat_i"].shape == ref["x_hat_i"].shape and out["d_hat_i"].shape == ref["d_hat_i"].shape
    assert max(errs) < tol, errs
    assert max(sums) < tol, sums


def _trace_of(ref):
    tr = ref["trace"]
    return [t["n_iter"] for t in tr], [t["trig"] for t in tr], [t["n_up"] for t in tr], [t["adapt_iters"] for t in tr]


def _single(ctx, s, Bx, Bd, ps, H0, Ad0, feed=None, **kw):
    """One OnlineSeparator run: outputs concatenated over the calls, the trace, the final dictionary."""
    from se_snmf_nat_amd.online import OnlineSeparator
    sep = OnlineSeparator(Bx, Bd, ps, H0=H0, Ad_blk0=Ad0, ctx=ctx, **kw)
    parts = [sep.process(s, flush=True)] if feed is None else \
        [sep.process(s[i:i + feed]) for i in range(0, len(s), feed)] + [sep.process(s[:0], flush=True)]
    tr = sep.trace()
    Bn = sep.mel_basis() if sep.mel else sep.basis()
    sep.close()
    out = {k: np.concatenate([q[k] for q in parts], axis=-1) for k in parts[0]}
    return out, tr, Bn


@pytest.mark.gpu
def test_fp32_classes_match_the_reference(gpu_ctx, capsys):
    s, Bx, Bd, H0, Ad0 = fixture_inputs(60)
    p = default_params()
    ref = class_reference(s, Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK)
    out, tr, Bn = _single(gpu_ctx, s, Bx, Bd, _settings(p), H0, Ad0, class_outputs=True)
    assert out["x_hat_i"].dtype == np.float32 and out["d_hat_i"].dtype == np.float32
    assert sum(t["solved"] for t in tr) > 0
    _check_trace(tr, *_trace_of(ref))
    with capsys.disabled():
        _check_classes(out, ref, REL_OUT, "fp32 DFT")


@pytest.mark.gpu
@pytest.mark.parametrize("melconv", [1, 0], ids=["MelConv1", "MelConv0-coupled"])
def test_fp32_mel_classes_match_the_reference(gpu_ctx, melconv, capsys):
    """The setup of tests/test_online.py::test_device_mel_mode_matches_the_oracle."""
    from oracle.frontend_oracle import mel_matrix
    s, Bx, Bd, H0, Ad0 = fixture_inputs(40)
    p = dict(default_params(), B_sep_mode="Mel", MelConv=melconv, F_order=64)
    melmat = mel_matrix(p["fs"], 64, p["fftlength"], 1.0, p["fs"] / 2).T
    BM = melmat @ np.concatenate([Bx, Bd], axis=1)
    BM = BM / np.sqrt((BM ** 2).sum(0)) + 1e-9
    mel = dict(B_Mel_x=BM[:, :100], B_Mel_d=BM[:, 100:], melmat=melmat)
    ref = class_reference(s, Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK, mel=mel)
    out, tr, _ = _single(gpu_ctx, s, Bx, Bd, _settings(p), H0, Ad0, class_outputs=True, B_Mel_x=mel["B_Mel_x"], B_Mel_d=mel["B_Mel_d"])
    _check_trace(tr, *_trace_of(ref))
    assert sum(t["solved"] for t in tr) > 5
    with capsys.disabled():
        _check_classes(out, ref, REL_OUT, f"fp32 Mel MelConv={melconv}")


@pytest.mark.gpu
def test_fp32_semi_supervised_classes_match_the_reference(gpu_ctx, capsys):
    """basis_update_N: the solve's private W is discarded; the classes are reconstructed from the unmodified dictionary."""
    s, Bx, Bd, H0, Ad0 = fixture_inputs(36)
    p = dict(default_params(), basis_update_N=1, max_iter=30)
    ref = class_reference(s, Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK)
    out, tr, _ = _single(gpu_ctx, s, Bx, Bd, _settings(p), H0, Ad0, class_outputs=True)
    _check_trace(tr, *_trace_of(ref))
    with capsys.disabled():
        _check_classes(out, ref, REL_OUT, "fp32 semi-supervised")


@pytest.mark.gpu
def test_fp64_classes_match_the_reference(gpu_ctx, capsys):
    """The 124-frame fixture of tests/test_online_f64.py::test_class_outputs_match_the_oracle."""
    s, Bx, Bd, H0, Ad0 = fixture_inputs()
    p = default_params()
    ref = class_reference(s, Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK)
    out, tr, Bn = _single(gpu_ctx, s, Bx, Bd, _settings(p), H0, Ad0, class_outputs=True, precision="fp64")
    for key in ("x_tilde_f", "x_hat", "d_hat", "x_hat_i", "d_hat_i"):
        assert out[key].dtype == np.float64, key
    _check_trace(tr, *_trace_of(ref))
    with capsys.disabled():
        _check_classes(out, ref, FIX_OVERALL, "fp64 DFT")


@pytest.mark.gpu
def test_fixed_dictionary_classes_match_the_reference(gpu_ctx, capsys):
    """adapt_train_N = 0: the frame solves of a call run in one launch, and so do their class spectra (all three separators)."""
    s, Bx, Bd, H0, Ad0 = fixture_inputs(36)
    p = dict(default_params(), adapt_train_N=0)
    ref = class_reference(s, Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK)
    for kw, tol in ((dict(), REL_OUT), (dict(precision="fp64"), FIX_OVERALL)):
        out, tr, _ = _single(gpu_ctx, s, Bx, Bd, _settings(p), H0, Ad0, class_outputs=True, **kw)
        _check_trace(tr, *_trace_of(ref))
        with capsys.disabled():
            _check_classes(out, ref, tol, f"fixed dictionary {kw.get('precision', 'fp32')}")
    res = _batch(gpu_ctx, [s, s[:160 * 20]], Bx, [Bd, Bd], _settings(p), [H0, H0], None, class_outputs=True)
    with capsys.disabled():
        _check_classes(res[0][0], ref, REL_OUT, "fixed dictionary batch stream 0")
    ref1 = class_reference(s[:160 * 20], Bx, Bd, p, H0, Ad0, EVENT_RANK, NOISE_RANK)
    with capsys.disabled():
        _check_classes(res[1][0], ref1, REL_OUT, "fixed dictionary batch stream 1")


def _batch(ctx, pcms, Bx, Bds, ps, H0s, Ads, feed=None, **kw):
    """One OnlineBatchSeparator run: per stream (outputs, trace, final dictionary)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    S = len(pcms)
    sep = OnlineBatchSeparator(Bx, Bds, ps, S, H0=H0s, Ad_blk0=Ads, ctx=ctx, **kw)
    calls = [sep.process(chunk, flush=fl) for chunk, fl in (feed or [(pcms, True)])]
    res = []
    for k in range(S):
        out = {key: np.concatenate([c[k][key] for c in calls], axis=-1) for key in calls[0][k]}
        res.append((out, sep.trace(k), sep.mel_basis(k) if sep.mel else sep.basis(k)))
    sep.close()
    return res


def _same(a, b):
    assert a[0].keys() == b[0].keys()
    for key in a[0]:
        assert np.array_equal(a[0][key], b[0][key]), key
    assert a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_batch_classes_match_the_reference_per_stream(gpu_ctx, capsys):
    from test_online_batch import _streams
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams(30, S=3)
    res = _batch(gpu_ctx, pcms, Bx, Bds, _settings(p), H0s, Ads, class_outputs=True)
    for k in range(3):
        ref = class_reference(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], EVENT_RANK, NOISE_RANK)
        _check_trace(res[k][1], *_trace_of(ref))
        with capsys.disabled():
            _check_classes(res[k][0], ref, REL_OUT, f"batch DFT stream {k}")
    assert sum(t["solved"] for t in res[0][1]) > 0


@pytest.mark.gpu
def test_batch_mel_classes_match_the_reference_per_stream(gpu_ctx, capsys):
    from test_online_batch_mel import _mel_params, _mel_streams, _melmat
    p = _mel_params(1)
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(30, S=3, p=p)
    res = _batch(gpu_ctx, pcms, Bx, Bds, _settings(p), H0s, Ads, class_outputs=True, B_Mel_x=BMx, B_Mel_d=BMds)
    for k in range(3):
        mel = dict(B_Mel_x=BMx, B_Mel_d=BMds[k], melmat=_melmat(p, p["F_order"]))
        ref = class_reference(pcms[k], Bx, Bds[k], p, H0s[k], Ads[k], EVENT_RANK, NOISE_RANK, mel=mel)
        _check_trace(res[k][1], *_trace_of(ref))
        with capsys.disabled():
            _check_classes(res[k][0], ref, REL_OUT, f"batch Mel stream {k}")


@pytest.mark.gpu
def test_batch_class_bits_do_not_depend_on_the_company(gpu_ctx):
    """tests/test_online_batch.py::test_bits_do_not_depend_on_the_company, class outputs included."""
    from test_online_batch import _streams
    ps = _settings(default_params())
    pcms, Bx, Bds, H0s, Ads = _streams(30)
    alone = _batch(gpu_ctx, pcms[:1], Bx, Bds[:1], ps, H0s[:1], Ads[:1], class_outputs=True)[0]
    full = _batch(gpu_ctx, pcms, Bx, Bds, ps, H0s, Ads, class_outputs=True)
    order = [3, 1, 4, 0, 2]
    perm = _batch(gpu_ctx, [pcms[i] for i in order], Bx, [Bds[i] for i in order], ps, [H0s[i] for i in order],
                  [Ads[i] for i in order], class_outputs=True)
    assert alone[0]["x_hat_i"].shape[0] == 3 and alone[0]["d_hat_i"].shape[0] == 2 and alone[0]["x_hat_i"].shape[1] > 0
    _same(alone, full[0])
    _same(alone, perm[order.index(0)])
    for j, i in enumerate(order):  # every stream, not only the first
        _same(perm[j], full[i])


@pytest.mark.gpu
def test_batch_restart_gives_a_fresh_batchs_class_bits(gpu_ctx):
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    from test_online_batch import _streams
    ps = _settings(default_params())
    pcms, Bx, Bds, H0s, Ads = _streams(30, S=3)
    fresh = _batch(gpu_ctx, pcms, Bx, Bds, ps, H0s, Ads, class_outputs=True)
    # stream 1 first runs another recording, then is restarted with stream 1's inputs while the others start theirs
    sep = OnlineBatchSeparator(Bx, [Bds[0], Bds[2], Bds[2]], ps, 3, H0=[H0s[0], H0s[2], H0s[2]], Ad_blk0=[Ads[0], Ads[2], Ads[2]],
                               ctx=gpu_ctx, class_outputs=True)
    empty = pcms[0][:0]
    first = sep.process([empty, pcms[2], empty], flush=[False, True, False])
    assert first[1]["x_hat_i"].shape[1] > 0
    sep.restart(1, B_DFT_d=Bds[1].astype(np.float32).astype(np.float64), H0=H0s[1], Ad_blk0=Ads[1])
    outs = sep.process(pcms, flush=True)
    for k in range(3):
        for key in ("x_tilde_f", "x_tilde", "x_hat", "d_hat", "x_hat_i", "d_hat_i"):
            assert np.array_equal(outs[k][key], fresh[k][0][key]), (k, key)
    sep.close()


@pytest.mark.gpu
def test_nothing_else_moves(gpu_ctx):
    """With the partition and with the keys absent: x_tilde, x_tilde_f, x_hat, d_hat, the final dictionary and the whole trace
    are the same bits, on each of the three separators."""
    from test_online_batch import _streams
    s, Bx, Bd, H0, Ad0 = fixture_inputs(60)
    p = default_params()
    keys = ("x_tilde", "x_tilde_f", "x_hat", "d_hat")
    for kw in (dict(), dict(precision="fp64")):
        a = _single(gpu_ctx, s, Bx, Bd, _settings(p), H0, Ad0, class_outputs=True, **kw)
        b = _single(gpu_ctx, s, Bx, Bd, _settings(p, classes=False), H0, Ad0, class_outputs=True, **kw)
        assert a[0]["x_hat_i"].shape[0] == 3 and b[0]["x_hat_i"].shape[0] == 1
        assert np.array_equal(b[0]["x_hat_i"][0], b[0]["x_hat"]) and np.array_equal(b[0]["d_hat_i"][0], b[0]["d_hat"])
        for key in keys:
            assert np.array_equal(a[0][key], b[0][key]), (kw, key)
        assert a[1] == b[1] and np.array_equal(a[2], b[2])
    pcms, Bx, Bds, H0s, Ads = _streams(30, S=3)
    a = _batch(gpu_ctx, pcms, Bx, Bds, _settings(p), H0s, Ads, class_outputs=True)
    b = _batch(gpu_ctx, pcms, Bx, Bds, _settings(p, classes=False), H0s, Ads, class_outputs=True)
    for k in range(3):
        for key in keys:
            assert np.array_equal(a[k][0][key], b[k][0][key]), (k, key)
        assert a[k][1] == b[k][1] and np.array_equal(a[k][2], b[k][2])


@pytest.mark.gpu
def test_feeding_in_chunks_gives_the_same_class_bits(gpu_ctx):
    s, Bx, Bd, H0, Ad0 = fixture_inputs(40)
    s = np.concatenate([s, s[:33]])  # trailing partial hop
    ps = _settings(default_params())
    for kw in (dict(), dict(precision="fp64")):
        whole = _single(gpu_ctx, s, Bx, Bd, ps, H0, Ad0, class_outputs=True, **kw)
        assert whole[0]["x_hat_i"].shape == (3, len(whole[0]["x_hat"]))
        for chunk in (160, 1000, 57):
            fed = _single(gpu_ctx, s, Bx, Bd, ps, H0, Ad0, feed=chunk, class_outputs=True, **kw)
            for key in ("x_hat_i", "d_hat_i", "x_hat", "d_hat", "x_tilde_f"):
                assert np.array_equal(whole[0][key], fed[0][key]), (kw, chunk, key)
            assert whole[1] == fed[1] and np.array_equal(whole[2], fed[2])


def _i32(v):
    return np.array(v, dtype=np.int32)


@pytest.mark.gpu
def test_error_and_state_codes(gpu_ctx):
    """The C entries' own checks (the Python separators refuse the same partitions before they get here); after each refusal a
    valid separator still runs and gives the bits it gave before."""
    from se_snmf_nat_amd import _lib
    from se_snmf_nat_amd.online import OnlineBatchSeparator, OnlineSeparator
    lib = _lib.load()
    s, Bx, Bd, H0, Ad0 = fixture_inputs(12)
    plain, ps = _settings(default_params(), classes=False), _settings(default_params())

    def valid_run():
        return _single(gpu_ctx, s, Bx, Bd, ps, H0, Ad0, class_outputs=True)[0]
    before = valid_run()

    def still_the_same():
        now = valid_run()
        for key in before:
            assert np.array_equal(before[key], now[key]), key

    def set_classes(sep, ev, nz, batch=False, n_ev=None, n_nz=None):
        ev, nz = _i32(ev), _i32(nz)
        fn = lib.snmf_online_batch_set_classes if batch else lib.snmf_online_set_classes
        return fn(sep._h, len(ev) if n_ev is None else n_ev, ev.ctypes.data, len(nz) if n_nz is None else n_nz, nz.ctypes.data)

    cases = [(([2, 41], [1]), 8), (([1], [2]), 8), (([1, 71, 41], [1]), 1), (([1, 41, 41], [1]), 1), (([1, 101], [1]), 1),
             (([1], [1, 51, 101]), 1), (([0, 41], [1]), 1), ((list(range(1, 35)), [1]), 8)]
    makers = [(lambda: OnlineSeparator(Bx, Bd, plain, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, class_outputs=True), False),
              (lambda: OnlineSeparator(Bx, Bd, plain, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, class_outputs=True, precision="fp64"), False),
              (lambda: OnlineBatchSeparator(Bx, Bd, plain, 2, ctx=gpu_ctx, class_outputs=True), True)]
    for make, batch in makers:
        sep = make()
        for (ev, nz), code in cases:
            assert set_classes(sep, ev, nz, batch) == code, (ev, nz)
        assert set_classes(sep, [1], [1], batch, n_ev=0) == 1
        assert set_classes(sep, [1, 41], [1, 51], batch) == 0       # 16 classes per side are within the limit, too
        assert set_classes(sep, list(range(1, 17)), list(range(1, 33, 2)), batch) == 0
        assert set_classes(sep, EVENT_RANK, NOISE_RANK, batch) == 0  # the last call holds
        out = sep.process([s, s] if batch else s, flush=True)
        assert set_classes(sep, EVENT_RANK, NOISE_RANK, batch) == 7  # after the first sample: SNMF_ERR_STATE
        sep.close()
        still_the_same()
    # the plain process entries on a separator that has classes: everything but the class signals
    sep = OnlineSeparator(Bx, Bd, plain, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, class_outputs=True)
    assert set_classes(sep, EVENT_RANK, NOISE_RANK) == 0
    out = sep.process(s, flush=True)  # (this Python object knows of no partition: it calls snmf_online_process_f32)
    sep.close()
    for key in ("x_tilde", "x_tilde_f", "x_hat", "d_hat"):
        assert np.array_equal(out[key], before[key]), key
    # a separator made without class_outputs
    for make, batch in ((lambda: OnlineSeparator(Bx, Bd, plain, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx), False),
                        (lambda: OnlineSeparator(Bx, Bd, plain, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision="fp64"), False),
                        (lambda: OnlineBatchSeparator(Bx, Bd, plain, 2, ctx=gpu_ctx), True)):
        sep = make()
        assert set_classes(sep, EVENT_RANK, NOISE_RANK, batch) == 7
        sep.close()
    # the Python separators raise the same codes, and a partition in p without class_outputs is checked and otherwise ignored
    with pytest.raises(_lib.SnmfError) as e:
        OnlineSeparator(Bx, Bd, dict(plain, EVENT_RANK=[2]), H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, class_outputs=True)
    assert e.value.status == 8
    sep = OnlineSeparator(Bx, Bd, ps, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx)
    assert sorted(sep.process(s, flush=True)) == ["x_tilde", "x_tilde_f"]
    sep.close()
    still_the_same()
