"""CPU tests of the training-signal assembly (assemble_training_signals, run_basis_train_assembled_batch,
run_basis_train_clips_batch; snmf_train_signals_*, snmf_run_basis_train_signals_batch_*): the NumPy restatement of
run_basis_train.m:16-57 (tests/assemble_cases.py) against hand-built cases, the Python-side errors before the library is loaded,
the C names in the header and in the binding, the C entries' refusals without a device, the exports, and the condition that keeps
the GPU comparison honest: no frame quotient of a GPU case lies within 1e-9 of the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assemble_cases as ac
import train_batch_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ["snmf_train_signals_assemble_i16", "snmf_train_signals_assemble_f64", "snmf_train_signals_info", "snmf_train_signals_get_f64",
           "snmf_train_signals_destroy", "snmf_run_basis_train_signals_batch_f64", "snmf_run_basis_train_signals_batch_fp64"]
MARGIN = 1e-9


# ---- the restatement against hand-built cases ------------------------------------------------------------------------------------
def test_frames_overlap_by_half_and_there_are_floor_len_over_shift_minus_one():
    for n, want in ((50, 4), (59, 4), (60, 5), (61, 5), (69, 5), (70, 6), (19, 0), (20, 1), (9, 0)):
        q, starts = ac.vad_frames(np.ones(n), min(50, n), 20)
        assert len(q) == want and list(starts) == [10 * k for k in range(want)], (n, len(q))
    # one loud sample at 0-based 35 lies in the frames starting at 20 and 30 only: samples 20 .. 49 become voiced
    s = np.full(100, 1.0)
    s[35] = 1000.0
    vad = ac.vadenergy_simple(s, 10, 20)
    assert np.array_equal(np.flatnonzero(vad), np.arange(20, 50))
    # the last frame of a 59-sample clip ends at sample 49, that of a 60-sample clip at 59
    for n, kept in ((59, 0), (60, 20)):
        s = np.r_[np.full(50, 1.0), np.full(n - 50, 1000.0)]
        assert int(ac.vadenergy_simple(s, 50, 20).sum()) == kept


def test_zeros_are_dropped_in_mode_1_only():
    s = np.r_[np.full(50, 1.0), np.full(50, 1000.0)]
    s[60] = s[75] = 0.0
    s[5] = 0.0
    kept = ac.treat_clip(s, 1, None, 1000, 0)
    assert np.array_equal(kept, np.r_[np.full(10, 1.0), np.full(48, 1000.0)])  # frames from 40 on are voiced: the quiet 40 .. 49, 50 loud samples - 2 zeros
    assert len(ac.treat_clip(s, 0, None, 1000, 0)) == 100 and len(ac.treat_clip(s, 2, (1, 100), 1000, 0)) == 100
    assert np.array_equal(ac.treat_clip(s, 2, (0, 300), 1000, 0), s)              # src/load_anot.m:9-15
    assert np.array_equal(ac.treat_clip(s, 2, (60, 62), 1000, 0), s[59:62])       # zeros stay
    assert np.array_equal(ac.treat_clip(s, 0, None, 1000, 61), s[:61]) and len(ac.treat_clip(s, 0, None, 1000, -1)) == 100
    assert len(ac.treat_clip(s, 1, None, 1000, 10)) == 58                          # mode 1 is not cut to train_file_len_max


def test_greater_than_against_greater_or_equal_at_the_limit_and_clips_after_the_stop():
    rs = np.random.RandomState(3)
    clips = [rs.standard_normal(n) for n in (40, 60, 30, 25)]
    s, used, seg = ac.assemble_class(clips, 0, None, 1000, 100, 0)   # exactly the limit after two clips: the third is still read
    assert (len(s), used, seg) == (100, 3, [(0, 40), (40, 100), (100, 100)])
    s, used, seg = ac.assemble_class(clips, 0, None, 1000, 99, 0)    # passed inside the second clip: cut, the third is not used
    assert (len(s), used, seg) == (99, 2, [(0, 40), (40, 99)])
    s, used, seg = ac.assemble_class(clips, 0, None, 1000, 1000, 0)  # never reached
    assert (len(s), used) == (155, 4)
    for a, b in seg:  # every clip: unit variance before the peak scaling, peak 30000
        assert abs(np.abs(s[a:b]).max() - 30000.0) < 1e-9
    t = ac.normalise(clips[0])
    assert np.array_equal(s[:40], t) and abs(np.var(t / t.std(ddof=1), ddof=1) - 1) < 1e-12
    late = list(clips)
    late[3] = np.full(25, np.nan)  # behind the stop: never looked at
    assert np.array_equal(ac.assemble_class(late, 0, None, 1000, 99, 0)[0], ac.assemble_class(clips, 0, None, 1000, 99, 0)[0])


def test_an_all_silent_clip_contributes_nothing_and_counts_as_used():
    rs = np.random.RandomState(4)
    loud = ac.vad_clip(rs, 400)
    for silent in (np.zeros(200, np.int16), ac.vad_clip(rs, 200, silent=True)):
        assert len(ac.treat_clip(silent, 1, None, 1000, 0)) == 0
        s, used, seg = ac.assemble_class([silent, loud], 1, None, 1000, 10_000, 0)
        assert used == 2 and seg[0] == (0, 0) and np.array_equal(s, ac.assemble_class([loud], 1, None, 1000, 10_000, 0)[0])


def test_the_cases_are_what_they_claim():
    ref = ac.reference("mixed")
    assert [(len(s), u) for s, u, _ in ref] == [(2931, 8), (6000, 4), (6000, 7), (6000, 5), (271, 5), (5273, 300), (6000, 2)]
    assert ref[0][2][:5] == [(0, 0), (0, 0), (0, 0), (0, 20), (20, 20)]  # nothing, nothing, the 59 / 60 edge, the silent clip
    assert ref[2][2][5] == (4559, 6000) and ref[2][2][6] == (6000, 6000)  # exactly the limit, then a clip that is read and cut away
    assert ref[3][2][-1] == (5999, 6000)                                  # a stop in the middle of a clip
    assert ref[4][2][0] == (0, 2)                                         # a range of two samples
    no = ac.reference("nocut")
    assert [(len(s), u) for s, u, _ in no][0] == (2 * ac.SPAN + 133, 2) and no[1][1] == 2 and len(no[1][0]) > 1_000_000


# ---- the condition that keeps the GPU comparison honest --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_no_frame_quotient_of_a_gpu_case_is_near_the_threshold(name):
    case = ac.CASES[name]()
    bg_len, frame_len = ac.vad_settings(case["p"]["fs"])
    ms = [(k, i, ac.vad_margin(ac.pcm_to_double(c), bg_len, frame_len)) for k, i, c in ac.mode1_clips(case)]
    print(name, "smallest |q - thr| per mode-1 clip:", [f"{m:.3g}" for _, _, m in ms])
    assert ms and all(m >= MARGIN for _, _, m in ms), ms


def test_the_seeded_generator_keeps_its_margin_and_plants_zeros():
    rs = np.random.RandomState(11)
    worst, dropped = np.inf, []
    for n in rs.randint(50, 3002, size=40):
        c = ac.vad_clip(rs, int(n))
        s = ac.pcm_to_double(c)
        worst = min(worst, ac.vad_margin(s, 50, 20))
        dropped.append(int(((s == 0) & (ac.vadenergy_simple(s, 50, 20) == 1)).sum()))
    print(f"40 clips: worst margin {worst:.3g}, zeros dropped per clip {min(dropped)} .. {max(dropped)}")
    assert worst >= MARGIN and max(dropped) >= 2


# ---- the Python side ------------------------------------------------------------------------------------------------------------
def test_every_argument_error_is_raised_before_any_library_call(monkeypatch):
    from se_snmf_nat_amd import _lib, frontend, train
    from se_snmf_nat_amd.train import TrainSignals, assemble_training_signals, run_basis_train_assembled_batch, run_basis_train_clips_batch

    def no_device(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(train, "default_context", no_device)
    monkeypatch.setattr(frontend, "default_context", no_device)
    rs = np.random.RandomState(5)
    a, b = ac.vad_clip(rs, 300), ac.plain_clip(rs, 120)
    p = dict(fs=1000, train_seq_len_max=1000, train_file_len_max=100)

    def status(classes, pq=p, **kw):
        with pytest.raises(_lib.SnmfError) as e:
            assemble_training_signals(classes, pq, **kw)
        return e.value.status

    assert status([]) == 1                                                # no class
    assert status([[a], []]) == 1                                         # a class with no clip
    assert status([[a]], vad=[True, False]) == 1 and status([[a]], ranges=[None, None]) == 1
    assert status([[a, b]], ranges=[[(1, 5)]]) == 1                       # one range per clip
    assert status([[a.reshape(2, -1)]]) == 3 and status([[a[:0]]]) == 3
    assert status([[a[:49]]], vad=[True]) == 3                            # a mode-1 clip shorter than bg_len
    assert status([[b]], ranges=[[(7, 6)]]) == 3 and status([[b]], ranges=[[(121, 130)]]) == 3 and status([[b]], ranges=[[(-1, 5)]]) == 3
    assert status([[a]], pq=dict(p, fs=1010)) == 1                        # 0.05 * fs is not a whole number of samples
    assert status([[a]], pq=dict(p, fs=250)) == 1                         # frame_len = 5 is odd
    assert status([[a]], pq=dict(p, fs=50)) == 1                          # frame_len = 1
    assert status([[a]], pq=dict(p, train_seq_len_max=-1)) == 1
    with pytest.raises(KeyError):
        assemble_training_signals([[a]], dict(fs=1000))
    # valid calls pass every check and only then reach the library
    for kw in (dict(), dict(vad=[True, False]), dict(ranges=[None, [(0, 500)]]), dict(vad=[False, True], ranges=[[(3, 4)], None])):
        with pytest.raises(AssertionError, match="reached the library"):
            assemble_training_signals([[a], [b]], p, **kw)
    with pytest.raises(AssertionError, match="reached the library"):
        assemble_training_signals([[a.astype(np.float64), b]], dict(p, train_file_len_max=0))

    # the training call on assembled signals: the checks of run_basis_train_signal_batch, from the handle's lengths
    q = tc.P_STOP
    ts = TrainSignals(C.c_void_p(1), None, [tc.n_samples(T) for T in (33, 70)], [1, 1])
    ts.close = lambda: None

    def tstatus(t=ts, R=tc.R, pq=q, **kw):
        with pytest.raises(_lib.SnmfError) as e:
            run_basis_train_assembled_batch(t, R, pq, **kw)
        return e.value.status

    short = TrainSignals(C.c_void_p(1), None, [tc.n_samples(33), tc.N + 1], [1, 1])
    short.close = lambda: None
    assert tstatus(t=[np.zeros(500)]) == 1                                # not a TrainSignals
    assert tstatus(t=short) == 3                                          # a class shorter than one analysis frame
    assert tstatus(R=34) == 3                                             # cluster_buff * R > T_k
    assert tstatus(sample_idx=[tc.sample_idx()[4]]) == 3
    assert tstatus(h0="philox") == 3
    assert tstatus(pq={k: v for k, v in q.items() if k != "cost_check"}) == 4
    closed = TrainSignals(None, None, [500], [1])
    assert tstatus(t=closed) == 7
    with pytest.raises(ValueError):
        run_basis_train_assembled_batch(ts, tc.R, q, precision="bf16")
    for kw in (dict(), dict(h0="device"), dict(precision="fp64"), dict(DC_bin=2), dict(sample_idx=[tc.sample_idx()[4], tc.sample_idx()[5]])):
        with pytest.raises(AssertionError, match="reached the library"):
            run_basis_train_assembled_batch(ts, tc.R, q, **kw)
    # both steps in one call: the errors of either step that need no lengths come before the library
    pq = dict(q, **p)
    with pytest.raises(ValueError):
        run_basis_train_clips_batch([[a]], tc.R, pq, precision="bf16")
    for bad in (dict(h0="philox"), dict(vad=[True, True])):
        with pytest.raises(_lib.SnmfError):
            run_basis_train_clips_batch([[a]], tc.R, pq, **bad)
    with pytest.raises(_lib.SnmfError) as e:
        run_basis_train_clips_batch([[a]], tc.R, {k: v for k, v in pq.items() if k != "cost_check"})
    assert e.value.status == 4
    with pytest.raises(AssertionError, match="reached the library"):
        run_basis_train_clips_batch([[a]], tc.R, pq, vad=[True])


def test_c_names_stand_in_the_header_and_in_the_binding_once():
    from se_snmf_nat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snmf.h")).read(), flags=re.S)
    for nm in C_NAMES:
        assert len(re.findall(r"\b%s\s*\(" % nm, txt)) == 1, nm
        assert _lib.SYMBOLS.count(nm) == 1, nm
    assert "snmf_tu_assemble.hip" in _lib._TU_HDRS and "snmf_assemble.h" in _lib._TU_HDRS["snmf_tu_frontend_batch.hip"]


def test_python_names_are_exported():
    import se_snmf_nat_amd as pkg
    from se_snmf_nat_amd import train
    for nm in ("assemble_training_signals", "run_basis_train_assembled_batch", "run_basis_train_clips_batch"):
        assert getattr(pkg, nm) is getattr(train, nm)


def test_c_entries_refuse_without_a_device(lib):
    """What the entries refuse comes before the device is touched, so it can be checked where there is none.  The context is
    never dereferenced on these paths: a dummy pointer stands in."""
    from se_snmf_nat_amd import _lib, frontend as fe
    from se_snmf_nat_amd.api import _make_params
    ctx = C.c_void_p(8)
    clips = [np.arange(1, 101, dtype=np.int16), np.arange(1, 201, dtype=np.int16)]

    def call(ty="i16", *, ctx=ctx, ap=(20, 50, 0.7, 1000, 0), n=2, n_clips=(1, 1), lens=(100, 200), mode=(1, 0), rng=None, null=None, null_clip=False):
        dt = np.int16 if ty == "i16" else np.float64
        keep = [c.astype(dt) for c in clips]
        cp = (C.c_void_p * 2)(*[c.ctypes.data for c in keep])
        if null_clip:
            cp[1] = None
        a = dict(ap=_lib.SnmfAssembleParams(*ap), n_clips=np.array(n_clips, np.int32), lens=np.array(lens, np.int64), mode=np.array(mode, np.int32),
                 rng=None if rng is None else np.array(rng, np.int64))
        vp = lambda k: None if (null == k or a[k] is None) else C.c_void_p(a[k].ctypes.data)  # noqa: E731
        h = C.c_void_p()
        st = getattr(lib, f"snmf_train_signals_assemble_{ty}")(
            None if null == "ctx" else ctx, None if null == "ap" else C.byref(a["ap"]), n, vp("n_clips"), None if null == "clips" else cp,
            vp("lens"), vp("mode"), vp("rng"), None if null == "out" else C.byref(h))
        assert h.value is None
        return st

    for ty in ("i16", "f64"):
        for nm in ("ctx", "ap", "n_clips", "clips", "lens", "mode", "out"):
            assert call(ty, null=nm) == 1, (ty, nm)
        assert call(ty, null_clip=True) == 1
        assert call(ty, n=0) == 1
        assert call(ty, n_clips=(2, 0)) == 1 and b"class 1 has no clip" in lib.snmf_last_error()
        assert call(ty, mode=(1, 3)) == 1
        assert call(ty, mode=(1, 2)) == 1                                   # a mode-2 class and range == NULL
        assert call(ty, ap=(21, 50, 0.7, 1000, 0)) == 1 and call(ty, ap=(0, 50, 0.7, 1000, 0)) == 1
        assert call(ty, ap=(20, 0, 0.7, 1000, 0)) == 1 and call(ty, ap=(20, 50, 0.7, -1, 0)) == 1
        assert call(ty, lens=(49, 200)) == 3 and b"fewer than bg_len" in lib.snmf_last_error()
        assert call(ty, lens=(100, 0)) == 3
        for r in ((1, 1, 0, 5), (1, 1, 5, 201), (1, 1, 6, 5)):
            assert call(ty, mode=(1, 2), rng=r) == 3, r
    assert lib.snmf_train_signals_info(None, None, None, None) == 1
    assert lib.snmf_train_signals_get_f64(None, 0, None) == 1
    assert lib.snmf_train_signals_destroy(None) == 0
    sp, _win = fe._params(tc.TINY)
    q = _make_params(tc.F, 1, tc.R, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    for ty in ("f64", "fp64"):
        fn = getattr(lib, f"snmf_run_basis_train_signals_batch_{ty}")
        assert fn(ctx, C.byref(q), C.byref(sp), -1.0, None, 0, None, None, 0, None, None, None, None, None, None, None) == 1
        assert fn(None, None, None, -1.0, None, 0, None, None, 0, None, None, None, None, None, None, None) == 1
