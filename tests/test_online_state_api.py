"""The single-stream online separator's state g as a value and its restart in place, the host-side rules
(include/snmf.h: snmf_online_stream_state_info / snmf_online_get_state / snmf_online_set_state / snmf_online_restart_f32 /
_f64; se_snmf_nat_amd/online.py: OnlineSeparator.get_state / set_state / restart, ntf_sep_event_rt_chain).  No device is
used: every Python refusal here is raised before the library is loaded (the loader is patched to fail), and the shapes of a
state are computed from the constructor's arguments alone, so they are compared with a batch of one on the CPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snmf_online_stream_state_info", "snmf_online_get_state", "snmf_online_set_state", "snmf_online_restart_f32",
       "snmf_online_restart_f64")
GEO = (128, 100, 25, 16, 20, dict(P_len_k=12, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2, R_a=8, m_a=12, overlap_m_a=0.3))
PARTITION = dict(EVENT_NUM=2, EVENT_RANK=[1, 9], NOISE_NUM=2, NOISE_RANK=[1, 11])


def test_the_new_symbols_are_declared_marked_bound_once_and_reject_null(lib):
    from se_snmf_nat_amd import _lib
    raw = open(os.path.join(ROOT, "include", "snmf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert re.search(r"/\* Added within 5\.(?:(?!\*/).)*\*/\s*int\s+%s\s*\(" % name, raw, re.S), name
        assert _lib.SYMBOLS.count(name) == 1 and getattr(lib, name).argtypes is not None
    assert lib.snmf_abi_version() == 5
    q = _lib.SnmfOnlineStateInfo()
    assert lib.snmf_online_stream_state_info(None, C.byref(q)) == 1
    assert lib.snmf_online_get_state(None, None, 0) == 1
    assert lib.snmf_online_set_state(None, None, 0) == 1
    assert lib.snmf_online_restart_f32(None, None, None, None, None) == 1
    assert lib.snmf_online_restart_f64(None, None, None, None, None) == 1


def test_the_python_methods_and_the_chain_function_exist():
    from se_snmf_nat_amd import online
    from se_snmf_nat_amd.online import OnlineSeparator, ntf_sep_event_rt_chain
    assert list(inspect.signature(OnlineSeparator.get_state).parameters) == ["self"]
    assert list(inspect.signature(OnlineSeparator.set_state).parameters) == ["self", "state"]
    assert list(inspect.signature(OnlineSeparator.restart).parameters) == ["self", "B_DFT_d", "H0", "Ad_blk0", "B_Mel_d"]
    assert all(v.default is None for k, v in inspect.signature(OnlineSeparator.restart).parameters.items() if k != "self")
    sig = inspect.signature(ntf_sep_event_rt_chain).parameters
    assert list(sig) == ["files", "B_DFT_x", "B_DFT_d", "p", "H0", "Ad_blk0", "ctx", "chunk", "B_Mel_x", "B_Mel_d", "precision", "class_outputs"]
    assert sig["precision"].default == "fp32" and sig["class_outputs"].default is False
    assert "ntf_sep_event_rt_chain" in online.__all__


# ---------------------------------------------------------------- separators without a device ---------------------------
def _patch(monkeypatch):
    from se_snmf_nat_amd import _lib, online

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0

    class Ctx:
        _h = None
        _plans = set()
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(online, "default_context", lambda: Ctx())


def _unpatch(monkeypatch):
    from se_snmf_nat_amd import _lib

    def fail(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", fail)


def _inputs(mode, **over):
    """(p, B_DFT_x, B_DFT_d, H0, Ad_blk0, Mel keywords) of stream 0 of a configuration."""
    from test_online_batch import _geo_streams, _settings
    if mode == "mel":
        from test_online_batch_mel import _mel_params, _mel_streams
        p = _mel_params(1)
        pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(2, S=1, p=p)
        return dict(_settings(p), **over), Bx, Bds[0], H0s[0], Ads[0], dict(B_Mel_x=BMx, B_Mel_d=BMds[0])
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(GEO, 48)
    return dict(_settings(p), **over), Bx, Bds[0], H0s[0], Ads[0], {}


def _separator(monkeypatch, mode="dft", precision="fp32", class_outputs=False, batch=False, **over):
    """An OnlineSeparator (batch: an OnlineBatchSeparator of one stream with the same arguments) whose library calls all
    succeed and do nothing; the loader is then patched to fail, so whatever a method checks, it checks before it."""
    from se_snmf_nat_amd import online
    _patch(monkeypatch)
    p, Bx, Bd, H0, Ad, mel = _inputs(mode, **over)
    if batch:
        sep = online.OnlineBatchSeparator(Bx, [Bd], p, 1, H0=[H0], Ad_blk0=[Ad], class_outputs=class_outputs, precision=precision, **mel)
    else:
        sep = online.OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad, class_outputs=class_outputs, precision=precision, **mel)
    _unpatch(monkeypatch)
    return sep


@pytest.mark.parametrize("part", [False, True], ids=["one-class", "partition"])
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "class-outputs"])
@pytest.mark.parametrize("mode,precision", [("dft", "fp32"), ("mel", "fp32"), ("dft", "fp64")], ids=["fp32-dft", "fp32-mel", "fp64"])
def test_state_shapes_are_those_of_a_batch_of_one(monkeypatch, mode, precision, cls, part):
    over = dict(PARTITION) if part else {}
    if part and mode == "mel":
        over = dict(EVENT_NUM=2, EVENT_RANK=[1, 41], NOISE_NUM=2, NOISE_RANK=[1, 51])
    one = _separator(monkeypatch, mode, precision, cls, **over)._state_shapes()
    ref = _separator(monkeypatch, mode, precision, cls, batch=True, **over)._state_shapes()
    assert list(one) == list(ref) and one == ref
    assert ("B_Mel_d" in one) == (mode == "mel") and ("x_hat_tail" in one) == cls and ("class_tails" in one) == (cls and part)
    assert one["Xm_tilde"][1] == (np.float64 if precision == "fp64" else np.float32) and one["B_DFT_d"][1] == np.float64


def test_state_shapes_without_the_rings(monkeypatch):
    one = _separator(monkeypatch, adapt_train_N=0, blk_sparse=0)._state_shapes()
    ref = _separator(monkeypatch, batch=True, adapt_train_N=0, blk_sparse=0)._state_shapes()
    assert one == ref and one["r_blk"][0] == (65, 1) and one["lambda_d_blk"][0] == (65, 1) and one["Ad_blk"][0] == (1, 1)


def _hand_built(sep, rs):
    st = {}
    for key, (shape, dt) in sep._state_shapes().items():
        st[key] = rs.random_sample(7).astype(dt) if shape is None else np.asarray(rs.random_sample(shape) + 1, dtype=dt)
    st.update(n_push=14, update_switch=2, l=23)
    return st


def _refused(call, status, match):
    from se_snmf_nat_amd import SnmfError
    with pytest.raises(SnmfError, match=match) as e:
        call()
    assert e.value.status == status, match


def test_a_well_formed_call_passes_the_checks_and_reaches_the_loader(monkeypatch):
    sep = _separator(monkeypatch)
    st = _hand_built(sep, np.random.RandomState(3))
    rs = np.random.RandomState(4)
    calls = (lambda: sep.get_state(), lambda: sep.set_state(st), lambda: sep.set_state(b"\0" * 16), lambda: sep.set_state(bytearray(16)),
             lambda: sep.set_state(dict(record=b"\0" * 16)), lambda: sep.set_state(dict(record=b"\0" * 16, Xm_tilde=st["Xm_tilde"])),
             lambda: sep.restart(), lambda: sep.restart(B_DFT_d=rs.random_sample((65, 20)), H0=rs.random_sample(36), Ad_blk0=rs.random_sample((8, 12))),
             lambda: sep.restart(H0=rs.random_sample((36, 1))))
    for call in calls:
        with pytest.raises(AssertionError, match="reached the device"):
            call()


def test_set_state_keys_and_shapes_are_checked_before_the_loader(monkeypatch):
    sep = _separator(monkeypatch)
    st = _hand_built(sep, np.random.RandomState(3))
    _refused(lambda: sep.set_state(3.5), 1, "float")
    _refused(lambda: sep.set_state(dict(st, g=1)), 1, "'g'")
    _refused(lambda: sep.set_state(dict(st, B_Mel_d=np.ones((24, 20)))), 1, "'B_Mel_d'")  # no such field outside Mel mode
    _refused(lambda: sep.set_state(dict(st, x_hat_tail=np.ones(300))), 1, "'x_hat_tail'")  # nor without class_outputs
    for key in st:  # a hand-built g holds every field ...
        _refused(lambda: sep.set_state({k: v for k, v in st.items() if k != key}), 1, repr(key))
    bad = dict(Xm_tilde=np.ones(64), lambda_dav=np.ones((65, 2)), r_blk=np.ones((65, 4)), lambda_d_blk=np.ones((12, 65)), Ad_blk=np.ones((8, 11)),
               B_DFT_d=np.ones((65, 19)), B_fix=np.ones((64, 20)), H0=np.ones(35), Ad_blk0=np.ones((12, 8)), y_hist=np.ones(100),
               x_tilde_tail=np.ones(75), n_push=np.ones(2), l=np.ones((1, 2)))
    for key, a in bad.items():
        _refused(lambda: sep.set_state(dict(st, **{key: a})), 3, repr(key))
    _refused(lambda: sep.set_state(dict(st, pending=np.ones(25))), 1, "'pending'")
    _refused(lambda: sep.set_state(dict(st, n_push=-1)), 1, "'n_push'")
    _refused(lambda: sep.set_state(dict(st, update_switch=0)), 1, "'update_switch'")
    _refused(lambda: sep.set_state(dict(st, l=0)), 1, "'l'")


def test_set_state_in_mel_mode_and_with_classes_knows_its_own_fields(monkeypatch):
    sep = _separator(monkeypatch, "mel", class_outputs=True, EVENT_NUM=2, EVENT_RANK=[1, 41], NOISE_NUM=1, NOISE_RANK=[1])
    st = _hand_built(sep, np.random.RandomState(5))
    assert st["B_Mel_d"].shape == (64, 100) and st["class_tails"].shape[0] == 3
    with pytest.raises(AssertionError, match="reached the device"):
        sep.set_state(st)
    _refused(lambda: sep.set_state(dict(st, B_Mel_d=np.ones((63, 100)))), 3, "'B_Mel_d'")
    _refused(lambda: sep.set_state(dict(st, class_tails=np.ones((2, st["class_tails"].shape[1])))), 3, "'class_tails'")
    _refused(lambda: sep.set_state({k: v for k, v in st.items() if k != "x_hat_tail"}), 1, "'x_hat_tail'")


def test_restart_shapes_and_the_mel_dictionary_are_checked_before_the_loader(monkeypatch):
    sep = _separator(monkeypatch)
    _refused(lambda: sep.restart(B_DFT_d=np.ones((65, 19))), 1, "B_DFT_d")
    _refused(lambda: sep.restart(B_DFT_d=np.ones((20, 65))), 1, "B_DFT_d")
    _refused(lambda: sep.restart(H0=np.ones(35)), 1, "H0")
    _refused(lambda: sep.restart(Ad_blk0=np.ones((12, 8))), 1, "Ad_blk0")
    _refused(lambda: sep.restart(B_Mel_d=np.ones((24, 20))), 7, "Mel")
    f64 = _separator(monkeypatch, precision="fp64")
    _refused(lambda: f64.restart(B_Mel_d=np.ones((24, 20))), 7, "Mel")
    _refused(lambda: f64.restart(H0=np.ones((2, 36))), 1, "H0")
    mel = _separator(monkeypatch, "mel")
    _refused(lambda: mel.restart(B_Mel_d=np.ones((64, 99))), 1, "B_Mel_d")
    with pytest.raises(AssertionError, match="reached the device"):
        mel.restart(B_Mel_d=np.ones((64, 100)))
