"""Get-state / set-state of the batched online separator, the host-side rules (include/snmf.h: snmf_online_state_info,
snmf_online_state_field, snmf_online_batch_state_info / _get_state / _set_state; se_snmf_nat_amd/online.py:
OnlineBatchSeparator.get_state / set_state).  No device is used: the layout function is pure host code, and every Python
refusal here is raised before the library is loaded (the loader is patched to fail)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snmf_online_batch_state_info", "snmf_online_state_field", "snmf_online_batch_get_state", "snmf_online_batch_set_state")
ITEM = (4, 8, 4, 8)  # bytes of snmf_online_state_type F32, F64, I32, I64


def _info(elem=4, mel=0, cls=0, n_classes=0, **kw):
    from se_snmf_nat_amd._lib import SnmfOnlineStateInfo
    q = SnmfOnlineStateInfo(elem_size=elem, mel=mel, mel_conv=mel, F=65, F_order=24 if mel else 0, R_x=16, R_d=20, R_a=8, m_a=12,
                            P_len_l=5, framelength=100, frameshift=25, ntail=300, class_outputs=cls, n_classes=n_classes)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _layout(lib, q):
    from se_snmf_nat_amd._lib import STATE_FIELDS
    out = {}
    for f, name in enumerate(STATE_FIELDS):
        off, cnt, typ = C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
        assert lib.snmf_online_state_field(C.byref(q), f, C.byref(off), C.byref(cnt), C.byref(typ)) == 0, name
        out[name] = (off.value, cnt.value, typ.value)
    return out


def test_new_symbols_are_declared_bound_once_and_reject_null(lib):
    from se_snmf_nat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snmf.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert _lib.SYMBOLS.count(name) == 1 and getattr(lib, name).argtypes is not None
    q = _info()
    assert lib.snmf_online_batch_state_info(None, C.byref(q)) == 1
    assert lib.snmf_online_state_field(None, 0, None, None, None) == 1
    assert lib.snmf_online_batch_get_state(None, 0, None, None, 0) == 1
    assert lib.snmf_online_batch_set_state(None, 0, None, None, 0) == 1


def test_the_info_struct_and_the_field_enum_mirror_the_header():
    from se_snmf_nat_amd import _lib
    txt = open(os.path.join(ROOT, "include", "snmf.h")).read()
    body = re.search(r"typedef struct snmf_online_state_info \{(.*?)\} snmf_online_state_info;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_int64 if typ == "int64_t" else C.c_int32) for n in names.split(",")]
    assert fields == list(_lib.SnmfOnlineStateInfo._fields_)
    assert C.sizeof(_lib.SnmfOnlineStateInfo) == 72 and _lib.STATE_HEADER_BYTES == 8 + 72
    enum = re.search(r"typedef enum snmf_online_state_field_id \{(.*?)\} snmf_online_state_field_id;", txt, re.S).group(1)
    names = re.findall(r"\bSNMF_STATE_([A-Z0-9_]+)\b\s*(?:=\s*0)?,", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
    assert [n.lower() for n in names] == [f.lower() for f in _lib.STATE_FIELDS]
    assert int(re.search(r"#define SNMF_ONLINE_STATE_MAGIC (0x[0-9A-Fa-f]+)u", txt).group(1), 16) == _lib.STATE_MAGIC
    assert int(re.search(r"#define SNMF_ONLINE_STATE_VERSION (\d+)", txt).group(1)) == _lib.STATE_VERSION


@pytest.mark.parametrize("kw", [dict(), dict(elem=8), dict(mel=1), dict(cls=1), dict(elem=8, cls=1, n_classes=2), dict(mel=1, cls=1, n_classes=3),
                                dict(F=33, R_a=1, m_a=1, P_len_l=1, framelength=64, frameshift=64, ntail=64)],
                         ids=["fp32", "fp64", "mel", "cls", "fp64-part", "mel-part", "odd"])
def test_field_offsets_cover_every_enum_value_without_overlap_inside_bytes(lib, kw):
    from se_snmf_nat_amd._lib import STATE_FIELDS, STATE_HEADER_BYTES
    q = _info(**kw)
    lay = _layout(lib, q)
    assert set(lay) == set(STATE_FIELDS)
    E = 0 if q.elem_size == 4 else 1
    F, r = q.F, q.R_x + q.R_d
    want = {"Xm_tilde": (F, E), "lambda_dav": (F, E), "r_blk": (F * q.P_len_l, E), "lambda_d_blk": (F * q.m_a, E), "Ad_blk": (q.R_a * q.m_a, E),
            "n_push": (1, 2), "update_switch": (1, 2), "B_DFT_d": (F * q.R_d, 1), "B_fix": (F * q.R_d, 1),
            "B_Mel_d": (q.F_order * q.R_d if q.mel else 0, 1), "H0": (r, E), "Ad_blk0": (q.R_a * q.m_a, E), "l": (1, 3),
            "y_hist": (q.framelength - q.frameshift, E), "pending": (q.frameshift, E), "pending_count": (1, 2),
            "x_tilde_tail": (q.ntail, E), "x_hat_tail": (q.ntail if q.class_outputs else 0, E),
            "d_hat_tail": (q.ntail if q.class_outputs else 0, E), "class_tails": (q.ntail * q.n_classes, E)}
    assert {k: v[1:] for k, v in lay.items()} == want
    spans = sorted((off, off + cnt * ITEM[typ], name) for name, (off, cnt, typ) in lay.items())
    assert spans[0][0] >= STATE_HEADER_BYTES
    for (a0, a1, na), (b0, b1, nb) in zip(spans, spans[1:]):
        assert a1 <= b0, (na, nb)
    # bytes is the handle's to report; the layout's end is what a batch reports: recomputed here from the last span
    end = (spans[-1][1] + 7) // 8 * 8
    for off, cnt, typ in lay.values():
        assert off % ITEM[typ] == 0 and off + cnt * ITEM[typ] <= end
    assert lay["update_switch"][0] == lay["n_push"][0] + 4  # one pair, as the device keeps it


def test_an_unknown_field_or_a_nonsensical_info_is_invalid(lib):
    from se_snmf_nat_amd._lib import STATE_FIELDS
    q = _info()
    off = C.c_int64()
    assert lib.snmf_online_state_field(C.byref(q), len(STATE_FIELDS), C.byref(off), None, None) == 1
    assert lib.snmf_online_state_field(C.byref(q), -1, C.byref(off), None, None) == 1
    for bad in (dict(elem_size=2), dict(F=0), dict(m_a=0), dict(frameshift=0), dict(framelength=10)):
        assert lib.snmf_online_state_field(C.byref(_info(**bad)), 0, C.byref(off), None, None) == 1, bad
    assert lib.snmf_online_state_field(C.byref(q), 0, None, None, None) == 0  # every out pointer may be NULL


def test_the_python_methods_exist():
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    assert list(inspect.signature(OnlineBatchSeparator.get_state).parameters) == ["self", "streams"]
    assert list(inspect.signature(OnlineBatchSeparator.set_state).parameters) == ["self", "streams", "states"]


# ---------------------------------------------------------------- argument checks before the loader ---------------------
GEO = (128, 100, 25, 16, 20, dict(P_len_k=12, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2, R_a=8, m_a=12, overlap_m_a=0.3))


def _separator(monkeypatch, precision="fp32", class_outputs=False, **over):
    """An OnlineBatchSeparator of three streams on the small geometry whose library calls all succeed and do nothing; the
    loader is then patched to fail, so whatever get_state / set_state check, they check before it."""
    from se_snmf_nat_amd import _lib, online
    from test_online_batch import _geo_streams, _settings

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0

    class Ctx:
        _h = None
        _plans = set()
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(online, "default_context", lambda: Ctx())
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(GEO, 48)
    p = dict(_settings(p), **over)
    sep = online.OnlineBatchSeparator(Bx, Bds, p, 3, H0=H0s, Ad_blk0=Ads, class_outputs=class_outputs, precision=precision)

    def fail(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", fail)
    return sep


def _hand_built(sep, rs):
    st = {}
    for key, (shape, dt) in sep._state_shapes().items():
        st[key] = rs.random_sample(7).astype(dt) if shape is None else np.asarray(rs.random_sample(shape) + 1, dtype=dt)
    st.update(n_push=14, update_switch=2, l=23)
    return st


def test_state_shapes_follow_the_mode(monkeypatch):
    sep = _separator(monkeypatch)
    sh = sep._state_shapes()
    assert sh["r_blk"] == ((65, 5), np.float32) and sh["lambda_d_blk"] == ((65, 12), np.float32) and sh["Ad_blk"] == ((8, 12), np.float32)
    assert sh["B_DFT_d"] == ((65, 20), np.float64) and sh["B_fix"] == ((65, 20), np.float64) and sh["H0"] == ((36,), np.float32)
    assert sh["y_hist"] == ((75,), np.float32) and sh["x_tilde_tail"] == ((300,), np.float32)
    assert "B_Mel_d" not in sh and "x_hat_tail" not in sh and "class_tails" not in sh
    sep = _separator(monkeypatch, precision="fp64", class_outputs=True, EVENT_RANK=[1, 11], EVENT_NUM=2, NOISE_RANK=[1])
    sh = sep._state_shapes()
    assert sh["Xm_tilde"] == ((65,), np.float64) and sh["x_hat_tail"] == ((300,), np.float64) and sh["class_tails"] == ((3, 300), np.float64)
    sep = _separator(monkeypatch, adapt_train_N=0, blk_sparse=0)
    sh = sep._state_shapes()
    assert sh["r_blk"][0] == (65, 1) and sh["lambda_d_blk"][0] == (65, 1) and sh["Ad_blk"][0] == (1, 1)


def test_a_well_formed_state_passes_the_checks_and_reaches_the_loader(monkeypatch):
    sep = _separator(monkeypatch)
    st = _hand_built(sep, np.random.RandomState(3))
    for call in (lambda: sep.set_state(1, st), lambda: sep.set_state([2, 0], [st, st]), lambda: sep.set_state(0, b"\0" * 16),
                 lambda: sep.set_state(0, dict(record=b"\0" * 16)), lambda: sep.get_state(0), lambda: sep.get_state([0, 2])):
        with pytest.raises(AssertionError, match="reached the device"):
            call()


def test_stream_lists_keys_and_shapes_are_checked_before_the_loader(monkeypatch):
    from se_snmf_nat_amd import SnmfError
    sep = _separator(monkeypatch)
    st = _hand_built(sep, np.random.RandomState(3))

    def refused(call, status, match):
        with pytest.raises(SnmfError, match=match) as e:
            call()
        assert e.value.status == status, match
    for streams in (3, -1, [0, 3], [1, 1]):
        refused(lambda: sep.get_state(streams), 1, "stream|twice")
        refused(lambda: sep.set_state(streams, [st, st] if isinstance(streams, list) else st), 1, "stream|twice")
    refused(lambda: sep.set_state([0, 1], [st]), 1, "1 states for 2 streams")
    refused(lambda: sep.set_state(0, 3.5), 1, "float")
    refused(lambda: sep.set_state(0, dict(st, g=1)), 1, "'g'")
    refused(lambda: sep.set_state(0, dict(st, B_Mel_d=np.ones((24, 20)))), 1, "'B_Mel_d'")  # no such field outside Mel mode
    refused(lambda: sep.set_state(0, dict(st, x_hat_tail=np.ones(300))), 1, "'x_hat_tail'")  # nor without class_outputs
    for key in st:  # a hand-built g holds every field ...
        refused(lambda: sep.set_state(0, {k: v for k, v in st.items() if k != key}), 1, repr(key))
    with pytest.raises(AssertionError, match="reached the device"):  # ... a record's overrides need not
        sep.set_state(0, dict(record=b"\0" * 16, Xm_tilde=st["Xm_tilde"]))
    bad = dict(Xm_tilde=np.ones(64), lambda_dav=np.ones((65, 2)), r_blk=np.ones((65, 4)), lambda_d_blk=np.ones((12, 65)), Ad_blk=np.ones((8, 11)),
               B_DFT_d=np.ones((65, 19)), B_fix=np.ones((64, 20)), H0=np.ones(35), Ad_blk0=np.ones((12, 8)), y_hist=np.ones(100),
               x_tilde_tail=np.ones(75), n_push=np.ones(2), l=np.ones((1, 2)))
    for key, a in bad.items():
        refused(lambda: sep.set_state(0, dict(st, **{key: a})), 3, repr(key))
    refused(lambda: sep.set_state(0, dict(st, pending=np.ones(25))), 1, "'pending'")
    refused(lambda: sep.set_state(0, dict(st, n_push=-1)), 1, "'n_push'")
    refused(lambda: sep.set_state(0, dict(st, update_switch=0)), 1, "'update_switch'")
    refused(lambda: sep.set_state(0, dict(st, l=0)), 1, "'l'")
