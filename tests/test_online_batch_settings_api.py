"""Settings and an event dictionary per stream of the fp64 batched online separator, the host-side rules
(se_snmf_nat_amd/online.py: OnlineBatchSeparator(settings=, B_DFT_x=[...]), restart(B_DFT_x=, settings=), ntf_sep_event_rt_batch /
_chains(settings=); include/snmf.h: snmf_online_stream_settings, snmf_online_batch_create_streams_f64 / _restart_streams_f64 /
_get_settings).  Every refusal here is raised before the library is loaded: the loader is patched to fail."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_online_batch_f64 import HOP, _fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snmf_online_batch_create_streams_f64", "snmf_online_batch_restart_streams_f64", "snmf_online_batch_get_settings")


@pytest.fixture
def no_device(monkeypatch):
    from se_snmf_nat_amd import _lib, online

    def fail(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", fail)
    monkeypatch.setattr(online, "default_context", fail)
    return fail


def _calls(Bx, Bd, p, s, **kw):
    """The three entry points with the same per-stream arguments (two streams / recordings / chains)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator, ntf_sep_event_rt_batch, ntf_sep_event_rt_chains
    x = s[:2 * HOP]
    return (lambda: OnlineBatchSeparator(Bx, Bd, p, 2, **kw),
            lambda: ntf_sep_event_rt_batch([x, x], Bx, Bd, p, **kw),
            lambda: ntf_sep_event_rt_chains([[x], [x]], Bx, Bd, p, **kw))


def test_settings_is_a_keyword_of_the_entry_points_and_of_restart():
    from se_snmf_nat_amd import online
    for fn in (online.OnlineBatchSeparator.__init__, online.ntf_sep_event_rt_batch, online.ntf_sep_event_rt_chains):
        assert inspect.signature(fn).parameters["settings"].default is None
    sig = inspect.signature(online.OnlineBatchSeparator.restart).parameters
    assert sig["settings"].default is None and sig["B_DFT_x"].default is None


def test_a_changed_shared_key_is_invalid_and_named(no_device):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import default_settings
    s, Bx, Bd = _fixture()
    p = default_settings()
    shared = dict(fftlength=512, framelength=320, frameshift=80, delay=2, DCbin=3, preemph=0.5, pow=1, nonzerofloor=1e-6, R_a=20, m_a=50,
                  P_len_l=10, cost_check=0, EVENT_RANK=[1, 4], win_STFT=np.ones(640), Splice=1, overlapscale=1.0)
    for key, v in shared.items():
        for call in _calls(Bx, Bd, p, s, precision="fp64", settings=[{}, {key: v}]):
            with pytest.raises(SnmfError, match=re.escape(repr(key))) as e:
                call()
            assert e.value.status == 1, key
    with pytest.raises(SnmfError, match="'no_such_key'") as e:  # a key p does not hold is no stream key either
        _calls(Bx, Bd, p, s, precision="fp64", settings=[{"no_such_key": 1}, {}])[0]()
    assert e.value.status == 1


def test_a_shared_key_repeated_with_its_own_value_passes_the_check(no_device):
    """An entry may carry the whole settings dict of a variant: equal shared keys are no change.  (It then reaches the
    loader, which is patched to fail.)"""
    from se_snmf_nat_amd.online import default_settings
    s, Bx, Bd = _fixture()
    p = default_settings()
    variant = dict(default_settings(), ENHANCE_METHOD="Wiener", sparsity=50, cf="ed", adapt_train_N=0, alpha_eta=0.5, alpha_d=0.7, beta=2.0,
                   max_iter=30, conv_eps=0.0, beta_max=100.0, blk_sparse=0, P_len_k=40, blk_gap=5, alpha_p=0.3, init_N_len=3,
                   overlap_m_a=0.05, Ar_up=2.0)
    for call in _calls(Bx, Bd, p, s, precision="fp64", settings=[variant, {}]):
        with pytest.raises(AssertionError, match="reached the device"):
            call()


def test_what_the_fp64_batch_does_not_run_is_unsupported_in_an_entry(no_device):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import default_settings
    s, Bx, Bd = _fixture()
    p = default_settings()
    for entry in (dict(basis_update_N=1), dict(basis_update_E=1), dict(B_sep_mode="Mel")):
        for call in _calls(Bx, Bd, p, s, precision="fp64", settings=[{}, entry]):
            with pytest.raises(SnmfError) as e:
                call()
            assert e.value.status == 8, entry


def test_fp32_takes_neither_a_settings_list_nor_a_list_of_event_dictionaries(no_device):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import default_settings
    s, Bx, Bd = _fixture()
    p = default_settings()
    for kw in (dict(settings=[{}, {}]), dict(settings=[{}, {}], precision="fp32"), dict(precision="fp32")):
        Bxa = Bx if "settings" in kw else [Bx, Bx]
        for call in _calls(Bxa, Bd, p, s, **kw):
            with pytest.raises(SnmfError) as e:
                call()
            assert e.value.status == 8, kw


def test_list_lengths_and_shapes_are_checked(no_device):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import default_settings
    s, Bx, Bd = _fixture()
    p = default_settings()
    bad = (dict(settings=[{}]), dict(settings=[{}, {}, {}]), dict(settings=[{}, 3]))
    for kw in bad:
        for call in _calls(Bx, Bd, p, s, precision="fp64", **kw):
            with pytest.raises(SnmfError) as e:
                call()
            assert e.value.status == 1, kw
    for Bxa in ([Bx], [Bx, Bx[:, :50]], [Bx, Bx[:100]]):
        for call in _calls(Bxa, Bd, p, s, precision="fp64"):
            with pytest.raises(SnmfError) as e:
                call()
            assert e.value.status == 1
    with pytest.raises(ValueError, match="ENHANCE_METHOD"):
        _calls(Bx, Bd, p, s, precision="fp64", settings=[{}, dict(ENHANCE_METHOD="LSA")])[0]()


def test_the_uniform_call_does_not_go_through_the_new_entry(monkeypatch):
    """Scalar B_DFT_x with settings=None: the existing create entry, with the arguments it always had."""
    from se_snmf_nat_amd import _lib, online
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                seen.append((name, len(a)))
                raise RuntimeError("stop at the first library call")
            return f

    class Ctx:
        _h = None
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(online, "default_context", lambda: Ctx())
    s, Bx, Bd = _fixture()
    for kw, name, nargs in ((dict(precision="fp64"), "snmf_online_batch_create_f64", 10),
                            (dict(), "snmf_online_batch_create", 10),
                            (dict(precision="fp64", settings=[{}, {}]), "snmf_online_batch_create_streams_f64", 11),
                            (dict(precision="fp64", B=[Bx, Bx]), "snmf_online_batch_create_streams_f64", 11)):
        del seen[:]
        Bxa = kw.pop("B", Bx)
        with pytest.raises(RuntimeError, match="first library call"):
            OnlineBatchSeparator(Bxa, Bd, default_settings(), 2, **kw)
        assert seen == [(name, nargs)], (kw, seen)


def test_the_settings_struct_mirrors_the_header():
    """snmf_online_stream_settings in include/snmf.h and its ctypes mirror: the same fields, types and order; it carries
    overlap_m_a (the reference's unit), not the switch count."""
    from se_snmf_nat_amd._lib import SnmfOnlineStreamSettings
    txt = open(os.path.join(ROOT, "include", "snmf.h")).read()
    body = re.search(r"typedef struct snmf_online_stream_settings \{(.*?)\} snmf_online_stream_settings;", txt, re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_double if typ == "double" else C.c_int32) for n in names.split(",")]
    assert fields == list(SnmfOnlineStreamSettings._fields_)
    names = [n for n, _ in fields]
    assert "overlap_m_a" in names and "switch_at" not in names
    assert set(names) == {"beta_div", "sparsity", "conv_eps", "max_iter", "enhance_method", "init_N_len", "alpha_eta", "alpha_d", "beta",
                          "beta_max", "blk_sparse", "P_len_k", "blk_gap", "alpha_p", "adapt_train_N", "overlap_m_a", "Ar_up"}


def test_new_symbols_are_declared_bound_and_reject_null(lib):
    from se_snmf_nat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snmf.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert _lib.SYMBOLS.count(name) == 1 and getattr(lib, name).argtypes is not None
    h = C.c_void_p()
    assert lib.snmf_online_batch_create_streams_f64(None, None, 2, None, None, None, None, None, None, None, C.byref(h)) == 1
    assert not h.value
    assert lib.snmf_online_batch_restart_streams_f64(None, 0, None, None, None, None, None, None) == 1
    assert lib.snmf_online_batch_get_settings(None, 0, None) == 1
