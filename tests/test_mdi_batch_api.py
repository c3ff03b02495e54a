"""CPU tests of the batched missing-data solves (se_snmf_nat_amd/batch.py: snmf_mdi_batch, snmf_mdi_Sm_batch, BatchPlanMdi64;
include/snmf.h: snmf_batch_create_mdi_fp64, snmf_batch_set_problem_mdi_f64, snmf_batch_get_v_mdi_f64, snmf_mdi_batch_fp64): the
names exist at every layer; the defaulting and the errors of snmf_mdi and the refusals of the batch are raised in Python before
the library is loaded or a context is made, and in C before a device is touched; and the draws are those of B snmf_mdi calls
fed from one generator in list order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("snmf_batch_create_mdi_fp64", "snmf_batch_set_problem_mdi_f64", "snmf_batch_get_v_mdi_f64", "snmf_mdi_batch_fp64")
ENTRIES = ("snmf_mdi_batch", "snmf_mdi_Sm_batch")


@pytest.fixture
def no_device(monkeypatch):
    from se_snmf_nat_amd import _lib, batch

    def refuse(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(batch, "default_context", refuse)


def _vs(F=6, Ts=(5, 3, 8)):
    rs = np.random.RandomState(0)
    return [rs.rand(F, T) + 0.1 for T in Ts]


def _ms(vs, seed=1):
    rs = np.random.RandomState(seed)
    return [(rs.rand(*v.shape) > 0.3).astype(np.float64) for v in vs]


def _entry(name):
    import se_snmf_nat_amd
    return getattr(se_snmf_nat_amd, name)


def test_exports():
    import se_snmf_nat_amd as pkg
    from se_snmf_nat_amd import batch
    assert callable(pkg.snmf_mdi_batch) and callable(pkg.snmf_mdi_Sm_batch)
    assert issubclass(pkg.BatchPlanMdi64, pkg.BatchPlan64)
    assert {"snmf_mdi_batch", "snmf_mdi_Sm_batch", "BatchPlanMdi64"} <= set(batch.__all__)


def test_header_and_binding_name_the_new_symbols():
    from se_snmf_nat_amd import _lib
    with open(os.path.join(ROOT, "include", "snmf.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS) == len(set(_lib.SYMBOLS))


@pytest.mark.parametrize("name", ENTRIES)
def test_lengths_and_shapes_before_any_device_call(no_device, name):
    from se_snmf_nat_amd import SnmfError
    fn = _entry(name)
    vs = _vs()
    ms = _ms(vs)
    p = dict(init_w=np.ones((6, 2)), cost_check=1)
    with pytest.raises(SnmfError, match="2 masks for 3 problems") as e:
        fn(vs, ms[:2], p)
    assert e.value.status == 3
    with pytest.raises(SnmfError, match=r"mask of problem 1 is \(6, 4\)") as e:
        fn(vs, [ms[0], np.ones((6, 4)), ms[2]], p)
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="rows") as e:  # differing row counts
        fn([vs[0], np.ones((7, 4))], [ms[0], np.ones((7, 4))], p)
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="empty") as e:
        fn([], [], p)
    assert e.value.status == 1
    with pytest.raises(SnmfError, match="at least one column") as e:
        fn([vs[0], np.ones((6, 0))], [ms[0], np.ones((6, 0))], p)
    assert e.value.status == 1
    with pytest.raises(SnmfError, match="init_w is a list of 2") as e:
        fn(vs, ms, dict(p, init_w=[np.ones((6, 2))] * 2))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_h must be a list of 3") as e:
        fn(vs, ms, dict(p, init_h="ones"))  # (the list form only, as in sparse_nmf_batch)
    assert e.value.status == 3
    with pytest.raises(SnmfError, match=r"init_h is \(3, 3\), expected \(2, 3\)") as e:
        fn(vs, ms, dict(p, init_h=[np.ones((2, 5)), np.ones((3, 3)), np.ones((2, 8))]))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="Number of components or initialization must be given") as e:
        fn(vs, ms, dict(cost_check=1))
    assert e.value.status == 2


@pytest.mark.parametrize("name", ENTRIES)
def test_defaulting_and_refusals_before_any_device_call(no_device, name):
    from se_snmf_nat_amd import SnmfError
    fn = _entry(name)
    vs = _vs()
    ms = _ms(vs)
    w0 = np.ones((6, 4))
    with pytest.raises(KeyError, match="cost_check"):  # src/snmf_mdi.m:260, snmf_mdi's own error
        fn(vs, ms, dict(init_w=w0))
    # the _mdi defaults are installed only when the plain field is ABSENT (src/snmf_mdi.m:87-93)
    with pytest.raises(KeyError, match="sparsity_mdi"):
        fn(vs, ms, dict(init_w=w0, cost_check=1, sparsity=5))
    with pytest.raises(KeyError, match="conv_eps_mdi"):
        fn(vs, ms, dict(init_w=w0, cost_check=1, conv_eps=1e-3))
    with pytest.raises(SnmfError, match="r x n matrix") as e:  # a sparsity matrix has no batched form
        fn(vs, ms, dict(init_w=w0, sparsity_mdi=np.ones((4, 5)), cost_check=1))
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="sparsity column has 3 rows") as e:
        fn(vs, ms, dict(init_w=w0, sparsity_mdi=np.ones(3), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="partial h_update_ind") as e:
        fn(vs, ms, dict(init_w=w0, h_update_ind=np.array([1, 1, 0, 1], bool), cost_check=1))
    assert e.value.status == 3


def test_plan_refusals_before_any_device_call(no_device):
    from se_snmf_nat_amd import BatchPlanMdi64, SnmfError
    with pytest.raises(SnmfError, match="partial h_update_ind") as e:
        BatchPlanMdi64(None, 6, 4, [5, 3], h_update_ind=[1, 0, 1, 1])
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="r x n matrix") as e:
        BatchPlanMdi64(None, 6, 4, [5, 3], sparsity=np.ones((4, 5)))
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="empty") as e:
        BatchPlanMdi64(None, 6, 4, [])
    assert e.value.status == 1


class _Recorder:
    """Stands for the library: records what the one-shot entries are handed and returns SNMF_OK."""

    def __init__(self):
        self.calls = []

    def _arrs(self, ptrs, B, sizes):
        return [np.ctypeslib.as_array(C.cast(C.c_void_p(ptrs[k]), C.POINTER(C.c_double)), (sizes[k],)).copy() for k in range(B)]

    def snmf_mdi_batch_fp64(self, ctx, sp, B, Ts, V, ldV, M, ldM, W0, H0, S, *rest):
        T = np.ctypeslib.as_array(C.cast(Ts, C.POINTER(C.c_int32)), (B,)).copy()
        r, F = sp._obj.r, sp._obj.F
        self.calls.append(dict(m=self._arrs(M, B, [F * int(t) for t in T]), w=self._arrs(W0, B, [F * r] * B),
                               h=self._arrs(H0, B, [r * int(t) for t in T]), scalar=sp._obj.sparsity_scalar, kind=sp._obj.sparsity_kind,
                               conv_eps=sp._obj.conv_eps, cost_check=sp._obj.cost_check, max_iter=sp._obj.max_iter, beta=sp._obj.beta))
        return 0

    def snmf_mdi_fp64(self, ctx, sp, V, ldV, M, ldM, W0, H0, *rest):
        F, T, r = sp._obj.F, sp._obj.T, sp._obj.r
        get = lambda q, n: np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_double)), (n,)).copy()  # noqa: E731
        self.calls.append(dict(m=get(M, F * T), w=get(W0, F * r), h=get(H0, r * T)))
        return 0


class _FakeCtx:
    _h = None


def test_draws_are_those_of_single_calls_fed_from_one_generator(monkeypatch):
    """With the C entries replaced by a recorder: the batch hands over the initial factors that B snmf_mdi calls draw from one
    generator in list order (w then h per problem, a narrow init_w widened by drawn columns), and the masks as snmf_mdi
    complements them."""
    from se_snmf_nat_amd import _lib, snmf_mdi, snmf_mdi_batch, snmf_mdi_Sm, snmf_mdi_Sm_batch
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    vs = _vs()
    Dms = [(m * 3).astype(np.int64) for m in _ms(vs)]  # observed entries are 3, not 1: a binary mask is `!= 0`
    p = dict(r=3, cost_check=1, max_iter=2, init_w=np.ones((6, 1)))  # two columns of W and every H are drawn
    snmf_mdi_batch(vs, Dms, p, ctx=_FakeCtx(), rng=np.random.RandomState(7))
    rng = np.random.RandomState(7)
    for v, d in zip(vs, Dms):
        snmf_mdi(v, d, p, ctx=_FakeCtx(), rng=rng, precision="fp64")
    b, singles = rec.calls[0], rec.calls[1:]
    assert len(singles) == 3
    for k, s in enumerate(singles):
        assert b["w"][k].tobytes() == s["w"].tobytes() and b["h"][k].tobytes() == s["h"].tobytes(), k
        assert b["m"][k].tobytes() == s["m"].tobytes() and set(np.unique(b["m"][k])) <= {0.0, 1.0}, k
    assert not np.array_equal(b["w"][0], b["w"][1])  # (list order: the problems do not share a draw)
    # the default generator is snmf_mdi's: RandomState(random_seed)
    rec.calls.clear()
    snmf_mdi_batch(vs[:1], Dms[:1], dict(p, random_seed=11), ctx=_FakeCtx())
    snmf_mdi(vs[0], Dms[0], dict(p, random_seed=11), ctx=_FakeCtx(), precision="fp64")
    assert rec.calls[0]["w"][0].tobytes() == rec.calls[1]["w"].tobytes() and rec.calls[0]["h"][0].tobytes() == rec.calls[1]["h"].tobytes()
    # a soft mask goes through as it is
    rec.calls.clear()
    Sms = [np.clip(0.8 * m + 0.1, 0, 1) for m in _ms(vs)]
    snmf_mdi_Sm_batch(vs, Sms, p, ctx=_FakeCtx(), rng=np.random.RandomState(7))
    snmf_mdi_Sm(vs[1], Sms[1], p, ctx=_FakeCtx(), rng=np.random.RandomState(7), precision="fp64")
    assert rec.calls[0]["m"][1].tobytes() == rec.calls[1]["m"].tobytes() == np.asfortranarray(Sms[1]).tobytes(order="F")


def test_settings_reach_the_entry_as_snmf_mdi_reads_them(monkeypatch):
    from se_snmf_nat_amd import _lib, snmf_mdi_batch
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    vs = _vs()
    ms = _ms(vs)
    info = {}
    out = snmf_mdi_batch(vs, ms, dict(init_w=np.ones((6, 2)), cost_check=0, cf="ed", max_iter=4), ctx=_FakeCtx(), info=info)
    c = rec.calls[0]
    assert (c["kind"], c["scalar"], c["conv_eps"], c["cost_check"], c["max_iter"], c["beta"]) == (0, 0.0, 0.0, 0, 4, 2.0)  # the defaults
    assert len(out) == 3 and [w.shape for w in info["w"]] == [(6, 2)] * 3
    assert [(v.shape, h.shape) for v, h, _ in out] == [((6, 5), (2, 5)), ((6, 3), (2, 3)), ((6, 8), (2, 8))]
    snmf_mdi_batch(vs, ms, dict(init_w=np.ones((6, 2)), cost_check=1, sparsity_mdi=2.5, conv_eps_mdi=1e-4, sparsity=9, conv_eps=1),
                   ctx=_FakeCtx())
    c = rec.calls[1]
    assert (c["scalar"], c["conv_eps"], c["cost_check"], c["beta"]) == (2.5, 1e-4, 1, 1.0)  # (the plain fields are not read)


def test_c_entries_reject_null_and_refuse_before_any_device(lib):
    """The new C entries check their arguments before they touch a device, with the refusals of snmf_batch_create_fp64."""
    from se_snmf_nat_amd.api import _make_params
    T = np.array([5, 3], np.int32)
    Tp = C.c_void_p(T.ctypes.data)
    h = C.c_void_p()
    ctx = C.c_void_p(1)  # never dereferenced by the checks below
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    create = lib.snmf_batch_create_mdi_fp64
    assert create(None, C.byref(sp), 2, Tp, C.byref(h)) == 1
    assert create(ctx, None, 2, Tp, C.byref(h)) == 1
    assert create(ctx, C.byref(sp), 2, None, C.byref(h)) == 1
    assert create(ctx, C.byref(sp), 2, Tp, None) == 1
    assert create(ctx, C.byref(sp), 0, Tp, C.byref(h)) == 1
    Tz = np.array([5, 0], np.int32)
    assert create(ctx, C.byref(sp), 2, C.c_void_p(Tz.ctypes.data), C.byref(h)) == 1
    assert b"T = 0" in lib.snmf_last_error()
    hi = np.array([1, 1, 0, 1, 1, 1, 1, 1], np.uint8)
    sp_h = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, hi)
    assert create(ctx, C.byref(sp_h), 2, Tp, C.byref(h)) == 3
    assert b"partial h_update_ind" in lib.snmf_last_error()
    sp_full = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 2, 0.0, None, None)
    assert create(ctx, C.byref(sp_full), 2, Tp, C.byref(h)) == 8
    assert b"r x n matrix" in lib.snmf_last_error()
    Tbig = np.ones(65536, np.int32)
    sp_s = _make_params(8, 1, 2, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert create(ctx, C.byref(sp_s), 65536, C.c_void_p(Tbig.ctypes.data), C.byref(h)) == 8
    assert b"65535" in lib.snmf_last_error()
    assert h.value is None
    # a NULL handle
    a = np.ones(64 * 8)
    ap = C.c_void_p(a.ctypes.data)
    assert lib.snmf_batch_set_problem_mdi_f64(None, 0, ap, 64, ap, 64, ap, ap) == 1
    assert lib.snmf_batch_get_v_mdi_f64(None, 0, ap, 64) == 1
    # the one-shot entry
    two = (C.c_void_p * 2)()
    full = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    ld = np.array([64, 64], np.int64)
    ldp = C.c_void_p(ld.ctypes.data)
    one = lib.snmf_mdi_batch_fp64
    args = lambda cx, spx, n, Tx, M=full, Vm=full: (cx, spx, n, Tx, full, ldp, M, ldp, full, full, None, Vm, None, full, full,  # noqa: E731
                                                    None, None, None)
    assert one(*args(None, C.byref(sp), 2, Tp)) == 1
    assert one(*args(ctx, None, 2, Tp)) == 1
    assert one(*args(ctx, C.byref(sp), 2, None)) == 1
    assert one(*args(ctx, C.byref(sp), 2, Tp, M=None)) == 1
    assert one(*args(ctx, C.byref(sp), 2, Tp, Vm=None)) == 1
    assert one(*args(ctx, C.byref(sp), 2, Tp, M=two)) == 1  # NULL arrays
    assert b"NULL" in lib.snmf_last_error()
    assert one(*args(ctx, C.byref(sp), 0, Tp)) == 1
    assert one(*args(ctx, C.byref(sp), 2, C.c_void_p(Tz.ctypes.data))) == 1
    assert one(*args(ctx, C.byref(sp_h), 2, Tp)) == 3
    assert one(*args(ctx, C.byref(sp_full), 2, Tp)) == 8
