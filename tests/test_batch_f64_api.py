"""CPU tests of the fp64 mode of the batched offline solve (se_snmf_nat_amd/batch.py: sparse_nmf_batch_fp64, BatchPlan64;
include/snmf.h: snmf_batch_create_fp64, snmf_sparse_nmf_batch_fp64): the names exist at every layer, and the reference's own
errors and the batch's refusals are raised with the status and the wording of the fp32 functions -- in Python before the
library is loaded or a context is made, in C before a device is touched."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("snmf_batch_create_fp64", "snmf_sparse_nmf_batch_fp64")


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


def test_exports():
    import se_snmf_nat_amd as pkg
    from se_snmf_nat_amd import batch
    assert callable(pkg.sparse_nmf_batch_fp64) and isinstance(pkg.BatchPlan64, type)
    assert issubclass(pkg.BatchPlan64, pkg.BatchPlan)
    assert {"sparse_nmf_batch_fp64", "BatchPlan64"} <= set(batch.__all__)


def test_header_and_binding_name_the_new_symbols():
    from se_snmf_nat_amd import _lib
    with open(os.path.join(ROOT, "include", "snmf.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS
    assert "snmf_tu_batch64.hip" in _lib._TU_HDRS  # the dependency map knows the new translation unit


def test_precision_error_names_the_new_functions(no_device):
    from se_snmf_nat_amd import BatchPlan, sparse_nmf_batch
    with pytest.raises(ValueError, match="precision") as e:
        sparse_nmf_batch(_vs(), dict(init_w=np.ones((6, 2)), cost_check=1), precision="fp64")
    assert "sparse_nmf_batch_fp64" in str(e.value) and "BatchPlan64" in str(e.value)
    with pytest.raises(ValueError, match="precision") as e:
        BatchPlan(None, 6, 4, [5, 3], precision="fp64")
    assert "BatchPlan64" in str(e.value)


def test_reference_errors_before_any_device_call(no_device):
    from se_snmf_nat_amd import SnmfError, sparse_nmf_batch_fp64
    vs = _vs()
    w0 = np.ones((6, 2))
    with pytest.raises(SnmfError, match="rows") as e:  # differing row counts
        sparse_nmf_batch_fp64([vs[0], np.ones((7, 4))], dict(init_w=w0, cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="rows") as e:  # ... also without an init_w to compare with
        sparse_nmf_batch_fp64([vs[0], np.ones((7, 4))], dict(r=2, cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_w is a list of 2") as e:
        sparse_nmf_batch_fp64(vs, dict(init_w=[w0, w0], cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_w") as e:  # (7, 2) against 6 rows, sparse_nmf's words
        sparse_nmf_batch_fp64(vs, dict(init_w=np.ones((7, 2)), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match=r"init_h is \(3, 3\), expected \(2, 3\)") as e:
        sparse_nmf_batch_fp64(vs, dict(init_w=w0, init_h=[np.ones((2, 5)), np.ones((3, 3)), np.ones((2, 8))], cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_h must be a list of 3") as e:
        sparse_nmf_batch_fp64(vs, dict(init_w=w0, init_h=[np.ones((2, 5))], cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="cost_check") as e:  # src/sparse_nmf.m:260
        sparse_nmf_batch_fp64(vs, dict(init_w=w0))
    assert e.value.status == 4
    with pytest.raises(SnmfError, match="Number of components or initialization must be given") as e:  # :117-119
        sparse_nmf_batch_fp64(vs, dict(cost_check=1))
    assert e.value.status == 2
    with pytest.raises(SnmfError, match="at least one column") as e:  # a zero frame count
        sparse_nmf_batch_fp64([vs[0], np.ones((6, 0))], dict(init_w=w0, cost_check=1))
    assert e.value.status == 1


def test_batch_refusals_before_any_device_call(no_device):
    from se_snmf_nat_amd import BatchPlan64, SnmfError, sparse_nmf_batch_fp64
    vs = _vs()
    w0 = np.ones((6, 4))
    with pytest.raises(SnmfError, match="partial h_update_ind") as e:
        sparse_nmf_batch_fp64(vs, dict(init_w=w0, h_update_ind=np.array([1, 1, 0, 1], bool), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="r x n matrix") as e:  # a sparsity matrix has no batched form
        sparse_nmf_batch_fp64(vs, dict(init_w=w0, sparsity=np.ones((4, 5)), cost_check=1))
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="sparsity column has 3 rows") as e:
        sparse_nmf_batch_fp64(vs, dict(init_w=w0, sparsity=np.ones(3), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="empty") as e:
        sparse_nmf_batch_fp64([], dict(init_w=w0, cost_check=1))
    assert e.value.status == 1
    with pytest.raises(SnmfError, match="partial h_update_ind") as e:
        BatchPlan64(None, 6, 4, [5, 3], h_update_ind=[1, 0, 1, 1])
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="r x n matrix") as e:
        BatchPlan64(None, 6, 4, [5, 3], sparsity=np.ones((4, 5)))
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="empty") as e:
        BatchPlan64(None, 6, 4, [])
    assert e.value.status == 1
    with pytest.raises(TypeError):  # the mode is in the name: the fp64 plan takes no `precision`
        BatchPlan64(None, 6, 4, [5, 3], precision="fp64")


def test_draws_are_those_of_the_fp32_function(monkeypatch):
    """One host side: with the C entry replaced by a recorder, both functions hand over the same initial factors, drawn from
    one generator in list order."""
    import ctypes as C
    from se_snmf_nat_amd import _lib, batch
    seen = {}

    class FakeLib:
        def __getattr__(self, name):
            def entry(ctx, sp, B, Ts, V, ldV, W0, H0, *rest):
                T = np.ctypeslib.as_array(C.cast(Ts, C.POINTER(C.c_int32)), (B,)).copy()
                r, F = sp._obj.r, sp._obj.F
                w = [np.ctypeslib.as_array(C.cast(C.c_void_p(W0[k]), C.POINTER(C.c_double)), (F * r,)).copy() for k in range(B)]
                h = [np.ctypeslib.as_array(C.cast(C.c_void_p(H0[k]), C.POINTER(C.c_double)), (r * int(T[k]),)).copy() for k in range(B)]
                seen[name] = (w, h)
                return 0
            return entry

    class FakeCtx:
        _h = None
    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    vs = _vs()
    p = dict(r=3, cost_check=1, max_iter=2, random_seed=7, init_w=np.ones((6, 1)))  # two columns of W and every H are drawn
    batch.sparse_nmf_batch(vs, p, ctx=FakeCtx())
    batch.sparse_nmf_batch_fp64(vs, p, ctx=FakeCtx())
    a, b = seen["snmf_sparse_nmf_batch_f64"], seen["snmf_sparse_nmf_batch_fp64"]
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(a[0][0], a[0][1])  # (list order: the problems do not share a draw)


def test_c_entries_reject_null_and_refuse_before_any_device(lib):
    """The two new C entries check their arguments before they touch a device: NULL -> 1, a partial h_update_ind -> 3, a
    sparsity matrix -> 8, an empty batch -> 1, a zero frame count -> 1; and F and r above the fp32 batch's envelope are not
    refused for their size."""
    import ctypes as C
    from se_snmf_nat_amd.api import _make_params
    T = np.array([5, 3], np.int32)
    Tp = C.c_void_p(T.ctypes.data)
    h = C.c_void_p()
    ctx = C.c_void_p(1)  # never dereferenced by the checks below
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_batch_create_fp64(None, C.byref(sp), 2, Tp, C.byref(h)) == 1
    assert lib.snmf_batch_create_fp64(ctx, None, 2, Tp, C.byref(h)) == 1
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 2, None, C.byref(h)) == 1
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 2, Tp, None) == 1
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 0, Tp, C.byref(h)) == 1  # an empty batch
    Tz = np.array([5, 0], np.int32)
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 2, C.c_void_p(Tz.ctypes.data), C.byref(h)) == 1  # a zero frame count
    assert b"T = 0" in lib.snmf_last_error()
    hi = np.array([1, 1, 0, 1, 1, 1, 1, 1], np.uint8)
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, hi)
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 2, Tp, C.byref(h)) == 3
    assert b"partial h_update_ind" in lib.snmf_last_error()
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 2, 0.0, None, None)
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 2, Tp, C.byref(h)) == 8
    assert b"r x n matrix" in lib.snmf_last_error()
    # F = 600 and r = 300 are outside the fp32 batch's envelope only: what refuses them here is the zero frame count
    sp = _make_params(600, 1, 300, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, C.c_void_p(Tz.ctypes.data), C.byref(h)) == 8
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 2, C.c_void_p(Tz.ctypes.data), C.byref(h)) == 1
    # more problems than a launch grid's second dimension: refused with the limit, before anything is allocated
    Tbig = np.ones(65536, np.int32)
    sp = _make_params(8, 1, 2, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_batch_create_fp64(ctx, C.byref(sp), 65536, C.c_void_p(Tbig.ctypes.data), C.byref(h)) == 8
    assert b"65535" in lib.snmf_last_error()
    assert h.value is None
    # the one-shot entry
    two = (C.c_void_p * 2)()
    ld = np.array([64, 64], np.int64)
    ldp = C.c_void_p(ld.ctypes.data)
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_sparse_nmf_batch_fp64(None, C.byref(sp), 2, Tp, two, ldp, two, two, None, two, two, None, None, None) == 1
    assert lib.snmf_sparse_nmf_batch_fp64(ctx, None, 2, Tp, two, ldp, two, two, None, two, two, None, None, None) == 1
    assert lib.snmf_sparse_nmf_batch_fp64(ctx, C.byref(sp), 2, None, two, ldp, two, two, None, two, two, None, None, None) == 1
    assert lib.snmf_sparse_nmf_batch_fp64(ctx, C.byref(sp), 2, Tp, two, ldp, two, two, None, two, two, None, None, None) == 1  # NULL arrays
    assert b"NULL" in lib.snmf_last_error()
    a = np.ones(64 * 8)
    full = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    args = lambda spx, n, Tx: (ctx, C.byref(spx), n, Tx, full, ldp, full, full, None, full, full, None, None, None)  # noqa: E731
    assert lib.snmf_sparse_nmf_batch_fp64(*args(sp, 0, Tp)) == 1  # an empty batch
    assert lib.snmf_sparse_nmf_batch_fp64(*args(sp, 2, C.c_void_p(Tz.ctypes.data))) == 1  # a zero frame count
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, hi)
    assert lib.snmf_sparse_nmf_batch_fp64(*args(sp, 2, Tp)) == 3
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 2, 0.0, None, None)
    assert lib.snmf_sparse_nmf_batch_fp64(*args(sp, 2, Tp)) == 8
