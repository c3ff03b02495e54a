"""CPU tests of the batched offline solve's host side (se_snmf_nat_amd/batch.py): the reference's own errors and the
batch's refusals are raised in Python, in sparse_nmf's words, before the library is loaded or a context is made."""
import numpy as np
import pytest


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
    assert callable(pkg.sparse_nmf_batch) and isinstance(pkg.BatchPlan, type)


def test_reference_errors_before_any_device_call(no_device):
    from se_snmf_nat_amd import SnmfError, sparse_nmf_batch
    vs = _vs()
    w0 = np.ones((6, 2))
    with pytest.raises(SnmfError, match="rows") as e:  # differing row counts
        sparse_nmf_batch([vs[0], np.ones((7, 4))], dict(init_w=w0, cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="rows") as e:  # ... also without an init_w to compare with
        sparse_nmf_batch([vs[0], np.ones((7, 4))], dict(r=2, cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_w is a list of 2") as e:
        sparse_nmf_batch(vs, dict(init_w=[w0, w0], cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_w") as e:  # (7, 2) against 6 rows, sparse_nmf's words
        sparse_nmf_batch(vs, dict(init_w=np.ones((7, 2)), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match=r"init_h is \(3, 3\), expected \(2, 3\)") as e:
        sparse_nmf_batch(vs, dict(init_w=w0, init_h=[np.ones((2, 5)), np.ones((3, 3)), np.ones((2, 8))], cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_h must be a list of 3") as e:
        sparse_nmf_batch(vs, dict(init_w=w0, init_h=[np.ones((2, 5))], cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="cost_check") as e:  # src/sparse_nmf.m:260
        sparse_nmf_batch(vs, dict(init_w=w0))
    assert e.value.status == 4
    with pytest.raises(SnmfError, match="Number of components or initialization must be given") as e:  # :117-119
        sparse_nmf_batch(vs, dict(cost_check=1))
    assert e.value.status == 2


def test_batch_refusals_before_any_device_call(no_device):
    from se_snmf_nat_amd import BatchPlan, SnmfError, sparse_nmf_batch
    vs = _vs()
    w0 = np.ones((6, 4))
    with pytest.raises(SnmfError, match="partial h_update_ind") as e:
        sparse_nmf_batch(vs, dict(init_w=w0, h_update_ind=np.array([1, 1, 0, 1], bool), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="r x n matrix") as e:  # a sparsity matrix has no batched form
        sparse_nmf_batch(vs, dict(init_w=w0, sparsity=np.ones((4, 5)), cost_check=1))
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="sparsity column has 3 rows") as e:
        sparse_nmf_batch(vs, dict(init_w=w0, sparsity=np.ones(3), cost_check=1))
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="empty") as e:
        sparse_nmf_batch([], dict(init_w=w0, cost_check=1))
    assert e.value.status == 1
    for bad in ("fp64", "bf16", None):
        with pytest.raises(ValueError, match="precision"):
            sparse_nmf_batch(vs, dict(init_w=w0, cost_check=1), precision=bad)
        with pytest.raises(ValueError, match="precision"):
            BatchPlan(None, 6, 4, [5, 3], precision=bad)
    with pytest.raises(SnmfError, match="partial h_update_ind") as e:
        BatchPlan(None, 6, 4, [5, 3], h_update_ind=[1, 0, 1, 1])
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="r x n matrix") as e:
        BatchPlan(None, 6, 4, [5, 3], sparsity=np.ones((4, 5)))
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="empty") as e:
        BatchPlan(None, 6, 4, [])
    assert e.value.status == 1


def test_c_entries_reject_null_and_refuse_outside_the_envelope(lib):
    """The C entries check their arguments before they touch a device: NULL -> 1, F / r above the envelope -> 8 with the
    limit in the message, a partial h_update_ind -> 3, a sparsity matrix -> 8."""
    import ctypes as C
    from se_snmf_nat_amd.api import _make_params
    assert lib.snmf_batch_run(None, 0) == 1
    assert lib.snmf_batch_get_f64(None, 0, None, None, None, None, None) == 1
    assert lib.snmf_batch_set_problem_f64(None, 0, None, 1, None, None) == 1
    assert lib.snmf_batch_describe(None, None, 0) == 1
    lib.snmf_batch_destroy(None)
    T = np.array([5, 3], np.int32)
    h = C.c_void_p()
    ctx = C.c_void_p(1)  # never dereferenced by the checks below
    sp = _make_params(600, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, C.c_void_p(T.ctypes.data), C.byref(h)) == 8
    assert b"513" in lib.snmf_last_error()
    sp = _make_params(64, 1, 300, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, C.c_void_p(T.ctypes.data), C.byref(h)) == 8
    assert b"200" in lib.snmf_last_error()
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 2, 0.0, None, None)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, C.c_void_p(T.ctypes.data), C.byref(h)) == 8
    hi = np.array([1, 1, 0, 1, 1, 1, 1, 1], np.uint8)
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, hi)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, C.c_void_p(T.ctypes.data), C.byref(h)) == 3
    sp = _make_params(64, 1, 8, 1.0, 10, 0.0, 1, 1, 0, 0.0, None, None)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 0, C.c_void_p(T.ctypes.data), C.byref(h)) == 1
    Tz = np.array([5, 0], np.int32)
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, C.c_void_p(Tz.ctypes.data), C.byref(h)) == 1
    assert lib.snmf_batch_create(ctx, C.byref(sp), 2, None, C.byref(h)) == 1
