"""The `precision` keyword of sparse_nmf / sparse_nmf_GPU (the fp64 solve mode, snmf_sparse_nmf_fp64): what is decided on
the host, before any device work.  Runs without a GPU.  The solve itself is judged in tests/test_gpu_solve_f64.py."""
import inspect

import numpy as np
import pytest

from se_snmf_nat_amd import SnmfError, sparse_nmf, sparse_nmf_GPU

V = np.ones((6, 5))


def test_precision_keyword_defaults_to_fp32():
    for fn in (sparse_nmf, sparse_nmf_GPU):
        par = inspect.signature(fn).parameters["precision"]
        assert par.default == "fp32" and par.kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("fn", [sparse_nmf, sparse_nmf_GPU])
def test_unknown_precision_is_a_value_error(fn):
    with pytest.raises(ValueError, match="precision"):
        fn(V, dict(r=2, cost_check=1), precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        fn(V, dict(r=2, cost_check=1), precision="FP64")


@pytest.mark.parametrize("fn", [sparse_nmf, sparse_nmf_GPU])
def test_fp64_with_float32_buffers_is_invalid(fn):
    with pytest.raises(SnmfError) as e:
        fn(V, dict(r=2, cost_check=1), precision="fp64", dtype=np.float32)
    assert e.value.status == 1


def test_fp64_over_a_device_list_is_unsupported():
    with pytest.raises(SnmfError) as e:
        sparse_nmf(V, dict(r=2, cost_check=1), precision="fp64", devices=[0, 1])
    assert e.value.status == 8


def test_reference_errors_come_first():
    """src/sparse_nmf.m:117-119 and :260 are raised as without the keyword, also where the combination is refused."""
    for kw in (dict(precision="fp64"), dict(precision="fp64", dtype=np.float32), dict(precision="fp64", devices=[0, 1])):
        with pytest.raises(SnmfError, match="Number of components or initialization must be given") as e:
            sparse_nmf(V, dict(cost_check=1), **kw)
        assert e.value.status == 2
        with pytest.raises(SnmfError, match="cost_check") as e:
            sparse_nmf(V, dict(r=2), **kw)
        assert e.value.status == 4
    with pytest.raises(SnmfError, match="h_update_ind"):
        sparse_nmf(V, dict(r=2, cost_check=1, h_update_ind=[1, 0, 1]), precision="fp64")  # wrong length: host-side DIM


def test_fp64_entry_is_bound(lib):
    from se_snmf_nat_amd import _lib
    assert "snmf_sparse_nmf_fp64" in _lib.SYMBOLS
    assert lib.snmf_sparse_nmf_fp64.argtypes == lib.snmf_sparse_nmf_oop_f64.argtypes
    assert lib.snmf_sparse_nmf_fp64(None, None, None, 0, None, None, None, None, None, None, None, None) == 1  # ctx is NULL


def test_fp64_without_a_device_fails_loudly(lib):
    """No CPU fallback in this mode either: without a device the call ends in NO_DEVICE; with one it must solve."""
    p = dict(r=2, cost_check=1, max_iter=2)
    if lib.snmf_device_count() > 0:
        w, h, obj = sparse_nmf(V, p, precision="fp64")
        assert w.shape == (6, 2) and h.shape == (2, 5) and obj["n_iter"] == 2
        return
    with pytest.raises(SnmfError, match="NO_DEVICE"):
        sparse_nmf(V, p, precision="fp64")
    with pytest.raises(SnmfError, match="NO_DEVICE"):
        sparse_nmf_GPU(V, dict(r=2), precision="fp64")
