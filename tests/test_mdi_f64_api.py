"""The `precision` keyword of snmf_mdi / snmf_mdi_Sm / dnmf_adapt (the fp64 missing-data solve, snmf_mdi_fp64): what is
decided on the host, before any device work.  Runs without a GPU.  The solve itself is judged in tests/test_gpu_mdi_f64.py."""
import inspect
import os
import re

import numpy as np
import pytest

from se_snmf_nat_amd import SnmfError, dnmf_adapt, snmf_mdi, snmf_mdi_Sm
from se_snmf_nat_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = np.ones((6, 5))
M = np.ones((6, 5))
OK = dict(r=2, cost_check=1, max_iter=2)


@pytest.fixture
def no_library(monkeypatch):
    """Any load of the library, any context and any plan is a failure: the rules under test come before all of them."""
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(api, "default_context", boom)
    monkeypatch.setattr(api, "Plan", boom)


def test_precision_keyword_defaults_to_fp32():
    for fn in (snmf_mdi, snmf_mdi_Sm, dnmf_adapt):
        par = inspect.signature(fn).parameters["precision"]
        assert par.default == "fp32" and par.kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (snmf_mdi, snmf_mdi_Sm):
        par = inspect.signature(fn).parameters["info"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("fn", [snmf_mdi, snmf_mdi_Sm])
def test_unknown_precision_is_a_value_error_before_any_library_call(no_library, fn):
    for bad in ("fp16", "FP64", None):
        with pytest.raises(ValueError, match="precision"):
            fn(V, M, OK, precision=bad)


@pytest.mark.parametrize("fn", [snmf_mdi, snmf_mdi_Sm])
def test_fp64_with_float32_buffers_is_invalid_before_any_library_call(no_library, fn):
    with pytest.raises(SnmfError) as e:
        fn(V, M, OK, precision="fp64", dtype=np.float32)
    assert e.value.status == 1


def test_dnmf_adapt_rules_fire_before_any_library_call(no_library):
    B = np.ones((6, 4))
    p = dict(R_x=2, R_d=2, cost_check=1, max_iter=2)
    with pytest.raises(ValueError, match="precision"):
        dnmf_adapt(V, V, B, p, precision="fp16")
    with pytest.raises(SnmfError) as e:
        dnmf_adapt(V, V, B, p, precision="fp64", dtype=np.float32)
    assert e.value.status == 1


@pytest.mark.parametrize("fn", [snmf_mdi, snmf_mdi_Sm])
@pytest.mark.parametrize("kw", [dict(), dict(precision="fp64"), dict(precision="fp64", dtype=np.float32), dict(precision="fp16")],
                         ids=["fp32", "fp64", "fp64-float32", "fp16"])
def test_reference_errors_come_first_in_both_precisions(no_library, fn, kw):
    """src/snmf_mdi.m:87-93: the defaults of sparsity_mdi / conv_eps_mdi are installed only when p.sparsity / p.conv_eps are
    ABSENT; p.cost_check has no default; :117-119 neither r nor init_w."""
    with pytest.raises(KeyError, match="sparsity_mdi"):
        fn(V, M, dict(r=2, cost_check=1, sparsity=5), **kw)
    with pytest.raises(KeyError, match="conv_eps_mdi"):
        fn(V, M, dict(r=2, cost_check=1, conv_eps=1e-3), **kw)
    with pytest.raises(KeyError, match="cost_check"):
        fn(V, M, dict(r=2), **kw)
    with pytest.raises(SnmfError, match="Number of components or initialization must be given") as e:
        fn(V, M, dict(cost_check=1), **kw)
    assert e.value.status == 2
    with pytest.raises(SnmfError, match="mask") as e:
        fn(V, M[:, 1:], OK, **kw)
    assert e.value.status == 3
    with pytest.raises(SnmfError, match="init_h"):
        fn(V, M, dict(OK, init_w=np.ones((6, 2)), init_h=np.ones((3, 5))), **kw)


def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "snmf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    mt = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert mt, f"{name} is not declared in include/snmf.h"
    return [a.strip() for a in mt.group(1).split(",")]


def test_fp64_entry_is_declared_and_bound(lib):
    args = _prototype("snmf_mdi_fp64")
    assert "snmf_mdi_fp64" in _lib.SYMBOLS
    assert len(args) == len(lib.snmf_mdi_fp64.argtypes) == 16
    # the plain fp64 entry plus the mask, its leading dimension, V_mdi and its leading dimension
    assert len(_prototype("snmf_sparse_nmf_fp64")) == len(lib.snmf_sparse_nmf_fp64.argtypes) == 12
    for a, ty in zip(args, lib.snmf_mdi_fp64.argtypes):
        assert ("int64_t" in a and "*" not in a) == (ty is _lib.C.c_int64), (a, ty)
    assert lib.snmf_mdi_fp64(*([None] * 3), 0, None, 0, *([None] * 4), 0, *([None] * 5)) == 1  # ctx is NULL


def test_fp64_without_a_device_fails_loudly(lib):
    """No CPU fallback in this mode either: without a device the call ends in NO_DEVICE; with one it must solve."""
    if lib.snmf_device_count() > 0:
        info = {}
        v, h, obj = snmf_mdi(V, M, OK, precision="fp64", info=info)
        assert v.shape == (6, 5) and h.shape == (2, 5) and obj["n_iter"] == 2 and info["w"].shape == (6, 2)
        return
    with pytest.raises(SnmfError, match="NO_DEVICE"):
        snmf_mdi(V, M, OK, precision="fp64")
    with pytest.raises(SnmfError, match="NO_DEVICE"):
        snmf_mdi_Sm(V, M, OK, precision="fp64")
