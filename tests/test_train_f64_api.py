"""The `precision` keyword of the front-end, the DNMF loop and the basis-training caller (the fp64 mode: snmf_*_fp64 of
include/snmf.h): what is decided on the host, before any device work, and how the new entries are bound.  Runs without a
GPU.  The computation itself is judged in tests/test_gpu_train_f64.py."""
import inspect

import numpy as np
import pytest

from se_snmf_nat_amd import SnmfError, api, frontend, train

P_FE = frontend.default_params()
P_SOLVE = dict(cf="kl", sparsity=5, max_iter=2, conv_eps=0, cost_check=1)
P_DNMF = dict(P_FE, **P_SOLVE, R_x=2, R_d=3, random_seed=1)
Y = np.ones((6, 5))
B = np.ones((6, 5))
SIG = np.ones(4000)

KEYWORD_FUNCTIONS = [api.run_basis_dnmf, train.run_basis_DNMF, train.run_basis_DNMF_Mel, train.run_basis_train_signal,
                     frontend.stft_features, frontend.mel_features, frontend.tf_dd]


def calls(precision, **kw):
    """One call of each of the seven functions with the given precision."""
    return [
        lambda: api.run_basis_dnmf(Y, Y, Y, B, 2, 3, P_SOLVE, precision=precision, **kw),
        lambda: train.run_basis_DNMF(SIG, SIG, np.ones((513, 5)), P_DNMF, precision=precision, **kw),
        lambda: train.run_basis_DNMF_Mel(SIG, SIG, np.ones((64, 5)), P_DNMF, precision=precision, **kw),
        lambda: train.run_basis_train_signal(SIG, 2, dict(P_FE, **P_SOLVE), sample_idx=[1, 2], precision=precision),
        lambda: frontend.stft_features(SIG, P_FE, precision=precision),
        lambda: frontend.mel_features(np.ones((513, 3)), P_FE, precision=precision),
        lambda: frontend.tf_dd(np.ones((4, 3)), {"alpha_eta": 0.4}, precision=precision),
    ]


@pytest.mark.parametrize("fn", KEYWORD_FUNCTIONS, ids=lambda f: f.__name__)
def test_precision_keyword_is_keyword_only_and_defaults_to_fp32(fn):
    par = inspect.signature(fn).parameters["precision"]
    assert par.default == "fp32" and par.kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("i", range(7), ids=[f.__name__ for f in KEYWORD_FUNCTIONS])
def test_unknown_precision_is_a_value_error(i):
    for bad in ("fp16", "FP64", "double"):
        with pytest.raises(ValueError, match="precision"):
            calls(bad)[i]()


def test_fp64_with_float32_buffers_is_invalid():
    for call in calls("fp64", dtype=np.float32)[:3]:
        with pytest.raises(SnmfError) as e:
            call()
        assert e.value.status == 1
    with pytest.raises(SnmfError) as e:  # the three separate calls refuse it as sparse_nmf does
        api.run_basis_dnmf(Y, Y, Y, B, 2, 3, P_SOLVE, precision="fp64", dtype=np.float32, resident=False)
    assert e.value.status == 1


@pytest.mark.parametrize("resident", [True, False])
def test_fp64_over_a_device_list_is_unsupported(resident):
    with pytest.raises(SnmfError) as e:
        api.run_basis_dnmf(Y, Y, Y, B, 2, 3, P_SOLVE, precision="fp64", devices=[0, 1], resident=resident)
    assert e.value.status == 8


def test_reference_errors_come_first():
    """A missing cost_check (src/sparse_nmf.m:260) and the shape mismatches are raised as without the keyword, also where
    the combination is refused."""
    no_cc = {k: v for k, v in P_SOLVE.items() if k != "cost_check"}
    for kw in (dict(), dict(dtype=np.float32), dict(devices=[0, 1])):
        for resident in (True, False):
            with pytest.raises(SnmfError, match="cost_check") as e:
                api.run_basis_dnmf(Y, Y, Y, B, 2, 3, no_cc, precision="fp64", resident=resident, **kw)
            assert e.value.status == 4
        with pytest.raises(SnmfError) as e:
            api.run_basis_dnmf(Y, Y[:, :4], Y, B, 2, 3, P_SOLVE, precision="fp64", **kw)
        assert e.value.status == 3
        with pytest.raises(SnmfError) as e:
            api.run_basis_dnmf(Y, Y, Y, B[:, :4], 2, 3, P_SOLVE, precision="fp64", **kw)
        assert e.value.status == 3
    p_no_cc = {k: v for k, v in P_DNMF.items() if k != "cost_check"}
    for fn, rows in ((train.run_basis_DNMF, 513), (train.run_basis_DNMF_Mel, 64)):
        for kw in (dict(), dict(dtype=np.float32)):
            with pytest.raises(SnmfError, match="cost_check") as e:
                fn(SIG, SIG, np.ones((rows, 5)), p_no_cc, precision="fp64", **kw)
            assert e.value.status == 4
            with pytest.raises(SnmfError) as e:
                fn(SIG, SIG, np.ones((rows + 1, 5)), P_DNMF, precision="fp64", **kw)
            assert e.value.status == 3
    with pytest.raises(SnmfError, match="cost_check") as e:
        train.run_basis_train_signal(SIG, 2, dict(P_FE, **no_cc), sample_idx=[1, 2], precision="fp64")
    assert e.value.status == 4


NAMESAKES = {"snmf_stft_features_fp64": "snmf_stft_features_f32", "snmf_mel_features_fp64": "snmf_mel_features_f32",
             "snmf_tf_dd_fp64": "snmf_tf_dd_f32", "snmf_run_basis_dnmf_fp64": "snmf_run_basis_dnmf_f64",
             "snmf_run_basis_dnmf_audio_fp64": "snmf_run_basis_dnmf_audio_f64",
             "snmf_run_basis_train_audio_fp64": "snmf_run_basis_train_audio_f64"}


def test_fp64_entries_are_bound(lib):
    from se_snmf_nat_amd import _lib
    assert _lib.ABI_VERSION == 5 and lib.snmf_abi_version() == 5  # added within 5
    for new, old in NAMESAKES.items():
        assert new in _lib.SYMBOLS
        assert getattr(lib, new).argtypes == getattr(lib, old).argtypes, new
        assert getattr(lib, new).restype == getattr(lib, old).restype
        n = len(getattr(lib, new).argtypes)
        args = [0.0 if t is _lib.C.c_double else (0 if t in (_lib.C.c_int, _lib.C.c_int32, _lib.C.c_int64, _lib.C.c_uint64) else None)
                for t in getattr(lib, new).argtypes]
        assert len(args) == n and getattr(lib, new)(*args) == 1, new  # ctx is NULL


def test_fp64_without_a_device_fails_loudly(lib):
    """No CPU fallback in this mode either: without a device every call ends in NO_DEVICE; with one it must compute."""
    if lib.snmf_device_count() > 0:
        b_hat, a_hat = api.run_basis_dnmf(Y, Y, Y, B, 2, 3, P_SOLVE, precision="fp64")
        assert b_hat.shape == (6, 5) and a_hat.shape == (5, 5) and b_hat.dtype == np.float64
        assert frontend.tf_dd(np.ones((4, 3)), {"alpha_eta": 0.4}, precision="fp64").dtype == np.float64
        return
    for call in calls("fp64"):
        with pytest.raises(SnmfError, match="NO_DEVICE"):
            call()
