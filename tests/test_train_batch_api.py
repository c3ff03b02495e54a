"""CPU tests of run_basis_train_signal_batch (snmf_run_basis_train_audio_batch_*): the Python-side errors fire before the library
is loaded, the two C names stand in the header and in the binding, the Python name is exported, the C entries refuse NULL
arguments without a device, and the signals of the GPU tests stop where those tests need them to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import train_batch_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ["snmf_run_basis_train_audio_batch_f64", "snmf_run_basis_train_audio_batch_fp64"]


def test_every_argument_error_is_raised_before_any_library_call(monkeypatch):
    from se_snmf_nat_amd import _lib, frontend, train
    from se_snmf_nat_amd.train import run_basis_train_signal_batch

    def no_device(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(train, "default_context", no_device)
    monkeypatch.setattr(frontend, "default_context", no_device)
    p = tc.P_STOP
    s, T = tc.signals()[3], tc.TS[3]
    ix = tc.sample_idx()[3]

    def status(sigs, R=tc.R, pq=p, **kw):
        with pytest.raises(_lib.SnmfError) as e:
            run_basis_train_signal_batch(sigs, R, pq, **kw)
        return e.value.status

    assert status([]) == 1                                                     # an empty batch
    assert status([s, s], sample_idx=[ix]) == 3                                # list lengths that disagree
    assert status([s], sample_idx=[ix, ix]) == 3
    assert status([s, s[:tc.N + 1]]) == 3                                      # a signal shorter than one analysis frame
    assert status([s, tc.signals()[0]], R=tc.TS[0] + 1) == 3                   # cluster_buff * R > T_k
    assert status([s, tc.signals()[0]], R=4, pq=dict(p, cluster_buff=2)) == 3
    assert status([s], sample_idx=[np.r_[ix[:-1], T + 1]]) == 3                # an index outside [1, T_k]
    assert status([s], sample_idx=[np.r_[ix[:-1], 0]]) == 3
    assert status([s], sample_idx=[ix[:-1]]) == 3                              # not cluster_buff * R of them
    assert status([s], R=3, pq=dict(p, cluster_buff=2, train_Exemplar=1)) == 3  # run_basis_train.m:125-126
    assert status([s], pq={k: v for k, v in p.items() if k != "cost_check"}) == 4   # src/sparse_nmf.m:260
    assert status([s], pq=dict(p, sparsity=np.ones(tc.R))) == 3                # a non-scalar sparsity
    assert status([s], h0="philox") == 3
    assert status([s], pq=dict(p, win_STFT=p["win_STFT"][:-1])) == 3
    with pytest.raises(ValueError):
        run_basis_train_signal_batch([s], tc.R, p, precision="bf16")
    # valid calls pass every check and only then reach the library
    for kw in (dict(), dict(h0="device"), dict(precision="fp64"), dict(sample_idx=[ix, ix]), dict(DC_bin=2),
               dict(precision="fp64", h0="device", sample_idx=[ix, ix])):
        with pytest.raises(AssertionError, match="reached the library"):
            run_basis_train_signal_batch([s, s], tc.R, p, **kw)
    for q in (dict(p, train_Exemplar=1), dict(p, cluster_buff=2), dict(p, domain_DD=1, alpha_eta=0.4),
              {k: v for k, v in dict(p, train_Exemplar=1).items() if k != "cost_check"}):  # (no solve, no cost_check: as the single call)
        with pytest.raises(AssertionError, match="reached the library"):
            run_basis_train_signal_batch([s, tc.signals()[5]], 3, q)


def test_c_names_stand_in_the_header_and_in_the_binding_once():
    from se_snmf_nat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snmf.h")).read(), flags=re.S)
    for nm in C_NAMES:
        assert len(re.findall(r"\b%s\s*\(" % nm, txt)) == 1, nm
        assert _lib.SYMBOLS.count(nm) == 1, nm


def test_python_name_is_exported():
    import se_snmf_nat_amd as pkg
    from se_snmf_nat_amd import train
    assert pkg.run_basis_train_signal_batch is train.run_basis_train_signal_batch


def test_c_entries_refuse_null_arguments_without_a_device(lib):
    """What the entries refuse comes before the device is touched, so it can be checked where there is none."""
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    sp, _win = fe._params(tc.TINY)
    q = _make_params(tc.F, 1, tc.R, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    for ty in ("f64", "fp64"):
        fn = getattr(lib, f"snmf_run_basis_train_audio_batch_{ty}")
        assert fn.argtypes is not None
        assert fn(None, C.byref(q), C.byref(sp), -1.0, None, 0, 1, None, None, None, 0, None, None, None, None, None, None, None) == 1
        assert fn(None, None, None, -1.0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None, None) == 1


def test_the_signals_stop_where_the_gpu_tests_need_them_to():
    """The DFT solves of the six problems on the oracle (fp64 reference features): at least one runs to max_iter, the others stop
    on their own at no fewer than two different iterations, so the problems of one batch end at different iterations."""
    n = tc.oracle_stop_indices()
    print("oracle stop indices [n_dft, n_mel] per problem:", n)
    n_dft = [a for a, _ in n]
    assert tc.stops_are_spread(n_dft, tc.P_STOP["max_iter"]), n_dft
    assert {a % 2 for a in n_dft if a < tc.P_STOP["max_iter"]} == {0, 1}, n_dft  # (both H buffers of the fp32 engine hold a stop iterate)
