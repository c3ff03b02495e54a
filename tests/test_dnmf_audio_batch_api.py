"""CPU tests of the batched front-end and of run_basis_DNMF_batch / run_basis_DNMF_Mel_batch (snmf_stft_features_batch_*,
snmf_run_basis_dnmf_audio_batch_*): the Python-side errors fire before the library is loaded, the four C names stand in the
header and in the binding, the Python names are exported, the wrapper's frame count is the library's around the frame edges, the
C entries refuse bad arguments without a device, and the waveforms of the GPU tests stop where those tests need them to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dnmf_audio_batch_cases as ac
import dnmf_batch_cases as dc
import frontend_envelope as env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ["snmf_stft_features_batch_f32", "snmf_stft_features_batch_fp64", "snmf_run_basis_dnmf_audio_batch_f64",
           "snmf_run_basis_dnmf_audio_batch_fp64"]


def test_every_argument_error_is_raised_before_any_library_call(monkeypatch):
    from se_snmf_nat_amd import _lib, frontend, train
    from se_snmf_nat_amd.train import run_basis_DNMF_batch, run_basis_DNMF_Mel_batch

    def no_device(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(train, "default_context", no_device)
    monkeypatch.setattr(frontend, "default_context", no_device)
    p = ac.P_STOP
    r = ac.R_X + ac.R_D
    x, d = ac.waves()[3]
    T = ac.TS[3]
    B, H = np.ones((ac.F, r)), np.ones((r, T))

    def status(xs, ds, Bq=B, pq=p, fn=run_basis_DNMF_batch, **kw):
        with pytest.raises(_lib.SnmfError) as e:
            fn(xs, ds, Bq, pq, **kw)
        return e.value.status

    assert status([], []) == 1                                            # an empty batch
    assert status([x, x], [d]) == 1                                       # lists of different lengths
    assert status([x], [d, d]) == 1
    assert status([x], [d], Bq=np.ones((ac.F, r + 1))) == 3               # B of the wrong shape
    assert status([x], [d], Bq=np.ones((ac.F + 1, r))) == 3
    assert status([x, x], [d, d], Bq=[B]) == 3                            # B of the wrong list length
    assert status([x, x], [d, d], Bq=[B, B[:-1]]) == 3
    assert status([x], [d], fn=run_basis_DNMF_Mel_batch) == 3             # the Mel twin wants F_order * (2 Splice + 1) rows
    assert status([x], [d], h0=[np.ones((r, T + 1))]) == 3                # h0 of the wrong shape
    assert status([x, x], [d, d], h0=[H]) == 3                            # h0 of the wrong list length
    assert status([x], [d], h0="philox") == 3
    assert status([x, x[:ac.N + 1]], [d, d]) == 3                         # a problem shorter than one analysis frame
    assert status([x], [d], pq={k: v for k, v in p.items() if k != "cost_check"}) == 4   # src/sparse_nmf.m:260
    assert status([x], [d], pq=dict(p, sparsity=np.ones(r))) == 3         # a non-scalar sparsity
    assert status([x], [d], precision="fp64", dtype=np.float32) == 1      # the fp64 mode takes doubles
    assert status([x], [d], dtype=np.int32) == 1
    with pytest.raises(ValueError):
        run_basis_DNMF_batch([x], [d], B, p, precision="bf16")
    with pytest.raises(_lib.SnmfError) as e:
        frontend.stft_features_batch([], ac.TINY)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        frontend.stft_features_batch([x], ac.TINY, precision="bf16")
    # valid calls pass every check and only then reach the library
    for kw in (dict(h0=[H, H]), dict(h0="device"), dict(h0="host", precision="fp64"), dict(precision="fp64", dtype=np.float64)):
        with pytest.raises(AssertionError, match="reached the library"):
            run_basis_DNMF_batch([x, x], [d, d], [B, B], p, **kw)
    with pytest.raises(AssertionError, match="reached the library"):
        run_basis_DNMF_Mel_batch([x], [d], np.ones((8, r)), p)
    with pytest.raises(AssertionError, match="reached the library"):
        frontend.stft_features_batch([x, d], ac.TINY, mel=True)


def test_c_names_stand_in_the_header_and_in_the_binding_once():
    from se_snmf_nat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snmf.h")).read(), flags=re.S)
    for nm in C_NAMES:
        assert len(re.findall(r"\b%s\s*\(" % nm, txt)) == 1, nm
        assert _lib.SYMBOLS.count(nm) == 1, nm


def test_python_names_are_exported():
    import se_snmf_nat_amd as pkg
    from se_snmf_nat_amd import frontend, train
    assert pkg.run_basis_DNMF_batch is train.run_basis_DNMF_batch
    assert pkg.run_basis_DNMF_Mel_batch is train.run_basis_DNMF_Mel_batch
    assert pkg.stft_features_batch is frontend.stft_features_batch


@pytest.mark.parametrize("N,shift", [(64, 10), (64, 1), (512, 160), (1024, 160), (4096, 4096)])
def test_the_wrappers_frame_count_is_the_librarys_around_the_frame_edges(lib, N, shift):
    from se_snmf_nat_amd import frontend as fe
    p = dict(ac.TINY, fftlength=N, framelength=min(40, N), frameshift=shift)
    sp, _win = fe._params(p)
    lengths = [0, 1, N - 1, N, N + 1, N + 2, N + 3]
    for T in (1, 2, 3, 31, 32, 33):
        lengths += [N + 1 + T * shift + e for e in (-1, 0, 1, 2)]
    for L in lengths:
        assert fe.num_frames_host(L, p) == int(lib.snmf_stft_num_frames(C.byref(sp), L)), L
    assert [fe.num_frames_host(ac.n_samples(T), ac.TINY) for T in ac.TS] == ac.TS and fe.num_frames_host(ac.N + 1, ac.TINY) == 0


def test_c_entries_refuse_bad_arguments_without_a_device(lib):
    """What the entries refuse comes before the device is touched, so it can be checked where there is none."""
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    sp, _win = fe._params(ac.TINY)
    q = _make_params(ac.F, 1, ac.R_X + ac.R_D, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    for ty in ("f32", "fp64"):
        fn = getattr(lib, f"snmf_stft_features_batch_{ty}")
        assert fn(None, C.byref(sp), 1, None, None, None, 0, None, None) == 1
    for ty in ("f64", "fp64"):
        fn = getattr(lib, f"snmf_run_basis_dnmf_audio_batch_{ty}")
        assert fn(None, C.byref(q), C.byref(sp), ac.R_X, ac.R_D, 1, None, None, None, None, None, 0, None, None, None, None, None, None) == 1


def test_the_waveforms_stop_where_the_gpu_tests_need_them_to():
    """Solve 1 of the six problems on the oracle (fp64 reference features): one runs to max_iter, the others stop at odd and at
    even iterates, so problems of one batch end at different iterations."""
    n1 = []
    for (x, d), B, H0 in zip(ac.waves(), ac.bases(), ac.given_h0()):
        n = min(len(x), len(d))
        Y, X, D = (env.features(s, ac.TINY) for s in (x[:n] + d[:n], x[:n], d[:n]))
        assert Y.shape == (ac.F, H0.shape[1])
        n1.append(dc.oracle_dnmf(Y, X, D, B, H0, ac.R_X, ac.R_D, ac.P_STOP)[2][0])
    print("oracle solve-1 stop indices:", n1)
    assert dc.covers_both_buffers(n1, ac.P_STOP["max_iter"])
