"""The CPU side of tests/test_gpu_frontend_envelope.py: what its references and its fp32 bound rest on.

    frame count      the oracle's loop fills exactly snmf_stft_num_frames columns wherever frameshift <= fftlength
    splice           frontend_envelope.splice_zero_outside is the oracle's frame_splice to the bit where that can run (T > Splice)
    fp32 bound       1e-4 |ref| + 2e-6 colmax (tests/test_frontend.py::_close) holds a single-precision restatement of the chain
                     (float32 pre-emphasis and window, complex64 FFT) within a quarter of itself on every case of the table:
                     measured <= 0.046 of the bound (n4096_odd_len_shiftN_pow05), <= 2.3e-7 of the column maximum
"""
import ctypes as C

import numpy as np
import pytest

import frontend_envelope as env
from oracle import frontend_oracle as fo


def test_oracle_fills_exactly_num_frames_columns_at_every_size(lib):
    from se_snmf_nat_amd._lib import SnmfStftParams
    for N in env.SIZES:
        for fl in (N, N // 2 + 3, 1):
            for shift in (1, N // 8 + 1, N):
                sp = SnmfStftParams()
                sp.framelength, sp.frameshift, sp.fftlength, sp.dcbin = fl, shift, N, 1
                for extra in (1, 2, 1 + shift, 2 + shift, 3 + shift, 2 + 4 * shift):
                    L = N + extra
                    want = max(0, -(-(L - N - 1) // shift))  # ceil((L - N - 1) / shift)
                    assert lib.snmf_stft_num_frames(C.byref(sp), L) == want
                    S = fo.stft_fft(env.signal(L, 1), fl, shift, N, 1, env.window(fl), 0.0)
                    assert S.shape[1] >= want
                    assert int(np.any(S != 0, axis=0).sum()) == want and not S[:, want:].any(), (N, fl, shift, extra)
    # L - N = 1, 2, 1 + shift, 2 + shift, 3 + shift: 0, 1, 1, 2, 2 frames (a frame starts wherever 1 + i * shift < L - N)
    assert [max(0, -(-(e - 1) // 9)) for e in (1, 2, 10, 11, 12)] == [0, 1, 1, 2, 2]


def test_the_table_reaches_every_size_and_option():
    c = env.STFT_CASES.values()
    assert {p["fftlength"] for p in c} == set(env.SIZES)
    for p in c:
        N = p["fftlength"]
        assert p["frameshift"] <= N and p["framelength"] in (N, N // 2 + 3, 1) and p["frameshift"] in (1, N // 8 + 1, N)
        assert N + 2 + (p["T"] - 1) * p["frameshift"] == env.n_samples(p)
    assert {p["pow"] for p in c} == {2, 1, 0.7, 0.5} and {p["preemph"] for p in c} == {0.0, 0.92}
    assert {(p["Splice"], p["T"]) for p in c if p["Splice"]} >= {(1, 1), (1, 2), (1, 5), (2, 1), (2, 2), (2, 5)}
    assert any(p["DCbin"] == p["fftlength"] // 2 + 1 for p in c) and any(p["DCbin"] == 1 for p in c)
    for kind in (lambda p: p["framelength"] == p["fftlength"], lambda p: p["framelength"] == 1, lambda p: p["frameshift"] == 1,
                 lambda p: p["frameshift"] == p["fftlength"], lambda p: p["framelength"] == p["fftlength"] // 2 + 3,
                 lambda p: p["frameshift"] == p["fftlength"] // 8 + 1):
        assert any(kind(p) for p in c)


@pytest.mark.parametrize("name", sorted(env.STFT_CASES))
def test_reference_is_the_oracle_and_single_precision_stays_within_a_quarter_of_the_fp32_bound(name):
    p, s, ref = env.STFT_CASES[name], env.case_signal(name), env.case_reference(name)
    assert ref.shape == ((2 * p["Splice"] + 1) * (p["fftlength"] // 2 + 1), p["T"])
    if p["T"] > p["Splice"]:
        assert fo.dft_features(s, p).tobytes() == ref.tobytes()
    else:  # the reference's loop reads column t + sft of a T-column matrix (src/frame_splice.m:12)
        with pytest.raises(IndexError):
            fo.dft_features(s, p)
        K = p["fftlength"] // 2 + 1
        blocks = ref.reshape(-1, K, p["T"])
        for d in range(-p["Splice"], p["Splice"] + 1):
            for t in range(p["T"]):
                if not 0 <= t + d < p["T"]:
                    assert (blocks[p["Splice"] + d, :, t] == p["nonzerofloor"]).all()
    got = env.features_single(s, p)
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref)
    cm = env.colmax(ref, p)
    bound = 1e-4 * np.abs(ref) + 2e-6 * cm
    print(f"single-precision restatement {name}: max err/bound = {float((err / bound).max()):.3f}  max err/colmax = {float((err / cm).max()):.2e}")
    assert (err <= 0.25 * bound).all(), float((err / bound).max())
