"""The STFT case table of tests/test_gpu_frontend_envelope.py and its CPU references (a helper, not a test; also read by
scripts/train_f64_sensitivity.py, which measures the fp64 bounds of these cases).

Every case holds frameshift <= fftlength: the oracle preallocates L // shift columns (src/stft_fft.m:17), which is then at
least the snmf_stft_num_frames columns its loop fills (tests/test_frontend_envelope_cpu.py checks the rule).
"""
import functools

import numpy as np

from oracle import frontend_oracle as fo

FS = 16000
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


def window(n):
    """sqrt of the periodic Hann window (settings/initial_setting_SNMF_NAT.m:37), shifted by half a sample so that no entry
    is zero: a framelength of 1 keeps its sample."""
    return np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n))


def case(N, fl, shift, dc, preemph, pw, splice, T):
    return dict(fs=FS, fftlength=N, framelength=fl, frameshift=shift, DCbin=dc, preemph=preemph, pow=pw, Splice=splice,
                nonzerofloor=1e-9, win_STFT=window(fl), T=T)


# fftlength, framelength, frameshift, DCbin, preemph, pow, Splice, frames.  L = N + 2 + (T - 1) * shift samples give T frames.
# framelength: N, N/2 + 3 (odd), 1.  frameshift: 1, N/8 + 1 (odd), N.  DCbin: 1 .. N/2 + 1 (every bin is the DC value).
# Splice 1 / 2 with T = 1, 2, 5: with T <= Splice every neighbour block is the floor.
STFT_CASES = {
    "n64_full_shift9_pow2": case(64, 64, 9, 1, 0.0, 2, 0, 6),
    "n64_len1_shift1_pow1": case(64, 1, 1, 1, 0.92, 1, 0, 4),
    "n64_splice1_T1": case(64, 35, 64, 2, 0.0, 2, 1, 1),
    "n64_splice2_T1": case(64, 64, 9, 1, 0.92, 1, 2, 1),
    "n128_alldc": case(128, 67, 17, 65, 0.0, 2, 0, 3),
    "n128_splice2_T2": case(128, 128, 17, 3, 0.0, 0.7, 2, 2),
    "n256_shiftN_pow07_splice1_T5": case(256, 131, 256, 1, 0.92, 0.7, 1, 5),
    "n512_pow05_splice2_T5": case(512, 512, 65, 3, 0.0, 0.5, 2, 5),
    "n1024_odd_len_shift1_pow1": case(1024, 515, 1, 1, 0.92, 1, 0, 4),
    "n2048_splice1_T2": case(2048, 2048, 257, 2, 0.0, 2, 1, 2),
    "n2048_len1_shiftN_pow05": case(2048, 1, 2048, 1, 0.0, 0.5, 0, 3),
    "n4096_full_shift513_pow2": case(4096, 4096, 513, 5, 0.0, 2, 0, 6),
    "n4096_odd_len_shiftN_pow05": case(4096, 2051, 4096, 1, 0.92, 0.5, 0, 3),
}
ALL_DC = ("n128_alldc",)  # the output does not depend on the samples


def n_samples(p, T=None):
    T = p["T"] if T is None else T
    return p["fftlength"] + 2 + (T - 1) * p["frameshift"]


def signal(L, seed):
    """Seeded noise of the scale of 16-bit audio plus a tone."""
    rs = np.random.RandomState(seed)
    return rs.randn(L) * 1000 + 3000 * np.sin(2 * np.pi * 0.0371 * np.arange(L) + 0.3)


@functools.lru_cache(maxsize=None)
def case_signal(name):
    s = signal(n_samples(STFT_CASES[name]), sorted(STFT_CASES).index(name) + 1)
    s.setflags(write=False)
    return s


def splice_zero_outside(Feat, Splice):
    """src/frame_splice.m:8-23 as out[(S + d) K + f, t] = Feat[f, t + d], zero outside the signal.  With T > Splice this is
    fo.frame_splice to the bit; with T <= Splice the reference's own loop reads a column past the end (MATLAB: index
    exceeds matrix dimensions, the oracle: IndexError), and zero outside the signal is what the C ABI documents."""
    K, T = Feat.shape
    out = np.zeros(((2 * Splice + 1) * K, T))
    for t in range(T):
        for d in range(-Splice, Splice + 1):
            if 0 <= t + d < T:
                out[(Splice + d) * K:(Splice + d + 1) * K, t] = Feat[:, t + d]
    return out


def features(s, p):
    """fo.dft_features with splice_zero_outside: the fp64 reference of every STFT case."""
    S = fo.stft_fft(s, p["framelength"], p["frameshift"], p["fftlength"], p["DCbin"], p["win_STFT"], p["preemph"])
    S = S[:, np.any(S != 0, axis=0)]
    return splice_zero_outside(S, p["Splice"]) ** p["pow"] + p["nonzerofloor"]


@functools.lru_cache(maxsize=None)
def case_reference(name):
    ref = features(case_signal(name), STFT_CASES[name])
    ref.setflags(write=False)
    return ref


def colmax(ref, p):
    """The scale of tests/test_frontend.py: the largest bin of the column (of all its spliced blocks), floored."""
    K = p["fftlength"] // 2 + 1
    cm = ref.reshape(-1, K, ref.shape[1]).max(axis=(0, 1)) if p["Splice"] else ref.max(0)
    return np.maximum(cm, ref.max() * 1e-3)[None, :]


def features_single(s, p):
    """The chain restated in single precision: float32 samples, pre-emphasis and window in float32, np.fft.fft of the
    float32 frame (complex64 in NumPy 2), magnitude, power and floor in float32."""
    f32 = np.float32
    s = np.asarray(s, f32)
    N, sz, shift = p["fftlength"], p["framelength"], p["frameshift"]
    win = p["win_STFT"].astype(f32)
    T = max(0, -(-(len(s) - N - 1) // shift))
    K = N // 2 + 1
    S = np.zeros((K, T), f32)
    for t in range(T):
        x = s[t * shift:t * shift + sz]
        y = x.copy()
        y[1:] -= f32(p["preemph"]) * x[:-1]
        pad = np.zeros(N, f32)
        pad[:sz] = y * win
        m = np.abs(np.fft.fft(pad)[:K]).astype(f32)
        m[:p["DCbin"]] = f32(0.000001)
        S[:, t] = m
    return (splice_zero_outside(S, p["Splice"]).astype(f32) ** f32(p["pow"]) + f32(p["nonzerofloor"])).astype(f32)
