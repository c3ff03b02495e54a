"""The waveforms of the batched front-end / batched DNMF-from-waveforms tests (test_dnmf_audio_batch_api.py,
test_gpu_dnmf_audio_batch.py) and the conditions they share.  A helper, not a test.

The geometry is the tiny one of the single front-end tests (fftlength 64, framelength 40, frameshift 10, DCbin 1: F = 33, the
32n+1 extra row of the fp32 engine); L = N + 2 + (T - 1) * shift samples give T frames.  The frame counts are one frame, two, a
partial last 32-frame tile, an exact tile, one frame over, and several tiles.  x_k and d_k have DIFFERENT lengths (the shorter
one has exactly L(T_k) samples, so the truncation of run_basis_DNMF.m:5-9 decides T_k), and which of the two is the longer one
alternates.  With conv_eps = 1.5e-3 and max_iter = 20 the first solve of problems 0 and 5 runs to max_iter and the others stop at odd and
at even iterates (test_dnmf_audio_batch_api.py checks it on the oracle).
"""
import functools

import numpy as np

import frontend_envelope as env

N, FL, SHIFT = 64, 40, 10
F, R_X, R_D = 33, 5, 7
TS = [1, 2, 31, 32, 33, 70]
TINY = dict(fs=16000, fftlength=N, framelength=FL, frameshift=SHIFT, DCbin=1,
            win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(FL) / FL)), preemph=0.0, pow=2, nonzerofloor=1e-9, Splice=0,
            F_order=8, R_x=R_X, R_d=R_D)
P_STOP = dict(TINY, cf="kl", sparsity=5, max_iter=20, conv_eps=1.5e-3, cost_check=1, random_seed=1)


def n_samples(T, shift=SHIFT, n=N):
    return n + 2 + (T - 1) * shift


@functools.lru_cache(maxsize=None)
def signals():
    """One signal per frame count of TS and one without a frame, read only."""
    out = [env.signal(n_samples(T), 50 + k) for k, T in enumerate(TS)] + [env.signal(N + 1, 49)]
    for s in out:
        s.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def waves():
    """[(x_k, d_k)] of unequal lengths whose common part has TS[k] frames."""
    out = []
    for k, T in enumerate(TS):
        n = n_samples(T)
        lx, ld = (n, n + 7 + k) if k % 2 else (n + 5 + k, n)
        x, d = env.signal(lx, 100 + k), np.random.RandomState(200 + k).randn(ld) * 700
        x.setflags(write=False)
        d.setflags(write=False)
        out.append((x, d))
    return out


@functools.lru_cache(maxsize=None)
def bases(rows=F):
    """One basis per problem, drawn in order from one generator."""
    rng = np.random.default_rng(3)
    out = [rng.random((rows, R_X + R_D)) + 0.05 for _ in TS]
    for b in out:
        b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def given_h0():
    out = [np.random.RandomState(10 + k).random_sample((R_X + R_D, T)) for k, T in enumerate(TS)]
    for h in out:
        h.setflags(write=False)
    return out
