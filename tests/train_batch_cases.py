"""The signals of the batched basis-training tests (test_train_batch_api.py, test_gpu_train_batch.py) and the conditions they
share.  A helper, not a test.

The geometry is the tiny one of tests/dnmf_audio_batch_cases.py (fftlength 64, framelength 40, frameshift 10, DCbin 1: F = 33, the
32n+1 extra row of the fp32 engine; F_order = 8), R = 6 and cluster_buff = 1.  The frame counts are T = n_ex (every column is an
exemplar), one more, a partial 32-frame tile, an exact tile, one frame over, and several tiles.  The exemplar columns of a
problem are a seeded draw without replacement.  With conv_eps = 5e-4 and max_iter = 20 the DFT solves of two problems run to max_iter
on the fp64 oracle and the others stop at odd and at even iterations (test_train_batch_api.py asserts it).
"""
import functools

import numpy as np

import frontend_envelope as env
from dnmf_audio_batch_cases import F, N, TINY as _TINY, n_samples

R = 6
TS = [6, 7, 31, 32, 33, 70]
TINY = {k: v for k, v in _TINY.items() if k not in ("R_x", "R_d")}
P_STOP = dict(TINY, cf="kl", sparsity=5, max_iter=20, conv_eps=5e-4, cost_check=1, random_seed=1, cluster_buff=1, train_Exemplar=0)
F_MEL = TINY["F_order"]
assert F == 33 and N == 64


@functools.lru_cache(maxsize=None)
def signals():
    """One training signal per frame count of TS, read only."""
    out = [env.signal(n_samples(T), 300 + k) for k, T in enumerate(TS)]
    for s in out:
        s.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sample_idx(n_ex=R):
    """The 1-based exemplar columns of every problem: n_ex of its T_k columns, seeded (problem 0 with n_ex = R: all of them)."""
    out = [np.random.RandomState(40 + k).choice(T, size=n_ex, replace=False) + 1 for k, T in enumerate(TS)]
    for ix in out:
        ix.setflags(write=False)
    return out


def host_h0(T, p=P_STOP, n_ex=R):
    """The rand(r, n) the single call draws for both of its solves (the RandomState stand-in of src/sparse_nmf.m:112-114, :133-134)."""
    return np.asfortranarray(np.random.RandomState(p["random_seed"]).random_sample((n_ex, T)))


def oracle_stop_indices(p=P_STOP):
    """[n_dft, n_mel] per problem: the logic of oracle.frontend_oracle.run_basis_train_signal on the oracle's features, restated
    for the iteration counts, which it does not return."""
    from oracle import frontend_oracle as fo
    from oracle.sparse_nmf_oracle import sparse_nmf
    out = []
    for s, ix in zip(signals(), sample_idx()):
        TF_mag = env.features(s, p)
        if p.get("domain_DD", 0):
            TF_mag = fo.tf_dd(TF_mag, p)
        TF_Mel = fo.mel_features(TF_mag, p)
        q = {k: p[k] for k in ("cf", "beta", "sparsity", "max_iter", "conv_eps", "cost_check", "random_seed") if k in p}
        n2 = []
        for V in (TF_mag, TF_Mel):
            n2.append(int(sparse_nmf(V, dict(q, init_w=V[:, ix - 1]))[2]["n_iter"]))
        out.append(n2)
    return out


def stops_are_spread(n_dft, max_iter):
    """One solve runs to max_iter and the others stop on their own, at no fewer than two different iterations."""
    return max(n_dft) == max_iter and len({n for n in n_dft if n < max_iter}) >= 2
