"""The cases of the mixed-rank tests (test_batch_ranks_api.py, test_gpu_batch_ranks_f64.py, test_gpu_train_batch_ranks.py): an fp64
batch whose problems each have a rank of their own.  A helper, not a test.

Training: the signals and settings of tests/train_batch_cases.py (F = 33, T = 6, 7, 31, 32, 33, 70) with one dictionary size per
problem, RANKS = 6, 3, 1, 6, 5, 2 -- the shared R of those tests, a rank of one, and T_0 = n_ex_0 (every column an exemplar).
With cluster_buff = 2 the sizes are RANKS_CB2 = 3, 3, 1, 3, 2, 1, so that 2 * R_k <= T_k.  The exemplar columns of a problem are
a seeded draw of its own n_ex_k columns; H0 is the single call's host draw, RandomState(random_seed).random_sample((n_ex_k, T_k)).
"""
import functools

import numpy as np

import frontend_envelope as env
import train_batch_cases as tc

RANKS = [6, 3, 1, 6, 5, 2]
RANKS_CB2 = [3, 3, 1, 3, 2, 1]
assert len(RANKS) == len(RANKS_CB2) == len(tc.TS)
assert all(r <= T for r, T in zip(RANKS, tc.TS)) and all(2 * r <= T for r, T in zip(RANKS_CB2, tc.TS))


@functools.lru_cache(maxsize=None)
def sample_idx(n_exs=tuple(RANKS)):
    """The 1-based exemplar columns of every problem: n_exs[k] of its T_k columns, seeded."""
    out = [np.random.RandomState(40 + k).choice(T, size=n, replace=False) + 1 for k, (T, n) in enumerate(zip(tc.TS, n_exs))]
    for ix in out:
        ix.setflags(write=False)
    return out


def oracle_stop_indices(p=tc.P_STOP, ranks=tuple(RANKS)):
    """[n_dft, n_mel] per problem on the oracle, from the exemplar columns above and the H0 the GPU tests use (tc.host_h0):
    tc.oracle_stop_indices with a rank per problem."""
    from oracle import frontend_oracle as fo
    from oracle.sparse_nmf_oracle import sparse_nmf
    out = []
    for s, ix, T, r in zip(tc.signals(), sample_idx(tuple(ranks)), tc.TS, ranks):
        TF_mag = env.features(s, p)
        TF_Mel = fo.mel_features(TF_mag, p)
        q = {k: p[k] for k in ("cf", "beta", "sparsity", "max_iter", "conv_eps", "cost_check", "random_seed") if k in p}
        H0 = tc.host_h0(T, p, r)
        out.append([int(sparse_nmf(V, dict(q, init_w=V[:, ix - 1], init_h=H0))[2]["n_iter"]) for V in (TF_mag, TF_Mel)])
    return out
