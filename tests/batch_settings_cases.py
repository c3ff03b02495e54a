"""The cases of the settings-per-problem tests (test_batch_settings_api.py, test_gpu_batch_settings_f64.py,
test_gpu_train_batch_settings.py): an fp64 batch whose problems each have a divergence, a sparsity weight, a stop threshold and an
iteration limit of their own.  A helper, not a test.

The sweep case: six problems at F = 37 with frame counts and ranks of their own, four divergences (kl twice, ed, is, beta = 0.5 and
1.5), six sparsity weights, four thresholds and three iteration limits.  T = 2049 splits the W products (kS64ChunkK = 2048) of one
problem only.  On the fp64 oracle with max_iter = 40 for all, the problems stop at 4, 7, 26, 24, 17 and 16: problems 3 and 5 reach
their own max_iter (20, 12) first and the others stop by their test at four different iterations (test_batch_settings_api.py
asserts the conditions).
"""
import functools

import numpy as np

from oracle.sparse_nmf_oracle import synth_problem

F = 37
TS = (100, 45, 300, 60, 2049, 33)
RANKS = (13, 1, 24, 5, 3, 8)
MODES = (dict(cf="kl", sparsity=5), dict(cf="ed", sparsity=0.5), dict(cf="is", sparsity=0.1), dict(cf="beta", beta=0.5, sparsity=0.3),
         dict(cf="kl", sparsity=0.5), dict(cf="beta", beta=1.5, sparsity=1.0))
CONV_EPS = (1e-2, 3e-3, 3e-2, 3e-3, 1e-3, 1e-2)
MAX_ITER = (40, 40, 40, 20, 40, 12)
MAX_ITER_NO_CC = (12, 7, 10, 5, 1, 3)
assert len(TS) == len(RANKS) == len(MODES) == len(CONV_EPS) == len(MAX_ITER) == len(MAX_ITER_NO_CC) == 6


def sweep_settings(max_iter=MAX_ITER, cost_check=1):
    """The settings dict of every problem of the sweep case (without r and the initial factors)."""
    return [dict(m, conv_eps=e, max_iter=mi, cost_check=cost_check) for m, e, mi in zip(MODES, CONV_EPS, max_iter)]


@functools.lru_cache(maxsize=None)
def problems(ranks=RANKS, Ts=TS, F=F):
    """(V, W0, H0) per problem, read only."""
    out = [synth_problem(F, T, r, seed_data=10 * b, seed_init=10 * b + 1, r_true=max(1, min(r, 16) // 2)) for b, (T, r) in enumerate(zip(Ts, ranks))]
    for q in out:
        for a in q:
            a.setflags(write=False)
    return out


def oracle_stop_indices(max_iter=40):
    """n_iter of every problem of the sweep case on the fp64 oracle, with one max_iter for all."""
    from oracle.sparse_nmf_oracle import sparse_nmf
    out = []
    for (V, W0, H0), q in zip(problems(), sweep_settings(max_iter=(max_iter,) * len(TS))):
        out.append(int(sparse_nmf(V, dict(q, init_w=np.array(W0), init_h=np.array(H0)))[2]["n_iter"]))
    return out
