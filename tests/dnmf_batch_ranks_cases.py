"""The problems of the mixed-rank DNMF batch tests (test_dnmf_batch_ranks_api.py, test_gpu_dnmf_batch_ranks.py) and the
conditions they share.  A helper, not a test.

The "edges" batch of dnmf_batch_cases.py (F = 33, the frame counts on every edge of the layouts) with a rank pair per problem:
a rank of one on either side, R_x > R_d, R_x < R_d, and ranks that are no multiples of 4, so that the rows a problem takes from
A_hat start at an offset of its own in a block of its own width.  SETTINGS gives every problem a divergence, a sparsity weight, an
iteration limit and a stop threshold of its own: a limit below the largest that is reached (problem 3), a single iteration
(problem 5), and all four divergences.
"""
import functools

import numpy as np

import dnmf_batch_cases as dc

F, TS, P_EDGES = dc.F, dc.TS, dc.P_EDGES
PAIRS = [(5, 7), (1, 1), (7, 5), (3, 9), (12, 1), (1, 4)]
SETTINGS = [dict(cf="kl", sparsity=0.1, max_iter=20, conv_eps=5e-3),
            dict(cf="ed", sparsity=0.5, max_iter=9, conv_eps=5e-3),
            dict(cf="is", sparsity=0.01, max_iter=20, conv_eps=5e-3),
            dict(cf="kl", sparsity=2.0, max_iter=13, conv_eps=0),
            dict(cf="x", beta=1.5, sparsity=0.1, max_iter=20, conv_eps=5e-3),
            dict(cf="kl", sparsity=0.1, max_iter=1, conv_eps=5e-3)]
# what the oracle gives (test_dnmf_batch_ranks_api.py asserts it): [n1, n2, n3] per problem
TRIPLES_SHARED = [[20, 20, 13], [5, 13, 10], [17, 20, 16], [17, 16, 19], [20, 20, 4], [8, 6, 20]]
TRIPLES_SETTINGS = [[20, 20, 13], [5, 7, 7], [17, 20, 17], [13, 13, 13], [20, 20, 7], [1, 1, 1]]


@functools.lru_cache(maxsize=None)
def problems(pairs=tuple(PAIRS)):
    """[(Y, X, D, B, H0)] per problem, drawn in order from one generator as dc.edges() draws them, each at its own ranks; read only."""
    rng = np.random.default_rng(0)
    out = []
    for T, (rx, rd) in zip(TS, pairs):
        X = rng.gamma(0.5, 1.0, (F, rx)) @ rng.gamma(0.3, 1.0, (rx, T)) + 1e-9
        D = rng.gamma(0.5, 1.0, (F, rd)) @ rng.gamma(0.3, 1.0, (rd, T)) + 1e-9
        Y = X + D
        B = rng.random((F, rx + rd))
        H0 = rng.random((rx + rd, T))
        for m in (Y, X, D, B, H0):
            m.setflags(write=False)
        out.append((Y, X, D, B, H0))
    return out


def p_of(k):
    """The settings dict of problem k alone: the shared ones with SETTINGS[k] in their place."""
    return dict(P_EDGES, **SETTINGS[k])


@functools.lru_cache(maxsize=None)
def oracle(with_settings):
    """[(B_hat, A_hat, [n1, n2, n3])] of the oracle's loop on every problem, once; read only."""
    out = []
    for k, (q, (rx, rd)) in enumerate(zip(problems(), PAIRS)):
        b, a, n = dc.oracle_dnmf(*q, rx, rd, p_of(k) if with_settings else P_EDGES)
        b.setflags(write=False)
        a.setflags(write=False)
        out.append((b, a, n))
    return out
