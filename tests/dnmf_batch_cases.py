"""The problems of the batched DNMF tests (test_dnmf_batch_api.py, test_gpu_dnmf_batch.py) and the conditions they share.

"edges": the smallest batch at which the hand-off of A_hat between the phases can still go wrong.  F = 33 is the 32n+1 extra
row; R_x = 5 and R_d = 7 are unequal and no multiples of 4; the frame counts are one frame, a partial last 32-frame tile, an
exact tile, one frame over, and several tiles.  With conv_eps = 5e-3 one problem's first solve runs to max_iter and the others
stop at odd and at even iterates, so the stop iterate lies in either H buffer of the fp32 engine.
"""
import numpy as np

from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf

F, R_X, R_D = 33, 5, 7
TS = [1, 31, 32, 33, 70, 100]
P_EDGES = dict(cf="kl", sparsity=0.1, max_iter=20, conv_eps=5e-3, cost_check=1)


def edges():
    """[(Y, X, D, B, H0)] per problem, drawn in order from one generator."""
    rng = np.random.default_rng(0)
    r = R_X + R_D
    out = []
    for T in TS:
        X = rng.gamma(0.5, 1.0, (F, R_X)) @ rng.gamma(0.3, 1.0, (R_X, T)) + 1e-9
        D = rng.gamma(0.5, 1.0, (F, R_D)) @ rng.gamma(0.3, 1.0, (R_D, T)) + 1e-9
        Y = X + D
        B = rng.random((F, r))
        H0 = rng.random((r, T))
        out.append((Y, X, D, B, H0))
    return out


def oracle_dnmf(Y, X, D, B, H0, R_x, R_d, p):
    """The three calls of oracle.run_basis_dnmf_solves with solve 1 started from H0 -> (B_hat, A_hat, [n1, n2, n3])."""
    p = dict(p)
    p.update(w_update_ind=np.zeros(R_x + R_d, bool), h_update_ind=np.ones(R_x + R_d, bool), init_w=B, init_h=H0)
    _, A_hat, o1 = oracle_nmf(Y, p)
    p.update(w_update_ind=np.ones(R_x, bool), h_update_ind=np.zeros(R_x, bool), init_w=B[:, :R_x], init_h=A_hat[:R_x])
    Bx, _, o2 = oracle_nmf(X, p)
    p.update(w_update_ind=np.ones(R_d, bool), h_update_ind=np.zeros(R_d, bool), init_w=B[:, R_x:], init_h=A_hat[R_x:])
    Bd, _, o3 = oracle_nmf(D, p)
    return np.concatenate([Bx, Bd], axis=1), A_hat, [int(o["n_iter"]) for o in (o1, o2, o3)]


def covers_both_buffers(n1, max_iter):
    """The solve-1 counts hold max_iter, a smaller even value and a smaller odd value."""
    n1 = [int(v) for v in n1]
    return max_iter in n1 and any(v < max_iter and v % 2 == 0 for v in n1) and any(v < max_iter and v % 2 == 1 for v in n1)
