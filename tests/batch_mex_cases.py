"""What the tests of integration/snmf_batch_mex.cpp share (test_batch_mex_api.py, test_gpu_batch_mex.py): the packing of
per-problem matrices into the one double array the shim takes, its inverse, and the settings matrix.  A helper, not a test.

A packed array holds the matrices' column-major elements, one problem after the other; equal row counts make it the
matrices side by side."""
import numpy as np

NAME = "snmf_batch_mex"
COMMANDS = ("solve", "dnmf", "dnmf_audio", "train", "assemble", "signals_info", "signals_get", "train_signals", "signals_destroy")


def pack(arrs):
    """A list of matrices (or vectors) -> one column of their column-major elements."""
    return np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, order="F") for a in arrs])


def side(arrs):
    """Matrices of one row count side by side: the packed array as a matrix."""
    return np.asfortranarray(np.concatenate([np.asarray(a, dtype=np.float64) for a in arrs], axis=1))


def unpack(a, shapes):
    """The inverse: a packed array (any shape) -> the list of matrices of `shapes`, each a copy."""
    flat = np.asarray(a).reshape(-1, order="F")
    assert flat.size == sum(m * n for m, n in shapes), (flat.size, shapes)
    out, at = [], 0
    for m, n in shapes:
        out.append(flat[at:at + m * n].reshape((m, n), order="F").copy(order="F"))
        at += m * n
    return out


def col(x):
    """A count vector as the shim takes it: n x 1 doubles."""
    return np.asarray(x, dtype=np.float64).reshape(-1, 1)


def settings_matrix(resolved):
    """(beta, sparsity, max_iter, conv_eps) per problem, the order of se_snmf_nat_amd.batch._problem_settings -> the shim's
    n x 4 matrix [beta sparsity conv_eps max_iter]."""
    return np.array([[b, s, e, mi] for b, s, mi, e in resolved], dtype=np.float64)


def short(a):
    """One element short."""
    return np.asarray(a, dtype=np.float64).reshape(-1, order="F")[:-1].copy()


def long(a):
    """One element long."""
    return np.append(np.asarray(a, dtype=np.float64).reshape(-1, order="F"), 0.5)


def swap(args, i, v):
    """The argument tuple with argument i replaced."""
    return tuple(args[:i]) + (v,) + tuple(args[i + 1:])


def without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}
