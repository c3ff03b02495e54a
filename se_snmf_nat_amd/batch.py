"""Batched offline solve: many independent factorizations in shared launches (include/snmf.h: snmf_batch_*).

    results = sparse_nmf_batch(vs, p)       a list of (w, h, objective), one per v in vs -- each what sparse_nmf(v, p) means
    BatchPlan                               the resident handle: set_problem / run / get / describe / close
    sparse_nmf_batch_fp64, BatchPlan64      the same two in the fp64 mode (snmf_batch_create_fp64): every problem's results are
                                            bit for bit those of sparse_nmf(v, p, precision="fp64") run alone
    snmf_mdi_batch, snmf_mdi_Sm_batch       the missing-data solves in the fp64 batch: a list of (v_mdi, h, objective), each bit
                                            for bit snmf_mdi / snmf_mdi_Sm(v, mask, p, precision="fp64") run alone
    BatchPlanMdi64                          their resident handle (snmf_batch_create_mdi_fp64): set_problem takes the mask too
    run_basis_dnmf_batch                    run_basis_dnmf for a list of (Y, X, D) problems: three batches, A_hat resident between
                                            them; a list of (B_hat, A_hat)

The problems share the row count F and the settings `p`; every problem has its own frame count, its own initial factors and
its own stop index.  The rank r is shared too, except in the fp64 batch (sparse_nmf_batch_fp64, BatchPlan64), where every
problem may have a rank of its own (snmf_batch_create_ranks_fp64): a list for r, or init_w arrays of different widths.  The fp32
engine, the missing-data batches and the DNMF batches stay at one rank.  In the fp64 batch the settings may differ per problem
as well (snmf_batch_create_settings_fp64): a list of settings dicts for sparse_nmf_batch_fp64, settings=[...] for BatchPlan64 --
divergence, sparsity weight, max_iter and conv_eps of its own for every problem, so that a sweep over them is one batch;
cost_check, floor_v and the masks stay shared.  All arithmetic happens in libsnmf_hip.so on the GPU;
this module does the reference's defaulting and its own errors (src/sparse_nmf.m:75-164, :260) on the host, before any device call.
Every host rule has one statement, shared by all forms and by train.py: the problem list (_problem_arrays, _row_count), ints per
problem (_ints_per_problem), rank and initial factors of a problem (_rank_and_init_w, _init_h; _batch_inits for the dict forms),
the draws (_batch_draws), settings per problem (_problem_settings, _settings_array), the solve through the handle
(_solve_through_handle).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SnmfError
from .api import _cf_to_beta, _check_precision, _colmajor, _display, _make_params, _mask, _ptr, _solver_scalars, default_context

__all__ = ["sparse_nmf_batch", "BatchPlan", "sparse_nmf_batch_fp64", "BatchPlan64", "snmf_mdi_batch", "snmf_mdi_Sm_batch",
           "BatchPlanMdi64", "run_basis_dnmf_batch"]


def _check_batch_precision(precision):
    if precision != "fp32":
        raise ValueError(f"precision must be 'fp32' for the batched solve (got {precision!r}); "
                         "the fp64 mode has names of its own: sparse_nmf_batch_fp64 and BatchPlan64")


def _batch_sparsity(sparsity, r):
    """src/sparse_nmf.m:150-155 for a batch -> (kind, scalar, r-vector or None); a matrix has no batched form."""
    sp = np.asarray(sparsity, dtype=np.float64)
    if sp.size == 1:
        return 0, float(sp.reshape(-1)[0]), None
    if sp.ndim == 1 or (sp.ndim == 2 and sp.shape[1] == 1):
        if sp.size != r:
            raise SnmfError(3, f"sparsity column has {sp.size} rows, h has {r}")
        return 1, 0.0, np.ascontiguousarray(sp.reshape(-1))
    raise SnmfError(8, "the batched solve takes a scalar or an r-vector sparsity, not an r x n matrix")


def _h_ind_all_or_none(p, r):
    h_ind = _mask(p, "h_update_ind", r)
    n_h = int(h_ind.sum())
    if n_h not in (0, r):
        raise SnmfError(3, f"partial h_update_ind ({n_h} of {r} rows): dimension mismatch in src/sparse_nmf.m:192/197/202")
    return h_ind


def _is_seq(x):
    return isinstance(x, (list, tuple)) or (isinstance(x, np.ndarray) and x.ndim > 0)


def _at_least_1(v, k, name):
    if v < 1:
        raise SnmfError(1, f"{name} of problem {k} is {v} (at least 1)")


def _ints_per_problem(x, n, name):
    """An int per problem (a rank, a dictionary size) given as a sequence -> the list of n ints, none below 1; anything that is
    no sequence (an int, None, a 0-d array) -> None.  Its own errors: a length that is not n (3), an entry below 1 (1)."""
    if not _is_seq(x):
        return None
    xs = [int(v) for v in np.asarray(x).reshape(-1)]
    if len(xs) != n:
        raise SnmfError(3, f"{name} is a list of {len(xs)}, the batch has {n} problems")
    for k, v in enumerate(xs):
        _at_least_1(v, k, name)
    return xs


def _mixed_rank_rules(sparsity, masks):
    """What a batch with differing ranks takes: a scalar sparsity, and masks that are absent, all ones or all zeros (an r-vector
    has no meaning across ranks) -> (scalar, {key: 0 or 1}); SnmfError status 8 otherwise."""
    sp = np.asarray(sparsity, dtype=np.float64)
    if sp.size != 1:
        raise SnmfError(8, "a batch with differing ranks takes a scalar sparsity, not a vector or a matrix")
    on = {}
    for key, m in masks.items():
        on[key] = 1
        if m is not None:
            m = np.asarray(m).reshape(-1) != 0
            if m.size == 0 or (m.any() and not m.all()):
                raise SnmfError(8, f"a batch with differing ranks takes a {key} of all ones or all zeros")
            on[key] = int(m.all())
    return float(sp.reshape(-1)[0]), on


_SETTING_KEYS = ("cf", "beta", "sparsity", "max_iter", "conv_eps")


def _problem_settings(settings, B, shared):
    """Settings per problem (BatchPlan64, the batched training calls): a list of B dicts with keys among cf, beta, sparsity,
    max_iter, conv_eps -> a list of B tuples (beta, sparsity, max_iter, conv_eps); a missing key takes the value of `shared`
    (a dict with those four).  Its own errors, all before the library is loaded: a list of another length (3), an entry that is
    no dict or has an unknown key (1), a sparsity that is not a scalar (8), a max_iter below 0 (1)."""
    if isinstance(settings, dict) or not isinstance(settings, (list, tuple)):
        raise SnmfError(3, f"settings must be a list of {B} dicts, one per problem")
    if len(settings) != B:
        raise SnmfError(3, f"settings is a list of {len(settings)}, the batch has {B} problems")
    out = []
    for k, s in enumerate(settings):
        if not isinstance(s, dict):
            raise SnmfError(1, f"settings of problem {k} must be a dict with keys among {_SETTING_KEYS}")
        unknown = sorted(set(s) - set(_SETTING_KEYS))
        if unknown:
            raise SnmfError(1, f"settings of problem {k} have unknown keys {unknown} (known: {_SETTING_KEYS})")
        if "cf" in s:
            beta = _cf_to_beta(s)  # src/sparse_nmf.m:95-110
        elif "beta" in s:
            beta = float(s["beta"])
        else:
            beta = float(shared["beta"])
        sp = np.asarray(s.get("sparsity", shared["sparsity"]), dtype=np.float64)
        if sp.size != 1:
            raise SnmfError(8, f"settings of problem {k}: a batch with settings per problem takes a scalar sparsity, not a vector or a matrix")
        mi = int(s.get("max_iter", shared["max_iter"]))
        if mi < 0:
            raise SnmfError(1, f"settings of problem {k}: max_iter must be >= 0")
        out.append((beta, float(sp.reshape(-1)[0]), mi, float(s.get("conv_eps", shared["conv_eps"]))))
    return out


def _settings_array(resolved):
    """The tuples of _problem_settings as the C array of snmf_problem_settings."""
    arr = (_lib.SnmfProblemSettings * len(resolved))()
    for a, (beta, sparsity, mi, eps) in zip(arr, resolved):
        a.beta, a.sparsity, a.conv_eps, a.max_iter, a.reserved = beta, sparsity, eps, mi, 0
    return arr


def _objective(div, cost, ni, max_iter, cost_check):
    if cost_check:
        n = ni if ni < max_iter else max_iter  # :279-280 truncate to 1:it on convergence
        return {"div": div[:n].copy(), "cost": cost[:n].copy(), "n_iter": ni}
    return {"div": np.zeros(max_iter), "cost": np.zeros(max_iter), "n_iter": ni}


def _problem_arrays(vs, what="v"):
    """The problems of a batch as a list of arrays, at least one (SnmfError status 1)."""
    vs = [np.asarray(v) for v in vs]
    if not vs:
        raise SnmfError(1, f"the batch is empty: {what}s must hold at least one matrix")
    return vs


def _row_count(vs, what="v", masks=None):
    """The problem-list check: every problem a 2-D matrix with at least one column (status 1) -- and, where the problems have
    masks, a mask of its own shape (3) -- and one row count for all (3) -> that row count."""
    for k, v in enumerate(vs):
        if v.ndim != 2 or v.shape[1] < 1:
            raise SnmfError(1, f"every {what} must be a 2-D matrix with at least one column")
        if masks is not None and masks[k].shape != v.shape:
            raise SnmfError(3, f"the mask of problem {k} is {masks[k].shape}, its {what} is {v.shape}")
    m = vs[0].shape[0]  # src/sparse_nmf.m:71
    for k, v in enumerate(vs):
        if v.shape[0] != m:
            raise SnmfError(3, f"{what} of problem {k} has {v.shape[0]} rows, problem 0 has {m}: a batch shares the row count")
    return m


def _rank_and_init_w(m, r, iw, empty_ok=False):
    """src/sparse_nmf.m:116-131 for one problem: its r (or None) and init_w (or None) -> (rank, init_w as float64 or None).  The
    rank is init_w's width, or r where that is larger (the missing columns are drawn).  empty_ok: an init_w without a column
    counts as one (the engines with one rank take :123-130 as it stands); otherwise it is status 3."""
    if iw is None:
        if r is None:
            raise SnmfError(2, "Number of components or initialization must be given")
        return int(r), None
    iw = np.asarray(iw, dtype=np.float64)
    if iw.ndim != 2 or iw.shape[0] != m or (iw.shape[1] < 1 and not empty_ok):
        raise SnmfError(3, f"init_w is {iw.shape}, v has {m} rows")
    return (int(r) if (r is not None and iw.shape[1] < int(r)) else iw.shape[1]), iw  # :123-130


def _init_h(ih, r, T):
    """src/sparse_nmf.m:133-140 for one problem: its init_h (or None) as float64, r x T (status 3 otherwise)."""
    if ih is None:
        return None
    ih = np.asarray(ih, dtype=np.float64)
    if ih.shape != (r, T):
        raise SnmfError(3, f"init_h is {ih.shape}, expected ({r}, {T})")
    return ih


def _batch_inits(p, vs, m, per_problem=False):
    """src/sparse_nmf.m:116-140 for a batch: the dict forms of r / init_w / init_h are spread into one (r, init_w) per problem,
    each resolved by _rank_and_init_w, then init_h -> (r, init_w per problem or None, init_h list or None).
    per_problem (the fp64 batch): p["r"] may be a list and the init_w arrays may differ in width, and r is the list of the
    problems' ranks.  Otherwise one rank, as an int, and differing ranks or widths are SnmfError status 3."""
    B = len(vs)
    prs = _ints_per_problem(p.get("r", None), B, "r")
    if prs is not None and not per_problem and len(set(prs)) > 1:
        raise SnmfError(3, f"r is {prs}: a batch shares the rank")
    iw = p.get("init_w", None)
    if isinstance(iw, (list, tuple)):
        if len(iw) != B:
            raise SnmfError(3, f"init_w is a list of {len(iw)}, the batch has {B} problems")
        iw = [np.asarray(x, dtype=np.float64) for x in iw]  # (only an absent key means "no init_w": a None entry is no matrix, status 3)
    else:  # one array (or none) for every problem
        iw = [iw if iw is None else np.asarray(iw, dtype=np.float64)] * B
    rs, iws = [], []
    for r, x in zip(prs or [p.get("r", None)] * B, iw):
        r, x = _rank_and_init_w(m, r, x, empty_ok=not per_problem)
        if not per_problem and iws and x is not None and x.shape[1] != iws[0].shape[1]:
            raise SnmfError(3, f"init_w is {x.shape}, problem 0 has {iws[0].shape[1]} columns: a batch shares the rank")
        rs.append(r)
        iws.append(x)
    return (rs if per_problem else rs[0]), iws, _batch_init_h(p, vs, rs)


def _batch_init_h(p, vs, rs):
    """The list form of init_h (src/sparse_nmf.m:133-140): r_k x T_k arrays, or None when it is absent."""
    ih = p.get("init_h", None)
    if ih is None:
        return None
    if isinstance(ih, str) or not isinstance(ih, (list, tuple)) or len(ih) != len(vs):
        raise SnmfError(3, f"init_h must be a list of {len(vs)} arrays (r x T_b each), or absent")
    return [_init_h(np.asarray(x, dtype=np.float64), r, v.shape[1]) for v, x, r in zip(vs, ih, rs)]  # (a None entry: status 3)


def _batch_draws(vs, m, r, iws, ihs, rng, dt):
    """The initial factors of every problem, drawn in list order from one generator (w then h, as one solve draws them, each of
    its own shape) -- the only draw loop of the batched solves.  r: the shared rank, or a list with one per problem; ihs: None,
    or a list in which None stands for a problem without init_h (the list of dicts)."""
    w0s, h0s = [], []
    rs = r if isinstance(r, list) else [r] * len(vs)
    for k, v in enumerate(vs):
        n, r = v.shape[1], rs[k]
        if iws[k] is None:
            w0 = rng.random_sample((m, r))
        elif iws[k].shape[1] < r:
            w0 = np.concatenate([iws[k], rng.random_sample((m, r - iws[k].shape[1]))], axis=1)
        else:
            w0 = iws[k]
        h0 = rng.random_sample((r, n)) if ihs is None or ihs[k] is None else ihs[k]
        w0s.append(np.asfortranarray(w0, dtype=dt))
        h0s.append(np.asfortranarray(h0, dtype=dt))
    return w0s, h0s


def _cost_check(p):
    if "cost_check" not in p:  # src/sparse_nmf.m:260
        raise SnmfError(4, "Reference to non-existent field 'cost_check'.")
    return 1 if p["cost_check"] else 0


def _ptrs(arrs):
    """A list of arrays as the C array of their addresses; None stays None (NULL)."""
    return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs]) if arrs is not None else None


def _ptr_or_null(a):
    return _ptr(a) if a is not None else None


def _lds(arrs):
    """The leading dimensions of a list of column-major arrays (one column: the row count)."""
    return np.array([(a.strides[1] // a.itemsize) if a.shape[1] > 1 else a.shape[0] for a in arrs], np.int64)


def _one_shot_buffers(vs, m, r, max_iter, dt):
    """What a one-shot entry takes beside the problems -> (Ts, W, H, div, cost, n_iter)."""
    nh = max(max_iter, 1)
    return (np.array([v.shape[1] for v in vs], np.int32), [np.empty((m, r), dtype=dt, order="F") for _ in vs], [np.empty((r, v.shape[1]), dtype=dt, order="F") for v in vs],
            [np.zeros(nh) for _ in vs], [np.zeros(nh) for _ in vs], np.zeros(len(vs), np.int32))


def sparse_nmf_batch(vs, p=None, *, ctx=None, dtype=np.float64, rng=None, precision="fp32"):
    """[w, h, objective] = sparse_nmf(v, p) for every v in `vs`, solved together (snmf_sparse_nmf_batch_*).

    vs: a list of F x T_b arrays (one F).  p: the reference's settings, shared; p["r"] is the rank (a list of len(vs) equal
    ranks is the same; differing ranks are SnmfError status 3 here); p["init_w"] is one F x r array (every
    problem starts from it) or a list of len(vs) of them; p["init_h"] is a list of len(vs) arrays r x T_b, or absent (drawn
    per problem as sparse_nmf draws it, from one generator in list order); p["sparsity"] is a scalar or an r-vector;
    p["display"] prints each problem's lines after the solve.  Returns a list of (w, h, objective).
    Every problem stops at its own iteration, with the results of a solve that ran alone; the results of a problem do not
    depend on the batch around it.  `precision` accepts only "fp32" (ValueError otherwise)."""
    _check_batch_precision(precision)
    if isinstance(p, (list, tuple)):
        raise SnmfError(8, "settings per problem need the fp64 batch: sparse_nmf_batch_fp64(vs, [p_0, ...])")
    return _solve_batch(vs, p, ctx, dtype, rng, "fp32")


def sparse_nmf_batch_fp64(vs, p=None, *, ctx=None, rng=None):
    """sparse_nmf_batch in the fp64 mode (snmf_sparse_nmf_batch_fp64): float64 arrays in and out, the same settings, defaulting,
    draws in list order and errors.  Problem k's w, h, div, cost and n_iter are bit for bit those of
    sparse_nmf(vs[k], p_k, precision="fp64") run alone on the same initial factors.  No F or r limit of its own.
    A rank per problem: p["r"] may be a list of len(vs) ranks and the arrays of an init_w list may differ in width; problem k's
    rank then follows src/sparse_nmf.m:116-131 on its own (init_w_k's width, or p["r"][k] when that is larger: the missing
    columns are drawn), init_h[k] is r_k x T_k, and the draws stay in list order, w then h per problem, each of its own shape.
    With differing ranks the sparsity must be a scalar and the masks absent, all ones or all zeros (SnmfError status 8
    otherwise), and the solve goes through the resident handle (snmf_batch_create_ranks_fp64); equal ranks are the call above.
    Settings per problem: p may be a list of len(vs) dicts, one per problem (snmf_batch_create_settings_fp64) -- a sweep over
    divergence, sparsity, max_iter or conv_eps in one batch.  Per problem: cf, beta, sparsity (a scalar; a vector is status 8),
    max_iter, conv_eps, r, init_w, init_h and display (differing ranks under the rules above).  Shared, and equal in every dict
    (status 3 otherwise): cost_check (status 4 where absent), the masks and random_seed.  The draws are the dict call's: one
    generator, list order, w then h.  Problem k is bit for bit sparse_nmf(vs[k], p[k], precision="fp64") alone on the same
    initial factors, and its objective vectors have the single call's length; a list of equal dicts gives the dict call's bits."""
    if isinstance(p, (list, tuple)):
        return _solve_batch_settings(vs, list(p), ctx, rng)
    return _solve_batch(vs, p, ctx, np.float64, rng, "fp64")


def _solve_batch(vs, p, ctx, dtype, rng, mode):
    """The one host side of sparse_nmf_batch and sparse_nmf_batch_fp64: the reference's defaulting, its errors and the batch's
    refusals, the draws, then one call of the C entry of `mode` -- or, for differing ranks, the resident handle."""
    p = dict(p or {})
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise SnmfError(1, "dtype must be float64 or float32")
    vs = _problem_arrays(vs)
    m, B = _row_count(vs), len(vs)
    max_iter = int(p.get("max_iter", 100))  # :79-81
    random_seed = p.get("random_seed", 1)  # :83-85
    conv_eps = float(p.get("conv_eps", 0))  # :91-93
    beta = _cf_to_beta(p)
    if rng is None:  # :112-114
        rng = np.random.RandomState(int(random_seed) if random_seed and random_seed > 0 else None)

    r, iws, ihs = _batch_inits(p, vs, m, per_problem=mode == "fp64")  # :116-131
    if isinstance(r, list) and len(set(r)) == 1:
        r = r[0]
    if isinstance(r, list):  # differing ranks: the remaining checks and the draws, then the resident handle (no one-shot entry)
        scalar, on = _mixed_rank_rules(p.get("sparsity", 0), {k: p.get(k, None) for k in ("w_update_ind", "h_update_ind")})
        cost_check = _cost_check(p)
        w0s, h0s = _batch_draws(vs, m, r, iws, ihs, rng, dt)
        return _solve_through_handle(vs, ctx, m, r, w0s, h0s, [(beta, max_iter, conv_eps)] * B, [p.get("display", 0)] * B,
                                     beta=beta, max_iter=max_iter, conv_eps=conv_eps, cost_check=cost_check, sparsity=scalar,
                                     w_update_ind=bool(on["w_update_ind"]), h_update_ind=bool(on["h_update_ind"]))
    w_ind = _mask(p, "w_update_ind", r)
    h_ind = _h_ind_all_or_none(p, r)
    kind, scalar, sarr = _batch_sparsity(p.get("sparsity", 0), r)
    cost_check = _cost_check(p)

    w0s, h0s = _batch_draws(vs, m, r, iws, ihs, rng, dt)  # the draws, in list order (:116-140)

    sp = _make_params(m, 1, r, beta, max_iter, conv_eps, cost_check, True, kind, scalar, w_ind, h_ind)
    lib = _lib.load()
    ctx = ctx or default_context()
    vv = [_colmajor(v, dt) for v in vs]
    ldv = _lds(vv)
    Ts, W, H, div, cost, n_iter = _one_shot_buffers(vs, m, r, max_iter, dt)
    if mode == "fp64":
        fn = lib.snmf_sparse_nmf_batch_fp64
    else:
        fn = lib.snmf_sparse_nmf_batch_f64 if dt == np.float64 else lib.snmf_sparse_nmf_batch_f32
    _lib.check(fn(ctx._h, C.byref(sp), B, _ptr(Ts), _ptrs(vv), _ptr(ldv), _ptrs(w0s), _ptrs(h0s), _ptr_or_null(sarr),
                  _ptrs(W), _ptrs(H), _ptrs(div), _ptrs(cost), _ptr(n_iter)))
    out = []
    for k in range(B):
        ni = int(n_iter[k])
        if p.get("display", 0) != 0:
            _display(beta, div[k], cost[k], ni, max_iter, cost_check, conv_eps, False)
        out.append((W[k], H[k], _objective(div[k], cost[k], ni, max_iter, cost_check)))
    return out


def _solve_through_handle(vs, ctx, m, rs, w0s, h0s, per, displays, **plan_kw):
    """The fp64 solves that have no one-shot entry (differing ranks, settings per problem), after every check and the draws:
    BatchPlan64(ctx, m, rs, Ts, **plan_kw) -- set every problem, run to the end, get, close -- then the display and the
    objective of every problem from per[k] = its (beta, max_iter, conv_eps) and displays[k] = its p["display"]."""
    dt = np.dtype(np.float64)
    plan = BatchPlan64(ctx, m, rs, [v.shape[1] for v in vs], **plan_kw)
    try:
        for k, v in enumerate(vs):
            plan.set_problem(k, np.asarray(v, dtype=dt), w0s[k], h0s[k])
        plan.run()
        raw = [plan._get(k, dt) for k in range(len(vs))]
    finally:
        plan.close()
    out = []
    for (W, H, div, cost, ni), (beta, mi, eps), display in zip(raw, per, displays):
        div, cost = div[:max(mi, 1)], cost[:max(mi, 1)]  # (the handle's vectors have the largest limit's length)
        if display != 0:
            _display(beta, div, cost, ni, mi, plan.cost_check, eps, False)
        out.append((W, H, _objective(div, cost, ni, mi, plan.cost_check)))
    return out


def _mask_key(m):
    return None if m is None else tuple(bool(x) for x in np.asarray(m).reshape(-1) != 0)


def _solve_batch_settings(vs, ps, ctx, rng):
    """sparse_nmf_batch_fp64 with a list of settings dicts: the reference's defaulting and errors per problem, the batch's
    refusals and the draws, all before the library is loaded; then BatchPlan64 with the settings (and the ranks, where they
    differ) through _solve_through_handle."""
    vs = _problem_arrays(vs)
    B = len(vs)
    if len(ps) != B:
        raise SnmfError(3, f"p is a list of {len(ps)} settings, the batch has {B} problems")
    m = _row_count(vs)
    ps = [dict(q or {}) for q in ps]
    # ---- per problem: the settings (:79-110, :150-155) and the rank with its initial factors (:116-140)
    resolved, rs, iws, ihs = [], [], [], []
    for k, (q, v) in enumerate(zip(ps, vs)):
        sp = np.asarray(q.get("sparsity", 0), dtype=np.float64)
        if sp.size != 1:
            raise SnmfError(8, f"problem {k}: a batch with settings per problem takes a scalar sparsity, not a vector or a matrix")
        mi = int(q.get("max_iter", 100))
        if mi < 0:
            raise SnmfError(1, f"problem {k}: max_iter must be >= 0")
        resolved.append((_cf_to_beta(q), float(sp.reshape(-1)[0]), mi, float(q.get("conv_eps", 0))))
        r, iw = _rank_and_init_w(m, q.get("r", None), q.get("init_w", None))
        _at_least_1(r, k, "r")  # (only a given r can fail: an init_w has a column)
        rs.append(r)
        iws.append(iw)
        ihs.append(_init_h(q.get("init_h", None), r, v.shape[1]))
    # ---- shared: cost_check, the masks, random_seed
    for q in ps:
        _cost_check(q)
    cost_check = _cost_check(ps[0])
    seed = ps[0].get("random_seed", 1)
    mixed = len(set(rs)) > 1
    masks = {}
    for key in ("w_update_ind", "h_update_ind"):
        if mixed:  # the classes of the ranks rules: absent or all ones, all zeros
            cls = [_mixed_rank_rules(0.0, {key: q.get(key, None)})[1][key] for q in ps]
        else:
            cls = [_mask_key(_mask(q, key, rs[0])) for q in ps]
        if any(c != cls[0] for c in cls):
            raise SnmfError(3, f"{key} differs between the problems: a batch shares the masks")
        masks[key] = bool(cls[0]) if mixed else np.array(cls[0], np.uint8)
    for k, q in enumerate(ps):
        if (1 if q["cost_check"] else 0) != cost_check:
            raise SnmfError(3, f"cost_check of problem {k} differs from problem 0: a batch shares it")
        if q.get("random_seed", 1) != seed:
            raise SnmfError(3, f"random_seed of problem {k} differs from problem 0: a batch shares it")
    if not mixed:
        _h_ind_all_or_none(dict(h_update_ind=masks["h_update_ind"]), rs[0])
    if rng is None:  # :112-114
        rng = np.random.RandomState(int(seed) if seed and seed > 0 else None)
    w0s, h0s = _batch_draws(vs, m, rs, iws, ihs, rng, np.dtype(np.float64))  # the dict call's: list order, w then h (:116-140)
    return _solve_through_handle(vs, ctx, m, rs if mixed else rs[0], w0s, h0s, [(b, mi, e) for b, _, mi, e in resolved],
                                 [q.get("display", 0) for q in ps], cost_check=cost_check, w_update_ind=masks["w_update_ind"],
                                 h_update_ind=masks["h_update_ind"],
                                 settings=[dict(beta=b, sparsity=s, max_iter=mi, conv_eps=e) for b, s, mi, e in resolved])


class BatchPlan:
    """snmf_batch: B problems of one (F, r) and one settings struct resident in HBM.  Call order: set_problem for every
    k -> run -> get; run(n) runs n more iterations (None: up to max_iter) and a later run continues."""

    _create = "snmf_batch_create"
    _create_ranks = None  # the entry that takes a rank per problem, where the engine has one
    _rank_status = 3      # what differing ranks are where it has none
    _create_settings = None  # the entry that takes settings per problem, where the engine has one (status 8 where it has none)

    def __init__(self, ctx, F, r, Ts, *, beta=1.0, max_iter=100, conv_eps=0.0, cost_check=True, floor_v=True, sparsity=0.0,
                 w_update_ind=None, h_update_ind=None, precision="fp32", settings=None):
        _check_batch_precision(precision)
        self._init(ctx, F, r, Ts, beta, max_iter, conv_eps, cost_check, floor_v, sparsity, w_update_ind, h_update_ind, settings)

    def _init(self, ctx, F, r, Ts, beta, max_iter, conv_eps, cost_check, floor_v, sparsity, w_update_ind, h_update_ind, settings=None):
        self.Ts = np.ascontiguousarray(np.asarray(Ts, dtype=np.int32).reshape(-1))
        self.B = int(self.Ts.size)
        if self.B == 0:
            raise SnmfError(1, "the batch is empty: Ts must hold at least one frame count")
        self.settings = None  # settings per problem (BatchPlan64): a list of (beta, sparsity, max_iter, conv_eps); None: shared
        if settings is not None:
            if self._create_settings is None:
                raise SnmfError(8, "this batch has one settings struct for all problems (settings per problem: BatchPlan64)")
            self.settings = _problem_settings(settings, self.B, dict(beta=beta, sparsity=sparsity, max_iter=max_iter, conv_eps=conv_eps))
            max_iter = max(s[2] for s in self.settings)  # the handle's: the largest
            sparsity = 0.0  # (every problem has its own)
        masks = dict(w_update_ind=w_update_ind, h_update_ind=h_update_ind)
        self.ranks = None  # a rank per problem (BatchPlan64 with a sequence for r); None: self.r for every problem
        rs = _ints_per_problem(r, self.B, "r")
        if rs is not None:
            r = self._take_ranks(rs, sparsity, masks)
        self.F, self.r, self.max_iter = int(F), int(r), int(max_iter)
        self.cost_check = 1 if cost_check else 0
        # ---- the masks and the sparsity under the rules of the form
        self._sarr = self._rk = self._st = None
        if self.ranks is not None:  # a rank per problem: a scalar, and masks of all ones or all zeros
            kind = 0
            scalar, on = _mixed_rank_rules(sparsity, masks)
            self._w_ind, self._h_ind = (np.full(self.r, on[key], np.uint8) for key in ("w_update_ind", "h_update_ind"))
            self._rk = np.array(self.ranks, np.int32)
        else:
            if self.settings is not None:  # (this form takes a bool for a mask, as the form with ranks does)
                masks = {k: (np.full(self.r, m, np.uint8) if isinstance(m, (bool, np.bool_)) else m) for k, m in masks.items()}
            self._w_ind = _mask(masks, "w_update_ind", self.r)
            self._h_ind = _h_ind_all_or_none(masks, self.r)
            kind, scalar, self._sarr = _batch_sparsity(sparsity, self.r)
        if self.settings is not None:
            beta, scalar, _, conv_eps = self.settings[0]  # (the handle ignores these three fields of its params)
        sp = _make_params(self.F, 1, self.r, beta, self.max_iter, conv_eps, self.cost_check, floor_v, kind, scalar, self._w_ind, self._h_ind)
        # ---- the entry of the form
        if self.settings is not None:
            self._st = _settings_array(self.settings)
            self._open(ctx, self._create_settings, sp, _ptr_or_null(self._rk), self._st)
        elif self.ranks is not None:
            self._open(ctx, self._create_ranks, sp, _ptr(self._rk))
        else:
            self._open(ctx, self._create, sp)
            if self._sarr is not None:
                _lib.check(self._lib.snmf_batch_set_sparsity_f64(self._h, _ptr(self._sarr)))

    def _take_ranks(self, rs, sparsity, masks):
        """r given as a sequence -> the rank the handle is made with.  Where the engine takes a rank per problem and the settings
        allow it, self.ranks is set (and the largest returned); equal ranks are otherwise that rank; differing ones are refused."""
        equal = len(set(rs)) == 1
        if self._create_ranks is None:
            if not equal:
                raise SnmfError(self._rank_status, f"r is {rs}: this batch shares the rank (a rank per problem: BatchPlan64)")
            return rs[0]
        try:
            _mixed_rank_rules(sparsity, masks)
        except SnmfError:
            if not equal:
                raise
            return rs[0]  # equal ranks with an r-vector: the int form
        self.ranks = rs
        return max(rs)

    def _open(self, ctx, entry, sp, *extra):
        """Load the library, take the context, create the handle through `entry` (params, B, Ts, *extra) and register it."""
        self._lib = _lib.load()
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        _lib.check(getattr(self._lib, entry)(self.ctx._h, C.byref(sp), self.B, _ptr(self.Ts), *extra, C.byref(h)))
        self._h = h
        self.ctx._plans.add(self)

    def _index(self, k):
        k = int(k)
        if not 0 <= k < self.B:
            raise SnmfError(1, f"problem index {k} outside [0, {self.B})")
        return k

    def rank(self, k):
        """The rank of problem k."""
        return self.r if self.ranks is None else self.ranks[k]

    def max_iter_of(self, k):
        """The iteration limit of problem k."""
        return self.max_iter if self.settings is None else self.settings[k][2]

    def set_problem(self, k, v, w0, h0):
        self._set_problem(k, v, w0, h0)

    def _set_problem(self, k, v, w0, h0, mask=None):
        """set_problem of every engine; mask: the missing-data batch's (its one entry takes doubles)."""
        k = self._index(k)
        v = np.asarray(v)
        if mask is not None:
            mask = np.asarray(mask, dtype=np.float64)
        dt = np.dtype(np.float32) if (mask is None and v.dtype == np.float32) else np.dtype(np.float64)
        T, r = int(self.Ts[k]), self.rank(k)
        if v.shape != (self.F, T):
            raise SnmfError(3, f"v is {v.shape}, problem {k} is ({self.F}, {T})")
        if mask is not None and mask.shape != v.shape:
            raise SnmfError(3, f"the mask is {mask.shape}, v is {v.shape}")
        w0, h0 = np.asarray(w0), np.asarray(h0)
        if w0.shape != (self.F, r):
            raise SnmfError(3, f"init_w is {w0.shape}, problem {k} is ({self.F}, {r})" if self.ranks is not None
                            else f"init_w is {w0.shape}, v has {self.F} rows")
        if h0.shape != (r, T):
            raise SnmfError(3, f"init_h is {h0.shape}, expected ({r}, {T})")
        vv = _colmajor(v, dt)
        w0 = np.asfortranarray(w0, dtype=dt)
        h0 = np.asfortranarray(h0, dtype=dt)
        ld = lambda a: a.strides[1] // dt.itemsize if T > 1 else self.F  # noqa: E731
        if mask is None:
            entry, extra = ("snmf_batch_set_problem_f64" if dt == np.float64 else "snmf_batch_set_problem_f32"), ()
        else:
            mm = _colmajor(mask, dt)
            entry, extra = "snmf_batch_set_problem_mdi_f64", (_ptr(mm), ld(mm))
        _lib.check(getattr(self._lib, entry)(self._h, k, _ptr(vv), ld(vv), *extra, _ptr(w0), _ptr(h0)))
        self.ctx.sync()  # (the host arrays may go out of scope)

    def run(self, n_iters=None):
        _lib.check(self._lib.snmf_batch_run(self._h, 0 if n_iters is None else int(n_iters)))

    def get(self, k, dtype=np.float64):
        W, H, div, cost, ni = self._get(k, np.dtype(dtype))
        mi = self.max_iter_of(k)  # (the objective vectors of the single solve with the problem's own limit)
        return W, H, _objective(div[:max(mi, 1)], cost[:max(mi, 1)], ni, mi, self.cost_check)

    def _get(self, k, dt):
        k = self._index(k)
        W = np.empty((self.F, self.rank(k)), dtype=dt, order="F")
        H = np.empty((self.rank(k), int(self.Ts[k])), dtype=dt, order="F")
        nh = max(self.max_iter, 1)
        div, cost = np.zeros(nh), np.zeros(nh)
        ni = C.c_int32()
        fn = self._lib.snmf_batch_get_f64 if dt == np.float64 else self._lib.snmf_batch_get_f32
        _lib.check(fn(self._h, k, _ptr(W), _ptr(H), _ptr(div), _ptr(cost), C.byref(ni)))
        return W, H, div, cost, ni.value

    def describe(self):
        buf = C.create_string_buffer(1024)
        _lib.check(self._lib.snmf_batch_describe(self._h, buf, 1024))
        return buf.value.decode()

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):  # a destroyed context has already destroyed its plans
                self._lib.snmf_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchPlan64(BatchPlan):
    """BatchPlan in the fp64 mode (snmf_batch_create_fp64): the same methods and call order; every problem's results are bit
    for bit those of sparse_nmf(..., precision="fp64") on it alone.  float32 arrays given to set_problem are widened,
    get(dtype=np.float32) rounds the fp64 results; describe() gives the tables, the grids, the launches per iteration and the bytes.
    r may be a sequence of len(Ts): a rank per problem (snmf_batch_create_ranks_fp64).  set_problem(k, ...) then takes init_w
    F x r[k] and init_h r[k] x Ts[k], get(k) returns those shapes, .ranks holds the list (.r its largest entry) and describe()
    names the ranks.  Such a batch takes a scalar sparsity and masks that are absent, a bool, all ones or all zeros; with
    differing ranks anything else is SnmfError status 8, while a sequence of equal ranks with a vector sparsity or a partial
    mask is the int form.  An int for r is snmf_batch_create_fp64, as before.
    settings: None, or a list of len(Ts) dicts with keys among cf, beta, sparsity, max_iter, conv_eps -- settings per problem
    (snmf_batch_create_settings_fp64); a missing key takes the plan's shared value, an unknown key is SnmfError status 1, a list
    of another length status 3, a vector sparsity status 8.  .settings then holds (beta, sparsity, max_iter, conv_eps) per
    problem, .max_iter the largest limit, max_iter_of(k) problem k's own; get(k) returns the objective vectors of the single
    solve with problem k's settings, and describe() names the modes and the limits.  cost_check, floor_v and the masks stay
    shared.  BatchPlan and BatchPlanMdi64 refuse settings (status 8)."""

    _create = "snmf_batch_create_fp64"
    _create_ranks = "snmf_batch_create_ranks_fp64"
    _create_settings = "snmf_batch_create_settings_fp64"

    def __init__(self, ctx, F, r, Ts, *, beta=1.0, max_iter=100, conv_eps=0.0, cost_check=True, floor_v=True, sparsity=0.0,
                 w_update_ind=None, h_update_ind=None, settings=None):
        self._init(ctx, F, r, Ts, beta, max_iter, conv_eps, cost_check, floor_v, sparsity, w_update_ind, h_update_ind, settings)


def snmf_mdi_batch(vs, Dms, p=None, *, ctx=None, rng=None, info=None):
    """[v_MDI, h, objective] = snmf_mdi(v, Dm, p) for every (v, Dm) of the two lists, solved together in the fp64 batch
    (snmf_mdi_batch_fp64).  Dm: 1 = observed, 0 = missing.  p: snmf_mdi's settings, shared (sparsity_mdi a scalar or an r-vector,
    conv_eps_mdi, cost_check, ...), with init_w / init_h in the list forms of sparse_nmf_batch and the draws in list order.
    Returns a list of (v_mdi, h, objective); info, when given, receives info["w"], the list of each problem's dictionary.
    Problem k's results are bit for bit those of snmf_mdi(vs[k], Dms[k], p_k, precision="fp64") run alone."""
    return _mdi_batch(vs, [np.asarray(d) != 0 for d in Dms], p, ctx, rng, info)


def snmf_mdi_Sm_batch(vs, Sms, p=None, *, ctx=None, rng=None, info=None):
    """snmf_mdi_batch for soft masks in [0, 1]: problem k is snmf_mdi_Sm(vs[k], Sms[k], p_k, precision="fp64") bit for bit."""
    return _mdi_batch(vs, Sms, p, ctx, rng, info)


def _mdi_batch(vs, masks, p, ctx, rng, info):
    """The host side of the two entries above: api._mdi's defaulting and errors (src/snmf_mdi.m:83-93, :260) and the batch's
    refusals, all before the library is loaded; then one call of snmf_mdi_batch_fp64."""
    p = dict(p or {})
    dt = np.dtype(np.float64)
    masks = [np.asarray(mk, dtype=np.float64) for mk in masks]
    vs = _problem_arrays(vs)
    B = len(vs)
    if len(masks) != B:
        raise SnmfError(3, f"{len(masks)} masks for {B} problems")
    m = _row_count(vs, masks=masks)
    max_iter = int(p.get("max_iter", 100))  # src/snmf_mdi.m:83-85
    seed = p.get("random_seed", 1)
    if "sparsity" not in p:  # :87-89 (the default is installed only when p.sparsity is ABSENT)
        p.setdefault("sparsity_mdi", 0)
    if "conv_eps" not in p:  # :91-93
        p.setdefault("conv_eps_mdi", 0)
    for fld in ("sparsity_mdi", "conv_eps_mdi", "cost_check"):
        if fld not in p:
            raise KeyError(f"Reference to non-existent field '{fld}'.")
    beta = _cf_to_beta(p)
    if rng is None:
        rng = np.random.RandomState(int(seed) if seed and seed > 0 else None)
    r, iws, ihs = _batch_inits(p, vs, m)
    w_ind = _mask(p, "w_update_ind", r)
    h_ind = _h_ind_all_or_none(p, r)
    kind, scalar, sarr = _batch_sparsity(p["sparsity_mdi"], r)
    cost_check = 1 if p["cost_check"] else 0
    conv_eps = float(p["conv_eps_mdi"])
    w0s, h0s = _batch_draws(vs, m, r, iws, ihs, rng, dt)

    sp = _make_params(m, 1, r, beta, max_iter, conv_eps, cost_check, True, kind, scalar, w_ind, h_ind)
    lib = _lib.load()
    ctx = ctx or default_context()
    vv = [_colmajor(v, dt) for v in vs]
    mm = [_colmajor(mk, dt) for mk in masks]
    ldv, ldm = _lds(vv), _lds(mm)
    Vm = [np.empty(v.shape, dtype=dt, order="F") for v in vs]
    Ts, W, H, div, cost, n_iter = _one_shot_buffers(vs, m, r, max_iter, dt)
    _lib.check(lib.snmf_mdi_batch_fp64(ctx._h, C.byref(sp), B, _ptr(Ts), _ptrs(vv), _ptr(ldv), _ptrs(mm), _ptr(ldm), _ptrs(w0s), _ptrs(h0s),
                                       _ptr_or_null(sarr), _ptrs(Vm), None, _ptrs(W), _ptrs(H), _ptrs(div), _ptrs(cost), _ptr(n_iter)))
    if info is not None:
        info["w"] = W
    out = []
    for k in range(B):
        ni = int(n_iter[k])
        n = ni if ni < max_iter else max_iter  # src/snmf_mdi.m:286-287: truncation on convergence only
        out.append((Vm[k], H[k], {"div": div[k][:n].copy(), "cost": cost[k][:n].copy(), "n_iter": ni}))
    return out


class BatchPlanMdi64(BatchPlan64):
    """BatchPlan64 for missing-data solves (snmf_batch_create_mdi_fp64): set_problem takes the problem's mask (1 = observed, soft
    masks in [0, 1]) and get_v_mdi(k) reads the gain-matched final imputation of problem k from the state the last run left,
    without writing it: run(n) + get_v_mdi + run() gives the bytes of one run().  Every problem's results are bit for bit those
    of snmf_mdi / snmf_mdi_Sm(..., precision="fp64") on it alone.  floor_v has no meaning here (the masked start floors)."""

    _create = "snmf_batch_create_mdi_fp64"
    _create_ranks = None  # a missing-data batch shares the rank
    _rank_status = 8
    _create_settings = None  # and the settings

    def set_problem(self, k, v, mask, w0, h0):
        self._set_problem(k, v, w0, h0, mask=mask)

    def get_v_mdi(self, k):
        k = self._index(k)
        out = np.empty((self.F, int(self.Ts[k])), dtype=np.float64, order="F")
        _lib.check(self._lib.snmf_batch_get_v_mdi_f64(self._h, k, _ptr(out), self.F))
        return out


def _dnmf_rank_pairs(R_x, R_d, n, settings, precision):
    """R_x, R_d and settings of the batched DNMF calls -> None for two scalars without settings (the uniform entries), else the
    two lists of n ranks (a scalar beside a sequence counts for every problem).  A rank pair or settings per problem are the fp64
    engine's: SnmfError status 8 in fp32.  Its own errors: a length that is not n (3), a rank below 1 (1)."""
    if not _is_seq(R_x) and not _is_seq(R_d) and settings is None:
        return None
    if precision != "fp64":
        raise SnmfError(8, "a rank pair or settings per problem need precision='fp64': the fp32 batch engine has one rank and one "
                           "settings struct for all problems")
    return [_ints_per_problem(R if _is_seq(R) else [int(R)] * n, n, name) for name, R in (("R_x", R_x), ("R_d", R_d))]


def _dnmf_rank_inputs(B, h0, rs, F, Ts, modes, p):
    """B and h0 of a DNMF batch with ranks rs[k] = R_x[k] + R_d[k] (the uniform call: one rank n times) -> (Bs, H0s) as float64:
    B a list of F x rs[k] arrays, or one array when every pair is the same; h0 one of the strings in `modes`, or a list of
    rs[k] x T_k arrays.  "host": rand(rs[k], T_k) per problem, in list order, from one RandomState(p["random_seed"]) -- what
    sparse_nmf draws for solve 1 of each problem (init_w is given, so h is its first draw); another string: H0s is None.
    All errors are SnmfError status 3."""
    n = len(Ts)
    if isinstance(B, (list, tuple)):
        if len(B) != n:
            raise SnmfError(3, f"B is a list of {len(B)}, the batch has {n} problems")
        Bs = [np.asfortranarray(b, dtype=np.float64) for b in B]
    else:
        if len(set(rs)) > 1:
            raise SnmfError(3, f"one B for problems of different ranks {rs}: B must be a list of F x (R_x[k] + R_d[k]) arrays")
        Bs = [np.asfortranarray(B, dtype=np.float64)] * n
    for k, b in enumerate(Bs):
        if b.shape != (F, rs[k]):
            raise SnmfError(3, f"B of problem {k} is {b.shape}, expected ({F}, {rs[k]})")
    what = f"h0 must be {', '.join(repr(m) for m in modes)} or a list of {n} arrays ((R_x[k] + R_d[k]) x T_k each)"
    if isinstance(h0, str):
        if h0 not in modes:
            raise SnmfError(3, what)
        if h0 != "host":
            return Bs, None
        seed = int(p.get("random_seed", 1))
        rng = np.random.RandomState(seed if seed > 0 else None)
        return Bs, [np.asfortranarray(rng.random_sample((r, T))) for r, T in zip(rs, Ts)]
    if not isinstance(h0, (list, tuple)) or len(h0) != n:
        raise SnmfError(3, what)
    H0s = [np.asfortranarray(h, dtype=np.float64) for h in h0]
    for k, (h, r, T) in enumerate(zip(H0s, rs, Ts)):
        if h.shape != (r, T):
            raise SnmfError(3, f"init_h of problem {k} is {h.shape}, expected ({r}, {T})")
    return Bs, H0s


def _dnmf_rank_params(p, settings, n, F, r_max):
    """(snmf_params, the C array of settings or None) of a DNMF batch with ranks: p's own errors (_solver_scalars), then the
    settings per problem resolved by _problem_settings with p's values as the shared ones; params.max_iter is the largest limit."""
    beta, max_iter, conv_eps, cost_check, lam = _solver_scalars(p)
    sarr = None
    if settings is not None:
        st = _problem_settings(settings, n, dict(beta=beta, sparsity=lam, max_iter=max_iter, conv_eps=conv_eps))
        max_iter = max(s[2] for s in st)
        sarr = _settings_array(st)
    return _make_params(F, 1, r_max, beta, max_iter, conv_eps, cost_check, True, 0, lam, None, None), sarr


def run_basis_dnmf_batch(Ys, Xs, Ds, B, R_x, R_d, p, *, ctx=None, dtype=np.float64, h0="host", precision="fp32", info=None, settings=None):
    """(B_hat, A_hat) = run_basis_dnmf(Y, X, D, B, R_x, R_d, p) for every problem of the three lists, solved together
    (snmf_run_basis_dnmf_batch_*): the mixtures, the clean and the noise features are three batches, and A_hat stays on the
    device between them.  Ys, Xs, Ds: lists of F x T_k arrays (one F; X_k and D_k of Y_k's shape).  B: one F x (R_x + R_d)
    array for every problem, or a list of them.  h0: "host" = rand(r, T_k) of solve 1 drawn per problem, in list order, from one
    RandomState(p["random_seed"]); or a list of r x T_k arrays.  p: the settings, shared; a scalar sparsity.
    precision="fp32": the fp32 batch engine (F <= 513, R_x + R_d <= 200), bit for bit three chained sparse_nmf_batch calls.
    precision="fp64" (dtype float64): problem k's results are bit for bit run_basis_dnmf(..., precision="fp64", h0=H0_k) alone.
    Every problem stops each of its three solves at its own iteration; info["n_iter"] receives a list of [n1, n2, n3].
    A rank pair per problem (precision="fp64" only, snmf_run_basis_dnmf_batch_ranks_fp64): R_x and R_d may each be a sequence of
    len(Ys) ints (a scalar beside a sequence counts for every problem).  B is then a list of F x (R_x[k] + R_d[k]) arrays (one
    array only when every pair is the same), h0 a list of (R_x[k] + R_d[k]) x T_k arrays or "host", which draws
    rand(R_x[k] + R_d[k], T_k) per problem in list order from the one RandomState: with equal ranks the draw above.
    settings: one dict per problem with keys among cf, beta, sparsity, max_iter, conv_eps (the rules of
    sparse_nmf_batch_fp64(vs, [p_0, ...]); a missing key takes p's value); problem k's settings hold in all three of its solves.
    Problem k stays bit for bit run_basis_dnmf(Y_k, X_k, D_k, B_k, R_x[k], R_d[k], p_k, precision="fp64", h0=H0_k) alone.  A
    sequence or settings with precision="fp32" is SnmfError status 8.
    Returns a list of (B_hat, A_hat)."""
    _check_precision(precision)
    p = dict(p)
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise SnmfError(1, "dtype must be float64 or float32")
    Xs, Ds = ([np.asarray(v) for v in vs] for vs in (Xs, Ds))
    Ys = _problem_arrays(Ys, "Y")
    n = len(Ys)
    if len(Xs) != n or len(Ds) != n:
        raise SnmfError(1, f"{n} mixtures, {len(Xs)} clean and {len(Ds)} noise feature sets: one of each per problem")
    pairs = _dnmf_rank_pairs(R_x, R_d, n, settings, precision)  # None: two scalars, the uniform entries
    Rxs, Rds = pairs or ([int(R_x)] * n, [int(R_d)] * n)
    F = _row_count(Ys, "Y")
    for k, (y, x, d) in enumerate(zip(Ys, Xs, Ds)):
        if x.shape != y.shape or d.shape != y.shape:
            raise SnmfError(3, f"problem {k}: Y, X and D must have one size (got {y.shape}, {x.shape}, {d.shape})")
    rs = [a + b for a, b in zip(Rxs, Rds)]
    Ts = [y.shape[1] for y in Ys]
    Bs, H0s = _dnmf_rank_inputs(B, h0, rs, F, Ts, ("host",), p)
    sp, sarr = _dnmf_rank_params(p, settings, n, F, max(rs))
    if precision == "fp64" and dt != np.dtype(np.float64):
        raise SnmfError(1, "precision='fp64' needs dtype=np.float64 (the fp64 DNMF batch takes and returns doubles)")

    lib = _lib.load()
    ctx = ctx or default_context()
    yy, xx, dd, bb, hh = ([np.asfortranarray(a, dtype=dt) for a in arrs] for arrs in (Ys, Xs, Ds, Bs, H0s))  # (fp32: float32 where asked)
    B_hat = [np.empty((F, r), dtype=dt, order="F") for r in rs]
    A_hat = [np.empty((r, T), dtype=dt, order="F") for r, T in zip(rs, Ts)]
    n_iter = np.zeros(3 * n, np.int32)
    Tv, rx, rd = np.array(Ts, np.int32), np.array(Rxs, np.int32), np.array(Rds, np.int32)
    if pairs is not None:
        entry, head = "snmf_run_basis_dnmf_batch_ranks_fp64", (_ptr(rx), _ptr(rd), sarr, n)
    else:
        entry = "snmf_run_basis_dnmf_batch_" + ("fp64" if precision == "fp64" else "f64" if dt == np.float64 else "f32")
        head = (Rxs[0], Rds[0], n)
    _lib.check(getattr(lib, entry)(ctx._h, C.byref(sp), *head, _ptr(Tv), _ptrs(yy), _ptrs(xx), _ptrs(dd), _ptrs(bb), _ptrs(hh), _ptrs(B_hat),
                                   _ptrs(A_hat), _ptr(n_iter)))
    if info is not None:
        info["n_iter"] = [[int(v) for v in n_iter[3 * k:3 * k + 3]] for k in range(n)]
    return list(zip(B_hat, A_hat))
