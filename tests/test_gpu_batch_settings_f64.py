"""GPU tests of the fp64 batch with settings per problem (include/snmf.h: snmf_batch_create_settings_fp64;
se_snmf_nat_amd/batch.py: BatchPlan64(settings=...), sparse_nmf_batch_fp64 with a list of settings dicts).

THE CONTRACT is a bit equality: problem k of a batch whose problems have settings p_0, p_1, ... gives W, H, div, cost and n_iter of
sparse_nmf(v_k, p_k, precision="fp64") run alone on the same initial factors -- .tobytes() equality throughout, no tolerance --
whatever the divergences, sparsity weights, thresholds, iteration limits, ranks and sizes of the problems around it.  The cases
are those of tests/batch_settings_cases.py; the single solves of a case are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import batch_settings_cases as sc

pytestmark = pytest.mark.gpu

KL5, ED = dict(cf="kl", sparsity=5), dict(cf="ed", sparsity=0.5)
SMALL = ((100, 45, 300), (13, 1, 24))  # the first three problems of the sweep case
CASES = {
    # name: (Ts, ranks, settings per problem, the factor that is not updated)
    "sweep": (sc.TS, sc.RANKS, sc.sweep_settings(), ""),
    "sweep_r8": (sc.TS, (8,) * 6, sc.sweep_settings(), ""),
    "no_cost_check": (sc.TS, sc.RANKS, sc.sweep_settings(max_iter=sc.MAX_ITER_NO_CC, cost_check=0), ""),
    "h_only": SMALL + ([dict(KL5, max_iter=12, conv_eps=1e-2, cost_check=1), dict(ED, max_iter=9, cost_check=1), dict(KL5, sparsity=1, max_iter=12, cost_check=1)], "w"),
    "w_only": SMALL + ([dict(ED, max_iter=12, cost_check=1), dict(KL5, max_iter=9, cost_check=1), dict(ED, sparsity=2, max_iter=7, conv_eps=1e-2, cost_check=1)], "h"),
    # split W products (T > 2048) of a Euclidean and of a KL problem: the non-KL product tables beside KL row-sum chunks
    "split_T": ((2049, 100, 4500), (3, 13, 1), [dict(ED, max_iter=6, cost_check=1), dict(KL5, max_iter=4, cost_check=1), dict(KL5, sparsity=0.5, max_iter=6, cost_check=1)], ""),
    # a limit of zero beside others: the scaled initial factors, n_iter = 0
    "zero_limit": SMALL + ([dict(KL5, max_iter=5, cost_check=1), dict(ED, max_iter=0, cost_check=1), dict(KL5, max_iter=3, cost_check=1)], ""),
    # run(3) passes the own limit of problem 1
    "continuation": SMALL + ([dict(KL5, max_iter=12, cost_check=1), dict(ED, max_iter=2, cost_check=1), dict(cf="is", sparsity=0.1, max_iter=9, conv_eps=3e-2, cost_check=1)], ""),
}
_cache = {}


def _ps(name, k, r):
    """The settings dict of problem k of a case for a solve of rank r (the masks as arrays of that length)."""
    Ts, ranks, st, off = CASES[name]
    q = dict(st[k])
    for f in off:
        q[f + "_update_ind"] = np.zeros(r, bool)
    return q


def _case(ctx, name):
    """-> (problems, ranks, the single fp64 solves), computed once and read only."""
    if name not in _cache:
        from se_snmf_nat_amd import sparse_nmf
        Ts, ranks, st, off = CASES[name]
        probs = sc.problems(ranks=tuple(ranks), Ts=tuple(Ts))
        single = [sparse_nmf(V, dict(_ps(name, k, r), init_w=W0, init_h=H0), ctx=ctx, precision="fp64")
                  for k, ((V, W0, H0), r) in enumerate(zip(probs, ranks))]
        _cache[name] = (probs, ranks, single)
    return _cache[name]


def _batch(ctx, name, order=None):
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    probs, ranks, _ = _case(ctx, name)
    order = list(range(len(probs))) if order is None else order
    ps = [dict(_ps(name, k, ranks[k]), init_w=probs[k][1], init_h=probs[k][2]) for k in order]
    return sparse_nmf_batch_fp64([probs[k][0] for k in order], ps, ctx=ctx)


def _same_bits(a, b, what=""):
    (w, h, o), (w2, h2, o2) = a, b
    assert o["n_iter"] == o2["n_iter"], (what, o["n_iter"], o2["n_iter"])
    assert w.dtype == w2.dtype == np.float64 and h.dtype == h2.dtype == np.float64
    assert w.shape == w2.shape and h.shape == h2.shape, (what, w.shape, w2.shape, h.shape, h2.shape)
    assert w.tobytes() == w2.tobytes(), (what, "W", float(np.max(np.abs(w - w2))))
    assert h.tobytes() == h2.tobytes(), (what, "H", float(np.max(np.abs(h - h2))))
    assert o["div"].shape == o2["div"].shape and o["div"].tobytes() == o2["div"].tobytes(), (what, "div", o["div"].shape, o2["div"].shape)
    assert o["cost"].shape == o2["cost"].shape and o["cost"].tobytes() == o2["cost"].tobytes(), (what, "cost")


# ---- 1. the contract, case by case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n != "continuation"])
def test_every_problem_is_the_single_fp64_solve_with_its_own_settings(gpu_ctx, name):
    probs, ranks, single = _case(gpu_ctx, name)
    res = _batch(gpu_ctx, name)
    assert len(res) == len(probs)
    n = [o["n_iter"] for _, _, o in res]
    print(name, "n_iter", n, "single", [o["n_iter"] for _, _, o in single])
    for k, (x, s, r) in enumerate(zip(res, single, ranks)):
        assert x[0].shape == (sc.F, r) and np.isfinite(x[0]).all() and np.isfinite(x[1]).all()
        _same_bits(x, s, f"{name}[{k}]")
    limits = [q["max_iter"] for q in CASES[name][2]]
    if name == "sweep":  # what tests/test_batch_settings_api.py asserts on the oracle holds on the device
        assert n[3] == 20 and n[5] == 12                                     # an own max_iter below the largest, reached first
        assert all(a < mi for a, mi in zip(n[:3] + n[4:5], limits[:3] + limits[4:5]))   # the others stop by their test
        assert len(set(n)) >= 4, n
    if name == "no_cost_check":
        assert n == list(sc.MAX_ITER_NO_CC)
        for (_, _, o), mi in zip(res, sc.MAX_ITER_NO_CC):
            assert o["cost"].shape == (mi,) and o["div"].shape == (mi,) and not o["cost"].any() and not o["div"].any()
    if name in ("split_T", "zero_limit"):  # (no threshold: every problem ends at its own limit)
        assert n == limits


def test_continuation_passes_an_own_limit(gpu_ctx):
    """run(3) + run(0) gives the bits of run(0), with a problem whose max_iter = 2 falls inside the first run."""
    from se_snmf_nat_amd import BatchPlan64
    probs, ranks, single = _case(gpu_ctx, "continuation")
    Ts, _, st, _ = CASES["continuation"]
    keys = ("cf", "beta", "sparsity", "max_iter", "conv_eps")
    bp = BatchPlan64(gpu_ctx, sc.F, list(ranks), Ts, settings=[{k: q[k] for k in keys if k in q} for q in st])
    d = bp.describe()
    print(d)
    assert "settings: modes=3 max_iter min=2 max=12" in d and "ranks: min=1 max=24" in d
    assert bp.max_iter == 12 and [bp.max_iter_of(k) for k in range(3)] == [12, 2, 9]
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run(3)
    part = [bp.get(k) for k in range(3)]
    assert [o["n_iter"] for _, _, o in part] == [3, 2, 3]
    assert part[0][2]["cost"].tobytes() == single[0][2]["cost"][:3].tobytes()
    _same_bits(part[1], single[1], "the problem of max_iter 2 after run(3)")
    bp.run()
    for k in range(3):
        _same_bits(bp.get(k), single[k], f"run(3) + run()[{k}]")
    # a set_problem after a run starts a new batch on the same handle, with the same settings
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run()
    for k in range(3):
        _same_bits(bp.get(k), single[k], f"reuse[{k}]")
    bp.close()


# ---- 2. company, order, equal settings --------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_order_or_on_the_company(gpu_ctx):
    _, _, single = _case(gpu_ctx, "sweep")
    order = [3, 0, 5, 2, 4, 1]
    for x, k in zip(_batch(gpu_ctx, "sweep", order), order):
        _same_bits(x, single[k], f"permuted[{k}]")
    for sub in ([1, 3], [5], [4, 2, 0]):  # subsets: one mode less, one problem alone, the split problem in front
        for x, k in zip(_batch(gpu_ctx, "sweep", sub), sub):
            _same_bits(x, single[k], f"subset {sub}[{k}]")


def test_equal_settings_are_the_dict_call_and_the_plan_without_settings(gpu_ctx):
    from se_snmf_nat_amd import BatchPlan64, sparse_nmf_batch_fp64
    probs = sc.problems(ranks=(8,) * 5, Ts=(1, 31, 33, 100, 7))
    for q in (dict(cf="kl", sparsity=5, max_iter=31, conv_eps=1e-3, cost_check=1), dict(cf="ed", sparsity=0.5, max_iter=9, cost_check=1)):
        vs, iw, ih = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
        a = sparse_nmf_batch_fp64(vs, dict(q, init_w=iw, init_h=ih), ctx=gpu_ctx)
        b = sparse_nmf_batch_fp64(vs, [dict(q, init_w=w, init_h=h) for w, h in zip(iw, ih)], ctx=gpu_ctx)
        keys = {k: v for k, v in q.items() if k != "cost_check"}
        beta = {"kl": 1.0, "ed": 2.0}[q["cf"]]
        plans = [BatchPlan64(gpu_ctx, sc.F, 8, [v.shape[1] for v in vs], beta=beta, max_iter=q["max_iter"], conv_eps=q.get("conv_eps", 0.0),
                             sparsity=q["sparsity"]),
                 BatchPlan64(gpu_ctx, sc.F, 8, [v.shape[1] for v in vs], settings=[keys] * 5)]
        assert "settings:" not in plans[0].describe() and "settings: modes=1" in plans[1].describe()
        assert plans[0].describe().split(" | ")[:5] == plans[1].describe().split(" | ")[:5]  # the same tables, grids and launches
        got = []
        for bp in plans:
            for k, p in enumerate(probs):
                bp.set_problem(k, *p)
            bp.run()
            got.append([bp.get(k) for k in range(5)])
            bp.close()
        for k in range(5):
            _same_bits(b[k], a[k], f"{q['cf']} list of equal dicts[{k}]")
            _same_bits(got[0][k], a[k], f"{q['cf']} plan without settings[{k}]")
            _same_bits(got[1][k], a[k], f"{q['cf']} plan with equal settings[{k}]")
        if q["cf"] == "kl":
            assert len({o["n_iter"] for _, _, o in a}) >= 3


# ---- 3. refusals through ctypes ---------------------------------------------------------------------------------------------------
def test_c_refusals_come_with_their_status_and_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd._lib import SnmfProblemSettings
    from se_snmf_nat_amd.api import _make_params
    _, _, single = _case(gpu_ctx, "continuation")
    T = np.array(SMALL[0], np.int32)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731

    def create(mi=(12, 2, 9), p_mi=None, kind=0, ranks=SMALL[1], reserved=0, null_s=False, beta=(1.0, 2.0, 0.0), keep=False):
        s = (SnmfProblemSettings * 3)()
        for a, m, b in zip(s, mi, beta):
            a.beta, a.sparsity, a.conv_eps, a.max_iter, a.reserved = b, 0.5, 0.0, m, reserved
        rk = None if ranks is None else np.array(ranks, np.int32)
        # (beta = NaN, sparsity and conv_eps of p are ignored: the settings stand in their place)
        q = _make_params(sc.F, 1, 24 if ranks is None else max(ranks), float("nan"), max(mi) if p_mi is None else p_mi, -1.0, 1, True, kind, -3.0, None, None)
        h = C.c_void_p()
        st = lib.snmf_batch_create_settings_fp64(gpu_ctx._h, C.byref(q), 3, vp(T), vp(rk), None if null_s else s, C.byref(h))
        if st == 0 and not keep:
            lib.snmf_batch_destroy(h)
        elif st != 0:
            assert not h.value
        return (st, h) if keep else st

    assert create() == 0
    assert create(ranks=None) == 0                      # NULL r: p->r for all
    assert create(p_mi=13) == 3 and b"largest max_iter" in lib.snmf_last_error()   # p->max_iter is the largest limit
    assert create(p_mi=9) == 3
    assert create(null_s=True) == 1
    assert create(reserved=1) == 1 and b"reserved" in lib.snmf_last_error()
    assert create(mi=(12, -1, 9), p_mi=12) == 1 and b"problem 1" in lib.snmf_last_error()
    assert create(beta=(1.0, float("nan"), 0.0)) == 1 and b"problem 1" in lib.snmf_last_error()
    assert create(kind=1) == 8 and b"scalar sparsity" in lib.snmf_last_error()
    assert create(ranks=(13, 1, 23)) == 0 and create(ranks=(13, 0, 24)) == 1   # the rules of the ranks handle
    # there is no missing-data form: a settings handle is a plain one to the masked entries
    st, h = create(keep=True)
    assert st == 0
    one = np.ones((sc.F, 100), order="F")
    assert lib.snmf_batch_set_problem_mdi_f64(h, 0, vp(one), sc.F, vp(one), sc.F, vp(one), vp(one)) == 7
    assert lib.snmf_batch_get_v_mdi_f64(h, 0, vp(one), sc.F) == 7
    lib.snmf_batch_destroy(h)
    for k, (x, s) in enumerate(zip(_batch(gpu_ctx, "continuation"), single)):  # a valid batch afterwards still gives the earlier bits
        _same_bits(x, s, f"after the refusals[{k}]")
