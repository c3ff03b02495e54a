"""GPU tests of the mixed-rank fp64 batch (include/snmf.h: snmf_batch_create_ranks_fp64; se_snmf_nat_amd/batch.py: BatchPlan64 with
a sequence for r, sparse_nmf_batch_fp64 with a list for p["r"] or init_w arrays of different widths).

THE CONTRACT is a bit equality: problem k of a batch whose problems have ranks r_0, r_1, ... gives W (F x r_k), H (r_k x T_k), div,
cost and n_iter of sparse_nmf(v_k, p_k, precision="fp64") run alone on the same initial factors -- .tobytes() equality throughout,
no tolerance.  The shapes are the smallest that put a tile edge, a split of a contraction or a row-sum chunk edge at a different
place in every problem; the single solves of a case are computed once and shared.

`tiny` is the geometry of the batched training tests (tests/batch_ranks_cases.py): the DFT features of its six signals, their
exemplar columns as init_w and the host H0 draw, so that its stop indices are those tests/test_batch_ranks_api.py asserts on the
oracle."""
import ctypes as C

import numpy as np
import pytest

import batch_ranks_cases as rc
import frontend_envelope as env
import train_batch_cases as tc
from oracle.sparse_nmf_oracle import synth_problem

pytestmark = pytest.mark.gpu

KL = dict(cf="kl", sparsity=5, cost_check=1)
TINY_PS = dict(KL, conv_eps=5e-4, max_iter=20)
MASKED = (37, (100, 45, 300), (13, 1, 24))
CASES = {
    # the 64 x 64 GEMM tile edges fall in r: below, at and above one tile, and a rank of one
    "tile_edges_r": (65, (17, 64, 65, 130, 16, 1), (1, 63, 64, 65, 16, 8), dict(KL, max_iter=20)),
    # kS64ChunkK = 2048: only the middle problem's W * H is split
    "split_r": (5, (3, 9, 4), (2048, 2049, 1), dict(KL, max_iter=4)),
    # split W products (T > 2048) and several 256-frame row-sum chunks, at different ranks
    "split_T_kl": (37, (2049, 100, 4500), (3, 13, 1), dict(KL, max_iter=6)),
    "split_T_ed": (37, (2049, 100, 4500), (3, 13, 1), dict(cf="ed", sparsity=0.5, cost_check=1, max_iter=6)),
    "is": MASKED + (dict(cf="is", sparsity=0.1, cost_check=1, max_iter=12),),
    "b05": MASKED + (dict(cf="beta", beta=0.5, sparsity=0.3, cost_check=1, max_iter=10),),
    # uniform masks: ("w" / "h": that factor is not updated)
    "w_only": MASKED + (dict(KL, max_iter=12, off="h"),),
    "h_only": MASKED + (dict(KL, max_iter=12, off="w"),),
    "neither": MASKED + (dict(KL, max_iter=12, conv_eps=1e-3, off="wh"),),
    "w_only_ed": MASKED + (dict(cf="ed", sparsity=0.5, cost_check=1, max_iter=12, off="h"),),
    "no_cost_check": MASKED + (dict(cf="kl", sparsity=5, cost_check=0, conv_eps=1e-2, max_iter=12),),
}
_cache = {}


def _tiny_problems():
    out = []
    for s, ix, T, r in zip(tc.signals(), rc.sample_idx(), tc.TS, rc.RANKS):
        V = np.asfortranarray(env.features(s, tc.P_STOP))
        assert V.shape == (tc.F, T)
        out.append((V, np.asfortranarray(V[:, ix - 1]), tc.host_h0(T, tc.P_STOP, r)))
    return out


def _problems(name):
    if name == "tiny":
        return _tiny_problems(), tuple(rc.RANKS), TINY_PS
    F, Ts, ranks, ps = CASES[name]
    probs = [synth_problem(F, T, r, seed_data=10 * b, seed_init=10 * b + 1, r_true=max(1, min(r, 16) // 2)) for b, (T, r) in enumerate(zip(Ts, ranks))]
    return probs, ranks, ps


def _masks(ps, r):
    """The settings of a case for a solve of rank r (None: for the mixed batch, whose masks are all ones or all zeros of any length)."""
    q = {k: v for k, v in ps.items() if k != "off"}
    n = 1 if r is None else r
    for f in ps.get("off", ""):
        q[f + "_update_ind"] = np.zeros(n, bool)
    return q


def _case(ctx, name):
    """-> (problems, ranks, settings, the single fp64 solves), computed once and read only."""
    if name not in _cache:
        from se_snmf_nat_amd import sparse_nmf
        probs, ranks, ps = _problems(name)
        single = [sparse_nmf(V, dict(_masks(ps, r), init_w=W0, init_h=H0), ctx=ctx, precision="fp64") for (V, W0, H0), r in zip(probs, ranks)]
        for q in probs:
            for a in q:
                a.setflags(write=False)
        _cache[name] = (probs, ranks, ps, single)
    return _cache[name]


def _batch(ctx, probs, ps, **kw):
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    return sparse_nmf_batch_fp64([q[0] for q in probs], dict(_masks(ps, None), init_w=[q[1] for q in probs], init_h=[q[2] for q in probs], **kw),
                                 ctx=ctx)


def _same_bits(a, b, what=""):
    (w, h, o), (w2, h2, o2) = a, b
    assert o["n_iter"] == o2["n_iter"], (what, o["n_iter"], o2["n_iter"])
    assert w.dtype == w2.dtype == np.float64 and h.dtype == h2.dtype == np.float64
    assert w.shape == w2.shape and h.shape == h2.shape, (what, w.shape, w2.shape, h.shape, h2.shape)
    assert w.tobytes() == w2.tobytes(), (what, "W", float(np.max(np.abs(w - w2))))
    assert h.tobytes() == h2.tobytes(), (what, "H", float(np.max(np.abs(h - h2))))
    assert o["div"].shape == o2["div"].shape and o["div"].tobytes() == o2["div"].tobytes(), (what, "div")
    assert o["cost"].shape == o2["cost"].shape and o["cost"].tobytes() == o2["cost"].tobytes(), (what, "cost")


# ---- 1. the contract, case by case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny"] + list(CASES))
def test_every_problem_is_the_single_fp64_solve_at_its_own_rank(gpu_ctx, name):
    probs, ranks, ps, single = _case(gpu_ctx, name)
    res = _batch(gpu_ctx, probs, ps)
    assert len(res) == len(probs)
    print(name, "n_iter", [o["n_iter"] for _, _, o in res])
    for k, (x, s, q, r) in enumerate(zip(res, single, probs, ranks)):
        assert x[0].shape == (q[0].shape[0], r) and x[1].shape == (r, q[0].shape[1])
        assert np.isfinite(x[0]).all() and np.isfinite(x[1]).all()
        _same_bits(x, s, f"{name}[{k}] r = {r}")
    if name == "neither":  # nothing moves: the test of :272-284 fires at the second objective
        assert [o["n_iter"] for _, _, o in res] == [2, 2, 2]
    if name == "no_cost_check":
        for _, _, o in res:
            assert o["n_iter"] == 12 and not o["cost"].any() and not o["div"].any() and o["cost"].shape == (12,)
    if name == "w_only":  # (H is the scaled initial H; W moved)
        assert res[0][0].tobytes() != np.asfortranarray(probs[0][1] / np.sqrt((probs[0][1] ** 2).sum(0))).tobytes()


def test_the_problems_of_tiny_stop_at_their_own_iterations(gpu_ctx):
    probs, ranks, ps, single = _case(gpu_ctx, "tiny")
    n = [o["n_iter"] for _, _, o in _batch(gpu_ctx, probs, ps)]
    print("tiny n_iter", n)
    assert n == [o["n_iter"] for _, _, o in single]
    assert tc.stops_are_spread(n, ps["max_iter"]), n


def test_the_r_list_and_narrow_init_w_forms(gpu_ctx):
    """p["r"] as a list with no init_w, and init_w narrower than r[k]: the draws are those of single solves that share the generator,
    in list order, w then h."""
    from se_snmf_nat_amd import sparse_nmf, sparse_nmf_batch_fp64
    probs, ranks, ps, _ = _case(gpu_ctx, "tiny")
    vs = [q[0] for q in probs[:3]]
    res = sparse_nmf_batch_fp64(vs, dict(ps, r=[4, 2, 5], init_w=[probs[0][1][:, :2], probs[1][1][:, :3], probs[2][1]]), ctx=gpu_ctx,
                                rng=np.random.RandomState(11))
    g = np.random.RandomState(11)
    for k, (v, r, w) in enumerate(zip(vs, (4, 3, 5), (probs[0][1][:, :2], probs[1][1][:, :3], probs[2][1]))):
        one = sparse_nmf(v, dict(ps, r=(4, 2, 5)[k], init_w=w), ctx=gpu_ctx, precision="fp64", rng=g)
        assert res[k][0].shape == (tc.F, r)
        _same_bits(res[k], one, f"drawn[{k}]")


# ---- 2. uniform lists, company, order ---------------------------------------------------------------------------------------------
def _plan(ctx, F, ranks, probs, ps, **kw):
    from se_snmf_nat_amd import BatchPlan64
    return BatchPlan64(ctx, F, ranks, [q[0].shape[1] for q in probs], beta=1.0, max_iter=ps["max_iter"], conv_eps=ps.get("conv_eps", 0.0),
                       sparsity=ps["sparsity"], **kw)


def _run_plan(bp, probs):
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run()
    return [bp.get(k) for k in range(len(probs))]


def test_a_uniform_rank_list_gives_the_bits_of_the_int_form(gpu_ctx):
    probs = [synth_problem(65, T, 8, seed_data=10 * b, seed_init=10 * b + 1, r_true=4) for b, T in enumerate((1, 31, 33, 100, 7))]
    ps = dict(KL, max_iter=31, conv_eps=1e-3)
    a = _plan(gpu_ctx, 65, 8, probs, ps)
    b = _plan(gpu_ctx, 65, [8] * 5, probs, ps)
    assert a.ranks is None and b.ranks == [8] * 5 and "ranks:" not in a.describe() and "ranks: min=8 max=8 sum=40" in b.describe()
    ra, rb = _run_plan(a, probs), _run_plan(b, probs)
    a.close()
    b.close()
    assert len({o["n_iter"] for _, _, o in ra}) >= 3
    for k, (x, y) in enumerate(zip(ra, rb)):
        _same_bits(y, x, f"uniform list[{k}]")


def test_bits_do_not_depend_on_the_order_or_on_the_neighbours_ranks(gpu_ctx):
    probs, ranks, ps, single = _case(gpu_ctx, "tiny")
    for k, (x, s) in enumerate(zip(_batch(gpu_ctx, probs[::-1], ps)[::-1], single)):  # the list reversed
        _same_bits(x, s, f"reversed[{k}]")
    order = [3, 0, 5, 2, 4, 1]
    for x, k in zip(_batch(gpu_ctx, [probs[k] for k in order], ps), order):
        _same_bits(x, single[k], f"permuted[{k}]")
    # problem 4 (T = 33, r = 5) between neighbours of other ranks and frame counts
    for i, (ra, rb) in enumerate(((1, 70), (64, 2), (5, 5))):
        a = synth_problem(tc.F, 9 + i, ra, seed_data=70 + i, seed_init=71 + i, r_true=2)
        b = synth_problem(tc.F, 300 - 100 * i, rb, seed_data=80 + i, seed_init=81 + i, r_true=2)
        _same_bits(_batch(gpu_ctx, [a, probs[4], b], ps)[1], single[4], f"neighbours of ranks {ra}, {rb}")
    _same_bits(_batch(gpu_ctx, [probs[4]], ps)[0], single[4], "alone")
    # a split problem behind direct ones
    sp, _, sps, ssingle = _case(gpu_ctx, "split_T_kl")
    _same_bits(_batch(gpu_ctx, [sp[1], sp[2]], sps)[1], ssingle[2], "T = 4500, r = 1 behind T = 100, r = 13")


# ---- 3. the handle ----------------------------------------------------------------------------------------------------------------
def test_continuation_reuse_and_describe(gpu_ctx):
    probs, ranks, ps, single = _case(gpu_ctx, "tiny")
    bp = _plan(gpu_ctx, tc.F, list(ranks), probs, ps)
    d = bp.describe()
    print(d)
    assert "k_b64_gemm" in d and "ranks: min=1 max=6 sum=23" in d and f"h_elems={sum(r * T for r, T in zip(ranks, tc.TS))}" in d
    assert bp.ranks == list(ranks) and bp.r == 6 and bp.rank(2) == 1
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run(3)
    part = bp.get(0)
    assert part[2]["n_iter"] == 3 and part[2]["cost"].tobytes() == single[0][2]["cost"][:3].tobytes()
    assert bp.get(2)[2]["n_iter"] == 3  # (the rank-one problem has stopped by now, at its own iteration)
    bp.run()
    for k in range(len(probs)):
        _same_bits(bp.get(k), single[k], f"run(3) + run()[{k}]")
    # a set_problem after a run starts a new batch: other data in the same slots, against a fresh plan
    from se_snmf_nat_amd import SnmfError
    other = [synth_problem(tc.F, T, r, seed_data=500 + k, seed_init=600 + k, r_true=2) for k, (T, r) in enumerate(zip(tc.TS, ranks))]
    with pytest.raises(SnmfError) as e:  # problem 1 is 3 wide, not 6
        bp.set_problem(1, other[1][0], other[0][1], other[1][2])
    assert e.value.status == 3
    reused = _run_plan(bp, other)
    bp.close()
    fresh = _plan(gpu_ctx, tc.F, list(ranks), other, ps)
    for k, y in enumerate(_run_plan(fresh, other)):
        _same_bits(reused[k], y, f"reuse[{k}]")
    fresh.close()
    assert reused[0][0].tobytes() != single[0][0].tobytes()


def test_f32_transfers_widen_on_the_way_in_and_round_on_the_way_out(gpu_ctx):
    probs, ranks, ps, _ = _case(gpu_ctx, "tiny")
    p32 = [tuple(np.asarray(a, np.float32) for a in q) for q in probs]
    widened = [tuple(a.astype(np.float64) for a in q) for q in p32]
    a = _plan(gpu_ctx, tc.F, list(ranks), probs, ps)
    b = _plan(gpu_ctx, tc.F, list(ranks), probs, ps)
    ra, rb = _run_plan(a, p32), _run_plan(b, widened)
    for k in range(len(probs)):
        _same_bits(ra[k], rb[k], f"f32 in[{k}]")
        w32, h32, o32 = a.get(k, dtype=np.float32)
        assert w32.dtype == np.float32 and h32.dtype == np.float32 and w32.shape == (tc.F, ranks[k]) and h32.shape == (ranks[k], tc.TS[k])
        assert w32.tobytes() == ra[k][0].astype(np.float32).tobytes() and h32.tobytes() == ra[k][1].astype(np.float32).tobytes()
        assert o32["n_iter"] == ra[k][2]["n_iter"] and o32["cost"].tobytes() == ra[k][2]["cost"].tobytes()
    a.close()
    b.close()


# ---- 4. refusals through ctypes ---------------------------------------------------------------------------------------------------
def test_c_refusals_come_with_their_status_and_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd.api import _make_params
    probs, ranks, ps, single = _case(gpu_ctx, "tiny")
    T = np.array(tc.TS, np.int32)
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731

    def create(r=ranks, p_r=None, kind=0, w_ind=None, h_ind=None, null_r=False, n=len(tc.TS)):
        rk = np.array(r, np.int32)
        q = _make_params(tc.F, 1, max(r) if p_r is None else p_r, 1.0, 5, 0.0, 1, True, kind, 0.1, w_ind, h_ind)
        h = C.c_void_p()
        st = lib.snmf_batch_create_ranks_fp64(gpu_ctx._h, C.byref(q), n, vp(T), None if null_r else vp(rk), C.byref(h))
        if st == 0:
            lib.snmf_batch_destroy(h)
        else:
            assert not h.value
        return st

    on, off = np.ones(6, np.uint8), np.zeros(6, np.uint8)
    part = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    assert create() == 0
    assert create(null_r=True) == 1
    assert create(r=(6, 3, 0, 6, 5, 2)) == 1 and create(r=(6, 3, -1, 6, 5, 2)) == 1
    assert create(n=0) == 1
    assert create(kind=1) == 8 and b"scalar sparsity" in lib.snmf_last_error()
    assert create(kind=2) == 8
    assert create(w_ind=part) == 8 and b"w_update_ind" in lib.snmf_last_error()
    assert create(h_ind=part) == 8 and b"h_update_ind" in lib.snmf_last_error()
    assert create(w_ind=off, h_ind=on) == 0 and create(w_ind=on, h_ind=off) == 0 and create(w_ind=off, h_ind=off) == 0
    assert create(p_r=7) == 3 and create(p_r=5) == 3  # p->r is the largest rank
    for k, (x, s) in enumerate(zip(_batch(gpu_ctx, probs, ps), single)):  # a valid batch afterwards still gives the earlier bits
        _same_bits(x, s, f"after the refusals[{k}]")
