"""GPU tests of the fp64 mode of the batched offline solve (include/snmf.h: snmf_batch_create_fp64, snmf_sparse_nmf_batch_fp64;
se_snmf_nat_amd/batch.py: sparse_nmf_batch_fp64, BatchPlan64).

Every problem of every case is judged twice:
  (a) against the single fp64 solve, sparse_nmf(v_b, p, precision="fp64", init_w=..., init_h=...): W, H, div and cost
      compare with .tobytes() equality and n_iter is equal -- the contract of the mode;
  (b) against oracle/sparse_nmf_oracle.py at the bounds of tests/test_gpu_solve_f64.py, REL_WH = 1e-11 and REL_COST = 1e-12
      (derived there from the oracle's own sensitivity), and the exact n_iter.
The shapes are the smallest that reach each edge of the 64 x 64 x 16 tiles, the 2048-long splits of a contraction and the
256-frame row-sum chunks; the references of a case are computed once and shared."""
import functools

import numpy as np
import pytest

from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem
from test_gpu_solve_f64 import REL_COST, REL_WH, judge

pytestmark = pytest.mark.gpu


def _problems(F, Ts, r, seeds=None):
    seeds = seeds if seeds is not None else [10 * b for b in range(len(Ts))]
    return [synth_problem(F, T, r, seed_data=s, seed_init=s + 1, r_true=max(1, r // 2)) for T, s in zip(Ts, seeds)]


def _oracle(probs, ps, **kw):
    out = []
    for V, W0, H0 in probs:
        w, h, o = oracle_nmf(V, dict(ps, init_w=W0, init_h=H0), **kw)
        out.append((w, h, o["div"], o["cost"], o["n_iter"]))
    return out


def _single(probs, ps, ctx):
    from se_snmf_nat_amd import sparse_nmf
    return [sparse_nmf(V, dict(ps, init_w=W0, init_h=H0), ctx=ctx, precision="fp64") for V, W0, H0 in probs]


def _batch(probs, ps, ctx):
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    p = dict(ps, init_w=[q[1] for q in probs], init_h=[q[2] for q in probs])
    return sparse_nmf_batch_fp64([q[0] for q in probs], p, ctx=ctx)


def _same_bits(a, b, what=""):
    (w, h, o), (w2, h2, o2) = a, b
    assert o["n_iter"] == o2["n_iter"], (what, o["n_iter"], o2["n_iter"])
    assert w.dtype == w2.dtype == np.float64 and h.dtype == h2.dtype == np.float64
    assert w.shape == w2.shape and h.shape == h2.shape
    assert w.tobytes() == w2.tobytes(), (what, "W", float(np.max(np.abs(w - w2))))
    assert h.tobytes() == h2.tobytes(), (what, "H", float(np.max(np.abs(h - h2))))
    assert o["div"].tobytes() == o2["div"].tobytes(), (what, "div")
    assert o["cost"].tobytes() == o2["cost"].tobytes(), (what, "cost")


def _judge_both(name, res, singles, refs):
    assert len(res) == len(singles) == len(refs)
    for b, (x, s, ref) in enumerate(zip(res, singles, refs)):
        judge(f"batch {name}[{b}]", x, ref)                  # (b): prints the measured errors, then asserts the bounds
        _same_bits(x, s, f"{name}[{b}] against the single solve")  # (a)


# ---- 1. every edge of the tiles, the splits and the row-sum chunks -------------------------------------------------------
KL = dict(cf="kl", sparsity=5, cost_check=1)
CASES = {
    # one row in the second row tile, a contraction (r = 8) shorter than one 16-deep step, every frame-tile edge
    "tile_edges": (65, (1, 15, 16, 17, 63, 64, 65, 130), 8, dict(KL, max_iter=20)),
    # T: exactly one split, a one-frame second split, two whole splits and a ragged third, a direct store -- one launch; and
    # the ragged 256-frame row-sum chunk
    "split_T_kl": (37, (2048, 2049, 4500, 100), 13, dict(KL, max_iter=8)),
    "split_T_ed": (37, (2048, 2049, 4500, 100), 13, dict(cf="ed", sparsity=0.5, cost_check=1, max_iter=8)),
    # F = 2100: W' * R goes through partials
    "split_F": (2100, (70, 3), 5, dict(KL, max_iter=8)),
    "tile_multiples_b05": (64, (64, 128), 64, dict(cf="beta", beta=0.5, sparsity=0.3, cost_check=1, max_iter=10)),
    "is_129": (129, (300, 45, 96), 24, dict(cf="is", sparsity=0.1, cost_check=1, max_iter=15)),
    # update patterns
    "w_only": (65, (33, 100, 7), 8, dict(KL, max_iter=12, h_update_ind=np.zeros(8, bool))),
    "h_only": (65, (33, 100, 7), 8, dict(KL, max_iter=12, w_update_ind=np.zeros(8, bool))),
    "neither": (65, (33, 100, 7), 8, dict(KL, max_iter=12, w_update_ind=np.zeros(8, bool), h_update_ind=np.zeros(8, bool), conv_eps=1e-3)),
    "semi_supervised": (65, (33, 100, 7), 8, dict(KL, max_iter=12, w_update_ind=np.arange(8) >= 4)),
    "w_only_ed": (65, (33, 100, 7), 8, dict(cf="ed", sparsity=0.5, cost_check=1, max_iter=12, h_update_ind=np.zeros(8, bool))),
    # an r-vector sparsity
    "rvec_sparsity": (65, (33, 100, 7), 8, dict(cf="kl", sparsity=np.linspace(0.0, 9.0, 8), cost_check=1, max_iter=12)),
    "rvec_sparsity_column_is": (65, (33, 100, 7), 8, dict(cf="is", sparsity=np.linspace(0.0, 0.2, 8).reshape(-1, 1), cost_check=1,
                                                          max_iter=12)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    F, Ts, r, ps = CASES[name]
    probs = _problems(F, Ts, r)
    return probs, ps, _oracle(probs, ps)


@pytest.mark.parametrize("name", list(CASES))
def test_every_problem_is_the_single_fp64_solve(gpu_ctx, name):
    probs, ps, refs = _case(name)
    _judge_both(name, _batch(probs, ps, gpu_ctx), _single(probs, ps, gpu_ctx), refs)
    if name == "neither":  # nothing moves: the test of :272-284 fires at the second objective
        assert [ref[4] for ref in refs] == [2, 2, 2]


def test_no_cost_check_records_nothing_and_runs_to_the_end(gpu_ctx):
    F, Ts, r, _ = CASES["w_only"]
    probs = _problems(F, Ts, r)
    ps = dict(cf="kl", sparsity=5, cost_check=0, conv_eps=1e-2, max_iter=12)  # (conv_eps is not looked at without the objective)
    res = _batch(probs, ps, gpu_ctx)
    _judge_both("nocheck", res, _single(probs, ps, gpu_ctx), _oracle(probs, ps))
    for _, _, o in res:
        assert o["n_iter"] == 12 and not o["cost"].any() and not o["div"].any() and o["cost"].shape == (12,)


def test_floor_v_off_through_the_plan(gpu_ctx):
    """floor_v = 0 (sparse_nmf_GPU.m: no max(v, 1e-9)) through BatchPlan64, on a V with entries below the floor.  The oracle's
    gpu_variant leaves the objective vectors zero, so the factors and n_iter are judged, at the bounds of (b); sparse_nmf has
    no floor_v switch, so (a) does not apply."""
    from se_snmf_nat_amd import BatchPlan64
    F, Ts, r = 65, (33, 100, 7), 8
    probs = [(np.where(V < 0.02, 1e-12, V), W0, H0) for V, W0, H0 in _problems(F, Ts, r)]
    assert all((q[0] < 1e-9).any() for q in probs)
    ps = dict(cf="kl", sparsity=5, max_iter=12)
    refs = _oracle(probs, ps, gpu_variant=True)
    bp = BatchPlan64(gpu_ctx, F, r, Ts, beta=1.0, max_iter=12, sparsity=5, floor_v=False)
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run()
    res = [bp.get(k) for k in range(len(probs))]
    bp.close()
    for b, ((w, h, o), ref) in enumerate(zip(res, refs)):
        # (the plan records the objective of the unfloored V; the variant's vectors are zeros and are not compared)
        judge(f"batch floor_v=0 [{b}]", (w, h, dict(o, div=ref[2], cost=ref[3])), ref)
    # and the switch does something: the floored batch differs
    floored = _batch(probs, dict(ps, cost_check=1), gpu_ctx)
    assert floored[0][0].tobytes() != res[0][0].tobytes()


# ---- 2. every problem stops at its own iteration -------------------------------------------------------------------------
STOP_PS = dict(cf="kl", sparsity=5, max_iter=31, conv_eps=1e-3, cost_check=1)
STOP_IDX = [10, 31, 29, 30, 23]  # on the oracle; problem 1 would stop at 32 and reaches max_iter instead


@functools.lru_cache(maxsize=None)
def _stop_case():
    probs = [synth_problem(65, T, 8, seed_data=10 * b, seed_init=10 * b + 1, r_true=4) for b, T in ((0, 1), (1, 31), (2, 33), (3, 100), (5, 7))]
    return probs, _oracle(probs, STOP_PS)


def _stop_margin(cost, conv_eps):
    e = np.abs(np.diff(cost)) / cost[:-1]
    return np.min(np.abs(e - conv_eps) / conv_eps)


def test_every_problem_stops_at_its_own_iteration(gpu_ctx):
    probs, refs = _stop_case()
    # the condition on the inputs, on the oracle's history: no stop decision within 2 * REL_COST / conv_eps of its threshold
    assert [ref[4] for ref in refs] == STOP_IDX
    assert len(set(n for n in STOP_IDX if n < STOP_PS["max_iter"])) >= 3 and STOP_PS["max_iter"] in STOP_IDX
    assert len(refs[1][3]) == STOP_PS["max_iter"]  # (problem 1 ran to the end: a full-length history)
    for ref in refs:
        assert _stop_margin(ref[3], STOP_PS["conv_eps"]) >= 2 * REL_COST / STOP_PS["conv_eps"]
    res = _batch(probs, STOP_PS, gpu_ctx)
    assert [o["n_iter"] for _, _, o in res] == STOP_IDX
    # (a) holds the factors of a stopped problem to those of its own stop iterate: the single solve's
    _judge_both("own_stop", res, _single(probs, STOP_PS, gpu_ctx), refs)


# ---- 3. company, order, entry -------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_company_or_the_order(gpu_ctx):
    probs, _ = _stop_case()
    base = _batch(probs, STOP_PS, gpu_ctx)
    for b in range(len(probs)):  # each problem as a batch of one
        _same_bits(_batch([probs[b]], STOP_PS, gpu_ctx)[0], base[b], f"alone[{b}]")
    for b, (x, y) in enumerate(zip(_batch(probs[::-1], STOP_PS, gpu_ctx)[::-1], base)):  # the list reversed
        _same_bits(x, y, f"reversed[{b}]")
    # a split problem among direct ones, alone and in company
    sp, ps, _ = _case("split_T_kl")
    whole = _batch(sp, ps, gpu_ctx)
    _same_bits(_batch([sp[2]], ps, gpu_ctx)[0], whole[2], "T = 4500 alone")
    _same_bits(_batch([sp[3], sp[2]], ps, gpu_ctx)[1], whole[2], "T = 4500 behind T = 100")


def _plan(ctx, probs, ps, F=65, r=8):
    from se_snmf_nat_amd import BatchPlan64
    return BatchPlan64(ctx, F, r, [q[0].shape[1] for q in probs], beta=1.0, max_iter=ps["max_iter"], conv_eps=ps["conv_eps"],
                       sparsity=ps["sparsity"])


def test_continuation_and_reuse(gpu_ctx):
    probs, _ = _stop_case()
    base = _batch(probs, STOP_PS, gpu_ctx)
    bp = _plan(gpu_ctx, probs, STOP_PS)
    d = bp.describe()
    print(d)
    assert "k_b64_gemm" in d and "launches_per_iter=13" in d and "bytes=" in d
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run()
    for k in range(len(probs)):  # the resident entry against the one-shot entry
        _same_bits(bp.get(k), base[k], f"resident[{k}]")
    bp.close()
    # run(3) then run() against one run()
    bp = _plan(gpu_ctx, probs, STOP_PS)
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)
    bp.run(3)
    part = bp.get(0)
    assert part[2]["n_iter"] == 3 and len(part[2]["cost"]) == 3 and part[2]["cost"].tobytes() == base[0][2]["cost"][:3].tobytes()
    bp.run()
    for k in range(len(probs)):
        _same_bits(bp.get(k), base[k], f"run(3) + run()[{k}]")
    # a set_problem after a run starts a new batch: other data in the same slots (the frame counts are the plan's), against a
    # fresh plan
    other = [synth_problem(65, q[0].shape[1], 8, seed_data=500 + k, seed_init=600 + k, r_true=4) for k, q in enumerate(probs)]
    for k, q in enumerate(other):
        bp.set_problem(k, *q)
    bp.run()
    reused = [bp.get(k) for k in range(len(other))]
    bp.close()
    fresh = _plan(gpu_ctx, other, STOP_PS)
    for k, q in enumerate(other):
        fresh.set_problem(k, *q)
    fresh.run()
    for k in range(len(other)):
        _same_bits(reused[k], fresh.get(k), f"reuse[{k}]")
    fresh.close()
    assert reused[0][0].tobytes() != base[0][0].tobytes()


def test_f32_transfers_widen_on_the_way_in_and_round_on_the_way_out(gpu_ctx):
    probs, _ = _stop_case()
    p32 = [tuple(np.asarray(a, np.float32) for a in q) for q in probs]
    widened = [tuple(a.astype(np.float64) for a in q) for q in p32]
    a = _plan(gpu_ctx, probs, STOP_PS)
    b = _plan(gpu_ctx, probs, STOP_PS)
    for k in range(len(probs)):
        a.set_problem(k, *p32[k])      # float32 arrays: snmf_batch_set_problem_f32
        b.set_problem(k, *widened[k])  # their widened values: snmf_batch_set_problem_f64
    a.run()
    b.run()
    for k in range(len(probs)):
        ra, rb = a.get(k), b.get(k)
        _same_bits(ra, rb, f"f32 in[{k}]")
        w32, h32, o32 = a.get(k, dtype=np.float32)
        assert w32.dtype == np.float32 and h32.dtype == np.float32
        assert w32.tobytes() == ra[0].astype(np.float32).tobytes() and h32.tobytes() == ra[1].astype(np.float32).tobytes()
        assert o32["n_iter"] == ra[2]["n_iter"] and o32["cost"].tobytes() == ra[2]["cost"].tobytes()
    a.close()
    b.close()


# ---- 4. the fp32 batch is untouched, refusals leave the context usable ----------------------------------------------------------
def test_fp32_batch_gives_the_same_bits_around_an_fp64_batch(gpu_ctx):
    from se_snmf_nat_amd import BatchPlan64, SnmfError, sparse_nmf_batch
    probs, _ = _stop_case()
    p = dict(STOP_PS, init_w=[q[1] for q in probs], init_h=[q[2] for q in probs])
    vs = [q[0] for q in probs]
    before = sparse_nmf_batch(vs, p, ctx=gpu_ctx)
    r64 = _batch(probs, STOP_PS, gpu_ctx)
    # a refusal: more memory than the device has, checked before anything is allocated, with the limit in the message
    with pytest.raises(SnmfError, match="bytes of device memory") as e:
        BatchPlan64(gpu_ctx, 100000, 1000, [2000000, 2000000])
    assert e.value.status == 8
    bp = BatchPlan64(gpu_ctx, 65, 8, [7, 31], max_iter=5, sparsity=5)
    bp.set_problem(0, *probs[4])
    with pytest.raises(SnmfError) as e:  # run before every problem is set, get before run
        bp.run()
    assert e.value.status == 7
    with pytest.raises(SnmfError) as e:
        bp.get(0)
    assert e.value.status == 7
    bp.close()
    after = sparse_nmf_batch(vs, p, ctx=gpu_ctx)
    for b, (x, y) in enumerate(zip(before, after)):
        _same_bits(x, y, f"fp32 batch[{b}]")
    again = _batch(probs, STOP_PS, gpu_ctx)
    for b, (x, y) in enumerate(zip(r64, again)):
        _same_bits(x, y, f"fp64 batch after the refusals[{b}]")
    # and the two modes are two computations: the fp32 batch sits orders of magnitude above the fp64 bound
    d = float(np.linalg.norm(before[3][0] - r64[3][0]) / np.linalg.norm(r64[3][0]))
    assert 1e-9 < d < 1e-3, d
