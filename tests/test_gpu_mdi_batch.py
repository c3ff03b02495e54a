"""GPU tests of the batched missing-data solves (include/snmf.h: snmf_batch_create_mdi_fp64, snmf_batch_set_problem_mdi_f64,
snmf_batch_get_v_mdi_f64, snmf_mdi_batch_fp64; se_snmf_nat_amd/batch.py: snmf_mdi_batch, snmf_mdi_Sm_batch, BatchPlanMdi64).

The contract is bit equality with the single call: for every problem of every case v_mdi, h, w, div and cost compare with
.tobytes() equality and n_iter is equal to what snmf_mdi / snmf_mdi_Sm(v_b, mask_b, p_b, precision="fp64") gives on that
problem alone.  Nothing is held to a tolerance except in the last section, where two cases are also held to
oracle/mdi_oracle.py at the bounds of tests/test_gpu_mdi_f64.py (REL_WH = 1e-11, REL_COST = 1e-12, n_iter equal; derived there
from the oracle's own sensitivity).

Shapes: F = 65 (one row in a second 64-row tile), r = 9 (shorter than one 16-deep step of the contraction), and in ONE batch
the frame counts 1, 63, 64, 90, 257 (one frame past a 256-frame row-sum chunk) and 2100 (past the 2048-frame split: a problem
with split partials and problems with a direct store share the grouped GEMM launch).  Inputs: synth_problem values rounded to
fp32 and held as doubles; the binary mask of problem b is RandomState(100 + b).rand(F, T) > 0.3, the soft mask
clip(0.8 M + 0.2 rand, 0, 1); frame 7 of the T = 90 problem and the last frame of the T = 257 problem have no observed entry.
The references of a case are computed once and shared."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from oracle.mdi_oracle import snmf_mdi as oracle_mdi
from oracle.sparse_nmf_oracle import synth_problem

pytestmark = pytest.mark.gpu
REL_WH = 1e-11    # tests/test_gpu_mdi_f64.py
REL_COST = 1e-12  # tests/test_gpu_mdi_f64.py
FLR = 1e-9
STATE = 7  # SNMF_ERR_STATE
F, R = 65, 9
TS = (1, 63, 64, 90, 257, 2100)


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    nz = b != 0
    if (a[~nz] != 0).any():
        return float("inf")
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


@functools.lru_cache(maxsize=None)
def _problem(T, b, other=False):
    """(V, W0, H0, binary mask, soft mask) of problem b with T frames, read-only."""
    s = 500 + 10 * b if other else 10 * b
    V, W0, H0 = (f32r(a) for a in synth_problem(F, T, R, seed_data=s, seed_init=s + 1, r_true=4))
    rs = np.random.RandomState(100 + s)
    M = (rs.rand(F, T) > 0.3).astype(np.float64)
    if T == 90:
        M[:, 7] = 0.0
    if T == 257:
        M[:, 256] = 0.0
    Ms = np.clip(M * 0.8 + rs.rand(F, T) * 0.2, 0, 1)
    for a in (V, W0, H0, M, Ms):
        a.setflags(write=False)
    return V, W0, H0, M, Ms


def _problems(Ts=TS, other=False):
    return [_problem(T, b, other) for b, T in enumerate(Ts)]


def _single(probs, ps, ctx, soft=False):
    """Every problem alone: [(v_mdi, h, objective, w)]"""
    from se_snmf_nat_amd import snmf_mdi, snmf_mdi_Sm
    out = []
    for V, W0, H0, M, Ms in probs:
        info = {}
        v, h, o = (snmf_mdi_Sm if soft else snmf_mdi)(V, Ms if soft else M, dict(ps, init_w=W0, init_h=H0), ctx=ctx, precision="fp64",
                                                       info=info)
        out.append((v, h, o, info["w"]))
    return out


def _batch(probs, ps, ctx, soft=False):
    from se_snmf_nat_amd import snmf_mdi_batch, snmf_mdi_Sm_batch
    p = dict(ps, init_w=[q[1] for q in probs], init_h=[q[2] for q in probs])
    info = {}
    res = (snmf_mdi_Sm_batch if soft else snmf_mdi_batch)([q[0] for q in probs], [q[4] if soft else q[3] for q in probs], p, ctx=ctx,
                                                          info=info)
    assert len(res) == len(info["w"]) == len(probs)
    return [(v, h, o, w) for (v, h, o), w in zip(res, info["w"])]


def _same_bits(a, b, what=""):
    (v, h, o, w), (v2, h2, o2, w2) = a, b
    assert o["n_iter"] == o2["n_iter"], (what, o["n_iter"], o2["n_iter"])
    for x, y, nm in ((v, v2, "v_mdi"), (h, h2, "h"), (w, w2, "w"), (o["div"], o2["div"], "div"), (o["cost"], o2["cost"], "cost")):
        assert x.dtype == y.dtype == np.float64 and x.shape == y.shape, (what, nm, x.shape, y.shape)
        assert np.asfortranarray(x).tobytes(order="F") == np.asfortranarray(y).tobytes(order="F"), (what, nm, float(np.max(np.abs(x - y))))


# ---- 1. bit equality with the single call ------------------------------------------------------------------------------------
KL = dict(cf="kl", sparsity_mdi=0.5, conv_eps_mdi=0, cost_check=1, max_iter=10)
CASES = {  # name -> (settings, soft)
    "kl": (KL, False),
    "ed": (dict(KL, cf="ed"), False),
    "is": (dict(KL, cf="is", sparsity_mdi=0.1), False),
    "b15": (dict(KL, cf="beta", beta=1.5, sparsity_mdi=1), False),
    "kl_soft": (KL, True),
    "h_only": (dict(KL, w_update_ind=np.zeros(R, bool)), False),
    "w_only": (dict(KL, h_update_ind=np.zeros(R, bool)), False),
    "neither": (dict(KL, max_iter=4, w_update_ind=np.zeros(R, bool), h_update_ind=np.zeros(R, bool)), False),
    "nocheck": (dict(KL, cost_check=0, conv_eps_mdi=1e-2), False),
    "ed_nocheck_soft": (dict(KL, cf="ed", cost_check=0), True),
    # no iteration at all: v_mdi is the gain-matched imputation from the scaled initial factors, as in the single call
    "zero_iters": (dict(KL, max_iter=0), False),
    "zero_iters_ed_soft": (dict(KL, cf="ed", max_iter=0, cost_check=0), True),
    "rvec_semi": (dict(KL, sparsity_mdi=np.linspace(0.0, 4.0, R), w_update_ind=np.arange(R) >= 4), False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_problem_is_the_single_fp64_missing_data_solve(gpu_ctx, name):
    ps, soft = CASES[name]
    probs = _problems()
    res, singles = _batch(probs, ps, gpu_ctx, soft), _single(probs, ps, gpu_ctx, soft)
    for b, (x, s) in enumerate(zip(res, singles)):
        _same_bits(x, s, f"{name}[{b}] T={TS[b]}")
        assert np.isfinite(x[0]).all() and x[0].min() >= FLR
    if "zero_iters" in name:
        for (v, h, o, w), (V, W0, H0, _, _) in zip(res, probs):
            assert o["n_iter"] == 0 and len(o["cost"]) == 0 and len(o["div"]) == 0
            # only the initial scaling touched the factors: an F-term sum, a root, a quotient or a product, each rounded once
            nrm = np.sqrt((W0 ** 2).sum(0))
            assert rel(w, W0 / nrm) < (F + 4) * 2.0 ** -53 and rel(h, H0 * nrm[:, None]) < (F + 4) * 2.0 ** -53
    if "nocheck" in name:  # cost_check = 0: zero vectors and no stop, the imputation runs all the same
        for v, _, o, _ in res:
            assert o["n_iter"] == 10 and not o["div"].any() and not o["cost"].any() and len(o["cost"]) == 10
        assert not np.array_equal(res[3][0], np.maximum(probs[3][0] * probs[3][3], FLR))
    if not soft:  # observed entries are the input's bits; a frame without an observed entry is the floor
        for (v, _, _, _), (V, _, _, M, _) in zip(res, probs):
            assert np.array_equal(v[M == 1], np.maximum(V, FLR)[M == 1])
        assert (res[3][0][:, 7] == FLR).all() and (res[4][0][:, 256] == FLR).all()
        assert (res[3][0][:, 8][probs[3][3][:, 8] == 0] > FLR).all()  # (and a missing entry of an observed frame is not)


# ---- 2. every problem stops at its own iteration -----------------------------------------------------------------------------
# conv_eps_mdi chosen on the CPU oracle: its stop indices on the six problems are 8, 31, 27, 26, 27, 28 (the second would stop
# later and reaches max_iter), and none of its |dcost| / cost comes within 0.1 % of the threshold
STOP_PS = dict(cf="kl", sparsity_mdi=5, conv_eps_mdi=2e-3, cost_check=1, max_iter=31)
PLAIN_STOP_PS = dict(cf="kl", sparsity=5, conv_eps=2e-3, cost_check=1, max_iter=31)  # the same settings under sparse_nmf's names


def _oracle(probs, ps, soft=False):
    out = []
    for V, W0, H0, M, Ms in probs:
        v, h, o = oracle_mdi(V, Ms if soft else M, dict(ps, init_w=W0, init_h=H0))
        out.append((v, h, o["w"], o["div"], o["cost"], o["n_iter"]))
    return out


@functools.lru_cache(maxsize=None)
def _stop_case():
    probs = _problems()
    return probs, _oracle(probs, STOP_PS)


def _judge(name, res, ref):
    """The errors against the oracle, printed, then the bounds of tests/test_gpu_mdi_f64.py."""
    v, h, o, w = res
    vr, hr, wr, divr, costr, nr = ref
    ev, eh, ew = rel(v, vr), rel(h, hr), rel(w, wr)
    same_len = len(o["div"]) == len(divr) and len(o["cost"]) == len(costr)
    ed = relmax(o["div"], divr) if same_len else float("inf")
    ec = relmax(o["cost"], costr) if same_len else float("inf")
    print(f"mdi batch {name}: n_iter={o['n_iter']} (oracle {nr}) relV={ev:.2e} relH={eh:.2e} relW={ew:.2e} reldiv={ed:.2e} relcost={ec:.2e}")
    assert o["n_iter"] == nr and same_len
    assert ev < REL_WH and eh < REL_WH and ew < REL_WH, (ev, eh, ew)
    assert ed < REL_COST and ec < REL_COST, (ed, ec)


def test_every_problem_stops_at_its_own_iteration(gpu_ctx):
    probs, refs = _stop_case()
    stops = [ref[5] for ref in refs]
    print("oracle stop indices", stops)
    mi = STOP_PS["max_iter"]
    # conv_eps_mdi was chosen on the CPU oracle: the problems stop at different iterations and one runs to max_iter
    assert len(set(n for n in stops if n < mi)) >= 3 and mi in stops
    assert any(len(ref[4]) == mi for ref in refs)
    res = _batch(probs, STOP_PS, gpu_ctx)
    for b, (x, s) in enumerate(zip(res, _single(probs, STOP_PS, gpu_ctx))):
        _same_bits(x, s, f"own_stop[{b}] T={TS[b]}")
    got = [o["n_iter"] for _, _, o, _ in res]
    assert len(set(got)) >= 3 and mi in got, got


# ---- 3. M == 1 is the plain fp64 batch ---------------------------------------------------------------------------------------
def test_full_masks_give_the_plain_fp64_batch_bit_for_bit(gpu_ctx):
    from se_snmf_nat_amd import snmf_mdi_batch, sparse_nmf_batch_fp64
    probs = _problems()
    vs = [q[0] for q in probs]
    inits = dict(init_w=[q[1] for q in probs], init_h=[q[2] for q in probs])
    plain = sparse_nmf_batch_fp64(vs, dict(PLAIN_STOP_PS, **inits), ctx=gpu_ctx)
    info = {}
    masked = snmf_mdi_batch(vs, [np.ones_like(v) for v in vs], dict(STOP_PS, **inits), ctx=gpu_ctx, info=info)
    for b, ((w, h, o), (vm, hm, om), wm) in enumerate(zip(plain, masked, info["w"])):
        assert om["n_iter"] == o["n_iter"], b
        assert wm.tobytes() == w.tobytes() and hm.tobytes() == h.tobytes(), b
        assert om["div"].tobytes() == o["div"].tobytes() and om["cost"].tobytes() == o["cost"].tobytes(), b
        assert vm.tobytes() == np.asfortranarray(np.maximum(vs[b], FLR)).tobytes(), b
    assert min(o["n_iter"] for _, _, o in plain) < 31


# ---- 4. company independence -------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_company_or_the_slot(gpu_ctx):
    probs, _ = _stop_case()
    base = _batch(probs, STOP_PS, gpu_ctx)  # (problem 3 in slot 3 of a batch of 6)
    x = probs[3]
    _same_bits(_batch([x], STOP_PS, gpu_ctx)[0], base[3], "T = 90 in slot 0 of a batch of 1")
    _same_bits(_batch([probs[5], x, probs[0]], STOP_PS, gpu_ctx)[1], base[3], "T = 90 between T = 2100 and T = 1")
    _same_bits(_batch([_problem(64, 9, True), _problem(257, 8, True), x], STOP_PS, gpu_ctx)[2], base[3], "T = 90 behind other data")
    # the split problem alone and behind a direct one
    _same_bits(_batch([probs[5]], STOP_PS, gpu_ctx)[0], base[5], "T = 2100 alone")
    _same_bits(_batch([probs[1], probs[5]], STOP_PS, gpu_ctx)[1], base[5], "T = 2100 behind T = 63")


# ---- 5. the handle's state machine -------------------------------------------------------------------------------------------
HTS = TS[:5]  # (the handle's life does not depend on the split: the five direct problems)


def _plan(ctx, cls="BatchPlanMdi64", **kw):
    import se_snmf_nat_amd
    ps = dict(beta=1.0, max_iter=STOP_PS["max_iter"], conv_eps=STOP_PS["conv_eps_mdi"], sparsity=STOP_PS["sparsity_mdi"])
    return getattr(se_snmf_nat_amd, cls)(ctx, F, R, HTS, **dict(ps, **kw))


def _fill(bp, probs):
    for k, (V, W0, H0, M, _) in enumerate(probs):
        bp.set_problem(k, V, M, W0, H0)


def _results(bp):
    out = []
    for k in range(len(HTS)):
        w, h, o = bp.get(k)
        out.append((bp.get_v_mdi(k), h, o, w))
    return out


def _launches(d):
    return int(re.search(r"launches_per_iter=(\d+)", d).group(1))


def test_continuation_reading_v_mdi_does_not_disturb_the_run(gpu_ctx):
    probs = _problems(HTS)
    base = _batch(probs, STOP_PS, gpu_ctx)
    assert all(o["n_iter"] > 3 for _, _, o, _ in base)
    bp = _plan(gpu_ctx)
    _fill(bp, probs)
    bp.run(3)
    part = _results(bp)
    for k, ((v, _, o, _), (vb, _, ob, _)) in enumerate(zip(part, base)):
        assert o["n_iter"] == 3 and o["cost"].tobytes() == ob["cost"][:3].tobytes(), k
        assert v.shape == vb.shape and v.min() >= FLR and v.tobytes() != vb.tobytes(), k  # (the imputation of the third iterate)
    bp.run()
    for k, (x, y) in enumerate(zip(_results(bp), base)):
        _same_bits(x, y, f"run(3) + get_v_mdi + run()[{k}]")
    for k, (x, y) in enumerate(zip(_results(bp), base)):  # (and reading twice gives the same bytes)
        _same_bits(x, y, f"read again[{k}]")
    bp.close()


def test_cross_mode_entries_are_refused_and_leave_the_handle_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.api import _ptr
    probs = _problems(HTS)
    base = _batch(probs, STOP_PS, gpu_ctx)
    V, W0, H0, M, _ = (np.asfortranarray(a) for a in probs[1])
    V32, W32, H32 = (np.asfortranarray(a, dtype=np.float32) for a in (V, W0, H0))
    out = np.empty((F, HTS[1]), order="F")
    bp = _plan(gpu_ctx)
    for k, (v, w0, h0, m, _) in enumerate(probs):
        assert lib.snmf_batch_set_problem_f64(bp._h, 1, _ptr(V), F, _ptr(W0), _ptr(H0)) == STATE  # a problem without its mask
        assert b"snmf_batch_set_problem_mdi_f64" in lib.snmf_last_error()
        assert lib.snmf_batch_set_problem_f32(bp._h, 1, _ptr(V32), F, _ptr(W32), _ptr(H32)) == STATE
        with pytest.raises(SnmfError) as e:  # nothing has run
            bp.get_v_mdi(0)
        assert e.value.status == STATE
        bp.set_problem(k, v, m, w0, h0)
    assert lib.snmf_batch_get_v_mdi_f64(bp._h, 1, _ptr(out), F) == STATE
    assert b"before snmf_batch_run" in lib.snmf_last_error()
    bp.run(2)
    assert lib.snmf_batch_set_problem_f64(bp._h, 1, _ptr(V), F, _ptr(W0), _ptr(H0)) == STATE  # (does not start a new batch)
    assert lib.snmf_batch_get_v_mdi_f64(bp._h, 1, _ptr(out), F - 1) == 1 and lib.snmf_batch_get_v_mdi_f64(bp._h, 5, _ptr(out), F) == 1
    bp.run()
    for k, (x, y) in enumerate(zip(_results(bp), base)):
        _same_bits(x, y, f"masked handle after the refusals[{k}]")
    bp.close()
    # a plain fp64 batch refuses the masked entries, before and after a run, and gives the bytes of an untouched one
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    plain = sparse_nmf_batch_fp64([q[0] for q in probs], dict(PLAIN_STOP_PS, init_w=[q[1] for q in probs], init_h=[q[2] for q in probs]), ctx=gpu_ctx)
    bq = _plan(gpu_ctx, "BatchPlan64")
    for k, (v, w0, h0, _, _) in enumerate(probs):
        assert lib.snmf_batch_set_problem_mdi_f64(bq._h, 1, _ptr(V), F, _ptr(M), F, _ptr(W0), _ptr(H0)) == STATE
        bq.set_problem(k, v, w0, h0)
    bq.run(2)
    assert lib.snmf_batch_set_problem_mdi_f64(bq._h, 1, _ptr(V), F, _ptr(M), F, _ptr(W0), _ptr(H0)) == STATE
    assert lib.snmf_batch_get_v_mdi_f64(bq._h, 1, _ptr(out), F) == STATE
    assert b"snmf_batch_create_mdi_fp64" in lib.snmf_last_error()
    bq.run()
    for k, (w, h, o) in enumerate(plain):
        w2, h2, o2 = bq.get(k)
        assert o2["n_iter"] == o["n_iter"] and w2.tobytes() == w.tobytes() and h2.tobytes() == h.tobytes(), k
        assert o2["cost"].tobytes() == o["cost"].tobytes(), k
    bq.close()


def test_a_new_batch_on_a_used_masked_handle(gpu_ctx):
    from se_snmf_nat_amd import SnmfError
    probs, other = _problems(HTS), _problems(HTS, other=True)
    bp = _plan(gpu_ctx)
    _fill(bp, probs)
    bp.run()
    first = _results(bp)
    # a set_problem after a run starts a new batch: run and the reads are refused until every problem is set again
    for k, (V, W0, H0, M, _) in enumerate(other):
        bp.set_problem(k, V, M, W0, H0)
        if k + 1 < len(other):
            for call in (bp.run, lambda: bp.get(0), lambda: bp.get_v_mdi(0)):
                with pytest.raises(SnmfError) as e:
                    call()
                assert e.value.status == STATE
    bp.run()
    reused = _results(bp)
    bp.close()
    fresh = _batch(other, STOP_PS, gpu_ctx)
    for k, (x, y) in enumerate(zip(reused, fresh)):
        _same_bits(x, y, f"reuse[{k}]")
    assert reused[1][0].tobytes() != first[1][0].tobytes()


def test_describe_counts_the_mask_block_and_the_launches(gpu_ctx):
    sumT = sum(HTS)
    d = {}
    for cls in ("BatchPlan64", "BatchPlanMdi64"):
        for cc in (True, False):
            bp = _plan(gpu_ctx, cls, cost_check=cc)
            d[cls, cc] = bp.describe()
            bp.close()
    print(d["BatchPlanMdi64", True])
    print(d["BatchPlanMdi64", False])
    byt = lambda s: int(re.search(r" bytes=(\d+)", s).group(1))  # noqa: E731
    for cc in (True, False):
        m, q = d["BatchPlanMdi64", cc], d["BatchPlan64", cc]
        assert f"mask_bytes={8 * F * sumT}" in m and "k_b64_mdi_impute" in m and "mask_bytes" not in q
        # the two blocks are in the total (each piece of the device block is rounded up to 256 bytes)
        assert 0 <= byt(m) - byt(q) - 8 * F * (sumT + max(HTS)) < 512
    # with the objective the fused kernel takes the objective's place; without it the re-imputation is one more launch
    assert _launches(d["BatchPlan64", True]) == 13 and _launches(d["BatchPlanMdi64", True]) == 13
    assert _launches(d["BatchPlan64", False]) == 11 and _launches(d["BatchPlanMdi64", False]) == 12
    assert "k_b64_mdi_obj grid=" in d["BatchPlanMdi64", True] and "k_b64_obj grid=" in d["BatchPlan64", True]


# ---- 6. against the oracle ---------------------------------------------------------------------------------------------------
def _stop_margin(cost, conv_eps):
    e = np.abs(np.diff(cost)) / cost[:-1]
    return np.min(np.abs(e - conv_eps) / conv_eps)


def test_the_stop_case_against_the_oracle(gpu_ctx):
    probs, refs = _stop_case()
    for ref in refs:  # no stop decision of the oracle within 2 * REL_COST / conv_eps of its threshold
        assert _stop_margin(ref[4], STOP_PS["conv_eps_mdi"]) >= 2 * REL_COST / STOP_PS["conv_eps_mdi"]
    for b, (x, ref) in enumerate(zip(_batch(probs, STOP_PS, gpu_ctx), refs)):
        _judge(f"own_stop[{b}] T={TS[b]}", x, ref)


def test_a_soft_mask_case_against_the_oracle(gpu_ctx):
    ps = dict(CASES["b15"][0], w_update_ind=np.arange(R) >= 4)
    probs = _problems()
    for b, (x, ref) in enumerate(zip(_batch(probs, ps, gpu_ctx, soft=True), _oracle(probs, ps, soft=True))):
        _judge(f"b15_soft_semi[{b}] T={TS[b]}", x, ref)
