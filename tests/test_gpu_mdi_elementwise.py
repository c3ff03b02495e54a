"""The missing-data-imputation solves judged element by element, on every geometry a masked plan reaches, and the state machine of
the deferred re-imputation judged exactly.  tests/mdi_elementwise.py has the fp64 masked step, the bounds and the case table.

PER CASE (mdi_elementwise.MDI_CASES).  A Plan with the case's mask (set_mask), conv_eps = 0, max_iter = 3; V (fp32), W0, H0; init();
then three steps run(1) at a time.  The plan's V cannot be read back, so V is tracked in fp64: V_0 = mdi_start, V_k =
mdi_impute(V_{k-1}, M, W_k, H_k) with the (W_k, H_k) read from the device.  Per step:
  - H_k against ref_hstep(V_{k-1}, W_{k-1}, H_{k-1}) and W_k against ref_wstep(V_{k-1}, W_{k-1}, H_k), per element and per region
    within tau_H + dV_{k-1} and tau_W + 4 dV_{k-1};
  - an H-only plan leaves W bit for bit, a W-only plan H; semi mode's fixed columns stay within 4u.
After the last step:
  - the objective of every iterate against the fp64 divergence on the re-imputed V_k + sum(S .* H_k) on the device's (W_k, H_k),
    with REL_COST and the 2e-7 * sum(V_k) floor of the unmasked module;
  - v_MDI against mdi_final(V_3, M, W_3, H_3): the floored fp32 input bit for bit where M = 1, within tau_V elsewhere, per frame;
    with a mask of ones, all of it bit for bit.  With cost_check off the last re-imputation runs as a pass of its own, and v_MDI is
    the only witness of it.
The plan's describe() must name the MDI pass with the grid it launches (min(Tp / 32, n_cu) workgroups of 512 threads) and the
statistics geometry the case is there for.

No limit of this module was measured on the kernels it judges: the bounds are derived (tests/mdi_elementwise.py), and the
statistics kernels' own rounding is pinned by tests/test_gpu_elementwise.py.  What is new here is the V they are given, and an error
in that V is structural.  For information, measured on an MI355X (n_cu = 256): per case the largest worst-element relative error
over bound and the largest RMS relative error over the three steps and the regions, and v_MDI's.

    case                        worst H / tau_H    RMS H   worst W / tau_W    RMS W   worst v_MDI / tau_V  RMS
    kl_two_rounds_F257         1.1e-06 / 3.7e-05  2.4e-07   3.5e-08 / 9.2e-05  6.2e-09   5.0e-07 / 8.5e-06  1.0e-07
    kl_3tiles_F65              4.9e-07 / 1.0e-05  1.5e-07   1.5e-07 / 3.5e-05  3.9e-08   2.1e-07 / 2.9e-06  6.4e-08
    kl_T20_F513                1.4e-06 / 7.5e-05  3.6e-07   4.1e-07 / 1.5e-04  6.6e-08   5.7e-07 / 1.9e-05  1.0e-07
    ed_gram_5tiles_F130        8.6e-07 / 2.0e-05  2.2e-07   1.5e-07 / 5.4e-05  3.4e-08   3.7e-07 / 5.6e-06  8.5e-08
    kl_sync_F513               1.6e-06 / 6.5e-05  3.5e-07   1.3e-07 / 1.2e-04  2.0e-08   3.5e-07 / 4.9e-06  8.0e-08
    kl_sync_F422               1.4e-06 / 5.6e-05  3.5e-07   7.0e-08 / 1.1e-04  1.3e-08   4.5e-07 / 7.0e-06  7.6e-08
    is_F33                     5.9e-07 / 1.0e-05  1.3e-07   5.1e-08 / 4.0e-05  1.3e-08   3.4e-07 / 4.9e-06  7.3e-08
    b05_F64                    7.1e-07 / 1.6e-05  1.7e-07   4.5e-08 / 5.5e-05  1.1e-08   4.3e-07 / 8.5e-06  1.0e-07
    b15_F257                   1.5e-06 / 3.9e-05  3.4e-07   6.3e-08 / 8.7e-05  1.2e-08   5.7e-07 / 1.2e-05  9.0e-08
    is_wonly_F130              -                        -   4.6e-08 / 6.0e-05  9.5e-09   3.7e-07 / 5.6e-06  8.5e-08
    b15_honly_F65              7.9e-07 / 1.2e-05  1.7e-07   -                        -   4.5e-07 / 5.6e-06  7.4e-08
    kl_loader4_F129            8.7e-07 / 2.9e-05  1.9e-07   3.3e-08 / 9.8e-05  5.5e-09   7.2e-07 / 1.9e-05  1.5e-07
    kl_loader8_F289_wonly      -                        -   5.3e-08 / 1.3e-04  9.4e-09   8.7e-07 / 1.9e-05  1.1e-07
    kl_nk8_F513                1.7e-06 / 8.6e-05  3.6e-07   9.3e-08 / 2.3e-04  1.6e-08   1.1e-06 / 3.6e-05  2.1e-07
    kl_nk16_kg2_F65            8.2e-07 / 8.1e-05  1.5e-07   6.3e-08 / 3.2e-04  1.0e-08   1.5e-06 / 1.1e-04  2.2e-07
    kl_two_row_groups_F513     1.9e-06 / 7.5e-05  3.6e-07   7.9e-08 / 2.1e-04  1.4e-08   8.5e-07 / 1.9e-05  1.5e-07
    kl_wsf_F64_r100            6.9e-07 / 2.1e-05  1.4e-07   3.1e-08 / 8.6e-05  5.4e-09   7.9e-07 / 1.9e-05  1.1e-07
    kl_wsf_shared_F64_r40      6.6e-07 / 1.4e-05  1.5e-07   2.6e-08 / 5.8e-05  5.3e-09   5.6e-07 / 8.5e-06  1.0e-07
    kl_wsr_F513_r20            1.7e-06 / 6.5e-05  3.8e-07   3.4e-08 / 1.3e-04  6.4e-09   4.2e-07 / 4.9e-06  6.9e-08
    kl_wsr_semi_F422           1.5e-06 / 5.6e-05  3.2e-07   2.9e-08 / 1.2e-04  5.8e-09   5.3e-07 / 7.0e-06  9.5e-08
    ed_nk16_gram_F257          1.7e-06 / 6.8e-05  3.4e-07   8.0e-08 / 2.2e-04  1.2e-08   1.2e-06 / 5.5e-05  1.6e-07
    ed_nk16_wonly_F257         -                        -   7.1e-08 / 2.2e-04  1.4e-08   1.2e-06 / 5.5e-05  2.6e-07
    ed_honly_F130              9.5e-07 / 2.0e-05  2.2e-07   -                        -   3.7e-07 / 5.6e-06  8.6e-08
    kl_honly_F257              1.2e-06 / 3.7e-05  2.5e-07   -                        -   5.0e-07 / 8.5e-06  8.2e-08
    kl_wonly_F257              -                        -   6.2e-08 / 8.5e-05  1.2e-08   4.7e-07 / 8.5e-06  1.0e-07
    kl_ones_F65                5.2e-07 / 9.4e-06  1.6e-07   9.7e-08 / 3.1e-05  3.7e-08   0.0e+00 / 1.7e-06  0.0e+00
    kl_nocost_F257             1.1e-06 / 3.7e-05  2.4e-07   8.1e-08 / 8.5e-05  1.4e-08   4.9e-07 / 8.5e-06  8.1e-08

THE STATE MACHINE (the re-imputation of iteration j rides on the Lam pass of iteration j + 1, on the final objective pass, or on a
pass of its own):
  - a soft-mask solve that stops early, stepped with run(1) beyond the stop (and into max_iter), and in one run() call: H, W, the
    objective and v_MDI are those of the stop iterate; a launch that re-imputed V after the stop would move v_MDI at every entry;
  - one run() against run(1) x n at conv_eps = 0: bit-identical H, W, objective history and v_MDI, for full, H-only and W-only
    plans with cost_check on and off;
  - run() after max_iter and a second get_v_mdi() change nothing;
  - frames and rows that are entirely missing or entirely observed, against oracle/mdi_oracle.py with the tolerances of
    tests/test_mdi.py, plus the exact facts (the floor in an entirely missing frame, the input in an entirely observed one).
"""
import time

import numpy as np
import pytest

from elementwise import FLR, U, chain_t, compare, ref_hstep, ref_wstep
from mdi_elementwise import (MDI_CASES, case_masks, compare_vmdi, mask_image, mdi_case_data, mdi_cost, mdi_final, mdi_grid,
                             mdi_impute, mdi_regions, mdi_start, tau_h_mdi, tau_vmdi, tau_w_mdi)
from oracle.mdi_oracle import snmf_mdi as oracle_mdi
from oracle.sparse_nmf_oracle import synth_problem

pytestmark = pytest.mark.gpu

REL_COST = 1e-5  # test_gpu_parity.REL_COST
REL = 1e-4       # tests/test_mdi.REL

SWITCHES = ("SNMF_HSTEP_RP", "SNMF_HSTEP_SPLIT", "SNMF_WSTATS_NL", "SNMF_ITER_SF", "SNMF_GRAM_P", "SNMF_NO_SMALL", "SNMF_HFOLD")


@pytest.fixture(autouse=True)
def default_plans(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _f32_floor(V):
    return np.fmax(np.asarray(V, np.float32), np.float32(FLR))


def run_case(ctx, case, dtype=np.float64):
    """One case through its steps with every assertion of the module docstring.  Returns {"H" / "W": {region: (worst, rms)}} with
    the largest values over the steps, the bounds of the last step, v_MDI's (worst, tau_V, rms) and the describe() text.
    dtype = np.float32: V, the mask and v_MDI through the fp32 entry points."""
    from se_snmf_nat_amd import Plan
    F, T, r, beta, mode, steps = case["F"], case["T"], case["r"], case["beta"], case["mode"], case["steps"]
    V, M, W0, H0, S = mdi_case_data(case)
    ones = bool((M == 1.0).all())
    w_ind, h_ind = case_masks(mode, r)
    upd_h, upd_w = mode != "w", mode != "h"
    pl = Plan(ctx, F, T, r, beta=beta, max_iter=steps, conv_eps=0.0, cost_check=case["cost_check"], sparsity=S,
              w_update_ind=w_ind, h_update_ind=h_ind)
    try:
        pl.set_mask(M.astype(np.float32) if dtype == np.float32 else M)
        desc = pl.describe()
        tiles, grid = mdi_grid(desc)  # (asserts that the text's grid is min(Tp / 32, n_cu))
        assert "hstep: k_hstep (MDI pass" in desc and f"grid={grid} x 512 thr" in desc, desc
        for tok in case["tokens"]:
            assert tok in desc, (tok, desc)
        pl.set_v(V)
        pl.set_w(W0)
        pl.set_h(H0)
        pl.init()
        W, H = pl.get_w(), pl.get_h(np.float32)
        wn = np.sqrt((W0 ** 2).sum(0))
        np.testing.assert_allclose(W, W0 / wn, rtol=4 * 2.0 ** -52 * F)
        np.testing.assert_allclose(H, H0 * wn[:, None], rtol=4 * U)
        regs = mdi_regions(desc, F, T, r, mode)
        for name in case["expect"]:
            assert name in regs and len(regs[name][2]) > 0, (name, sorted(regs), desc)
        t_c = chain_t(desc, T)
        gram = "Gram matrix" in desc
        fixed = np.zeros(r, bool) if w_ind is None else ~w_ind
        stats = {"H": {}, "W": {}}
        Vt = mdi_start(V, M)
        iterates = []
        t_h = t_w = None

        def keep(m, st):
            for name, (worst, _ij, rms) in st.items():
                w0, r0 = stats[m].get(name, (0.0, 0.0))
                stats[m][name] = (max(w0, worst), max(r0, rms))

        for k in range(1, steps + 1):
            pl.run(1)
            Wk, Hk = pl.get_w(), pl.get_h(np.float32)
            t_h = tau_h_mdi(F, r, beta, k, mode, ones)
            t_w = tau_w_mdi(F, r, beta, t_c, k, mode, ones)
            if upd_h:
                Hr, info = ref_hstep(Vt, W, H, beta, S, exact_v=True)
                keep("H", compare(Hk, Hr, t_h, regs, "H", floors=info, what=f"{case['id']} step {k} H"))
            else:
                assert np.array_equal(Hk, H), f"step {k}: a W-only plan changed H"
            if upd_w:
                Wr, info = ref_wstep(Vt, W, Hk, beta, w_ind, gram=gram, exact_v=True)
                keep("W", compare(Wk, Wr, t_w, regs, "W", floors=info, what=f"{case['id']} step {k} W"))
                if fixed.any():
                    d = np.abs(Wk[:, fixed] - W[:, fixed])
                    assert (d <= 4 * U * W[:, fixed]).all(), f"step {k}: fixed columns moved by {float((d / W[:, fixed]).max()):.3e}"
            else:
                assert np.array_equal(Wk, W), f"step {k}: an H-only plan changed W"
            W, H = Wk, Hk
            Vt = mdi_impute(Vt, M, Wk, Hk)
            iterates.append((Wk, Hk, Vt))
        if case["cost_check"]:
            _div, cost, n = pl.get_objective()
            assert n == steps, (n, steps)
            for k, (Wk, Hk, Vk) in enumerate(iterates):
                c = mdi_cost(Vk, Wk, Hk, beta, S)
                vsum = float(Vk.sum()) if beta != 0.0 else float(F * T)
                print(f"{case['id']}: objective of iterate {k + 1}: device {cost[k]:.12g}, fp64 {c:.12g}, off by {abs(cost[k] - c) / abs(c):.2e}")
                assert abs(cost[k] - c) <= REL_COST * abs(c) + 2e-7 * vsum, (k + 1, cost[k], c)
        v_dev = pl.get_v_mdi(dtype)
        assert v_dev.dtype == dtype
        if dtype == np.float32:  # the fp32 getter returns the kernel's fp32 values, the fp64 getter their widening
            assert np.array_equal(v_dev, pl.get_v_mdi(np.float64).astype(np.float32))
        v_ref, _nt = mdi_final(Vt, M, W, H)
        t_v = tau_vmdi(r, steps, ones)
        worst, _ft, rms = compare_vmdi(v_dev, v_ref, V, M, t_v, what=f"{case['id']} v_MDI")
        if ones:
            assert np.array_equal(pl.get_v_mdi(np.float32), _f32_floor(V)), "a mask of ones: v_MDI is the floored input, bit for bit"
    finally:
        pl.close()
    return stats, (t_h, t_w), (worst, t_v, rms), desc


def _row(case_id, stats, taus, vm):
    def col(m, tau):
        if not stats[m]:
            return "-                        -"
        return f"{max(w for w, _ in stats[m].values()):.1e} / {tau:.1e}  {max(x for _, x in stats[m].values()):.1e}"
    return f"    {case_id:<26} {col('H', taus[0])}   {col('W', taus[1])}   {vm[0]:.1e} / {vm[1]:.1e}  {vm[2]:.1e}"


@pytest.mark.parametrize("case", MDI_CASES, ids=lambda c: c["id"])
def test_masked_step_elementwise(gpu_ctx, case):
    t0 = time.perf_counter()
    stats, taus, vm, _desc = run_case(gpu_ctx, case)
    print(_row(case["id"], stats, taus, vm))
    print(f"{case['id']}: {time.perf_counter() - t0:.2f} s")


def test_fp32_entry_points_end_to_end(gpu_ctx):
    """set_mask_f32 / set_v_f32 / get_v_mdi_f32: the same case through the fp32 doors, judged like the others; its fp32 v_MDI is the
    fp64 getter's, rounded."""
    case = next(c for c in MDI_CASES if c["id"] == "kl_sync_F422")
    run_case(gpu_ctx, case, dtype=np.float32)


# ---- the deferred-imputation state machine -------------------------------------------------------------------------------------

def _soft_problem(F=65, T=90, r=9, seed=0):
    V, W0, H0 = synth_problem(F, T, r)
    rs = np.random.RandomState(seed)
    M = (rs.rand(F, T) > 0.3).astype(np.float64)
    M = mask_image(np.clip(M * 0.8 + rs.rand(F, T) * 0.2, 0, 1))  # tests/test_mdi.problem(soft=True), on the fp32 grid
    return V.astype(np.float32), M, W0, H0.astype(np.float32)


def _plan(ctx, V, M, W0, H0, **kw):
    from se_snmf_nat_amd import Plan
    F, T = V.shape
    pl = Plan(ctx, F, T, W0.shape[1], **kw)
    pl.set_mask(M)
    pl.set_v(V)
    pl.set_w(W0)
    pl.set_h(H0)
    pl.init()
    return pl


def _outputs(pl):
    div, cost, n = pl.get_objective()
    return dict(h=pl.get_h(np.float32), w=pl.get_w(), div=div.copy(), cost=cost.copy(), n=n, v=pl.get_v_mdi(np.float32))


def _same(a, b, what, keys=("h", "w", "div", "cost", "n", "v")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def _early_stop_threshold(V, M, W0, H0, beta, sp):
    """conv_eps from the oracle's own cost history, and the stop iteration n.  The oracle's relative cost change never falls by the
    factor of four between two consecutive tests that a margin of two on either side of a threshold needs (checked over the
    divergences, sparsity weights, modes and soft masks of these shapes), except at the FIRST test, iteration 2, which has no
    test before it: the rule of test_gpu_frame_solvers.test_frame_solve_data_edges[stop_at_2].  n = 2 is not congruent 3 mod 4, so
    the run loop, which polls the flag after every fourth iteration, has issued iterations 3 (which raises the flag) and 4 (after
    it) before it reads it."""
    p = dict(cf="beta", beta=beta, sparsity_mdi=sp, conv_eps_mdi=0.0, max_iter=4, cost_check=1, init_w=W0, init_h=H0.astype(np.float64))
    c = oracle_mdi(V.astype(np.float64), M, p)[2]["cost"]
    e2 = abs(c[1] - c[0]) / c[0]
    eps = 2.0 * e2
    n = 2
    assert e2 < eps / 2 * (1 + 1e-12) and n % 4 != 3  # the margin, on the oracle's numbers (no test precedes iteration 2)
    return eps, n


@pytest.mark.parametrize("beta", [1.0, 2.0], ids=["kl", "ed"])
@pytest.mark.parametrize("into_max_iter", [False, True], ids=["beyond_the_stop", "into_max_iter"])
def test_soft_mask_early_stop_freezes_v(gpu_ctx, beta, into_max_iter):
    V, M, W0, H0 = _soft_problem()
    r, sp = W0.shape[1], 0.5
    eps, n = _early_stop_threshold(V, M, W0, H0, beta, sp)
    p = dict(cf="beta", beta=beta, sparsity_mdi=sp, conv_eps_mdi=eps, max_iter=40, cost_check=1, init_w=W0, init_h=H0.astype(np.float64))
    v_o, h_o, o = oracle_mdi(V.astype(np.float64), M, p)
    assert o["n_iter"] == n
    max_iter = n + 3 if into_max_iter else 40
    kw = dict(beta=beta, max_iter=max_iter, conv_eps=eps, cost_check=True, sparsity=sp)
    pl = _plan(gpu_ctx, V, M, W0, H0, **kw)
    try:
        W, H = pl.get_w(), pl.get_h(np.float32)
        Vt = mdi_start(V, M)
        states, flags = [], []
        for k in range(1, n + 4):  # the flag of iterate n rises while iteration n + 1 runs; three more calls after that
            pl.run(1)
            flags.append(pl.stopped())
            states.append((pl.get_w(), pl.get_h(np.float32)))
            if k <= n:
                Vt = mdi_impute(Vt, M, *states[-1])
        assert flags == [False] * n + [True] * 3, flags
        Wn, Hn = states[n - 1]
        for Wk, Hk in states[n:]:
            assert np.array_equal(Wk, Wn) and np.array_equal(Hk, Hn), "H or W moved after the stop"
        out = _outputs(pl)
        assert out["n"] == n and pl.run(1) == n
        np.testing.assert_allclose(out["cost"][:n], o["cost"], rtol=REL_COST, atol=2e-7 * float(V.sum()))
        v_ref, _nt = mdi_final(Vt, M, Wn, Hn)
        compare_vmdi(pl.get_v_mdi(), v_ref, V, M, tau_vmdi(r, n), what="v_MDI of the stop iterate")
        assert np.linalg.norm(out["h"] - h_o) / np.linalg.norm(h_o) < REL
        assert np.array_equal(out["h"], Hn) and np.array_equal(out["w"], Wn)
        _same(out, _outputs(pl), "a second read")
    finally:
        pl.close()
    one = _plan(gpu_ctx, V, M, W0, H0, **kw)
    try:
        assert one.run() == n and one.stopped()
        _same(out, _outputs(one), "one run() call against run(1) at a time")
    finally:
        one.close()


@pytest.mark.parametrize("cost_check", [True, False], ids=["cost", "nocost"])
@pytest.mark.parametrize("mode", ["full", "h", "w"])
def test_one_run_equals_single_steps(gpu_ctx, mode, cost_check):
    """run() and run(1) x n issue the same launches in the same order, the last re-imputation included (the final objective pass,
    or mdi_final's own pass without cost_check; the W-only plan's first Lam pass only where there is something to impute or to
    evaluate): every output bit for bit.  And nothing moves afterwards."""
    V, M, W0, H0 = _soft_problem(129, 200, 24, seed=3)
    w_ind, h_ind = case_masks(mode, 24)
    n = 6
    kw = dict(beta=1.0, max_iter=n, conv_eps=0.0, cost_check=cost_check, sparsity=0.5, w_update_ind=w_ind, h_update_ind=h_ind)
    a = _plan(gpu_ctx, V, M, W0, H0, **kw)
    b = _plan(gpu_ctx, V, M, W0, H0, **kw)
    try:
        assert a.run() == n
        for _k in range(n):
            b.run(1)
        oa, ob = _outputs(a), _outputs(b)
        _same(oa, ob, f"{mode}, cost_check={cost_check}: run() against run(1) x {n}")
        assert a.run() == n and a.run(1) == n  # nothing left to do
        _same(oa, _outputs(a), "run() after max_iter")
        _same(oa, _outputs(a), "get_v_mdi() twice")
        # ... and the value itself: the oracle's, as a trajectory (tests/test_mdi.py's tolerance)
        p = dict(cf="kl", sparsity_mdi=0.5, conv_eps_mdi=0.0, max_iter=n, cost_check=1, init_w=W0, init_h=H0.astype(np.float64))
        if w_ind is not None:
            p["w_update_ind"] = w_ind
        if h_ind is not None:
            p["h_update_ind"] = h_ind
        v_o, h_o, o = oracle_mdi(V.astype(np.float64), M, p)
        assert np.linalg.norm(oa["v"] - v_o) / np.linalg.norm(v_o) < REL
        assert np.linalg.norm(oa["h"] - h_o) / np.linalg.norm(h_o) < REL
        if cost_check:
            np.testing.assert_allclose(oa["cost"], o["cost"], rtol=REL_COST, atol=2e-7 * float(V.sum()))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape", [(65, 90, 9, "kl"), (257, 300, 40, "kl"), (64, 200, 20, "ed")], ids=lambda s: f"{s[0]}x{s[1]}-r{s[2]}-{s[3]}")
@pytest.mark.parametrize("soft", [False, True], ids=["01", "soft"])
def test_entirely_missing_and_entirely_observed_frames_and_rows(gpu_ctx, shape, soft):
    from se_snmf_nat_amd import snmf_mdi, snmf_mdi_Sm
    F, T, r, cf = shape
    V, W0, H0 = synth_problem(F, T, r)
    rs = np.random.RandomState(4)
    M = (rs.rand(F, T) > 0.3).astype(np.float64)
    if soft:
        M = np.clip(M * 0.8 + rs.rand(F, T) * 0.2, 0, 1)
    gone_t, full_t, gone_f, full_f = [3, 31, 32, T - 1], [0, 40, T - 2], [5, F - 1], [0, F - 2]
    M[gone_f, :] = 0.0
    M[full_f, :] = 1.0
    M[:, full_t] = 1.0
    M[:, gone_t] = 0.0
    M = mask_image(M)
    p = dict(cf=cf, sparsity_mdi=0.5, conv_eps_mdi=0, max_iter=8, cost_check=1, init_w=W0, init_h=H0)
    v_ref, h_ref, o_ref = oracle_mdi(V, M, p)
    v_dev, h_dev, o_dev = (snmf_mdi_Sm if soft else snmf_mdi)(V, M, p, ctx=gpu_ctx)
    assert np.isfinite(v_dev).all() and np.isfinite(h_dev).all() and np.isfinite(o_dev["cost"]).all()
    assert o_dev["n_iter"] == o_ref["n_iter"] == 8
    assert np.linalg.norm(h_dev - h_ref) / np.linalg.norm(h_ref) < REL
    assert np.linalg.norm(v_dev - v_ref) / np.linalg.norm(v_ref) < REL
    np.testing.assert_allclose(o_dev["cost"], o_ref["cost"], rtol=REL_COST, atol=2e-7 * V.sum())
    # the exact facts: the floor in an entirely missing frame (Nt = 0 / max(0, flr)), the input in an entirely observed one and row
    assert (v_ref[:, gone_t] == FLR).all() and np.array_equal(v_ref[:, full_t], np.fmax(V, FLR)[:, full_t])
    assert np.array_equal(v_dev[:, gone_t].astype(np.float32), np.full((F, len(gone_t)), np.float32(FLR)))
    assert np.array_equal(v_dev[:, full_t].astype(np.float32), _f32_floor(V)[:, full_t])
    keep = np.setdiff1d(np.arange(T), gone_t)
    assert np.array_equal(v_dev[np.ix_(full_f, keep)].astype(np.float32), _f32_floor(V)[np.ix_(full_f, keep)])
