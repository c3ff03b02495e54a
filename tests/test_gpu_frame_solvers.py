"""Per-frame H-only solvers (the online call, src/bnmf_sep_event_RT_IS16.m:138-154 -> src/sparse_nmf.m:186-286 with
w_update_ind = 0) through the plan, against the fp64 oracle (oracle/sparse_nmf_oracle.py).

Two persistent kernels run these solves (snmf_api.hip: the plan's small_ok / frame_fb, snmf_tu_small.hip: launch_small):
  k_hsolve_frame<FB, KB, BM, OBJ>  T = 1, dictionary in registers: FB in {4, 8} from F <= 64*FB + 1 (F = 64*FB + 1 adds
                                   the extra row xr), KB in {16, 25} from r <= 8*KB
  k_hsolve_small<BM, OBJ>          T <= 32, H in LDS, while the LDS images fit (snmf_api.hip, `need <= lds_cap`)
and everything else takes the per-iteration plan loop.  The covering array below launches every (FB, KB) x BM x OBJ
instantiation of k_hsolve_frame, each at an edge F and an edge r, and the cases beside it pin the sparsity forms, the
data edges, the SNMF_NO_SMALL switches, both sides of k_hsolve_small's LDS bound and Plan.solve_frames.

Tolerances: the stop index exactly; W, H and the objective with tests/test_gpu_parity.py's check (REL_WH 1e-4,
REL_COST 1e-5); and a per-component bound max|h - h_ref| <= C_H * max|h_ref|, which a whole-vector Frobenius check
would dilute when the error sits in one activation (C_H = 8e-5: 4x the worst measured, 2.0e-5).
"""
import numpy as np
import pytest

from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem
from test_gpu_parity import REL_COST, REL_WH, check, rel

pytestmark = pytest.mark.gpu

# worst measured on an MI355X over the covering array: 2.0e-5 (F = 300, r = 201, Euclidean, 80 un-stopped iterations:
# k_hsolve_small); every other case below 8.4e-6
C_H = 8e-5

# BM of the kernels: (cf, beta) of src/sparse_nmf.m:95-110
BMS = {"kl": ("kl", 1.0), "ed": ("ed", 2.0), "is": ("is", 0.0), "b05": ("beta", 0.5), "b15": ("beta", 1.5)}
EDGE_F = {4: (5, 64, 65, 256, 257), 8: (258, 512, 513)}
EDGE_R = {16: (1, 2, 17, 127, 128), 25: (129, 199, 200)}


# (F, r, BM, OBJ, seed): every (FB, KB) x BM x OBJ of k_hsolve_frame once, F and r walking the edge lists above so that
# every edge of a (FB, KB) pair is met.  The seed of synth_problem is the first one (from F + 7 r up) on which the oracle's
# cost is monotone and its relative change never within 5 % of conv_eps (tests/fuzz_cases.py's borderline rule, widened).
FRAME_CASES = [
    # FB = 4, KB = 16
    (5, 1, 'kl', True, 12),  # oracle stops at 7
    (64, 2, 'kl', False, 78),
    (65, 17, 'ed', True, 233),  # oracle stops at 46
    (256, 127, 'ed', False, 1145),
    (257, 128, 'is', True, 1153),  # oracle stops at 5
    (5, 2, 'is', False, 19),
    (64, 17, 'b05', True, 232),  # oracle stops at 45
    (65, 127, 'b05', False, 954),
    (256, 128, 'b15', True, 1152),  # oracle stops at 80
    (257, 1, 'b15', False, 264),
    # FB = 4, KB = 25
    (5, 129, 'kl', True, 957),  # oracle stops at 25
    (64, 199, 'kl', False, 1457),
    (65, 200, 'ed', True, 1465),  # oracle stops at 80
    (256, 129, 'ed', False, 1159),
    (257, 199, 'is', True, 1650),  # oracle stops at 5
    (5, 129, 'is', False, 908),
    (64, 199, 'b05', True, 1457),  # oracle stops at 4
    (65, 200, 'b05', False, 1465),
    (256, 129, 'b15', True, 1159),  # oracle stops at 80
    (257, 199, 'b15', False, 1650),
    # FB = 8, KB = 16
    (258, 1, 'kl', True, 265),  # oracle stops at 2
    (512, 2, 'kl', False, 526),
    (513, 17, 'ed', True, 632),  # oracle stops at 2
    (258, 128, 'ed', False, 1154),
    (512, 1, 'is', True, 519),  # oracle stops at 2
    (513, 2, 'is', False, 527),
    (258, 127, 'b05', True, 1147),  # oracle stops at 3
    (512, 128, 'b05', False, 1408),
    (513, 1, 'b15', True, 520),  # oracle stops at 2
    (258, 17, 'b15', False, 377),
    # FB = 8, KB = 25
    (258, 129, 'kl', True, 1184),  # oracle stops at 2
    (512, 199, 'kl', False, 1905),
    (513, 200, 'ed', True, 1915),  # oracle stops at 80
    (258, 199, 'ed', False, 1651),
    (512, 200, 'is', True, 1912),  # oracle stops at 5
    (513, 129, 'is', False, 1416),
    (258, 200, 'b05', True, 1658),  # oracle stops at 3
    (512, 129, 'b05', False, 1415),
    (513, 199, 'b15', True, 1920),  # oracle stops at 2
    (258, 129, 'b15', False, 1161),
    # just outside k_hsolve_frame: F = 514 and r = 201 take k_hsolve_small at T = 1
    (514, 100, 'kl', True, 1214),  # oracle stops at 2
    (300, 201, 'kl', True, 1707),  # oracle stops at 2
    (514, 100, 'ed', True, 1232),  # oracle stops at 2
    (300, 201, 'ed', True, 1707),  # oracle stops at 80
    (514, 100, 'is', True, 1214),  # oracle stops at 4
    (300, 201, 'is', True, 1709),  # oracle stops at 5
]


def _params(F, r, bm, obj, *, seed=0, sparsity=0.5, max_iter=None, conv_eps=1e-3, T=1):
    V, W0, H0 = synth_problem(F, T, r, seed_data=seed, seed_init=seed + 1)
    cf, beta = BMS[bm]
    p = dict(cf=cf, beta=beta, sparsity=sparsity, init_w=W0, init_h=H0, w_update_ind=np.zeros(r, bool))
    if obj:
        p.update(cost_check=1, conv_eps=conv_eps, max_iter=max_iter or 80)
    else:
        p.update(cost_check=0, conv_eps=0.0, max_iter=max_iter or 12)
    return V, p


def BMS_BETA(p):
    return {"kl": 1.0, "ed": 2.0, "is": 0.0}.get(p["cf"], p.get("beta"))


def h_ratio(h, hr):
    """max|h - h_ref| / max|h_ref|: the per-component error."""
    return float(np.max(np.abs(h - hr)) / max(np.max(np.abs(hr)), 1e-300))


def _check_solve(res, ref, V, p):
    """Stop index, W / H / objective (test_gpu_parity.check) and the per-component bound on H.  The objective's absolute
    floor is test_gpu_parity's ABS_DIV on the floored V (src/sparse_nmf.m:169); Itakura-Saito terms are scale-free (each
    cancels from O(1)), so there the floor is eps_f32 per bin."""
    obj = bool(p["cost_check"])
    vsum = float(np.fmax(V, 1e-9).sum()) if BMS_BETA(p) != 0.0 else float(V.shape[0] * V.shape[1])
    check(res, ref, cost=obj, vsum=vsum)
    assert h_ratio(res[1], ref[1]) <= C_H, h_ratio(res[1], ref[1])


def run_frame_case(ctx, case):
    from se_snmf_nat_amd import sparse_nmf
    F, r, bm, obj, seed = case
    V, p = _params(F, r, bm, obj, seed=seed)
    return V, p, sparse_nmf(V, p, ctx=ctx), oracle_nmf(V, p)


@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: f"F{c[0]}-r{c[1]}-{c[2]}-{'obj' if c[3] else 'noobj'}")
def test_frame_solve_covering_array(gpu_ctx, case):
    """k_hsolve_frame<FB, KB, BM, OBJ> (snmf_kernels.h) at every register-block geometry x divergence x objective mode,
    each at an edge of F (64*FB, 64*FB + 1 with the extra row xr, the first F of FB = 8) and of r (1, 8*KB, the first
    rank of KB = 25), and the first shapes past it; src/sparse_nmf.m:189-208 (the H update of each beta, the generic
    one with lam.^(beta-2) through den.^2 at beta = 0), :257-284 (objective and stop test)."""
    V, p, res, ref = run_frame_case(gpu_ctx, case)
    _check_solve(res, ref, V, p)


def _full_sparsity_form(sp, r, n, dtype):
    """the r x n matrix form of p.sparsity kept as a matrix also at n = 1 (api._sparsity_form reads an r x 1 array as
    the column form: the same numbers, a different kernel operand)."""
    a = np.asarray(sp, dtype=dtype)
    if a.size == 1:
        return 0, float(a.reshape(-1)[0]), None
    return 2, 0.0, np.asfortranarray(a.reshape(r, n))


@pytest.mark.parametrize("shape", [(257, 100, "kl"), (513, 200, "b05"), (65, 17, "ed")], ids=lambda s: f"F{s[0]}-r{s[1]}-{s[2]}")
def test_frame_solve_sparsity_forms(gpu_ctx, shape, monkeypatch):
    """p.sparsity as a scalar, an r x 1 column and a full r x n matrix (src/sparse_nmf.m:150-155) in k_hsolve_frame: the
    scalar and the column reach the kernel as lamk, the matrix as a.S re-based by the frame's column (a.S += c0 * rp)."""
    from se_snmf_nat_amd import api, sparse_nmf
    F, r, bm = shape
    rs = np.random.RandomState(F + r)
    forms = [("scalar", 2.0), ("column", rs.random_sample((r, 1)) * 4), ("matrix", rs.random_sample((r, 1)) * 3)]
    for name, sp in forms:
        V, p = _params(F, r, bm, True, seed=F, sparsity=sp, conv_eps=0.0, max_iter=25)
        if name == "matrix":
            monkeypatch.setattr(api, "_sparsity_form", _full_sparsity_form)
        res = sparse_nmf(V, p, ctx=gpu_ctx)
        monkeypatch.undo()
        _check_solve(res, oracle_nmf(V, p), V, p)


def _edge_frame(kind, F):
    V, _, _ = synth_problem(F, 1, 12, seed_data=F)
    if kind == "silent":
        return np.zeros((F, 1))  # every bin at the floor of src/sparse_nmf.m:169
    if kind == "range1e6":
        return V / V.max() * np.logspace(0, 6, F)[:, None] * 1e-3  # 1e-9 .. 1e3 across the bins (times the frame's shape)
    return V


@pytest.mark.parametrize("shape", [(513, 200, "kl"), (257, 40, "is"), (130, 150, "ed")], ids=lambda s: f"F{s[0]}-r{s[1]}-{s[2]}")
@pytest.mark.parametrize("kind", ["silent", "range1e6", "stop_at_2", "to_max_iter"])
def test_frame_solve_data_edges(gpu_ctx, shape, kind):
    """Data edges of the one-frame solve: an all-zero frame (V floored to 1e-9, src/sparse_nmf.m:169), a frame spanning
    six decades, a frame whose solve stops at the first possible test (iteration 2, :272-284) and one that runs to
    max_iter with the test armed."""
    from se_snmf_nat_amd import sparse_nmf
    F, r, bm = shape
    _, W0, H0 = synth_problem(F, 1, r, seed_data=1, seed_init=F)
    cf, beta = BMS[bm]
    V = _edge_frame(kind, F)
    p = dict(cf=cf, beta=beta, sparsity=0.5, init_w=W0, init_h=H0, w_update_ind=np.zeros(r, bool), cost_check=1,
             conv_eps=1e-3, max_iter=60)
    if kind == "stop_at_2":
        c = oracle_nmf(V, dict(p, conv_eps=0.0, max_iter=3))[2]["cost"]
        p["conv_eps"] = 2.0 * abs(c[1] - c[0]) / c[0]  # the first test (iteration 2) passes by a factor of two
    elif kind == "to_max_iter":
        p.update(conv_eps=1e-12, max_iter=40)
    elif kind == "range1e6":
        p.update(conv_eps=0.0, max_iter=30)  # (the range is the point here, not the stop)
    ref = oracle_nmf(V, p)
    if kind == "stop_at_2":
        assert ref[2]["n_iter"] == 2
    elif kind == "to_max_iter":
        assert ref[2]["n_iter"] == 40
    _check_solve(sparse_nmf(V, p, ctx=gpu_ctx), ref, V, p)


@pytest.mark.parametrize("case", [(513, 200, "kl", 5), (257, 128, "is", 6), (65, 17, "b05", 9), (512, 129, "ed", 12), (129, 64, "b15", 9)],
                         ids=lambda c: f"F{c[0]}-r{c[1]}-{c[2]}")
def test_frame_kernel_equals_the_lds_kernel_and_the_plan_loop(gpu_ctx, case, monkeypatch):
    """The same T = 1 solve through k_hsolve_frame (default), k_hsolve_small (SNMF_NO_SMALL=2) and the per-iteration
    plan loop (SNMF_NO_SMALL=1): each matches the oracle, and the two others match the frame kernel to 1e-5 with the
    same stop index (src/sparse_nmf.m:186-286 is one algorithm, whichever kernel runs it)."""
    from se_snmf_nat_amd import sparse_nmf
    F, r, bm, seed = case
    # (the Euclidean case stops at 25: un-stopped ED iterations drift apart by ~1e-5 per 50, like fp32 against fp64)
    V, p = _params(F, r, bm, True, seed=seed, max_iter=25 if bm == "ed" else 60)
    ref = oracle_nmf(V, p)
    out = {}
    for mode in ("0", "2", "1"):
        monkeypatch.setenv("SNMF_NO_SMALL", mode)
        out[mode] = sparse_nmf(V, p, ctx=gpu_ctx)
        _check_solve(out[mode], ref, V, p)
    monkeypatch.delenv("SNMF_NO_SMALL")
    for mode in ("2", "1"):
        assert out[mode][2]["n_iter"] == out["0"][2]["n_iter"]
        assert rel(out[mode][1], out["0"][1]) < 1e-5


def small_lds_need(F, r):
    """LDS bytes of k_hsolve_small for an F x T (T <= 32) H-only plan: the `need` of snmf_api.hip's persistent-path block
    (32 * (ldh + ldr) + rp rounded to 4) floats + 2 x 512 doubles, with the plan's row geometry (snmf_api.hip: xr, nf, Fq,
    rp, ldh, ldr).  Mirrored here so that the cases below sit on either side of the bound."""
    xr = 1 if (F % 32 == 1 and F > 32) else 0
    nf = F // 32 if xr else (F + 31) // 32
    Fq = 32 * nf + 8 * xr
    rp = (r + 31) // 32 * 32
    ldh, ldr = rp + 4, Fq + 4
    return (32 * (ldh + ldr) + ((rp + 3) & ~3)) * 4 + 2 * 512 * 8


LDS_CAP = 160 * 1024
# (inside, outside) pairs: across the bound by one row at r = 128 (F = 1057 has the extra row) and by one rank at F = 1024
LDS_EDGES = {"F": ((1057, 128), (1058, 128)), "r": ((1024, 160), (1024, 161))}


@pytest.mark.parametrize("T", [2, 7, 31, 32])
@pytest.mark.parametrize("bm", ["kl", "ed", "b15", "b05"])
def test_small_kernel_lds_bound(gpu_ctx, T, bm):
    """k_hsolve_small<BM, OBJ> (snmf_kernels.h) for 1 < T <= 32 right at its LDS envelope: the shape just inside runs
    in the persistent kernel, the one just outside in the plan loop; both must match the oracle
    (src/sparse_nmf.m:186-286, H-only)."""
    from se_snmf_nat_amd import sparse_nmf
    edge = "F" if T in (2, 31) else "r"
    inside, outside = LDS_EDGES[edge]
    assert small_lds_need(*inside) <= LDS_CAP < small_lds_need(*outside)
    for F, r in (inside, outside):
        V, p = _params(F, r, bm, True, seed=T, T=T, conv_eps=0.0, max_iter=12)
        _check_solve(sparse_nmf(V, p, ctx=gpu_ctx), oracle_nmf(V, p), V, p)


SOLVE_FRAMES_GEOMETRIES = [(257, 100, "kl", 21), (512, 150, "b15", 22)]  # FB = 4 (with xr), KB = 16; FB = 8, KB = 25


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("geo", SOLVE_FRAMES_GEOMETRIES, ids=lambda g: f"F{g[0]}-r{g[1]}-{g[2]}")
def test_solve_frames_equals_independent_calls(gpu_ctx, geo, dtype):
    """Plan.solve_frames (snmf_plan_solve_frames_*: one persistent workgroup per solve, k_hsolve_frame at one frame per
    solve, k_hsolve_small above) with 1, 2, 7 and 32 frames per solve and up to 300 solves in one launch (more than the
    CUs): every solve equals the independent sparse_nmf call on its columns bit for bit (the reference re-seeds and
    re-normalises per call, src/sparse_nmf.m:112-114,:157-160), and a sample matches the oracle."""
    from se_snmf_nat_amd import Plan, sparse_nmf
    F, r, bm, seed = geo
    cf, beta = BMS[bm]
    n_distinct = 10
    plan = Plan(gpu_ctx, F, 600, r, beta=beta, max_iter=60, conv_eps=1e-3, cost_check=True, sparsity=0.5,
                w_update_ind=np.zeros(r, bool))
    _, W, _ = synth_problem(F, 1, r, seed_data=seed, seed_init=seed)
    W = W.astype(np.float32).astype(np.float64)  # the same dictionary bits whichever dtype the solves take
    plan.set_w(W)
    for tps, n in ((1, 300), (2, 300), (7, 40), (32, 12)):
        Vd, _, _ = synth_problem(F, n_distinct * tps, r, seed_data=seed + tps, r_true=12)
        H0 = np.random.RandomState(tps).random_sample((r, tps))
        blocks = [Vd[:, j * tps:(j + 1) * tps] for j in range(n_distinct)]
        Vall = np.concatenate([blocks[j % n_distinct] for j in range(n)], axis=1)
        Hs, nit, lc = plan.solve_frames(Vall, H0, dtype=dtype)
        p = dict(cf=cf, beta=beta, sparsity=0.5, max_iter=60, conv_eps=1e-3, init_w=W, init_h=H0, cost_check=1,
                 w_update_ind=np.zeros(r, bool))
        singles = [sparse_nmf(b, p, ctx=gpu_ctx, dtype=dtype) for b in blocks]
        for j in range(n):
            _, h1, o1 = singles[j % n_distinct]
            assert nit[j] == o1["n_iter"] and lc[j] == o1["cost"][-1]
            assert np.array_equal(Hs[:, j * tps:(j + 1) * tps], h1)
        if dtype == np.float64:
            # the three distinct blocks whose oracle stop decision is clearest (largest distance of the relative cost
            # change from conv_eps over the solve): a decision within fp32 rounding of the threshold is no finding
            refs = [oracle_nmf(b, p) for b in blocks]
            margin = [np.min(np.abs(np.abs(np.diff(o["cost"])) / o["cost"][:-1] - 1e-3)) for _, _, o in refs]
            for j in np.argsort(margin)[-3:]:
                _, hr, orf = refs[j]
                h = Hs[:, j * tps:(j + 1) * tps]
                assert nit[j] == orf["n_iter"]
                assert rel(h, hr) < REL_WH and h_ratio(h, hr) <= C_H
                assert abs(lc[j] - orf["cost"][-1]) <= REL_COST * orf["cost"][-1]
