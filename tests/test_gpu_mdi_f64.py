"""The fp64 mode of the missing-data solves (snmf_mdi / snmf_mdi_Sm with precision="fp64" -> snmf_mdi_fp64: the kernels of
the fp64 solve mode plus the masked start, the re-imputation fused with the objective and the gain-matched final imputation,
csrc/snmf_solve64.h) against oracle/mdi_oracle.py, judged the way tests/test_gpu_solve_f64.py judges the plain solve.

Inputs: synth_problem values rounded to fp32 and held as doubles; the mask is RandomState(0).rand(F, T) > 0.3, the soft mask
clip(0.8 M + 0.2 rand, 0, 1).

Bounds (not measured on the code under test: they come from the oracle's own sensitivity).  On the cases below the oracle's
results move by at most 2.1e-13 in relative Frobenius norm (V_mdi, H, W) and by at most 2.8e-14 in cost when V, W0 and H0
are each perturbed by a relative 1e-13 (three draws); n_iter is unchanged on every case.  So, as for the plain fp64 solve,
    REL_WH   = 1e-11   relative Frobenius error of V_mdi, of H and of W          (>= 47 x that response)
    REL_COST = 1e-12   relative error of EVERY div and cost entry                 (>= 35 x)
    n_iter           equal (the oracle's |dcost|/cost stays >= 1 % of conv_eps away from conv_eps at its stop and before it:
                     1.1 % on kl_65x90_r9_stop, which stops at 43, and 9 % on kl_65x4500_r20_stop, which stops at 10)
The fp32 path sits between 1e-7 and 1e-6 on the cases it takes: a fall-back to it cannot pass.

Where the kernels can go wrong: T = 4500 = 2 L + 404 (L = kS64ChunkK = 2048) gives two whole splits and a ragged third in the
T contractions and 1125 workgroups of the final imputation (a wave per frame); F = 2600 splits the W' * R contraction and
gives every lane of the final imputation 40 rows and a ragged 41st; 2700 x 64, r = 8 is the shape
tests/test_gpu_generic.py::test_mdi_still_refuses_out_of_envelope_shapes shows the fp32 path refusing; 1 x 50 has frames
without an observed entry (Nt = 0: the missing entries are the floor); 64 x 4096, r = 64 is a multiple of every tile dimension.

Measured on an MI355X (max over the cases of each group; every case prints its own line):
    65 x 90, r = 9 (9 cases)    relV <= 3.7e-16  relH <= 1.2e-15  relW <= 1.5e-15  reldiv <= 5.6e-16  relcost <= 3.7e-16   n_iter equal in all
    the 11 larger / edge cases   relV <= 6.9e-16  relH <= 3.4e-15  relW <= 3.3e-15  reldiv <= 2.9e-15  relcost <= 2.2e-15   n_iter equal in all
    full mask (KL stop, ED)     H, W, div, cost, n_iter and V_mdi equal to the plain fp64 solve's, bit for bit
    dnmf_adapt in fp64          relB_a = 2.2e-15 against the oracle's two solves
    fp32 on kl_65x90_r9         relV = 7.3e-08 (four orders of magnitude above the bound)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from mexhost import MexError, mex_shims  # noqa: F401  (session fixture)
from oracle.mdi_oracle import snmf_mdi as oracle_mdi
from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem

pytestmark = pytest.mark.gpu
REL_WH = 1e-11
REL_COST = 1e-12
FLR = 1e-9


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    nz = b != 0
    if (a[~nz] != 0).any():  # (the zero vectors of cost_check = 0 must be zeros)
        return float("inf")
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def bits(a):
    return np.asfortranarray(a).tobytes(order="F")


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(V, W0, H0, binary mask, soft mask) of a shape, read-only."""
    F, T, r = shape
    V, W0, H0 = (f32r(a) for a in synth_problem(F, T, r))
    rs = np.random.RandomState(0)
    M = (rs.rand(F, T) > 0.3).astype(np.float64)
    Ms = np.clip(M * 0.8 + rs.rand(F, T) * 0.2, 0, 1)
    for a in (V, W0, H0, M, Ms):
        a.setflags(write=False)
    return V, W0, H0, M, Ms


def _cases():
    """name -> (shape, p, soft)"""
    c = {}
    kl = dict(cf="kl", sparsity_mdi=0.5, conv_eps_mdi=0, cost_check=1)
    s = (65, 90, 9)
    c["kl_65x90_r9"] = (s, dict(kl, max_iter=25), False)
    c["kl_65x90_r9_stop"] = (s, dict(kl, sparsity_mdi=5, conv_eps_mdi=1e-3, max_iter=100), False)
    c["kl_65x90_r9_soft"] = (s, dict(kl, max_iter=25), True)
    c["ed_65x90_r9"] = (s, dict(kl, cf="ed", max_iter=25), False)
    c["is_65x90_r9"] = (s, dict(kl, cf="is", sparsity_mdi=0.1, max_iter=25), False)
    c["kl_65x90_r9_honly"] = (s, dict(kl, max_iter=25, w_update_ind=np.zeros(9, bool)), False)
    c["kl_65x90_r9_wonly"] = (s, dict(kl, max_iter=25, h_update_ind=np.zeros(9, bool)), False)
    c["kl_65x90_r9_nocheck"] = (s, dict(kl, max_iter=25, conv_eps_mdi=1e-3, cost_check=0), False)
    c["kl_65x90_r9_neither"] = (s, dict(kl, max_iter=5, w_update_ind=np.zeros(9, bool), h_update_ind=np.zeros(9, bool)), False)
    s = (65, 4500, 20)
    c["kl_65x4500_r20"] = (s, dict(kl, max_iter=20), False)
    c["kl_65x4500_r20_stop"] = (s, dict(kl, sparsity_mdi=5, conv_eps_mdi=1e-3, max_iter=100), False)
    s = (97, 2100, 33)
    c["b15_97x2100_r33_soft_semi"] = (s, dict(kl, cf="beta", beta=1.5, sparsity_mdi=1, max_iter=20, w_update_ind=np.arange(33) >= 17), True)
    c["ed_97x2100_r33"] = (s, dict(kl, cf="ed", sparsity_mdi=2, max_iter=20), False)
    rs = np.random.RandomState(3)
    c["kl_97x2100_r33_rvec"] = (s, dict(kl, sparsity_mdi=0.5 + 5 * rs.random_sample(33), max_iter=15), False)
    c["b15_97x2100_r33_full_sparsity"] = (s, dict(kl, cf="beta", beta=1.5, sparsity_mdi=2 * rs.random_sample((33, 2100)), max_iter=15), True)
    c["kl_2600x130_r20"] = ((2600, 130, 20), dict(kl, max_iter=15), False)
    c["kl_2700x64_r8"] = ((2700, 64, 8), dict(kl, max_iter=10), False)
    c["kl_1x50_r3"] = ((1, 50, 3), dict(kl, max_iter=10), False)
    c["kl_17x15_r1"] = ((17, 15, 1), dict(kl, max_iter=10), False)
    c["kl_64x4096_r64_tiles"] = ((64, 4096, 64), dict(kl, max_iter=10), False)
    return c


CASES = _cases()
# the stop iterations of the two early-stop cases (the oracle's; the margins to conv_eps are in the docstring)
STOPS = {"kl_65x90_r9_stop": 43, "kl_65x4500_r20_stop": 10}


def _args(name):
    shape, p, soft = CASES[name]
    V, W0, H0, M, Ms = problem(shape)
    return V, (Ms if soft else M), dict(p, init_w=W0, init_h=H0), soft


@functools.lru_cache(maxsize=None)
def oracle(name):
    V, M, p, _ = _args(name)
    v, h, o = oracle_mdi(V, M, p)
    return v, h, o["w"], o["div"], o["cost"], o["n_iter"]


def device(name, ctx, **kw):
    from se_snmf_nat_amd import snmf_mdi, snmf_mdi_Sm
    V, M, p, soft = _args(name)
    info = {}
    v, h, o = (snmf_mdi_Sm if soft else snmf_mdi)(V, M, p, ctx=ctx, precision="fp64", info=info, **kw)
    return v, h, o, info["w"]


def judge(name, res, ref):
    """Print the measured errors, then assert the bounds."""
    v, h, o, w = res
    vr, hr, wr, divr, costr, nr = ref
    ev, eh, ew = rel(v, vr), rel(h, hr), rel(w, wr)
    same_len = len(o["div"]) == len(divr) and len(o["cost"]) == len(costr)
    ed = relmax(o["div"], divr) if same_len else float("inf")
    ec = relmax(o["cost"], costr) if same_len else float("inf")
    print(f"fp64 mdi {name}: n_iter={o['n_iter']} (oracle {nr}) relV={ev:.2e} relH={eh:.2e} relW={ew:.2e} reldiv={ed:.2e} relcost={ec:.2e}")
    assert o["n_iter"] == nr
    assert same_len
    assert np.isfinite(v).all() and np.isfinite(h).all() and np.isfinite(w).all()
    assert ev < REL_WH, ev
    assert eh < REL_WH, eh
    assert ew < REL_WH, ew
    assert ed < REL_COST, ed
    assert ec < REL_COST, ec


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_mdi_in_fp64(gpu_ctx, name):
    res, ref = device(name, gpu_ctx), oracle(name)
    judge(name, res, ref)
    v, h, o, w = res
    assert v.min() >= FLR
    if name in STOPS:
        assert ref[5] == STOPS[name] and len(o["cost"]) == STOPS[name]
    if name.endswith("nocheck"):  # cost_check = 0: zero vectors and no stop, the imputation runs all the same
        assert not o["div"].any() and not o["cost"].any() and len(o["cost"]) == 25 and o["n_iter"] == 25
    if name == "kl_1x50_r3":  # frames without an observed entry: Nt = 0 and the entry is the floor
        M = _args(name)[1]
        assert (M[0] == 0).sum() >= 5 and (v[0, M[0] == 0] == FLR).all() and (v[0, M[0] == 1] > FLR).all()


def test_neither_factor_updated_solves_in_fp64_and_is_refused_in_fp32(gpu_ctx):
    from se_snmf_nat_amd import SnmfError, snmf_mdi
    name = "kl_65x90_r9_neither"
    V, M, p, _ = _args(name)
    v, h, o, w = device(name, gpu_ctx)
    judge(name, (v, h, o, w), oracle(name))
    assert rel(h, p["init_h"] * np.sqrt((p["init_w"] ** 2).sum(0))[:, None]) < 1e-15  # (only the initial scaling touched it)
    with pytest.raises(SnmfError):
        snmf_mdi(V, M, p, ctx=gpu_ctx)


def test_the_out_of_envelope_shape_is_still_refused_in_fp32(gpu_ctx):
    from se_snmf_nat_amd import SnmfError, snmf_mdi
    V, M, p, _ = _args("kl_2700x64_r8")
    with pytest.raises(SnmfError, match="too large"):
        snmf_mdi(V, M, p, ctx=gpu_ctx)


# ---- 2. identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [dict(cf="kl", sparsity=5, conv_eps=1e-3, max_iter=100), dict(cf="ed", sparsity=2, conv_eps=0, max_iter=20)],
                         ids=["kl_stop", "ed"])
def test_full_mask_is_the_plain_fp64_solve_bit_for_bit(gpu_ctx, p):
    """v * 1 + lam * 0 = v exactly, so M == 1 leaves V alone and the fused kernel must sum what k_s64_obj sums, in its order."""
    from se_snmf_nat_amd import snmf_mdi, sparse_nmf
    V, W0, H0, _, _ = problem((65, 4500, 20))
    p = dict(p, init_w=W0, init_h=H0, cost_check=1)
    w, h, o = sparse_nmf(V, p, ctx=gpu_ctx, precision="fp64")
    pm = dict(p, sparsity_mdi=p["sparsity"], conv_eps_mdi=p["conv_eps"])
    info = {}
    vm, hm, om = snmf_mdi(V, np.ones_like(V), pm, ctx=gpu_ctx, precision="fp64", info=info)
    print(f"full mask: n_iter {om['n_iter']} / {o['n_iter']}, max |dH| = {np.abs(hm - h).max():.1e}, "
          f"max |dcost| = {np.abs(om['cost'] - o['cost']).max() if len(om['cost']) == len(o['cost']) else -1:.1e}")
    assert om["n_iter"] == o["n_iter"] and (p["conv_eps"] == 0 or o["n_iter"] < 100)
    assert np.array_equal(hm, h) and np.array_equal(info["w"], w)
    assert np.array_equal(om["div"], o["div"]) and np.array_equal(om["cost"], o["cost"])
    assert np.array_equal(vm, np.maximum(V, FLR))


def test_observed_entries_are_the_inputs_bits(gpu_ctx):
    for name in ("kl_65x90_r9", "kl_65x4500_r20_stop", "kl_2600x130_r20"):
        V, M, _, _ = _args(name)
        v = device(name, gpu_ctx)[0]
        assert np.array_equal(v[M == 1], np.maximum(V, FLR)[M == 1]), name


@pytest.mark.parametrize("name", ["kl_65x4500_r20", "b15_97x2100_r33_soft_semi", "kl_2600x130_r20"])
def test_two_runs_give_the_same_bits(gpu_ctx, name):
    v1, h1, o1, w1 = device(name, gpu_ctx)
    v2, h2, o2, w2 = device(name, gpu_ctx)
    assert bits(v1) == bits(v2) and bits(h1) == bits(h2) and bits(w1) == bits(w2)
    assert bits(o1["div"]) == bits(o2["div"]) and bits(o1["cost"]) == bits(o2["cost"])


# ---- 3. argument rules -------------------------------------------------------------------------------------------------
def test_argument_rules_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import SnmfError, snmf_mdi
    from se_snmf_nat_amd.api import _make_params
    name = "kl_65x90_r9"
    V, M, p, _ = _args(name)
    before = snmf_mdi(V, M, p, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="precision"):
        snmf_mdi(V, M, p, ctx=gpu_ctx, precision="fp16")
    with pytest.raises(SnmfError) as e:
        snmf_mdi(V, M, p, ctx=gpu_ctx, precision="fp64", dtype=np.float32)
    assert e.value.status == 1
    # the raw entry: NULL V_mdi, NULL M, ldM < F
    F, T, r = CASES[name][0]
    sp = _make_params(F, T, r, 1.0, 3, 0.0, 1, 1, 0, 0.5, None, None)
    Vf, Mf, W0, H0 = (np.asfortranarray(a) for a in (V, M, p["init_w"], p["init_h"]))
    vm, H = np.empty((F, T), order="F"), np.empty((r, T), order="F")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    call = lambda m, ldm, out: lib.snmf_mdi_fp64(gpu_ctx._h, C.byref(sp), ptr(Vf), F, m, ldm, ptr(W0), ptr(H0), None, out, F, None,  # noqa: E731
                                                 ptr(H), None, None, None)
    assert call(ptr(Mf), F, None) == 1
    assert call(None, F, ptr(vm)) == 1
    assert call(ptr(Mf), F - 1, ptr(vm)) == 1
    assert call(ptr(Mf), F, ptr(vm)) == 0  # (W, div, cost and n_iter may be NULL)
    # the context solves correctly afterwards, and the default path returns the bits it returned before
    judge(name, device(name, gpu_ctx), oracle(name))
    after = snmf_mdi(V, M, p, ctx=gpu_ctx)
    assert bits(before[0]) == bits(after[0]) and bits(before[1]) == bits(after[1]) and bits(before[2]["cost"]) == bits(after[2]["cost"])
    e32 = rel(before[0], oracle(name)[0])
    print(f"fp32 mdi {name}: relV={e32:.2e}")
    assert e32 > 1e-9  # (and the two modes are two computations)


def test_leading_dimensions(gpu_ctx, lib):
    """V, M and V_mdi as the top rows of taller column-major arrays give the bits of the tight call."""
    from se_snmf_nat_amd.api import _make_params
    name = "kl_65x90_r9"
    V, M, p, _ = _args(name)
    F, T, r = CASES[name][0]
    v_ref, h_ref, _, _ = device(name, gpu_ctx)
    sp = _make_params(F, T, r, 1.0, 25, 0.0, 1, 1, 0, 0.5, None, None)
    tall = lambda a, extra: np.asfortranarray(np.concatenate([a, np.full((extra, T), np.nan)], axis=0))  # noqa: E731
    Vt, Mt, out = tall(V, 3), tall(M, 5), np.full((F + 7, T), -1.0, order="F")
    W0, H0, H = np.asfortranarray(p["init_w"]), np.asfortranarray(p["init_h"]), np.empty((r, T), order="F")
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.snmf_mdi_fp64(gpu_ctx._h, C.byref(sp), ptr(Vt), F + 3, ptr(Mt), F + 5, ptr(W0), ptr(H0), None, ptr(out), F + 7, None, ptr(H),
                             None, None, None) == 0
    assert np.array_equal(out[:F], v_ref) and (out[F:] == -1.0).all() and np.array_equal(H, h_ref)


# ---- 4. dnmf_adapt -----------------------------------------------------------------------------------------------------
def test_dnmf_adapt_in_fp64(gpu_ctx):
    from se_snmf_nat_amd import dnmf_adapt, sparse_nmf
    F, T, Rx, Rd = 65, 300, 6, 6
    Y, B, _ = (f32r(a) for a in synth_problem(F, T, Rx + Rd))
    D = f32r(synth_problem(F, T, Rd, seed_data=5)[0])
    p = dict(cf="kl", sparsity=5, max_iter=20, conv_eps=0, cost_check=1, R_x=Rx, R_d=Rd, random_seed=1)
    B_a = dnmf_adapt(Y, D, B, p, ctx=gpu_ctx, precision="fp64")

    def two_solves(solve):
        q = dict(p, w_update_ind=np.zeros(Rx + Rd, bool), h_update_ind=np.ones(Rx + Rd, bool), init_w=B)
        _, A, _ = solve(Y, q)
        q = dict(p, w_update_ind=np.ones(Rd, bool), h_update_ind=np.zeros(Rd, bool), init_w=B[:, Rx:], init_h=A[Rx:])
        return solve(D, q)[0]

    assert np.array_equal(B_a, two_solves(lambda v, q: sparse_nmf(v, q, ctx=gpu_ctx, precision="fp64")))
    e = rel(B_a, two_solves(oracle_nmf))
    print(f"dnmf_adapt fp64: relB_a = {e:.2e}")
    assert e < REL_WH
    with pytest.raises(ValueError, match="precision"):
        dnmf_adapt(Y, D, B, p, ctx=gpu_ctx, precision="fp16")


# ---- 5. the MEX shim ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
def test_snmf_mdi_mex_in_fp64(mex_shims, gpu_ctx, soft):
    from se_snmf_nat_amd import snmf_mdi, snmf_mdi_Sm
    V, W0, H0, M, Ms = problem((65, 90, 9))
    M = Ms if soft else M
    p = dict(cf="kl", sparsity_mdi=0.5, conv_eps_mdi=1e-4, max_iter=40, cost_check=1, init_w=W0, init_h=H0)
    opts = dict(beta=1.0, max_iter=40.0, conv_eps=1e-4, cost_check=1.0, device=0.0, precision="fp64")
    v, w, h, div, cost, n = mex_shims["snmf_mdi_mex"](6, V, M, W0, H0, 0.5, opts)
    info = {}
    v_b, h_b, o_b = (snmf_mdi_Sm if soft else snmf_mdi)(V, M, p, ctx=gpu_ctx, precision="fp64", info=info)
    k = int(n[0, 0])
    assert k == o_b["n_iter"] and div.shape == cost.shape == (1, 40)
    assert bits(v) == bits(v_b) and bits(h) == bits(h_b) and bits(w) == bits(info["w"])
    kk = len(o_b["cost"])
    assert bits(div[0, :kk]) == bits(o_b["div"]) and bits(cost[0, :kk]) == bits(o_b["cost"])
    (v1,) = mex_shims["snmf_mdi_mex"](1, V, M, W0, H0, 0.5, opts)
    assert bits(v1) == bits(v_b)


@pytest.mark.parametrize("bad", [64.0, "fp16"])
def test_snmf_mdi_mex_refuses_another_precision(mex_shims, bad):
    V, W0, H0, M, _ = problem((65, 90, 9))
    with pytest.raises(MexError) as e:
        mex_shims["snmf_mdi_mex"](1, V, M, W0, H0, 0.5, dict(beta=1.0, max_iter=3.0, device=0.0, precision=bad))
    assert e.value.id == "snmf:type"
