"""The fp64 solve mode (precision="fp64" -> snmf_sparse_nmf_fp64: fp64 storage, f64 MFMA contractions) against the fp64 oracle.

Bounds (not measured on the code under test: they come from the oracle's own sensitivity):
the oracle's results move by at most 4.1e-13 (W), 1.8e-13 (H) relative Frobenius and 7.7e-15 (cost) when V, W0 and H0 are
each perturbed by a relative 1e-13, the response is linear, and another summation order in an fp64 contraction of
length <= 4500 is a perturbation of at most K u ~ 5e-13 (typically sqrt(K) u ~ 1e-14).  So
    REL_WH   = 1e-11   relative Frobenius error of W and of H          (25 x the response to 1e-13)
    REL_COST = 1e-12   relative error of EVERY div and cost entry
    n_iter           equal (the oracle's |dcost|/cost stays >= 1 % of conv_eps away from conv_eps on every case here)
The fp32 path sits near 1e-6 on the same cases: a fall-back to it cannot pass.

L = 2048 (kS64ChunkK in csrc/snmf_solve64.h) is the split length of a contraction: T = 4500 = 2 L + 404 spans two whole
splits and a ragged third; F = 2600 splits the W' * R contraction; 64 x 4096, r = 64 is a multiple of every tile
dimension (64 x 64 x 16 tiles, L, the 256-frame row-sum chunks).

Measured on an MI355X (max over the cases of each group; every case prints its own line):
    the 11 goldens            relW <= 9.7e-16  relH <= 4.8e-15  reldiv <= 1.3e-15  relcost <= 5.2e-16   n_iter equal in all
    the 14 tile-edge cases    relW <= 3.7e-15  relH <= 4.2e-15  reldiv <= 9.8e-16  relcost <= 6.0e-16   n_iter equal in all
    C2 full size, 12 iter.    relW = 6.7e-16   relH(head) = 9.0e-16  relH(tail) = 9.9e-16  reldiv = 2.1e-15  relcost = 2.7e-15
    C2 full size, 260 iter.   reldiv <= 4.3e-15  relcost <= 4.1e-15 over all 260 iterations (0.9 s for the call)
    fp32 on the same cases    ~1e-7 .. 1e-6
"""
import functools
import os
import time

import numpy as np
import pytest

from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem
from test_oracle import GOLD, SOLVE_CASES, load_case

pytestmark = pytest.mark.gpu
REL_WH = 1e-11
REL_COST = 1e-12
N_COST_C2 = 260  # iterations of the full-size golden's objective history that test_full_size_c2_in_fp64 compares (all of them)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    nz = b != 0
    if (a[~nz] != 0).any():  # (the zero vectors of cost_check = 0 / sparse_nmf_GPU must be zeros)
        return float("inf")
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def judge(name, res, ref):
    """Print the measured errors, then assert the bounds.  ref: (W or None, H, div, cost, n_iter)."""
    w, h, o = res
    wr, hr, divr, costr, nr = ref
    ew = rel(w, wr) if wr is not None else 0.0
    eh = rel(h, hr)
    same_len = len(o["div"]) == len(divr) and len(o["cost"]) == len(costr)
    ed = relmax(o["div"], divr) if same_len else float("inf")
    ec = relmax(o["cost"], costr) if same_len else float("inf")
    print(f"fp64 solve {name}: n_iter={o['n_iter']} (oracle {nr}) relW={ew:.2e} relH={eh:.2e} reldiv={ed:.2e} relcost={ec:.2e}")
    assert o["n_iter"] == nr
    assert same_len
    assert np.isfinite(w).all() and np.isfinite(h).all()
    assert ew < REL_WH, ew
    assert eh < REL_WH, eh
    assert ed < REL_COST, ed
    assert ec < REL_COST, ec


def f32r(a):
    """fp32-rounded values held as doubles (how the goldens' inputs were made)."""
    return np.asarray(a, np.float32).astype(np.float64)


# ---- 1. the goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", SOLVE_CASES, ids=lambda p: os.path.basename(p)[:-4])
def test_goldens_in_fp64(gpu_ctx, path):
    from se_snmf_nat_amd import sparse_nmf
    d, p = load_case(path)
    res = sparse_nmf(d["V"].astype(np.float64), p, ctx=gpu_ctx, precision="fp64")
    judge(os.path.basename(path)[:-4], res, (d.get("W"), d["H"], d["div"], d["cost"], int(d["n_iter"])))


# ---- 2. tile edges ----------------------------------------------------------------------------------------------------
def _cases():
    c = {}
    kl = dict(cf="kl", sparsity=5, cost_check=1)
    c["kl_65x4500_r20"] = ((65, 4500, 20), dict(kl, max_iter=30, conv_eps=0), {})
    c["kl_65x4500_r20_stop"] = ((65, 4500, 20), dict(kl, max_iter=100, conv_eps=1e-3), {})
    c["ed_97x2100_r33"] = ((97, 2100, 33), dict(cf="ed", sparsity=2, max_iter=25, cost_check=1), {})
    c["b15_97x2100_r33_semi"] = ((97, 2100, 33), dict(cf="beta", beta=1.5, sparsity=1, max_iter=25, cost_check=1,
                                                      w_update_ind=np.arange(33) >= 17), {})
    c["kl_honly_97x2100_r33_stop"] = ((97, 2100, 33), dict(kl, max_iter=100, conv_eps=1e-3, w_update_ind=np.zeros(33, bool)), {})
    c["kl_wonly_97x2100_r33_stop"] = ((97, 2100, 33), dict(kl, max_iter=100, conv_eps=1e-3, h_update_ind=np.zeros(33, bool)), {})
    c["kl_2600x130_r20"] = ((2600, 130, 20), dict(kl, max_iter=15), {})
    c["kl_1x50_r3"] = ((1, 50, 3), dict(kl, max_iter=10), {})
    c["kl_17x15_r1"] = ((17, 15, 1), dict(kl, max_iter=10), {})
    c["kl_64x4096_r64_tiles"] = ((64, 4096, 64), dict(kl, max_iter=10), {})
    rs = np.random.RandomState(3)
    c["kl_97x2100_r33_rvec"] = ((97, 2100, 33), dict(cf="kl", sparsity=0.5 + 5 * rs.random_sample(33), max_iter=20, cost_check=1), {})
    c["b15_97x2100_r33_full_sparsity"] = ((97, 2100, 33), dict(cf="beta", beta=1.5, sparsity=2 * rs.random_sample((33, 2100)),
                                                               max_iter=20, cost_check=1), {})
    c["kl_97x2100_r33_nocheck"] = ((97, 2100, 33), dict(cf="kl", sparsity=5, max_iter=20, conv_eps=1e-3, cost_check=0), {})
    c["kl_97x2100_r33_gpu_variant"] = ((97, 2100, 33), dict(cf="kl", sparsity=5, max_iter=20), dict(gpu_variant=True))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def problem(shape):
    V, W0, H0 = synth_problem(*shape)
    V, W0, H0 = f32r(V), f32r(W0), f32r(H0)
    for a in (V, W0, H0):
        a.setflags(write=False)
    return V, W0, H0


@functools.lru_cache(maxsize=None)
def oracle(name):
    shape, p, kw = CASES[name]
    V, W0, H0 = problem(shape)
    w, h, o = oracle_nmf(V, dict(p, init_w=W0, init_h=H0), **kw)
    return w, h, o["div"], o["cost"], o["n_iter"]


def device(name, ctx):
    from se_snmf_nat_amd import sparse_nmf, sparse_nmf_GPU
    shape, p, kw = CASES[name]
    V, W0, H0 = problem(shape)
    fn = sparse_nmf_GPU if kw.get("gpu_variant") else sparse_nmf
    return fn(V, dict(p, init_w=W0, init_h=H0), ctx=ctx, precision="fp64")


@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_edges_in_fp64(gpu_ctx, name):
    res, ref = device(name, gpu_ctx), oracle(name)
    judge(name, res, ref)
    if name.endswith("nocheck") or name.endswith("gpu_variant"):
        # cost_check = 0: zero vectors and no stop (src/sparse_nmf.m:260); sparse_nmf_GPU.m never fills them (:263-264)
        assert not res[2]["div"].any() and not res[2]["cost"].any() and len(res[2]["cost"]) == 20 and res[2]["n_iter"] == 20
    np.testing.assert_allclose(np.sqrt((res[0] ** 2).sum(0)), 1.0, rtol=1e-13)


# ---- 3. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kl_65x4500_r20", "b15_97x2100_r33_semi", "kl_2600x130_r20"])
def test_two_runs_give_the_same_bits(gpu_ctx, name):
    w1, h1, o1 = device(name, gpu_ctx)
    w2, h2, o2 = device(name, gpu_ctx)
    assert w1.tobytes() == w2.tobytes() and h1.tobytes() == h2.tobytes()
    assert o1["div"].tobytes() == o2["div"].tobytes() and o1["cost"].tobytes() == o2["cost"].tobytes()


# ---- 4. full size -----------------------------------------------------------------------------------------------------
def test_full_size_c2_in_fp64(gpu_ctx):
    """BASELINE C2 (257 x 100000, r = 256, KL, sparsity 5) on the inputs of bench.make_problem, rounded as
    tests/golden/make_golden_c2.py rounds them, 12 iterations: W12, the head / tail frames of H12 and cost[:12], div[:12]
    of the committed golden at the bounds above; then the objective of all 260 iterations the golden holds."""
    from bench import F_, R_, SPARSITY, T_, make_problem
    from se_snmf_nat_amd import sparse_nmf
    g = np.load(os.path.join(GOLD, "c2_full_257x100000_r256.npz"))
    assert (int(g["F"]), int(g["T"]), int(g["r"])) == (F_, T_, R_)
    V, W0, H0 = make_problem(F_, T_, R_)
    V, H0 = f32r(V), f32r(H0)
    t = time.time()
    w, h, o = sparse_nmf(V, dict(cf="kl", sparsity=SPARSITY, conv_eps=0, init_w=W0, init_h=H0, cost_check=1, max_iter=12),
                         ctx=gpu_ctx, precision="fp64")
    dt = time.time() - t
    ew, eh0, eh1 = rel(w, g["W12"]), rel(h[:, :64], g["H12_head"]), rel(h[:, -64:], g["H12_tail"])
    ec, ed = relmax(o["cost"], g["cost"][:12]), relmax(o["div"], g["div"][:12])
    print(f"fp64 solve C2 full size, 12 iterations in {dt:.2f} s (transfers included): relW={ew:.2e} relH(head)={eh0:.2e} "
          f"relH(tail)={eh1:.2e} reldiv={ed:.2e} relcost={ec:.2e}")
    assert o["n_iter"] == 12
    assert ew < REL_WH and eh0 < REL_WH and eh1 < REL_WH
    assert ed < REL_COST and ec < REL_COST
    # the device makes the golden's whole objective history affordable: all N_COST_C2 iterations of it, at the same bound
    t = time.time()
    _, _, o = sparse_nmf(V, dict(cf="kl", sparsity=SPARSITY, conv_eps=0, init_w=W0, init_h=H0, cost_check=1, max_iter=N_COST_C2),
                         ctx=gpu_ctx, precision="fp64")
    dt = time.time() - t
    ec, ed = relmax(o["cost"], g["cost"][:N_COST_C2]), relmax(o["div"], g["div"][:N_COST_C2])
    print(f"fp64 solve C2 full size, {N_COST_C2} iterations in {dt:.2f} s: reldiv={ed:.2e} relcost={ec:.2e} (max over all iterations)")
    assert o["n_iter"] == N_COST_C2 and len(g["cost"]) >= N_COST_C2
    assert ed < REL_COST and ec < REL_COST


# ---- 5. the fp32 path is untouched ------------------------------------------------------------------------------------
def test_fp32_solve_gives_the_same_bits_around_an_fp64_solve(gpu_ctx):
    from se_snmf_nat_amd import sparse_nmf
    V, W0, H0 = problem((97, 2100, 33))
    p = dict(cf="kl", sparsity=5, max_iter=20, conv_eps=1e-3, init_w=W0, init_h=H0, cost_check=1)
    w1, h1, o1 = sparse_nmf(V, p, ctx=gpu_ctx)
    w64, h64, o64 = sparse_nmf(V, p, ctx=gpu_ctx, precision="fp64")
    w2, h2, o2 = sparse_nmf(V, p, ctx=gpu_ctx)
    assert w1.tobytes() == w2.tobytes() and h1.tobytes() == h2.tobytes() and o1["cost"].tobytes() == o2["cost"].tobytes()
    assert o1["n_iter"] == o2["n_iter"]
    # and the two modes are two computations: fp32 sits orders of magnitude above the fp64 bound
    assert rel(w1, w64) > 1e-9 and rel(w1, w64) < 1e-4
