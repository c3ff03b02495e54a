"""The extra row (F = 32n+1) off the MFMA waves' path: k_hstep_rp adds the row's term of W^T*ratio as FMAs in front of the P2
epilogue (no k-block of its own), k_wstats_xg runs the row of the statistics behind P3's first W-fragment loads.

Per shape: three full KL iterations, sparsity 5, with the objective.
  - the default plan runs k_hstep_rp's uncut form (the one with the FMAs) and, by its describe(), not the old placement of
    the statistics' row; the plan with SNMF_WSTATS_XG=0 names that placement;
  - every iterate of the default plan -- W (the fp64 master), H, div, cost -- equals BIT FOR BIT what the plan with the switch
    off computes: the same code on the same frames in the same tile order, on the same deal of the row groups;
  - W and H of every step of the default plan stay within the per-element one-step bounds of tests/elementwise.py, region by
    region (W.rows.extra_valu among them), against the fp64 step from the device's own previous iterate.
(H of k_hstep_rp against the barrier-phased k_hstep, bit for bit: tests/test_gpu_pipelined_vs_plain.py.)

Shapes: every one has at least 3 tiles per statistics chunk and more tiles than H-step workgroups (below that neither the
buffer rotation nor the role pipeline is exercised).
    257 x 20 000, r = 256   the headline geometry
    257 x 16 411, r = 200   rp < 256 and a ragged last tile
    161 x 20 000, r = 136   the second row group is a single row tile
    193 x 12 345, r = 129   three tiles per chunk: every buffer gets its last tenant, none a fourth
     97 x 24 600, r = 200   one row group of three row tiles: the fourth consumer wave has a share of the row and no row tile
"""
import re

import numpy as np
import pytest

from elementwise import chain_t, compare, ref_hstep, ref_wstep, regions, tau_h, tau_w

pytestmark = pytest.mark.gpu

SPARSITY = 5.0
STEPS = 3
SHAPES = [(257, 256, 20000), (257, 200, 16411), (161, 136, 20000), (193, 129, 12345), (97, 200, 24600)]


def problem(F, r, T):
    rs = np.random.default_rng(7919 * F + 31 * r + T)
    V = (rs.gamma(0.5, 1.0, (F, 16)) @ rs.gamma(0.3, 1.0, (16, T)) + 1e-3).astype(np.float32)
    return V, rs.random((F, r)), rs.random((r, T)).astype(np.float32)


def run_plan(ctx, F, r, T, data):
    """(describe(), state after init, [(W_k, H_k)] for k = 1..STEPS, div, cost) of a plan created under the current switches."""
    from se_snmf_nat_amd import Plan
    V, W0, H0 = data
    pl = Plan(ctx, F, T, r, beta=1.0, max_iter=STEPS, conv_eps=0.0, cost_check=True, sparsity=SPARSITY)
    try:
        desc = pl.describe()
        pl.set_v(V)
        pl.set_w(W0)
        pl.set_h(H0)
        pl.init()
        start = (pl.get_w(), pl.get_h(np.float32))
        its = []
        for _ in range(STEPS):
            pl.run(1)
            its.append((pl.get_w(), pl.get_h(np.float32)))
        div, cost, n = pl.get_objective()
        assert n == STEPS, (n, STEPS)
    finally:
        pl.close()
    return desc, start, its, np.array(div[:STEPS]), np.array(cost[:STEPS])


def grid_of(desc):
    return tuple(int(x) for x in re.search(r"grid=\((\d+) chunks,(\d+) fgroups,(\d+) kgroups; group-1 chunks (\d+)\)", desc).groups())


OFF = ", extra row at the top of the tile (SNMF_WSTATS_XG=0)"


@pytest.mark.parametrize("F,r,T", SHAPES, ids=lambda v: str(v))
def test_extra_row_paths(gpu_ctx, F, r, T, monkeypatch):
    for k in ("SNMF_HSTEP_RP", "SNMF_HSTEP_SPLIT", "SNMF_WSTATS_NL", "SNMF_WSTATS_XG"):
        monkeypatch.delenv(k, raising=False)
    data = problem(F, r, T)
    V = data[0]
    desc, (W, H), its, div, cost = run_plan(gpu_ctx, F, r, T, data)
    assert "k_hstep_rp (4 P1 + 4 P2 + 4 loader waves;" in desc and "(+1 VALU row)" in desc, desc
    assert "NK=8 waves=4+4" in desc and OFF not in desc, desc
    ch, nfg, nkg, ch1 = grid_of(desc)
    assert nfg == (2 if F > 129 else 1) and nkg == 1, desc
    tiles = (T + 31) // 32
    assert tiles >= 3 * max(ch, ch1) and tiles > int(re.search(r"grid=(\d+) x 768 thr", desc).group(1)), desc

    # the one-step bounds, region by region, against the fp64 step from the device's own previous iterate
    regs = regions(desc, F, T, r)
    assert "W.rows.extra_valu" in regs
    t_h, t_w = tau_h(F, r, 1.0), tau_w(F, r, 1.0, chain_t(desc, T))
    for k, (Wk, Hk) in enumerate(its, 1):
        Hr, info = ref_hstep(V, W, H, 1.0, SPARSITY)
        st = compare(Hk, Hr, t_h, regs, "H", floors=info, what=f"{F}x{T} r={r} step {k} H")
        Wr, info = ref_wstep(V, W, Hk, 1.0)
        sw = compare(Wk, Wr, t_w, regs, "W", floors=info, what=f"{F}x{T} r={r} step {k} W")
        print(f"{F}x{T} r={r} step {k}: worst H {st['H.all'][0]:.2e} / {t_h:.2e}, worst W {sw['W.all'][0]:.2e} / {t_w:.2e}, "
              f"extra row {sw['W.rows.extra_valu'][0]:.2e}")
        W, H = Wk, Hk

    # the row at the top of the tile: every iterate bit for bit
    monkeypatch.setenv("SNMF_WSTATS_XG", "0")
    desc0, _s0, its0, div0, cost0 = run_plan(gpu_ctx, F, r, T, data)
    assert desc0 == desc.replace(" B | W finish", " B" + OFF + " | W finish") and OFF in desc0, (desc, desc0)
    for k, ((Wa, Ha), (Wb, Hb)) in enumerate(zip(its, its0), 1):
        assert np.array_equal(Ha, Hb), f"step {k}: H differs from the plan with SNMF_WSTATS_XG=0 at {np.argwhere(Ha != Hb)[:4].tolist()}"
        assert np.array_equal(Wa, Wb), f"step {k}: W differs from the plan with SNMF_WSTATS_XG=0 at {np.argwhere(Wa != Wb)[:4].tolist()}"
    assert np.array_equal(div, div0) and np.array_equal(cost, cost0), (div, div0, cost, cost0)
