"""The rules behind tests/test_gpu_mdi_elementwise.py, checked without a device: the chained fp64 pieces of the masked step equal
oracle/mdi_oracle.py, the case table selects the statistics geometries it names inside the mask's envelope and covers what it
claims, the mask's share of the bounds behaves, and the element-wise comparator catches the faults this module exists for -- a
tile of V not re-imputed, a soft-mask tile re-imputed twice, the extra row's V left behind, a pad frame entering the W statistics
-- where the whole-matrix criterion of tests/test_mdi.py (rel < 1e-4) lets the first three through."""
import re

import numpy as np
import pytest

from elementwise import FLR, U, chain_t, compare, ref_hstep, ref_wstep, rel, tau_h, tau_w
from mdi_elementwise import (MDI_CASES, case_masks, compare_vmdi, dv_mdi, in_mask_envelope, make_mask, mask_image, mdi_cost,
                             mdi_final, mdi_grid, mdi_impute, mdi_regions, mdi_start, mdi_step, tau_h_mdi, tau_vmdi, tau_w_mdi)
from oracle.mdi_oracle import snmf_mdi as oracle_mdi

BETAS = [0.0, 0.5, 1.0, 1.5, 2.0]
MODES = ["full", "h", "w", "semi"]
MASKS = ["01", "soft", "ones", "blocks"]
REL = 1e-4  # tests/test_mdi.REL


def _problem(F, T, r, seed):
    rs = np.random.default_rng(seed)
    V = (rs.gamma(0.5, 1.0, (F, 6)) @ rs.gamma(0.3, 1.0, (6, T)) + 1e-3).astype(np.float32)
    return rs, V, rs.random((F, r)), rs.random((r, T)).astype(np.float32)


def _normalised(W0, H0):
    wn = np.sqrt((W0 ** 2).sum(0))
    return W0 / wn, H0.astype(np.float64) * wn[:, None]  # src/snmf_mdi.m:163-165


# ---- the fp64 pieces ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("beta", BETAS)
def test_chained_pieces_equal_the_oracle(beta, mode, mask):
    F, T, r, n = 37, 150, 7, 3
    rs, V, W0, H0 = _problem(F, T, r, 11)
    M = make_mask(mask, F, T, rs)
    S = [0.5, rs.uniform(0.0, 2.0, r), rs.uniform(0.0, 2.0, (r, T))][(BETAS.index(beta) + MODES.index(mode)) % 3]
    w_ind, h_ind = case_masks(mode, r)
    p = dict(cf="beta", beta=beta, sparsity_mdi=S, conv_eps_mdi=0, max_iter=n, cost_check=1, init_w=W0, init_h=H0.astype(np.float64))
    if w_ind is not None:
        p["w_update_ind"] = w_ind
    if h_ind is not None:
        p["h_update_ind"] = h_ind
    v_o, h_o, o = oracle_mdi(V.astype(np.float64), M, p)
    W, H = _normalised(W0, H0)
    Vt = mdi_start(V, M)
    cost = []
    for _k in range(n):
        Vt, W, H, _floors = mdi_step(Vt, M, W, H, beta, S, mode, w_ind)
        cost.append(mdi_cost(Vt, W, H, beta, S))
    np.testing.assert_allclose(H, h_o, rtol=1e-12)
    np.testing.assert_allclose(W, o["w"], rtol=1e-12)
    np.testing.assert_allclose(cost, o["cost"], rtol=1e-12)
    np.testing.assert_allclose(mdi_final(Vt, M, W, H)[0], v_o, rtol=1e-12)


def test_the_steps_take_v_as_it_is_only_on_request():
    """ref_hstep / ref_wstep round V to fp32 unless told otherwise: an fp64 V off the fp32 grid moves the result by ~u."""
    rs, V, W0, H0 = _problem(37, 53, 7, 3)
    W, H = _normalised(W0, H0)
    V64 = V.astype(np.float64) * (1.0 + 0.4 * U)
    assert np.array_equal(ref_hstep(V64, W, H, 1.0, 0.5)[0], ref_hstep(V, W, H, 1.0, 0.5)[0])
    a, b = ref_hstep(V64, W, H, 1.0, 0.5, exact_v=True)[0], ref_hstep(V, W, H, 1.0, 0.5)[0]
    assert 0.3 * U < np.abs(a / b - 1).max() < 0.5 * U
    a, b = ref_wstep(V64, W, H, 1.0, exact_v=True)[0], ref_wstep(V, W, H, 1.0)[0]
    assert 0 < np.abs(a / b - 1).max() < 2 * U


# ---- the bounds ---------------------------------------------------------------------------------------------------------------

def test_the_masks_share_of_the_bounds():
    F, r, t_c = 257, 40, 96
    for beta in BETAS:
        # nothing to add for a mask of ones: the unmasked bounds
        for k in (1, 2, 3):
            assert tau_h_mdi(F, r, beta, k, all_observed=True) == tau_h(F, r, beta)
            assert tau_w_mdi(F, r, beta, t_c, k, all_observed=True) == tau_w(F, r, beta, t_c)
        # monotone in k, and the W finish carries four times what the H step does
        th = [tau_h_mdi(F, r, beta, k) for k in (1, 2, 3, 4)]
        tw = [tau_w_mdi(F, r, beta, t_c, k) for k in (1, 2, 3, 4)]
        assert all(a < b for a, b in zip(th, th[1:])) and all(a < b for a, b in zip(tw, tw[1:]))
        for k in (1, 2, 3):
            assert np.isclose(tw[k - 1] - tau_w(F, r, beta, t_c), 4 * (th[k - 1] - tau_h(F, r, beta)), rtol=1e-9)
    assert dv_mdi(r, 0) == U and dv_mdi(r, 1) == (r + 5) * U and dv_mdi(r, 3) == (r + 11) * U
    # the recursion dV_k <= max(dV_{k-1} + u, (r + 4) u) + u that the closed form covers
    d = U
    for k in range(1, 9):
        d = max(d + U, (r + 4) * U) + U
        assert d <= dv_mdi(r, k)
    assert all(dv_mdi(r, k, all_observed=True) == 0.0 for k in range(4))
    assert tau_vmdi(r, 3) == U * (2 * (r + 2) + 7) + dv_mdi(r, 3) and tau_vmdi(r, 2) < tau_vmdi(r, 3) < tau_vmdi(2 * r, 3)
    # no bound for a factor the mode leaves alone
    assert tau_h_mdi(F, r, 1.0, 1, "w") is None and tau_w_mdi(F, r, 1.0, t_c, 1, "h") is None


# ---- the case table -----------------------------------------------------------------------------------------------------------

def _describe(c):
    from se_snmf_nat_amd.api import geometry_describe
    w, h = case_masks(c["mode"], c["r"])
    return geometry_describe(c["F"], c["T"], c["r"], beta=c["beta"], n_cu=256, w_update_ind=w, h_update_ind=h)


@pytest.fixture(scope="module")
def described(lib):
    return {c["id"]: _describe(c) for c in MDI_CASES}


@pytest.mark.parametrize("case", MDI_CASES, ids=lambda c: c["id"])
def test_each_case_selects_its_statistics_and_stays_in_the_envelope(described, case):
    desc = described[case["id"]]
    for tok in case["tokens"]:
        assert tok in desc[desc.index("| wstats") if not tok.startswith("beta=") else 0:], (case["id"], tok, desc)
    assert in_mask_envelope(desc, case["r"]), (case["id"], desc)
    F, T, r = case["F"], case["T"], case["r"]
    regs = mdi_regions(desc, F, T, r, case["mode"])
    for name in case["expect"]:
        assert name in regs and len(regs[name][2]) > 0, (case["id"], name, sorted(regs))
    for name, (_m, axis, idx) in regs.items():
        n = {("W", 0): F, ("W", 1): r, ("H", 0): r, ("H", 1): T}[(_m, axis)]
        assert len(idx) == 0 or (idx.min() >= 0 and idx.max() < n), (case["id"], name)
    th = tau_h_mdi(F, r, case["beta"], 3, case["mode"])
    tw = tau_w_mdi(F, r, case["beta"], chain_t(desc, T), 3, case["mode"])
    assert (th is None) == (case["mode"] == "w") and (tw is None) == (case["mode"] == "h"), case["id"]
    assert all(t < 1e-3 for t in (th, tw) if t is not None), (case["id"], th, tw)
    # ... and well below what a structural error does (one wrong element of a frame moves that frame's H column by ~1/F)
    assert th is None or th < 0.1 / F, (case["id"], th)
    # the issue's shapes have a partial last tile and no frame or row without an observed entry (make_mask asserts the latter)
    assert T % 32 != 0, case["id"]


def test_in_mask_envelope_refuses_what_set_mask_refuses(lib):
    from se_snmf_nat_amd.api import geometry_describe
    assert not in_mask_envelope(geometry_describe(2700, 700, 40), 40)       # the out-of-envelope path
    assert not in_mask_envelope(geometry_describe(513, 3000, 1000), 1000)   # F + r > 1272: 16-frame tiles
    assert in_mask_envelope(geometry_describe(257, 1000, 40), 40)


def test_case_table_covers_what_the_pass_and_the_statistics_can_do(described):
    by = {c["id"]: (c, described[c["id"]]) for c in MDI_CASES}

    def cases(pred):
        return [(c, d) for c, d in by.values() if pred(c, d)]

    def bm(c):
        return "kl" if c["beta"] == 1.0 else "ed" if c["beta"] == 2.0 else "gen"

    # every MDI = true instantiation: BM x (OBJ, UPD).  (0, 1): step 1 of a plan that updates H; (1, 1): its steps 2, 3 with
    # cost_check; (1, 0): a W-only plan's pass, and the final objective pass of every plan with cost_check
    for b in ("kl", "ed", "gen"):
        assert cases(lambda c, d: bm(c) == b and c["mode"] != "w" and c["cost_check"] and c["steps"] >= 2), b
        assert cases(lambda c, d: bm(c) == b and c["mode"] == "w" and c["cost_check"]), b
        assert cases(lambda c, d: bm(c) == b and c["mode"] == "h"), b
    assert {0.0, 0.5, 1.0, 1.5, 2.0} == {c["beta"] for c, _d in by.values()}
    # the extra row on (F = 65, 257, 513) and off (F = 64, 130, 422), T < 32, three to five tiles, more tiles than workgroups
    assert {65, 257, 513} <= {c["F"] for c, d in by.values() if "(+1 VALU row)" in d}
    assert {64, 130, 422} <= {c["F"] for c, d in by.values() if "(+0 VALU row)" in d}
    assert cases(lambda c, d: c["T"] < 32)
    assert cases(lambda c, d: 3 <= (c["T"] + 31) // 32 <= 5)
    two = cases(lambda c, d: (c["T"] + 31) // 32 > mdi_grid(d)[1])
    assert two and any((c["T"] + 31) // 32 < 2 * mdi_grid(d)[1] for c, d in two)  # some workgroups take two tiles and some one
    assert cases(lambda c, d: (c["F"], c["T"], c["r"]) == (257, 8300, 40) and c["mask"] == "blocks")
    # the statistics geometries
    assert cases(lambda c, d: "waves=4+0" in d and (c["T"] + 31) // 32 <= 8)                            # synchronous, few tiles
    assert cases(lambda c, d: "NK=4 waves=4+4" in d and "k_wstats_s" not in d)                           # loaders, four consumers
    assert cases(lambda c, d: "NK=4 waves=8+4" in d and "k_wstats_s" not in d and c["F"] >= 257)          # loaders, eight consumers
    assert cases(lambda c, d: "NK=8 " in d)
    assert cases(lambda c, d: "NK=16 " in d and "2 kgroups" in d)
    m = [re.search(r"grid=\((\d+) chunks,(\d+) fgroups,1 kgroups; group-1 chunks (\d+)\)", d) for c, d in by.values() if c["F"] == 513]
    assert any(x and int(x.group(2)) == 2 and x.group(1) != x.group(3) for x in m)                        # two row groups, n_ch1 != 0
    assert cases(lambda c, d: "k_wstats_sf" in d and c["F"] == 64 and 70 <= c["r"] <= 128 and c["mode"] == "full")  # k_iter_sf unmasked
    assert cases(lambda c, d: "k_iter_sf (" in d)
    assert cases(lambda c, d: "single remainder tile shared by the eight waves" in d)
    assert cases(lambda c, d: "k_wstats_sr" in d and c["mode"] == "full") and cases(lambda c, d: "k_wstats_sr" in d and c["mode"] == "semi")
    assert cases(lambda c, d: "Gram matrix" in d and c["beta"] == 2.0 and c["r"] <= 256)
    assert cases(lambda c, d: c["beta"] == 2.0 and c["r"] > 256 and "NK=16" in d and "Gram matrix" in d)
    assert cases(lambda c, d: c["beta"] == 2.0 and c["r"] > 256 and "NK=16" in d and "Gram matrix" not in d)
    # modes, masks, sparsity forms, the final imputation as a pass of its own
    assert {"full", "h", "w", "semi"} == {c["mode"] for c, _d in by.values()}
    assert {"01", "soft", "ones", "blocks"} == {c["mask"] for c, _d in by.values()}
    assert {"scalar", "rvec", "entry"} == {c["sp"] for c, _d in by.values()}
    assert [c["id"] for c, _d in by.values() if not c["cost_check"]] == ["kl_nocost_F257"]
    assert 20 <= len(MDI_CASES) <= 30


# ---- the comparator against the faults of the MDI state ------------------------------------------------------------------------
#
# The fp64 "device": the chained reference itself, rounded to fp32 with noise at a quarter of the bound, and ONE fault in the V it
# hands to the next step.  65 rows, r = 9 on 256 workgroups: the extra row, a partial last tile and tiles in the second round of
# the tile loop (0/1 mask: 8300 frames, four such tiles, 12 frames in the last; soft mask: 8196 frames, the 4-frame last tile is
# the second round).  The fault sits late in the solve (iteration N + 1), where Lam moves little between iterates: this is where
# the whole-matrix criterion of tests/test_mdi.py -- on H and v_MDI; it never looks at W -- is blind.

N_BEFORE = 60


def _noisy(ref, tau, rs):
    return (ref * (1.0 + rs.uniform(-0.25, 0.25, ref.shape) * tau)).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module", params=[("01", 8300), ("soft", 8196)], ids=lambda p: p[0])
def late(lib, request):
    """N_BEFORE iterations of the fp64 chain, then the state (V_{N-1}, V_N, W_N, H_N) around which a fault is injected."""
    from se_snmf_nat_amd.api import geometry_describe
    kind, T = request.param
    F, r, beta, S = 65, 9, 1.0, 0.5
    desc = geometry_describe(F, T, r, beta=beta, n_cu=256)
    rs, V, W0, H0 = _problem(F, T, r, 5)
    M = make_mask(kind, F, T, rs)
    W, H = _normalised(W0, H0)
    Vt = mdi_start(V, M)
    Vprev = Vt
    for _k in range(N_BEFORE):
        Vprev = Vt
        Vt, W, H, _fl = mdi_step(Vt, M, W, H, beta, S, "full")
    k = N_BEFORE + 1
    return dict(kind=kind, F=F, T=T, r=r, beta=beta, S=S, M=M, V32=V, Vprev=Vprev, V=Vt, W=W, H=H, k=k,
                regs=mdi_regions(desc, F, T, r), th=tau_h_mdi(F, r, beta, k), tw=tau_w_mdi(F, r, beta, chain_t(desc, T), k),
                grid=mdi_grid(desc)[1])


def _faulty_step(s, V_fault):
    """Step k on the device side from a faulty V against the reference from the tracked V: (H_dev, H_ref, W_dev, W_ref)."""
    rs = np.random.default_rng(1)
    Hr, ih = ref_hstep(s["V"], s["W"], s["H"], s["beta"], s["S"], exact_v=True)
    Hd = _noisy(ref_hstep(V_fault, s["W"], s["H"], s["beta"], s["S"], exact_v=True)[0], s["th"], rs)
    Wr, iw = ref_wstep(s["V"], s["W"], Hd, s["beta"], exact_v=True)
    Wd = _noisy(ref_wstep(V_fault, s["W"], Hd, s["beta"], exact_v=True)[0], s["tw"], rs)
    assert min(ih["lam"], ih["dph"], iw["dpw"]) > 10 * FLR
    return Hd, Hr, Wd, Wr


def _flagged(dev, ref, tau, regs, matrix, region, spared=()):
    with pytest.raises(AssertionError) as e:
        compare(dev, ref, tau, regs, matrix)
    msg = str(e.value)
    assert f"region {region}:" in msg, msg
    for sp in spared:
        assert f"region {sp}:" not in msg, msg
    return msg


def test_comparator_passes_the_faultless_step(late):
    Hd, Hr, Wd, Wr = _faulty_step(late, late["V"])
    st = compare(Hd, Hr, late["th"], late["regs"], "H")
    assert {"H.frames.mdi_first_round", "H.frames.mdi_later_rounds", "H.frames.last_partial_tile"} <= set(st)
    assert "W.rows.extra_valu" in compare(Wd, Wr, late["tw"], late["regs"], "W")


def test_comparator_names_a_tile_that_was_not_re_imputed(late):
    """Tile 257 (a second-round tile) keeps V_{N-1}: the imputation of iteration N skipped it.  (0/1 mask: under the soft one V
    settles too slowly for the whole-matrix criterion to miss a whole tile.)"""
    s = late
    if s["kind"] != "01":
        return
    t0 = 32 * (s["grid"] + 1)
    Vf = s["V"].copy()
    Vf[:, t0:t0 + 32] = s["Vprev"][:, t0:t0 + 32]
    Hd, Hr, Wd, Wr = _faulty_step(s, Vf)
    assert rel(Hd, Hr) < REL  # the whole-matrix criterion lets it through
    msg = _flagged(Hd, Hr, s["th"], s["regs"], "H", "H.frames.mdi_later_rounds", ["H.frames.mdi_first_round", "H.frames.last_partial_tile"])
    t = int(re.search(r"region H.frames.mdi_later_rounds: element \((\d+), (\d+)\)", msg).group(2))
    assert t0 <= t < t0 + 32, msg


def test_comparator_names_a_soft_tile_re_imputed_twice(late):
    """The last, partial tile is re-imputed a second time with the same (W_N, H_N): not idempotent under a soft mask -- and
    without any effect under a 0/1 mask, where v .* M + Lam .* (1 - M) forgets the missing entries' previous values."""
    s = late
    t0 = 32 * (s["T"] // 32)
    Vf = s["V"].copy()
    Vf[:, t0:] = mdi_impute(s["V"], s["M"], s["W"], s["H"])[:, t0:]
    if s["kind"] == "01":
        assert np.array_equal(Vf, s["V"])
        return
    Hd, Hr, Wd, Wr = _faulty_step(s, Vf)
    assert rel(Hd, Hr) < REL
    _flagged(Hd, Hr, s["th"], s["regs"], "H", "H.frames.last_partial_tile", ["H.frames.mdi_first_round"])


def test_comparator_names_the_extra_row_left_behind(late):
    """Row F - 1 (the VALU row of hstep_p1_xrow) keeps V_{N-1} in every frame."""
    s = late
    if s["kind"] != "01":
        return
    Vf = s["V"].copy()
    Vf[-1] = s["Vprev"][-1]
    Hd, Hr, Wd, Wr = _faulty_step(s, Vf)
    assert rel(Hd, Hr) < REL
    _flagged(Wd, Wr, s["tw"], s["regs"], "W", "W.rows.extra_valu", ["W.rows.mfma"])


def test_comparator_flags_a_pad_frame_in_the_statistics(lib):
    """T = 300 is not a multiple of 32: a pad frame of V that is not zero enters the sums over the frames wherever its H column is
    not zero either.  Modelled as one more frame (a stale copy of the last one) in the W statistics."""
    from se_snmf_nat_amd.api import geometry_describe
    F, T, r, beta, S = 65, 300, 9, 1.0, 0.5
    desc = geometry_describe(F, T, r, beta=beta, n_cu=256)
    rs, V, W0, H0 = _problem(F, T, r, 7)
    M = make_mask("01", F, T, rs)
    W, H = _normalised(W0, H0)
    Vt = mdi_start(V, M)
    for _k in range(2):
        Vt, W, H, _fl = mdi_step(Vt, M, W, H, beta, S, "full")
    Hn = ref_hstep(Vt, W, H, beta, S, exact_v=True)[0]
    tw = tau_w_mdi(F, r, beta, chain_t(desc, T), 3)
    Wr = ref_wstep(Vt, W, Hn, beta, exact_v=True)[0]
    Wd = ref_wstep(np.c_[Vt, Vt[:, -1]], W, np.c_[Hn, Hn[:, -1]], beta, exact_v=True)[0]
    regs = mdi_regions(desc, F, T, r)
    compare(_noisy(Wr, tw, np.random.default_rng(2)), Wr, tw, regs, "W")
    _flagged(_noisy(Wd, tw, np.random.default_rng(2)), Wr, tw, regs, "W", "W.all")


def test_vmdi_comparator(lib):
    F, T, r = 65, 90, 9
    rs, V, W0, H0 = _problem(F, T, r, 9)
    for kind in ("01", "soft"):
        M = make_mask(kind, F, T, rs)
        W, H = _normalised(W0, H0)
        Vt = mdi_start(V, M)
        for _k in range(3):
            Vt, W, H, _fl = mdi_step(Vt, M, W, H, 1.0, 0.5, "full")
        ref, Nt = mdi_final(Vt, M, W, H)
        tau = tau_vmdi(r, 3)
        dev = _noisy(ref, tau, np.random.default_rng(3))
        obs = M == 1.0
        dev[obs] = np.fmax(V, np.float32(FLR))[obs]
        worst, _ij, rms = compare_vmdi(dev, ref, V, M, tau)
        assert 0 < rms <= worst <= tau
        bad = dev.copy()
        bad[~obs[:, 17], 17] *= 1.0 + 1e-4  # one frame's Nt
        assert rel(bad, ref) < REL
        with pytest.raises(AssertionError, match=r"in 1 frames \(first \[17\]\)"):
            compare_vmdi(bad, ref, V, M, tau)
        if kind == "01":
            bad = dev.copy()
            f = int(np.nonzero(obs[:, 5])[0][0])
            bad[f, 5] = np.nextafter(np.float32(bad[f, 5]), np.float32(np.inf))
            with pytest.raises(AssertionError, match="observed entries"):
                compare_vmdi(bad, ref, V, M, tau)
    ones = np.ones((F, T))
    assert compare_vmdi(np.fmax(V, np.float32(FLR)), mdi_final(mdi_start(V, ones), ones, W, H)[0], V, ones, 0.0)[0] == 0.0
    assert mask_image(np.float64(0.1)) != 0.1
