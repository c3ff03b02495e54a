"""The rules behind tests/test_gpu_elementwise.py, checked without a device: the fp64 one-step restatement equals the oracle, the
case table selects and covers every kernel family it names (through snmf_plan_geometry_describe), and the element-wise comparator
catches a 1e-3 error in one small region that the whole-matrix criterion of the trajectory tests lets through."""
import numpy as np
import pytest

from elementwise import (CASES, FLR, case_masks, chain_t, compare, family, ref_hstep, ref_wstep, regions, rel, tau_h, tau_w,
                         wstats_remainder_shared)
from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf

BETAS = [0.0, 0.5, 1.0, 1.5, 2.0]
MODES = ["full", "h", "w", "semi"]
FORMS = ["scalar", "rvec", "entry", "zero"]


def _sparsity(form, r, T, rs):
    return {"scalar": 0.7, "zero": 0.0, "rvec": rs.uniform(0.0, 2.0, r), "entry": rs.uniform(0.0, 2.0, (r, T))}[form]


def _problem(F, T, r, seed):
    rs = np.random.default_rng(seed)
    V = (rs.gamma(0.5, 1.0, (F, 6)) @ rs.gamma(0.3, 1.0, (6, T)) + 1e-3).astype(np.float32)
    return rs, V, rs.random((F, r)), rs.random((r, T)).astype(np.float32)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("beta", BETAS)
def test_one_step_restatement_equals_the_oracle(beta, mode, form):
    F, T, r = 37, 53, 7
    rs, V, W0, H0 = _problem(F, T, r, 11)
    S = _sparsity(form, r, T, rs)
    w_ind, h_ind = case_masks(mode, r)
    p = dict(cf="beta", beta=beta, sparsity=S, max_iter=1, cost_check=1, init_w=W0, init_h=H0.astype(np.float64))
    if w_ind is not None:
        p["w_update_ind"] = w_ind
    if h_ind is not None:
        p["h_update_ind"] = h_ind
    w_o, h_o, _ = oracle_nmf(V.astype(np.float64), p)
    wn = np.sqrt((W0 ** 2).sum(0))
    W, H = W0 / wn, H0.astype(np.float64) * wn[:, None]  # src/sparse_nmf.m:157-160
    if mode != "w":
        H, _ = ref_hstep(V, W, H, beta, S)
    if mode != "h":
        W, _ = ref_wstep(V, W, H, beta, w_ind)
    np.testing.assert_allclose(H, h_o, rtol=1e-12)
    np.testing.assert_allclose(W, w_o, rtol=1e-12)


def test_gram_form_equals_the_plain_form_where_no_floor_binds():
    rs, V, W0, H0 = _problem(65, 300, 20, 3)
    W = W0 / np.sqrt((W0 ** 2).sum(0))
    for w_ind in (None, case_masks("semi", 20)[0]):
        a, ia = ref_wstep(V, W, H0, 2.0, w_ind, gram=True)
        b, ib = ref_wstep(V, W, H0, 2.0, w_ind, gram=False)
        assert ia["lam"] > 10 * FLR and ib["dpw"] > 10 * FLR
        np.testing.assert_allclose(a, b, rtol=1e-12)


# ---- the case table ------------------------------------------------------------------------------------------------------------

def _describe(c):
    from se_snmf_nat_amd.api import geometry_describe
    w, h = case_masks(c["mode"], c["r"])
    return geometry_describe(c["F"], c["T"], c["r"], beta=c["beta"], n_cu=256, w_update_ind=w, h_update_ind=h)


@pytest.fixture(scope="module")
def described(lib):
    return {c["id"]: _describe(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_each_case_selects_its_family_and_regions(described, case):
    desc = described[case["id"]]
    for tok in case["tokens"]:
        assert tok in desc, (case["id"], tok, desc)
    regs = regions(desc, case["F"], case["T"], case["r"], case["mode"])
    for name in case["expect"]:
        assert name in regs and len(regs[name][2]) > 0, (case["id"], name, sorted(regs))
    for name, (_m, axis, idx) in regs.items():  # indices inside the matrix
        n = {("W", 0): case["F"], ("W", 1): case["r"], ("H", 0): case["r"], ("H", 1): case["T"]}[(_m, axis)]
        assert len(idx) == 0 or (idx.min() >= 0 and idx.max() < n), (case["id"], name)
    # a bound exactly where the mode updates the factor, and below the 1e-3 that the comparator tests inject into one element
    th = tau_h(case["F"], case["r"], case["beta"], case["mode"])
    tw = tau_w(case["F"], case["r"], case["beta"], chain_t(desc, case["T"]), case["mode"])
    assert (th is None) == (case["mode"] == "w") and (tw is None) == (case["mode"] == "h"), case["id"]
    assert all(t < 1e-3 for t in (th, tw) if t is not None), (case["id"], th, tw)


def _rp_geometry(desc):
    import re
    m = re.search(r"(\d+) of (\d+) tiles pipelined, last round split (\d+) ways, grid (\d+)", desc)
    return tuple(int(x) for x in m.groups())


def test_case_table_covers_every_family(described):
    by = {c["id"]: (c, described[c["id"]]) for c in CASES}
    text = " ".join(described.values())
    for tok in ("k_hstep_rp (", "split 2 ways", "split 4 ways", "P2 cut four ways over the contraction;",
                "P2 in wave pairs cut over the contraction;", "k_hstep_rh (", "leftover columns as 4x4x1 MFMAs",
                "on half tiles;", "hstep: k_hstep,", "NK=4 ", "NK=8 ", "NK=16 ", "2 kgroups", "Gram matrix", "k_iter_sf (",
                "remainder tile shared by the four pairs", "k_hstep_sf (", "k_wstats_sf", "single remainder tile shared by the eight waves",
                "k_hstep_sr (", "k_wstats_sr", "W finish (run loop): k_wfin", "on the H step's last workgroup", "out-of-envelope"):
        assert tok in text, tok

    def cases(pred):
        return [(c, d) for c, d in by.values() if pred(c, d)]

    # k_hstep_rp: >= 3 tiles per workgroup, the extra row at F = 65, 257, 513
    rp = cases(lambda c, d: family(d) == "k_hstep_rp")
    assert any(_rp_geometry(d)[1] >= 3 * _rp_geometry(d)[3] for _c, d in rp)
    assert {65, 257, 513} <= {c["F"] for c, d in rp if "(+1 VALU row)" in d}
    # k_hstep_rh: leftover columns in both forms
    lx = {c["r"] for c, d in cases(lambda c, d: "leftover columns" in d)}
    assert lx & set(range(97, 101)) and lx & set(range(193, 201))
    assert cases(lambda c, d: c["F"] == 449 and c["T"] == 9000 and c["r"] == 250 and "on half tiles;" in d)
    # the plain k_hstep: fewer tiles than workgroups, W-only, beta = 0 / 0.5 / 1.5 / 2 at F = 33 / 64 / 257 / 513
    plain = cases(lambda c, d: family(d) == "k_hstep")
    assert any((c["T"] + 31) // 32 < 256 and c["mode"] != "w" for c, _d in plain)
    assert any(c["mode"] == "w" for c, _d in plain)
    assert {(0.0, 33), (0.5, 64), (1.5, 257), (2.0, 513)} <= {(c["beta"], c["F"]) for c, _d in plain if c["mode"] != "w"}
    # the W statistics: two matrices (beta != 1) and the Euclidean Gram form on W updates
    assert cases(lambda c, d: c["beta"] not in (1.0, 2.0) and c["mode"] != "h")
    assert cases(lambda c, d: "Gram matrix" in d and c["beta"] == 2.0 and c["r"] < 2 * c["F"])
    # small F: tiles shared by four waves (1025..1279 tiles), the single remainder tile of k_wstats_sf in some chunk
    assert cases(lambda c, d: "k_hstep_sf (" in d and "the last 0 shared" not in d and 1025 <= (c["T"] + 31) // 32 <= 1279)
    assert any(wstats_remainder_shared(d, c["T"]) for c, d in by.values())
    # small rank: k_wfin's row slices (r <= 32, a W update)
    assert cases(lambda c, d: c["r"] <= 32 and c["mode"] != "h" and "W finish (run loop): k_wfin" in d)
    # the two H-only objective folds: on the H step's last workgroup, and k_reduce (the out-of-envelope path folds no objective)
    assert cases(lambda c, d: c["mode"] == "h" and "on the H step's last workgroup" in d)
    assert cases(lambda c, d: c["mode"] == "h" and "out-of-envelope" in d)
    # the out-of-envelope shapes and the headline
    for F, T, r, beta, mode in ((2700, 700, 40, 1.0, "full"), (2600, 300, 24, 1.5, "full"), (129, 5000, 1100, 1.0, "w"),
                                (257, 100000, 256, 1.0, "full")):
        assert cases(lambda c, d: (c["F"], c["T"], c["r"], c["beta"], c["mode"]) == (F, T, r, beta, mode)), (F, T, r)
    # partial last tiles of both kinds, and the data variants
    assert {1, 31} <= {c["T"] % 32 for c in (x for x, _d in by.values())}
    assert cases(lambda c, d: c["data"] == "wide" and c["beta"] not in (1.0, 2.0))
    assert cases(lambda c, d: c["data"] == "quiet" and "Gram matrix" in d)
    # every H-step family with each sparsity form
    fams = {}
    for c, d in by.values():
        if c["mode"] != "w":
            fams.setdefault(family(d), set()).add(c["sp"])
    assert set(fams) == {"k_hstep_rp", "k_hstep_rh", "k_hstep", "k_hstep_sf", "k_iter_sf", "k_hstep_sr", "out-of-envelope"}
    for f, forms in fams.items():
        assert forms == set(FORMS), (f, forms)


# ---- the comparator ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def step(lib):
    """An fp64 H and W step on the geometry of 513 x 9023, r = 97 (k_hstep_rh: the extra VALU row, leftover 4x4x1 columns, the
    split last round, a partial last tile)."""
    from se_snmf_nat_amd.api import geometry_describe
    F, T, r = 513, 9023, 97
    desc = geometry_describe(F, T, r, beta=1.0, n_cu=256)
    rs, V, W0, H0 = _problem(F, T, r, 5)
    W = W0 / np.sqrt((W0 ** 2).sum(0))
    Hr, ih = ref_hstep(V, W, H0, 1.0, 1.0)
    Wr, iw = ref_wstep(V, W, Hr, 1.0)
    return dict(desc=desc, regs=regions(desc, F, T, r), Hr=Hr, Wr=Wr, ih=ih, iw=iw, th=tau_h(F, r, 1.0),
                tw=tau_w(F, r, 1.0, chain_t(desc, T)), rs=rs, F=F, T=T, r=r)


def _noisy(ref, tau, rs):
    """fp32 rounding plus relative noise at the bound's typical size (a quarter of it)."""
    return (ref * (1.0 + rs.uniform(-0.25, 0.25, ref.shape) * tau)).astype(np.float32).astype(np.float64)


def test_comparator_passes_rounding_noise(step):
    rs = np.random.default_rng(0)
    st = compare(_noisy(step["Hr"], step["th"], rs), step["Hr"], step["th"], step["regs"], "H", floors=step["ih"])
    assert {"H.frames.split_round", "H.frames.last_partial_tile", "H.comp.leftover_4x4x1"} <= set(st)
    st = compare(_noisy(step["Wr"], step["tw"], rs), step["Wr"], step["tw"], step["regs"], "W", floors=step["iw"])
    assert "W.rows.extra_valu" in st


def _inject(step, matrix, where, region, spared):
    rs = np.random.default_rng(1)
    ref = step[matrix + "r"]
    tau = step["th"] if matrix == "H" else step["tw"]
    dev = _noisy(ref, tau, rs)
    dev[where] *= 1.0 + 1e-3
    # the whole-matrix criterion of the trajectory tests (test_gpu_parity.REL_WH) lets it through: why this module exists
    assert rel(dev, ref) < 1e-4
    with pytest.raises(AssertionError) as e:
        compare(dev, ref, tau, step["regs"], matrix)
    msg = str(e.value)
    assert f"region {region}:" in msg, msg
    for s in spared:
        assert f"region {s}:" not in msg, msg


def test_comparator_names_one_frame_of_the_last_partial_tile(step):
    t = step["T"] - 3
    _inject(step, "H", (slice(None), t), "H.frames.last_partial_tile", ["H.frames.pipelined"])


def test_comparator_names_one_split_round_tile(step):
    n_full = _rp_geometry(step["desc"])[0]
    t = 32 * n_full + 40
    assert t < 32 * (step["T"] // 32)  # (not the partial last tile)
    _inject(step, "H", (slice(None), t), "H.frames.split_round", ["H.frames.pipelined", "H.frames.last_partial_tile"])


def test_comparator_names_the_extra_w_row(step):
    _inject(step, "W", (step["F"] - 1, slice(None)), "W.rows.extra_valu", ["W.rows.mfma"])


def test_comparator_names_one_leftover_component_in_one_tile(step):
    _inject(step, "H", (step["r"] - 1, slice(64, 96)), "H.comp.leftover_4x4x1", ["H.comp.full_tiles"])


def test_comparator_refuses_what_the_bound_does_not_cover(step):
    ref = step["Hr"].copy()
    with pytest.raises(AssertionError, match="floor on lam"):
        compare(ref, ref, step["th"], step["regs"], "H", floors={"lam": 5e-9})
    ref[0, 0] = 0.0
    with pytest.raises(AssertionError, match="entry <= 0"):
        compare(ref, ref, step["th"], step["regs"], "H")


@pytest.mark.parametrize("F,T,r,beta,t_c", [
    (257, 100000, 256, 1.0, 832),   # group-1 chunks 125 (two row groups dealt unevenly): 3125 tiles -> 25 per chunk, + 1
    (289, 20000, 40, 1.0, 192),     # 128 chunks: 625 tiles -> 5 per chunk, + 1
    (513, 9000, 193, 1.0, 192),     # 71 chunks for row group 0, 61 for the others: 282 tiles -> 5, + 1
    (129, 20000, 250, 2.0, 192),    # 256 statistics chunks, but the Gram launch deals over 256 / ceil(8 col tiles / 4 waves) = 128
    (257, 4000, 400, 2.0, 96),      # NK = 16: the Euclidean Q launch on ceil(13 / 8) = 2 kappa-groups x 2 fgroups -> 64 chunks
    (513, 60000, 512, 2.0, 1920),   # ... 256 / (4 fgroups x 2 kappa-groups) = 32 chunks: 1875 tiles -> 59, + 1
    (2700, 700, 40, 1.0, 700),      # out of envelope: chunks of 2048 frames (kGChunkT), here the whole T
    (129, 5000, 1100, 1.0, 2048),
])
def test_chain_length_follows_the_plan_geometry(lib, F, T, r, beta, t_c):
    """T_c restates the statistics' chunk grids of csrc/snmf_tu_geometry.hip (n_chunks / n_ch1, gram_chunks, kq_chunks) and
    csrc/snmf_generic.h: pinned here, worked out by hand from the plans' describe() numbers."""
    from se_snmf_nat_amd.api import geometry_describe
    assert chain_t(geometry_describe(F, T, r, beta=beta, n_cu=256), T) == t_c


def test_bounds_grow_with_every_chain_they_count():
    F, r = 257, 100
    for mode in ("full", "semi"):
        assert tau_w(F, r, 1.0, 64, mode) < tau_w(F, r, 1.0, 832, mode) < tau_w(F, r, 1.0, 2048, mode)
        assert tau_w(F, r, 1.0, 64, mode) < tau_w(2 * F, r, 1.0, 64, mode) and tau_w(F, r, 1.0, 64, mode) < tau_w(F, 2 * r, 1.0, 64, mode)
    assert tau_h(F, r, 1.0) < tau_h(2 * F, r, 1.0) and tau_h(F, r, 1.0) < tau_h(F, 2 * r, 1.0)
    # powf(Lam, beta - 1) and powf(Lam, beta - 2) scale Lam's error by their exponents: Itakura-Saito (-1, -2) > beta = 0.5 > KL
    assert tau_h(F, r, 0.0) > tau_h(F, r, 0.5) > tau_h(F, r, 1.0) == tau_h(F, r, 1.5) == tau_h(F, r, 2.0)
    assert tau_w(F, r, 0.0, 64) > tau_w(F, r, 1.0, 64) == tau_w(F, r, 2.0, 64)
    # no bound for a factor the mode leaves alone
    assert tau_h(F, r, 1.0, "w") is None and tau_w(F, r, 1.0, 64, "h") is None
