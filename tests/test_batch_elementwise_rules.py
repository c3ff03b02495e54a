"""The rules behind tests/test_gpu_batch_elementwise.py, checked without a device: the case table reaches every instantiation of
the batch kernels (through a restatement of snmf_batch_create's geometry function), the fp64 reference satisfies the comparator's
conditions on every problem of every case, the reference iteration equals the oracle's, and the element-wise comparator rejects
the errors batch geometry can make -- built as mutants of the fp64 reference -- naming the region and the problem, where the
whole-matrix criterion of tests/test_gpu_batch.py (REL_WH) lets them through."""
import functools

import numpy as np
import pytest

from batch_elementwise import (CASES, T_EDGES, batch_chain_t, batch_geometry, batch_regions, case_masks, mirror_geometry, normalised,
                               reference_steps)
from elementwise import FLR, compare, ref_hstep, ref_wstep, rel, tau_h, tau_w
from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf

REL_WH = 1e-4  # test_gpu_parity.REL_WH, the criterion of tests/test_gpu_batch.py


# ---- the describe() text and the geometry function -----------------------------------------------------------------------------

# snmf_batch_describe's text for F = 513, r = 200, Itakura-Saito, T = (100, 300, 63) (csrc/snmf_tu_batch.hip)
SAMPLE = ("batch B=3 F=513 r=200 beta upd_h=1 upd_w=1 xr=1 nf=16 nk=7 tiles=16 chunks=8 | k_bh grid=16 x512 lds=97920 cf=8 S=1 | "
          "k_bw grid=(8,4,2) x512 lds=65024 NA=2 | k_bfin grid=(200,3) x256 | poll_every=8")


def test_describe_text_is_parsed_and_equals_the_mirror():
    g = batch_geometry(SAMPLE)
    assert g == mirror_geometry(513, 200, 0.0, (100, 300, 63))
    assert (g["xr"], g["nf"], g["nk"], g["cf"], g["S"], g["n_fg"], g["n_kg"], g["NA"], g["tiles"], g["chunks"]) == (1, 16, 7, 8, 1, 4, 2, 2, 16, 8)
    assert (g["nfg"], g["nkg"], g["passes"]) == (4, 4, 2)
    with pytest.raises(AssertionError):  # group counts that do not follow from nf / nk are refused
        batch_geometry(SAMPLE.replace("grid=(8,4,2)", "grid=(8,3,2)"))
    # appended tokens do not disturb it
    assert batch_geometry(SAMPLE + " | nfg=4 nkg=4") == g


def test_chain_length_is_one_chunk():
    assert [batch_chain_t(T) for T in (1, 31, 63, 64, 65, 257, 10000)] == [1, 31, 63, 64, 64, 64, 64]


@functools.lru_cache(maxsize=None)
def _geoms():
    return {c["id"]: mirror_geometry(c["F"], c["r"], c["beta"], c["Ts"]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_each_case_reaches_what_it_is_listed_for(case):
    g = _geoms()[case["id"]]
    for k, v in case["expect"].items():
        assert g[k] == v, (case["id"], k, g[k], v)
    Ts = case["Ts"]
    assert 6 <= len(Ts) <= 8 and set(Ts) <= set(T_EDGES), Ts
    assert any(T < 8 for T in Ts) and any(T % 32 == 0 for T in Ts) and any(T in (257, 513) for T in Ts), Ts
    assert any(T % 32 for T in Ts[:-1]), Ts  # a partial tile followed by another problem's first tile
    assert sum(T >= 256 for T in Ts) == 2, Ts  # the two problems the GPU test also steps on a single Plan
    assert g["tiles"] == sum(-(-T // 32) for T in Ts) and g["chunks"] == sum(-(-T // batch_chain_t(10 ** 6)) for T in Ts)
    w_ind, h_ind = case_masks(case["mode"], case["r"])
    assert (h_ind is None or not h_ind.any()) and (w_ind is None or len(w_ind) == case["r"])  # (a batch takes no partial h_update_ind)
    th, tw = tau_h(case["F"], case["r"], case["beta"], case["mode"]), tau_w(case["F"], case["r"], case["beta"], batch_chain_t(513), case["mode"])
    assert (th is None) == (case["mode"] == "w") and (tw is None) == (case["mode"] == "h")
    assert all(t < 1e-3 for t in (th, tw) if t is not None)  # (a structural error of ~1/F stands above it)
    for T in Ts:
        regs = batch_regions(g, case["F"], T, case["r"], case["mode"])
        for name, (m, axis, idx) in regs.items():
            n = {("W", 0): case["F"], ("W", 1): case["r"], ("H", 0): case["r"], ("H", 1): T}[(m, axis)]
            assert len(idx) > 0 and idx.min() >= 0 and idx.max() < n and len(set(idx.tolist())) == len(idx), (case["id"], T, name)
        # the row groups / column groups / wave sets partition their axis
        for prefix, n in (("W.rows.fgroup", case["F"]), ("W.comp.kgroup", case["r"]), ("H.comp.ktile", case["r"])):
            got = np.sort(np.concatenate([v[2] for k, v in regs.items() if k.startswith(prefix)]))
            assert np.array_equal(got, np.arange(n)), (case["id"], prefix)
        assert ("H.frames.last_partial_tile" in regs) == (T % 32 != 0) and ("H.frames.full_tiles" in regs) == (T >= 32)
        assert ("W.rows.extra_valu" in regs) == bool(g["xr"])
        assert ("W.comp.fixed" in regs) == (case["mode"] == "semi")


def test_case_table_reaches_every_instantiation():
    gs = [(c, _geoms()[c["id"]]) for c in CASES]
    kl = [(c, g) for c, g in gs if c["beta"] == 1.0]
    other = [(c, g) for c, g in gs if c["beta"] != 1.0]
    upd_w = lambda c: c["mode"] != "h"  # noqa: E731  (k_bw runs)
    upd_h = lambda c: c["mode"] != "w"  # noqa: E731  (k_bh updates)
    # every instantiation of k_bw: NA = 1, 2, 4, 8 for KL, NA = 1, 2 for both other modes' code (BM_EUC, BM_GEN)
    assert {g["NA"] for c, g in kl if upd_w(c)} == {1, 2, 4, 8}
    assert {g["NA"] for c, g in other if c["beta"] == 2.0 and upd_w(c)} == {1, 2}
    assert {g["NA"] for c, g in other if c["beta"] != 2.0 and upd_w(c)} == {1, 2}
    assert {c["beta"] for c, _g in gs} == {0.0, 0.5, 1.0, 1.5, 2.0}
    # every column-tile count and with it every cut of the W' * ratio contraction (S = 8, 4, 2, 1)
    assert {g["nk"] for _c, g in gs} == set(range(1, 8))
    assert {g["S"] for c, g in gs if upd_h(c)} == {8, 4, 2, 1}
    # one and two passes over the ratio image; the extra row in the last of two passes, once beside a single tile (nf = 9)
    assert {g["passes"] for c, g in other if upd_h(c)} == {1, 2}
    assert any(g["passes"] == 2 and g["xr"] and g["nf"] % g["cf"] == 1 for c, g in other)
    assert any(g["passes"] == 2 and g["xr"] and g["nf"] % g["cf"] == 0 for c, g in other)
    # row groups and column groups of k_bw
    assert {g["n_fg"] for c, g in kl} == {1, 2} and {g["n_fg"] for c, g in other} >= {1, 3, 4}
    assert any(g["n_kg"] == 2 for c, g in other) and any(g["n_kg"] == 2 and g["nk"] % g["nkg"] == 1 for c, g in other)
    assert any(g["n_fg"] == 2 and g["nf"] - g["nfg"] == 2 for c, g in kl)  # a second row group with ntf = 2
    # KL with F > 256 together with r > 128: the largest KL instantiation, two row groups, NA = 8, the extra row
    assert any(g["n_fg"] == 2 and g["NA"] == 8 and g["xr"] and c["mode"] == "full" for c, g in kl)
    # the extra row with one row tile and with sixteen; partial row tiles; the degenerate corner
    assert {g["nf"] for c, g in gs if g["xr"]} >= {1, 16}
    assert any(not g["xr"] and c["F"] % 32 for c, g in gs) and any(c["F"] == 1 and c["r"] == 1 for c, g in gs)
    assert any(c["r"] % 32 == 0 for c, g in gs) and any(c["r"] < 8 for c, g in gs)
    # every update pattern, sparsity form and data variant
    assert {c["mode"] for c, _g in gs} == {"full", "h", "w", "semi"}
    assert {c["sp"] for c, _g in gs} == {"scalar", "zero", "rvec"}
    assert all(c["data"] == "wide" for c, _g in gs if c["beta"] not in (1.0, 2.0))
    assert set().union(*(c["Ts"] for c, _g in gs)) == set(T_EDGES)


# ---- conditions on the inputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_reference_satisfies_the_comparators_conditions(case):
    """compare()'s preconditions, from the fp64 reference alone: every entry > 0 and every floor (on Lam, dph, dpw) more than
    10x above 1e-9, on every problem and every step.  Conditions on the inputs, not measurements."""
    for b, steps in enumerate(reference_steps(case["id"])):
        assert len(steps) == case["steps"] == 3
        for k, (Hn, ih, Wn, iw) in enumerate(steps, 1):
            assert (Hn > 0).all() and (Wn > 0).all() and np.isfinite(Hn).all() and np.isfinite(Wn).all(), (case["id"], b, k)
            assert (Hn.astype(np.float32) >= 2.0 ** -100).all(), (case["id"], b, k)  # (far from fp32's subnormals)
            for info in (ih, iw):
                for name, v in (info or {}).items():
                    assert v > 10 * FLR, (case["id"], b, k, name, v)


# ---- agreement with the oracle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("beta,sp", [(1.0, "scalar"), (2.0, "rvec"), (0.0, "zero"), (0.5, "rvec")])
def test_reference_iteration_equals_the_oracle(beta, sp):
    rs = np.random.default_rng(17)
    F, T, r = 33, 41, 5
    V = (rs.gamma(0.5, 1.0, (F, 6)) @ rs.gamma(0.3, 1.0, (6, T)) + 1e-3).astype(np.float32)
    W0, H0 = rs.random((F, r)), rs.random((r, T))
    S = {"scalar": 0.7, "zero": 0.0, "rvec": rs.uniform(0.0, 2.0, r)}[sp]
    w_o, h_o, _ = oracle_nmf(V.astype(np.float64), dict(cf="beta", beta=beta, sparsity=S, max_iter=1, cost_check=1, init_w=W0, init_h=H0))
    wn = np.sqrt((W0 ** 2).sum(0))
    H, _ = ref_hstep(V, W0 / wn, H0 * wn[:, None], beta, S)
    W, _ = ref_wstep(V, W0 / wn, H, beta)
    np.testing.assert_allclose(H, h_o, rtol=1e-12)
    np.testing.assert_allclose(W, w_o, rtol=1e-12)


# ---- the test would fail on a subtly wrong kernel ------------------------------------------------------------------------------
#
# A batch of five KL problems at F = 65 (the extra row), r = 40 (two wave sets of k_bh), T = (31, 513, 33, 4097, 9).  Problem 1
# has nine chunks, the last of one tile with one frame, and its 31 padded frames are followed by problem 2's first tile; its
# state is that of a solve near convergence (300 reference iterations: consecutive iterates differ by ~1e-3, what the trajectory
# tests compare at the end of their runs).  Problem 3 is a long one (65 chunks, the last again of one frame).  The others are a
# solve under way (30 iterations).

MF, MR, MTS, MBETA, MS = 65, 40, (31, 513, 33, 4097, 9), 1.0, 1.0
M_WARM = (30, 300, 30, 10, 30)


@functools.lru_cache(maxsize=None)
def _mut():
    geom = mirror_geometry(MF, MR, MBETA, MTS)
    probs = []
    for b, T in enumerate(MTS):
        rs = np.random.default_rng(100 + b)
        V = (rs.gamma(0.5, 1.0, (MF, 16)) @ rs.gamma(0.3, 1.0, (16, T)) + 1e-3).astype(np.float32)
        W, H = normalised(rs.random((MF, MR)), rs.random((MR, T)))
        Hpp = H
        for _ in range(M_WARM[b]):
            Hpp = H
            H = ref_hstep(V, W, H, MBETA, MS)[0].astype(np.float32)
            W = ref_wstep(V, W, H, MBETA)[0]
        Hr, ih = ref_hstep(V, W, H, MBETA, MS)
        Hn = Hr.astype(np.float32)
        Wr, iw = ref_wstep(V, W, Hn, MBETA)
        probs.append(dict(V=V.astype(np.float64), W=W, H=H.astype(np.float64), Hpp=Hpp.astype(np.float64), Hr=Hr, Hn=Hn.astype(np.float64),
                          Wr=Wr, ih=ih, iw=iw, T=T, regs=batch_regions(geom, MF, T, MR)))
    return geom, probs, tau_h(MF, MR, MBETA), tau_w(MF, MR, MBETA, batch_chain_t(max(MTS)))


def _hstep_kl(p, ratio_of=None, rows=slice(None)):
    """ref_hstep for KL on the mutant batch's state, with a hook on the ratio image that components `rows` contract."""
    lam = np.fmax(p["W"] @ p["H"], FLR)
    ratio = p["V"] / lam
    Hn = p["Hr"].copy()
    dph = p["W"].sum(0)[:, None] + MS
    Hn[rows] = (p["H"] * (p["W"].T @ (ratio if ratio_of is None else ratio_of(ratio))) / dph)[rows]
    return Hn


def _wstep_kl(p, V=None, H=None, s_extra=0.0):
    """ref_wstep for KL on the mutant batch's state, with other frames and an addition to the row sums of H."""
    V = p["V"] if V is None else V
    H = p["Hn"] if H is None else H
    W = p["W"]
    G = (V / np.fmax(W @ H, FLR)) @ H.T
    s = (H.sum(1) + s_extra)[None, :]
    Wn = W * (G + np.sum(s * W, axis=0)[None, :] * W) / (s + np.sum(G * W, axis=0)[None, :] * W)
    return Wn / np.sqrt(np.sum(Wn ** 2, axis=0))


def _rejects(b, matrix, dev, named, spared=(), diluted=None):
    _geom, probs, th, tw = _mut()
    p = probs[b]
    ref, tau, floors = (p["Hr"], th, p["ih"]) if matrix == "H" else (p["Wr"], tw, p["iw"])
    compare(ref.astype(np.float32), ref, tau, p["regs"], matrix, floors=floors, what=f"problem {b}")  # the unmutated step passes
    if diluted is not None:  # the whole-matrix criterion of tests/test_gpu_batch.py: the gap this module closes
        assert (rel(dev, ref) < REL_WH) == diluted, rel(dev, ref)
    with pytest.raises(AssertionError) as e:
        compare(dev, ref, tau, p["regs"], matrix, floors=floors, what=f"mutant batch problem {b} (T={p['T']})")
    msg = str(e.value)
    assert f"problem {b} (T={p['T']})" in msg, msg
    for name in named:
        assert f"region {name}:" in msg, msg
    for name in spared:
        assert f"region {name}:" not in msg, msg
    return msg


def test_helpers_restate_the_reference_step():
    _geom, probs, _th, _tw = _mut()
    for p in probs:
        np.testing.assert_allclose(_hstep_kl(p), p["Hr"], rtol=1e-13)
        np.testing.assert_allclose(_wstep_kl(p), p["Wr"], rtol=1e-13)


def test_mutant_last_chunk_left_out_of_w():
    """k_bfin sums n_chunks - 1 slabs: the last chunk (one frame of 513, of 4097) never reaches G or the row sums.  On the long
    problem the whole-matrix criterion lets it through."""
    for b, diluted in ((1, None), (3, True)):
        p = _mut()[1][b]
        n = p["T"] - 1
        _rejects(b, "W", _wstep_kl(p, V=p["V"][:, :n], H=p["Hn"][:, :n]), ["W.all", "W.rows.mfma", "W.comp.kgroup0"], diluted=diluted)


def test_mutant_one_block_of_the_contraction_dropped_from_h():
    """The wave set of columns 32..39 loses the 8-deep block of rows 24..31 of W' * ratio (a part that ends one block early)."""
    def drop(ratio):
        out = ratio.copy()
        out[24:32] = 0.0
        return out
    for b in range(5):
        _rejects(b, "H", _hstep_kl(_mut()[1][b], drop, rows=slice(32, 40)), ["H.all", "H.comp.ktile1", "H.comp.remainder"], ["H.comp.ktile0"],
                 diluted=False)


def test_mutant_extra_row_left_out_of_the_h_numerator():
    """qb without the + 1: row F - 1 of the ratio image is not contracted."""
    def drop(ratio):
        out = ratio.copy()
        out[MF - 1] = 0.0
        return out
    for b in range(5):
        _rejects(b, "H", _hstep_kl(_mut()[1][b], drop), ["H.all", "H.comp.ktile0", "H.comp.ktile1", "H.frames.first_tile"])


def test_mutant_last_partial_tile_from_the_previous_iterates_h():
    """The one-frame last tile of problem 1 is stepped from the other ping-pong buffer (H of iterate k - 2)."""
    p = _mut()[1][1]
    stale = dict(p, H=p["Hpp"])
    dev = p["Hr"].copy()
    dev[:, 512:] = _hstep_kl(stale)[:, 512:]
    _rejects(1, "H", dev, ["H.all", "H.frames.last_partial_tile"], ["H.frames.full_tiles", "H.frames.first_tile"], diluted=True)


def test_mutant_next_problems_first_frame_in_a_padded_frames_statistics():
    """The mask of a last tile lets one padded frame through: it holds the next problem's first frame (its V and its new H)."""
    _geom, probs, _th, _tw = _mut()
    for b, named, diluted in ((0, ["W.all", "W.rows.extra_valu"], False), (1, ["W.all"], None)):
        p, nxt = probs[b], probs[b + 1]
        dev = _wstep_kl(p, V=np.hstack([p["V"], nxt["V"][:, :1]]), H=np.hstack([p["Hn"], nxt["Hn"][:, :1]]))
        _rejects(b, "W", dev, named, diluted=diluted)


def test_mutant_row_sums_of_h_over_32_frames():
    """`hs` runs over the 32 frames of the tile instead of Tl: the padded frames' slots hold the next problem's H."""
    _geom, probs, _th, _tw = _mut()
    for b in (0, 1):
        p, nxt = probs[b], probs[b + 1]
        n_pad = 32 * (-(-p["T"] // 32)) - p["T"]
        assert n_pad in (1, 31)
        _rejects(b, "W", _wstep_kl(p, s_extra=nxt["Hn"][:, :n_pad].sum(1)), ["W.all", "W.comp.kgroup0"], diluted=False)
