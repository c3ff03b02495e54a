"""Element-wise judgement of ONE step of the batched offline solve (csrc/snmf_batch.h: k_bh, k_bw, k_bfin, k_bfold; host driver
csrc/snmf_tu_batch.hip).  Test infrastructure like tests/elementwise.py, whose fp64 step, bounds and comparator it imports: no test
functions here; imported by tests/test_batch_elementwise_rules.py (CPU) and tests/test_gpu_batch_elementwise.py (GPU).

WHY.  tests/test_gpu_batch.py holds every problem of a batch to the oracle with one Frobenius norm per matrix after 6 to 80
iterations.  What batch geometry can get wrong sits in one frame, one row or one tile of one problem -- the last partial tile, a
frame leaked across a problem boundary, a dropped 8-deep block of the extra row, a chunk slab left out of k_bfin's sum -- and that
norm dilutes it by the square root of the matrix size (tests/elementwise.py, "WHY ONE STEP AND NOT A TRAJECTORY").  Here every
problem of a batch is stepped from the device's own state and judged per element, region by region.

THE BOUNDS are those of tests/elementwise.py, unchanged: tau_h(F, r, beta) and tau_w(F, r, beta, T_c) with
T_c = batch_chain_t(T_b) = min(T_b, 64).  Both are derived worst cases (not fitted); every term they count still covers the
batch kernels:

  - Lam is an r-term MFMA chain over the fp32 image of W (b_lam_tile; the extra row: sixteen strided partial sums and a
    four-level tree, b_extra_row): (r + 2) u as counted.
  - k_bh forms the ratio image with fast_rcp / OCML powf as the single solver does, and contracts it with W over F rows in S
    partial chains added in part order (any order: at most (F - 1) u).  It then divides by `dp` with a TRUE division
    (ho * num / dp: a product and a quotient, u each) where the count allows a reciprocal and a product (2u + u): tighter.
  - for KL `dp` is colsum + sparsity: colsum is the fp32 image of an fp64 sum of the master copy (k_bfin), one rounding, where
    the count allows an F-term fp32 chain.  For beta != 1 `dp` is the contraction of the denominator image, as counted.
  - k_bw accumulates the statistics of one chunk of kBChunkTiles * 32 = 64 frames in MFMA chains (G, or P and Q), and the
    extra-row statistic `gxq` / `gxp` and the row sums `hs` of H as sequential fp32 sums over the same at most 64 frames:
    T_c = min(T_b, 64) terms each, as counted.  The slabs of a problem's chunks are then added in chunk order in fp64.
  - k_bfin's epilogue (sum(G .* w), sum(s .* w), the update, the norm) is fp64 on the fp64 master, where the count allows three
    F-term fp32 chains: over-covered.

THE REGIONS follow the geometry that snmf_batch_create derives and BatchPlan.describe() prints: batch_geometry() parses the
text, mirror_geometry() restates the function (the CPU rules hold the case table to it; the GPU test holds every describe() to
it).
"""
from __future__ import annotations

import functools
import re

import numpy as np

from elementwise import FLR, U, case_data, compare, cost_of, ref_hstep, ref_wstep, tau_h, tau_w  # noqa: F401 (re-exported)

B_CHUNK_TILES = 2   # kBChunkTiles, csrc/snmf_batch.h: 32-frame tiles per W-statistics chunk
B_WAVES = 8         # kBW: waves per workgroup of k_bh / k_bw
# the edges of the tile logic (32) and of problems of 8, 9, 10 and 17 tiles: whole chunks, a last chunk of one tile, one frame in it
T_EDGES = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 289, 513)


def batch_chain_t(T):
    """T_c of a problem of T frames: the longest fp32 chain over frames in k_bw is one chunk of kBChunkTiles * 32 frames; the
    slabs are added in fp64 by k_bfin (module docstring)."""
    return min(int(T), 32 * B_CHUNK_TILES)


def _mode_of(beta):
    return "kl" if beta == 1.0 else ("ed" if beta == 2.0 else "beta")


def mirror_geometry(F, r, beta, Ts):
    """The geometry function of snmf_batch_create (csrc/snmf_tu_batch.hip), restated: the dictionary batch_geometry() parses
    from the describe() text of such a batch, plus the group widths nfg / nkg and the number of passes of k_bh."""
    kl = beta == 1.0
    xr = 1 if (F > 32 and F % 32 == 1) else 0
    nf = (F - 1) // 32 if xr else (F + 31) // 32
    nk = (r + 31) // 32
    cf = min(nf, 16 if kl else 8)
    nfg = min(nf, 8 if kl else 4)
    nkg = min(nk, 8 if kl else 4)
    na = -(-(nfg * nkg) // B_WAVES)
    tiles = sum((int(T) + 31) // 32 for T in Ts)
    chunks = sum(-(-((int(T) + 31) // 32) // B_CHUNK_TILES) for T in Ts)
    return dict(B=len(Ts), F=int(F), r=int(r), cf_name=_mode_of(beta), xr=xr, nf=nf, nk=nk, cf=cf, S=B_WAVES // nk, n_fg=-(-nf // nfg),
                n_kg=-(-nk // nkg), NA=1 if na <= 1 else (2 if na <= 2 else (4 if na <= 4 else 8)), tiles=tiles, chunks=chunks,
                nfg=nfg, nkg=nkg, passes=-(-nf // cf))


def batch_geometry(describe_text):
    """xr, nf, nk, cf, S, n_fg, n_kg, NA, tiles, chunks (and B, F, r, the cost function's name) parsed from
    BatchPlan.describe(); nfg, nkg and passes are derived as snmf_batch_create derives them and cross-checked against the
    printed group counts."""
    def ints(pat):
        m = re.search(pat, describe_text)
        assert m is not None, (pat, describe_text)
        return tuple(int(x) for x in m.groups())

    B, F, r = ints(r"batch B=(\d+) F=(\d+) r=(\d+) ")
    name = re.search(r" r=\d+ (kl|ed|beta) upd_h=", describe_text).group(1)
    xr, nf, nk, tiles, chunks = ints(r"xr=(\d) nf=(\d+) nk=(\d+) tiles=(\d+) chunks=(\d+) \|")
    h_grid, cf, S = ints(r"k_bh grid=(\d+) x\d+ lds=\d+ cf=(\d+) S=(\d+) \|")
    w_grid, n_fg, n_kg, NA = ints(r"k_bw grid=\((\d+),(\d+),(\d+)\) x\d+ lds=\d+ NA=(\d+) \|")
    assert h_grid == tiles and w_grid == chunks, describe_text
    kl = name == "kl"
    nfg, nkg = min(nf, 8 if kl else 4), min(nk, 8 if kl else 4)
    assert n_fg == -(-nf // nfg) and n_kg == -(-nk // nkg), describe_text
    return dict(B=B, F=F, r=r, cf_name=name, xr=xr, nf=nf, nk=nk, cf=cf, S=S, n_fg=n_fg, n_kg=n_kg, NA=NA, tiles=tiles, chunks=chunks,
                nfg=nfg, nkg=nkg, passes=-(-nf // cf))


def batch_regions(geom, F, T_b, r, mode="full"):
    """Named index sets of one problem's outputs, in the format of elementwise.regions: {name: (matrix, axis, indices)}, matrix
    "W" (axis 0 rows, axis 1 components) or "H" (axis 0 components, axis 1 frames).  Regions the geometry does not have are
    absent.

    W.rows.mfma / extra_valu / last_partial_tile: the MFMA row tiles, the extra row of F = 32 nf + 1 (b_extra_row; `gxq` in
    k_bw), the rows of a row tile that F does not fill.  W.rows.fgroup<i> / W.comp.kgroup<i>: the rows / components of k_bw's
    blockIdx.y / blockIdx.z (the extra row belongs to the last row group).  H.comp.ktile<kp>: the 32 components of one
    (kap, part) wave set of k_bh.  H.frames.first_tile / full_tiles / last_partial_tile: the problem's first tile (which follows
    another problem's last in the frame layout), the tiles T_b fills, the masked one."""
    T = int(T_b)
    reg = {"W.all": ("W", 0, np.arange(F)), "H.all": ("H", 0, np.arange(r))}
    Fm = 32 * geom["nf"]
    if geom["xr"]:
        reg["W.rows.mfma"] = ("W", 0, np.arange(Fm))
        reg["W.rows.extra_valu"] = ("W", 0, np.array([F - 1]))
    else:
        reg["W.rows.mfma"] = ("W", 0, np.arange(F))
        if F % 32:
            reg["W.rows.last_partial_tile"] = ("W", 0, np.arange(32 * (F // 32), F))
    for i in range(geom["n_fg"]):
        lo, hi = 32 * geom["nfg"] * i, min(Fm, 32 * geom["nfg"] * (i + 1), F)
        rows = np.arange(lo, hi)
        if geom["xr"] and i == geom["n_fg"] - 1:
            rows = np.append(rows, F - 1)
        reg[f"W.rows.fgroup{i}"] = ("W", 0, rows)
    for i in range(geom["n_kg"]):
        reg[f"W.comp.kgroup{i}"] = ("W", 1, np.arange(32 * geom["nkg"] * i, min(r, 32 * geom["nkg"] * (i + 1))))
    full = 32 * (r // 32)
    if r % 32:
        reg["W.comp.remainder"] = ("W", 1, np.arange(full, r))
        reg["H.comp.remainder"] = ("H", 0, np.arange(full, r))
    if mode == "semi":  # w_update_ind zero on the first half (elementwise.case_masks)
        reg["W.comp.fixed"] = ("W", 1, np.arange(r // 2))
        reg["W.comp.updated"] = ("W", 1, np.arange(r // 2, r))
    for kp in range(geom["nk"]):
        reg[f"H.comp.ktile{kp}"] = ("H", 0, np.arange(32 * kp, min(r, 32 * kp + 32)))
    reg["H.frames.first_tile"] = ("H", 1, np.arange(0, min(T, 32)))
    if T >= 32:
        reg["H.frames.full_tiles"] = ("H", 1, np.arange(0, 32 * (T // 32)))
    if T % 32:
        reg["H.frames.last_partial_tile"] = ("H", 1, np.arange(32 * (T // 32), T))
    return reg


# ---- the case table ------------------------------------------------------------------------------------------------------------
#
# The smallest set of shapes that reaches every instantiation of the batch kernels (tests/test_batch_elementwise_rules.py holds
# it to mirror_geometry).  Every case is a BATCH: six to eight problems whose frame counts come from T_EDGES, with one T < 8, one
# multiple of 32 and one T whose last tile holds a single frame and opens a new chunk (257 or 513) in each, ordered so that a
# partial tile is followed by another problem's first tile, and with exactly two problems of T >= 256 (the ones the GPU test also
# steps on a single Plan).  Sparsity: "scalar" / "zero" / "rvec" (a batch takes no r x T matrix).  Data: elementwise.case_data's
# generators, "gamma" (+ 1e-3) and "wide", seeded per (case id, problem).

TS_A = (7, 33, 257, 32, 1, 289, 9)
TS_B = (9, 513, 31, 32, 1, 255, 8, 256)
TS_C = (31, 257, 7, 256, 33, 8, 1)
TS_D = (33, 513, 1, 32, 7, 255, 289)
TS_E = (7, 257, 33, 32, 1, 9, 256)


def _c(id, beta, F, r, Ts, mode="full", sp="scalar", data="gamma", steps=3, **expect):
    return dict(id=id, beta=float(beta), F=F, r=r, Ts=tuple(Ts), mode=mode, sp=sp, data=data, steps=steps, expect=expect)


CASES = [
    _c("kl_65_r8", 1, 65, 8, TS_B, xr=1, nk=1, S=8, NA=1),
    _c("kl_33_r3", 1, 33, 3, TS_A, sp="zero", xr=1, nf=1),
    _c("kl_1_r1", 1, 1, 1, TS_C, xr=0, nf=1, nk=1),
    _c("kl_257_r40", 1, 257, 40, TS_D, sp="rvec", xr=1, nf=8, S=4, NA=2),
    _c("kl_64_r70", 1, 64, 70, TS_B, xr=0, nk=3, S=2),
    _c("kl_37_r150", 1, 37, 150, TS_C, mode="semi", xr=0, nk=5, S=1),
    _c("kl_96_r180", 1, 96, 180, TS_A, mode="w", nk=6),
    _c("kl_513_r100", 1, 513, 100, TS_E, mode="h", xr=1, n_fg=2, NA=4, S=2),
    _c("kl_513_r200", 1, 513, 200, TS_A, xr=1, nf=16, n_fg=2, NA=8, nk=7),
    _c("kl_300_r200", 1, 300, 200, TS_C, sp="zero", xr=0, nf=10, n_fg=2, NA=8),
    _c("ed_129_r24", 2, 129, 24, TS_D, xr=1, nf=4, passes=1, NA=1, n_fg=1),
    _c("ed_513_r200", 2, 513, 200, TS_E, xr=1, passes=2, n_fg=4, n_kg=2, NA=2),
    _c("is_289_r40", 0, 289, 40, TS_A, data="wide", xr=1, nf=9, passes=2, n_fg=3),
    _c("b05_100_r130", 0.5, 100, 130, TS_E, sp="rvec", data="wide", xr=0, nk=5, n_kg=2, NA=2),
    _c("b15_257_r64", 1.5, 257, 64, TS_C, data="wide", xr=1, nk=2, passes=1),
]


def case_masks(mode, r):
    """(w_update_ind, h_update_ind) of a case's mode, as elementwise.case_masks."""
    from elementwise import case_masks as cm
    return cm(mode, r)


def case_sparsity(case):
    """The batch's sparsity (one for all its problems): a scalar or an r-vector."""
    if case["sp"] == "rvec":
        return np.random.default_rng(sum(map(ord, case["id"])) * 104729 + case["r"]).uniform(0.0, 2.0, case["r"])
    return {"scalar": 1.0, "zero": 0.0}[case["sp"]]


def case_problems(case):
    """[(V32, W0, H0)] of a case, deterministic per (case id, problem): elementwise.case_data's generators."""
    out = []
    for b, T in enumerate(case["Ts"]):
        V, W0, H0, _ = case_data(dict(id=f"{case['id']}#{b}", F=case["F"], T=T, r=case["r"], data=case["data"], sp="zero"))
        out.append((V, W0, H0))
    return out


def normalised(W0, H0):
    """src/sparse_nmf.m:157-160: unit columns of W, H rescaled by the norms (H as the fp32 values the device holds)."""
    wn = np.sqrt((np.asarray(W0, np.float64) ** 2).sum(0))
    return W0 / wn, (np.asarray(H0, np.float64) * wn[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_steps(case_id):
    """The fp64 reference of a case, computed once and shared: per problem the list over the steps of
    (H_k, info_h, W_k, info_w), each step taken from the previous fp64 state, H carried as its fp32 image as on the device.
    Nothing here is read from a device: the CPU rules assert compare()'s conditions on it."""
    case = next(c for c in CASES if c["id"] == case_id)
    S = case_sparsity(case)
    w_ind, _ = case_masks(case["mode"], case["r"])
    out = []
    for V, W0, H0 in case_problems(case):
        W, H = normalised(W0, H0)
        steps = []
        for _k in range(case["steps"]):
            ih = iw = None
            if case["mode"] != "w":
                Hn, ih = ref_hstep(V, W, H, case["beta"], S)
                H = Hn.astype(np.float32)
            else:
                Hn = H.astype(np.float64)
            if case["mode"] != "h":
                W, iw = ref_wstep(V, W, H, case["beta"], w_ind)
            steps.append((Hn, ih, W, iw))
        out.append(steps)
    return out


__all__ = ["U", "FLR", "ref_hstep", "ref_wstep", "tau_h", "tau_w", "compare", "cost_of", "batch_chain_t", "mirror_geometry", "batch_geometry", "batch_regions", "CASES", "T_EDGES", "case_masks", "case_sparsity",
           "case_problems", "normalised", "reference_steps", "B_CHUNK_TILES"]
