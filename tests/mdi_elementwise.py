"""Element-wise judgement of the missing-data-imputation solves (src/snmf_mdi.m, src/snmf_mdi_Sm.m): what tests/elementwise.py
does for unmasked plans, extended by what a mask adds.  Test infrastructure: no test functions here; imported by
tests/test_mdi_elementwise_rules.py (CPU) and tests/test_gpu_mdi_elementwise.py (GPU).

THE MASKED STEP.  One iteration of oracle/mdi_oracle.py, cut into the pieces the device exposes:
  mdi_start(V32, M)        v = max(v .* M, flr)                                   (:175)
  ref_hstep / ref_wstep    the two halves of tests/elementwise.py on v AS IT IS (exact_v=True): both read the v that the
                           PREVIOUS iteration left
  mdi_impute(V, M, W, H)   v = max(v .* M + max(W*H, flr) .* (1 - M), flr)        (:251-254), with this iteration's W and H
  mdi_cost(...)            the divergence on the RE-IMPUTED v + sum(S .* H)       (:257-268)
  mdi_final(V, M, W, H)    Nt = sum(v .* M) ./ max(sum(max(W*H, flr) .* M), flr),  v_MDI = max(v .* M + Nt .* max(W*H, flr) .* (1 - M), flr)
                                                                                  (:296-306)
The plan has no getter for its V, so the tests TRACK V in fp64: V_0 = mdi_start, V_k = mdi_impute(V_{k-1}, M, W_k, H_k) with the
(W_k, H_k) read from the device after step k.  Step k's reference is the fp64 step from (V_{k-1} tracked, W_{k-1}, H_{k-1} read
back), as in the unmasked module.  M is the fp32 image the device holds (an exact input, like V).

WHAT THE MASK ADDS TO THE BOUND (u = 2^-24; the derivation of tau_H, tau_W and dL = (r + 2) u is the docstring of
tests/elementwise.py).  The device's V differs from the tracked one only through fp32 roundings of the same formula:
  V_0      : one fp32 product v * M (exact for a 0/1 mask), and the fp32 image of the floor 1e-9 against the fp64 one (3.6e-9
             relative, below u)                                                                             dV_0 = u
  V_k      : fl(fl(V_{k-1} * M) + fl(Lam * fl(1 - M))).  The first term carries dV_{k-1} + u; the second the fp32 Lam of the
             pass (an r-term chain over the fp32 image of W: dL = (r + 2) u) + u for 1 - M + u for the product.  A sum of two
             non-negative terms keeps the worse relative error of the two and adds u:  dV_k <= max(dV_{k-1} + u, (r + 4) u) + u,
             so dV_1 <= (r + 5) u and dV_k <= (r + 5) u + 2 (k - 1) u.  Used, a little wider and simpler:
                                                                                       dV_k = (r + 2) u + 3 k u   (k >= 1)
             at an entry with M != 1.  At an entry with M = 1 the update is v * 1 + Lam * 0 = v, bit for bit: 0.  A mask of ones
             has dV = 0 for every k.
  H step   : both numerators (V ./ Lam, V .* Lam^(beta-2), V itself) are linear in V and are summed over non-negative terms, so
             the update inherits the worst dV of its column:                          tau_H + dV_{k-1}
  W step   : the statistics that read V (G, Q) are linear in V likewise; the finish doubles a relative error twice (W.*dmw./dpw,
             the column norm: tests/elementwise.py):                                  tau_W + 4 dV_{k-1}
  v_MDI    : where M = 1: v * 1 + Nt * Lam * 0 = the floored fp32 input, bit for bit.  Elsewhere: Nt = a / b with a = sum(v .* M)
             (fp32 products of v: dV_n + u, summed in fp64) and b = sum(Lam .* M) (dL + u), divided in fp64 and rounded to fp32
             (+ u): dV_n + dL + 3u.  The second term Nt * Lam * (1 - M) adds the entry's own Lam (dL, an r-term fp32 FMA chain of
             k_mdi_final, independent of the sum's), two products and 1 - M (3u); the first term carries dV_n + u; the sum keeps
             the worse and adds u:                                      tau_V = (2 (r + 2) + 7) u + dV_n
These are worst cases and are NOT fitted to observed errors.  What they are for is structural: a tile, row or frame of V that was
not re-imputed, was re-imputed twice or was re-imputed after a stop is off by the CHANGE of Lam between two iterates at every
non-observed entry, which moves its frame's H column and its row's W by orders of magnitude more than u (r + F).

The bounds need what tests/elementwise.py needs (positive reference entries, no floor on Lam, dph, dpw within 10x of binding:
compare() checks it), and no entirely missing frame (its H column collapses to the floor): the element-wise cases keep every frame
partly observed; entirely missing frames and rows are judged against the oracle as a trajectory.
"""
from __future__ import annotations

import re

import numpy as np

from elementwise import FLR, U, _floored_v, case_masks, cost_of, ref_hstep, ref_wstep, regions, tau_h, tau_w


# ---- the pieces of one masked iteration ---------------------------------------------------------------------------------------

def mask_image(M):
    """The fp32 image of a mask, as fp64: what the device holds (snmf_plan_set_mask_*)."""
    return np.asarray(M, dtype=np.float32).astype(np.float64)


def mdi_start(V32, M):
    """src/snmf_mdi.m:175 on the floored fp32 image of the input (max(max(v, flr) .* M, flr) == max(v .* M, flr) for M in [0, 1])."""
    return np.fmax(_floored_v(V32) * np.asarray(M, np.float64), FLR)


def mdi_impute(V, M, W, H):
    """:251-254: the missing part re-estimated from this iteration's (W, H)."""
    M = np.asarray(M, np.float64)
    lam = np.fmax(np.asarray(W, np.float64) @ np.asarray(H, np.float64), FLR)
    return np.fmax(np.asarray(V, np.float64) * M + lam * (1.0 - M), FLR)


def mdi_final(V, M, W, H):
    """:296-306: (v_MDI, Nt) from the solve's final V, W, H."""
    M = np.asarray(M, np.float64)
    V = np.asarray(V, np.float64)
    lam = np.fmax(np.asarray(W, np.float64) @ np.asarray(H, np.float64), FLR)
    Nt = np.sum(V * M, axis=0) / np.fmax(np.sum(lam * M, axis=0), FLR)
    return np.fmax(V * M + Nt[None, :] * lam * (1.0 - M), FLR), Nt


def mdi_cost(V, W, H, beta, S):
    """The objective of iterate (W, H): the divergence on the re-imputed V + sum(S .* H) (:257-268)."""
    return cost_of(V, W, H, beta, S, exact_v=True)


def mdi_step(V, M, W, H, beta, S, mode, w_ind=None, gram=False):
    """One whole iteration in fp64 from (V_{k-1}, W_{k-1}, H_{k-1}): returns (V_k, W_k, H_k, floors)."""
    floors = {}
    if mode != "w":
        H, info = ref_hstep(V, W, H, beta, S, exact_v=True)
        floors.update(info)
    if mode != "h":
        W, info = ref_wstep(V, W, H, beta, w_ind, gram=gram, exact_v=True)
        floors.update({k: min(v, floors.get(k, np.inf)) for k, v in info.items()})
    return mdi_impute(V, M, W, H), W, H, floors


# ---- the bounds ---------------------------------------------------------------------------------------------------------------

def dv_mdi(r, k, all_observed=False):
    """dV_k: the relative distance of the device's V from the tracked one after k imputations, at an entry with M != 1."""
    if all_observed:
        return 0.0
    return U if k == 0 else U * ((r + 2) + 3 * k)


def tau_h_mdi(F, r, beta, k, mode="full", all_observed=False):
    """The H step of iteration k (it reads V_{k-1}); None where the mode updates no H."""
    t = tau_h(F, r, beta, mode)
    return None if t is None else t + dv_mdi(r, k - 1, all_observed)


def tau_w_mdi(F, r, beta, t_c, k, mode="full", all_observed=False):
    """The W step of iteration k (it reads V_{k-1}); None where the mode updates no W."""
    t = tau_w(F, r, beta, t_c, mode)
    return None if t is None else t + 4 * dv_mdi(r, k - 1, all_observed)


def tau_vmdi(r, n, all_observed=False):
    """v_MDI after n iterations, at an entry with M != 1."""
    return U * (2 * (r + 2) + 7) + dv_mdi(r, n, all_observed)


# ---- the regions of a masked plan ---------------------------------------------------------------------------------------------

def mdi_grid(describe_text):
    """(tiles, workgroups) of the MDI pass: every 32-frame tile of Tp, pad tiles included, on min(Tp / 32, n_cu) workgroups
    (csrc/snmf_tu_geometry.hip grid_mdi).  Read from a masked plan's describe() text where it is one; an unmasked text (the
    device-free snmf_plan_geometry_describe) gives the same numbers through Tp and n_cu."""
    m = re.search(r"hstep: k_hstep \(MDI pass[^|]*; (\d+) tiles\), tile=32 frames, grid=(\d+) x 512 thr", describe_text)
    Tp = int(re.search(r"Tp=(\d+)", describe_text).group(1))
    n_cu = int(re.search(r"n_cu=(\d+)", describe_text).group(1))
    want = (Tp // 32, max(1, min(Tp // 32, n_cu)))
    if m is None:
        assert "MDI pass" not in describe_text, describe_text
        return want
    got = (int(m.group(1)), int(m.group(2)))
    assert got == want, (got, want, describe_text)
    return got


def mdi_regions(describe_text, F, T, r, mode="full"):
    """regions() of tests/elementwise.py (rows, components, the last tile) + the rounds of the MDI pass's tile loop: workgroup g
    takes tiles g, g + grid, ...; H.frames.mdi_first_round holds the frames of every workgroup's first tile, mdi_later_rounds
    the rest (absent when no workgroup takes a second tile that holds a frame)."""
    reg = regions(describe_text, F, T, r, mode)
    _tiles, grid = mdi_grid(describe_text)
    if T > 32 * grid:
        reg["H.frames.mdi_first_round"] = ("H", 1, np.arange(0, 32 * grid))
        reg["H.frames.mdi_later_rounds"] = ("H", 1, np.arange(32 * grid, T))
    return reg


def in_mask_envelope(describe_text, r):
    """What snmf_plan_set_mask refuses on: the out-of-envelope path, and tiles narrower than 32 frames on either side.  The H
    side's tile is in the text (32, or 64 as two sub-tiles); the statistics take 16-frame tiles only on NK = 16 where the 32-frame
    H image + V slab exceed the LDS (csrc/snmf_tu_geometry.hip: (32 ldhw + 32 * 32 * NWB) * 4 + 4 rp + 320 > 160 KiB)."""
    if "out-of-envelope" in describe_text:
        return False
    tile = int(re.search(r"tile=(\d+) frames", describe_text).group(1))
    nk, nwb = (int(x) for x in re.search(r"NK=(\d+) waves=(\d+)\+", describe_text).groups())
    n_kg = int(re.search(r"(\d+) kgroups", describe_text).group(1))
    rp = int(re.search(r"rp=(\d+)", describe_text).group(1))
    ldhw = max(rp, 32 * nk * n_kg) + 4
    ttw32 = not (nk == 16 and (32 * ldhw + 32 * 32 * nwb) * 4 + rp * 4 + 320 > 160 * 1024)
    return tile in (32, 64) and ttw32


# ---- the v_MDI comparator -----------------------------------------------------------------------------------------------------

def compare_vmdi(dev, ref, V32, M, tau, what=""):
    """v_MDI per element: where M = 1 the floored fp32 input bit for bit; elsewhere within tau of the reference, which must be
    10x above the floor.  Names the frame and the row of the worst element, so that one wrong Nt (a column) fails by itself.
    Returns (worst, (f, t), rms) over the entries with M != 1 (zeros where there are none)."""
    dev = np.asarray(dev, np.float64)
    ref = np.asarray(ref, np.float64)
    M = np.asarray(M, np.float64)
    assert dev.shape == ref.shape == M.shape, (what, dev.shape, ref.shape, M.shape)
    assert np.isfinite(dev).all(), f"{what}: non-finite v_MDI at {np.argwhere(~np.isfinite(dev))[:4].tolist()}"
    obs = M == 1.0
    v32 = np.fmax(np.asarray(V32, np.float32), np.float32(FLR))
    same = dev.astype(np.float32) == v32
    assert same[obs].all(), (f"{what}: v_MDI differs from the input at observed entries "
                             f"{np.argwhere(obs & ~same)[:4].tolist()} ({int((obs & ~same).sum())} in all)")
    if obs.all():
        return 0.0, (0, 0), 0.0
    assert ref[~obs].min() > 10 * FLR, f"{what}: the floor on v_MDI is within 10x of binding (min {ref[~obs].min():.3e})"
    e = np.where(obs, 0.0, np.abs(dev - ref) / ref)
    f, t = (int(x) for x in np.unravel_index(int(np.argmax(e)), e.shape))
    worst = float(e[f, t])
    bad_frames = np.nonzero((e > tau).any(axis=0))[0]
    assert worst <= tau, (f"{what}: v_MDI breaks its bound {tau:.3e} in {bad_frames.size} frames (first {bad_frames[:6].tolist()}): "
                          f"frame {t}, row {f} is off by {worst:.3e} relative (device {dev[f, t]:.9g}, reference {ref[f, t]:.9g})")
    return worst, (f, t), float(np.sqrt(np.mean(e[~obs] ** 2)))


# ---- the case table of tests/test_gpu_mdi_elementwise.py (checked without a device by tests/test_mdi_elementwise_rules.py) ----
#
# Three steps each, run(1) at a time, conv_eps = 0.  `tokens`: what the W-statistics half of describe() must contain (the same
# with and without a mask); `expect`: regions the case is meant to exercise.  mask: "01" (30 % missing), "soft" (as
# tests/test_mdi.problem(soft=True)), "ones", "blocks" (64 consecutive frames 90 % missing, beside untouched ones).
# The MDI pass k_hstep<8, 1, 0, BM, OBJ, UPD, MDI = true>: every plan that updates H launches (OBJ, UPD) = (0, 1) on step 1 and
# (1, 1) on steps 2 and 3 (cost_check on), a W-only plan (1, 0), and every plan with cost_check (1, 0) once more as its final
# objective pass; BM follows beta (KL, Euclidean, generic).

def _m(id, F, T, r, beta, mode, sp, mask, tokens, expect=(), cost_check=True):
    return dict(id=id, F=F, T=T, r=r, beta=float(beta), mode=mode, sp=sp, mask=mask, steps=3, tokens=list(tokens),
                expect=list(expect), cost_check=cost_check)


MDI_CASES = [
    # the tile loop: 260 tiles that hold a frame on 256 workgroups (n_cu = 256): four workgroups take two, the heavy blocks lie in both rounds
    _m("kl_two_rounds_F257", 257, 8300, 40, 1, "full", "scalar", "blocks", ["NK=4 waves=8+4", "256 chunks,1 fgroups"],
       ["H.frames.mdi_later_rounds", "W.rows.extra_valu", "H.frames.last_partial_tile"]),
    # few tiles, synchronous k_wstats: the shapes of tests/test_mdi.py and below (T < 32, three to five tiles)
    _m("kl_3tiles_F65", 65, 90, 9, 1, "full", "scalar", "01", ["NK=4 waves=4+0", "3 chunks,1 fgroups"],
       ["W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _m("kl_T20_F513", 513, 20, 100, 1, "full", "rvec", "soft", ["NK=4 waves=4+0", "1 chunks,4 fgroups"],
       ["W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _m("ed_gram_5tiles_F130", 130, 150, 24, 2, "full", "scalar", "01", ["NK=4 waves=4+0", "Gram matrix"],
       ["W.rows.last_partial_tile", "H.frames.last_partial_tile"]),
    _m("kl_sync_F513", 513, 401, 20, 1, "full", "entry", "01", ["NK=4 waves=4+0", "13 chunks,4 fgroups"],
       ["W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _m("kl_sync_F422", 422, 1001, 32, 1, "full", "scalar", "soft", ["NK=4 waves=4+0", "4 fgroups"],
       ["W.rows.last_partial_tile", "H.frames.last_partial_tile"]),
    # generic beta with a mask (launch_hstep_mdi_b<BM_GEN>): 0, 0.5, 1.5; the extra row on (F = 33 = 32 + 1 has it) and off
    _m("is_F33", 33, 1501, 20, 0, "full", "scalar", "soft", ["NK=4 waves=4+0", "beta=0 "], ["W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _m("b05_F64", 64, 2001, 40, 0.5, "full", "rvec", "01", ["NK=4 waves=4+0", "beta=0.5 "], ["H.frames.last_partial_tile"]),
    _m("b15_F257", 257, 1501, 60, 1.5, "full", "entry", "soft", ["NK=4 waves=4+0", "beta=1.5 ", "2 fgroups"],
       ["W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _m("is_wonly_F130", 130, 3001, 24, 0, "w", "scalar", "01", ["NK=4 waves=4+0", "beta=0 "], ["W.rows.last_partial_tile"]),
    _m("b15_honly_F65", 65, 1001, 24, 1.5, "h", "scalar", "soft", ["beta=1.5 "], ["H.frames.last_partial_tile"]),
    # the statistics geometries behind the pass: loader waves with four and eight consumers, NK = 8, NK = 16 on two kappa-groups,
    # two row groups dealt unevenly, k_wstats_sf (also the shape that is k_iter_sf without a mask), k_wstats_sr
    _m("kl_loader4_F129", 129, 9001, 100, 1, "full", "scalar", "01", ["NK=4 waves=4+4"], ["W.rows.extra_valu", "H.frames.mdi_later_rounds"]),
    _m("kl_loader8_F289_wonly", 289, 9001, 100, 1, "w", "scalar", "soft", ["NK=4 waves=8+4", "2 fgroups"], ["W.rows.extra_valu"]),
    _m("kl_nk8_F513", 513, 9001, 193, 1, "full", "rvec", "01", ["NK=8 waves=4+4", "71 chunks,4 fgroups,1 kgroups; group-1 chunks 61"],
       ["W.rows.extra_valu", "H.frames.mdi_later_rounds"]),
    _m("kl_nk16_kg2_F65", 65, 3001, 600, 1, "full", "scalar", "soft", ["NK=16", "2 kgroups"], ["W.rows.extra_valu", "H.comp.remainder"]),
    _m("kl_two_row_groups_F513", 513, 30001, 100, 1, "full", "scalar", "01", ["NK=4 waves=8+4", "134 chunks,2 fgroups,1 kgroups; group-1 chunks 122"],
       ["W.rows.extra_valu", "H.frames.mdi_later_rounds"]),
    _m("kl_wsf_F64_r100", 64, 9001, 100, 1, "full", "scalar", "soft", ["k_wstats_sf: a tile per wave"],
       ["H.frames.mdi_later_rounds", "H.frames.last_partial_tile"]),
    _m("kl_wsf_shared_F64_r40", 64, 12001, 40, 1, "full", "entry", "01", ["k_wstats_sf: a tile per wave, a single remainder tile shared by the eight waves"],
       ["H.frames.mdi_later_rounds"]),
    _m("kl_wsr_F513_r20", 513, 9001, 20, 1, "full", "scalar", "soft", ["k_wstats_sr"], ["W.rows.extra_valu", "H.frames.mdi_later_rounds"]),
    _m("kl_wsr_semi_F422", 422, 9001, 32, 1, "semi", "scalar", "01", ["k_wstats_sr"], ["W.comp.fixed", "W.rows.last_partial_tile"]),
    # Euclidean: r > 256 (the Q launch on 256-wide kappa-groups), with the Gram form (full) and without (W-only)
    _m("ed_nk16_gram_F257", 257, 3001, 300, 2, "full", "scalar", "soft", ["NK=16", "Gram matrix"], ["W.rows.extra_valu"]),
    _m("ed_nk16_wonly_F257", 257, 3001, 300, 2, "w", "scalar", "01", ["NK=16"], ["W.rows.extra_valu"]),
    _m("ed_honly_F130", 130, 1001, 24, 2, "h", "rvec", "01", ["beta=2 "], ["H.frames.last_partial_tile"]),
    # modes on the KL pass; a mask of ones; the final imputation as a pass of its own (cost_check off)
    _m("kl_honly_F257", 257, 1001, 40, 1, "h", "rvec", "soft", ["NK=4"], ["H.frames.last_partial_tile"]),
    _m("kl_wonly_F257", 257, 2001, 40, 1, "w", "scalar", "01", ["NK=4 waves=4+0", "k_wfin"], ["W.rows.extra_valu"]),
    _m("kl_ones_F65", 65, 301, 9, 1, "full", "scalar", "ones", ["NK=4 waves=4+0"], ["W.rows.extra_valu"]),
    _m("kl_nocost_F257", 257, 1001, 40, 1, "full", "scalar", "soft", ["NK=4 waves=4+0"], ["W.rows.extra_valu"], cost_check=False),
]


def make_mask(kind, F, T, rs):
    """The fp32 image of a case's mask, as fp64 (mask_image).  No kind leaves a frame or a row entirely missing (asserted)."""
    if kind == "ones":
        M = np.ones((F, T))
    elif kind == "blocks":
        M = np.ones((F, T))
        heavy = (np.arange(T) // 64) % 4 == 1
        M[:, heavy] = (rs.random((F, int(heavy.sum()))) > 0.9).astype(np.float64)
        empty = np.nonzero(M.max(axis=0) == 0)[0]
        M[empty % F, empty] = 1.0  # (a short frame may draw no observed entry at all: give it one)
    else:
        M = (rs.random((F, T)) > 0.3).astype(np.float64)
        if kind == "soft":
            M = np.clip(M * 0.8 + rs.random((F, T)) * 0.2, 0, 1)
    M = mask_image(M)
    assert (M.max(axis=0) > 0.5).all() and (M.max(axis=1) > 0.5).all(), kind
    return M


def mdi_case_data(case):
    """(V32, M, W0, H0, S) of a case: deterministic per case id.  The data of tests/elementwise.case_data ("gamma")."""
    F, T, r = case["F"], case["T"], case["r"]
    rs = np.random.default_rng(sum(map(ord, case["id"])) * 7919 + F)
    V = rs.gamma(0.5, 1.0, (F, 16)) @ rs.gamma(0.3, 1.0, (16, T)) + 1e-3
    W0 = rs.random((F, r))
    H0 = rs.random((r, T)).astype(np.float32)
    S = {"scalar": 0.5, "rvec": rs.uniform(0.0, 2.0, r), "entry": rs.uniform(0.0, 2.0, (r, T))}[case["sp"]]
    return V.astype(np.float32), make_mask(case["mask"], F, T, rs), W0, H0, S


__all__ = ["MDI_CASES", "mask_image", "mdi_start", "mdi_impute", "mdi_final", "mdi_cost", "mdi_step", "dv_mdi", "tau_h_mdi",
           "tau_w_mdi", "tau_vmdi", "mdi_grid", "mdi_regions", "in_mask_envelope", "compare_vmdi", "make_mask", "mdi_case_data",
           "case_masks"]
