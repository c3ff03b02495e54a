"""Element-wise judgement of ONE multiplicative-update step: the fp64 restatement of the two halves of an iteration, the worst-case
rounding bound of a single fp32 step, the plan's output regions read from its describe() text, and a comparator that names the
region and the element that break the bound.  Test infrastructure (like fuzz_cases.py): no test functions here; imported by
tests/test_elementwise_rules.py (CPU) and tests/test_gpu_elementwise.py (GPU).

WHY ONE STEP AND NOT A TRAJECTORY.  The other parity tests compare whole matrices with one Frobenius norm after several
iterations, which dilutes an error that sits in one frame, one row or one tile by the square root of the matrix size, and spends
part of its budget on the honest fp32-vs-fp64 drift of the trajectory.  Here the reference step starts from the device's own
state (W_{k-1} as the fp64 master, H_{k-1} as the fp32 values the device holds), so the comparison measures the rounding of one
step and nothing else, element by element.

THE BOUND.  Every quantity of src/sparse_nmf.m:189-244 is built from non-negative values as long as no 1e-9 floor binds: Lam = W*H,
V./Lam, Lam.^(beta-1), V.*Lam.^(beta-2), both contractions, the column sums, sum(G.*W)*W, the W statistics over the frames, the
column norms.  A sum of n non-negative terms formed in fp32 in ANY order (MFMA chains, VALU rows, split partial sums, LDS hand-offs)
has a relative error of at most (n-1) u, u = 2^-24 (gamma_n ~ n u with the products' roundings).  A rounding of an operand to fp32
adds u, a product or quotient u, v_rcp_f32 (fast_rcp) and OCML powf (fast_pow, csrc/snmf_kernels.h) about 1 ulp <= 2u, and x^p
multiplies a relative error of x by |p|.  V is the fp32 image the device holds (an exact input); H_{k-1} is read from the device
(exact); W_{k-1} is the fp64 master, of which the kernels contract the fp32 image (+u).

  Lam       : r-term fp32 chain over W image x H                          dL   = (r + 2) u
  H step (csrc/snmf_kernels.h hstep_p2, snmf_smallf.h, snmf_smallr.h, snmf_generic.h; src/sparse_nmf.m:189-207):
    KL      : ratio = V * rcp(Lam) (3u), dmh = W^T ratio (F-term chain + W image), dph = colsum(W) + S (counted as an F-term fp32
              chain although the plan forms it from the fp64 master), rcp(dph) and the two products of the update (6u)
    beta!=1 : den = powf(Lam, beta-1) (|beta-1| dL + 2u), dph = W^T den + S (F-term chain + W image + S + the floor), H ./ dph
              (rcp + product); num = V * powf(Lam, beta-2) (|beta-2| dL + 3u), dmh = W^T num (F-term chain), one product
    =>  tau_H = u * (2 F + (|beta-1| + |beta-2|) (r + 2) + c_H),  c_H = 16   (KL: |0| + |-1| = 1, Euclidean: den = Lam, num = V)
  W step (k_wstats / k_wstats_sf / k_wstats_sr / k_iter_sf / k_g_gemm + k_wfin / k_reduce + k_wapply; src/sparse_nmf.m:212-243):
    the statistics G (KL) or P, Q (beta != 1) and the row sums of H are fp32 chains over at most T_c frames per slab, the slabs
    summed in fp64 (k_wfin / k_reduce); an entry of P or Q carries T_c u + m_beta dL + 4u, m_beta = max(|beta-1|, |beta-2|)
    (KL: the ratio, exponent -1; the Gram form P = W*(H*H'): an r-term chain on a T_c-term chain, covered by the same count).
    dpw = s + sum(G.*W).*W and dmw = G + sum(s.*W).*W add non-negative terms: each keeps the worst relative error of its inputs;
    W.*dmw./dpw at most doubles it, and the column normalisation of :242 (the norm of entries that are each within e is within e)
    doubles it again.  The three F-term sums of the finish (sum(G.*W), sum(s.*W) or sum(P.*W), the norm) are counted as fp32 chains
    (3F), which over-covers k_wfin's fp64 sums.
    =>  tau_W = u * (4 (T_c + m_beta (r + 2) + 6) + 3 F + 8)
  T_c, the longest fp32 chain over frames, follows from the plan's geometry: 32 (ceil(tiles / chunks) + 1) with the statistics'
  chunk count (the smaller of group 0's and group 1's), the Gram launch's chunk count and the Euclidean Q launch's (csrc/
  snmf_tu_geometry.hip) where they are fewer; 2048 (kGChunkT, csrc/snmf_generic.h) on the out-of-envelope path.  The "+1" tile
  covers a remainder tile whose partial sums are shared between waves.  tau is a worst case and is NOT fitted to observed errors:
  a structural error -- a missing or doubled k block (~1/F), stale H in a tile, the wrong frame's V or sparsity entry, a padding
  lane in a sum -- is one or two orders of magnitude above it, while rounding sits one or two orders below it.

  The bound needs every reference entry > 0 and every floor of :193 / :207 / :218 / :243 (on Lam, dph, dpw) at least 10x away
  from binding: compare() fails otherwise (the 1e-9 floor that :169 applies to V on upload is part of the input).

  WITH A MASK (src/snmf_mdi.m; tests/mdi_elementwise.py derives it) V is no exact input any more: the solve re-imputes it every
  iteration from its fp32 Lam, so after k imputations the device's V is within dV_k = (r + 2) u + 3 k u of the V the test tracks in
  fp64 (0 where M = 1).  The numerators of the H step and the statistics G, Q of the W step are linear in V, so the bounds become
  tau_H + dV_{k-1} and tau_W + 4 dV_{k-1}; ref_hstep / ref_wstep / cost_of take that tracked V as it is with exact_v=True.
"""
from __future__ import annotations

import re

import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32
FLR = 1e-9      # src/sparse_nmf.m:166
G_CHUNK_T = 2048  # kGChunkT, csrc/snmf_generic.h: frames per split of a contraction over T on the out-of-envelope path


def _sparsity_matrix(S, r, T):
    """src/sparse_nmf.m:150-155: a scalar, an r-vector or an r x T matrix -> r x T."""
    sp = np.asarray(S, dtype=np.float64)
    if sp.size == 1:
        return np.full((r, T), float(sp.reshape(-1)[0]))
    if sp.ndim == 1 or (sp.ndim == 2 and sp.shape[1] == 1):
        return np.repeat(sp.reshape(-1, 1), T, axis=1)
    return sp


def _floored_v(V32, exact_v=False):
    """The V of a step: the fp32 image of the input, floored (:169 on upload).  exact_v: V is taken as it is, in fp64 -- the
    tracked state of a masked solve (tests/mdi_elementwise.py), which the re-imputation has moved off the fp32 grid."""
    if exact_v:
        return np.asarray(V32, dtype=np.float64)
    return np.fmax(np.asarray(V32, dtype=np.float32).astype(np.float64), FLR)


def ref_hstep(V32, W, H, beta, S=0.0, h_ind=None, exact_v=False):
    """The H half of one iteration in fp64, src/sparse_nmf.m:189-207 (oracle/sparse_nmf_oracle.py:180-207).

    Returns (H_new, info): info holds the smallest unclamped Lam = W*H and dph, whose distance from the 1e-9 floor the bound
    depends on.  Rows outside h_ind are returned unchanged (a partial h_ind is refused by the plan anyway).  exact_v: _floored_v."""
    V = _floored_v(V32, exact_v)
    W = np.asarray(W, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    F, T = V.shape
    r = W.shape[1]
    h_ind = np.ones(r, bool) if h_ind is None else np.asarray(h_ind).astype(bool).reshape(-1)
    Sm = _sparsity_matrix(S, r, T)[h_ind]
    lam0 = W @ H
    lam = np.fmax(lam0, FLR)  # :167 / :207 / :243
    wh = W[:, h_ind]
    if beta == 1:
        dph0 = np.sum(wh, axis=0)[:, None] + Sm  # :192
        dmh = wh.T @ (V / lam)  # :194
    elif beta == 2:
        dph0 = wh.T @ lam + Sm  # :197
        dmh = wh.T @ V  # :199
    else:
        dph0 = wh.T @ lam ** (beta - 1.0) + Sm  # :202
        dmh = wh.T @ (V * lam ** (beta - 2.0))  # :204
    dph = np.fmax(dph0, FLR)  # :193
    Hn = H.copy()
    Hn[h_ind] = H[h_ind] * dmh / dph  # :195
    info = {"lam": float(lam0.min()) if lam0.size else np.inf, "dph": float(dph0.min()) if dph0.size else np.inf}
    return Hn, info


def ref_wstep(V32, W, H, beta, w_ind=None, gram=False, exact_v=False):
    """The W half of one iteration in fp64, src/sparse_nmf.m:212-243 (oracle/sparse_nmf_oracle.py:210-233), with H the
    activations of THIS iteration.  All columns are normalised afterwards (:242).  gram=True forms P = W*(H*H') (what a plan
    reporting "through the Gram matrix" computes; equal to max(W*H, flr)*H' wherever the floor does not bind).

    Returns (W_new, info): info holds the smallest unclamped Lam and dpw.  exact_v: _floored_v."""
    V = _floored_v(V32, exact_v)
    W = np.asarray(W, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    r = W.shape[1]
    w_ind = np.ones(r, bool) if w_ind is None else np.asarray(w_ind).astype(bool).reshape(-1)
    lam0 = W @ H
    lam = np.fmax(lam0, FLR)
    ww, hw = W[:, w_ind], H[w_ind, :]
    if beta == 1:
        G = (V / lam) @ hw.T  # :217,:219
        s = np.sum(hw, axis=1)[None, :]  # :215
        dpw0 = s + np.sum(G * ww, axis=0)[None, :] * ww  # :215-217
        dmw = G + np.sum(s * ww, axis=0)[None, :] * ww  # :219-221
    else:
        if beta == 2:
            P = W @ (H @ hw.T) if gram else lam @ hw.T  # :224,:228
            Q = V @ hw.T  # :225,:227
        else:
            P = lam ** (beta - 1.0) @ hw.T  # :231,:238
            Q = (V * lam ** (beta - 2.0)) @ hw.T  # :233,:236
        dpw0 = P + np.sum(Q * ww, axis=0)[None, :] * ww
        dmw = Q + np.sum(P * ww, axis=0)[None, :] * ww
    dpw = np.fmax(dpw0, FLR)  # :218
    Wn = W.copy()
    Wn[:, w_ind] = ww * dmw / dpw  # :222,:229,:239
    Wn = Wn / np.sqrt(np.sum(Wn ** 2, axis=0))  # :242
    info = {"lam": float(lam0.min()), "dpw": float(dpw0.min()) if dpw0.size else np.inf}
    return Wn, info


def tau_h(F, r, beta, mode="full"):
    """Worst-case relative error of one H step per element (module docstring); None where the mode updates no H."""
    if mode == "w":
        return None
    return U * (2 * F + (abs(beta - 1.0) + abs(beta - 2.0)) * (r + 2) + 16)


def tau_w(F, r, beta, t_c, mode="full"):
    """Worst-case relative error of one W step per element (module docstring); None where the mode updates no W."""
    if mode == "h":
        return None
    m = max(abs(beta - 1.0), abs(beta - 2.0))
    return U * (4 * (t_c + m * (r + 2) + 6) + 3 * F + 8)


# ---- the plan's regions --------------------------------------------------------------------------------------------------------

def _ints(pat, text):
    m = re.search(pat, text)
    return None if m is None else tuple(int(x) for x in m.groups())


def family(describe_text):
    """The H-step family token of a describe() text: k_hstep_rp / k_hstep_rh / k_hstep / k_hstep_sf / k_iter_sf / k_hstep_sr /
    out-of-envelope."""
    if "out-of-envelope" in describe_text:
        return "out-of-envelope"
    m = re.search(r"hstep: (k_\w+)", describe_text)
    return m.group(1) if m else None


def chain_t(describe_text, T):
    """T_c: the longest fp32 chain over frames in the W statistics of this plan (module docstring)."""
    if "out-of-envelope" in describe_text:
        return min(T, G_CHUNK_T)
    nk, nwb, nlw = _ints(r"NK=(\d+) waves=(\d+)\+(\d+)", describe_text)
    ch, nfg, nkg, ch1 = _ints(r"grid=\((\d+) chunks,(\d+) fgroups,(\d+) kgroups; group-1 chunks (\d+)\)", describe_text)
    n_cu, = _ints(r"n_cu=(\d+)", describe_text)
    rp, = _ints(r"rp=(\d+)", describe_text)
    beta = float(re.search(r"beta=(\S+)", describe_text).group(1))
    tiles = (T + 31) // 32
    chunks = min(ch, ch1)
    nkc = rp // 32
    if beta == 2.0 and nk == 16:  # the Euclidean Q launch on 256-wide kappa-groups (kq_chunks)
        chunks = min(chunks, max(1, n_cu // max(1, nfg * -(-nkc // 8))))
    if "Gram matrix" in describe_text and nk != 16:  # the Gram launch's own chunk grid (gram_chunks)
        wps = 2 if nk <= 8 else 1
        chunks = min(chunks, max(1, min(tiles, n_cu * (1 if nlw else wps) // max(1, -(-nkc // nwb)))))
    return min(T, 32 * (-(-tiles // max(1, chunks)) + 1))


def regions(describe_text, F, T, r, mode="full"):
    """Named index sets of the outputs that individual kernel paths compute, parsed from the plan's describe() text.

    Returns {name: (matrix, axis, indices)}: matrix "W" (axis 0 rows, axis 1 components) or "H" (axis 0 components, axis 1
    frames).  Every matrix also has "all".  Regions that the geometry does not have are absent."""
    reg = {"W.all": ("W", 0, np.arange(F)), "H.all": ("H", 0, np.arange(r))}
    fam = family(describe_text)
    tiles = (T + 31) // 32

    def frames(a, b):
        return np.arange(max(0, a), min(T, b))

    # ---- W rows ----
    m = _ints(r"Fm=(\d+)\(\+(\d) VALU row\)", describe_text)
    if m is not None:
        Fm, xr = m
        if xr:
            reg["W.rows.mfma"] = ("W", 0, np.arange(Fm))
            reg["W.rows.extra_valu"] = ("W", 0, np.array([F - 1]))
        else:
            reg["W.rows.mfma"] = ("W", 0, np.arange(F))
            if F % 32:
                reg["W.rows.last_partial_tile"] = ("W", 0, np.arange(32 * (F // 32), F))
    # ---- components ----
    full = 32 * (r // 32)
    if full:
        reg["W.comp.full_tiles"] = ("W", 1, np.arange(full))
        reg["H.comp.full_tiles"] = ("H", 0, np.arange(full))
    if r % 32:
        # (the 4x4x1 leftover MFMAs are k_hstep_rh's H step; the W statistics of those columns come from k_wstats like any other)
        reg["W.comp.remainder"] = ("W", 1, np.arange(full, r))
        key = "leftover_4x4x1" if "leftover columns as 4x4x1 MFMAs" in describe_text else "remainder"
        reg["H.comp." + key] = ("H", 0, np.arange(full, r))
    if mode == "semi":  # w_update_ind zero on the first half (test_plan_geometry.masks)
        reg["W.comp.fixed"] = ("W", 1, np.arange(r // 2))
        reg["W.comp.updated"] = ("W", 1, np.arange(r // 2, r))
    # ---- frames ----
    if T % 32:
        reg["H.frames.last_partial_tile"] = ("H", 1, frames(32 * (T // 32), T))
    else:
        reg["H.frames.last_tile"] = ("H", 1, frames(T - 32, T))
    if fam in ("k_hstep_rp", "k_hstep_rh"):
        n_full, n_tiles, S, grid = _ints(r"(\d+) of (\d+) tiles pipelined, last round split (\d+) ways, grid (\d+)", describe_text)
        reg["H.frames.pipelined"] = ("H", 1, frames(0, 32 * n_full))
        if S:
            reg["H.frames.split_round"] = ("H", 1, frames(32 * n_full, 32 * n_tiles))
    elif fam == "k_hstep_sf":
        n_tiles, x, grid = _ints(r"(\d+) tiles, the last (\d+) shared by four waves each, grid (\d+)", describe_text)
        reg["H.frames.whole_tiles"] = ("H", 1, frames(0, 32 * (n_tiles - x)))
        if x:
            reg["H.frames.shared_tiles"] = ("H", 1, frames(32 * (n_tiles - x), 32 * n_tiles))
    elif fam == "k_iter_sf":
        n_tiles, grid = _ints(r"(\d+) tiles, grid (\d+); step API", describe_text)
        if "remainder tile shared by the four pairs" in describe_text:
            idx = _remainder_tiles(n_tiles, grid, 4)
            if idx.size:
                reg["H.frames.shared_remainder"] = ("H", 1, np.concatenate([frames(32 * t, 32 * t + 32) for t in idx]))
    return reg


def _remainder_tiles(n_tiles, n_chunks, ncl):
    """The single remainder tile of every chunk that has one: chunk c takes tiles [n c / N, n (c+1) / N), whole rounds of ncl
    tiles first (csrc/snmf_smallf.h)."""
    out = []
    for c in range(n_chunks):
        tb, te = n_tiles * c // n_chunks, n_tiles * (c + 1) // n_chunks
        if te > tb and (te - tb) % ncl == 1:
            out.append(te - 1)
    return np.array(out, dtype=np.int64)


def wstats_remainder_shared(describe_text, T):
    """Whether k_wstats_sf shares a single remainder tile among its eight waves in this plan, and in how many chunks."""
    if "a single remainder tile shared by the eight waves" not in describe_text:
        return 0
    ch, = _ints(r"grid=\((\d+) chunks", describe_text)
    return int(_remainder_tiles((T + 31) // 32, ch, 4).size)


# ---- the comparator ------------------------------------------------------------------------------------------------------------

def rel_err(dev, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(dev, dtype=np.float64) - ref) / ref


def compare(dev, ref, tau, regs, matrix, *, floors=None, what=""):
    """Per region of `matrix` ("W" or "H"): the worst element's relative error and its index, and the RMS relative error.
    Asserts the bound tau on every element, naming the region and the element; fails as well where the reference has an entry
    <= 0 or where a floor of `floors` ({name: smallest unclamped value}) is within 10x of binding (the bound does not hold
    there).  Returns {region: (worst, (i, j), rms)}."""
    ref = np.asarray(ref, dtype=np.float64)
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    assert np.isfinite(dev).all(), f"{what}: non-finite device output at {np.argwhere(~np.isfinite(dev))[:4].tolist()}"
    assert (ref > 0).all(), f"{what}: reference entry <= 0 at {np.argwhere(ref <= 0)[:4].tolist()}: the element-wise bound needs positive values"
    for name, v in (floors or {}).items():
        assert v > 10 * FLR, f"{what}: the 1e-9 floor on {name} is within 10x of binding (min {v:.3e}): the element-wise bound does not hold"
    e = rel_err(dev, ref)
    out, bad = {}, []
    for name, (mat, axis, idx) in regs.items():
        if mat != matrix or len(idx) == 0:
            continue
        sub = np.take(e, idx, axis=axis)
        k = np.unravel_index(int(np.argmax(sub)), sub.shape)
        ij = (int(idx[k[0]]), int(k[1])) if axis == 0 else (int(k[0]), int(idx[k[1]]))
        worst = float(sub[k])
        out[name] = (worst, ij, float(np.sqrt(np.mean(sub ** 2))))
        if not worst <= tau:
            bad.append(f"region {name}: element {ij} is off by {worst:.3e} relative (device {dev[ij]:.9g}, reference {ref[ij]:.9g})")
    assert not bad, f"{what}: the one-step bound {tau:.3e} is broken in\n  " + "\n  ".join(bad)
    return out


def rel(a, b):
    """The whole-matrix criterion of the trajectory tests (test_gpu_parity.rel)."""
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def cost_of(V32, W, H, beta, S, exact_v=False):
    """The objective of iterate (W, H) in fp64: divergence + sum(S .* H) (src/sparse_nmf.m:248-261).  exact_v: _floored_v."""
    from oracle.sparse_nmf_oracle import divergence
    V = _floored_v(V32, exact_v)
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    lam = np.fmax(W @ H, FLR)
    return divergence(V, lam, beta) + float(np.sum(_sparsity_matrix(S, W.shape[1], H.shape[1]) * H))


__all__ = ["U", "FLR", "ref_hstep", "ref_wstep", "tau_h", "tau_w", "family", "chain_t", "regions", "compare", "rel", "cost_of",
           "wstats_remainder_shared"]


# ---- the case table of tests/test_gpu_elementwise.py (checked without a device by tests/test_elementwise_rules.py) ------------
#
# Every H-step family with each sparsity form (scalar / per-component "rvec" / per-entry / zero), every W-statistics geometry,
# both epilogue folds and the out-of-envelope path, at n_cu = 256.  `tokens`: what describe() must contain; `expect`: the regions
# the case is meant to exercise.  Data: "gamma" (the mixtures of the other tests, + 1e-3), "wide" (the fuzzer's V**3 * 1e3: the
# beta != 1 powf / rcp paths over many decades), "quiet" (rows and frames 1e-6, sixty decibels below the rest: exact zeros would
# put Lam on the 1e-9 floor within one Euclidean step, where no element-wise bound holds).

def _c(id, F, T, r, beta, mode, sp, tokens, expect=(), data="gamma", steps=3):
    return dict(id=id, F=F, T=T, r=r, beta=float(beta), mode=mode, sp=sp, data=data, steps=steps, tokens=list(tokens),
                expect=list(expect))


CASES = [
    # k_hstep_rp: the split last round (2 / 4 ways), the contraction cut four ways and in wave pairs, >= 3 tiles per workgroup,
    # the extra VALU row at F = 65, 257, 513
    _c("rp_split2_F65", 65, 12001, 70, 1, "full", "scalar", ["k_hstep_rp (", "split 2 ways"],
       ["H.frames.split_round", "W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _c("rp_split4_F129", 129, 9791, 70, 1, "full", "rvec", ["k_hstep_rp (", "split 4 ways"],
       ["H.frames.split_round", "W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _c("rp_cut4_F289", 289, 20000, 40, 1, "full", "entry", ["k_hstep_rp (", "P2 cut four ways over the contraction;"],
       ["H.frames.pipelined", "W.rows.extra_valu", "H.comp.remainder"]),
    _c("rp_pairs_F513", 513, 12000, 50, 1, "full", "zero", ["k_hstep_rp (", "P2 in wave pairs cut over the contraction;"],
       ["H.frames.pipelined", "W.rows.extra_valu", "H.comp.remainder"]),
    _c("rp_3tiles_semi_F65", 65, 24577, 70, 1, "semi", "zero", ["k_hstep_rp (", "768 of 769 tiles", "split 2 ways"],
       ["H.frames.split_round", "W.comp.fixed", "W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _c("rp_3tiles_honly_F257", 257, 30000, 256, 1, "h", "rvec", ["k_hstep_rp (", "938 of 938 tiles", "on the H step's last workgroup"],
       ["H.frames.pipelined", "H.frames.last_partial_tile"]),
    # k_hstep_rh: leftover 4x4x1 columns (four-way cut: r = 97..100; wave pairs: r = 193..200) and the plain rh form
    _c("rh_lx4_r97", 513, 12000, 97, 1, "full", "scalar", ["k_hstep_rh (", "P2 cut four ways", "leftover columns as 4x4x1 MFMAs"],
       ["H.comp.leftover_4x4x1", "W.comp.remainder", "H.frames.split_round", "W.rows.extra_valu"]),
    _c("rh_lx4_r100_honly", 513, 9023, 100, 1, "h", "entry", ["k_hstep_rh (", "leftover columns as 4x4x1 MFMAs",
                                                              "on the H step's last workgroup"],
       ["H.comp.leftover_4x4x1", "H.frames.split_round", "H.frames.last_partial_tile"]),
    _c("rh_pairs_r193", 513, 9000, 193, 1, "full", "rvec", ["k_hstep_rh (", "P2 in wave pairs", "leftover columns as 4x4x1 MFMAs", "NK=8"],
       ["H.comp.leftover_4x4x1", "W.comp.remainder", "H.frames.split_round"]),
    _c("rh_pairs_r200_honly", 513, 9000, 200, 1, "h", "zero", ["k_hstep_rh (", "P2 in wave pairs", "leftover columns as 4x4x1 MFMAs"],
       ["H.comp.leftover_4x4x1", "H.frames.split_round"]),
    _c("rh_plain_449", 449, 9000, 250, 1, "full", "scalar", ["k_hstep_rh (4 P1 + 4 P2 + 4 loader waves on half tiles;"],
       ["H.frames.pipelined", "H.comp.remainder", "W.rows.extra_valu"]),
    # the plain k_hstep: fewer tiles than workgroups, W-only, beta = 0 / 0.5 / 1.5 / 2 (two statistics matrices, the Gram form)
    _c("plain_few_tiles", 257, 1000, 40, 1, "full", "entry", ["hstep: k_hstep,", "grid=34 x"], ["W.rows.extra_valu", "H.comp.remainder"]),
    _c("plain_wonly", 257, 2000, 40, 1, "w", "scalar", ["hstep: k_hstep,", "k_wfin"], ["W.rows.extra_valu", "W.comp.remainder"]),
    _c("plain_is_F33", 33, 3000, 20, 0.0, "full", "scalar", ["hstep: k_hstep,", "beta=0 "], ["W.rows.extra_valu", "H.frames.last_partial_tile"],
       data="wide"),
    _c("plain_b05_F64", 64, 2000, 40, 0.5, "full", "rvec", ["hstep: k_hstep,", "beta=0.5 "], ["H.frames.last_partial_tile"], data="wide"),
    _c("plain_b15_F257", 257, 1500, 60, 1.5, "full", "entry", ["hstep: k_hstep,", "beta=1.5 "], ["W.rows.extra_valu", "H.frames.last_partial_tile"],
       data="wide"),
    _c("plain_ed_gram_F513", 513, 1200, 100, 2.0, "full", "zero", ["hstep: k_hstep,", "NK=4", "Gram matrix"],
       ["W.rows.extra_valu", "H.frames.last_partial_tile"]),
    _c("wstats_nk16_gram", 257, 4000, 400, 2.0, "full", "scalar", ["NK=16", "1 kgroups", "Gram matrix"], ["W.rows.extra_valu"]),
    _c("wstats_nk16_kg2_kl", 65, 3000, 600, 1.0, "full", "rvec", ["NK=16", "2 kgroups"], ["W.rows.extra_valu", "H.comp.remainder"]),
    _c("wstats_gram_quiet", 129, 3000, 100, 2.0, "full", "zero", ["Gram matrix"], ["W.rows.extra_valu"], data="quiet"),
    # small F: k_iter_sf (its shared remainder tile), k_hstep_sf (tiles shared by four waves), k_wstats_sf (its single remainder tile)
    _c("isf_F64_r70", 64, 12031, 70, 1, "full", "scalar", ["k_iter_sf (", "remainder tile shared by the four pairs"],
       ["H.frames.shared_remainder", "H.frames.last_partial_tile"]),
    _c("isf_F64_r100", 64, 9000, 100, 1, "full", "rvec", ["k_iter_sf (", "remainder tile shared by the four pairs"],
       ["H.frames.shared_remainder"]),
    _c("isf_F64_r96", 64, 9001, 96, 1, "full", "entry", ["k_iter_sf ("], ["H.frames.shared_remainder", "H.frames.last_partial_tile"]),
    _c("isf_F48_r128", 48, 12000, 128, 1, "full", "zero", ["k_iter_sf ("], ["H.frames.shared_remainder", "W.rows.last_partial_tile"]),
    _c("hsf_shared_r200", 64, 35000, 200, 1, "full", "rvec", ["k_hstep_sf (", "the last 70 shared by four waves each", "NK=8"],
       ["H.frames.shared_tiles"]),
    _c("hsf_wsf_remainder", 64, 12000, 40, 1, "full", "entry", ["k_hstep_sf (", "a single remainder tile shared by the eight waves"],
       ["H.frames.whole_tiles"]),
    _c("hsf_honly_F32", 32, 12000, 100, 1, "h", "zero", ["k_hstep_sf (", "on the H step's last workgroup"], ["H.frames.whole_tiles"]),
    _c("hsf_F40_r20", 40, 33000, 20, 1, "full", "scalar", ["k_hstep_sf (", "k_wstats_sf: a tile per wave"],
       ["W.rows.last_partial_tile", "H.frames.last_partial_tile"]),
    # small rank: k_hstep_sr / k_wstats_sr, k_wfin's row slices (r <= 32)
    _c("sr_F513_r20", 513, 12000, 20, 1, "full", "scalar", ["k_hstep_sr (", "k_wstats_sr", "k_wfin"], ["W.rows.extra_valu"]),
    _c("sr_wonly_r10", 513, 9000, 10, 1, "w", "scalar", ["k_wstats_sr", "k_wfin"], ["W.rows.extra_valu"]),
    _c("sr_honly_F257", 257, 20000, 32, 1, "h", "rvec", ["k_hstep_sr (", "on the H step's last workgroup"], ["H.frames.last_tile"]),
    _c("sr_F385_r10", 385, 12001, 10, 1, "full", "entry", ["k_hstep_sr (", "k_wstats_sr"], ["H.frames.last_partial_tile"]),
    _c("sr_semi_F422", 422, 17725, 32, 1, "semi", "zero", ["k_hstep_sr (", "k_wstats_sr"], ["W.comp.fixed", "W.rows.last_partial_tile"]),
    # the out-of-envelope path (csrc/snmf_generic.h): its H-only objective is folded by k_reduce
    _c("generic_2700", 2700, 700, 40, 1, "full", "scalar", ["out-of-envelope", "1 frame splits"]),
    _c("generic_b15_2600", 2600, 300, 24, 1.5, "full", "rvec", ["out-of-envelope"], data="wide"),
    _c("generic_wonly_r1100", 129, 5000, 1100, 1, "w", "scalar", ["out-of-envelope", "3 frame splits"]),
    _c("generic_is_honly_kreduce", 2800, 300, 30, 0.0, "h", "entry", ["out-of-envelope"]),
    _c("generic_semi_2600", 2600, 200, 16, 1, "semi", "zero", ["out-of-envelope"], ["W.comp.fixed"]),
    # the headline: C2, KL full at 257 x 100 000, r = 256 (one step: the fp64 reference is the cost)
    _c("headline_c2", 257, 100000, 256, 1, "full", "scalar", ["k_hstep_rp (", "split 4 ways", "NK=8"],
       ["H.frames.split_round", "W.rows.extra_valu"], steps=1),
]


def case_masks(mode, r):
    """(w_update_ind, h_update_ind) of a case's mode (as tests/test_plan_geometry.masks)."""
    if mode == "h":
        return np.zeros(r, bool), None
    if mode == "w":
        return None, np.zeros(r, bool)
    if mode == "semi":
        w = np.ones(r, bool)
        w[: r // 2] = False
        return w, None
    return None, None


def case_data(case):
    """(V32, W0, H0, S) of a case: deterministic per case id."""
    F, T, r = case["F"], case["T"], case["r"]
    rs = np.random.default_rng(sum(map(ord, case["id"])) * 7919 + F)
    V = rs.gamma(0.5, 1.0, (F, 16)) @ rs.gamma(0.3, 1.0, (16, T)) + 1e-3
    if case["data"] == "wide":
        V = V ** 3 * 1e3
    elif case["data"] == "quiet":
        V[F // 3: F // 3 + 5] = 1e-6
        V[:, 7::37] = 1e-6
    W0 = rs.random((F, r))
    H0 = rs.random((r, T)).astype(np.float32)
    S = {"scalar": 1.0, "zero": 0.0, "rvec": rs.uniform(0.0, 2.0, r), "entry": rs.uniform(0.0, 2.0, (r, T))}[case["sp"]]
    return V.astype(np.float32), W0, H0, S
