"""Element-wise judgement of ONE frame step of the batched online separator, from the device's own state g.  Test infrastructure
(like elementwise.py): no test functions here; imported by tests/test_online_step_rules.py (CPU), tests/test_gpu_online_step.py and
tests/test_gpu_online_single_step.py -- the single-stream OnlineSeparator returns the same record from get_state and is judged by
the same functions, one separator per stream (run_single, judge_run, SINGLE_CASES and wadapt_regions below; why its kernels need
no other bound is derived in that test's docstring).

THE METHOD.  OnlineBatchSeparator.get_state returns a stream's whole state g as a value, in the oracle's field names and ring order.
A batch of three streams is fed ONE hop per process call, with a get_state around every hop.  The fields of g_before are cast
exactly to fp64, the frame buffer y is y_hist followed by the hop, and oracle.online_oracle.sep_frame(y, l, g, p, H0) gives the
reference's g_after, its three synthesis frames and its trace.  g_after of the device is compared with it PER ELEMENT, field by
field and region by region.  Every frame is judged alone, from the device's own previous state: nothing accumulates over frames, a
decision that flips on frame l does not spoil frame l + 1, and no norm dilutes one bin, one ring slot or one dictionary column.

WHAT EACH FIELD JUDGES (kernel; oracle/online_oracle.py lines of sep_frame and blk_sparse)
  Ad_blk[:, -1] on a triggered frame = A[R_x : R_x + R_a]   k_hsolve_frame<.., BATCH = true> (snmf_kernels.h), activation by
                                                            activation (:167-168, :219); past its envelope the batch refuses
  trace A_x_mag, A_d_mag, beta, Q_control                   the sums of the same solve and k_obpost's scalars (:186-192, :207)
  r_blk[:, -1]                                              k_obpost / opost_frame: the reconstructions and blk_sparse :80-83
  lambda_dav                                                opost_frame :193 (Ds * beta, the smoothing)
  Xm_tilde                                                  opost_frame :196-205 (Wiener / MMSE gain, Q of blk_sparse, the init branch)
  lambda_d_blk[:, -1] on a triggered frame                  opost_frame :211-218 (D_ref, both branches of l <= init_N_len)
  x_tilde_tail[-framelength:]                               k_obistft / k_obtail: the reference's returned synthesis frame (:249-253)
  x_hat_tail, d_hat_tail, class_tails (class outputs)       k_obclass / oclass_dft and the same synthesis: B(:, R_c) * A(R_c) per class
  B_DFT_d (Mel mode: B_Mel_d) after `solved`                    k_wadapt_batch (the updated columns), k_obassemble / k_obrefresh (the order
                                                            [rem, B_tmp, fix] of :241)
The updated columns are judged from the device's OWN rings after the frame (W step of elementwise.ref_wstep on V = lambda_d_blk,
H = the r_up rows of Ad_blk, W = the r_up columns of the dictionary before the frame): one W step and nothing else, as the issue's
tau_w asks (the rules test pins that step to the oracle's own adaptation solve on the pure oracle run: judge(pin_oracle=True)).

THE BOUNDS (one-step cases: max_iter = 1, conv_eps = 0).  u is the unit roundoff of the mode (2^-24; fp64 mode 2^-53).  All bounds
are ABSOLUTE (relative part times |reference| plus absolute terms), first-order propagations through the formulas of sep_frame with
the condition numbers taken from the reference's own intermediates.  They are worst cases and are not fitted to a device.
  spectrum   Y = fft(win .* y): the window image and the product perturb every input by 2u, the radix-2 transform by at most
             eta log2(N) ||Y||_2 with eta = 7u (Higham, Accuracy and Stability, Thm 24.2: mu + gamma_4 (sqrt 2 + mu)), so every bin
             has |dY| <= eY = (7 log2 N + 2) u ||Y||_2.  Ym = |Y|^2 + flr:  dV_f = 2 |Y_f| eY + eY^2 + 4u Ym_f  (bins < DCbin: u flr).
  A          one H step: elementwise.tau_h(F, r, beta, "h") + 4u for H0 .* wn and the W image: the bound the newest Ad_blk column is
             judged under.  What is PROPAGATED into the fields below also carries the step's response to dV: the numerator
             W'(V .* Lam^(beta-2)) is linear in V, so  tauA_k = tau_h + 4u + (W' (dV .* Lam^(beta-2)))_k / (W' (V .* Lam^(beta-2)))_k.
  A_x_mag, A_d_mag   means of non-negative terms in any order: the weighted mean of tauA, + (R + 2) u.  The trace is float in every mode: + 2^-24.
  beta       20 log10(A_d_mag / A_x_mag) beta0, clamped (a clamp is 1-Lipschitz):  (20 / ln 10)(dA_d + dA_x + 4u) beta0 + 2u |raw|.
  Xs, Ds     B * A, non-negative r-term chains on the images of B and h .* wn:  dXs = Bx (A_x .* tauA_x) + (r + 6) u Xs.
  r_blk[:, -1]   snr = Xs ./ max(Ds, flr) / max(.): d_f = dXs_f / Xs_f + dDs_f / Ds_f + 4u; the maximum moves by at most the largest
             |d snr| (sup norm):  snr_f (d_f + max_g snr_g d_g / max snr).
  Q          P = (sqrt n - l1 / l2) / (sqrt n - 1) SUBTRACTS: absolute.  l1 and l2^2 are sums of non-negative ring entries of which
             only the newest column carries an error (the others are the device's own state):
             dP = (l1 / l2) (dl1 / l1 + dl2sq / (2 l2^2) + (n + 4) u) / (sqrt n - 1),  dQ = (1 - alpha_p) dP + 3u Q;  Q_control: mean dQ + (F + 2) u mean Q + 3u.
  lambda_dav alpha_d * old + (1 - alpha_d) Ds beta, non-negative:  alpha_d old 4u + (1 - alpha_d)(beta dDs + Ds dbeta + 6u Ds beta)
             (frame 1 starts from Ym: + alpha_d dV).
  gain       MMSE: eta = num / max(lambda_dav, flr), num = a Xm_tilde_old + (1 - a) Xs Q: dnum = 4u num + (1 - a)(Q dXs + Xs dQ);
             d eta / eta = dnum / num + dlambda / lambda + 2u;  G = eta / (eta + 1): dG / G = (d eta / eta) / (1 + eta) + 3u.
             Wiener: G = Xs / (Xs + Ds): dG / G = (1 - G)(dXs / Xs + dDs / Ds) + 3u.   1 - G subtracts: d(1 - G) = dG, absolute.
  Xm_tilde   G Ym: Ym dG + G dV + 2u G Ym;  init frames (G = flr): flr (dV + 2u Ym).
  lambda_d_blk[:, -1]   Ym (1 - G): Ym dG + (1 - G) dV + 3u Ym (1 - G); bins < DCbin: flr (dV + 2u Ym); init frames: dV + u Ym.
  synthesis  Z = sqrt(Xm_tilde) .* phase: |dZ_f| <= dXm_f / (2 sqrt Xm_f) + sqrt(G_f) eY (the phase of a bin is known to eY / |Y_f|)
             + 3u |Z_f|; the inverse transform adds 7 log2(N) u ||Z||_2 sqrt N (the treatment of tests/test_gpu_frontend_envelope.py:
             c log2(N) u of the frame's scale, absolute):  ds_n = overlapscale / N * win_n (sum_k |dZ_k| + 7 log2 N u sqrt N ||Z||_2) + 3u |s_n|.
  B_DFT_d    updated columns: elementwise.tau_w(F, n_up, beta, m_a, "w") (+ 4u: W ./ wn and h .* wn before the step) from the device's
             own rings, plus 4 x the smallest normal number of the format (the standard model with underflow: repeated
             multiplicative updates drive dictionary entries below 2^-126); rem and fix columns are bit copies of the fp64 master.
             (The dV terms were derived before any run, as elementwise.py derives dV of a masked solve: V of this step is the
             device's own spectrum, no exact input.  That they are needed shows on the CPU alone: with eY = 0 both emulations break
             the bounds of Xm_tilde and lambda_d_blk by up to 1e4 x and of the synthesis by 3 x in case 1.  A itself stays inside
             tau_h + 4u in both emulations (<= 0.12 of it in cases 1-4), so A is judged under tau_h + 4u alone.)
  MEL MODE   (k_obmel, k_obprep_mel; :148-154, :170-177, :224-230; fp32 only.)  The solve's V is the Mel features
             Vs = (M / ||M|| + 1e-9) ||Ym||, M = melmat Ym: dM = melmat dV + (F + 2) u M; the two norms move by at most
             ||dM|| / ||M|| + (F_order / 2 + 2) u and ||dV|| / ||Ym|| + (F / 2 + 2) u;  dVs = ||Ym|| (dM / ||M|| + M / ||M|| rel_vn) +
             Vs (rel_tn + 4u).  A: tau_h(F_order, r, beta) + 4u + the response to dVs -- V of this step is formed by the device
             from its spectrum, so, as for a masked solve in elementwise.py, dVs is part of A's own bound here.  MelConv = 1:
             Xs = melmat' (B_Mel_x A_x), an r-term chain under an F_order-term chain: dXs = melmat' (B dA + (r + 6) u Xm) +
             (F_order + 2) u Xs, and frame 1's lambda_dav starts from melmat' Vs.  MelConv = 0: the DFT bases on the Mel
             activations, as in DFT mode.  The updated columns of B_Mel_d: tau_w(F_order, n_up, beta, m_a) + 4u + 4 (F + 2) u, the
             last term elementwise.py's rule for a V that is no exact input (melmat * lambda_d_blk is an F-term chain on the
             device's own ring).  melmat is the float image the device holds; a bin no Mel filter reaches has Xs = Ds = 0 on both
             sides and is left out of r_blk by the floor rule (counted).
FLOORS.  max(x, flr), max(0.0031, eta) and min(G, 1) are 1-Lipschitz: a clamped value moves by no more than the unclamped one, so
the absolute bounds above hold on either side of such a floor and those elements are judged (stricter than leaving out every
element within 10x of a floor).  Where a bound is a RELATIVE propagation that divides by a floored quantity the issue's rule
is kept as written: a frame whose Lam is within 10x of flr is left out whole (tau_h does not hold there), and the elements
whose Xs or Ds is within 10x of flr are left out of r_blk (and, with the Wiener gain, of Xm_tilde and lambda_d_blk); both are
counted and capped (Tally.caps_ok: 10 % of the pairs, 2 % of a field's elements, 2 % of the r_up rows).  What IS left out, and counted, are decisions on the reference's own margin -- a trig or r_up
comparison whose two sides are within the bound of their operands -- with the fields that depend on them (the borderline rule of
tests/fuzz_cases.py); the cap is 10 % of the judged (frame, stream) pairs and no frame with `solved`.

THE CHECK OF THE BOUNDS BEFORE A GPU IS USED.  frame_step() below restates the whole step once more over a number type: in fp64 it
must agree with sep_frame to rounding (which pins the restatement), in float32 -- every operation rounded, the sums taken once in
index order and once reversed -- it must stay inside every bound on every case, and its RMS error per field is the yardstick of
the second, finer check: the device's RMS relative error per field is at most 4 x the larger emulation's (floor: u / sqrt 3;
synthesis frames: the error relative to the frame's own RMS, since single samples cross zero).
The planted errors of tests/test_online_step_rules.py are switches of the same restatement in fp64.

MEASURED on an MI355X at commit 503c09f plus these tests (the full table per case and field: docs/KERNELS.md, "How the online frame
step is judged"; tests/test_online_step_rules.py prints the emulations' figures, tests/test_gpu_online_step.py the device's):
  twelve cases, 110 ... 254 (frame, stream) pairs each, 32 ... 64 frames with `solved`; no decision differed, no r_up row was on the
  reference's margin, no frame and no element was left out.  Worst element / bound: A 0.007 ... 0.075 (under tau_h + 4u alone),
  lambda_dav <= 0.014, r_blk <= 0.005, Xm_tilde and lambda_d_blk <= 0.02 away from the DC bins (0.32 on them: the float image of
  flr), updated dictionary columns 0.010 ... 0.046, synthesis frames <= 0.002, trace scalars <= 0.24 (fp64 mode 0.94: the float
  conversion is most of their bound, so they judge little there).  Device RMS / emulation RMS: 0.12 ... 1.35 (the limit is 4).
  Mel mode (case 7, MelConv 1 / 0): A 0.005 / 0.004, updated B_Mel_d columns 0.008 / 0.007, RMS ratios 0.35 ... 1.19.
  One rank past the frame kernel (case 6) the batched separator refuses the geometry, which is asserted.
  THE STOP-ARMED CASES 10 AND 11 have their reference run, their amplification measurement, their bound 4 n_iter tau max(1, amp_e)
  and their borderline counting at the end of this module (STOP_CASES, stop_armed_oracle_run), and the rules test asserts on the
  CPU what they reach; they are NOT judged on the device, because the issue's borderline rule and its cap exclude each other.
  In the pure oracle run a relative cost change within 5 % of conv_eps occurs at an iteration of the frame solve or of the
  adaptation solve on 67 of the 110 pairs of case 11 (25 of its 35 frames with `solved`; median 16 iterations, at most 30) and on
  65 of the 80 pairs of case 10 (55 of 70; median 25, at most 40; adaptation up to 43): the cost change falls by 10 ... 20 % per
  iteration, so most solves have an iterate inside a band 10 % wide, whatever the seed, against a cap of 10 % of the pairs and no
  frame with `solved`.  On the pairs that are left (43 and 15) no draw changed a decision; amp_e has a median of 0.6 and reaches
  7.3e4 (case 11) and 2.1e4 (case 10) on single elements.  One of the two has to be restated in the issue first.
"""
from __future__ import annotations

import numpy as np

from elementwise import U, ref_wstep, tau_h, tau_w
from oracle.online_oracle import frame_stft, sep_frame, synth_ifft_buff

U64 = 2.0 ** -53
C_FFT = 7.0     # eta / u of one radix-2 stage (module docstring)
RMS_FACTOR = 4.0
TINY = {U: 2.0 ** -126, U64: 2.0 ** -1022}  # smallest normal number of the mode's format

PLANTS = ("extra_row", "xs_column", "ad_last", "alpha_d_swapped", "q_prev", "ring_early", "swap_rem_tmp", "norm_neighbour",
          "syn_shift", "init_long", "wg_partial", "r_up_shift")
# what the failure of each planted error must name: the field and the region (all of these substrings in one failure message)
PLANT_FIELDS = {"extra_row": ("field Ad_blk,", "region all"), "xs_column": ("field r_blk,", "region all"),
                "ad_last": ("field Ad_blk,", "region last_activation"), "alpha_d_swapped": ("field lambda_dav,", "region all"),
                "q_prev": ("field Xm_tilde,", "region blk_bins"), "ring_early": ("field ring lambda_d_blk:",),
                "swap_rem_tmp": ("field B_DFT_d,", "region rem"), "norm_neighbour": ("field B_DFT_d,", "region B_tmp:"),
                "syn_shift": ("field x_tilde_tail,", "region all"), "init_long": ("frame 6:", "field Xm_tilde,", "region all"),
                # the two that belong to the single-stream adaptation (k_wadapt's exchange, the r_up mask k_oprep writes to w_ind)
                "wg_partial": ("field B_DFT_d,", "region B_tmp.wg_low"), "r_up_shift": ("field B_DFT_d,", "region rem")}


def beta_of(p):
    return {"is": 0.0, "kl": 1.0, "ed": 2.0}.get(p.get("cf", "kl"), float(p.get("beta_div", 1.0)))


# ---- the step over a number type ---------------------------------------------------------------------------------------------

class _Arith:
    """Every operation rounded to dt.  seq: sums sequential in index order (rev: reversed) -- the emulations; otherwise numpy's own
    sums (the fp64 restatement that is pinned to the oracle)."""

    def __init__(self, dt, rev=False, seq=None):
        self.dt, self.rev = np.dtype(dt).type, rev
        self.seq = (self.dt is np.float32) if seq is None else seq  # sequential sums in dt (the emulations) or numpy's own

    def c(self, x):
        return np.asarray(x, dtype=self.dt)

    def sum(self, x, axis=-1):
        if not self.seq:
            return np.sum(x, axis=axis)
        x = np.asarray(x, dtype=self.dt)
        if x.shape[axis] == 0:
            return np.zeros(np.delete(x.shape, axis), self.dt)
        if self.rev:
            x = np.flip(x, axis=axis)
        return np.take(np.cumsum(x, axis=axis, dtype=self.dt), -1, axis=axis)

    def mv(self, M, v):
        return self.sum(M * v[None, :], axis=1)

    def tmv(self, M, v):
        return self.sum(M * v[:, None], axis=0)

    def mm(self, A, B):
        if not self.seq:
            return A @ B
        acc = np.zeros((A.shape[0], B.shape[1]), self.dt)
        for k in (range(A.shape[1] - 1, -1, -1) if self.rev else range(A.shape[1])):
            acc = acc + A[:, k, None] * B[None, k, :]
        return acc

    def fft(self, x):
        ct = np.complex128 if self.dt is np.float64 else np.complex64
        x = np.asarray(x).astype(ct)
        if not self.seq:
            return np.fft.fft(x)
        # fft_lds of csrc/snmf_online_common.h: the radix-2 Stockham autosort transform, twiddles formed in double and rounded to dt
        N = x.size
        tw = np.exp(-2j * np.pi * np.arange(N // 2) / N).astype(ct)
        idx = np.arange(N // 2)
        l, m = N // 2, 1
        while l >= 1:
            j, k = idx // m, idx % m
            c0, c1 = x[k + j * m], x[k + j * m + l * m]
            y = np.empty(N, ct)
            y[k + 2 * j * m] = c0 + c1
            y[k + 2 * j * m + m] = tw[j * (N // (2 * l))] * (c0 - c1)
            x, l, m = y, l // 2, m * 2
        return x


def _blk_q(ar, ring, l, p, F):
    """blk_sparse :84-97 on a ring whose newest column is in place."""
    c = ar.c
    Q = np.concatenate([np.zeros(p["DCbin"]), 0.1 * np.ones(F - p["DCbin"])]).astype(ar.dt)
    n = p["P_len_l"] * p["P_len_k"]
    k2, gap2 = p["P_len_k"] // 2, (p["blk_gap"] - 1) // 2
    sqn, ap = c(np.sqrt(n)), c(p["alpha_p"])
    if l > p["P_len_l"]:
        for k in range(k2 + p["DCbin"], F - k2 + 1, p["blk_gap"]):
            b = ring[k - k2:k + k2, :].reshape(-1)
            l1 = ar.sum(b)
            l2 = np.sqrt(ar.sum(b * b))
            P_tmp = (sqn - l1 / l2) / (sqn - c(1))
            P_val = ap * Q[k - 2] + (c(1) - ap) * P_tmp
            Q[k - gap2 - 1:k] = P_val
            Q[k - 1:k + gap2] = P_val
        Q[:p["P_len_k"] - 1] = Q[p["P_len_k"] + p["DCbin"] - 1]
    Q[:p["DCbin"]] = 0
    return Q


def _w_step(ar, V, W0, H0, beta, flr, plant=None):
    """src/sparse_nmf.m:157-160 and one W update :212-243 with H fixed (oracle/sparse_nmf_oracle.py:137-139, :203-232): W0 the fp64
    columns, H0 their activation rows.  Returns the normalised columns in fp64."""
    c = ar.c
    wn = np.sqrt(np.sum(W0 ** 2, axis=0))
    W = c(W0 / wn)
    H = c(H0 * wn[:, None])
    HT = H.T.copy()
    V = np.fmax(c(V), flr)
    lam = np.fmax(ar.mm(W, H), flr)
    if beta == 1:
        G = ar.mm(V / lam, HT)
        s = ar.sum(H, axis=1)[None, :]
        dpw = s + ar.sum(G * W, axis=0)[None, :] * W
        dmw = G + ar.sum(s * W, axis=0)[None, :] * W
    else:
        if beta == 2:
            P, Qm = ar.mm(lam, HT), ar.mm(V, HT)
        else:
            P = ar.mm(lam ** c(beta - 1.0), HT)
            Qm = ar.mm(V * lam ** c(beta - 2.0), HT)
        dpw = P + ar.sum(Qm * W, axis=0)[None, :] * W
        dmw = Qm + ar.sum(P * W, axis=0)[None, :] * W
    Wn = W * dmw / np.fmax(dpw, flr)
    nrm = np.sqrt(ar.sum(Wn * Wn, axis=0))
    if plant == "wg_partial":  # one workgroup's partial left out of the cross_sum: the column norm over rows that skip rows 8..15
        keep = np.ones(Wn.shape[0], bool)
        keep[8:16] = False
        nrm = np.sqrt(ar.sum((Wn * Wn)[keep], axis=0))
    if plant == "norm_neighbour" and nrm.size >= 2:
        nrm = nrm.copy()
        nrm[0] = nrm[1]
    return (Wn / nrm[None, :]).astype(np.float64)


def class_cols(p, Rx, Rd):
    """p.EVENT_RANK / p.NOISE_RANK (1-based class starts, src/bnmf_sep_event_RT_IS16.m:158-163, :180-185) as column index arrays over
    the r columns of [B_x | B_d], event classes first; None for one class per side."""
    ev, nz = list(p.get("EVENT_RANK", [1])), list(p.get("NOISE_RANK", [1]))
    if len(ev) == 1 and len(nz) == 1:
        return None
    cols = [np.arange(a - 1, b - 1) for a, b in zip(ev, ev[1:] + [Rx + 1])]
    return cols + [Rx + np.arange(a - 1, b - 1) for a, b in zip(nz, nz[1:] + [Rd + 1])]


def after_state(g, ga, fr, sz):
    """A step's results as the state after the frame: every tail g holds shifted by one synthesis frame."""
    dev = dict(g, **ga)
    for tail, key in (("x_tilde_tail", "x_tilde"), ("x_hat_tail", "x_hat"), ("d_hat_tail", "d_hat")):
        if tail in g:
            dev[tail] = np.concatenate([g[tail][sz:], fr[key]])
    if "class_tails" in g:
        dev["class_tails"] = np.stack([np.concatenate([t[sz:], f]) for t, f in zip(g["class_tails"], fr["class"])])
    return dev


def frame_step(g, y, l, p, H0, Bx, dt=np.float64, rev=False, plant=None, seq=None):
    """One frame of sep_frame (pow = 2, preemph = 0, max_iter H steps without a stop) over the number type dt.
    g: the state before (fp64 values; rings in time order; B_DFT_d and B_fix the fp64 masters).  Returns (g_after, frames, trace)
    in the layout reference() returns.  plant: one of PLANTS.  B_sep_mode 'Mel' (:146-156, :170-177, :224-230): p["_melmat"]
    (F_order x F, the values the device holds) and p["_B_Mel_x"] are the mode's configuration, g["B_Mel_d"] its dictionary."""
    assert p["pow"] == 2 and p["preemph"] == 0.0
    mel = p.get("B_sep_mode", "DFT") == "Mel"
    melconv = mel and bool(p.get("MelConv", 1))
    ar = _Arith(dt, rev, seq)
    c = ar.c
    F, Rx = Bx.shape
    Bd = np.asarray(g["B_DFT_d"], np.float64)
    Rd = Bd.shape[1]
    Ra, ma, dcb, N, sz = p["R_a"], p["m_a"], p["DCbin"], p["fftlength"], p["framelength"]
    flr, one = c(p["nonzerofloor"]), c(1)
    beta_div = beta_of(p)
    # ---- :121-135 the frame's spectrum
    pad = np.zeros(N, ar.dt)
    pad[:sz] = c(p["win_STFT"]) * c(y)
    Y = ar.fft(pad)[:F]
    mag = np.sqrt(Y.real * Y.real + Y.imag * Y.imag)
    Ym = mag * mag
    Ym[:dcb] = 0
    Ym = Ym + flr
    with np.errstate(all="ignore"):
        ph = np.where(mag > 0, Y / np.where(mag > 0, mag, 1), 1)
    # ---- :157-168 the supervised solve: max_iter H steps (src/sparse_nmf.m:157-160, :189-207)
    if mel:  # :148-154 the Mel features, normalised to the frame's own norm
        mm = c(p["_melmat"])
        Ymel = ar.mv(mm, Ym)
        vn, tn = np.sqrt(ar.sum(Ymel * Ymel)), np.sqrt(ar.sum(Ym * Ym))
        Ymel = (Ymel / vn + c(1e-9)) * tn
        BMd = np.asarray(g["B_Mel_d"], np.float64)
        W0 = np.concatenate([np.asarray(p["_B_Mel_x"], np.float64), BMd], axis=1)
        V = np.fmax(Ymel, flr)
    else:
        W0 = np.concatenate([np.asarray(Bx, np.float64), Bd], axis=1)
        V = np.fmax(Ym, flr)
    wn = np.sqrt(np.sum(W0 ** 2, axis=0))
    W = c(W0 / wn)
    h = c(np.asarray(H0, np.float64) * wn)
    sp = c(p["sparsity"])
    assert p["conv_eps"] == 0  # (max_iter H steps without a stop: the one-step cases)
    # the semi-supervised frame solve (:125-131; src/sparse_nmf.m:212-243): the noise (basis_update_N) or the event columns of the
    # solve's PRIVATE W are updated after every H step and all columns renormalised, H not rescaled; the frame keeps A only
    w_ind = None
    if p.get("basis_update_N", 0):
        w_ind = np.arange(Rx, W.shape[1])
    elif p.get("basis_update_E", 0):
        w_ind = np.arange(Rx)
    n_it = int(p["max_iter"])
    for it in range(n_it):
        Wd = W[:-1] if plant == "extra_row" else W  # (the planted error: the extra row F - 1 left out of W' * ratio)
        if it and w_ind is not None:  # the W step that closed the previous iteration (the last one's W is discarded)
            lam = np.fmax(ar.mv(W, h), flr)
            ww, hw = W[:, w_ind], h[w_ind][None, :]
            if beta_div == 1:
                G = (V / lam)[:, None] * hw
                dpw = hw + ar.sum(G * ww, axis=0)[None, :] * ww
                dmw = G + ar.sum(hw * ww, axis=0)[None, :] * ww
            else:
                P = (lam if beta_div == 2 else lam ** c(beta_div - 1.0))[:, None] * hw
                Qm = (V if beta_div == 2 else V * lam ** c(beta_div - 2.0))[:, None] * hw
                dpw = P + ar.sum(Qm * ww, axis=0)[None, :] * ww
                dmw = Qm + ar.sum(P * ww, axis=0)[None, :] * ww
            W = W.copy()
            W[:, w_ind] = ww * dmw / np.fmax(dpw, flr)
            W = W / np.sqrt(ar.sum(W * W, axis=0))[None, :]
            Wd = W[:-1] if plant == "extra_row" else W
        lam = np.fmax(ar.mv(W, h), flr)
        if beta_div == 1:
            dph, num = ar.sum(W, axis=0) + sp, V / lam
        elif beta_div == 2:
            dph, num = ar.tmv(W, lam) + sp, V
        else:
            dph, num = ar.tmv(W, lam ** c(beta_div - 1.0)) + sp, V * lam ** c(beta_div - 2.0)
        dmh = ar.tmv(Wd, num[:-1] if plant == "extra_row" else num)
        h = h * dmh / np.fmax(dph, flr)
    A = h
    # ---- :175-176 reconstructions
    Ax_, Bxc = A[:Rx], c(Bx)
    if plant == "xs_column":
        Ax_, Bxc = np.delete(Ax_, Rx // 2), np.delete(Bxc, Rx // 2, axis=1)
    Ymd = Ym
    if melconv:  # :170-173 the reconstructions in the Mel domain, mapped back with melmat'
        Xs = ar.tmv(mm, ar.mv(c(W0[:, :Rx]), A[:Rx]))
        Ds = ar.tmv(mm, ar.mv(c(W0[:, Rx:]), A[Rx:]))
        Ymd = ar.tmv(mm, Ymel)
    else:  # DFT mode, or Mel activations on the DFT bases
        Xs = ar.mv(Bxc, Ax_)
        Ds = ar.mv(c(Bd), A[Rx:])
    # ---- blk_sparse :76-98
    ring_old = c(g["r_blk"])
    if p["blk_sparse"]:
        snr = Xs / np.fmax(Ds, flr)
        snr = snr / np.max(snr)
        r_new = np.concatenate([ring_old[:, 1:], snr[:, None]], axis=1)
        Q = _blk_q(ar, r_new, l, p, F)
    else:
        r_new, Q = ring_old, np.ones(F, ar.dt)
    # ---- :184-205 the gain
    A_d_mag = ar.sum(A[Rx:]) / c(Rd)
    A_x_mag = ar.sum(A[:Rx]) / c(Rx)
    with np.errstate(all="ignore"):
        beta = c(20.0 * np.log10(np.float64(A_d_mag) / np.float64(A_x_mag))) * c(p["beta"])
    beta = c(min(max(beta, c(p["beta"])), c(p["beta_max"])))
    ld_old = Ymd if l == 1 else c(g["lambda_dav"])
    ad = c(p["alpha_d"])
    if plant == "alpha_d_swapped":
        ld = (one - ad) * ld_old + ad * Ds * beta
    else:
        ld = ad * ld_old + (one - ad) * Ds * beta
    if p["ENHANCE_METHOD"] == "Wiener":
        G = Xs / (Xs + Ds)
    else:
        Qg = _blk_q(ar, ring_old, l - 1, p, F) if (plant == "q_prev" and p["blk_sparse"]) else Q
        ae = c(p["alpha_eta"])
        eta = (ae * c(g["Xm_tilde"]) + (one - ae) * Xs * Qg) / np.fmax(ld, flr)
        eta = np.fmax(c(0.0031), eta)
        G = eta / (eta + one)
    G = np.fmin(G, one)
    init = l <= p["init_N_len"] + (1 if plant == "init_long" else 0)
    if init:
        G = np.zeros(F, ar.dt) + flr
        A_x_mag = flr
    Xt = G * Ym
    # ---- :207-247 the adaptation
    Q_control = (one - ar.sum(Q) / c(F)) * c(p["Ar_up"])
    trig = bool(p["adapt_train_N"] and (Q_control * A_d_mag > A_x_mag))
    ga = dict(Xm_tilde=Xt, lambda_dav=ld, r_blk=r_new, lambda_d_blk=c(g["lambda_d_blk"]), Ad_blk=c(g["Ad_blk"]), B_DFT_d=Bd,
              update_switch=int(g["update_switch"]), n_push=int(g["n_push"]), l=int(l) + 1)
    if mel:
        ga["B_Mel_d"] = BMd
    n_up, solved = 0, False
    r_up = np.zeros(Ra, bool)
    if trig:
        if init:
            D_ref = Ym.copy()
        else:
            M_ref = one - G
            M_ref[:dcb] = flr
            D_ref = Ym * M_ref
        a_new = A[Rx:Rx + Ra].copy()
        if plant == "ad_last":
            a_new[-1] = A[Rx + Ra]
        if plant == "ring_early":
            put = lambda ring, col: np.concatenate([ring[:, 1:-1], col[:, None], ring[:, -1:]], axis=1)  # noqa: E731
        else:
            put = lambda ring, col: np.concatenate([ring[:, 1:], col[:, None]], axis=1)  # noqa: E731
        ga["lambda_d_blk"], ga["Ad_blk"] = put(ga["lambda_d_blk"], D_ref), put(ga["Ad_blk"], a_new)
        ga["n_push"] += 1
        r_up = Q_control * (ar.sum(ga["Ad_blk"], axis=1) / c(ma)) > A_x_mag
        if plant == "r_up_shift":  # the mask the adaptation solve reads, shifted by one column
            r_up = np.roll(r_up, 1)
        n_up = int(r_up.sum())
        if ga["update_switch"] == int(np.floor(p["overlap_m_a"] * ma)):
            Bsrc = BMd if mel else Bd  # :224-230: Mel mode adapts B_Mel_d on melmat * lambda_d_blk, and its fix columns are its own
            key = "B_Mel_d" if mel else "B_DFT_d"
            Vad = ar.mm(mm, ga["lambda_d_blk"]) if mel else ga["lambda_d_blk"]
            rem, fix = Bsrc[:, :Ra][:, ~r_up], (BMd if mel else np.asarray(g["B_fix"], np.float64))[:, Ra:]
            if n_up:
                assert p["max_iter"] == 1
                B_tmp = _w_step(ar, Vad, Bsrc[:, :Ra][:, r_up], np.asarray(ga["Ad_blk"], np.float64)[r_up], beta_div, flr, plant)
                solved = True
                ga[key] = np.concatenate([B_tmp, rem, fix] if plant == "swap_rem_tmp" else [rem, B_tmp, fix], axis=1)
            else:
                ga[key] = np.concatenate([rem, fix], axis=1)
            ga["update_switch"] = 1
        else:
            ga["update_switch"] += 1
    # ---- :249-253 the synthesis (src/synth_ifft_buff.m)
    half, scale, wi = N // 2, c(p["overlapscale"] / N), c(p["win_ISTFT"])

    def syn(M):
        m = np.array(M, dtype=ar.dt)
        m[:p["DCbin_back"]] = 0
        Z = np.sqrt(m) * ph
        full = np.concatenate([Z, np.conj(Z[1:half][::-1])])
        s = ar.fft(np.conj(full)).real[:sz] * scale * wi
        return np.roll(s, 1) if plant == "syn_shift" else s

    frames = dict(x_tilde=syn(Xt), x_hat=syn(Xs), d_hat=syn(Ds))
    cc = class_cols(p, Rx, Rd)
    if cc is not None:  # :158-202 per class, from the dictionary the frame solve saw
        Bc = c(W0)
        frames["class"] = [syn(ar.mv(Bc[:, cols], A[cols])) for cols in cc]
    trace = dict(n_iter=int(p["max_iter"]), trig=trig, n_up=n_up, solved=solved, adapt_iters=int(p["max_iter"]) if solved else 0,
                 beta=float(beta), A_x_mag=float(A_x_mag), A_d_mag=float(A_d_mag), Q_control=float(Q_control), A=A, G=G, Q=Q, r_up=r_up)
    return {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in ga.items()}, \
        {k: (np.asarray(v, np.float64) if k != "class" else [np.asarray(x, np.float64) for x in v]) for k, v in frames.items()}, trace


# ---- the reference: the oracle's own sep_frame from a state ---------------------------------------------------------------------

def state64(st):
    """A get_state dict with every array cast exactly to fp64."""
    return {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in st.items() if k != "record"}


def frame_buffer(g, hop_samples):
    return np.concatenate([np.asarray(g["y_hist"], np.float64), np.asarray(hop_samples, np.float64)])


def reference(g, y, p, Bx):
    """oracle.online_oracle.sep_frame from the state g (fp64 values, as state64 returns them) -> (g_after, frames, trace), the
    layout of frame_step."""
    l = int(g["l"])
    go = dict(Xm_tilde=g["Xm_tilde"].copy(), lambda_dav=g["lambda_dav"].copy(), lambda_Gy=np.zeros_like(g["Xm_tilde"]),
              r_blk=g["r_blk"].copy(), Ad_blk=g["Ad_blk"].copy(), lambda_d_blk=g["lambda_d_blk"].copy(),
              update_switch=int(g["update_switch"]), B_DFT_x=np.asarray(Bx, np.float64), B_DFT_d=g["B_DFT_d"].copy(),
              B_Mel_d=g["B_fix"].copy())
    mel = p.get("B_sep_mode", "DFT") == "Mel"
    if mel:
        go.update(B_Mel_x=np.asarray(p["_B_Mel_x"], np.float64), B_Mel_d=g["B_Mel_d"].copy(), melmat=np.asarray(p["_melmat"], np.float64))
    xt, xh, dh, tr = sep_frame(y, l, go, p, g["H0"])
    ga = dict(Xm_tilde=go["Xm_tilde"], lambda_dav=go["lambda_dav"], r_blk=go["r_blk"], lambda_d_blk=go["lambda_d_blk"], Ad_blk=go["Ad_blk"],
              B_DFT_d=go["B_DFT_d"], update_switch=go["update_switch"], n_push=int(g["n_push"]) + int(tr["trig"]), l=l + 1)
    if mel:
        ga["B_Mel_d"] = go["B_Mel_d"]
    fr = dict(x_tilde=xt, x_hat=xh, d_hat=dh)
    cc = class_cols(p, Bx.shape[1], g["B_DFT_d"].shape[1])
    if cc is not None:  # the oracle's own synthesis of B(:, R_c) * A(R_c) (:158-202; the driver's :105-119 per class)
        _, Yp = frame_stft(y, p)
        B = np.concatenate([np.asarray(Bx, np.float64), g["B_DFT_d"]], axis=1)
        fr["class"] = [synth_ifft_buff(B[:, cols] @ tr["A"][cols], Yp, p["framelength"], p["fftlength"], p["win_ISTFT"], p["preemph"],
                                       p["DCbin_back"], p["pow"]) * p["overlapscale"] for cols in cc]
    return ga, fr, tr


# ---- the bounds ----------------------------------------------------------------------------------------------------------------

def bounds(g, y, p, Bx, ga_ref, fr_ref, tr, u=U):
    """Absolute bounds per field (module docstring) of one one-step frame, around the reference's values.  Returns (bnd, margins):
    bnd[field] an array (or float for the trace scalars); margins: the reference's decision margins in units of their bound
    (< 1: borderline)."""
    l = int(g["l"])
    F, Rx = Bx.shape
    Bd = g["B_DFT_d"]
    Rd = Bd.shape[1]
    r = Rx + Rd
    Ra, ma, dcb, N, sz = p["R_a"], p["m_a"], p["DCbin"], p["fftlength"], p["framelength"]
    flr, L = p["nonzerofloor"], np.log2(p["fftlength"])
    beta_div = beta_of(p)
    init = l <= p["init_N_len"]
    Ym, _ = frame_stft(y, p)
    absY = np.sqrt(np.maximum(Ym - flr, 0.0))
    Y2 = np.sqrt(N) * np.linalg.norm(p["win_STFT"] * y)
    eY = (C_FFT * L + 2) * u * Y2
    dV = 2 * absY * eY + eY ** 2 + 4 * u * Ym
    dV[:dcb] = u * flr
    # A
    mel = p.get("B_sep_mode", "DFT") == "Mel"
    melconv = mel and bool(p.get("MelConv", 1))
    dVf, Fs = dV, F  # (the spectrum's own error; the solve's V and row count)
    if mel:  # the Mel features (module docstring, "Mel mode")
        mm = np.asarray(p["_melmat"], np.float64)
        n1 = Fs = mm.shape[0]
        M = mm @ Ym
        dM = mm @ dVf + (F + 2) * u * M
        vn, tn = np.linalg.norm(M), np.linalg.norm(Ym)
        rel_vn = np.linalg.norm(dM) / vn + (n1 / 2 + 2) * u
        rel_tn = np.linalg.norm(dVf) / tn + (F / 2 + 2) * u
        Vs = (M / vn + 1e-9) * tn
        dV = tn * (dM / vn + (M / vn) * rel_vn) + Vs * (rel_tn + 4 * u)
        W0 = np.concatenate([np.asarray(p["_B_Mel_x"], np.float64), g["B_Mel_d"]], axis=1)
    else:
        Vs = Ym
        W0 = np.concatenate([Bx, Bd], axis=1)
    wn = np.sqrt(np.sum(W0 ** 2, axis=0))
    W = W0 / wn
    lam = W @ (g["H0"] * wn)
    lam_floor = bool(lam.min() <= 10 * flr)  # tau_h does not hold there (elementwise.compare): the frame is left out and counted
    wgt = lam ** (beta_div - 2.0)
    V = np.fmax(Vs, flr)
    tau_step = (tau_h(Fs, r, beta_div, "h") / U) * u + 4 * u
    tauA = tau_step + (W.T @ (dV * wgt)) / (W.T @ (V * wgt))
    V, dV_solve, dV = np.fmax(Ym, flr), dV, dVf  # from here on V and dV are the DFT frame's again (the gain and the synthesis)
    A = tr["A"]
    dA = A * tauA
    Ax, Ad = A[:Rx].sum() / Rx, A[Rx:].sum() / Rd
    dAx, dAd = dA[:Rx].sum() / Rx + (Rx + 2) * u * Ax, dA[Rx:].sum() / Rd + (Rd + 2) * u * Ad
    raw = 20 * np.log10(Ad / Ax) * p["beta"]
    dbeta = (20 / np.log(10)) * (dAd / Ad + dAx / Ax + 4 * u) * p["beta"] + 2 * u * abs(raw)
    beta = tr["beta"]
    dYmd = dV  # what lambda_dav starts from at frame 1 (:185)
    if melconv:  # melmat' * (B_Mel * A): an r-term chain, then an F_order-term chain, all non-negative
        Xm, Dm = W0[:, :Rx] @ A[:Rx], W0[:, Rx:] @ A[Rx:]
        Xs, Ds = mm.T @ Xm, mm.T @ Dm
        dXs = mm.T @ (W0[:, :Rx] @ dA[:Rx] + (r + 6) * u * Xm) + (n1 + 2) * u * Xs
        dDs = mm.T @ (W0[:, Rx:] @ dA[Rx:] + (r + 6) * u * Dm) + (n1 + 2) * u * Ds
        dYmd = mm.T @ dV_solve + (n1 + 2) * u * (mm.T @ Vs)
    else:
        Xs, Ds = Bx @ A[:Rx], Bd @ A[Rx:]
        dXs = Bx @ dA[:Rx] + (r + 6) * u * Xs
        dDs = Bd @ dA[Rx:] + (r + 6) * u * Ds
    bnd = {}
    # elements whose relative propagation divides by a reconstruction within 10x of nonzerofloor: left out and counted
    near = (Xs <= 10 * flr) | (Ds <= 10 * flr)
    bnd["near_floor"] = near
    # r_blk newest column and Q
    Q = tr["Q"]
    if p["blk_sparse"]:
        Dsf = np.fmax(Ds, flr)
        snr0 = Xs / Dsf
        with np.errstate(all="ignore"):  # (a bin no Mel filter reaches has Xs = Ds = 0 on both sides: snr = 0 exactly)
            d = np.where(Xs > 0, dXs / np.where(Xs > 0, Xs, 1.0), 0.0) + dDs / Dsf + 4 * u
        mx = snr0.max()
        snr = snr0 / mx
        dsnr = snr * (d + (snr0 * d).max() / mx)
        bnd["r_blk"] = dsnr
        dQ = 3 * u * Q
        ring = ga_ref["r_blk"]
        if l > p["P_len_l"]:
            n = p["P_len_l"] * p["P_len_k"]
            k2, gap2 = p["P_len_k"] // 2, (p["blk_gap"] - 1) // 2
            for k in range(k2 + dcb, F - k2 + 1, p["blk_gap"]):
                rows = slice(k - k2, k + k2)
                b = ring[rows, :]
                l1, l2sq = b.sum(), (b ** 2).sum()
                dl1, dl2sq = dsnr[rows].sum(), (2 * snr[rows] * dsnr[rows]).sum()
                dP = (l1 / np.sqrt(l2sq)) * (dl1 / l1 + dl2sq / (2 * l2sq) + (n + 4) * u) / (np.sqrt(n) - 1)
                dq = (1 - p["alpha_p"]) * dP
                dQ[k - gap2 - 1:k] = dq + 3 * u * Q[k - gap2 - 1:k]
                dQ[k - 1:k + gap2] = dq + 3 * u * Q[k - 1:k + gap2]
            dQ[:p["P_len_k"] - 1] = dQ[p["P_len_k"] + dcb - 1]
        dQ[:dcb] = 0.0
    else:
        dQ = np.zeros(F)
    Qc = tr["Q_control"]
    dQc = (dQ.mean() + (F + 2) * u * Q.mean()) * p["Ar_up"] + 3 * u * abs(Qc)
    # lambda_dav
    a = p["alpha_d"]
    ld_old = (mm.T @ Vs if melconv else Ym) if l == 1 else g["lambda_dav"]
    dld = a * ld_old * 4 * u + (1 - a) * (beta * dDs + Ds * dbeta + 6 * u * Ds * beta) + (a * dYmd if l == 1 else 0.0)
    bnd["lambda_dav"] = dld
    ld = ga_ref["lambda_dav"]
    # gain
    if p["ENHANCE_METHOD"] == "Wiener":
        Gr = Xs / (Xs + Ds)
        with np.errstate(all="ignore"):
            dG = Gr * ((1 - Gr) * (dXs / Xs + dDs / Ds) + 3 * u)
    else:
        ae = p["alpha_eta"]
        num = ae * g["Xm_tilde"] + (1 - ae) * Xs * Q
        dnum = 4 * u * num + (1 - ae) * (Q * dXs + Xs * dQ)
        ldf = np.fmax(ld, flr)
        eta = num / ldf
        with np.errstate(all="ignore"):
            deta = np.where(num > 0, dnum / ldf + eta * (dld / ldf + 2 * u), dnum / ldf)  # absolute
        Gr = np.fmax(eta, 0.0031) / (np.fmax(eta, 0.0031) + 1.0)
        dG = deta / (1.0 + np.fmax(eta, 0.0031)) ** 2 + 3 * u * Gr
    if init:
        bnd["Xm_tilde"] = flr * (dV + 2 * u * Ym)
        dXt = bnd["Xm_tilde"]
        Gs = np.full(F, flr)
        dD = dV + u * Ym
    else:
        Gs = np.fmin(Gr, 1.0)
        bnd["Xm_tilde"] = Ym * dG + Gs * dV + 2 * u * Gs * Ym
        dXt = bnd["Xm_tilde"]
        dD = Ym * dG + (1 - Gs) * dV + 3 * u * Ym * (1 - Gs)
        dD[:dcb] = flr * (dV[:dcb] + 2 * u * Ym[:dcb])
    bnd["lambda_d_blk"] = dD
    # A itself under the bound the issue sets, tau_h + 4u (its dV share, tauA, only enters the fields derived from A)
    # (Mel mode: V of that step is no exact input -- the features are formed from the spectrum by k_obmel -- so their dV stays)
    bnd["Ad_blk"] = dA[Rx:Rx + Ra] if mel else A[Rx:Rx + Ra] * tau_step
    # trace (float in every mode)
    Ax_eff = flr if init else Ax
    dAx_eff = u * flr if init else dAx
    bnd["A_x_mag"] = dAx_eff + U * Ax_eff
    bnd["A_d_mag"] = dAd + U * Ad
    bnd["beta"] = dbeta + U * abs(beta)
    bnd["Q_control"] = dQc + U * abs(Qc)
    # synthesis
    def dsyn(M, dM, sq):
        m = np.array(M, np.float64)
        m[:p["DCbin_back"]] = 0.0
        z = np.sqrt(m)
        with np.errstate(all="ignore"):
            dz = np.where(z > 0, dM / (2 * np.where(z > 0, z, 1.0)), np.sqrt(dM)) + sq * eY + 3 * u * z
        dz[:p["DCbin_back"]] = 0.0
        half = N // 2
        tot = dz.sum() + dz[1:half].sum()
        z2 = np.sqrt((z ** 2).sum() + (z[1:half] ** 2).sum())
        return lambda s: p["overlapscale"] / N * np.abs(p["win_ISTFT"]) * (tot + C_FFT * L * u * np.sqrt(N) * z2) + 3 * u * np.abs(s)
    bnd["x_tilde_tail"] = dsyn(ga_ref["Xm_tilde"], dXt, np.sqrt(Gs))(fr_ref["x_tilde"])
    bnd["x_hat_tail"] = dsyn(Xs, dXs, np.sqrt(Xs / V))(fr_ref["x_hat"])
    bnd["d_hat_tail"] = dsyn(Ds, dDs, np.sqrt(Ds / V))(fr_ref["d_hat"])
    cc = class_cols(p, Rx, Rd)
    if cc is not None:
        bnd["class_tails"] = []
        for cols, s in zip(cc, fr_ref["class"]):
            Xc = W0[:, cols] @ A[cols]
            bnd["class_tails"].append(dsyn(Xc, W0[:, cols] @ dA[cols] + (r + 6) * u * Xc, np.sqrt(Xc / V))(s))
    # decisions: margins in units of the bound of the comparison's operands
    margins = {"lam_floor": lam_floor}
    if p["adapt_train_N"]:
        margins["trig"] = abs(Qc * Ad - Ax_eff) / (abs(Qc) * dAd + Ad * dQc + dAx_eff + 4 * u * abs(Qc * Ad))
        if tr["trig"]:
            rows = ga_ref["Ad_blk"].mean(axis=1)
            drows = dA[Rx:Rx + Ra] / ma + 2 * u * rows  # only the newest column carries an error (the mean is formed in double)
            margins["r_up"] = np.abs(Qc * rows - Ax_eff) / (abs(Qc) * drows + rows * dQc + dAx_eff + 4 * u * abs(Qc * rows))
    # (Mel mode: V = melmat * lambda_d_blk is an F-term chain on the device's own ring, k_obprep_mel: elementwise.py's rule for a
    # V that is no exact input, tau_W + 4 dV with dV = (F + 2) u)
    bnd["tau_w"] = lambda n_up: ((tau_w(Fs, max(1, n_up), beta_div, ma, "w") / U) + 4 + (4 * (F + 2) if mel else 0)) * u
    return bnd, margins


# ---- the comparator ------------------------------------------------------------------------------------------------------------

def field_regions(field, p, F, Ra):
    """Named index sets of a field's elements (the kernel paths of the module docstring)."""
    dcb, Pk = p["DCbin"], p["P_len_k"]
    if field in ("Xm_tilde", "lambda_dav", "r_blk", "lambda_d_blk"):
        reg = {"all": np.arange(F), "extra_row": np.array([F - 1]), "copied_bins": np.arange(dcb, max(dcb, Pk - 1)),
               "blk_bins": np.arange(max(dcb, Pk - 1), F)}
        if dcb:
            reg["dc_bins"] = np.arange(dcb)
        return reg
    if field == "Ad_blk":
        return {"all": np.arange(Ra), "last_activation": np.array([Ra - 1])}
    return None


def wadapt_regions(Fw, n_up, last_lane):
    """The updated columns (Fw x n_up, column-major) by the cooperative adaptation kernel's geometry: a workgroup holds 8 rows
    (kWaRB), the exchange sums the workgroups below and from ceil(nwg / 2) on in two thread groups, the last workgroup holds
    (Fw - 1) mod 8 + 1 rows, and column R_a - 1 of the solve's input (updated when its r_up is set: last_lane) is the last lane
    of the padded rank.  A set that is empty at a shape is skipped by the comparison and not counted."""
    idx = np.arange(Fw * n_up)
    wg = (idx % Fw) // 8
    nwg = (Fw + 7) // 8
    half = (nwg + 1) // 2
    return {"B_tmp.first_wg": idx[wg == 0], "B_tmp.last_wg": idx[wg == nwg - 1], "B_tmp.wg_low": idx[wg < half],
            "B_tmp.wg_high": idx[wg >= half], "B_tmp.col_Ra-1": idx[idx.size - Fw:] if last_lane else idx[:0]}


class Tally:
    """What a case's judged frames add up to: per field and region the worst error / bound and the squared relative errors."""

    def __init__(self):
        self.worst, self.sq, self.n = {}, {}, {}
        self.frames = self.left_out = self.triggered = self.solved = self.border_rows = self.rows = 0
        self.elem_out, self.elem_all = {}, {}
        self.fails = []

    def add(self, key, err, bound, ref, norm=None):
        """norm: the scale the RMS is relative to (a synthesis frame: its own RMS, since single samples cross zero)."""
        err, bound, ref = (np.atleast_1d(np.asarray(x, np.float64)) for x in (err, bound, ref))
        if norm is not None:
            ref = np.full(err.shape, float(norm))
        with np.errstate(all="ignore"):
            q = np.where(err > 0, err / bound, 0.0)
            relv = np.where(np.abs(ref) > 0, err / np.abs(ref), 0.0)
        self.worst[key] = max(self.worst.get(key, 0.0), float(q.max(initial=0.0)))
        self.sq[key] = self.sq.get(key, 0.0) + float((relv ** 2).sum())
        self.n[key] = self.n.get(key, 0) + int(relv.size)
        return q

    def caps_ok(self):
        """The issue's caps on what is left out: 10 % of the (frame, stream) pairs, 2 % of the elements of any field, 2 % of the
        r_up rows (a row on the reference's margin is judged on the device's own decision, and counted)."""
        return (self.left_out <= 0.1 * self.frames and self.border_rows <= 0.02 * max(1, self.rows)
                and all(n <= 0.02 * self.elem_all[f] for f, n in self.elem_out.items()))

    def rms(self, key):
        return float(np.sqrt(self.sq[key] / max(1, self.n[key])))

    def lines(self, other=None):
        out = []
        for key in sorted(self.worst):
            s = f"  {key:34s} worst/bound {self.worst[key]:9.3e}  rms {self.rms(key):9.3e}"
            if other is not None and key in other.sq:
                s += f"  emulation rms {other.rms(key):9.3e}"
            out.append(s)
        return out


def judge(dev_after, dev_trace, g, ref, bnd, margins, p, Bx, tally, what, u=U, pin_oracle=False):
    """Compare one frame: dev_after (fp64-cast state after the frame), dev_trace (its trace entry, or None) against ref =
    (g_after, frames, trace) of reference() under bnd.  Failures are appended to tally.fails as strings naming the field, the
    region and the element; the exact invariants are judged against g (the state before).  Returns False when the frame's
    decisions were borderline (its dependent fields left out)."""
    ga, fr, tr = ref
    F, Rx = Bx.shape
    Ra, ma, sz = p["R_a"], p["m_a"], p["framelength"]
    tally.frames += 1
    fails = tally.fails

    def cmp(field, dev, refv, bound, regs=None, frame_rms=False, skip=None):
        dev, refv = np.asarray(dev, np.float64), np.asarray(refv, np.float64)
        tally.elem_all[field] = tally.elem_all.get(field, 0) + dev.size
        if skip is not None and skip.any():
            tally.elem_out[field] = tally.elem_out.get(field, 0) + int(skip.sum())
            regs = {name: idx[~skip[idx]] for name, idx in (regs or {"all": np.arange(dev.size)}).items()}
        if not np.isfinite(dev).all():
            fails.append(f"{what}: {field}: non-finite at {np.argwhere(~np.isfinite(dev))[:3].ravel().tolist()}")
            return
        err = np.abs(dev - refv)
        for name, idx in (regs or {"all": np.arange(dev.size)}).items():
            if len(idx) == 0:
                continue
            q = tally.add(f"{field}.{name}", err[idx], np.broadcast_to(bound, err.shape)[idx], refv[idx],
                          norm=float(np.sqrt(np.mean(refv ** 2))) if frame_rms else None)
            if not (q <= 1.0).all():
                i = int(idx[int(np.argmax(q))])
                fails.append(f"{what}: field {field}, region {name}: element {i} is off by {err[i]:.3e} (device {dev[i]:.9g}, reference "
                             f"{refv[i]:.9g}), {float(q.max()):.3g} x its bound {float(np.broadcast_to(bound, err.shape)[i]):.3e}")

    # ---- decisions
    border_trig = ("trig" in margins and margins["trig"] < 1.0) or margins.get("lam_floor", False)
    dev_trig = int(dev_after["n_push"]) - int(g["n_push"])
    if dev_trace is not None:
        assert dev_trig == int(dev_trace["trig"]), (what, "n_push and the trace disagree")
    if border_trig:
        tally.left_out += 1
        if tr["solved"]:
            fails.append(f"{what}: a frame with `solved` is left out (trig margin {margins.get('trig', np.inf):.3g} bounds, Lam floor "
                         f"{margins.get('lam_floor')}): change the seed")
        return False
    if dev_trig != int(tr["trig"]):
        fails.append(f"{what}: decision trig: device {dev_trig}, reference {int(tr['trig'])} (margin {margins.get('trig'):.3g} bounds)")
        return True
    tally.triggered += int(tr["trig"])
    # r_up of :220: in the fp32 mode the trace holds the very floats the device compared (Q_control, the effective A_x_mag) and
    # the ring mean is a double sum of the state's own values, so the device's r_up is recomputed from its own state; a row may
    # differ from the reference's only where the reference's margin is inside its bound, and the dictionary is judged on the
    # device's rows (no frame is left out for an r_up comparison)
    r_up = ref_r_up(ga, tr, p) if tr["trig"] else np.zeros(Ra, bool)
    if tr["trig"] and dev_trace is not None and u == U:
        r_dev = float(dev_trace["Q_control"]) * dev_after["Ad_blk"].mean(axis=1) > float(dev_trace["A_x_mag"])
        diff = r_dev != r_up
        if (diff & (margins["r_up"] >= 1.0)).any():
            k = int(np.argmax(diff & (margins["r_up"] >= 1.0)))
            fails.append(f"{what}: decision r_up, row {k}: device {bool(r_dev[k])}, reference {bool(r_up[k])} (margin {margins['r_up'][k]:.3g} bounds)")
        tally.border_rows += int(diff.sum())
        tally.rows += Ra
        r_up = r_dev
    switch_due = bool(tr["trig"]) and int(g["update_switch"]) == int(np.floor(p["overlap_m_a"] * ma))
    n_up, solved = int(r_up.sum()), switch_due and bool(r_up.any())
    tally.solved += int(solved)
    if dev_trace is not None:
        want = dict(n_iter=tr["n_iter"], trig=tr["trig"], n_up=n_up, solved=solved, adapt_iters=tr["adapt_iters"] if solved == tr["solved"] else None)
        for key, w in want.items():
            if w is not None and int(dev_trace[key]) != int(w):
                fails.append(f"{what}: decision {key}: device {int(dev_trace[key])}, expected {int(w)} (reference {int(tr[key])})")
        init = int(g["l"]) <= p["init_N_len"]
        for key in ("A_x_mag", "A_d_mag", "beta", "Q_control"):
            refv = p["nonzerofloor"] if (key == "A_x_mag" and init) else tr[key]
            cmp("trace." + key, [dev_trace[key]], [refv], bnd[key])
    for key in ("n_push", "update_switch", "l"):
        if int(dev_after[key]) != int(ga[key]):
            fails.append(f"{what}: {key}: device {int(dev_after[key])}, reference {int(ga[key])}")
    # ---- per element
    near = bnd["near_floor"]
    wiener_near = near if p["ENHANCE_METHOD"] == "Wiener" else None  # (the Wiener gain divides by Xs and Xs + Ds)
    cmp("lambda_dav", dev_after["lambda_dav"], ga["lambda_dav"], bnd["lambda_dav"], field_regions("lambda_dav", p, F, Ra))
    cmp("Xm_tilde", dev_after["Xm_tilde"], ga["Xm_tilde"], bnd["Xm_tilde"], field_regions("Xm_tilde", p, F, Ra), skip=wiener_near)
    if p["blk_sparse"]:
        cmp("r_blk", dev_after["r_blk"][:, -1], ga["r_blk"][:, -1], bnd["r_blk"], field_regions("r_blk", p, F, Ra), skip=near)
        if not np.array_equal(dev_after["r_blk"][:, :-1], g["r_blk"][:, 1:]):
            fails.append(f"{what}: field ring r_blk: columns 1: of the old ring are not columns :-1 of the new one")
    for tail in ("x_tilde_tail", "x_hat_tail", "d_hat_tail"):
        if tail in dev_after:
            cmp(tail, dev_after[tail][-sz:], fr[tail[:-5]], bnd[tail], frame_rms=True)
            if not np.array_equal(dev_after[tail][:-sz], g[tail][sz:]):
                fails.append(f"{what}: field {tail}: the older frames have not shifted by framelength unchanged")
    if "class_tails" in dev_after:
        for ci, (s, b) in enumerate(zip(fr["class"], bnd["class_tails"])):
            cmp("class_tails", dev_after["class_tails"][ci][-sz:], s, b, {f"class{ci}": np.arange(sz)}, frame_rms=True)
        if not np.array_equal(dev_after["class_tails"][:, :-sz], g["class_tails"][:, sz:]):
            fails.append(f"{what}: field class_tails: the older frames have not shifted by framelength unchanged")
    for key in ("B_fix", "H0", "Ad_blk0"):
        if not np.array_equal(dev_after[key], g[key]):
            fails.append(f"{what}: {key} changed")
    for ring in ("lambda_d_blk", "Ad_blk"):
        if tr["trig"]:
            if not np.array_equal(dev_after[ring][:, :-1], g[ring][:, 1:]):
                fails.append(f"{what}: field ring {ring}: columns 1: of the old ring are not columns :-1 of the new one")
            cmp(ring, dev_after[ring][:, -1], ga[ring][:, -1], bnd[ring], field_regions(ring, p, F, Ra),
                skip=wiener_near if ring == "lambda_d_blk" else None)
        elif not np.array_equal(dev_after[ring], g[ring]):
            fails.append(f"{what}: field ring {ring}: changed on an untriggered frame")
    # ---- the dictionary (Mel mode: B_Mel_d on melmat * lambda_d_blk, its fix columns its own; B_DFT_d is never adapted, :224-230)
    mel = p.get("B_sep_mode", "DFT") == "Mel"
    key = "B_Mel_d" if mel else "B_DFT_d"
    if mel and not np.array_equal(dev_after["B_DFT_d"], g["B_DFT_d"]):
        fails.append(f"{what}: field B_DFT_d: changed in Mel mode")
    Bd0, Bd1 = g[key], dev_after[key]
    if not switch_due:
        if not np.array_equal(Bd1, Bd0):
            fails.append(f"{what}: field {key}: changed on a frame without a solve")
        return True
    n_rem = int((~r_up).sum())
    if not np.array_equal(Bd1[:, :n_rem], Bd0[:, :Ra][:, ~r_up]):
        fails.append(f"{what}: field {key}, region rem: columns :{n_rem} are not bit copies of the kept columns, in the reference's order")
    if not np.array_equal(Bd1[:, Ra:], (Bd0 if mel else g["B_fix"])[:, Ra:]):
        fails.append(f"{what}: field {key}, region fix: columns {Ra}: are not bit copies of {'the old B_Mel_d' if mel else 'B_fix'}")
    if r_up.any():
        beta_div = beta_of(p)
        W0 = Bd0[:, :Ra][:, r_up]
        wn = np.sqrt(np.sum(W0 ** 2, axis=0))
        Vad = np.asarray(p["_melmat"], np.float64) @ dev_after["lambda_d_blk"] if mel else dev_after["lambda_d_blk"]
        Wn, _ = ref_wstep(np.fmax(Vad, p["nonzerofloor"]), W0 / wn, dev_after["Ad_blk"][r_up] * wn[:, None], beta_div, exact_v=True)
        up = Bd1[:, n_rem:Ra]
        if pin_oracle and np.array_equal(r_up, ref_r_up(ga, tr, p)) and not np.allclose(Wn, ga[key][:, n_rem:Ra], rtol=1e-9, atol=0.0):
            fails.append(f"{what}: the W step from the rings is not the oracle's adaptation solve")
        Fw = Bd0.shape[0]
        regs = {"B_tmp": np.arange(up.size), "B_tmp.extra_row": np.arange(Fw - 1, up.size, Fw),
                "B_tmp.last_column": np.arange(up.size - Fw, up.size)}
        regs.update(wadapt_regions(Fw, n_up, bool(r_up[Ra - 1])))
        cmp(key, up.ravel(order="F"), Wn.ravel(order="F"), bnd["tau_w"](n_up) * Wn.ravel(order="F") + 4 * TINY[u], regs)
    return True


def ref_r_up(ga_ref, tr, p):
    """:220 from the reference's after-state and trace."""
    return tr["Q_control"] * ga_ref["Ad_blk"].mean(axis=1) > tr["A_x_mag"]  # (the trace holds flr on an init frame, :204)


# ---- the cases -----------------------------------------------------------------------------------------------------------------

GEO1 = (128, 100, 25, 16, 20, dict(P_len_k=12, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2, R_a=8, m_a=12, overlap_m_a=0.3))
GEO2 = (64, 64, 16, 8, 12, dict(R_a=6, m_a=12, overlap_m_a=0.2, Ar_up=2.0, P_len_k=8, P_len_l=4, init_N_len=4, DCbin=1, DCbin_back=1, delay=2,
                                 ENHANCE_METHOD="Wiener", cf="ed"))
GEO3 = (512, 400, 100, 60, 69, dict(R_a=33, m_a=40, overlap_m_a=0.05, P_len_k=30, P_len_l=6, init_N_len=4, DCbin=3, DCbin_back=3,
                                    cf="x", beta_div=1.5))
GEO4 = (1024, 640, 160, 72, 128, dict(R_a=64, m_a=64, overlap_m_a=0.05, cf="x", beta_div=0.5))
GEO5 = (1024, 640, 160, 72, 128, dict(R_a=80, m_a=80, overlap_m_a=0.05))
# (Ar_up = 0.8: with 1.0 every frame of the Mel run triggers; the first of 0.8, 0.6, ... that leaves untriggered frames too)
GEO7 = (256, 200, 50, 16, 20, dict(P_len_k=16, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2, R_a=8, m_a=12, overlap_m_a=0.3, Ar_up=0.8))
MEL_ORDER = 24
GEO6 = (1024, 640, 160, 100, 101, dict(R_a=40, m_a=48, overlap_m_a=0.05))
ONE_STEP = dict(max_iter=1, conv_eps=0.0)

# name -> (geometry, hops, precision, seed, class partition).  The seed rule: the first from 11 whose pure oracle run meets
# coverage_ok(); 11 itself does in every case, which tests/test_online_step_rules.py asserts (with the oracle's counts printed).
CASES = {
    "c1_fft128_kl": (GEO1, 40, "fp32", 11, None),
    "c2_fft64_wiener_ed": (GEO2, 40, "fp32", 11, None),
    "c3_fft512_r129_b15": (GEO3, 48, "fp32", 11, None),
    "c4_fft1024_r200_ra64_b05": (GEO4, 72, "fp32", 11, None),
    "c5_fft1024_r200_ra80_kl": (GEO5, 88, "fp32", 11, None),
    # class outputs: the partition of tests/test_gpu_online_batch_state.py::PARTITION, scaled to the ranks
    "c8_fft128_kl_classes": (GEO1, 40, "fp32", 11, dict(EVENT_NUM=2, EVENT_RANK=[1, 9], NOISE_NUM=2, NOISE_RANK=[1, 11])),
    "c8_fft512_r129_b15_classes": (GEO3, 48, "fp32", 11, dict(EVENT_NUM=2, EVENT_RANK=[1, 31], NOISE_NUM=2, NOISE_RANK=[1, 36])),
    # Mel mode (fft 256, F_order 24): the dictionaries as tests/test_online_batch_mel.py stores them (_mel_dict), MelConv 1 and 0
    "c7_fft256_mel24_conv1": (GEO7, 40, "fp32", 11, ("mel", 1)),
    "c7_fft256_mel24_conv0": (GEO7, 40, "fp32", 11, ("mel", 0)),
    "c9_fft128_kl_fp64": (GEO1, 40, "fp64", 11, None),
    # settings and an event dictionary per stream, as tests/test_gpu_online_batch_state.py::_small(..., streams=True)
    "c9_fft128_kl_fp64_streams": (GEO1, 40, "fp64", 11, "streams"),
    "c9_fft1024_r200_ra64_b05_fp64": (GEO4, 72, "fp64", 11, None),
}


# ---- the single-stream separator (OnlineSeparator): the smallest shapes at which each of ITS paths can still go wrong -------------
# s1: k_wadapt at the shipped row count: F = 513 -> 65 workgroups of 8 rows, both thread groups of cross_sum (33 + 32), a last
#     workgroup of one row, R_a at kWaRP = 64, operand images (m_a = 64).  s2: m_a = 21 is no multiple of 4 (no operand images),
#     F = 257 -> 33 workgroups (17 + 16), a last workgroup of one row.  s3: F = 1025 is past k_hsolve_frame (k_hsolve_small) and
#     129 workgroups are past k_wadapt (the W-only plan loop on T = m_a); the rest as tests/test_online.py::GEOMETRIES' fft 2048
#     row.  s4: r = 161 at F = 1025 is the smallest rank whose H-only plan has small_ok == false (rp = 192: the persistent kernel's
#     (32 (rp + 4 + Fq + 4) + rp) 4 + 8192 B = 166 656 B > 160 KiB; r = 160 needs 162 432 B and fits) -- tests/
#     test_online_step_rules.py asserts both from the plan's describe text.  s5: c1's geometry, the semi-supervised frame solve
#     (the plan hsemi): at one iteration H is updated before W, so A is the supervised step's and the solve's private W must
#     leave no trace.  s6: a fixed dictionary (adapt_train_N = 0): om_solve_run, all frames of a call in one launch_small.
GEO_S1 = GEO4[:5] + (dict(R_a=64, m_a=64, overlap_m_a=0.05),)
GEO_S2 = (512, 400, 100, 24, 40, dict(R_a=16, m_a=21, overlap_m_a=0.1, P_len_k=30, P_len_l=6, init_N_len=4, DCbin=3, DCbin_back=3))
# (the fft 2048 row of GEOMETRIES has Ar_up = 2 and overlap_m_a = 0.05: every frame triggers and floor(0.05 * 30) = 1 keeps
# update_switch at 1, which no seed changes; Ar_up = 1 -- the shipped value, the first of 1, 0.8, ... that leaves untriggered
# frames -- and overlap_m_a = 0.1 (a solve every third push) are the smallest changes that meet coverage_ok)
_FFT2048 = dict(R_a=24, m_a=30, overlap_m_a=0.1, Ar_up=1.0, P_len_k=100, P_len_l=6, init_N_len=4, DCbin=5, DCbin_back=5)
GEO_S3 = (2048, 1600, 400, 40, 40, _FFT2048)
GEO_S4 = (2048, 1600, 400, 61, 100, _FFT2048)


def _sc(geo, hops, precision="fp32", seed=11, over=None, env=None, base=None, fixed=False):
    return dict(geo=geo, hops=hops, precision=precision, seed=seed, over=over or {}, env=env or {}, base=base, fixed=fixed)


_NO_WADAPT = dict(SNMF_NO_WADAPT="1")  # (read when the separator is created: the W-only plan loop instead of k_wadapt)
# name -> geometry, hops, precision, seed (the rule of CASES), overrides on the one-step settings, environment of the device
# run, base (the case whose CPU trajectory this one shares: the environment changes the device's path and nothing else), fixed
# (no adaptation: the coverage rule is frames on both sides of init_N_len and of P_len_l).
SINGLE_CASES = {
    "s1_fft1024_kl_ra64_wadapt": _sc(GEO_S1, 72),
    "s1_fft1024_kl_ra64_wadapt_fp64": _sc(GEO_S1, 72, "fp64"),
    "s2_fft512_ma21_wadapt": _sc(GEO_S2, 40),
    "s1_fft1024_kl_ra64_plan": _sc(GEO_S1, 72, env=_NO_WADAPT, base="s1_fft1024_kl_ra64_wadapt"),
    "s2_fft512_ma21_plan": _sc(GEO_S2, 40, env=_NO_WADAPT, base="s2_fft512_ma21_wadapt"),
    "c1_fft128_kl_plan": _sc(GEO1, 40, env=_NO_WADAPT, base="c1_fft128_kl"),
    "s3_fft2048_small_plan": _sc(GEO_S3, 44),
    "s4_fft2048_r161_planloop": _sc(GEO_S4, 44),
    "s5_fft128_semi_N": _sc(GEO1, 40, over=dict(basis_update_N=1)),
    "s5_fft128_semi_E_fixed": _sc(GEO1, 40, over=dict(basis_update_E=1, adapt_train_N=0), fixed=True),
    # two iterations: the second H step sees the W the first iteration's W update left (the one-step cases never do); judged
    # under stop_bounds(..., n_iter=2).  Only the fixed-dictionary configuration: with basis_update_N the adaptation solve would
    # run two iterations too, and the rule has no bound for a two-step dictionary (amplification() measures no dictionary field)
    "s5_fft128_semi_E_fixed_2it": _sc(GEO1, 40, over=dict(basis_update_E=1, adapt_train_N=0, max_iter=2), fixed=True),
    "s6_fft128_fixed": _sc(GEO1, 40, over=dict(adapt_train_N=0), fixed=True),
    "s6_fft2048_fixed": _sc(GEO_S3, 44, over=dict(adapt_train_N=0), fixed=True),
}
# the cases of CASES the single-stream separator is judged on too, one separator per stream (the per-stream-settings case has
# no single-stream form)
SINGLE_REUSED = [n for n in CASES if n != "c9_fft128_kl_fp64_streams"]


def single_case(name):
    """(environment of the device run, the case whose inputs and CPU trajectory it has, fixed dictionary?)."""
    if name in CASES:
        return {}, name, False
    c = SINGLE_CASES[name]
    return c["env"], c["base"] or name, c["fixed"]


def case_inputs(name, seed=None):
    """(p, pcms, Bx, Bds, H0s, Ads, precision, settings) of a case: three streams as tests/test_online_batch.py::_geo_streams builds
    them (the second one shorter), the one-step settings.  A case with class outputs has its partition in p (EVENT_RANK /
    NOISE_RANK).  settings: None, or per stream the overrides on p, with Bx then a list of three event dictionaries
    (stream_view gives stream k's own p and Bx)."""
    from test_online_batch import _geo_streams, _settings
    over = {}
    if name in CASES:
        geo, hops, precision, seed0, classes = CASES[name]
    else:  # a single-stream case: the same streams, its own overrides on the one-step settings
        c = SINGLE_CASES[name]
        geo, hops, precision, seed0, classes, over = c["geo"], c["hops"], c["precision"], c["seed"], None, c.get("over", {})
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(geo, hops, seed=seed0 if seed is None else seed)
    settings, mel = None, None
    if isinstance(classes, tuple):
        mel, classes = dict(B_sep_mode="Mel", MelConv=classes[1], F_order=MEL_ORDER), None
    if classes == "streams":
        rs = np.random.RandomState(5)
        Bx = [Bx, Bx * (1.0 + 0.05 * rs.random_sample(Bx.shape)), Bx]
        settings, classes = [{}, dict(alpha_d=0.65), dict(sparsity=4)], None
    p = _settings(dict(p, **dict(ONE_STEP, **(classes or {}), **(mel or {}), **over)))
    if mel:  # the mode's configuration: the float image of melmat the device holds, the shared B_Mel_x, every stream's B_Mel_d
        from se_snmf_nat_amd.frontend import mel_matrix
        from test_online_batch_mel import _mel_dict, _melmat
        mm = _melmat(p, MEL_ORDER)
        p["_melmat"] = np.asarray(mel_matrix(p["fs"], MEL_ORDER, p["fftlength"], 1.0, p["fs"] / 2).T, np.float32).astype(np.float64)
        p["_B_Mel_x"], p["_B_Mel_ds"] = _mel_dict(mm, Bx), [_mel_dict(mm, B) for B in Bds]
    hop = p["frameshift"]
    pcms = [x[:(len(x) // hop) * hop] for x in pcms]  # whole hops: nothing pending between the calls
    return p, pcms, Bx, Bds, H0s, Ads, precision, settings


def stream_view(p, Bx, settings, k):
    """Stream k's own settings and event dictionary."""
    return (dict(p, **settings[k]) if settings else p), (Bx[k] if isinstance(Bx, list) else Bx)


def coverage(records, p):
    """What a run's judged frames reach, per stream list of (l, trace, n_push_after, update_switch_after) records."""
    ls = [l for rec in records for (l, *_r) in rec]
    out = dict(
        init_both=min(ls) <= p["init_N_len"] < max(ls),
        pl_both=min(ls) <= p["P_len_l"] < max(ls),
        triggered=min(sum(int(t["trig"]) for _, t, _, _ in rec) for rec in records),
        untriggered=sum(int(not t["trig"]) for rec in records for _, t, _, _ in rec),
        wrapped=max(n for rec in records for _, _, n, _ in rec) > p["m_a"],
        solved=sum(int(t["solved"]) for rec in records for _, t, _, _ in rec),
        switch_gt1=any(s > 1 for rec in records for _, _, _, s in rec),
        partial_up=any(t["solved"] and 0 < t["n_up"] < p["R_a"] for rec in records for _, t, _, _ in rec),
    )
    return out


def coverage_ok(cov):
    return (cov["init_both"] and cov["pl_both"] and cov["triggered"] >= 5 and cov["untriggered"] >= 1 and cov["wrapped"]
            and cov["solved"] >= 2 and cov["switch_gt1"] and cov["partial_up"])


def initial_state(p, Bx, Bd, H0, Ad0, dt=np.float32, B_Mel_d=None):
    """init_buff as the device holds it at frame 1 (the arrays the mode rounds to dt; the dictionary masters stay fp64)."""
    F = Bx.shape[0]
    sz, hop = p["framelength"], p["frameshift"]
    ntail = max(1, (sz + hop - 1) // hop - 1) * sz
    r = lambda a: np.asarray(np.asarray(a, dt), np.float64)  # noqa: E731
    st = dict(Xm_tilde=np.zeros(F), lambda_dav=np.zeros(F), r_blk=np.zeros((F, p["P_len_l"])), lambda_d_blk=np.zeros((F, p["m_a"])),
                Ad_blk=r(Ad0), n_push=0, update_switch=1, B_DFT_d=np.array(Bd, np.float64), B_fix=np.array(Bd, np.float64),
                H0=r(H0), Ad_blk0=r(Ad0), l=1, y_hist=np.zeros(sz - hop), x_tilde_tail=np.zeros(ntail))
    if B_Mel_d is not None:
        st["B_Mel_d"] = np.array(B_Mel_d, np.float64)
    cc = class_cols(p, Bx.shape[1], np.shape(Bd)[1])
    if cc is not None:
        st.update(x_hat_tail=np.zeros(ntail), d_hat_tail=np.zeros(ntail), class_tails=np.zeros((len(cc), ntail)))
    return st


def advance(g, ga, frames, y, p, dt=np.float32):
    """The state before the next frame from a step's results, rounded as the mode stores it."""
    r = lambda a: np.asarray(np.asarray(a, dt), np.float64)  # noqa: E731
    sz, hop = p["framelength"], p["frameshift"]
    gn = dict(g)
    for k in ("Xm_tilde", "lambda_dav", "r_blk", "lambda_d_blk", "Ad_blk"):
        gn[k] = r(ga[k])
    gn.update(n_push=ga["n_push"], update_switch=ga["update_switch"], l=ga["l"], B_DFT_d=ga["B_DFT_d"], y_hist=y[hop:].copy())
    if "B_Mel_d" in ga:
        gn["B_Mel_d"] = ga["B_Mel_d"]
    tails = after_state(g, {}, frames, sz)
    for k in ("x_tilde_tail", "x_hat_tail", "d_hat_tail", "class_tails"):
        if k in g:
            gn[k] = r(tails[k])
    return gn


# ---- judging a run: what tests/test_gpu_online_step.py (the batch) and tests/test_gpu_online_single_step.py share ------------------

def case_bounds(g, y, p, Bx, ref, u):
    """bounds() of a frame; a case with max_iter > 1 (the semi-supervised solve's W update) is judged under the project's rule
    for a k-iteration solve, stop_bounds: 4 n_iter tau max(1, amp_e) with the reference's own amplification."""
    bnd, margins = bounds(g, y, p, Bx, *ref, u=u)
    if int(p["max_iter"]) > 1:
        bnd = stop_bounds(bnd, amplification(g, y, p, Bx, ref)[0], n_iter=int(p["max_iter"]))
    return bnd, margins


def judge_run(name, views, precision, steps, fixed=False):
    """Judge every (frame, stream) pair of a run and assert the whole verdict.  views: per stream (p, Bx); steps: per stream the
    list of (state before, frame buffer, state after, trace entry), the states fp64-cast (state64).  Each pair is judged alone
    against sep_frame from the device's own before-state under the derived bounds, with both float32 emulations from the same
    state as the yardstick of the RMS check; one line per field and region is printed.  fixed: a run without adaptation, whose
    coverage rule is frames on both sides of init_N_len and of P_len_l.  Returns the device's Tally."""
    dt, u = (np.float32, U) if precision == "fp32" else (np.float64, U64)
    dev, emu = Tally(), (Tally(), Tally())
    records = []
    for k, ((p, Bx), sk) in enumerate(zip(views, steps)):
        rec = []
        for g, y, after, trace in sk:
            ref = reference(g, y, p, Bx)
            bnd, margins = case_bounds(g, y, p, Bx, ref, u)
            what = f"{name} stream {k} frame {g['l']}"
            judge(after, trace, g, ref, bnd, margins, p, Bx, dev, what, u=u)
            for rev, t in zip((False, True), emu):  # the yardstick of the RMS check, from the same state
                ga, fr, tr = frame_step(g, y, g["l"], p, g["H0"], Bx, dt=dt, rev=rev, seq=True)
                e = after_state(g, ga, fr, p["framelength"])
                judge(e, tr, g, ref, bnd, margins, p, Bx, t, what + " (emulation)", u=u)
            rec.append((g["l"], ref[2], after["n_push"], after["update_switch"]))
        records.append(rec)
    cov = coverage(records, views[0][0])
    print(f"\n{name}: {dev.frames} (frame, stream) pairs, triggered {dev.triggered}, solved {dev.solved}, left out {dev.left_out} "
          f"({100.0 * dev.left_out / dev.frames:.1f} %), r_up rows on the reference's margin {dev.border_rows} of {dev.rows}, elements "
          f"left out for a floor {dev.elem_out}; {cov}")
    rms_bad = []
    for key in sorted(dev.worst):
        yard = max(emu[0].rms(key) if key in emu[0].sq else 0.0, emu[1].rms(key) if key in emu[1].sq else 0.0, u / np.sqrt(3.0))
        limit = RMS_FACTOR * yard
        print(f"  {key:34s} worst/bound {dev.worst[key]:9.3e}  device rms {dev.rms(key):9.3e}  emulation rms {yard:9.3e}  ratio {dev.rms(key) / yard:6.2f}")
        if key.startswith("trace.") and precision == "fp64":
            continue  # (the trace is float in every mode: in the fp64 mode its RMS is that conversion's)
        if not dev.rms(key) <= limit:
            rms_bad.append(f"{key}: device rms {dev.rms(key):.3e} > {RMS_FACTOR} x emulation rms {yard:.3e}")
    assert not dev.fails, f"{len(dev.fails)} failures:\n" + "\n".join(dev.fails[:12])
    assert not emu[0].fails and not emu[1].fails, "\n".join((emu[0].fails + emu[1].fails)[:6])
    assert not rms_bad, "\n".join(rms_bad)
    assert (cov["init_both"] and cov["pl_both"]) if fixed else coverage_ok(cov), cov
    assert dev.caps_ok(), (dev.left_out, dev.border_rows, dev.elem_out)
    return dev


# ---- the single-stream driver: one separator per stream, one hop per process call, a get_state around every hop -------------------

class SimSeparator:
    """The emulation behind OnlineSeparator's calls (process / get_state / trace / close): frame_step over the mode's number type
    with the state rounded as the mode stores it.  The rules test runs the driver on it without a GPU ("a simulated device"),
    with a planted error where one is asked for."""

    def __init__(self, p, Bx, Bd, H0, Ad0, precision="fp32", rev=False, plant=None, B_Mel_d=None):
        self.p, self.Bx, self.rev, self.plant = p, Bx, rev, plant
        self.dt = np.float32 if precision == "fp32" else np.float64
        self.g = initial_state(p, Bx, Bd, H0, Ad0, self.dt, B_Mel_d)
        self._trace = []

    def get_state(self):
        return dict(self.g, pending=np.zeros(0))

    def process(self, pcm):
        hop = self.p["frameshift"]
        pcm = np.asarray(pcm, np.float64)
        assert pcm.size % hop == 0
        for i in range(pcm.size // hop):
            g = self.g
            y = frame_buffer(g, pcm[i * hop:(i + 1) * hop])
            ga, fr, tr = frame_step(g, y, g["l"], self.p, g["H0"], self.Bx, dt=self.dt, rev=self.rev, plant=self.plant, seq=True)
            self._trace.append({k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in tr.items()
                                if k in ("n_iter", "trig", "n_up", "solved", "adapt_iters", "beta", "A_x_mag", "A_d_mag", "Q_control")})
            self.g = advance(g, ga, fr, y, self.p, self.dt)

    def trace(self):
        return list(self._trace)

    def close(self):
        pass


def device_separator(ctx):
    """make(k, p, Bx, Bd, H0, Ad0, precision, class_outputs, mel) for run_single: the library's OnlineSeparator on ctx."""
    def make(k, p, Bx, Bd, H0, Ad0, precision, cls, mel):
        from se_snmf_nat_amd.online import OnlineSeparator
        return OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, precision=precision, class_outputs=cls, **mel)
    return make


def sim_separator(rev=False, plant=None):
    def make(k, p, Bx, Bd, H0, Ad0, precision, cls, mel):
        return SimSeparator(p, Bx, Bd, H0, Ad0, precision, rev, plant, mel.get("B_Mel_d"))
    return make


def run_single(make, name, streams=(0, 1, 2), hops_per_call=1, keep_outputs=False):
    """A case on single-stream separators, one per stream: per stream the list of (state before, frame buffer, state after,
    trace entry) for every frame when hops_per_call is 1 -- the after-state of frame l is the before-state of frame l + 1.
    With more hops per call (the fixed-dictionary path runs a whole call's frames in one launch) and keep_outputs: per stream
    (the states after every call, what the calls returned, the trace) instead.  Returns (views, precision, steps)."""
    _, base, _ = single_case(name)
    p0, pcms, Bx0, Bds, H0s, Ads, precision, settings = case_inputs(base)
    assert settings is None
    hop = p0["frameshift"]
    views, out, ns = [], [], []
    for k in streams:
        p, Bx = stream_view(p0, Bx0, settings, k)
        cls = class_cols(p, Bx.shape[1], Bds[k].shape[1]) is not None
        mel = dict(B_Mel_x=p["_B_Mel_x"], B_Mel_d=p["_B_Mel_ds"][k]) if "_melmat" in p else {}
        sep = make(k, p, Bx, Bds[k], H0s[k], Ads[k], precision, cls, mel)
        n = len(pcms[k]) // hop
        before = state64(sep.get_state())
        assert ("class_tails" in before) == cls and ("x_hat_tail" in before) == cls
        steps, states, outs = [], [], []
        for i in range(0, n, hops_per_call):
            feed = pcms[k][i * hop:min(n, i + hops_per_call) * hop]
            o = sep.process(feed)
            after = state64(sep.get_state())
            assert before["pending"].size == 0 and before["l"] == i + 1
            if hops_per_call == 1:
                steps.append((before, frame_buffer(before, feed), after))
            states.append(after)
            outs.append(o)
            before = after
        trace = sep.trace()
        sep.close()
        assert len(trace) == n
        ns.append(n)
        views.append((p, Bx))
        out.append((states, outs, trace) if keep_outputs else [s + (trace[i],) for i, s in enumerate(steps)])
    assert len(set(ns)) > 1 or len(streams) == 1  # the streams differ in length
    return views, precision, out


# ---- the stop-armed cases (shipped max_iter = 100, conv_eps = 1e-3) ----------------------------------------------------------------
#
# A k-iteration solve has no derived bound.  Per judged frame and element the bound is 4 n_iter tau max(1, amp_e): tau the one-step
# bound of bounds(), amp_e the reference's own amplification -- the largest relative change of element e over AMP_DRAWS seeded
# draws in which H0 and the dictionary images are multiplied by 1 + AMP_EPS N(0, 1), divided by AMP_EPS (the linear regime of
# profiles/online_f64_sensitivity.md).  Every iteration injects at most tau per element, and the reference's response to an
# injection at the start bounds, to first order, the carry of a later one; 4 is the project's usual margin.  A frame is
# BORDERLINE, and left out, where the reference's own stop decision has a small margin: a relative cost change within
# BORDER_BAND of conv_eps at an iteration of the frame solve or of the adaptation solve (src/sparse_nmf.m:273-275 compares every
# iterate from the second on, so every iterate counts), or a draw in which a decision differs (the regime is not linear there).

AMP_EPS, AMP_DRAWS, BORDER_BAND = 1e-9, 8, 0.05

# name -> what the pure oracle run reaches: (frame, stream) pairs, pairs whose frame solve / adaptation solve / either is
# borderline, frames with `solved`, and those of them that are borderline.  The counts are asserted by
# tests/test_online_step_rules.py: they are why these cases cannot be judged under the issue's cap (10 % of the pairs, no frame
# with `solved`) and the issue's 5 % rule at once.
STOP_CASES = {
    "c10_golden_shipped": dict(pairs=80, border_frame=65, border_adapt=9, border=65, solved=70, solved_border=55),
    "c11_fft128_kl_shipped": dict(pairs=110, border_frame=66, border_adapt=3, border=67, solved=35, solved_border=25),
}


def stop_case_inputs(name):
    """(p, pcms, Bx, Bds, H0s, Ads): case 10 = the shipped settings on the golden dictionaries (tests/test_online_batch_f64.py::
    _streams, 30 / 23 / 27 hops), case 11 = case 1 with the shipped iteration settings."""
    from oracle.online_oracle import default_params
    from test_online_batch import _geo_streams, _settings
    if name == "c10_golden_shipped":
        from test_online_batch_f64 import _streams
        pcms, Bx, Bds, H0s, Ads = _streams([30 * 160, 23 * 160, 27 * 160])
        return _settings(default_params()), pcms, Bx, Bds, H0s, Ads
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(GEO1, 40)
    p = _settings(p)
    hop = p["frameshift"]
    return p, [x[:(len(x) // hop) * hop] for x in pcms], Bx, Bds, H0s, Ads


def conv_borderline(cost, conv_eps, band=BORDER_BAND):
    """Whether a relative cost change of the history (oracle/sparse_nmf_oracle.py:250-253) is within band of conv_eps."""
    c = np.asarray(cost, np.float64)
    if c.size < 2 or conv_eps <= 0:
        return False
    e = np.abs(np.diff(c)) / c[:-1]
    return bool(np.any(np.abs(e - conv_eps) <= band * conv_eps))


def _solve_settings(p):
    q = dict(cf=p["cf"], sparsity=p["sparsity"], max_iter=p["max_iter"], conv_eps=p["conv_eps"], cost_check=p["cost_check"])
    if "beta_div" in p:
        q["beta"] = p["beta_div"]
    return q


def frame_cost_history(g, y, p, Bx):
    """The cost history of the frame solve of sep_frame (:158-167) from the state g."""
    from oracle.sparse_nmf_oracle import sparse_nmf
    Ym, _ = frame_stft(y, p)
    r = Bx.shape[1] + g["B_DFT_d"].shape[1]
    q = dict(_solve_settings(p), init_w=np.concatenate([np.asarray(Bx, np.float64), g["B_DFT_d"]], axis=1),
             init_h=np.asarray(g["H0"], np.float64).reshape(-1, 1), w_update_ind=np.zeros(r, bool), h_update_ind=np.ones(r, bool))
    return sparse_nmf(Ym[:, None], q)[2]["cost"]


def adapt_cost_history(g, ga_ref, tr, p):
    """The cost history of the adaptation solve of sep_frame (:224-239) on the reference's rings after the frame; None without one."""
    from oracle.sparse_nmf_oracle import sparse_nmf
    if not tr["solved"]:
        return None
    r_up = ref_r_up(ga_ref, tr, p)
    Ra = p["R_a"]
    q = dict(_solve_settings(p), init_w=g["B_DFT_d"][:, :Ra][:, r_up], init_h=ga_ref["Ad_blk"][r_up],
             w_update_ind=np.ones(int(r_up.sum()), bool), h_update_ind=np.zeros(int(r_up.sum()), bool))
    return sparse_nmf(ga_ref["lambda_d_blk"], q)[2]["cost"]


def _judged_values(ref):
    ga, fr, tr = ref
    v = dict(lambda_dav=ga["lambda_dav"], Xm_tilde=ga["Xm_tilde"], r_blk=ga["r_blk"][:, -1], lambda_d_blk=ga["lambda_d_blk"][:, -1],
             Ad_blk=ga["Ad_blk"][:, -1], x_tilde_tail=fr["x_tilde"], x_hat_tail=fr["x_hat"], d_hat_tail=fr["d_hat"])
    v.update({k: np.array([tr[k]], np.float64) for k in ("A_x_mag", "A_d_mag", "beta", "Q_control")})
    return {k: np.asarray(a, np.float64) for k, a in v.items()}


def _decisions(tr):
    return tuple(int(tr[k]) for k in ("n_iter", "trig", "n_up", "solved", "adapt_iters"))


def amplification(g, y, p, Bx, ref, seed=1000):
    """amp_e per judged field (module comment above) -> (amp, linear): linear is False where a draw's decisions differ."""
    base, dec = _judged_values(ref), _decisions(ref[2])
    amp, linear = {k: np.zeros(a.shape) for k, a in base.items()}, True
    for d in range(AMP_DRAWS):
        rs = np.random.RandomState(seed + d)
        pert = lambda a: np.asarray(a, np.float64) * (1.0 + AMP_EPS * rs.standard_normal(np.shape(a)))  # noqa: E731
        r2 = reference(dict(g, H0=pert(g["H0"]), B_DFT_d=pert(g["B_DFT_d"])), y, p, pert(Bx))
        if _decisions(r2[2]) != dec:
            linear = False
            continue
        for k, a in _judged_values(r2).items():
            with np.errstate(all="ignore"):
                amp[k] = np.maximum(amp[k], np.where(np.abs(base[k]) > 0, np.abs(a - base[k]) / (AMP_EPS * np.abs(base[k])), 0.0))
    return amp, linear


def stop_bounds(bnd, amp, n_iter):
    """4 n_iter tau max(1, amp_e) for every field of bounds() that amplification() measures."""
    out = dict(bnd)
    for k, a in amp.items():
        if k in bnd:
            out[k] = 4.0 * n_iter * np.asarray(bnd[k], np.float64) * np.maximum(1.0, a)
    return out


def stop_armed_oracle_run(name, with_amp=True):
    """The pure oracle run of a stop-armed case: per (frame, stream) pair a dict(l, n_iter, adapt_iters, solved, border_frame,
    border_adapt, linear, amp_max, amp_median) -- amp only on the pairs that are not borderline (the ones that would be judged)."""
    p, pcms, Bx, Bds, H0s, Ads = stop_case_inputs(name)
    hop, out = p["frameshift"], []
    for k in range(3):
        g = initial_state(p, Bx, Bds[k], H0s[k], Ads[k], np.float64)
        for i in range(len(pcms[k]) // hop):
            y = frame_buffer(g, pcms[k][i * hop:(i + 1) * hop])
            ref = reference(g, y, p, Bx)
            tr = ref[2]
            rec = dict(stream=k, l=g["l"], n_iter=tr["n_iter"], adapt_iters=tr["adapt_iters"], solved=bool(tr["solved"]),
                       border_frame=conv_borderline(frame_cost_history(g, y, p, Bx), p["conv_eps"]),
                       border_adapt=conv_borderline(adapt_cost_history(g, ref[0], tr, p), p["conv_eps"]) if tr["solved"] else False,
                       linear=True, amp_max=None, amp_median=None)
            if with_amp and not (rec["border_frame"] or rec["border_adapt"]):
                amp, rec["linear"] = amplification(g, y, p, Bx, ref)
                allv = np.concatenate([a.ravel() for a in amp.values()])
                rec["amp_max"], rec["amp_median"] = float(allv.max()), float(np.median(allv))
                bnd, _ = bounds(g, y, p, Bx, *ref, u=U)
                rec["bound_ok"] = all(np.all(np.isfinite(v)) for kk, v in stop_bounds(bnd, amp, tr["n_iter"]).items() if kk in amp)
            out.append(rec)
            g = advance(g, ref[0], ref[1], y, p, np.float64)
    return out
