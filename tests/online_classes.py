"""Per-class reference of the online separation loop (a helper of tests/test_online_classes.py, not a test).

    [x_hat_i, d_hat_i, x_tilde, g] = bnmf_sep_event_RT_IS16(y, l, g, p)      src/bnmf_sep_event_RT_IS16.m:1

Built only from the oracle's own functions (oracle/online_oracle.py: init_buff, sep_frame, frame_stft, synth_ifft_buff),
driven in the loop of its ntf_sep_event_rt (src/NTF_sep_event_RT.m:54-135).  Before each sep_frame call the dictionary
the frame solve will see is snapshotted (g["B_DFT_d"]; MelConv = 1: g["B_Mel_d"]) -- sep_frame replaces it at :318 / :336
-- and after the call the class spectra are formed from trace["A"]:

    event class i   columns EVENT_RANK(i) .. EVENT_RANK(i+1)-1 of B_x, the last one up to R_x            (:158-163)
    noise class i   columns NOISE_RANK(i) .. NOISE_RANK(i+1)-1 of B_d, the last one up to R_d            (:180-185)
    spectrum        B_DFT(:, R_i) * A(R_i);  'Mel' with MelConv = 1: melmat' * (B_Mel(:, R_i) * A(R_i))  (:165-171, :187-195)
    signal          synth_ifft_buff(spectrum, Yp, ...) * overlapscale                                    (:356-361)

overlap-added per class as the oracle overlap-adds x_hat / d_hat (src/NTF_sep_event_RT.m:112-126, frames l > delay).
"""
import numpy as np

from oracle.online_oracle import frame_stft, init_buff, sep_frame, synth_ifft_buff


def class_ranges(ranks, R):
    """1-based class starts -> [(lo, hi)) 0-based column ranges, the last class up to R."""
    rk = [int(v) for v in ranks]
    return [(rk[i] - 1, rk[i + 1] - 1 if i + 1 < len(rk) else R) for i in range(len(rk))]


def class_reference(pcm, B_DFT_x, B_DFT_d, p, H0, Ad_blk0, event_rank=(1,), noise_rank=(1,), mel=None):
    """The loop of oracle.online_oracle.ntf_sep_event_rt with per-class outputs.  Returns a dict: x_tilde_f, x_hat, d_hat
    [n], x_hat_i [E, n], d_hat_i [N, n], trace (the per-frame dicts of sep_frame) and basis (the final B_DFT_d; Mel: B_Mel_d)."""
    pcm = np.asarray(pcm, dtype=np.float64).reshape(-1)
    sz, hop = p["framelength"], p["frameshift"]
    g = init_buff(B_DFT_x, B_DFT_d, p, Ad_blk0, mel)
    R_x, R_d = g["B_DFT_x"].shape[1], g["B_DFT_d"].shape[1]
    is_mel = p.get("B_sep_mode", "DFT") == "Mel"
    melconv = is_mel and bool(p.get("MelConv", 1))
    ev, nz = class_ranges(event_rank, R_x), class_ranges(noise_rank, R_d)
    n_cls = len(ev) + len(nz)
    y = np.zeros(sz)
    bufs = np.zeros((3 + n_cls, sz))  # x_tilde, x_hat, d_hat, then the classes
    outs = [[] for _ in range(3 + n_cls)]
    traces = []
    pos, l, cnt_residue = 0, 1, 0
    while True:
        have = pos + hop <= len(pcm)
        if cnt_residue > p["delay"]:
            break
        if not have:
            pos = len(pcm)
            cnt_residue += 1
            y = np.zeros(sz)
        else:
            y[:sz - hop] = y[hop:].copy()
            y[sz - hop:] = pcm[pos:pos + hop]
            pos += hop
        # the dictionaries as the frame solve sees them (:141), before this frame's adaptation (:318 / :336)
        Bx = g["B_Mel_x"] if melconv else g["B_DFT_x"]
        Bd = (g["B_Mel_d"] if melconv else g["B_DFT_d"]).copy()
        _, Yp = frame_stft(y, p)
        frames = list(sep_frame(y, l, g, p, H0))
        tr = frames.pop()
        traces.append(tr)
        A = tr["A"]
        for B, off, ranges in ((Bx, 0, ev), (Bd, R_x, nz)):
            for lo, hi in ranges:
                spec = B[:, lo:hi] @ A[off + lo:off + hi]
                if melconv:
                    spec = g["melmat"].T @ spec
                frames.append(synth_ifft_buff(spec, Yp, sz, p["fftlength"], p["win_ISTFT"], p["preemph"], p["DCbin_back"], p["pow"])
                              * p["overlapscale"])
        if l > p["delay"]:
            for k, fr in enumerate(frames):
                bufs[k, :sz - hop] = bufs[k, hop:].copy()
                bufs[k, sz - hop:] = 0.0
                bufs[k] += fr
                outs[k].append(bufs[k, :hop].copy())
        l += 1
    cat = [np.concatenate(o) if o else np.zeros(0) for o in outs]
    return dict(x_tilde_f=cat[0], x_hat=cat[1], d_hat=cat[2], x_hat_i=np.array(cat[3:3 + len(ev)]), d_hat_i=np.array(cat[3 + len(ev):]),
                trace=traces, basis=g["B_Mel_d"] if is_mel else g["B_DFT_d"])
