"""How far does the fp64 oracle of the online loop move when its inputs move by eps?  (CPU only.)

The loop is a feedback system; this script measures its own response, which is where the tolerances of
tests/test_online_f64.py come from (not from the device).  For `lm_in` (the reference's wav/LM_in.wav, 1777 frames) and
for the 124-frame fixture of tests/test_online.py it runs oracle/online_oracle.py once as is and once per row with
B_DFT_x, B_DFT_d and H0 multiplied by 1 + eps * N(0,1) (first row: one ulp on one entry of H0), and reports

  the first frame whose decisions (n_iter, trig, n_up, adapt_iters) differ,
  the overall relative error of the float signal, the per-hop maximum of ||d_hop|| / max(||ref_hop||, 1),
  the number of int16 samples that differ (and by how much), the relative error of the final B_DFT_d.

    python scripts/online_f64_sensitivity.py            # prints, writes profiles/online_f64_sensitivity.md
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.online_oracle import default_params, ntf_sep_event_rt  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("n_iter", "trig", "n_up", "adapt_iters")
ROWS = [("1 ulp on one H0 entry", None), ("1e-15", 1e-15), ("1e-13", 1e-13), ("1e-11", 1e-11), ("1e-9", 1e-9), ("1e-7 (fp32 level)", 1e-7)]


def inputs(which):
    B = np.load(os.path.join(GOLD, "ref_data.npz"))["B"].astype(np.float64)
    if which == "lm_in":
        s = np.load(os.path.join(GOLD, "refwav_pairs.npz"))["lm_in"]
    else:
        s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"]
    rs = np.random.RandomState(1)
    H0 = rs.random_sample(200)
    Ad0 = rs.random_sample((50, 100))
    return s, B[:, :100], B[:, 100:], H0, Ad0


def run(s, Bx, Bd, H0, Ad0):
    o16, of, Bdn, tr = ntf_sep_event_rt(s, Bx, Bd, default_params(), H0, Ad0, return_trace=True)
    dec = np.array([[int(t[k]) for k in KEYS] for t in tr])
    return o16, of, Bdn, dec


def compare(ref, got, hop=160):
    o16, of, Bdn, dec = ref
    p16, pf, PBd, pdec = got
    bad = np.nonzero((dec != pdec).any(axis=1))[0]
    first = int(bad[0]) + 1 if bad.size else None
    d = pf - of
    nh = len(of) // hop
    per = np.array([np.linalg.norm(d[j * hop:(j + 1) * hop]) / max(np.linalg.norm(of[j * hop:(j + 1) * hop]), 1.0) for j in range(nh)])
    di = np.abs(p16.astype(int) - o16.astype(int))
    return dict(first=first, overall=np.linalg.norm(d) / np.linalg.norm(of), per_hop=per.max(), n16=int((di > 0).sum()),
                max16=int(di.max()), basis=np.linalg.norm(PBd - Bdn) / np.linalg.norm(Bdn))


def table(which):
    s, Bx, Bd, H0, Ad0 = inputs(which)
    ref = run(s, Bx, Bd, H0, Ad0)
    frames = len(ref[3])
    lines = [f"### {which}: {frames} frames, {len(ref[0])} samples", "",
             "| eps | first frame with a different decision | signal, overall rel. | per-hop max rel. | int16 samples that differ | final B_DFT_d rel. |",
             "|---|---|---|---|---|---|"]
    for name, eps in ROWS:
        rs = np.random.RandomState(12345)
        if eps is None:
            H1 = H0.copy()
            H1[17] = np.nextafter(H1[17], 2.0)
            got = run(s, Bx, Bd, H1, Ad0)
        else:
            got = run(s, Bx * (1 + eps * rs.randn(*Bx.shape)), Bd * (1 + eps * rs.randn(*Bd.shape)), H0 * (1 + eps * rs.randn(*H0.shape)), Ad0)
        c = compare(ref, got)
        first = "none in %d" % frames if c["first"] is None else str(c["first"])
        n16 = "%d" % c["n16"] + (" (up to %d LSB)" % c["max16"] if c["n16"] else "")
        lines.append("| %s | %s | %.2g | %.2g | %s | %.2g |" % (name, first, c["overall"], c["per_hop"], n16, c["basis"]))
        print(lines[-1], flush=True)
    return lines


def main():
    out = ["# Online loop: the fp64 oracle's response to input perturbations", "",
           "Written by scripts/online_f64_sensitivity.py (CPU, oracle/online_oracle.py, shipped settings, H0 / Ad_blk0 from",
           "RandomState(1)).  B_DFT_x, B_DFT_d and H0 are multiplied by 1 + eps * N(0,1).  The bounds of tests/test_online_f64.py",
           "are read off the linear part of these tables.", ""]
    for which in ("lm_in", "fixture124"):
        print(which, flush=True)
        out += table(which) + [""]
    path = os.path.join(ROOT, "profiles", "online_f64_sensitivity.md")
    with open(path, "w") as f:
        f.write("\n".join(out))
    print("wrote", path)


if __name__ == "__main__":
    main()
