"""Writes tests/golden/online_f64/lm_decisions.npz: the fp64 oracle's per-frame decisions (n_iter, trig, n_up, adapt_iters)
for `lm_in` of refwav_pairs.npz -- the reference's own wav/LM_in.wav, 1777 frames -- with the shipped settings and the
H0 / Ad_blk0 of tests/test_online.py's fixture_inputs().  (A directory of its own: tests/test_oracle.py takes every
tests/golden/*.npz for a solver case.)  tests/test_online_f64.py pins the oracle
to it on the CPU and the fp64 device path to the oracle on the GPU.

    python tests/golden/make_golden_online_f64.py
"""
import os
import sys

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))

from oracle.online_oracle import default_params, ntf_sep_event_rt  # noqa: E402


def lm_inputs():
    s = np.load(os.path.join(GOLD, "refwav_pairs.npz"))["lm_in"]
    B = np.load(os.path.join(GOLD, "ref_data.npz"))["B"].astype(np.float64)
    rs = np.random.RandomState(1)
    H0 = rs.random_sample(200)
    Ad0 = rs.random_sample((50, 100))
    return s, B[:, :100], B[:, 100:], H0, Ad0


def main():
    s, Bx, Bd, H0, Ad0 = lm_inputs()
    o16, of, Bdn, tr = ntf_sep_event_rt(s, Bx, Bd, default_params(), H0, Ad0, return_trace=True)
    dec = {k: np.array([int(t[k]) for t in tr], dtype=np.int16) for k in ("n_iter", "trig", "n_up", "adapt_iters")}
    os.makedirs(os.path.join(GOLD, "online_f64"), exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "online_f64", "lm_decisions.npz"), **dec)
    print("frames", len(tr), "samples", len(o16), "triggered", int(dec["trig"].sum()), "solves", int((dec["adapt_iters"] > 0).sum()),
          "mean adaptation iterations", float(dec["adapt_iters"][dec["adapt_iters"] > 0].mean()))


if __name__ == "__main__":
    main()
