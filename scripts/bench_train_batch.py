"""The batched basis training against the single call it batches (run on the GPU box; a script, not a test; fails without a GPU).

For each precision and each B in {1, 8, 64}, two legs from the same B training signals (257 x 2000 features each: fftlength 512,
frameshift 160; R = 40 exemplars, F_order = 64):
    (a) single   B run_basis_train_signal(s_k, R, p) calls, one after the other: the loop l = 1:length(DB_path_list);
    (b) batch    ONE run_basis_train_signal_batch call.
Whole calls from host arrays, allocation, transfers and the host epilogue included, each leg ending in a synchronise.  KL, sparsity
5, 50 iterations per solve with the objective, no early stop, H0 drawn on the host as the single call draws it.  The measurement of
one (precision, B) is a process of its own (this script started again with --one, under a time limit): a warm-up of both legs,
then they alternate REPS times and the medians are reported, with each leg's spread ((max - min) / median) and the worst-case
ratio.  (b) counts as faster than (a) only where the medians differ by more than the sum of the two legs' absolute spreads
(batch_beats_single), and the other way round (single_beats_batch).  On the timed runs, for problem 0 and problem B - 1: in the
fp64 mode (b) must have the bits of (a); in the fp32 mode the single call runs another fp32 solver than the batch engine, so the
relative Frobenius distance of the dictionaries is recorded, not asserted.  The context's transfer counters of the last (b) leg are
recorded.  One JSON line per (precision, B) goes to profiles/train_batch_bench.jsonl (or --out); no ratio is expected in advance.

    python scripts/bench_train_batch.py [--out FILE] [--B 1,8,64] [--reps 3] [--precisions fp32,fp64] [--limit SECONDS]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(fftlength=512, framelength=400, frameshift=160, T=2000, R=40, F_order=64, iters=50)  # F = 257: the shape of the batch tables
KEYS = ("B_DFT_sub", "B_Mel_sub", "A_DFT_sub", "A_Mel_sub")


def one(precision, B, reps):
    """The record of one (precision, B), measured in this process."""
    from se_snmf_nat_amd import Context, _lib, frontend, train
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_train_batch: no HIP device is visible (there is no CPU path to fall back to)")
    ctx = Context(0)
    N, fl, shift, T, R, M, iters = (SHAPE[k] for k in ("fftlength", "framelength", "frameshift", "T", "R", "F_order", "iters"))
    F = N // 2 + 1
    L = N + 2 + (T - 1) * shift
    p = dict(frontend.default_params(), fftlength=N, framelength=fl, frameshift=shift, DCbin=1, F_order=M,
             win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(fl) / fl)), cf="kl", sparsity=5.0, max_iter=iters, conv_eps=0.0,
             cost_check=1, cluster_buff=1, train_Exemplar=0, random_seed=1)
    assert frontend.num_frames_host(L, p) == T
    rs = np.random.default_rng(0)
    t = np.arange(L)
    sigs, idx = [], []
    for _ in range(B):  # every problem its own signal and exemplar columns
        tones = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in zip(rs.uniform(500, 3000, 4), rs.uniform(0.01, 0.4, 4), rs.uniform(0, 6, 4)))
        sigs.append(np.ascontiguousarray(tones * (0.5 + 0.5 * np.sin(2 * np.pi * t / 9000.0)) + rs.standard_normal(L) * 100))
        idx.append(rs.choice(T, size=R, replace=False) + 1)
    xfer = {}

    def single():
        t0 = time.perf_counter()
        out = []
        for s, ix in zip(sigs, idx):
            info = {}
            o = train.run_basis_train_signal(s, R, p, sample_idx=ix, ctx=ctx, precision=precision, info=info)
            out.append((o, info["n_iter"]))
        ctx.sync()
        return time.perf_counter() - t0, out

    def batch():
        ctx.xfer_stats(reset=True)
        t0 = time.perf_counter()
        info = {}
        out = train.run_basis_train_signal_batch(sigs, R, p, sample_idx=idx, ctx=ctx, precision=precision, info=info)
        ctx.sync()
        tt = time.perf_counter() - t0
        xfer["batch"] = dict(ctx.xfer_stats())
        return tt, list(zip(out, info["n_iter"]))

    single(), batch()  # warm-up
    ta, tb = [], []
    for _ in range(reps):
        tt, ra = single()
        ta.append(tt)
        tt, rb = batch()
        tb.append(tt)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))  # noqa: E731
    dist = {}
    for k in sorted({0, B - 1}):  # on the timed runs themselves
        assert rb[k][1] == ra[k][1] == [iters, iters]
        assert rb[k][0]["B_DFT_sub"].shape == (F, R) and rb[k][0]["B_Mel_sub"].shape == (M, R)
        if precision == "fp64":
            assert all(rb[k][0][key].tobytes() == ra[k][0][key].tobytes() for key in KEYS)
        dist[str(k)] = {key: rel(rb[k][0][key], ra[k][0][key]) for key in KEYS}
    med = lambda v: float(np.median(v))  # noqa: E731
    width = lambda v: float(max(v) - min(v))  # noqa: E731
    return dict(precision=precision, F=F, T=T, fftlength=N, frameshift=shift, R=R, F_order=M, iters=iters, B=B, reps=reps,
                single_s=ta, batch_s=tb, single_med_s=med(ta), batch_med_s=med(tb),
                spread_single=width(ta) / med(ta), spread_batch=width(tb) / med(tb),
                single_over_batch=med(ta) / med(tb), single_over_batch_worst=min(ta) / max(tb),
                batch_beats_single=bool(med(ta) - med(tb) > width(ta) + width(tb)),
                single_beats_batch=bool(med(tb) - med(ta) > width(ta) + width(tb)),
                batch_ms_per_problem=med(tb) / B * 1e3, batch_vs_single_rel=dist, batch_last_xfer=xfer["batch"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batch_bench.jsonl"))
    ap.add_argument("--B", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="fp32,fp64")
    ap.add_argument("--limit", type=int, default=240, help="seconds one (precision, B) may take")
    ap.add_argument("--one", default=None, help="PRECISION,B: measure this one here and print its JSON line")
    a = ap.parse_args()
    if a.one:
        precision, B = a.one.split(",")
        print(json.dumps(one(precision, int(B), a.reps)), flush=True)
        return
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for precision in a.precisions.split(","):
        for B in a.B.split(","):  # each GPU step is a fresh process under its own time limit; a failed one ends the script
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", f"{precision},{B}", "--reps", str(a.reps)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if res.returncode != 0:
                raise SystemExit(f"bench_train_batch: {precision} B={B} ended with status {res.returncode}; nothing more is started")
            line = res.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(json.loads(line))
            with open(a.out, "w") as f:  # (rewritten after every step: what was measured is kept)
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
