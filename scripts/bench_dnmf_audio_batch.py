"""The batched DNMF re-training FROM WAVEFORMS against the two ways the same waveforms could be re-trained before it (run on the
GPU box; a script, not a test; fails without a GPU).

For each shape, each precision and each B in {1, 8, 64}, three legs from the same B pairs of waveforms:
    (a) single   B run_basis_DNMF(x_k, d_k, B_k, p) calls, one after the other;
    (b) matrix   3 B stft_features calls (y_k = x_k + d_k formed on the host), then ONE run_basis_dnmf_batch on the 3 B spectrograms:
                 what a user of the batch did before run_basis_DNMF_batch existed;
    (c) audio    ONE run_basis_DNMF_batch call.
Whole calls from host arrays, allocation and transfers included, each leg ending in a synchronise.  KL, sparsity 5, 50
iterations per solve with the objective, no early stop; every leg starts solve 1 from the same given H0_k.  The measurement of
one (shape, precision, B) is a process of its own (this script started again with --one, under a time limit): a warm-up of the
three legs, then they alternate REPS times and the medians are reported, with each leg's spread ((max - min) / median) and the
worst-case ratios.  (c) counts as faster than (b) only where the medians differ by more than the sum of the two legs' absolute
spreads (c_beats_b).  The contracts are asserted on the timed runs, for problem 0 and problem B - 1: (c) has the bits of (b) in
both precisions, and of (a) in the fp64 mode.  The context's transfer counters of the last (b) and (c) legs are recorded
(stft_features moves its arrays outside the counted pipeline: the counters of (b) are those of its batch call).
One JSON line per (shape, precision, B) goes to profiles/dnmf_audio_batch_bench.jsonl (or --out); no ratio is expected in advance.

    python scripts/bench_dnmf_audio_batch.py [--out FILE] [--B 1,8,64] [--reps 3] [--shapes c1,f513] [--precisions fp32,fp64] [--limit SECONDS]
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

SHAPES = {
    "c1": dict(fftlength=512, framelength=400, frameshift=160, T=2000, R_x=20, R_d=20, iters=50),       # F = 257: the shape of the batch tables
    "f513": dict(fftlength=1024, framelength=640, frameshift=160, T=2000, R_x=100, R_d=100, iters=50),  # F = 513: the shipped front-end
}


def one(name, precision, B, reps):
    """The record of one (shape, precision, B), measured in this process."""
    from se_snmf_nat_amd import Context, _lib, frontend, run_basis_dnmf_batch, train
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_dnmf_audio_batch: no HIP device is visible (there is no CPU path to fall back to)")
    ctx = Context(0)
    sh = SHAPES[name]
    N, fl, shift, T, R_x, R_d, iters = (sh[k] for k in ("fftlength", "framelength", "frameshift", "T", "R_x", "R_d", "iters"))
    F, r = N // 2 + 1, R_x + R_d
    L = N + 2 + (T - 1) * shift
    sdt = np.float64 if precision == "fp64" else np.float32
    p = dict(frontend.default_params(), fftlength=N, framelength=fl, frameshift=shift, DCbin=1,
             win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(fl) / fl)), cf="kl", sparsity=5.0, max_iter=iters, conv_eps=0.0,
             cost_check=1, R_x=R_x, R_d=R_d, random_seed=1)
    assert frontend.num_frames_host(L, p) == T
    rs = np.random.default_rng(0)
    t = np.arange(L)
    xs, ds, Bs, H0s = [], [], [], []
    for _ in range(B):  # every problem its own waveforms, basis and initial activations
        tones = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in zip(rs.uniform(500, 3000, 4), rs.uniform(0.01, 0.4, 4), rs.uniform(0, 6, 4)))
        xs.append(np.ascontiguousarray((tones * (0.5 + 0.5 * np.sin(2 * np.pi * t / 9000.0)) + rs.standard_normal(L) * 100).astype(sdt)))
        ds.append(np.ascontiguousarray((rs.standard_normal(L) * 700).astype(sdt)))
        # (values that float32 holds exactly: leg (b) hands the fp32 engine float32 arrays, legs (a) and (c) doubles)
        Bs.append(np.asfortranarray((rs.random((F, r)) + 0.05).astype(np.float32).astype(np.float64)))
        H0s.append(np.asfortranarray(rs.random((r, T)).astype(np.float32).astype(np.float64)))
    xfer = {}

    def single():
        t0 = time.perf_counter()
        out = []
        for x, d, Bk, H0 in zip(xs, ds, Bs, H0s):
            info = {}
            b, a = train._run_basis_dnmf_audio(x, d, Bk, p, ctx=ctx, mel=False, h0=H0, want_a=True, precision=precision, info=info)
            out.append((b, a, info["n_iter"]))
        ctx.sync()
        return time.perf_counter() - t0, out

    def matrix():
        ctx.xfer_stats(reset=True)
        t0 = time.perf_counter()
        Ys, Xs, Ds = [], [], []
        for x, d in zip(xs, ds):
            Ys.append(frontend.stft_features(x + d, p, ctx=ctx, precision=precision))  # (the sum is taken in the sample type)
            Xs.append(frontend.stft_features(x, p, ctx=ctx, precision=precision))
            Ds.append(frontend.stft_features(d, p, ctx=ctx, precision=precision))
        info = {}
        out = run_basis_dnmf_batch(Ys, Xs, Ds, Bs, R_x, R_d, p, ctx=ctx, h0=H0s, precision=precision, dtype=sdt, info=info)
        ctx.sync()
        tt = time.perf_counter() - t0
        xfer["matrix"] = dict(ctx.xfer_stats())
        return tt, [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]

    def audio():
        ctx.xfer_stats(reset=True)
        t0 = time.perf_counter()
        info = {}
        out = train.run_basis_DNMF_batch(xs, ds, Bs, p, ctx=ctx, h0=H0s, precision=precision, info=info)
        ctx.sync()
        tt = time.perf_counter() - t0
        xfer["audio"] = dict(ctx.xfer_stats())
        return tt, [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]

    single(), matrix(), audio()  # warm-up
    ta, tb, tc = [], [], []
    for _ in range(reps):
        tt, ra = single()
        ta.append(tt)
        tt, rb = matrix()
        tb.append(tt)
        tt, rc = audio()
        tc.append(tt)
    for k in sorted({0, B - 1}):  # the contracts, on the timed runs themselves
        assert rc[k][2] == rb[k][2] == ra[k][2] == [iters] * 3
        assert rc[k][0].astype(sdt).tobytes() == rb[k][0].tobytes() and rc[k][1].astype(sdt).tobytes() == rb[k][1].tobytes()
        if precision == "fp64":
            assert rc[k][0].tobytes() == ra[k][0].tobytes() and rc[k][1].tobytes() == ra[k][1].tobytes()
    med = lambda v: float(np.median(v))  # noqa: E731
    width = lambda v: float(max(v) - min(v))  # noqa: E731
    return dict(shape=name, precision=precision, F=F, T=T, fftlength=N, frameshift=shift, R_x=R_x, R_d=R_d, iters=iters, B=B, reps=reps,
                single_s=ta, matrix_s=tb, audio_s=tc, single_med_s=med(ta), matrix_med_s=med(tb), audio_med_s=med(tc),
                spread_single=width(ta) / med(ta), spread_matrix=width(tb) / med(tb), spread_audio=width(tc) / med(tc),
                matrix_over_audio=med(tb) / med(tc), matrix_over_audio_worst=min(tb) / max(tc),
                single_over_audio=med(ta) / med(tc), single_over_audio_worst=min(ta) / max(tc),
                c_beats_b=bool(med(tb) - med(tc) > width(tb) + width(tc)), b_beats_c=bool(med(tc) - med(tb) > width(tb) + width(tc)),
                audio_ms_per_problem=med(tc) / B * 1e3, matrix_last_xfer=xfer["matrix"], audio_last_xfer=xfer["audio"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dnmf_audio_batch_bench.jsonl"))
    ap.add_argument("--B", default="1,8,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,f513")
    ap.add_argument("--precisions", default="fp32,fp64")
    ap.add_argument("--limit", type=int, default=240, help="seconds one (shape, precision, B) may take")
    ap.add_argument("--one", default=None, help="SHAPE,PRECISION,B: measure this one here and print its JSON line")
    a = ap.parse_args()
    if a.one:
        name, precision, B = a.one.split(",")
        print(json.dumps(one(name, precision, int(B), a.reps)), flush=True)
        return
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.shapes.split(","):
        for precision in a.precisions.split(","):
            for B in a.B.split(","):  # each GPU step is a fresh process under its own time limit; a failed one ends the script
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", f"{name},{precision},{B}",
                       "--reps", str(a.reps)]
                res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if res.returncode != 0:
                    raise SystemExit(f"bench_dnmf_audio_batch: {name} {precision} B={B} ended with status {res.returncode}; nothing more is started")
                line = res.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                lines.append(json.loads(line))
                with open(a.out, "w") as f:  # (rewritten after every step: what was measured is kept)
                    for rec in lines:
                        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
