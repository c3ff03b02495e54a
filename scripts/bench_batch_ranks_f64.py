"""The fp64 batch with a rank per problem: what it costs the uniform batch, and what it saves a workload with two ranks (run on the
GPU box; a script, not a test; fails without a GPU).

The script runs on a tree with the mixed-rank entries and on one without them (it looks for snmf_batch_create_ranks_fp64 in the
binding), so that the same legs can be timed on a commit and on its parent:
    uniform   64 problems of 257 x 2000, r = 40, ONE sparse_nmf_batch_fp64 call (snmf_batch_create_fp64).  The kernels now read the
              rank from the table of problems: this is the leg that could regress.
    mixed     32 problems at r = 40 plus 32 at r = 20.  With the entries: ONE call with the ranks.  Without: the two uniform batches,
              one after the other.
    training  run_basis_train_signal_batch in fp64 on 8 signals of 257 x 2000 (fftlength 512, frameshift 160, F_order = 64) with
              R = [40] * 4 + [20] * 4.  With the entries: ONE call.  Without: one call per R.
Whole calls from host arrays, allocation and transfers included, each ending in a synchronise; KL, sparsity 5, 50 iterations with
the objective, conv_eps = 0.  Every leg is warmed up once and then run --reps times (default 3); the line of a leg holds every
time, the median and the spread (max - min).  With the entries the timed mixed and training results are also checked, on their
first and last problem, for the bits of the uniform calls.  One JSON line per leg goes to --out (appended, with --label).

    python scripts/bench_batch_ranks_f64.py [--out FILE] [--label NAME] [--reps 3] [--legs uniform,mixed,training]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, T, ITERS = 257, 2000, 50
R_HI, R_LO = 40, 20
TRAIN = dict(fftlength=512, framelength=400, frameshift=160, F_order=64, n_hi=4, n_lo=4)
KEYS = ("B_DFT_sub", "B_Mel_sub", "A_DFT_sub", "A_Mel_sub")


def timed(fn, ctx, reps):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return ts, out


def stats(ts):
    return dict(times_ms=[1e3 * t for t in ts], median_ms=1e3 * float(np.median(ts)), spread_ms=1e3 * (max(ts) - min(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_ranks_f64_bench.jsonl"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="uniform,mixed,training")
    a = ap.parse_args()
    from se_snmf_nat_amd import Context, _lib, frontend, sparse_nmf_batch_fp64, train
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_batch_ranks_f64: no HIP device is visible (there is no CPU path to fall back to)")
    has_ranks = "snmf_batch_create_ranks_fp64" in _lib.SYMBOLS
    ctx = Context(0)
    legs = a.legs.split(",")
    ps = dict(cf="kl", sparsity=5.0, max_iter=ITERS, conv_eps=0.0, cost_check=1)
    rs = np.random.default_rng(0)

    def problems(n, r):  # every problem its own data
        out = []
        for _ in range(n):
            V = np.asfortranarray(rs.gamma(0.5, 1.0, (F, R_HI // 2)) @ rs.gamma(0.3, 1.0, (R_HI // 2, T)) + 1e-9)
            out.append((V, np.asfortranarray(rs.random((F, r))), np.asfortranarray(rs.random((r, T)))))
        return out

    def solve(probs):
        return sparse_nmf_batch_fp64([q[0] for q in probs], dict(ps, init_w=[q[1] for q in probs], init_h=[q[2] for q in probs]), ctx=ctx)

    lines = []

    def emit(leg, ts, **kw):
        rec = dict(label=a.label, has_ranks=has_ranks, leg=leg, F=F, T=T, iters=ITERS, reps=a.reps, **stats(ts), **kw)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    if "uniform" in legs:
        probs = problems(64, R_HI)
        ts, out = timed(lambda: solve(probs), ctx, a.reps)
        assert all(o["n_iter"] == ITERS for _, _, o in out)
        emit("uniform", ts, B=64, r=R_HI)
    if "mixed" in legs:
        hi, lo = problems(32, R_HI), problems(32, R_LO)
        if has_ranks:
            ts, out = timed(lambda: solve(hi + lo), ctx, a.reps)
            ref = solve(hi) + solve(lo)
            for k in (0, 31, 32, 63):
                assert out[k][0].tobytes() == ref[k][0].tobytes() and out[k][1].tobytes() == ref[k][1].tobytes()
                assert out[k][2]["cost"].tobytes() == ref[k][2]["cost"].tobytes()
            emit("mixed", ts, B=64, ranks=[R_HI] * 32 + [R_LO] * 32, how="one batch with a rank per problem")
        ts, _ = timed(lambda: (solve(hi), solve(lo)), ctx, a.reps)
        emit("mixed_as_two_uniform_batches", ts, B=64, ranks=[R_HI] * 32 + [R_LO] * 32, how="two uniform batches, one after the other")
    if "training" in legs:
        N, fl, shift, M = (TRAIN[k] for k in ("fftlength", "framelength", "frameshift", "F_order"))
        L = N + 2 + (T - 1) * shift
        p = dict(frontend.default_params(), fftlength=N, framelength=fl, frameshift=shift, DCbin=1, F_order=M,
                 win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(fl) / fl)), cluster_buff=1, train_Exemplar=0, random_seed=1, **ps)
        assert frontend.num_frames_host(L, p) == T
        t = np.arange(L)
        Rs = [R_HI] * TRAIN["n_hi"] + [R_LO] * TRAIN["n_lo"]
        sigs, idx = [], []
        for r in Rs:
            tones = sum(c * np.sin(2 * np.pi * f * t + ph) for c, f, ph in zip(rs.uniform(500, 3000, 4), rs.uniform(0.01, 0.4, 4), rs.uniform(0, 6, 4)))
            sigs.append(np.ascontiguousarray(tones * (0.5 + 0.5 * np.sin(2 * np.pi * t / 9000.0)) + rs.standard_normal(L) * 100))
            idx.append(rs.choice(T, size=r, replace=False) + 1)
        nh = TRAIN["n_hi"]

        def two_calls():
            return (train.run_basis_train_signal_batch(sigs[:nh], R_HI, p, sample_idx=idx[:nh], ctx=ctx, precision="fp64")
                    + train.run_basis_train_signal_batch(sigs[nh:], R_LO, p, sample_idx=idx[nh:], ctx=ctx, precision="fp64"))

        if has_ranks:
            ts, out = timed(lambda: train.run_basis_train_signal_batch(sigs, Rs, p, sample_idx=idx, ctx=ctx, precision="fp64"), ctx, a.reps)
            ref = two_calls()
            for k in (0, nh - 1, nh, len(Rs) - 1):
                assert all(out[k][key].tobytes() == ref[k][key].tobytes() for key in KEYS)
            emit("training", ts, B=len(Rs), R=Rs, F_order=M, how="one call with an R per problem")
        ts, _ = timed(two_calls, ctx, a.reps)
        emit("training_as_two_calls", ts, B=len(Rs), R=Rs, F_order=M, how="one call per R")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
