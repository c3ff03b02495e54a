"""The batched offline solve in the fp64 mode against the same problems solved one after the other in the fp64 mode (run on
the GPU box; a script, not a test; fails without a GPU).

For each shape and each B in {1, 8, 64}: ONE sparse_nmf_batch_fp64 call on B problems against B
sparse_nmf(..., precision="fp64") calls made one after the other -- whole calls, allocation and transfers included, each
ending in a synchronise (both return host arrays).  The two alternate in one process after a warm-up of every shape and B;
each is repeated REPS times so that the spread is known.  KL, sparsity 5, 50 iterations with the objective, no early stop.
Every (shape, B) also checks that problem 0 and problem B - 1 of the batch have the bits of the single solve.  One JSON line
per (shape, B) goes to profiles/batch_f64_bench.jsonl (or --out).

    python scripts/bench_batch_f64.py [--out FILE] [--B 1,8,64] [--reps 5] [--shapes c1,f513]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "c1": dict(F=257, T=2000, r=40, iters=50),  # BASELINE config C1: the shapes of the fp32 batch's table (scripts/bench_batch.py)
    "f513": dict(F=513, T=500, r=100, iters=50),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_f64_bench.jsonl"))
    ap.add_argument("--B", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,f513")
    a = ap.parse_args()
    from se_snmf_nat_amd import BatchPlan64, Context, _lib, sparse_nmf, sparse_nmf_batch_fp64
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_batch_f64: no HIP device is visible (there is no CPU path to fall back to)")
    ctx = Context(0)
    Bs = [int(x) for x in a.B.split(",")]
    cases = []
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        F, T, r, iters = sh["F"], sh["T"], sh["r"], sh["iters"]
        rs = np.random.default_rng(0)
        probs = []
        for _ in range(max(Bs)):  # every problem its own data: nothing is shared through a cache line or a host page
            V = np.asfortranarray(rs.gamma(0.5, 1.0, (F, r // 2)) @ rs.gamma(0.3, 1.0, (r // 2, T)) + 1e-9)
            probs.append((V, np.asfortranarray(rs.random((F, r))), np.asfortranarray(rs.random((r, T)))))
        ps = dict(cf="kl", sparsity=5.0, max_iter=iters, conv_eps=0.0, cost_check=1)
        for B in Bs:
            sub = probs[:B]

            def single(sub=sub, ps=ps):
                t0 = time.perf_counter()
                out = [sparse_nmf(V, dict(ps, init_w=W0, init_h=H0), ctx=ctx, precision="fp64") for V, W0, H0 in sub]
                ctx.sync()
                return time.perf_counter() - t0, out

            def batch(sub=sub, ps=ps):
                t0 = time.perf_counter()
                out = sparse_nmf_batch_fp64([q[0] for q in sub], dict(ps, init_w=[q[1] for q in sub], init_h=[q[2] for q in sub]), ctx=ctx)
                ctx.sync()
                return time.perf_counter() - t0, out

            cases.append((name, sh, B, single, batch))
    for _, _, _, single, batch in cases:  # warm-up of every shape and B
        single(), batch()
    lines = []
    for name, sh, B, single, batch in cases:
        ts, tb = [], []
        for _ in range(a.reps):
            t, rs_ = single()
            ts.append(t)
            t, rb_ = batch()
            tb.append(t)
        for k in (0, B - 1):  # the contract, on the timed runs themselves
            assert rb_[k][2]["n_iter"] == rs_[k][2]["n_iter"] == sh["iters"]
            assert rb_[k][0].tobytes() == rs_[k][0].tobytes() and rb_[k][1].tobytes() == rs_[k][1].tobytes()
            assert rb_[k][2]["cost"].tobytes() == rs_[k][2]["cost"].tobytes()
        bp = BatchPlan64(ctx, sh["F"], sh["r"], [sh["T"]] * B, beta=1.0, max_iter=sh["iters"], sparsity=5.0)
        geometry = bp.describe()
        bp.close()
        med = lambda x: float(np.median(x))  # noqa: E731
        rec = dict(shape=name, F=sh["F"], T=sh["T"], r=sh["r"], iters=sh["iters"], B=B, reps=a.reps, single_s=ts, batch_s=tb,
                   single_med_s=med(ts), batch_med_s=med(tb), ratio=med(ts) / med(tb), ratio_worst=min(ts) / max(tb),
                   spread_single=(max(ts) - min(ts)) / med(ts), spread_batch=(max(tb) - min(tb)) / med(tb),
                   single_ms_per_problem=med(ts) / B * 1e3, batch_ms_per_problem=med(tb) / B * 1e3, geometry=geometry)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
