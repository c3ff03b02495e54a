"""Batched offline solve against the same problems solved one after the other (run on the GPU box; a script, not a test).

For each shape and each B in {1, 8, 64, 256}: the time of ONE resident batch run (BatchPlan.run) of B problems against the
time of B resident single solves (Plan.run, the path every caller has without the batch), the same number of iterations
each, no early stop.  The two alternate in one process after a warm-up of each; the clock is the host's, around work that
ends in a synchronise (uploads, W / H initialisation and downloads are outside it); each is repeated REPS times so that
the spread is known.  One JSON line per (shape, B) goes to profiles/batch_bench.jsonl (or --out).

    python scripts/bench_batch.py [--out FILE] [--B 1,8,64,256] [--reps 3] [--shapes c1,f513,mel64]
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
    "c1": dict(F=257, T=2000, r=40, iters=50),      # BASELINE config C1 (profiles/r03_bench_other_configs.jsonl)
    "f513": dict(F=513, T=500, r=100, iters=50),
    "mel64": dict(F=64, T=500, r=100, iters=50),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.jsonl"))
    ap.add_argument("--B", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c1,f513,mel64")
    a = ap.parse_args()
    from se_snmf_nat_amd import BatchPlan, Context, Plan
    ctx = Context(0)
    lines = []
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        F, T, r, iters = sh["F"], sh["T"], sh["r"], sh["iters"]
        rs = np.random.default_rng(0)
        V = np.asfortranarray(rs.gamma(0.5, 1.0, (F, r // 2)) @ rs.gamma(0.3, 1.0, (r // 2, T)) + 1e-9, dtype=np.float32)
        W0 = np.asfortranarray(rs.random((F, r)), dtype=np.float32)
        H0 = np.asfortranarray(rs.random((r, T)), dtype=np.float32)
        kw = dict(beta=1.0, max_iter=iters, conv_eps=0.0, cost_check=True, sparsity=5.0)
        plan = Plan(ctx, F, T, r, **kw)
        plan.set_v(V)
        for B in [int(x) for x in a.B.split(",")]:
            bp = BatchPlan(ctx, F, r, [T] * B, **kw)

            def single():
                tot = 0.0
                for _ in range(B):
                    plan.set_w(W0)
                    plan.set_h(H0)
                    plan.init()
                    ctx.sync()
                    t0 = time.perf_counter()
                    plan.run(iters)  # (returns the iterations run: the objective state is read back, i.e. it synchronises)
                    ctx.sync()
                    tot += time.perf_counter() - t0
                return tot

            def batch():
                for k in range(B):
                    bp.set_problem(k, V, W0, H0)
                ctx.sync()
                t0 = time.perf_counter()
                bp.run()  # (ends in a synchronise: the states are read back)
                ctx.sync()
                return time.perf_counter() - t0

            single(), batch()  # warm-up
            ts, tb = [], []
            for _ in range(a.reps):
                ts.append(single())
                tb.append(batch())
            n_it = [bp.get(k)[2]["n_iter"] for k in (0, B - 1)]
            assert n_it == [iters, iters], n_it
            med = lambda x: float(np.median(x))  # noqa: E731
            rec = dict(shape=name, F=F, T=T, r=r, iters=iters, B=B, single_s=ts, batch_s=tb, single_med_s=med(ts), batch_med_s=med(tb),
                       ratio=med(ts) / med(tb), ratio_worst=min(ts) / max(tb), spread_single=(max(ts) - min(ts)) / med(ts),
                       spread_batch=(max(tb) - min(tb)) / med(tb), single_us_per_iter=med(ts) / B / iters * 1e6,
                       batch_us_per_iter_per_problem=med(tb) / B / iters * 1e6, geometry=bp.describe(), single_geometry=plan.describe())
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            bp.close()
        plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
