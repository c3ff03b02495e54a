"""The batched missing-data solve against the same problems solved one after the other in the fp64 mode (run on the GPU box; a
script, not a test; fails without a GPU).

For each shape and each B in {1, 8, 64}: ONE snmf_mdi_batch call on B problems against B snmf_mdi(..., precision="fp64")
calls made one after the other -- whole calls, allocation and transfers included, each ending in a synchronise (both return
host arrays).  Every problem has a binary mask that drops about 30 % of its entries.  KL, sparsity_mdi 5, 50 iterations with
the objective, no early stop.  The measurement of one (shape, B) is a process of its own (this script started again with
--one, under a time limit): a warm-up of both, then the two alternate REPS times and the medians are reported.  Every
(shape, B) also checks that problem 0 and problem B - 1 of the batch have the bits of the single solve.  One JSON line per
(shape, B) goes to profiles/mdi_batch_bench.jsonl (or --out); no ratio is expected in advance.

    python scripts/bench_mdi_batch.py [--out FILE] [--B 1,8,64] [--reps 5] [--shapes c1,f513] [--limit SECONDS]
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
    "c1": dict(F=257, T=2000, r=40, iters=50),  # the shapes of the batch tables (scripts/bench_batch_f64.py)
    "f513": dict(F=513, T=500, r=100, iters=50),
}
DROP = 0.3


def one(name, B, reps):
    """The record of one (shape, B), measured in this process."""
    from se_snmf_nat_amd import BatchPlanMdi64, Context, _lib, snmf_mdi, snmf_mdi_batch
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_mdi_batch: no HIP device is visible (there is no CPU path to fall back to)")
    ctx = Context(0)
    sh = SHAPES[name]
    F, T, r, iters = sh["F"], sh["T"], sh["r"], sh["iters"]
    rs = np.random.default_rng(0)
    probs = []
    for _ in range(B):  # every problem its own data and its own mask
        V = np.asfortranarray(rs.gamma(0.5, 1.0, (F, r // 2)) @ rs.gamma(0.3, 1.0, (r // 2, T)) + 1e-9)
        M = np.asfortranarray((rs.random((F, T)) > DROP).astype(np.float64))
        probs.append((V, M, np.asfortranarray(rs.random((F, r))), np.asfortranarray(rs.random((r, T)))))
    ps = dict(cf="kl", sparsity_mdi=5.0, max_iter=iters, conv_eps_mdi=0.0, cost_check=1)

    def single():
        t0 = time.perf_counter()
        out = [snmf_mdi(V, M, dict(ps, init_w=W0, init_h=H0), ctx=ctx, precision="fp64") for V, M, W0, H0 in probs]
        ctx.sync()
        return time.perf_counter() - t0, out

    def batch():
        t0 = time.perf_counter()
        out = snmf_mdi_batch([q[0] for q in probs], [q[1] for q in probs],
                             dict(ps, init_w=[q[2] for q in probs], init_h=[q[3] for q in probs]), ctx=ctx)
        ctx.sync()
        return time.perf_counter() - t0, out

    single(), batch()  # warm-up
    ts, tb = [], []
    for _ in range(reps):
        t, rs_ = single()
        ts.append(t)
        t, rb_ = batch()
        tb.append(t)
    for k in (0, B - 1):  # the contract, on the timed runs themselves
        assert rb_[k][2]["n_iter"] == rs_[k][2]["n_iter"] == iters
        assert rb_[k][0].tobytes() == rs_[k][0].tobytes() and rb_[k][1].tobytes() == rs_[k][1].tobytes()
        assert rb_[k][2]["cost"].tobytes() == rs_[k][2]["cost"].tobytes()
    bp = BatchPlanMdi64(ctx, F, r, [T] * B, beta=1.0, max_iter=iters, sparsity=5.0)
    geometry = bp.describe()
    bp.close()
    med = lambda x: float(np.median(x))  # noqa: E731
    return dict(shape=name, F=F, T=T, r=r, iters=iters, B=B, drop=DROP, reps=reps, single_s=ts, batch_s=tb, single_med_s=med(ts),
                batch_med_s=med(tb), ratio=med(ts) / med(tb), ratio_worst=min(ts) / max(tb), spread_single=(max(ts) - min(ts)) / med(ts),
                spread_batch=(max(tb) - min(tb)) / med(tb), single_ms_per_problem=med(ts) / B * 1e3,
                batch_ms_per_problem=med(tb) / B * 1e3, geometry=geometry)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mdi_batch_bench.jsonl"))
    ap.add_argument("--B", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="c1,f513")
    ap.add_argument("--limit", type=int, default=240, help="seconds one (shape, B) may take")
    ap.add_argument("--one", default=None, help="SHAPE,B: measure this one here and print its JSON line")
    a = ap.parse_args()
    if a.one:
        name, B = a.one.split(",")
        print(json.dumps(one(name, int(B), a.reps)), flush=True)
        return
    lines = []
    for name in a.shapes.split(","):
        for B in a.B.split(","):  # each GPU step is a fresh process under its own time limit; a failed one ends the script
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", f"{name},{B}", "--reps", str(a.reps)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if res.returncode != 0:
                raise SystemExit(f"bench_mdi_batch: {name} B={B} ended with status {res.returncode}; nothing more is started")
            line = res.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
