"""The fp64 batch with settings per problem: what it costs the uniform batch, and what a sweep gains from being one batch (run on
the GPU box; a script, not a test; fails without a GPU).

The script runs on a tree with the settings entries and on one without them (it looks for snmf_batch_create_settings_fp64 in the
binding), so that the same legs can be timed on a commit and on its parent, one process each:
    uniform    64 problems of 257 x 2000, r = 40, KL, ONE sparse_nmf_batch_fp64 call with a settings dict (snmf_batch_create_fp64).
               The kernels now read the settings from the table of problems: this is the leg that could regress.
    sparsity   16 problems x sparsity (1, 5, 20, 50), KL, r = 40.  Always: four uniform batches back to back.  With the entries
               also: ONE batch with a list of settings.
    modes      32 KL + 32 ED problems, r = 40.  Always: two uniform batches.  With the entries also: ONE batch.
Whole calls from host arrays, allocation and transfers included, each ending in a synchronise; 50 iterations with the objective,
conv_eps = 0.  Every leg is warmed up once and then run --reps times (default 3); the line of a leg holds every time, the median
and the spread (max - min).  With the entries the timed one-batch results are also checked, on the first and last problem of every
group, for the bits of the uniform calls.  One JSON line per leg goes to --out (appended, with --label).

    python scripts/bench_batch_settings_f64.py [--out FILE] [--label NAME] [--reps 3] [--legs uniform,sparsity,modes]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, T, R, ITERS = 257, 2000, 40, 50
SPARSITIES = (1.0, 5.0, 20.0, 50.0)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_settings_f64_bench.jsonl"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="uniform,sparsity,modes")
    a = ap.parse_args()
    from se_snmf_nat_amd import Context, _lib, sparse_nmf_batch_fp64
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_batch_settings_f64: no HIP device is visible (there is no CPU path to fall back to)")
    has_settings = "snmf_batch_create_settings_fp64" in _lib.SYMBOLS
    ctx = Context(0)
    legs = a.legs.split(",")
    base = dict(max_iter=ITERS, conv_eps=0.0, cost_check=1)
    rs = np.random.default_rng(0)

    def problems(n):  # every problem its own data
        out = []
        for _ in range(n):
            V = np.asfortranarray(rs.gamma(0.5, 1.0, (F, R // 2)) @ rs.gamma(0.3, 1.0, (R // 2, T)) + 1e-9)
            out.append((V, np.asfortranarray(rs.random((F, R))), np.asfortranarray(rs.random((R, T)))))
        return out

    def solve(probs, q):  # one uniform batch
        return sparse_nmf_batch_fp64([p[0] for p in probs], dict(base, **q, init_w=[p[1] for p in probs], init_h=[p[2] for p in probs]), ctx=ctx)

    def sweep(groups):  # one batch with settings per problem: groups = [(problems, settings), ...]
        vs = [p[0] for probs, _ in groups for p in probs]
        ps = [dict(base, **q, init_w=p[1], init_h=p[2]) for probs, q in groups for p in probs]
        return sparse_nmf_batch_fp64(vs, ps, ctx=ctx)

    def check(out, groups):
        ref = [x for probs, q in groups for x in solve(probs, q)]
        at = 0
        for probs, _ in groups:
            for k in (at, at + len(probs) - 1):
                assert out[k][0].tobytes() == ref[k][0].tobytes() and out[k][1].tobytes() == ref[k][1].tobytes(), k
                assert out[k][2]["cost"].tobytes() == ref[k][2]["cost"].tobytes(), k
            at += len(probs)

    lines = []

    def emit(leg, ts, **kw):
        rec = dict(label=a.label, has_settings=has_settings, leg=leg, F=F, T=T, r=R, iters=ITERS, reps=a.reps, **stats(ts), **kw)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def leg(name, groups):
        if has_settings:
            ts, out = timed(lambda: sweep(groups), ctx, a.reps)
            assert all(o["n_iter"] == ITERS for _, _, o in out)
            check(out, groups)
            emit(name, ts, B=sum(len(g) for g, _ in groups), how="one batch with settings per problem")
        ts, _ = timed(lambda: [solve(probs, q) for probs, q in groups], ctx, a.reps)
        emit(f"{name}_as_{len(groups)}_uniform_batches", ts, B=sum(len(g) for g, _ in groups), how="uniform batches, one after the other")

    if "uniform" in legs:
        probs = problems(64)
        ts, out = timed(lambda: solve(probs, dict(cf="kl", sparsity=5.0)), ctx, a.reps)
        assert all(o["n_iter"] == ITERS for _, _, o in out)
        emit("uniform", ts, B=64)
    if "sparsity" in legs:
        leg("sparsity", [(problems(16), dict(cf="kl", sparsity=s)) for s in SPARSITIES])
    if "modes" in legs:
        leg("modes", [(problems(32), dict(cf="kl", sparsity=5.0)), (problems(32), dict(cf="ed", sparsity=50.0))])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
