"""The fp64 DNMF batch with a rank pair and settings per problem: what a sweep gains from being one call, and that the uniform
call costs what it did (run on the GPU box; a script, not a test; fails without a GPU).

The script runs on a tree with the _ranks_fp64 entries and on one without them (it looks for snmf_run_basis_dnmf_batch_ranks_fp64
in the binding), so that the uniform leg can be timed on a commit and on its parent, one process each:
    uniform    64 re-trainings of 257 x 2000 at (R_x, R_d) = (20, 20), KL, ONE run_basis_dnmf_batch(precision="fp64") call with
               scalar ranks: the uniform entry, whose driver now shares its phases with the new one.
    ranks      32 re-trainings at (20, 20) plus 32 at (40, 20).  Always: two uniform calls back to back.  With the entries also:
               ONE call with the pairs as lists.
    sparsity   16 re-trainings x sparsity (1, 5, 20, 50) at (20, 20).  Always: four uniform calls.  With the entries also: ONE call
               with settings per problem.
Whole calls from host arrays, allocation and transfers included, each ending in a synchronise; 50 iterations per solve with the
objective, conv_eps = 0.  Every leg is warmed up once and then run --reps times (default 3); the line of a leg holds every time,
the median and the spread (max - min).  With the entries the timed one-call results are also checked, on the first and last problem
of every group, for the bits of the uniform calls.  One JSON line per leg goes to --out (appended, with --label).

    python scripts/bench_dnmf_batch_ranks_f64.py [--out FILE] [--label NAME] [--reps 3] [--legs uniform,ranks,sparsity]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dnmf_batch_ranks_f64_bench.jsonl"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="uniform,ranks,sparsity")
    a = ap.parse_args()
    from se_snmf_nat_amd import Context, _lib, run_basis_dnmf_batch
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_dnmf_batch_ranks_f64: no HIP device is visible (there is no CPU path to fall back to)")
    has_ranks = "snmf_run_basis_dnmf_batch_ranks_fp64" in _lib.SYMBOLS
    ctx = Context(0)
    legs = a.legs.split(",")
    base = dict(cf="kl", sparsity=5.0, max_iter=ITERS, conv_eps=0.0, cost_check=1)
    rs = np.random.default_rng(0)

    def problems(n, R_x, R_d):  # every problem its own data: (Y, X, D, B, H0)
        out = []
        for _ in range(n):
            X = np.asfortranarray(rs.gamma(0.5, 1.0, (F, R_x)) @ rs.gamma(0.3, 1.0, (R_x, T)) + 1e-9)
            D = np.asfortranarray(rs.gamma(0.5, 1.0, (F, R_d)) @ rs.gamma(0.3, 1.0, (R_d, T)) + 1e-9)
            out.append((X + D, X, D, np.asfortranarray(rs.random((F, R_x + R_d))), np.asfortranarray(rs.random((R_x + R_d, T)))))
        return out

    def run(probs, R_x, R_d, p, **kw):
        info = {}
        out = run_basis_dnmf_batch([q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs], [q[3] for q in probs], R_x, R_d, p,
                                   ctx=ctx, h0=[q[4] for q in probs], precision="fp64", info=info, **kw)
        assert all(n == [ITERS] * 3 for n in info["n_iter"]), info["n_iter"]
        return out

    # a group: (problems, (R_x, R_d), settings that differ from `base`)
    def uniform_calls(groups):
        return [x for probs, (rx, rd), q in groups for x in run(probs, rx, rd, dict(base, **q))]

    def one_call(groups, with_settings):
        probs = [v for g, _, _ in groups for v in g]
        rx = [pair[0] for g, pair, _ in groups for _ in g]
        rd = [pair[1] for g, pair, _ in groups for _ in g]
        if with_settings:
            return run(probs, rx, rd, base, settings=[q for g, _, q in groups for _ in g])
        return run(probs, rx, rd, base)

    def check(out, groups):
        ref = uniform_calls(groups)
        at = 0
        for g, _, _ in groups:
            for k in (at, at + len(g) - 1):
                assert out[k][0].tobytes() == ref[k][0].tobytes() and out[k][1].tobytes() == ref[k][1].tobytes(), k
            at += len(g)

    lines = []

    def emit(leg, ts, **kw):
        rec = dict(label=a.label, has_ranks=has_ranks, leg=leg, F=F, T=T, iters=ITERS, reps=a.reps, **stats(ts), **kw)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def leg(name, groups, with_settings):
        B = sum(len(g) for g, _, _ in groups)
        if has_ranks:
            ts, out = timed(lambda: one_call(groups, with_settings), ctx, a.reps)
            check(out, groups)
            emit(name, ts, B=B, how="one call with " + ("settings" if with_settings else "a rank pair") + " per problem")
        ts, _ = timed(lambda: uniform_calls(groups), ctx, a.reps)
        emit(f"{name}_as_{len(groups)}_uniform_calls", ts, B=B, how="uniform calls, one after the other")

    if "uniform" in legs:
        probs = problems(64, 20, 20)
        ts, _ = timed(lambda: run(probs, 20, 20, base), ctx, a.reps)
        emit("uniform", ts, B=64, R_x=20, R_d=20)
    if "ranks" in legs:
        leg("ranks", [(problems(32, 20, 20), (20, 20), {}), (problems(32, 40, 20), (40, 20), {})], False)
    if "sparsity" in legs:
        leg("sparsity", [(problems(16, 20, 20), (20, 20), dict(sparsity=s)) for s in SPARSITIES], True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
