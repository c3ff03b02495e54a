"""The batched DNMF re-training against the same problems re-trained one after the other (run on the GPU box; a script, not a
test; fails without a GPU).

For each shape, each precision and each B in {1, 8, 64}: ONE run_basis_dnmf_batch call on B problems against B
run_basis_dnmf(..., precision=...) calls made one after the other -- whole calls from host arrays, allocation and transfers
included, each ending in a synchronise.  KL, sparsity 5, 50 iterations per solve with the objective, no early stop.  The
measurement of one (shape, precision, B) is a process of its own (this script started again with --one, under a time limit): a
warm-up of both, then the two alternate REPS times and the medians are reported.  The contract is asserted on the timed runs,
for problem 0 and problem B - 1: in the fp64 mode the batch has the bits of the single loop it is timed against; in the fp32
mode it has the bits of three chained sparse_nmf_batch calls (the single fp32 loop runs other kernels), formed after the timing.
The context's transfer counters of the last batch call are recorded with it (batch_last_s, batch_last_xfer).
One JSON line per (shape, precision, B) goes to profiles/dnmf_batch_bench.jsonl (or --out); no ratio is expected in advance.

    python scripts/bench_dnmf_batch.py [--out FILE] [--B 1,8,64] [--reps 3] [--shapes c1,f513] [--precisions fp32,fp64] [--limit SECONDS]
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
    "c1": dict(F=257, T=2000, R_x=20, R_d=20, iters=50),      # the shape of the batch tables
    "f513": dict(F=513, T=2000, R_x=100, R_d=100, iters=50),  # the shipped dictionaries
}


def chained(ctx, q, R_x, R_d, ps):
    """Problem q through three sparse_nmf_batch calls of one problem each: the fp32 mode's contract."""
    from se_snmf_nat_amd import sparse_nmf_batch
    Y, X, D, B, H0 = q
    r = R_x + R_d
    on, off = (lambda n: np.ones(n, bool)), (lambda n: np.zeros(n, bool))
    _, A, _ = sparse_nmf_batch([Y], dict(ps, init_w=[B], init_h=[H0], w_update_ind=off(r), h_update_ind=on(r)), ctx=ctx)[0]
    w2 = sparse_nmf_batch([X], dict(ps, init_w=[B[:, :R_x]], init_h=[A[:R_x]], w_update_ind=on(R_x), h_update_ind=off(R_x)), ctx=ctx)[0][0]
    w3 = sparse_nmf_batch([D], dict(ps, init_w=[B[:, R_x:]], init_h=[A[R_x:]], w_update_ind=on(R_d), h_update_ind=off(R_d)), ctx=ctx)[0][0]
    return np.concatenate([w2, w3], axis=1), A


def one(name, precision, B, reps):
    """The record of one (shape, precision, B), measured in this process."""
    from se_snmf_nat_amd import Context, _lib, run_basis_dnmf, run_basis_dnmf_batch
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_dnmf_batch: no HIP device is visible (there is no CPU path to fall back to)")
    ctx = Context(0)
    sh = SHAPES[name]
    F, T, R_x, R_d, iters = sh["F"], sh["T"], sh["R_x"], sh["R_d"], sh["iters"]
    r = R_x + R_d
    rs = np.random.default_rng(0)
    probs = []
    for _ in range(B):  # every problem its own features, basis and initial activations
        X = np.asfortranarray(rs.gamma(0.5, 1.0, (F, R_x // 2)) @ rs.gamma(0.3, 1.0, (R_x // 2, T)) + 1e-9)
        D = np.asfortranarray(rs.gamma(0.5, 1.0, (F, R_d // 2)) @ rs.gamma(0.3, 1.0, (R_d // 2, T)) + 1e-9)
        probs.append((np.asfortranarray(X + D), X, D, np.asfortranarray(rs.random((F, r))), np.asfortranarray(rs.random((r, T)))))
    ps = dict(cf="kl", sparsity=5.0, max_iter=iters, conv_eps=0.0, cost_check=1)
    xfer = {}

    def single():
        t0 = time.perf_counter()
        out = []
        for Y, X, D, Bk, H0 in probs:
            info = {}
            b, a = run_basis_dnmf(Y, X, D, Bk, R_x, R_d, ps, ctx=ctx, precision=precision, h0=H0, info=info)
            out.append((b, a, info["n_iter"]))
        ctx.sync()
        return time.perf_counter() - t0, out

    def batch():
        ctx.xfer_stats(reset=True)
        t0 = time.perf_counter()
        info = {}
        out = run_basis_dnmf_batch([q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs], [q[3] for q in probs], R_x, R_d,
                                   ps, ctx=ctx, h0=[q[4] for q in probs], precision=precision, info=info)
        ctx.sync()
        t = time.perf_counter() - t0
        xfer.update(ctx.xfer_stats())  # (of the last batch call: what of its time went into moving the arrays)
        return t, [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]

    single(), batch()  # warm-up
    ts, tb = [], []
    for _ in range(reps):
        t, rs_ = single()
        ts.append(t)
        t, rb_ = batch()
        tb.append(t)
    for k in sorted({0, B - 1}):  # the contract, on the timed runs themselves
        assert rb_[k][2] == rs_[k][2] == [iters] * 3
        ref = rs_[k][:2] if precision == "fp64" else chained(ctx, probs[k], R_x, R_d, ps)
        assert rb_[k][0].tobytes() == ref[0].tobytes() and rb_[k][1].tobytes() == ref[1].tobytes()
    med = lambda x: float(np.median(x))  # noqa: E731
    return dict(shape=name, precision=precision, F=F, T=T, R_x=R_x, R_d=R_d, iters=iters, B=B, reps=reps, single_s=ts, batch_s=tb,
                single_med_s=med(ts), batch_med_s=med(tb), ratio=med(ts) / med(tb), ratio_worst=min(ts) / max(tb),
                spread_single=(max(ts) - min(ts)) / med(ts), spread_batch=(max(tb) - min(tb)) / med(tb),
                single_ms_per_problem=med(ts) / B * 1e3, batch_ms_per_problem=med(tb) / B * 1e3,
                batch_last_s=tb[-1], batch_last_xfer=xfer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dnmf_batch_bench.jsonl"))
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
                    raise SystemExit(f"bench_dnmf_batch: {name} {precision} B={B} ended with status {res.returncode}; nothing more is started")
                line = res.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                lines.append(json.loads(line))
                with open(a.out, "w") as f:  # (rewritten after every step: what was measured is kept)
                    for rec in lines:
                        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
