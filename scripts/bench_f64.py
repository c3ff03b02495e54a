#!/usr/bin/env python3
"""Per-iteration cost of the fp64 solve mode (precision="fp64", snmf_sparse_nmf_fp64) next to the fp32 path, same process.

The one-shot entries upload V, W0, H0 and download W, H on every call, so a single call's wall time is mostly PCIe.
The per-iteration cost is therefore taken as a difference in which the transfers cancel:

    s_per_iter = (time of a max_iter = N2 call - time of a max_iter = N1 call) / (N2 - N1)

each time the minimum over --reps calls.  Shapes: C2 (257 x 100000, r = 256, KL, sparsity 5: bench.py's flagship) and
a11 (513 x 72000, r = 100, KL), inputs from bench.make_problem, V and H0 rounded to fp32 as tests/golden/make_golden_c2.py
rounds them.  One JSON line per shape is appended to profiles/solve_f64_bench.jsonl:
iterations/s in fp64 and fp32, the f64 rate of the five GEMM products (4 * 2 F T r flop per KL iteration: W*H twice,
W'*R, R*H') and, with --f64-mfma-tflops X (the "f64 16x16x4" line of scripts/mfma_shape_bench.hip on the same device),
that rate as a fraction of the measured f64 MFMA rate.

    python scripts/bench_f64.py [--shapes c2,a11] [--f64-mfma-tflops X] [--out profiles/solve_f64_bench.jsonl]

--legs dnmf,mel: the resident fp64 DNMF loop (run_basis_dnmf(..., precision="fp64"): snmf_run_basis_dnmf_fp64) on BASELINE
config 4 (513 x 100000, R_x = R_d = 100, KL, 3 solves x --dnmf-iters iterations) and on its 64-row Mel twin, each next to
the three separate sparse_nmf(precision="fp64") calls it replaces (resident=False) and to the fp32 resident call.  Wall time
of the whole call, transfers included (that is what the resident form saves), minimum over --reps; h0 is an array drawn
outside the timed region.  One JSON line per leg is appended to profiles/train_f64_bench.jsonl.

    python scripts/bench_f64.py --legs dnmf,mel [--dnmf-iters 50] [--reps 2]

--legs mdi: the fp64 missing-data solve (snmf_mdi(..., precision="fp64"): snmf_mdi_fp64) next to the plain fp64 solve at a11,
binary mask with 30 % of the entries missing, by the same difference of two calls, each the minimum over --reps; the two
solves alternate inside every repetition, so that another job on the machine falls on both.  One JSON line is appended to
profiles/mdi_f64_bench.jsonl.

    python scripts/bench_f64.py --legs mdi [--n64 20,120] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c2": (257, 100000, 256), "a11": (513, 72000, 100)}


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


DNMF_LEGS = {"dnmf": (513, 100000, 100, 100), "mel": (64, 100000, 100, 100)}


def dnmf_legs(a):
    from se_snmf_nat_amd import Context, run_basis_dnmf
    ctx = Context(0)
    out = os.path.join(ROOT, "profiles", "train_f64_bench.jsonl") if a.out.endswith("solve_f64_bench.jsonl") else a.out
    for name in a.legs.split(","):
        F, T, Rx, Rd = DNMF_LEGS[name]
        rd = np.random.default_rng(1)
        X = np.asfortranarray(rd.gamma(0.5, 1.0, (F, Rx)) @ rd.gamma(0.3, 1.0, (Rx, T)))
        D = np.asfortranarray(rd.gamma(0.5, 1.0, (F, Rd)) @ rd.gamma(0.3, 1.0, (Rd, T)))
        Y = np.asfortranarray(X + D + 1e-9)
        B = np.asfortranarray(np.random.default_rng(3).random((F, Rx + Rd)))
        H0 = np.asfortranarray(np.random.RandomState(1).random_sample((Rx + Rd, T)))
        p = dict(cf="kl", sparsity=5, max_iter=a.dnmf_iters, conv_eps=0, cost_check=1, random_seed=1)
        modes = (("fp64_resident", dict(precision="fp64")), ("fp64_three_calls", dict(precision="fp64", resident=False)),
                 ("fp32_resident", dict()))
        line = dict(leg=name, F=F, T=T, R_x=Rx, R_d=Rd, cf="kl", sparsity=5, iters_per_solve=a.dnmf_iters, reps=a.reps)
        res = {}
        for mode, kw in modes:
            run_basis_dnmf(Y[:, :4096], X[:, :4096], D[:, :4096], B, Rx, Rd, dict(p, max_iter=2), ctx=ctx, h0=H0[:, :4096].copy(order="F"), **kw)  # warm-up
            t = timed(lambda: res.__setitem__(mode, run_basis_dnmf(Y, X, D, B, Rx, Rd, p, ctx=ctx, h0=H0, **kw)), a.reps)
            line[mode + "_s"] = round(t, 4)
            print(f"{name} {mode}: {t:.3f} s per call ({3 * a.dnmf_iters / t:.1f} solver iterations/s)", flush=True)
        line["three_calls_over_resident"] = line["fp64_three_calls_s"] / line["fp64_resident_s"]
        line["fp64_over_fp32_resident"] = line["fp64_resident_s"] / line["fp32_resident_s"]
        line["resident_equals_three_calls_bitwise"] = bool(res["fp64_resident"][0].tobytes() == res["fp64_three_calls"][0].tobytes())
        line["rel_fp32_vs_fp64_B_hat"] = float(np.linalg.norm(res["fp32_resident"][0] - res["fp64_resident"][0]) / np.linalg.norm(res["fp64_resident"][0]))
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)


def mdi_leg(a):
    from bench import SPARSITY, make_problem
    from se_snmf_nat_amd import Context, snmf_mdi, sparse_nmf
    ctx = Context(0)
    out = os.path.join(ROOT, "profiles", "mdi_f64_bench.jsonl") if a.out.endswith("solve_f64_bench.jsonl") else a.out
    F, T, r = SHAPES["a11"]
    V, W0, H0 = make_problem(F, T, r)
    V = np.asfortranarray(V.astype(np.float32).astype(np.float64))
    H0 = H0.astype(np.float32).astype(np.float64)
    M = np.asfortranarray(np.random.RandomState(0).rand(F, T) > 0.3, dtype=np.float64)
    n1, n2 = (int(x) for x in a.n64.split(","))
    base = dict(cf="kl", conv_eps=0, conv_eps_mdi=0, sparsity=SPARSITY, sparsity_mdi=SPARSITY, init_w=W0, init_h=H0, cost_check=1)
    solves = {"plain": lambda n: sparse_nmf(V, dict(base, max_iter=n), ctx=ctx, precision="fp64"),
              "mdi": lambda n: snmf_mdi(V, M, dict(base, max_iter=n), ctx=ctx, precision="fp64")}
    for fn in solves.values():
        fn(1)  # warm-up: allocations, code load
    best = {}
    for _ in range(a.reps):
        for n in (n1, n2):
            for k, fn in solves.items():
                t0 = time.perf_counter()
                fn(n)
                best[k, n] = min(best.get((k, n), float("inf")), time.perf_counter() - t0)
    line = dict(leg="mdi", F=F, T=T, r=r, cf="kl", sparsity=SPARSITY, missing=float(1 - M.mean()), n1=n1, n2=n2, reps=a.reps)
    for k in solves:
        spi = (best[k, n2] - best[k, n1]) / (n2 - n1)
        line[k] = dict(t_n1_s=round(best[k, n1], 4), t_n2_s=round(best[k, n2], 4), s_per_iter=spi, iter_per_s=1.0 / spi)
        print(f"a11 fp64 {k}: {1.0 / spi:.2f} iterations/s ({spi * 1e3:.2f} ms per iteration)", flush=True)
    line["mdi_over_plain"] = line["mdi"]["iter_per_s"] / line["plain"]["iter_per_s"]
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="", help="dnmf,mel: the resident fp64 DNMF loop instead of the one-shot shapes; mdi: the fp64 missing-data solve")
    ap.add_argument("--dnmf-iters", type=int, default=50)
    ap.add_argument("--shapes", default="c2,a11")
    ap.add_argument("--n64", default="20,120", help="N1,N2 of the fp64 calls")
    ap.add_argument("--n32", default="20,220", help="N1,N2 of the fp32 calls")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--f64-mfma-tflops", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_f64_bench.jsonl"))
    a = ap.parse_args()
    if a.legs == "mdi":
        return mdi_leg(a)
    if a.legs:
        return dnmf_legs(a)
    from bench import SPARSITY, make_problem
    from se_snmf_nat_amd import Context, sparse_nmf
    ctx = Context(0)
    for name in a.shapes.split(","):
        F, T, r = SHAPES[name]
        V, W0, H0 = make_problem(F, T, r)
        V = V.astype(np.float32).astype(np.float64)
        H0 = H0.astype(np.float32).astype(np.float64)
        base = dict(cf="kl", sparsity=SPARSITY, conv_eps=0, init_w=W0, init_h=H0, cost_check=1)
        line = dict(shape=name, F=F, T=T, r=r, cf="kl", sparsity=SPARSITY, reps=a.reps)
        for prec, ns in (("fp64", a.n64), ("fp32", a.n32)):
            n1, n2 = (int(x) for x in ns.split(","))
            sparse_nmf(V, dict(base, max_iter=1), ctx=ctx, precision=prec)  # warm-up: allocations, code load
            t1 = timed(lambda: sparse_nmf(V, dict(base, max_iter=n1), ctx=ctx, precision=prec), a.reps)
            t2 = timed(lambda: sparse_nmf(V, dict(base, max_iter=n2), ctx=ctx, precision=prec), a.reps)
            spi = (t2 - t1) / (n2 - n1)
            line[prec] = dict(n1=n1, n2=n2, t_n1_s=round(t1, 4), t_n2_s=round(t2, 4), s_per_iter=spi, iter_per_s=1.0 / spi)
            print(f"{name} {prec}: {1.0 / spi:.2f} iterations/s ({spi * 1e3:.2f} ms per iteration; calls {t1:.3f} s / {t2:.3f} s)",
                  flush=True)
        gemm_tflops = 4 * 2.0 * F * T * r / line["fp64"]["s_per_iter"] / 1e12
        line["fp64_gemm_tflops"] = gemm_tflops
        line["fp32_over_fp64"] = line["fp64"]["s_per_iter"] / line["fp32"]["s_per_iter"]
        if a.f64_mfma_tflops:
            line["f64_mfma_tflops_measured"] = a.f64_mfma_tflops
            line["fraction_of_f64_mfma_rate"] = gemm_tflops / a.f64_mfma_tflops
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
