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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,a11")
    ap.add_argument("--n64", default="20,120", help="N1,N2 of the fp64 calls")
    ap.add_argument("--n32", default="20,220", help="N1,N2 of the fp32 calls")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--f64-mfma-tflops", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_f64_bench.jsonl"))
    a = ap.parse_args()
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
