#!/usr/bin/env python3
"""Settings per stream in the fp64 batched online separator (OnlineBatchSeparator(precision="fp64", settings=[...])) on
bench_online_batch.py's fixture: the committed 1.2 s audio tiled, the shipped dictionaries, stream k reading from its own
offset with its own H0 / Ad_blk0 (RandomState(1 + k)).  ONE measurement per process (a fresh process per run, as
DESIGN.md's figures are taken); prints one JSON line and, with --out, appends it to that file.

  --mode mixed    the settings sweep as ONE batch: --per streams under each of the four settings (shipped, Wiener,
                  adapt_train_N = 0, ED with sparsity 50), 4 * per streams, settings per stream
  --mode sweep    the same work without settings per stream: four uniform batches of --per streams, one after the other
  --mode uniform  one uniform batch of --streams streams at the shipped settings, through the interface that has no settings
                  list (--package-root: the checkout to import the package from, to measure another commit with this script)
Usage: python scripts/bench_online_batch_settings_f64.py --mode mixed [--per 64] [--seconds 3] [--out profiles/online_batch_settings_f64_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("mixed", "sweep", "uniform"), required=True)
ap.add_argument("--per", type=int, default=64)
ap.add_argument("--streams", type=int, default=64)
ap.add_argument("--seconds", type=float, default=3.0)
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--label", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.package_root))
import numpy as np  # noqa: E402

from se_snmf_nat_amd import Context  # noqa: E402
from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
s0 = np.load(os.path.join(G, "frontend_audio.npz"))["samples"].astype(np.float64)
n = int(a.seconds * 16000)
tiled = np.tile(s0, int(np.ceil((n + 16000) / len(s0))) + 1)
p = default_settings()
ctx = Context(0)
SWEEP = [dict(), dict(ENHANCE_METHOD="Wiener"), dict(adapt_train_N=0), dict(cf="ed", sparsity=50.0)]
NAMES = ["shipped", "Wiener", "adapt_train_N=0", "ED sparsity 50"]


def inputs(ks):
    xs, H, A = [], [], []
    for k in ks:
        off = (k * 997) % 16000
        xs.append(tiled[off:off + n])
        rs = np.random.RandomState(1 + k)
        H.append(rs.random_sample(200))
        A.append(rs.random_sample((50, 100)))
    return xs, H, A


def run(ks, pk, settings=None):
    """-> (seconds of the whole-file call, frames, adaptation solves) of one batch; a short warm-up batch first (kernels loaded)."""
    xs, H, A = inputs(ks)
    kw = dict(settings=settings) if settings is not None else {}
    w = OnlineBatchSeparator(Bx, Bd, pk, len(ks), H0=H, Ad_blk0=A, ctx=ctx, precision="fp64", **kw)
    w.process([x[:1600] for x in xs])
    w.close()
    sep = OnlineBatchSeparator(Bx, Bd, pk, len(ks), H0=H, Ad_blk0=A, ctx=ctx, precision="fp64", **kw)
    t = time.perf_counter()
    sep.process(xs, flush=True)
    dt = time.perf_counter() - t
    tr = [sep.trace(k) for k in range(len(ks))]
    sep.close()
    return dt, sum(len(q) for q in tr), sum(f["solved"] for q in tr for f in q)


if a.mode == "mixed":
    S = 4 * a.per
    dt, nfr, solved = run(range(S), p, settings=[SWEEP[k // a.per] for k in range(S)])
    out = {"config": "settings sweep as one fp64 batch: %d streams x 4 settings (%s), settings per stream" % (a.per, ", ".join(NAMES)),
           "streams": S, "seconds": dt}
elif a.mode == "sweep":
    dt = nfr = solved = 0
    parts = []
    for j, var in enumerate(SWEEP):  # the same streams as the mixed batch's, variant by variant
        d, f, sv = run(range(j * a.per, (j + 1) * a.per), dict(p, **var))
        parts.append(round(d, 4))
        dt, nfr, solved = dt + d, nfr + f, solved + sv
    out = {"config": "settings sweep as four uniform fp64 batches of %d streams, one after the other (%s)" % (a.per, ", ".join(NAMES)),
           "streams": 4 * a.per, "seconds": dt, "seconds_per_batch": parts}
else:
    dt, nfr, solved = run(range(a.streams), p)
    out = {"config": "uniform fp64 batch, shipped settings, %d streams" % a.streams, "streams": a.streams, "seconds": dt}
out.update(mode=a.mode, label=a.label, frames=nfr, adaptation_solves=solved, value=nfr / dt, unit="frames/s (all streams, whole file per call)",
           seconds_per_stream=a.seconds)
line = json.dumps(out)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")
