#!/usr/bin/env python3
"""The chain driver (ntf_sep_event_rt_chains: slots restarted in place, Do_MultiBatch_IS16_20160324.m:183-205 +
run_ntf_sep_RT.m:10-41) against the status quo without restarts, on bench_online_batch.py's fixture: the committed audio
tiled, the shipped dictionaries and settings, adaptation on.  A seeded queue of files with lengths uniform in 2-8 s.
  independent: 6 S files, each from the shipped dictionary.  Status quo: consecutive groups of S files through
               ntf_sep_event_rt_batch (every group waits for its longest file).
  chains4:     S chains of 4 files, the dictionary carried from file to file.  Status quo: file i of every chain as one
               ntf_sep_event_rt_batch, started from the basis() each chain's file i-1 ended with.
Reports files/s, aggregate real frames/s, slot utilisation (real frames / (device frame steps x S)) and the longest
process call.  The driver runs with its default chunk_hops (one device chunk, 16384 / S hops) and, where that differs,
with --chunk-hops (a slot whose file ended waits for the end of the call before it restarts).  File f / chain c draws H0 / Ad_blk0 from RandomState(1 + f) / RandomState(1 + c) in both runs.  One JSON line.
Usage: python scripts/bench_online_chains.py [--streams 64,256] [--seed 7] [--chunk-hops 64]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from se_snmf_nat_amd import Context  # noqa: E402
from se_snmf_nat_amd import online  # noqa: E402
from se_snmf_nat_amd.online import default_settings, ntf_sep_event_rt_batch, ntf_sep_event_rt_chains  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="64,256")
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--chunk-hops", type=int, default=64)
a = ap.parse_args()

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
s0 = np.load(os.path.join(G, "frontend_audio.npz"))["samples"]
tiled = np.tile(s0, int(np.ceil((8 * 16000 + 16000) / len(s0))) + 1)
p = default_settings()
hop, tail = p["frameshift"], p["delay"] + 1
ctx = Context(0)


def files(n, seed):
    rs = np.random.RandomState(seed)
    lens = (rs.uniform(2.0, 8.0, n) * 16000).astype(int)
    return [tiled[(k * 997) % 16000:(k * 997) % 16000 + m] for k, m in enumerate(lens)]


def draws(k):
    rs = np.random.RandomState(1 + k)
    return rs.random_sample(200), rs.random_sample((50, 100))


class Meter:
    """Wraps OnlineBatchSeparator.process: device frame steps (the longest stream of a call sets them: every stream
    advances in the same launches) and the longest call."""

    def __init__(self):
        self.steps, self.longest = 0, 0.0
        self.orig = online.OnlineBatchSeparator.process

    def __enter__(self):
        meter = self

        def process(sep, pcms, flush=False):
            fl = [bool(flush)] * sep.S if np.isscalar(flush) else list(flush)
            meter.steps += max(len(x) // hop + (tail if f else 0) for x, f in zip(pcms, fl))
            t = time.perf_counter()
            r = meter.orig(sep, pcms, flush)
            meter.longest = max(meter.longest, time.perf_counter() - t)
            return r
        online.OnlineBatchSeparator.process = process
        self.t = time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.dt = time.perf_counter() - self.t
        online.OnlineBatchSeparator.process = self.orig


def report(m, fl, S):
    real = sum(len(x) // hop for x in fl)
    return {"files_per_s": round(len(fl) / m.dt, 2), "frames_per_s": round(real / m.dt, 1),
            "slot_utilisation": round(real / (m.steps * S), 3), "longest_call_ms": round(m.longest * 1e3, 1),
            "seconds": round(m.dt, 2)}


def drivers(ch, fl, S):
    out = {}
    for hops in (None, a.chunk_hops):
        if hops is not None and hops == max(1, min(4096, 16384 // S)):
            continue
        with Meter() as m:
            ntf_sep_event_rt_chains(ch, Bx, Bd, p, n_streams=S, ctx=ctx, chunk_hops=hops)
        out["driver" if hops is None else f"driver_chunk_hops_{hops}"] = report(m, fl, S)
    return out


def independent(S):
    fl = files(6 * S, a.seed + S)
    with Meter() as m:
        for g in range(0, len(fl), S):
            grp = list(range(g, min(g + S, len(fl))))
            ds = [draws(f) for f in grp]
            ntf_sep_event_rt_batch([fl[f] for f in grp], Bx, Bd, p, H0=[d[0] for d in ds], Ad_blk0=[d[1] for d in ds], ctx=ctx)
    return dict(drivers([[x] for x in fl], fl, S), status_quo=report(m, fl, S))


def chains4(S):
    fl = files(4 * S, a.seed + 1000 + S)
    ch = [fl[4 * c:4 * c + 4] for c in range(S)]
    ds = [draws(c) for c in range(S)]
    with Meter() as m:
        Bcur = [Bd] * S
        for i in range(4):
            res = ntf_sep_event_rt_batch([c[i] for c in ch], Bx, Bcur, p, H0=[d[0] for d in ds], Ad_blk0=[d[1] for d in ds], ctx=ctx)
            Bcur = [r[2] for r in res]
    return dict(drivers(ch, fl, S), status_quo=report(m, fl, S))


out = {"config": "C3 online separation, chain driver vs regrouped batches (shipped settings, adaptation on), 513 bins, r=200, "
                 "files uniform in 2-8 s", "unit": "files/s, real frames/s, real frames / (frame steps x S), ms"}
for S in [int(x) for x in a.streams.split(",") if x]:
    warm = files(2, a.seed)  # kernels loaded, chunk buffers of this S sized
    warm = [x[:3200] for x in warm]
    ntf_sep_event_rt_chains([warm] * S, Bx, Bd, p, n_streams=S, ctx=ctx)
    ntf_sep_event_rt_batch([warm[0]] * S, Bx, Bd, p, ctx=ctx)
    r = {"independent": independent(S), "chains4": chains4(S)}
    out[f"S={S}"] = r
    for k, v in r.items():
        print(f"# S={S} {k}: {v}", file=sys.stderr, flush=True)
print(json.dumps(out), flush=True)
