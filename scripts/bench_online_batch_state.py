#!/usr/bin/env python3
"""What a snapshot of the batched online separator costs: get_state and set_state of ALL streams of a running batch at the
shipped geometry (513 bins, r = 200, the 50 x 100 ring), next to the nearest operation there was before them, a restart of the
same streams with new dictionaries.  bench_online_batch.py's fixture: the committed audio tiled, the shipped dictionaries,
stream k reading from its own offset with its own H0 / Ad_blk0 (RandomState(1 + k)).

Timed are the C entries (snmf_online_batch_get_state / _set_state / _restart[_f64]) through ctypes with the buffers made
beforehand, each ended by a device synchronise (get and set synchronise themselves; the restart is followed by
snmf_ctx_sync), --reps times after one untimed call; the median and the whole spread (min, max) are reported, and once the
Python methods (which also build / read the per-field arrays).  One JSON line per (precision, S); with --out appended there.

Usage: python scripts/bench_online_batch_state.py [--streams 64 512] [--precisions fp32 fp64] [--reps 7] [--out profiles/online_batch_state_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, nargs="+", default=[64, 512])
ap.add_argument("--precisions", nargs="+", default=["fp32", "fp64"])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--seconds", type=float, default=0.25, help="audio every stream has consumed when its state is taken")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from se_snmf_nat_amd import Context, _lib  # noqa: E402
from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
s0 = np.load(os.path.join(G, "frontend_audio.npz"))["samples"].astype(np.float64)
n = int(a.seconds * 16000) + 7  # (a few samples stay pending)
tiled = np.tile(s0, int(np.ceil((n + 16000) / len(s0))) + 1)
p = default_settings()
ctx = Context(0)
lib = _lib.load()


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 3), "min_ms": round(1e3 * ts[0], 3), "max_ms": round(1e3 * ts[-1], 3)}


def timed(call, sync=False):
    out = []
    for i in range(a.reps + 1):  # the first call is the warm-up (code objects, the staging slab)
        t = time.perf_counter()
        call()
        if sync:
            _lib.check(lib.snmf_ctx_sync(ctx._h))
        out.append(time.perf_counter() - t)
    return spread(out[1:])


for prec in a.precisions:
    for S in a.streams:
        H = [np.random.RandomState(1 + k).random_sample(200) for k in range(S)]
        A = [np.random.RandomState(1 + k).random_sample((50, 100)) for k in range(S)]
        xs = [tiled[(k * 997) % 16000:(k * 997) % 16000 + n] for k in range(S)]
        sep = OnlineBatchSeparator(Bx, Bd, p, S, H0=H, Ad_blk0=A, ctx=ctx, precision=prec)
        sep.process(xs)  # running streams, not flushed
        info, _ = sep._state_layout(lib)
        rb = int(info.bytes)
        buf = np.zeros(S * rb, dtype=np.uint8)
        sl = np.arange(S, dtype=np.int32)
        get = timed(lambda: _lib.check(lib.snmf_online_batch_get_state(sep._h, S, sl.ctypes.data, buf.ctypes.data, buf.size)))
        put = timed(lambda: _lib.check(lib.snmf_online_batch_set_state(sep._h, S, sl.ctypes.data, buf.ctypes.data, buf.size)))
        t = time.perf_counter()
        states = sep.get_state(list(range(S)))
        py_get = time.perf_counter() - t
        t = time.perf_counter()
        sep.set_state(list(range(S)), states)
        py_set = time.perf_counter() - t
        del states
        sep.close()
        # the nearest operation before: fresh streams restarted with new dictionaries (F x R_d fp64 each), H0 and Ad_blk0
        sep = OnlineBatchSeparator(Bx, Bd, p, S, H0=H, Ad_blk0=A, ctx=ctx, precision=prec)
        dt = np.float64 if prec == "fp64" else np.float32
        Bn = np.ascontiguousarray(np.concatenate([np.asfortranarray(Bd * (1.0 + 1e-3 * k)).ravel(order="F") for k in range(S)]))
        Hn = np.ascontiguousarray(np.concatenate(H), dtype=dt)
        An = np.ascontiguousarray(np.concatenate([x.ravel(order="F") for x in A]), dtype=dt)
        restart = lib.snmf_online_batch_restart_f64 if prec == "fp64" else lib.snmf_online_batch_restart
        rst = timed(lambda: _lib.check(restart(sep._h, S, sl.ctypes.data, Bn.ctypes.data, Hn.ctypes.data, An.ctypes.data)), sync=True)
        sep.close()
        line = json.dumps({
            "config": "get_state / set_state of all streams of a running batch vs restart with new dictionaries; shipped geometry "
                      "(513 bins, r = 200, 50 x 100 ring), %s" % prec,
            "precision": prec, "streams": S, "record_bytes": rb, "bytes_moved": S * rb, "reps": a.reps,
            "get_state": get, "set_state": put, "restart_new_dictionaries": rst, "restart_bytes_uploaded": int(Bn.nbytes + Hn.nbytes + An.nbytes),
            "python_get_state_ms": round(1e3 * py_get, 3), "python_set_state_ms": round(1e3 * py_set, 3),
            "unit": "ms per call over all streams, host clock around a call that ends in a device synchronise"})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
