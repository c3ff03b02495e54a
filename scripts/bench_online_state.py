#!/usr/bin/env python3
"""What the single-stream online separator's restart and state record cost at the shipped geometry (513 bins, r = 200, the
50 x 100 ring): OnlineSeparator.restart() on a flushed separator next to what there was before it, close() plus a new
OnlineSeparator, and get_state / set_state of one record.  bench_online.py's fixture: the committed audio, the shipped
dictionaries.

Every timed call is ended by a device synchronise (get and set synchronise themselves; the restart and the creation are
followed by snmf_ctx_sync), --reps times after one untimed call; the median and the whole spread (min, max) are reported.
The restart is timed as the Python method (a carry: no upload) and with a new dictionary and new draws (three uploads); the
state calls as the C entries through ctypes with the buffer made beforehand, and once as the Python methods (which also
build / read the per-field arrays).  One JSON line per precision; with --out appended there.

Usage: python scripts/bench_online_state.py [--precisions fp32 fp64] [--reps 9] [--out profiles/online_state_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--precisions", nargs="+", default=["fp32", "fp64"])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--seconds", type=float, default=0.4, help="audio of the file that is run between two restarts")
ap.add_argument("--out", default="")
a = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from se_snmf_nat_amd import Context, _lib  # noqa: E402
from se_snmf_nat_amd.online import OnlineSeparator, default_settings  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
s = np.load(os.path.join(G, "frontend_audio.npz"))["samples"].astype(np.float64)[:int(a.seconds * 16000) + 7]
p = default_settings()
rs = np.random.RandomState(1)
H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
ctx = Context(0)
lib = _lib.load()


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 3), "min_ms": round(1e3 * ts[0], 3), "max_ms": round(1e3 * ts[-1], 3)}


def sync():
    _lib.check(lib.snmf_ctx_sync(ctx._h))


def timed(call, between=None):
    out = []
    for i in range(a.reps + 1):  # the first call is the warm-up (code objects, the staging record)
        if between:
            between()
        sync()
        t = time.perf_counter()
        call()
        sync()
        out.append(time.perf_counter() - t)
    return spread(out[1:])


for prec in a.precisions:
    new = lambda: OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, precision=prec)  # noqa: E731
    box = [new()]

    def a_file():
        box[0].process(s, flush=True)

    def close_and_new():
        box[0].close()
        box[0] = new()
    line = {"config": "single-stream online separator, shipped geometry (513 bins, r = 200, 50 x 100 ring)", "precision": prec,
            "file_frames": len(s) // 160, "reps": a.reps}
    line["close_plus_new_ms"] = timed(close_and_new, a_file)
    line["restart_carry_ms"] = timed(lambda: box[0].restart(), a_file)
    line["restart_all_given_ms"] = timed(lambda: box[0].restart(B_DFT_d=Bd, H0=H0, Ad_blk0=Ad0), a_file)
    # one record out and in, on a running stream (7 samples pending)
    sep = box[0]
    sep.restart()
    sep.process(s[:len(s) // 2 // 160 * 160 + 7])
    info, _ = sep._state_layout(lib)
    buf = np.zeros(int(info.bytes), dtype=np.uint8)
    line["record_bytes"] = int(info.bytes)
    line["get_state_c_ms"] = timed(lambda: _lib.check(lib.snmf_online_get_state(sep._h, buf.ctypes.data, buf.size)))
    line["set_state_c_ms"] = timed(lambda: _lib.check(lib.snmf_online_set_state(sep._h, buf.ctypes.data, buf.size)))
    st = [None]

    def get_py():
        st[0] = sep.get_state()
    line["get_state_py_ms"] = timed(get_py)
    line["set_state_py_ms"] = timed(lambda: sep.set_state(st[0]))
    line["get_plus_set_c_median_ms"] = round(line["get_state_c_ms"]["median_ms"] + line["set_state_c_ms"]["median_ms"], 3)
    sep.close()
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, a.out)) or ".", exist_ok=True)
        with open(os.path.join(ROOT, a.out), "a") as f:
            f.write(json.dumps(line) + "\n")
