#!/usr/bin/env python3
"""The native chain driver (OnlineBatchSeparator.run_chains: one snmf_online_batch_run_chains_f32 call) against the Python
driver ntf_sep_event_rt_chains, on the corpus of scripts/bench_online_chains.py / profiles/online_chains_bench.jsonl: the
committed audio tiled, the shipped dictionaries and settings with adaptation on, a seeded queue of files with lengths
uniform in 2-8 s.
  independent: 6 S files, each a chain of its own from the shipped dictionary.
  chains4:     S chains of 4 files, the dictionary carried from file to file.
Both sides run in this process, in alternating order (A B B A ...), --reps times each, and each run includes making and
closing its batch.  Chain c draws H0 / Ad_blk0 from RandomState(1 + c) on both sides, so the outputs must be equal; the
first and last file's int16 signals are compared.  Both drivers feed fixed chunks (one device chunk, 16384 / S hops), so
they share one schedule: slot utilisation (real frames / (device frame steps x S)) is computed from it on the host.
Reports, per side, files/s and real frames/s of the median run and the run-to-run spread (max - min) / median of the
seconds.  Appends one JSON line to profiles/online_chains_native_bench.jsonl and prints it.
Usage: python scripts/bench_online_chains_native.py [--streams 64,256] [--seed 7] [--reps 4] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from se_snmf_nat_amd import Context  # noqa: E402
from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings, ntf_sep_event_rt_chains  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="64,256")
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_chains_native_bench.jsonl"))
a = ap.parse_args()

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
s0 = np.load(os.path.join(G, "frontend_audio.npz"))["samples"]
tiled = np.tile(s0, int(np.ceil((8 * 16000 + 16000) / len(s0))) + 1)
p = default_settings()
hop, tail = p["frameshift"], p["delay"] + 1
ctx = Context(0)


def files(n, seed):  # scripts/bench_online_chains.py's
    rs = np.random.RandomState(seed)
    lens = (rs.uniform(2.0, 8.0, n) * 16000).astype(int)
    return [tiled[(k * 997) % 16000:(k * 997) % 16000 + m] for k, m in enumerate(lens)]


def python_driver(ch, S):
    return ntf_sep_event_rt_chains(ch, Bx, Bd, p, n_streams=S, ctx=ctx)


def native_driver(ch, S):
    sep = OnlineBatchSeparator(Bx, Bd, p, S, ctx=ctx)
    try:
        return sep.run_chains(ch, Bd)
    finally:
        sep.close()


def schedule_steps(ch, S):
    """Device frame steps of the fixed-chunk schedule both drivers follow: per call the longest stream's frames."""
    step = max(1, min(4096, 16384 // S))
    queue = [c for c in range(len(ch)) if ch[c]][::-1]
    busy = {k: [queue.pop(), 0, 0] for k in range(min(S, len(queue)))}
    steps = 0
    while busy:
        longest = 0
        for k in list(busy):
            c, i, fed = busy[k]
            n = min(step * hop, len(ch[c][i]) - fed)
            busy[k][2] = fed = fed + n
            done = fed >= len(ch[c][i])
            longest = max(longest, (n + (fed - n) % hop) // hop + (tail if done else 0))
            if done:
                if i + 1 < len(ch[c]):
                    busy[k] = [c, i + 1, 0]
                elif queue:
                    busy[k] = [queue.pop(), 0, 0]
                else:
                    del busy[k]
        steps += longest
    return steps


def measure(ch, S):
    fl = [x for c in ch for x in c]
    real = sum(len(x) // hop for x in fl)
    sides = {"python": python_driver, "native": native_driver}
    secs = {k: [] for k in sides}
    ends = {}
    order = ["python", "native", "native", "python"] * ((a.reps + 1) // 2)
    for name in order[:2 * a.reps]:
        t = time.perf_counter()
        res = sides[name](ch, S)
        secs[name].append(time.perf_counter() - t)
        ends[name] = (res[0][0][0], res[-1][-1][0])
    same = all(np.array_equal(x, y) for x, y in zip(ends["python"], ends["native"]))
    out = {"slot_utilisation": round(real / (schedule_steps(ch, S) * S), 3), "outputs_equal": bool(same)}
    for name, v in secs.items():
        med = float(np.median(v))
        out[name] = {"files_per_s": round(len(fl) / med, 2), "frames_per_s": round(real / med, 1), "seconds": [round(x, 2) for x in v],
                     "spread": round((max(v) - min(v)) / med, 4)}
    out["native_over_python"] = round(float(np.median(secs["python"]) / np.median(secs["native"])), 4)
    return out


out = {"config": "C3 online separation, native chain driver (run_chains) vs the Python driver (ntf_sep_event_rt_chains), shipped "
                 "settings, adaptation on, 513 bins, r=200, files uniform in 2-8 s, alternating order, batch creation included",
       "unit": "files/s and real frames/s of the median run, seconds per run, spread = (max - min) / median, "
               "slot_utilisation = real frames / (frame steps x S) of the shared fixed-chunk schedule", "reps": a.reps}
for S in [int(x) for x in a.streams.split(",") if x]:
    warm = [x[:3200] for x in files(2, a.seed)]  # kernels loaded, chunk buffers of this S sized
    python_driver([warm] * S, S)
    native_driver([warm] * S, S)
    fi = files(6 * S, a.seed + S)
    f4 = files(4 * S, a.seed + 1000 + S)
    r = {"independent": measure([[x] for x in fi], S), "chains4": measure([f4[4 * c:4 * c + 4] for c in range(S)], S)}
    out[f"S={S}"] = r
    for k, v in r.items():
        print(f"# S={S} {k}: {v}", file=sys.stderr, flush=True)
line = json.dumps(out)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "a") as f:
    f.write(line + "\n")
print(line, flush=True)
