#!/usr/bin/env python3
"""BASELINE config 3 end to end: the online separation loop (src/NTF_sep_event_RT.m frame loop +
src/bnmf_sep_event_RT_IS16.m, shipped settings, noise-dictionary adaptation on) over the committed 1.2 s
audio fixture tiled to --seconds, shipped dictionaries.  Reports frames/s and the real-time factor
(10 ms hop), whole file in one process() call and hop-by-hop calls (real-time use), next to the CPU
oracle on a bounded sample.  One JSON line.  --precision fp64 runs the fp64 mode (OnlineSeparator(precision="fp64")).
--classes "1,41,71/1,51" (EVENT_RANK / NOISE_RANK) measures the per-class outputs instead: the same stream with
class_outputs=True, once with one class per side and once with the partition, in this process on this device; prints both
JSON lines (the second carries their ratio) and appends them to profiles/online_classes_bench.jsonl.
--precision fp64 --streams "1,16,64,256" measures the fp64 mode of the batched separator instead (OnlineBatchSeparator(precision="fp64")):
for every S, S copies of the stream with per-stream draws, adaptation as given by --no-adapt; beside each rate the fp32 batch
at the same S and the single-stream fp64 separator of the same build.  One JSON line per S, appended to
profiles/online_batch_f64_bench.jsonl.
Usage: python scripts/bench_online.py [--seconds 12] [--cpu] [--no-adapt] [--precision fp32|fp64] [--classes E/N] [--streams S,...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from se_snmf_nat_amd import Context  # noqa: E402
from se_snmf_nat_amd.online import OnlineBatchSeparator, OnlineSeparator, default_settings  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=12.0)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--no-adapt", action="store_true")
ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp32")
ap.add_argument("--classes", default=None, help='EVENT_RANK/NOISE_RANK, e.g. "1,41,71/1,51"')
ap.add_argument("--streams", default=None, help='with --precision fp64: stream counts of the batched separator, e.g. "1,16,64,256"')
a = ap.parse_args()

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
s = np.load(os.path.join(G, "frontend_audio.npz"))["samples"]
s = np.tile(s, int(np.ceil(a.seconds * 16000 / len(s))))[:int(a.seconds * 16000)]
p = default_settings()
if a.no_adapt:
    p["adapt_train_N"] = 0
rs = np.random.RandomState(1)
H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
ctx = Context(0)


def run(chunk, p=p, **kw):
    sep = OnlineSeparator(B[:, :100], B[:, 100:], p, H0=H0, Ad_blk0=Ad0, ctx=ctx, precision=a.precision, **kw)
    sep.process(s[:1600])  # warm-up: kernels loaded, buffers sized
    sep.close()
    sep = OnlineSeparator(B[:, :100], B[:, 100:], p, H0=H0, Ad_blk0=Ad0, ctx=ctx, precision=a.precision, **kw)
    t = time.perf_counter()
    if chunk is None:
        sep.process(s, flush=True)
    else:
        for i in range(0, len(s), chunk):
            sep.process(s[i:i + chunk])
        sep.process(s[:0], flush=True)
    dt = time.perf_counter() - t
    tr = sep.trace()
    sep.close()
    return dt, tr


def run_batch(S, precision):
    """S streams: the same samples, per-stream H0 / Ad_blk0 (so the streams' adaptation solves fall on different frames)."""
    rsb = np.random.RandomState(7)
    H0s = [H0] + [rsb.random_sample(200) for _ in range(S - 1)]
    Ads = [Ad0] + [rsb.random_sample((50, 100)) for _ in range(S - 1)]
    best, trs = np.inf, None
    for rep in range(3):  # the first repetition is the warm-up (kernels loaded, buffers sized); best of the other two
        sep = OnlineBatchSeparator(B[:, :100], B[:, 100:], p, S, H0=H0s, Ad_blk0=Ads, ctx=ctx, precision=precision)
        sep.process([s[:1600]] * S)
        sep.close()
        sep = OnlineBatchSeparator(B[:, :100], B[:, 100:], p, S, H0=H0s, Ad_blk0=Ads, ctx=ctx, precision=precision)
        t = time.perf_counter()
        sep.process([s] * S, flush=True)
        dt = time.perf_counter() - t
        trs = [sep.trace(k) for k in range(S)]
        sep.close()
        if rep:
            best = min(best, dt)
    return best, trs


if a.streams:
    if a.precision != "fp64":
        sys.exit("--streams measures the fp64 batch: add --precision fp64")
    dt1, tr1 = min((run(None) for _ in range(2)), key=lambda q: q[0])  # the single-stream fp64 separator, whole file per call
    single = len(tr1) / dt1
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for S in [int(v) for v in a.streams.split(",")]:
        dt64, trs = run_batch(S, "fp64")
        dt32, _ = run_batch(S, "fp32")
        nfr = sum(len(tr) for tr in trs)
        ln = {"config": "C3 online separation, fp64 batch, %d streams x %d frames%s" % (S, len(trs[0]), ", adaptation off" if a.no_adapt else ""),
              "streams": S, "adaptation": not a.no_adapt, "value": nfr / dt64, "unit": "frames/s (all streams, whole file per call)",
              "per_stream_frames_per_s": len(trs[0]) / dt64, "single_stream_fp64_frames_per_s": single,
              "per_stream_vs_single_stream_fp64": (len(trs[0]) / dt64) / single, "aggregate_vs_single_stream_fp64": (nfr / dt64) / single,
              "fp32_batch_frames_per_s": nfr / dt32, "fp64_vs_fp32_batch": dt32 / dt64,
              "adaptation_solves": int(sum(t["solved"] for tr in trs for t in tr)),
              "adaptation_iters_mean": float(np.mean([t["adapt_iters"] for tr in trs for t in tr if t["solved"]] or [0]))}
        print(json.dumps(ln), flush=True)
        with open(os.path.join(ROOT, "profiles", "online_batch_f64_bench.jsonl"), "a") as f:
            f.write(json.dumps(ln) + "\n")
    sys.exit(0)

if a.classes:
    ev, nz = ([int(v) for v in part.split(",")] for part in a.classes.split("/"))
    lines = []
    for label, q in (("one class per side", dict(p, EVENT_NUM=1, EVENT_RANK=[1], NOISE_NUM=1, NOISE_RANK=[1])),
                     ("EVENT_RANK=%s NOISE_RANK=%s" % (ev, nz), dict(p, EVENT_NUM=len(ev), EVENT_RANK=ev, NOISE_NUM=len(nz), NOISE_RANK=nz))):
        best_file, best_hop, tr = np.inf, np.inf, None
        for _ in range(3):  # best of three: the loop is latency-bound and the host shares its cores
            dt, tr = run(None, q, class_outputs=True)
            best_file = min(best_file, dt)
            best_hop = min(best_hop, run(160, q, class_outputs=True)[0])
        lines.append({"config": "C3 online separation, class_outputs=True, %s%s, %d frames" % (label, ", adaptation off" if a.no_adapt else "", len(tr)),
                      "precision": a.precision, "classes": label, "value": len(tr) / best_file, "unit": "frames/s (whole file per call)",
                      "hop_by_hop_frames_per_s": len(tr) / best_hop, "adaptation_solves": int(sum(t["solved"] for t in tr))})
    lines[1]["ratio_to_one_class_per_side"] = lines[1]["value"] / lines[0]["value"]
    lines[1]["hop_by_hop_ratio"] = lines[1]["hop_by_hop_frames_per_s"] / lines[0]["hop_by_hop_frames_per_s"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "online_classes_bench.jsonl"), "a") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")
    sys.exit(0)

dt_file, tr = run(None)
dt_hop, _ = run(160)
nfr = len(tr)
out = {"config": "C3 online separation end to end (bnmf_sep_event_RT_IS16, shipped settings%s), 513 bins, r=200, %d frames"
                 % (", adaptation off" if a.no_adapt else "", nfr),
       "precision": a.precision, "value": nfr / dt_file, "unit": "frames/s (whole file per call)", "realtime_factor": (nfr * 0.010) / dt_file,
       "hop_by_hop_frames_per_s": nfr / dt_hop, "hop_by_hop_ms_per_frame": dt_hop / nfr * 1e3,
       "frame_solve_iters_mean": float(np.mean([t["n_iter"] for t in tr])),
       "adaptation_solves": int(sum(t["solved"] for t in tr)),
       "adaptation_iters_mean": float(np.mean([t["adapt_iters"] for t in tr if t["solved"]] or [0]))}
if a.cpu:
    from oracle.online_oracle import default_params, ntf_sep_event_rt
    po = default_params()
    if a.no_adapt:
        po["adapt_train_N"] = 0
    n = 160 * 200
    t = time.perf_counter()
    _, _, _, tro = ntf_sep_event_rt(s[:n], B[:, :100], B[:, 100:], po, H0, Ad0, return_trace=True)
    dtc = time.perf_counter() - t
    out["cpu_oracle_frames_per_s"] = len(tro) / dtc
    out["cpu_oracle_sample"] = "first %d frames, fp64 NumPy oracle, %s host threads" % (len(tro), os.cpu_count())
print(json.dumps(out), flush=True)
