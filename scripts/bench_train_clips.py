"""Basis training from clips: the device-side assembly against the host-side one (run on the GPU box; a script, not a test; fails
without a GPU).

Workload: B in {8, 64} classes, each a 12-min training signal at 16 kHz built from 1-min int16 clips (the shipped limits:
train_seq_len_max 12 min, train_file_len_max 1 min), VAD on and off, F = 257 (fftlength 512, frameshift 160), R = 40, F_order = 64,
KL, sparsity 5, 10 iterations per solve, H0 drawn on the device, both precisions.  Two legs:
    (a) today's way   the NumPy assembly (the line-by-line restatement of run_basis_train.m:16-57 in tests/assemble_cases.py, timed
                      on the host) plus run_basis_train_signal_batch on its doubles;
    (b) the new way   run_basis_train_clips_batch on the int16 clips.
Without VAD a class has 13 clips of 1 000 000 samples (each cut to 1 min; 12 reach the limit exactly, so the 13th is read and cut
away); with VAD it has 25 clips of which about half of every one is voiced (23 are consumed).  The clips of a class are drawn from a pool of 14
distinct ones, rotated per class.  The measurement of one (B, VAD) is a process of its own (this script started again with --one,
under a time limit): a warm-up of the device legs, then per repetition the NumPy assembly once and, per precision, leg (a)'s
training call and leg (b) in turn.  Leg (a)'s whole call is the NumPy assembly of that repetition plus its training call.
The assembly alone is measured on a call of assemble_training_signals: the host wall time, and the device time of its ten launches
from events around them (snmf_ctx_timing, family "assemble").  The device's lengths and clips_used must equal the restatement's,
and class 0 must agree within 1e-12 * 30000.  One JSON line per (B, VAD) goes to profiles/train_clips_bench.jsonl (or --out); no
ratio is expected in advance.

    python scripts/bench_train_clips.py [--out FILE] [--B 8,64] [--reps 2] [--limit SECONDS]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000
SHAPE = dict(fftlength=512, framelength=400, frameshift=160, R=40, F_order=64, iters=10)
SEQ, FILE = 12 * 60 * FS, 60 * FS
POOL = 14


def make_pool(vad, rs):
    """POOL int16 clips of 1 000 000 samples.  VAD: a background in +-12 with loud stretches in +-9000 of 0.2 - 1 s, about half
    of the clip, and exact zeros inside them; else +-9000 throughout."""
    n = 1_000_000
    out = []
    for _ in range(POOL):
        if not vad:
            out.append(rs.integers(-9000, 9001, size=n, dtype=np.int16))
            continue
        c = rs.integers(-12, 13, size=n, dtype=np.int16)
        at = FS  # (the first second is background: bg_len is 50 ms)
        while at < n:
            L = int(rs.integers(FS // 5, FS))
            c[at:at + L] = rs.integers(-9000, 9001, size=min(L, n - at), dtype=np.int16)
            c[at + L // 3:at + L // 3 + 1] = 0
            at += L + int(rs.integers(FS // 5, FS))
        out.append(c)
    return out


def one(B, vad, reps):
    """The record of one (B, VAD), measured in this process."""
    import assemble_cases as ac
    from se_snmf_nat_amd import Context, _lib, assemble_training_signals, frontend, train
    if _lib.load().snmf_device_count() < 1:
        raise SystemExit("bench_train_clips: no HIP device is visible (there is no CPU path to fall back to)")
    ctx = Context(0)
    N, fl, shift, R, M, iters = (SHAPE[k] for k in ("fftlength", "framelength", "frameshift", "R", "F_order", "iters"))
    p = dict(frontend.default_params(), fs=FS, fftlength=N, framelength=fl, frameshift=shift, DCbin=1, F_order=M,
             win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(fl) / fl)), cf="kl", sparsity=5.0, max_iter=iters, conv_eps=0.0,
             cost_check=1, cluster_buff=1, train_Exemplar=0, random_seed=1, train_seq_len_max=SEQ, train_file_len_max=FILE)
    pool = make_pool(vad, np.random.default_rng(1))
    per = 25 if vad else 13
    classes = [[pool[(k + i) % POOL] for i in range(per)] for k in range(B)]
    vads = [bool(vad)] * B
    kw = dict(h0="device")

    def numpy_assembly():
        t0 = time.perf_counter()
        out = [ac.assemble_class(cl, 1 if vad else 0, None, FS, SEQ, FILE) for cl in classes]
        return time.perf_counter() - t0, out

    def leg_a_train(sigs, precision):
        t0 = time.perf_counter()
        info = {}
        out = train.run_basis_train_signal_batch(sigs, R, p, ctx=ctx, precision=precision, info=info, **kw)
        ctx.sync()
        return time.perf_counter() - t0, out, info

    def leg_b(precision):
        t0 = time.perf_counter()
        info = {}
        out = train.run_basis_train_clips_batch(classes, R, p, vad=vads, ctx=ctx, precision=precision, info=info, **kw)
        ctx.sync()
        return time.perf_counter() - t0, out, info

    def assembly_alone():
        ctx.timing(True)
        t0 = time.perf_counter()
        ts = assemble_training_signals(classes, p, vad=vads, ctx=ctx)
        wall = time.perf_counter() - t0
        ms, n = ctx.timing_get("assemble")
        ctx.timing(False)
        return wall, ms, n, ts

    # warm-up: the device legs on the first two classes (code objects, the transfer pipeline), then the assembly alone at full size
    for precision in ("fp32", "fp64"):
        train.run_basis_train_clips_batch(classes[:2], R, p, vad=vads[:2], ctx=ctx, precision=precision, **kw)
    assembly_alone()[3].close()
    t_np, t_a, t_b, t_asm_wall, t_asm_dev = [], {"fp32": [], "fp64": []}, {"fp32": [], "fp64": []}, [], []
    check = {}
    for _ in range(reps):
        tn, ref = numpy_assembly()
        t_np.append(tn)
        sigs = [s for s, _, _ in ref]
        wall, ms, n_launch_groups, ts = assembly_alone()
        t_asm_wall.append(wall), t_asm_dev.append(ms * 1e-3)
        assert n_launch_groups == 1
        assert ts.lengths == [len(s) for s in sigs] and ts.clips_used == [u for _, u, _ in ref]
        check = dict(lengths=ts.lengths[:2], clips_used=ts.clips_used[:2], class0_max_abs_diff=float(np.abs(ts.signal(0) - sigs[0]).max()))
        assert check["class0_max_abs_diff"] <= ac.TOL
        ts.close()
        for precision in ("fp32", "fp64"):
            ta, oa, ia = leg_a_train(sigs, precision)
            tb, ob, ib = leg_b(precision)
            t_a[precision].append(tn + ta), t_b[precision].append(tb)
            assert ia["T"] == ib["T"] and ia["n_iter"] == ib["n_iter"]
            del oa, ob
        del sigs, ref
    med = lambda v: float(np.median(v))  # noqa: E731
    rec = dict(B=B, vad=bool(vad), reps=reps, clips_per_class=per, clip_samples=1_000_000, fs=FS, seq_len_max=SEQ, file_len_max=FILE,
               F=N // 2 + 1, R=R, F_order=M, iters=iters, frameshift=shift, T=ib["T"][:2],
               numpy_assembly_s=t_np, device_assembly_wall_s=t_asm_wall, device_assembly_launches_s=t_asm_dev,
               numpy_over_device_assembly_wall=med(t_np) / med(t_asm_wall), check=check)
    for precision in ("fp32", "fp64"):
        rec[precision] = dict(a_numpy_plus_signal_batch_s=t_a[precision], b_clips_batch_s=t_b[precision],
                              a_over_b=med(t_a[precision]) / med(t_b[precision]),
                              a_over_b_worst=min(t_a[precision]) / max(t_b[precision]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_clips_bench.jsonl"))
    ap.add_argument("--B", default="8,64")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=600, help="seconds one (B, VAD) may take")
    ap.add_argument("--one", default=None, help="B,VAD: measure this one here and print its JSON line")
    a = ap.parse_args()
    if a.one:
        B, vad = a.one.split(",")
        print(json.dumps(one(int(B), int(vad), a.reps)), flush=True)
        return
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for B in a.B.split(","):
        for vad in (1, 0):  # each GPU step is a fresh process under its own time limit; a failed one ends the script
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", f"{B},{vad}", "--reps", str(a.reps)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if res.returncode != 0:
                raise SystemExit(f"bench_train_clips: B={B} vad={vad} ended with status {res.returncode}; nothing more is started")
            line = res.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            lines.append(json.loads(line))
            with open(a.out, "w") as f:  # (rewritten after every step: what was measured is kept)
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
