#!/usr/bin/env python3
"""The batched online separator (OnlineBatchSeparator, include/snmf.h: snmf_online_batch_*) on bench_online.py's fixture:
the committed 1.2 s audio tiled, the shipped dictionaries, adaptation on.  Stream k reads the tiled signal from its own
offset and has its own H0 / Ad_blk0 (RandomState(1 + k)).  Reports aggregate frames/s for whole-file calls at several
S, ms per call for hop-by-hop calls (one 160-sample hop per stream per call, as live microphones feed it), and the
single-stream OnlineSeparator figure of the same process.  One JSON line.
--mel: B_sep_mode = 'Mel' instead (F_order = 64, MelConv = 1), two configurations, each with its single-stream figure:
the shipped settings with adaptation on (Mel dictionaries = melmat * the shipped ones, unit columns), and the reference's
Mel setting settings/bak_IS16_results/initial_setting_IMCRA.m (R_x = R_d = 50 of the shipped B_Mel_sub / B_DFT_sub,
adaptation off, max_iter = 25).  One JSON line per configuration.
Usage: python scripts/bench_online_batch.py [--seconds 4] [--streams 1,8,32,64,128,256,512] [--hop-streams 1,64,256] [--mel]"""
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
ap.add_argument("--seconds", type=float, default=4.0)
ap.add_argument("--streams", default="1,8,32,64,128,256,512")
ap.add_argument("--hop-streams", default="1,64,256")
ap.add_argument("--hop-calls", type=int, default=100)
ap.add_argument("--mel", action="store_true")
a = ap.parse_args()

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
s0 = np.load(os.path.join(G, "frontend_audio.npz"))["samples"]
n = int(a.seconds * 16000)
tiled = np.tile(s0, int(np.ceil((n + 16000) / len(s0))) + 1)
p = default_settings()
ctx = Context(0)
MEL = {}  # OnlineSeparator / OnlineBatchSeparator keyword arguments of the current configuration (Mel mode)
R, RA, MA = 200, 50, 100  # rank, R_a x m_a of the draws


def stream(k, length):
    off = (k * 997) % 16000
    return tiled[off:off + length]


def draws(S):
    H, A = [], []
    for k in range(S):
        rs = np.random.RandomState(1 + k)
        H.append(rs.random_sample(R))
        A.append(rs.random_sample((RA, MA)))
    return H, A


def single():
    rs = np.random.RandomState(1)
    H0, Ad0 = rs.random_sample(R), rs.random_sample((RA, MA))
    x = stream(0, n)
    w = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, **MEL)
    w.process(x[:1600])
    w.close()
    sep = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, **MEL)
    t = time.perf_counter()
    sep.process(x, flush=True)
    dt = time.perf_counter() - t
    nfr = len(sep.trace())
    sep.close()
    return nfr / dt


def whole(S):
    H, A = draws(S)
    xs = [stream(k, n) for k in range(S)]
    w = OnlineBatchSeparator(Bx, Bd, p, S, H0=H, Ad_blk0=A, ctx=ctx, **MEL)
    w.process([x[:1600] for x in xs])  # warm-up: kernels loaded, buffers sized
    w.close()
    sep = OnlineBatchSeparator(Bx, Bd, p, S, H0=H, Ad_blk0=A, ctx=ctx, **MEL)
    t = time.perf_counter()
    sep.process(xs, flush=True)
    dt = time.perf_counter() - t
    nfr = sum(len(sep.trace(k)) for k in range(S))
    solved = sum(t["solved"] for t in sep.trace(0))
    sep.close()
    return nfr / dt, solved


def hop_by_hop(S):
    H, A = draws(S)
    xs = [stream(k, 160 * (a.hop_calls + 10)) for k in range(S)]
    sep = OnlineBatchSeparator(Bx, Bd, p, S, H0=H, Ad_blk0=A, ctx=ctx, **MEL)
    for i in range(10):  # warm-up
        sep.process([x[i * 160:(i + 1) * 160] for x in xs])
    t = time.perf_counter()
    for i in range(10, 10 + a.hop_calls):
        sep.process([x[i * 160:(i + 1) * 160] for x in xs])
    dt = time.perf_counter() - t
    sep.close()
    return dt / a.hop_calls * 1e3


def run(config):
    one = single()
    agg = {}
    for S in [int(x) for x in a.streams.split(",") if x]:
        fps, solved = whole(S)
        agg[str(S)] = round(fps, 1)
        print(f"# S={S}: {fps:.0f} frames/s aggregate ({fps / one:.1f}x single; stream 0 ran {solved} adaptation solves)", file=sys.stderr,
              flush=True)
    hop = {}
    for S in [int(x) for x in a.hop_streams.split(",") if x]:
        hop[str(S)] = round(hop_by_hop(S), 3)
        print(f"# hop-by-hop S={S}: {hop[str(S)]:.2f} ms per call", file=sys.stderr, flush=True)
    out = {"config": config % a.seconds, "single_stream_frames_per_s": round(one, 1), "aggregate_frames_per_s": agg,
           "speedup_vs_single": {k: round(v / one, 2) for k, v in agg.items()},
           "hop_by_hop_ms_per_call": hop, "unit": "frames/s (whole file per call), ms per call (one hop per stream)"}
    print(json.dumps(out), flush=True)


if not a.mel:
    run("C3 online separation, batched streams (shipped settings, adaptation on), 513 bins, r=200, %.1f s per stream")
else:
    from se_snmf_nat_amd.frontend import mel_matrix
    from se_snmf_nat_amd.train import load_basis_mat
    mm = mel_matrix(p["fs"], 64, p["fftlength"], 1.0, p["fs"] / 2).T
    BM = mm @ B
    BM = BM / np.sqrt((BM ** 2).sum(0)) + 1e-9  # the stored form of run_basis_train.m:115-116
    p = dict(default_settings(), B_sep_mode="Mel", MelConv=1, F_order=64)
    MEL.update(B_Mel_x=BM[:, :100], B_Mel_d=BM[:, 100:])
    run("C3 online separation, batched streams, Mel mode (F_order 64, MelConv 1; shipped settings, adaptation on), r=200, "
        "%.1f s per stream")
    sp = load_basis_mat(os.path.join(G, "ref_basis", "R_100_Clean_train_TIMIT_test.mat"))
    nz = load_basis_mat(os.path.join(G, "ref_basis", "R_100_CHiME3_bgn_ch6.mat"))
    Bx, Bd = sp["B_DFT_sub"][:, :50], nz["B_DFT_sub"][:, :50]
    MEL.update(B_Mel_x=sp["B_Mel_sub"][:, :50], B_Mel_d=nz["B_Mel_sub"][:, :50])
    p = dict(default_settings(), B_sep_mode="Mel", MelConv=1, F_order=64, adapt_train_N=0, init_N_len=10, m_a=40, overlap_m_a=0.5,
             blk_sparse=0, P_len_k=50, P_len_l=3, max_iter=25, conv_eps=1e-3, DCbin=10, DCbin_back=10)
    R, RA, MA = 100, 1, 1
    run("C3 online separation, batched streams, Mel mode, initial_setting_IMCRA.m (F_order 64, MelConv 1, R_x = R_d = 50, "
        "adaptation off, max_iter 25), %.1f s per stream")
