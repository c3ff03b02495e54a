#!/usr/bin/env python3
"""Bits of the online separators on the 124-frame fixture (shipped settings, adaptation on), dumped to an .npz: every path
of the single-stream separator that runs through its host driver (csrc/snmf_online_host.h) in both modes --
  single_f64                   the fp64 separator (the four arrays this script has always written)
  one_f32 / one_f64            default settings
  one_f32_fixed / one_f64_fixed  adapt_train_N = 0: all frame solves of a call in one launch
  one_f32_semi                 basis_update_N = 1: the semi-supervised frame solve
  one_f32_mel1 / one_f32_mel0  B_sep_mode 'Mel' with MelConv 1 and 0
  one_f32_co                   class_outputs without a partition
  one_f32_cls / one_f64_cls    class_outputs with the 2 + 2 class partition
  one_f32_fed<n>               the partition run fed in 160- / 1000- / 57-sample pieces, the flush in a call of its own
  one_f32_big                  R_x = R_d = 500 over 20 hops: the frame solve through the plan loop
-- per group x_tilde_f, the int16 stream, with class_outputs x_hat, d_hat and the class signals, the final B_DFT_d (Mel: and
B_Mel_d) and every field of the trace; and every path of the batched separator that runs through its host driver
(csrc/snmf_online_batch_host.h) in both modes --
  batch_f32 / batch_f64        three heterogeneous streams (the fixture is stream 1), class_outputs, fp64 with a class partition
  batch_f32_cls                the fp32 batch with the class partition
  mel0 / mel1                  the fp32 Mel batch with MelConv 0 and 1
  chains_f32 / chains_f64      ntf_sep_event_rt_chains: 3 chains on 2 slots (restarts on used slots), one carry, one empty file
  fed_f32 / fed_f64            the three streams fed in 160- / 1000- / 57-sample pieces, the flush in a call of its own
  cross_f32 / cross_f64        one call across device chunks (tests/test_online_batch_chunks.py): S = 140, and S = 34 with 4 classes
  set_f64                      the fp64 batch with settings per stream: beta_div 1, 2 and 0.5, all three adapting
  rs_f32 / rs_f64              restarts onto used slots: stream 0 with a new B_DFT_d / H0 / Ad_blk0, stream 2 as a carry
  rs_mel                       the Mel batch (MelConv 0): stream 0 restarts with a new B_Mel_d, stream 2 as a carry
  state_f32 / state_f64        the raw bytes of get_state for stream 1 after 557 samples (tests/test_gpu_online_batch_state.py)
-- per stream x_tilde_f, the int16 stream, x_hat, d_hat, the class signals, the final B_DFT_d (Mel: and B_Mel_d) and the
trace's adapt_iters / n_iter / trig; the chains groups hold per file what ntf_sep_event_rt_chains returns (the int16 stream,
x_tilde_f and the final B_DFT_d: it hands out no trace, x_hat or d_hat).
A change that must not move these separators' bits is checked by dumping once per build and comparing the two files;
SNMF_PACKAGE_ROOT names the directory that holds the other build's se_snmf_nat_amd package (its
Python and its libsnmf_hip.so; the fixtures are read from this checkout):
    SNMF_PACKAGE_ROOT=/path/to/parent python scripts/online_bits_dump.py parent.npz
    python scripts/online_bits_dump.py new.npz
    python scripts/online_bits_dump.py --compare parent.npz new.npz      (exit status 1 on any differing array)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SNMF_PACKAGE_ROOT") or ROOT)
import numpy as np  # noqa: E402

if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k], equal_nan=True)]
    for k in a.files:
        print("%-32s %-8s %-14s %s" % (k, a[k].dtype, a[k].shape, "DIFFERS" if k in bad else "bit-identical"))
    print("%d arrays, %d differ" % (len(a.files), len(bad)))
    sys.exit(1 if bad or set(a.files) != set(b.files) else 0)
if len(sys.argv) != 2:
    sys.exit(__doc__)

from se_snmf_nat_amd import Context  # noqa: E402
from se_snmf_nat_amd.frontend import mel_matrix  # noqa: E402
from se_snmf_nat_amd.online import OnlineBatchSeparator, OnlineSeparator, default_settings, ntf_sep_event_rt_chains  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
s = np.load(os.path.join(G, "frontend_audio.npz"))["samples"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
rs = np.random.RandomState(1)
H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
p = default_settings()
CLS = dict(EVENT_NUM=2, EVENT_RANK=[1, 51], NOISE_NUM=2, NOISE_RANK=[1, 51])
ctx = Context(0)
out = {}
sep = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, precision="fp64")
o = sep.process(s, flush=True)
out.update(single_f64_x_tilde_f=o["x_tilde_f"], single_f64_i16=o["x_tilde"], single_f64_basis=sep.basis_f64(),
           single_f64_adapt_iters=np.array([t["adapt_iters"] for t in sep.trace()]))
sep.close()


def one(tag, p=p, precision="fp32", pieces=None, x=s, dicts=(Bx, Bd), draws=(H0, Ad0), **kw):
    """One single-stream separator on `x`: in one call with the flush, or in `pieces`-sample calls and the flush on its own."""
    sep = OnlineSeparator(dicts[0], dicts[1], p, H0=draws[0], Ad_blk0=draws[1], ctx=ctx, precision=precision, **kw)
    if pieces is None:
        parts = [sep.process(x, flush=True)]
    else:
        parts = [sep.process(x[i:i + pieces]) for i in range(0, len(x), pieces)] + [sep.process(x[:0], flush=True)]
    for key in parts[0]:
        out["%s_%s" % (tag, key)] = np.concatenate([q[key] for q in parts], axis=-1)
    out[tag + "_basis"] = sep.basis_f64()
    if sep.mel:
        out[tag + "_mel_basis"] = sep.mel_basis()
    tr = sep.trace()
    for key in tr[0]:
        out["%s_tr_%s" % (tag, key)] = np.array([t[key] for t in tr])
    sep.close()


mm = mel_matrix(p["fs"], 64, p["fftlength"], 1.0, p["fs"] / 2).T
BM = mm @ B
BM = BM / np.sqrt((BM ** 2).sum(0)) + 1e-9  # the stored form of run_basis_train.m:115-116
one("one_f32")
one("one_f32_fixed", p=dict(p, adapt_train_N=0), class_outputs=True)
one("one_f32_semi", p=dict(p, basis_update_N=1), class_outputs=True)
for conv in (1, 0):
    one("one_f32_mel%d" % conv, p=dict(p, B_sep_mode="Mel", MelConv=conv, F_order=64), class_outputs=True, B_Mel_x=BM[:, :100],
        B_Mel_d=BM[:, 100:])
one("one_f32_co", class_outputs=True)
one("one_f32_cls", p=dict(p, **CLS), class_outputs=True)
for n in (160, 1000, 57):
    one("one_f32_fed%d" % n, p=dict(p, **CLS), class_outputs=True, pieces=n)
rs = np.random.RandomState(1024)  # tests/test_online.py: the exemplar geometry's dictionaries
Bbig = rs.gamma(0.6, 1.0, (513, 1000)) + 1e-3
Bbig = Bbig / np.sqrt((Bbig ** 2).sum(0)) + 1e-9
rs = np.random.RandomState(7)
one("one_f32_big", x=s[:20 * 160], dicts=(Bbig[:, :500], Bbig[:, 500:]), draws=(rs.random_sample(1000), rs.random_sample((50, 100))))
one("one_f64", precision="fp64")
one("one_f64_fixed", p=dict(p, adapt_train_N=0), precision="fp64", class_outputs=True)
one("one_f64_cls", p=dict(p, **CLS), precision="fp64", class_outputs=True)
assert all(out["one_%s_tr_solved" % t].sum() > 0 for t in ("f32", "f32_mel1", "f32_mel0", "f32_cls", "f32_fed57", "f64", "f64_cls"))
assert not out["one_f32_fixed_tr_solved"].any() and out["one_f32_cls_x_hat_i"].shape[0] == 2
rs = np.random.RandomState(5)
pcms = [np.round(s[1733:1733 + 40 * 160] * 0.75 + rs.randn(40 * 160) * 30.0), s, np.round(s[:30 * 160 + 57] * 0.5)]
Bds = [Bd[:, rs.permutation(100)], Bd, Bd * (1.0 + 0.05 * rs.random_sample(Bd.shape))]
H0s, Ads = [rs.random_sample(200), H0, rs.random_sample(200)], [rs.random_sample((50, 100)), Ad0, rs.random_sample((50, 100))]
short = (np.round(s[1733:1733 + 5 * 160] * 0.75), Bd, rs.random_sample(200), rs.random_sample((50, 100)))


def batch(tag, pcms, Bds, H0s, Ads, p=p, precision="fp32", feed=None, keep=None, then=None, **kw):
    """One batch: `feed` is a list of (pcm list, flush) calls (default: everything in one call, with the flush); dumps the
    streams `keep` (default: all) as <tag>_s<k>_<array>.  `then(sep)` runs behind the feed and returns a second feed, whose
    outputs are dumped in the place of the first one's."""
    S = len(pcms)
    sep = OnlineBatchSeparator(Bx, Bds, p, S, H0=H0s, Ad_blk0=Ads, ctx=ctx, class_outputs=True, precision=precision, **kw)

    def run(calls):
        parts = [{} for _ in range(S)]
        for xs, fl in calls:
            for k, o in enumerate(sep.process(xs, flush=fl)):
                for key, v in o.items():
                    parts[k].setdefault(key, []).append(v)
        return parts

    parts = run(feed or [(pcms, True)])
    if then is not None:
        parts = run(then(sep))
    for k in (range(S) if keep is None else keep):
        for key, v in parts[k].items():
            out["%s_s%d_%s" % (tag, k, key)] = np.concatenate(v, axis=-1)
        out["%s_s%d_basis" % (tag, k)] = sep.basis_f64(k)
        if sep.mel:
            out["%s_s%d_mel_basis" % (tag, k)] = sep.mel_basis_f64(k)
        tr = sep.trace(k)
        for key in ("adapt_iters", "n_iter", "trig"):
            out["%s_s%d_%s" % (tag, k, key)] = np.array([t[key] for t in tr])
    sep.close()


batch("batch_f32", pcms, Bds, H0s, Ads)
out.update(batch_f32_x_tilde_f=out["batch_f32_s1_x_tilde_f"], batch_f32_i16=out["batch_f32_s1_x_tilde"], batch_f32_basis=out["batch_f32_s1_basis"],
           batch_f32_adapt_iters=out["batch_f32_s1_adapt_iters"])  # (the names this script has always written)
batch("batch_f32_cls", pcms, Bds, H0s, Ads, p=dict(p, **CLS))
batch("batch_f64", pcms, Bds, H0s, Ads, p=dict(p, **CLS), precision="fp64")
for conv in (0, 1):
    batch("mel%d" % conv, pcms, Bds, H0s, Ads, p=dict(p, B_sep_mode="Mel", MelConv=conv, F_order=64), B_Mel_x=BM[:, :100],
          B_Mel_d=[BM[:, 100:], BM[:, 100:] * 1.01, BM[:, 100:]])
# chains: 3 chains on 2 slots, so a used slot restarts with a fresh dictionary; chain 0 carries its dictionary over an empty
# file into a third one
chains = [[pcms[0], s[:0], pcms[2]], [pcms[1][:50 * 160]], [pcms[2], pcms[0][:20 * 160 + 31]]]
for prec in ("fp32", "fp64"):
    res = ntf_sep_event_rt_chains(chains, Bx, Bds, p, n_streams=2, H0=H0s, Ad_blk0=Ads, ctx=ctx, chunk_hops=16, precision=prec)
    for c, files in enumerate(res):
        for i, (o16, of, Bn) in enumerate(files):
            tag = "chains_f%s_c%d_f%d" % (prec[2:], c, i)
            out.update({tag + "_i16": o16, tag + "_x_tilde_f": of, tag + "_basis": Bn})
# 160- / 1000- / 57-sample pieces (some streams get nothing in some calls), then the flush in a call of its own
sizes, pos, feed, rnd = [160, 1000, 57], [0, 0, 0], [], 0
while any(pos[k] < len(pcms[k]) for k in range(3)):
    piece = []
    for k in range(3):
        if (rnd + k) % 4 == 3:
            piece.append(pcms[k][:0])
            continue
        piece.append(pcms[k][pos[k]:pos[k] + sizes[k]])
        pos[k] += sizes[k]
    feed.append((piece, False))
    rnd += 1
feed.append(([x[:0] for x in pcms], True))
batch("fed_f32", pcms, Bds, H0s, Ads, feed=feed)
batch("fed_f64", pcms, Bds, H0s, Ads, precision="fp64", feed=feed)
# one call across device chunks: the fixture on the three start dictionaries in wide batches, 5 hops on every other stream
for tag, prec, S, slots, q in (("cross_f32", "fp32", 140, (0, 69, 139), p), ("cross_f64", "fp64", 34, (0, 16, 33), dict(p, **CLS))):
    where = {slot: j for j, slot in enumerate(slots)}
    pick = lambda long_ones, the_short: [long_ones[where[k]] if k in where else the_short for k in range(S)]  # noqa: E731
    batch(tag, pick([s] * 3, short[0]), pick(Bds, short[1]), pick(H0s, short[2]), pick(Ads, short[3]), p=q, precision=prec,
          keep=list(slots) + [1, S - 2])
# settings per stream: every instantiation of the fp64 adaptation kernel, and the restart's per-stream "this stream adapts"
batch("set_f64", pcms, Bds, H0s, Ads, precision="fp64", settings=[dict(cf="kl"), dict(cf="ed"), dict(cf="beta", beta_div=0.5)])
# restarts onto used slots behind a whole recording: stream 0 with new arrays, stream 2 as a carry (all None), stream 1 left
# flushed; the two then run each other's recording
rs_new = np.random.RandomState(11)
newB, newH, newA = Bds[2][:, rs_new.permutation(100)], rs_new.random_sample(200), rs_new.random_sample((50, 100))
none = pcms[0][:0]


def restarts(mel_d=None):
    def then(sep):
        sep.restart(0, B_DFT_d=None if mel_d is not None else newB, H0=newH, Ad_blk0=newA, B_Mel_d=mel_d)
        sep.restart(2)
        return [([pcms[2], none, pcms[0]], [True, False, True])]
    return then


batch("rs_f32", pcms, Bds, H0s, Ads, then=restarts(), keep=(0, 2))
batch("rs_f64", pcms, Bds, H0s, Ads, precision="fp64", then=restarts(), keep=(0, 2))
batch("rs_mel", pcms, Bds, H0s, Ads, p=dict(p, B_sep_mode="Mel", MelConv=0, F_order=64), B_Mel_x=BM[:, :100],
      B_Mel_d=[BM[:, 100:], BM[:, 100:] * 1.01, BM[:, 100:]], then=restarts(BM[:, 100:][:, rs_new.permutation(100)]), keep=(0, 2))
# a stream's state g as raw bytes, mid-recording and mid-hop
for prec in ("fp32", "fp64"):
    sep = OnlineBatchSeparator(Bx, Bds, dict(p, **CLS), 3, H0=H0s, Ad_blk0=Ads, ctx=ctx, class_outputs=True, precision=prec)
    sep.process([x[:557] for x in pcms])
    out["state_f%s_record" % prec[2:]] = np.frombuffer(sep.get_state(1)["record"], dtype=np.uint8)
    sep.close()
assert all(out["%s_s%d_adapt_iters" % (t, k)].max() > 0 for t in ("set_f64", "rs_f32", "rs_f64", "rs_mel") for k in (0, 2))
assert out["single_f64_adapt_iters"].max() > 0 and out["batch_f32_adapt_iters"].max() > 0  # the adaptation ran
assert all(out["%s_s1_adapt_iters" % t].max() > 0 for t in ("batch_f64", "batch_f32_cls", "mel0", "mel1", "fed_f32", "fed_f64"))
np.savez(sys.argv[1], **out)
print("wrote %s: %d arrays" % (sys.argv[1], len(out)))
