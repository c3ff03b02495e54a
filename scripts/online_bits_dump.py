#!/usr/bin/env python3
"""Bits of the online separators on the 124-frame fixture (shipped settings, adaptation on): the single-stream fp64
separator and the fp32 batch (the fixture as stream 1 of 3), dumped to an .npz -- x_tilde_f, the int16 stream and the final
B_DFT_d of each.  A change that must not move these separators' bits is checked by dumping once per build and comparing the
two files; SNMF_PACKAGE_ROOT names the directory that holds the other build's se_snmf_nat_amd package (its Python and its
libsnmf_hip.so; the fixtures are read from this checkout):
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
        print("%-24s %-8s %-14s %s" % (k, a[k].dtype, a[k].shape, "DIFFERS" if k in bad else "bit-identical"))
    sys.exit(1 if bad or set(a.files) != set(b.files) else 0)
if len(sys.argv) != 2:
    sys.exit(__doc__)

from se_snmf_nat_amd import Context  # noqa: E402
from se_snmf_nat_amd.online import OnlineBatchSeparator, OnlineSeparator, default_settings  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
B = np.load(os.path.join(G, "ref_data.npz"))["B"].astype(np.float64)
s = np.load(os.path.join(G, "frontend_audio.npz"))["samples"].astype(np.float64)
Bx, Bd = B[:, :100], B[:, 100:]
rs = np.random.RandomState(1)
H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
p = default_settings()
ctx = Context(0)
out = {}
sep = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, precision="fp64")
o = sep.process(s, flush=True)
out.update(single_f64_x_tilde_f=o["x_tilde_f"], single_f64_i16=o["x_tilde"], single_f64_basis=sep.basis_f64(),
           single_f64_adapt_iters=np.array([t["adapt_iters"] for t in sep.trace()]))
sep.close()
rs = np.random.RandomState(5)
pcms = [np.round(s[1733:1733 + 40 * 160] * 0.75 + rs.randn(40 * 160) * 30.0), s, np.round(s[:30 * 160 + 57] * 0.5)]
Bds = [Bd[:, rs.permutation(100)], Bd, Bd * (1.0 + 0.05 * rs.random_sample(Bd.shape))]
H0s, Ads = [rs.random_sample(200), H0, rs.random_sample(200)], [rs.random_sample((50, 100)), Ad0, rs.random_sample((50, 100))]
sep = OnlineBatchSeparator(Bx, Bds, p, 3, H0=H0s, Ad_blk0=Ads, ctx=ctx)
o = sep.process(pcms, flush=True)[1]
out.update(batch_f32_x_tilde_f=o["x_tilde_f"], batch_f32_i16=o["x_tilde"], batch_f32_basis=sep.basis_f64(1),
           batch_f32_adapt_iters=np.array([t["adapt_iters"] for t in sep.trace(1)]))
sep.close()
assert out["single_f64_adapt_iters"].max() > 0 and out["batch_f32_adapt_iters"].max() > 0  # the adaptation ran
np.savez(sys.argv[1], **out)
print("wrote %s: %s" % (sys.argv[1], ", ".join(sorted(out))))
