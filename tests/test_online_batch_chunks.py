"""A process call of the batched online separator that spans device chunks (csrc/snmf_online_batch_host.h).

One call gives a stream at most min(4096, 16384 / S) frames per device chunk (fp64 mode: 16384 / (S * classes)); the other
tests have S <= 5 (or a few hops per stream), so no stream of theirs ever crosses a chunk edge within one call.  Here the
124-frame fixture (adaptation on) runs in batches wide enough that it does: the `consumed` offsets into the pending
samples, the history handed from chunk to chunk, the overlap-add tails across the edge, and flush frames that land in a later
chunk than the stream's last PCM frame.

  fp32: S = 140, chunk = 117 frames; streams 0, 69, 139 carry the fixture, every other stream 5 hops.
  fp64: S = 34 with a 2 + 2 class partition, chunk = 16384 / 136 = 120 frames; streams 0, 16, 33 carry the fixture.

The reference is a small batch (chunk 4096 frames, never crossed) of the same three streams and, as its fourth stream, the
5-hop stream: a stream's bits depend neither on its company nor on its slot (tests/test_online_batch.py and
test_online_batch_f64.py assert that), so every array must be bit-identical (and finite: NaN equals nothing here)."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOP = 160
CASES = [
    # precision, S, the long streams' slots, class partition, frames per chunk
    ("fp32", 140, (0, 69, 139), None, 117),
    ("fp64", 34, (0, 16, 33), dict(EVENT_NUM=2, EVENT_RANK=[1, 51], NOISE_NUM=2, NOISE_RANK=[1, 51]), 120),
]


def _inputs():
    """The fixture on three start dictionaries / H0 / Ad_blk0 (those of scripts/online_bits_dump.py's three streams), and one
    5-hop stream."""
    B = np.load(os.path.join(GOLD, "ref_data.npz"))["B"].astype(np.float64)
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"].astype(np.float64)
    Bx, Bd = B[:, :100], B[:, 100:]
    rs = np.random.RandomState(1)
    H0, Ad0 = rs.random_sample(200), rs.random_sample((50, 100))
    rs = np.random.RandomState(5)
    rs.randn(40 * HOP)  # (the draw order of the script)
    Bds = [Bd[:, rs.permutation(100)], Bd, Bd * (1.0 + 0.05 * rs.random_sample(Bd.shape))]
    H0s, Ads = [rs.random_sample(200), H0, rs.random_sample(200)], [rs.random_sample((50, 100)), Ad0, rs.random_sample((50, 100))]
    short = (np.round(s[1733:1733 + 5 * HOP] * 0.75), Bd, rs.random_sample(200), rs.random_sample((50, 100)))
    return s, Bx, Bds, H0s, Ads, short


def _run(ctx, p, precision, pcms, Bx, Bds, H0s, Ads, pick):
    """One batch, one process call with the flush -> for the streams `pick`: (outputs, trace, final B_DFT_d)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    sep = OnlineBatchSeparator(Bx, Bds, p, len(pcms), H0=H0s, Ad_blk0=Ads, ctx=ctx, class_outputs=True, precision=precision)
    outs = sep.process(pcms, flush=True)
    res = [({k: v.copy() for k, v in outs[k].items()}, sep.trace(k), sep.basis_f64(k)) for k in pick]
    sep.close()
    return res


def _same(label, got, ref, dtype):
    keys = ("x_tilde_f", "x_tilde", "x_hat", "d_hat", "x_hat_i", "d_hat_i")
    assert set(keys) <= set(got[0]) and set(keys) <= set(ref[0])
    assert len(got[0]["x_tilde_f"]) == len(ref[0]["x_tilde_f"]) > 0, label  # n_out: the length the small batch returns
    for k in keys:
        assert got[0][k].dtype == ref[0][k].dtype and got[0][k].shape == ref[0][k].shape, (label, k)
        assert np.array_equal(got[0][k], ref[0][k]), (label, k)
    assert got[0]["x_tilde_f"].dtype == dtype
    assert np.array_equal(got[2], ref[2]), (label, "B_DFT_d")
    for k in ("adapt_iters", "n_iter", "trig", "n_up", "solved"):
        assert [t[k] for t in got[1]] == [t[k] for t in ref[1]], (label, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_one_call_across_device_chunks(gpu_ctx, case):
    from se_snmf_nat_amd import online
    precision, S, slots, classes, chunk = case
    p = online.default_settings()
    assert p["adapt_train_N"]
    n_cls = 1
    if classes:
        p.update(classes)
        n_cls = len(classes["EVENT_RANK"]) + len(classes["NOISE_RANK"])
    assert min(4096, online._B_CHUNK_SLOTS // (S * (n_cls if precision == "fp64" else 1))) == chunk
    s, Bx, Bds, H0s, Ads, short = _inputs()
    n_frames = len(s) // HOP + p["delay"] + 1  # with the flush frames
    assert n_frames == 124 and len(s) // HOP >= chunk  # the fixture crosses the chunk edge: its flush frames (fp32: and PCM frames) lie behind it
    dtype = np.float64 if precision == "fp64" else np.float32

    ref = _run(gpu_ctx, p, precision, [s] * 3 + [short[0]], Bx, Bds + [short[1]], H0s + [short[2]], Ads + [short[3]], range(4))
    ref_short = ref[3]
    assert all(np.isfinite(r[0][k]).all() for r in ref for k in ("x_tilde_f", "x_hat", "d_hat", "x_hat_i", "d_hat_i"))
    where = {slot: j for j, slot in enumerate(slots)}
    pcms = [s if k in where else short[0] for k in range(S)]
    pick = lambda long_ones, the_short: [long_ones[where[k]] if k in where else the_short for k in range(S)]  # noqa: E731
    big = _run(gpu_ctx, p, precision, pcms, Bx, pick(Bds, short[1]), pick(H0s, short[2]), pick(Ads, short[3]), range(S))

    live = []
    for j, slot in enumerate(slots):
        it = np.array([t["adapt_iters"] for t in big[slot][1]])
        assert len(it) == n_frames
        print("%s stream %d: %d samples, adaptation solves in frames [0, %d): %d, in [%d, %d): %d"
              % (precision, slot, len(big[slot][0]["x_tilde_f"]), chunk, (it[:chunk] > 0).sum(), chunk, n_frames, (it[chunk:] > 0).sum()))
        live.append((it[:chunk] > 0).any() and (it[chunk:] > 0).any())
        _same("%s stream %d" % (precision, slot), big[slot], ref[j], dtype)
    assert any(live)  # the crossing happens with the adaptation live on both sides of the edge
    if classes:
        assert big[slots[0]][0]["x_hat_i"].shape[0] == 2 and big[slots[0]][0]["d_hat_i"].shape[0] == 2
    for k in range(S):
        if k not in where:
            _same("%s short stream %d" % (precision, k), big[k], ref_short, dtype)
