"""One frame step of the batched online separator judged per element from the device's own state g (tests/online_step.py holds
the method, the derivation of the bounds and the cases; tests/test_online_step_rules.py proves them on the CPU).

A batch of three streams, one hop per process call, a get_state after every hop: the after-state of frame l is the before-state of
frame l + 1.  Every (frame, stream) pair is judged alone against oracle.online_oracle.sep_frame run from the device's own
before-state: per element under the derived worst-case bounds, the exact invariants bit for bit, the decisions, and per field and
region the device's RMS relative error against 4 x the larger of the two float32 emulations run from the same states.

Every case prints, per field and region: worst / bound, the device's RMS against the emulations' RMS, and the left-out share.
The measured table is in docs/KERNELS.md ("How the online frame step is judged")."""
import numpy as np
import pytest

import online_step as os_

pytestmark = pytest.mark.gpu


def _run(ctx, name):
    """The case on the device: per stream the list of (state before, frame buffer, state after, trace entry)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p, pcms, Bx, Bds, H0s, Ads, precision, settings = os_.case_inputs(name)
    hop = p["frameshift"]
    views = [os_.stream_view(p, Bx, settings, k) for k in range(3)]
    cls = os_.class_cols(p, views[0][1].shape[1], Bds[0].shape[1]) is not None
    kw = dict(settings=settings) if settings else {}  # (with them Bx is a list: snmf_online_batch_create_streams_f64)
    if "_melmat" in p:  # Mel mode: the shared B_Mel_x and every stream's own B_Mel_d
        kw.update(B_Mel_x=p["_B_Mel_x"], B_Mel_d=p["_B_Mel_ds"])
    sep = OnlineBatchSeparator(Bx, Bds, p, 3, H0=H0s, Ad_blk0=Ads, ctx=ctx, precision=precision, class_outputs=cls, **kw)
    n = [len(x) // hop for x in pcms]
    assert len(set(n)) > 1  # the streams stand at different frames
    before = [os_.state64(st) for st in sep.get_state([0, 1, 2])]
    assert all(("class_tails" in st) == cls and ("x_hat_tail" in st) == cls for st in before)
    steps = [[] for _ in range(3)]
    for i in range(max(n)):
        feed = [pcms[k][i * hop:(i + 1) * hop] if i < n[k] else np.zeros(0) for k in range(3)]
        sep.process(feed)
        after = [os_.state64(st) for st in sep.get_state([0, 1, 2])]
        for k in range(3):
            if i < n[k]:
                assert before[k]["pending"].size == 0 and before[k]["l"] == i + 1
                steps[k].append((before[k], os_.frame_buffer(before[k], feed[k]), after[k]))
            else:  # a stream that was fed nothing stands still, bit for bit
                assert all(np.array_equal(after[k][key], before[k][key]) for key in after[k]), (name, k, i)
        before = after
    traces = [sep.trace(k) for k in range(3)]
    sep.close()
    assert [len(t) for t in traces] == n
    return views, precision, [[s + (traces[k][i],) for i, s in enumerate(steps[k])] for k in range(3)]


@pytest.mark.parametrize("name", list(os_.CASES))
def test_every_frame_step_is_inside_its_bounds(gpu_ctx, name):
    views, precision, steps = _run(gpu_ctx, name)
    os_.judge_run(name, views, precision, steps)  # (judges, prints and asserts: the single-stream test shares it)


def test_one_rank_past_the_frame_kernel_is_refused(gpu_ctx):
    """r = 201 at F = 513 is outside k_hsolve_frame's envelope, and the batched separator has no other frame solve: it must say
    so (SNMF_ERR_UNSUPPORTED) instead of taking a slower or different path."""
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    from test_online_batch import _geo_streams, _settings
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(os_.GEO6, 8)
    assert Bx.shape[0] == 513 and Bx.shape[1] + Bds[0].shape[1] == 201
    with pytest.raises(SnmfError, match="envelope") as e:
        OnlineBatchSeparator(Bx, Bds, _settings(dict(p, **os_.ONE_STEP)), 3, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    assert e.value.status == 8
