"""One frame step of the SINGLE-STREAM online separator (OnlineSeparator, the path the reference ships as NTF_sep_event_RT) judged
per element from its own state g.  The method, the bounds, the comparison and the driver are tests/online_step.py's, shared with
the batch's test (tests/test_gpu_online_step.py); tests/test_online_step_rules.py proves them on the CPU, every case below
included, and runs this driver on a simulated device with planted errors.

One separator per stream, one hop per process call, a get_state before the first hop and after every hop: the after-state of
frame l is the before-state of frame l + 1.  Every (frame, stream) pair is judged alone against oracle.online_oracle.sep_frame
run from the device's own before-state: per element under the derived worst-case bounds, the exact invariants bit for bit, the
decisions, and per field and region the device's RMS relative error against 4 x the larger of the two float32 emulations run
from the same states.

WHY NO BOUND DIFFERS FROM THE BATCH'S.  The single-stream separator runs other kernels than the batch, but what the bounds
assume holds for them as read from the code:
  k_ostft / k_oistft (snmf_online_common.h) call the same fft_lds that frame_step restates (radix-2 Stockham, twiddles formed
      in double and rounded), so the transform term (7 log2 N + 2) u ||Y||_2 is unchanged, at fft 2048 too (log2 N = 11).
  k_hsolve_frame<BATCH = false>, k_hsolve_small and the plan loop's k_hstep form Lam = W h and W' (V ./ Lam) as sums of F or r
      non-negative terms in some order (MFMA tiles, wave reductions); tau_h(F, r, beta) is a bound for ANY order of summation
      of that length, which is why both emulation orders are run.
  k_wadapt / k_wadapt64 and the W-only plan loop form the W step's products, the column sums (cross_sum: the workgroups'
      partials in DOUBLE, a fixed order) and the column norms as sums of m_a or F terms in some order: tau_w(F, n_up, beta,
      m_a) covers any order, and partials carried in double are no worse than in the mode's type.
  The semi-supervised solve (plan hsemi) at one iteration updates H before W: A is the supervised step's A, under tau_h + 4u,
      and its private W is discarded, so B_DFT_d is judged exactly as without the setting.

The measured table is in docs/KERNELS.md ("How the single-stream frame step is judged")."""
import numpy as np
import pytest

import online_step as os_

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", os_.SINGLE_REUSED + list(os_.SINGLE_CASES))
def test_every_frame_step_of_a_single_stream_is_inside_its_bounds(gpu_ctx, monkeypatch, name):
    """All three streams of every case are judged (none is dropped for time)."""
    env, _, fixed = os_.single_case(name)
    monkeypatch.delenv("SNMF_NO_WADAPT", raising=False)
    for key, val in env.items():  # (read when the separator is created)
        monkeypatch.setenv(key, val)
    views, precision, steps = os_.run_single(os_.device_separator(gpu_ctx), name)
    dev = os_.judge_run(name, views, precision, steps, fixed=fixed)
    assert (dev.triggered == 0 and dev.solved == 0) if fixed else dev.solved >= 2


def test_s4_frame_solve_is_outside_the_persistent_kernel(gpu_ctx):
    """s4's H-only plan on the device has small_ok == false (so OnlineSeparator's frame solve is the plan loop at T = 1): the
    persistent kernels' own entry, solve_frames, refuses the shape, and accepts s3's."""
    from se_snmf_nat_amd import Plan, SnmfError
    rs = np.random.RandomState(3)
    for geo, ok in ((os_.GEO_S4, False), (os_.GEO_S3, True)):
        F, r = geo[0] // 2 + 1, geo[3] + geo[4]
        pl = Plan(gpu_ctx, F, 1, r, max_iter=1, w_update_ind=np.zeros(r), sparsity=5.0)
        pl.set_w(rs.random_sample((F, r)) + 0.1)
        v, h0 = rs.random_sample((F, 1)) + 0.1, rs.random_sample((r, 1)) + 0.1
        if ok:
            H, nit, _ = pl.solve_frames(v, h0, dtype=np.float32)
            assert np.isfinite(H).all() and nit[0] == 1
        else:
            with pytest.raises(SnmfError, match="persistent online kernel") as e:
                pl.solve_frames(v, h0, dtype=np.float32)
            assert e.value.status == 8
        pl.close()


STATE_FIELDS = ("Xm_tilde", "lambda_dav", "r_blk", "lambda_d_blk", "Ad_blk", "n_push", "update_switch", "B_DFT_d", "B_fix", "H0", "Ad_blk0",
                "l", "y_hist", "pending", "x_tilde_tail")


@pytest.mark.parametrize("name", [n for n in os_.SINGLE_CASES if n.startswith("s6_")])
@pytest.mark.parametrize("hops_per_call", [5, 33])
def test_a_multi_frame_call_of_a_fixed_dictionary_run_has_the_bits_of_single_hops(gpu_ctx, name, hops_per_call):
    """adapt_train_N = 0: om_solve_run puts all frames of a call into one launch_small (33 hops: more than one 32-frame tile)
    and one k_opost launch walks them in order.  Frames are independent columns of the frame kernels, so the state record after
    every call, the outputs and the trace must be bit-identical to the hop-by-hop run at the same frame counts."""
    make = os_.device_separator(gpu_ctx)
    _, _, one = os_.run_single(make, name, keep_outputs=True)
    _, _, many = os_.run_single(make, name, hops_per_call=hops_per_call, keep_outputs=True)
    for k, ((st1, out1, tr1), (stn, outn, trn)) in enumerate(zip(one, many)):
        assert len(stn) == -(-len(st1) // hops_per_call) and len(st1) >= 33  # (every stream has a call of 33 frames)
        for c, st in enumerate(stn):
            at = st1[min(len(st1), (c + 1) * hops_per_call) - 1]
            assert st["l"] == at["l"]
            for key in STATE_FIELDS:
                assert np.array_equal(st[key], at[key]), (name, "stream", k, "call", c, "field", key)
        for key in ("x_tilde", "x_tilde_f"):
            assert np.array_equal(np.concatenate([o[key] for o in outn]), np.concatenate([o[key] for o in out1])), (name, k, key)
        assert trn == tr1, (name, "stream", k, "trace")
