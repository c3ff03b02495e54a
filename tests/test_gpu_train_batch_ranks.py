"""GPU tests of the batched basis-training calls with a dictionary size per problem (snmf_run_basis_train_audio_batch_ranks_fp64,
snmf_run_basis_train_signals_batch_ranks_fp64): run_basis_train_signal_batch, run_basis_train_assembled_batch and
run_basis_train_clips_batch with a sequence for R.

THE CONTRACT is a bit equality (np.array_equal throughout): problem k of run_basis_train_signal_batch(signals, [R_0, ...], p,
precision="fp64") is run_basis_train_signal(s_k, R_k, p, precision="fp64", ...) alone -- the four arrays and both iteration
counts, with n_ex_k = cluster_buff * R_k exemplar columns -- and the assembled and clips forms are the signal form on the signals
TrainSignals.signal(k) returns.  A sequence of equal R is the scalar call in both precisions.
Signals, ranks and exemplar columns: tests/batch_ranks_cases.py on tests/train_batch_cases.py."""
import numpy as np
import pytest

import assemble_cases as ac
import batch_ranks_cases as rc
import train_batch_cases as tc

pytestmark = pytest.mark.gpu
KEYS = ("B_DFT_sub", "B_Mel_sub", "A_DFT_sub", "A_Mel_sub")
VARIANTS = {
    "plain": (rc.RANKS, tc.P_STOP),
    "splice1": (rc.RANKS, dict(tc.P_STOP, Splice=1)),
    "domain_dd": (rc.RANKS, dict(tc.P_STOP, domain_DD=1, alpha_eta=0.4)),
    "exemplar": (rc.RANKS, dict(tc.P_STOP, train_Exemplar=1)),
    "cluster2": (rc.RANKS_CB2, dict(tc.P_STOP, cluster_buff=2, kmeans_seed=3)),
}


def _idx(name):
    R, p = VARIANTS[name]
    return rc.sample_idx(tuple(int(p["cluster_buff"]) * r for r in R))


def same_bits(res, ref):
    assert len(res) == len(ref)
    for k, ((o, n), (w, nr)) in enumerate(zip(res, ref)):
        assert list(n) == list(nr), (k, n, nr)
        for key in KEYS:
            if np.isscalar(w[key]):  # run_basis_train.m:95-96: the activations of the exemplar mode are the scalar 0
                assert np.isscalar(o[key]) and o[key] == w[key] == 0, (k, key)
                continue
            assert o[key].dtype == w[key].dtype == np.float64 and o[key].shape == w[key].shape, (k, key, o[key].shape, w[key].shape)
            assert np.array_equal(o[key], w[key]), (k, key, float(np.abs(o[key] - w[key]).max()))


_alone = {}


def alone(ctx, name, h0="host"):
    """run_basis_train_signal(s_k, R_k, p, precision="fp64") per problem, computed once."""
    from se_snmf_nat_amd import train
    if (name, h0) not in _alone:
        R, p = VARIANTS[name]
        out = []
        for s, ix, r in zip(tc.signals(), _idx(name), R):
            info = {}
            o = train.run_basis_train_signal(s, r, p, sample_idx=ix, ctx=ctx, h0=h0, precision="fp64", info=info)
            out.append((o, info["n_iter"]))
        _alone[(name, h0)] = out
    return _alone[(name, h0)]


def run_batch(ctx, name, h0="host", order=None):
    from se_snmf_nat_amd import train
    R, p = VARIANTS[name]
    order = list(range(len(tc.TS))) if order is None else order
    info = {}
    out = train.run_basis_train_signal_batch([tc.signals()[k] for k in order], [R[k] for k in order], p, sample_idx=[_idx(name)[k] for k in order],
                                             ctx=ctx, h0=h0, precision="fp64", info=info)
    assert info["T"] == [tc.TS[k] for k in order]
    return list(zip(out, info["n_iter"]))


@pytest.mark.parametrize("h0", ["host", "device"])
def test_every_problem_is_the_single_call_at_its_own_rank(gpu_ctx, h0):
    res = run_batch(gpu_ctx, "plain", h0=h0)
    print(f"h0={h0}: [n_dft, n_mel] per problem {[n for _, n in res]}")
    same_bits(res, alone(gpu_ctx, "plain", h0=h0))
    for (o, _), r, T in zip(res, rc.RANKS, tc.TS):
        assert o["B_DFT_sub"].shape == (tc.F, r) and o["B_Mel_sub"].shape == (tc.F_MEL, r)
        assert o["A_DFT_sub"].shape == (r, T) and o["A_Mel_sub"].shape == (r, T)
        assert all(np.isfinite(o[k]).all() for k in KEYS)
    if h0 == "host":  # (problems of one batch end at different iterations, as on the oracle: tests/test_batch_ranks_api.py)
        assert tc.stops_are_spread([n[0] for _, n in res], tc.P_STOP["max_iter"]), res
        same_bits(run_batch(gpu_ctx, "plain", order=[4, 1, 5, 0, 3, 2]), [res[k] for k in (4, 1, 5, 0, 3, 2)])  # and in any order
    else:
        assert not np.array_equal(res[5][0]["A_DFT_sub"], alone(gpu_ctx, "plain")[5][0]["A_DFT_sub"])  # (another start, another result)


@pytest.mark.parametrize("name", ["splice1", "domain_dd", "exemplar", "cluster2"])
def test_variants(gpu_ctx, name):
    R, p = VARIANTS[name]
    res = run_batch(gpu_ctx, name)
    same_bits(res, alone(gpu_ctx, name))
    K = 2 * p["Splice"] + 1
    for (o, n), r in zip(res, R):
        assert o["B_DFT_sub"].shape == (K * tc.F, r) and o["B_Mel_sub"].shape == (K * tc.F_MEL, r)
        if name == "exemplar":
            assert list(n) == [0, 0]
        else:
            assert o["A_DFT_sub"].shape[0] == r


def test_default_sample_idx_is_the_single_calls(gpu_ctx):
    """sample_idx=None: every problem gets the single call's own stand-in draw of n_ex_k columns."""
    from se_snmf_nat_amd import train
    R = [3, 1, 2]
    sigs = [tc.signals()[k] for k in (0, 2, 5)]
    ia = {}
    res = train.run_basis_train_signal_batch(sigs, R, tc.P_STOP, ctx=gpu_ctx, precision="fp64", info=ia)
    ref = []
    for s, r in zip(sigs, R):
        ib = {}
        ref.append((train.run_basis_train_signal(s, r, tc.P_STOP, ctx=gpu_ctx, precision="fp64", info=ib), ib["n_iter"]))
    same_bits(list(zip(res, ia["n_iter"])), ref)


def test_a_list_of_equal_r_is_the_scalar_call_in_both_precisions(gpu_ctx):
    from se_snmf_nat_amd import train
    sigs, ix = list(tc.signals()), tc.sample_idx()
    for mode in ("fp32", "fp64"):
        ia, ib = {}, {}
        a = train.run_basis_train_signal_batch(sigs, [tc.R] * len(sigs), tc.P_STOP, sample_idx=ix, ctx=gpu_ctx, precision=mode, info=ia)
        b = train.run_basis_train_signal_batch(sigs, tc.R, tc.P_STOP, sample_idx=ix, ctx=gpu_ctx, precision=mode, info=ib)
        same_bits(list(zip(a, ia["n_iter"])), list(zip(b, ib["n_iter"])))


# ---- the assembled and the clips forms -------------------------------------------------------------------------------------------
P_CLIPS = dict(tc.P_STOP, train_seq_len_max=700, train_file_len_max=300)
R_CLIPS = [4, 2, 6]


def clips():
    """Three small cut classes: one stops inside its third clip, one of two clips, one of T = 6 frames (every column an exemplar)."""
    rs = np.random.RandomState(78)
    return [[ac.plain_clip(rs, n) for n in (400, 250, 500)], [ac.plain_clip(rs, 600), ac.plain_clip(rs, 350)], [ac.plain_clip(rs, tc.n_samples(6))]]


@pytest.mark.parametrize("h0", ["host", "device"])
def test_assembled_and_clips_forms_give_the_bits_of_the_signal_form(gpu_ctx, h0):
    from se_snmf_nat_amd import (assemble_training_signals, run_basis_train_assembled_batch, run_basis_train_clips_batch,
                                 run_basis_train_signal_batch)
    cl = clips()
    ia, ib, ic = {}, {}, {}
    with assemble_training_signals(cl, P_CLIPS, ctx=gpu_ctx) as ts:
        assert ts.lengths[2] == tc.n_samples(6)
        res = run_basis_train_assembled_batch(ts, R_CLIPS, P_CLIPS, h0=h0, precision="fp64", info=ia)
        ref = run_basis_train_signal_batch([ts.signal(k) for k in range(3)], R_CLIPS, P_CLIPS, ctx=gpu_ctx, h0=h0, precision="fp64", info=ib)
    both = run_basis_train_clips_batch(cl, R_CLIPS, P_CLIPS, ctx=gpu_ctx, h0=h0, precision="fp64", info=ic)
    assert ia["T"] == ib["T"] == ic["T"] and ia["T"][2] == 6
    same_bits(list(zip(res, ia["n_iter"])), list(zip(ref, ib["n_iter"])))
    same_bits(list(zip(both, ic["n_iter"])), list(zip(ref, ib["n_iter"])))
    for o, r in zip(res, R_CLIPS):
        assert o["B_DFT_sub"].shape == (tc.F, r) and o["A_Mel_sub"].shape[0] == r
