"""GPU tests of the batched basis-training calls with settings per problem (snmf_run_basis_train_audio_batch_settings_fp64,
snmf_run_basis_train_signals_batch_settings_fp64): run_basis_train_signal_batch, run_basis_train_assembled_batch and
run_basis_train_clips_batch with settings=[...].

THE CONTRACT is a bit equality (np.array_equal throughout): problem k of run_basis_train_signal_batch(signals, R, p,
precision="fp64", settings=st) is run_basis_train_signal(s_k, R_k, dict(p, **st[k]), precision="fp64", ...) alone -- the four arrays
and both iteration counts -- and the assembled and clips forms are the signal form on the signals TrainSignals.signal(k) returns.
Signals, ranks and exemplar columns: tests/batch_ranks_cases.py on tests/train_batch_cases.py."""
import numpy as np
import pytest

import assemble_cases as ac
import batch_ranks_cases as rc
import train_batch_cases as tc

pytestmark = pytest.mark.gpu
KEYS = ("B_DFT_sub", "B_Mel_sub", "A_DFT_sub", "A_Mel_sub")
# the divergence (kl, ed), the sparsity weight and the iteration limit differ; tc.P_STOP gives the rest (conv_eps = 5e-4, max_iter = 20)
SETTINGS = [dict(cf="kl", sparsity=5), dict(cf="ed", sparsity=0.5, max_iter=7), dict(cf="kl", sparsity=1, max_iter=12),
            dict(cf="ed", sparsity=2.0, conv_eps=1e-2), dict(cf="kl", sparsity=0.5, max_iter=3, conv_eps=0), dict(cf="ed", sparsity=0.1, max_iter=9, conv_eps=0)]
assert len(SETTINGS) == len(tc.TS)


def same_bits(res, ref):
    assert len(res) == len(ref)
    for k, ((o, n), (w, nr)) in enumerate(zip(res, ref)):
        assert list(n) == list(nr), (k, n, nr)
        for key in KEYS:
            assert o[key].dtype == w[key].dtype == np.float64 and o[key].shape == w[key].shape, (k, key, o[key].shape, w[key].shape)
            assert np.array_equal(o[key], w[key]), (k, key, float(np.abs(o[key] - w[key]).max()))


_alone = {}


def alone(ctx, R, h0="host"):
    """run_basis_train_signal(s_k, R_k, dict(p, **settings_k), precision="fp64") per problem, computed once."""
    from se_snmf_nat_amd import train
    key = (tuple(R), h0)
    if key not in _alone:
        out = []
        for s, ix, r, st in zip(tc.signals(), rc.sample_idx(tuple(R)), R, SETTINGS):
            info = {}
            o = train.run_basis_train_signal(s, r, dict(tc.P_STOP, **st), sample_idx=ix, ctx=ctx, h0=h0, precision="fp64", info=info)
            out.append((o, info["n_iter"]))
        _alone[key] = out
    return _alone[key]


def run_batch(ctx, R, h0="host", order=None, scalar_R=False):
    from se_snmf_nat_amd import train
    order = list(range(len(tc.TS))) if order is None else order
    info = {}
    idx = rc.sample_idx(tuple(R))
    out = train.run_basis_train_signal_batch([tc.signals()[k] for k in order], R[0] if scalar_R else [R[k] for k in order], tc.P_STOP,
                                             sample_idx=[idx[k] for k in order], ctx=ctx, h0=h0, precision="fp64", info=info,
                                             settings=[SETTINGS[k] for k in order])
    assert info["T"] == [tc.TS[k] for k in order]
    return list(zip(out, info["n_iter"]))


@pytest.mark.parametrize("h0", ["host", "device"])
def test_every_signal_is_the_single_call_with_its_own_settings(gpu_ctx, h0):
    res = run_batch(gpu_ctx, rc.RANKS, h0=h0)
    print(f"h0={h0}: [n_dft, n_mel] per problem {[n for _, n in res]}")
    same_bits(res, alone(gpu_ctx, rc.RANKS, h0=h0))
    for (o, n), r, T, st in zip(res, rc.RANKS, tc.TS, SETTINGS):
        assert o["B_DFT_sub"].shape == (tc.F, r) and o["A_Mel_sub"].shape == (r, T)
        assert all(np.isfinite(o[k]).all() for k in KEYS)
        assert max(n) <= st.get("max_iter", tc.P_STOP["max_iter"])
    assert [n for _, n in res][5] == [9, 9] and [n for _, n in res][4] == [3, 3]  # (no threshold / a limit of 3: the own max_iter)
    if h0 == "host":
        order = [4, 1, 5, 0, 3, 2]
        same_bits(run_batch(gpu_ctx, rc.RANKS, order=order), [res[k] for k in order])  # and in any order


def test_one_dictionary_size_for_all(gpu_ctx):
    """n_atoms = NULL: R an int, the settings still per problem."""
    R = [tc.R] * len(tc.TS)
    same_bits(run_batch(gpu_ctx, R, scalar_R=True), alone(gpu_ctx, R))


# ---- the assembled and the clips forms -------------------------------------------------------------------------------------------
P_CLIPS = dict(tc.P_STOP, train_seq_len_max=700, train_file_len_max=300)
R_CLIPS = [4, 2, 6]
S_CLIPS = [dict(cf="ed", sparsity=0.5, max_iter=6), dict(cf="kl", sparsity=1), dict(cf="kl", sparsity=5, max_iter=4, conv_eps=0)]


def clips():
    """Three small cut classes: one stops inside its third clip, one of two clips, one of T = 6 frames (every column an exemplar)."""
    rs = np.random.RandomState(78)
    return [[ac.plain_clip(rs, n) for n in (400, 250, 500)], [ac.plain_clip(rs, 600), ac.plain_clip(rs, 350)], [ac.plain_clip(rs, tc.n_samples(6))]]


@pytest.mark.parametrize("h0", ["host", "device"])
def test_assembled_and_clips_forms_give_the_bits_of_the_single_calls(gpu_ctx, h0):
    from se_snmf_nat_amd import (assemble_training_signals, run_basis_train_assembled_batch, run_basis_train_clips_batch,
                                 run_basis_train_signal_batch, train)
    cl = clips()
    ia, ib, ic = {}, {}, {}
    ref = []
    with assemble_training_signals(cl, P_CLIPS, ctx=gpu_ctx) as ts:
        res = run_basis_train_assembled_batch(ts, R_CLIPS, P_CLIPS, h0=h0, precision="fp64", info=ia, settings=S_CLIPS)
        sigs = [ts.signal(k) for k in range(3)]
        sig = run_basis_train_signal_batch(sigs, R_CLIPS, P_CLIPS, ctx=gpu_ctx, h0=h0, precision="fp64", info=ib, settings=S_CLIPS)
    for s, r, st in zip(sigs, R_CLIPS, S_CLIPS):
        info = {}
        ref.append((train.run_basis_train_signal(s, r, dict(P_CLIPS, **st), ctx=gpu_ctx, h0=h0, precision="fp64", info=info), info["n_iter"]))
    both = run_basis_train_clips_batch(cl, R_CLIPS, P_CLIPS, ctx=gpu_ctx, h0=h0, precision="fp64", info=ic, settings=S_CLIPS)
    assert ia["T"] == ib["T"] == ic["T"] and ia["T"][2] == 6
    same_bits(list(zip(sig, ib["n_iter"])), ref)
    same_bits(list(zip(res, ia["n_iter"])), ref)
    same_bits(list(zip(both, ic["n_iter"])), ref)
    assert ia["n_iter"][2] == [4, 4]
