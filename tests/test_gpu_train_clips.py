"""GPU tests of run_basis_train_assembled_batch and run_basis_train_clips_batch (snmf_run_basis_train_signals_batch_*): basis
training on the signals a TrainSignals handle holds in HBM.

THE CONTRACT is a bit equality with what is already shipped (np.array_equal throughout): all four matrices and both iteration
counts of every class are those of run_basis_train_signal_batch([ts.signal(k) ...], R, p, ...) -- in fp64 on the doubles, in fp32
on those doubles rounded to float, which that call does on the host and the new one on the device.  Geometry and solver settings:
tests/train_batch_cases.py (TINY: fs 16000, so bg_len 800 and VAD frames of 320 samples)."""
import ctypes as C

import numpy as np
import pytest

import assemble_cases as ac
import train_batch_cases as tc

pytestmark = pytest.mark.gpu
MODES = ["fp32", "fp64"]
KEYS = ("B_DFT_sub", "B_Mel_sub", "A_DFT_sub", "A_Mel_sub")
P = dict(tc.P_STOP, train_seq_len_max=700, train_file_len_max=300)
VARIANTS = {
    "host_h0": (P, dict()),
    "device_h0": (P, dict(h0="device")),
    "domain_dd": (dict(P, domain_DD=1, alpha_eta=0.4), dict()),
    "exemplar": (dict(P, train_Exemplar=1), dict()),
    "dc_bin": (P, dict(DC_bin=3)),
}


def quiet_then_loud(rs, n, quiet):
    """int16 at 16 kHz: a background in +-12 over the first `quiet` samples (bg_len is 800), +-9000 behind it."""
    c = rs.randint(-12, 13, size=n).astype(np.int16)
    c[quiet:] = rs.randint(-9000, 9001, size=n - quiet)
    return c


def clips():
    """A cut class that stops inside its third clip, a VAD class whose second clip has no voiced frame (its loud end lies behind
    the last frame), a range class, a short cut class (T = 6 = R: every column an exemplar)."""
    rs = np.random.RandomState(77)
    return dict(classes=[[ac.plain_clip(rs, n) for n in (400, 250, 500)], [quiet_then_loud(rs, 1300, 900), quiet_then_loud(rs, 900, 820)],
                         [ac.plain_clip(rs, 600), ac.plain_clip(rs, 350)], [ac.plain_clip(rs, tc.n_samples(6))]],
                vad=[False, True, False, False], ranges=[None, None, [(11, 410), (0, 9999)], None])


@pytest.fixture(scope="module")
def ts(gpu_ctx):
    from se_snmf_nat_amd import assemble_training_signals
    c = clips()
    with assemble_training_signals(c["classes"], P, vad=c["vad"], ranges=c["ranges"], ctx=gpu_ctx) as t:
        yield t


def same_bits(res, ref, ia, ib):
    assert ia["T"] == ib["T"] and ia["n_iter"] == ib["n_iter"], (ia, ib)
    assert len(res) == len(ref)
    for k, (o, w) in enumerate(zip(res, ref)):
        for key in KEYS:
            if np.isscalar(w[key]):
                assert np.isscalar(o[key]) and o[key] == w[key] == 0, (k, key)
                continue
            assert o[key].dtype == np.float64 and o[key].shape == w[key].shape, (k, key)
            assert np.array_equal(o[key], w[key]), (k, key, float(np.abs(o[key] - w[key]).max()))


@pytest.mark.parametrize("name", sorted(VARIANTS))
@pytest.mark.parametrize("mode", MODES)
def test_resident_signals_train_to_the_bits_of_the_host_signals(gpu_ctx, ts, mode, name):
    from se_snmf_nat_amd import run_basis_train_assembled_batch, run_basis_train_signal_batch
    p, kw = VARIANTS[name]
    assert ts.lengths == [700, ts.lengths[1], 700, tc.n_samples(6)] and ts.clips_used == [3, 2, 2, 1] and 400 <= ts.lengths[1] < 700
    ia, ib = {}, {}
    res = run_basis_train_assembled_batch(ts, tc.R, p, precision=mode, info=ia, **kw)
    ref = run_basis_train_signal_batch([ts.signal(k) for k in range(4)], tc.R, p, ctx=gpu_ctx, precision=mode, info=ib, **kw)
    print(mode, name, "T", ia["T"], "n_iter", ia["n_iter"])
    same_bits(res, ref, ia, ib)
    assert ia["T"][3] == 6 and res[0]["B_DFT_sub"].shape == (tc.F, tc.R) and res[0]["B_Mel_sub"].shape == (tc.F_MEL, tc.R)
    assert all(np.isfinite(o[k]).all() for o in res for k in KEYS)


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_of_one_and_given_exemplar_columns(gpu_ctx, mode):
    from se_snmf_nat_amd import assemble_training_signals, run_basis_train_assembled_batch, run_basis_train_signal_batch
    c = clips()
    ix = [np.arange(1, 2 * tc.R, 2)]
    with assemble_training_signals([c["classes"][1]], P, vad=[True], ctx=gpu_ctx) as one:
        ia, ib = {}, {}
        res = run_basis_train_assembled_batch(one, tc.R, P, sample_idx=ix, precision=mode, info=ia)
        ref = run_basis_train_signal_batch([one.signal(0)], tc.R, P, sample_idx=ix, ctx=gpu_ctx, precision=mode, info=ib)
        same_bits(res, ref, ia, ib)


@pytest.mark.parametrize("mode", MODES)
def test_clips_in_dictionaries_out_equals_the_two_steps(gpu_ctx, ts, mode):
    from se_snmf_nat_amd import run_basis_train_assembled_batch, run_basis_train_clips_batch
    c = clips()
    ia, ib = {}, {}
    res = run_basis_train_clips_batch(c["classes"], tc.R, P, vad=c["vad"], ranges=c["ranges"], ctx=gpu_ctx, precision=mode, info=ia)
    ref = run_basis_train_assembled_batch(ts, tc.R, P, precision=mode, info=ib)
    same_bits(res, ref, ia, ib)
    assert ia["lengths"] == ts.lengths and ia["clips_used"] == ts.clips_used


def test_the_refusals_are_the_training_entrys(gpu_ctx, lib):
    """A class shorter than one analysis frame assembles fine; the training entry refuses it with the existing message.  A handle
    of another context is refused; so is what the existing entries refuse."""
    from se_snmf_nat_amd import Context, assemble_training_signals, frontend as fe
    from se_snmf_nat_amd.api import _make_params
    rs = np.random.RandomState(8)
    sp, _win = fe._params(tc.TINY)
    n = 2
    T = 33

    def call(ty, h, *, ctx=gpu_ctx._h, F=tc.F, null=None):
        sdt = np.float32 if ty == "f64" else np.float64
        q = _make_params(F, 1, tc.R, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
        keep = dict(idx=[np.arange(tc.R, dtype=np.int64) for _ in range(n)], H0=[np.full((tc.R, 40), 0.5, order="F") for _ in range(n)],
                    B_DFT=[np.ones((F, tc.R), order="F") for _ in range(n)], A_DFT=[np.ones((tc.R, 40), order="F") for _ in range(n)],
                    B_Mel=[np.ones((tc.F_MEL, tc.R), order="F") for _ in range(n)], A_Mel=[np.ones((tc.R, 40), order="F") for _ in range(n)])
        a = {k: (None if null == k else (C.c_void_p * n)(*[x.ctypes.data for x in v])) for k, v in keep.items()}
        mel = np.ones((tc.F_MEL, tc.F), dtype=sdt)
        n_iter = np.zeros(2 * n, np.int32)
        return getattr(lib, f"snmf_run_basis_train_signals_batch_{ty}")(
            ctx, C.byref(q), C.byref(sp), -1.0, C.c_void_p(mel.ctypes.data), tc.F_MEL, h, a["idx"], 0, a["H0"], None, a["B_DFT"], a["A_DFT"],
            a["B_Mel"], a["A_Mel"], C.c_void_p(n_iter.ctypes.data))

    p = dict(fs=16000, train_seq_len_max=10_000, train_file_len_max=0)
    with assemble_training_signals([[ac.plain_clip(rs, tc.n_samples(T))], [ac.plain_clip(rs, tc.N + 1)]], p, ctx=gpu_ctx) as short, \
            assemble_training_signals([[ac.plain_clip(rs, tc.n_samples(T))], [ac.plain_clip(rs, tc.n_samples(T))]], p, ctx=gpu_ctx) as good:
        assert short.lengths == [tc.n_samples(T), tc.N + 1]  # (assembled fine)
        other = Context(0)
        for ty in ("f64", "fp64"):
            assert call(ty, good._h) == 0
            assert call(ty, short._h) == 1 and b"snmf_run_basis_train_signals_batch" in lib.snmf_last_error() \
                and b"shorter than one analysis frame" in lib.snmf_last_error()
            assert call(ty, good._h, ctx=other._h) == 1 and b"another context" in lib.snmf_last_error()
            assert call(ty, None) == 1 and call(ty, good._h, ctx=None) == 1
            assert call(ty, good._h, null="idx") == 1 and call(ty, good._h, null="B_DFT") == 1 and call(ty, good._h, null="B_Mel") == 1
            assert call(ty, good._h, null="H0") == 1                      # no H0 and no seeds
            assert call(ty, good._h, F=tc.F + 1) == 3
            assert call(ty, good._h) == 0                                  # the context and the handle still work
        other.close()
