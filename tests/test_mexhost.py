"""The MEX shims (integration/*_mex.cpp) executed without MATLAB and without a device: tests/mexhost/mexhost.cpp implements
the prototypes of integration/mex_stub/mex.h, tests/mexhost.py drives a shim + host shared object through ctypes.

Here: the host's own rules (so that what it reports about a shim can be trusted), that all five shims compile with
-Wall -Werror and link against the library, every argument check a shim makes before it touches the device (one case per
message, judged by the error id), the frame count of snmf_dnmf_mex('nframes') against frontend.num_frames, what a call that
does reach the device raises where there is none, and the arity of every *_mex call in integration/*.m against the nrhs
test of the command it names -- the only check those files can get without MATLAB.

Defects these tests found in the shims, all fixed with them (without a device, 119 of the 159 validation cases ended in
snmf:device before the fixes: the argument was never looked at):
  * snmf_online_mex 'create' checked no array size: B_DFT_x / B_DFT_d rows, numel(H0), size(Ad_blk0), the two windows
    (test_validation: online-dim-*); 'basis' sized its output by what the caller said and 'set_mel' read three unchecked
    matrices (tests/test_gpu_mex.py::test_online_wrong_sizes_are_refused: they need a handle).
  * snmf_online_mex and snmf_frontend_mex created the device context before parsing anything; sparse_nmf_mex and
    snmf_mdi_mex before reading the masks (test_validation runs those paths with no device).
  * fill_mask of sparse_nmf_mex / snmf_mdi_mex read any non-logical mask through mxGetDoubles (sparse-type-mask-int16).
  * snmf_dnmf_mex took matrices for the waveforms x, d, s_full (numel samples read), 'mel' of snmf_frontend_mex read
    melmat through mxGetDoubles unchecked and failed in fp32 for T = 0 where the fp64 mode returned K*M x 0.
"""
import glob
import os
import re

import numpy as np
import pytest

from mexhost import SHIMS, HostError, MexError, mex_shims, misbehave  # noqa: F401  (session fixtures)
from se_snmf_nat_amd import frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the host itself ---------------------------------------------------------------------------------------------------
ROUND_TRIP = {
    "double": np.arange(12, dtype=np.float64).reshape(3, 4) / 7,
    "single": np.arange(6, dtype=np.float32).reshape(2, 3) / 3,
    "logical": np.array([[True, False, True]]),
    "int16": np.array([[-32768], [7], [32767]], dtype=np.int16),
    "int32": np.array([[1, -2, 2 ** 31 - 1]], dtype=np.int32),
    "char": "fp64 é",
    "struct": {"a": np.eye(2), "s": "kl", "inner": {"b": np.array([[True]])}, "e": np.zeros((0, 0))},
    "empty": np.zeros((0, 5)),
}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, str):
        return a == b
    return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("cls", list(ROUND_TRIP))
def test_host_round_trip(misbehave, cls):
    """Python -> mxArray -> mxDuplicateArray (deep) -> Python keeps class, shape, order and values."""
    x = ROUND_TRIP[cls]
    before = misbehave.live_arrays()
    (y,) = misbehave(1, "ok", x)
    assert _same(x, y), (x, y)
    assert y is not x and (not isinstance(y, np.ndarray) or y.size == 0 or y.flags.f_contiguous)
    assert misbehave.live_arrays() == before == 0, "the call's temporary, its inputs and its copied result must be gone"


def test_host_creates_zero_filled(misbehave):
    (s,) = misbehave(1, "make")
    assert list(s) == ["d", "i16", "i32", "s"]
    for k, (shape, dt) in {"d": ((2, 3), np.float64), "i16": ((3, 1), np.int16), "i32": ((1, 2), np.int32), "s": ((2, 2), np.float32)}.items():
        assert s[k].shape == shape and s[k].dtype == dt and not s[k].any()


@pytest.mark.parametrize("x,want", [(np.array([[2.5, 9.0]]), 2.5), (np.array([3], np.float32), 3.0), (np.array([True, False]), 1.0),
                                    (np.array([-7, 1], np.int16), -7.0), (np.array([70000], np.int32), 70000.0), ("A", 65.0)])
def test_host_get_scalar(misbehave, x, want):
    """mxGetScalar: the first element of any non-struct class, as a double."""
    assert misbehave(1, "scalar", x)[0][0, 0] == want


@pytest.mark.parametrize("x", [{"a": 1.0}, np.zeros((0, 0))])
def test_host_get_scalar_of_struct_or_empty_is_a_host_error(misbehave, x):
    with pytest.raises(HostError, match="mxGetScalar"):
        misbehave(1, "scalar", x)


@pytest.mark.parametrize("x,buflen,status,length", [("fp64", 16, 0, 4), ("fp64", 5, 0, 4), ("fp64", 4, 1, 3), ("", 8, 0, 0),
                                                    (np.array([1.0]), 8, 1, 0), (np.array([True]), 8, 1, 0)])
def test_host_get_string(misbehave, x, buflen, status, length):
    """mxGetString: 0 on success; non-zero for a non-char array or when the buffer truncates (buflen - 1 characters fit)."""
    (r,) = misbehave(1, "string", x, buflen)
    assert (r[0, 0], r[0, 1]) == (status, length)


def test_host_get_field_and_is_empty(misbehave):
    s = {"here": 1.0, "void": np.zeros((3, 0))}
    assert misbehave(1, "field", s, "here")[0].tolist() == [[1, 0]]
    assert misbehave(1, "field", s, "void")[0].tolist() == [[1, 1]]   # any dimension 0
    assert misbehave(1, "field", s, "absent")[0].tolist() == [[0, -1]]  # NULL
    assert misbehave(1, "field", 3.0, "here")[0].tolist() == [[0, -1]]  # not a struct: NULL


@pytest.mark.parametrize("cmd,arg,what", [
    ("guard", None, "guard zone"), ("guard_before", None, "guard zone"), ("guard_temp", None, "guard zone"),
    ("input", np.ones((2, 2)), "prhs\\[1\\] was modified"), ("double_free", None, "called twice"),
    ("free_input", np.ones(3), "on an input"), ("return_destroyed", None, "the call destroyed"),
    ("return_input", np.ones(3), "is an input array"), ("extra_plhs", None, "plhs\\[1\\] written"),
    ("wrong_type", np.array([True]), "mxGetDoubles on an array of class 3")])
def test_host_checks_fire(misbehave, cmd, arg, what):
    """Every rule the host enforces, broken on purpose by tests/mexhost/misbehave_mex.cpp: reported, never a crash."""
    before = misbehave.live_arrays()
    with pytest.raises(HostError, match=what):
        misbehave(1, cmd, *([] if arg is None else [arg]))
    assert misbehave.live_arrays() == before == 0
    assert misbehave(1, "ok", 1.0)[0][0, 0] == 1.0  # and the host goes on working


def test_host_extra_plhs_counts_from_nlhs(misbehave):
    with pytest.raises(HostError, match="plhs\\[3\\] written"):
        misbehave(3, "extra_plhs")
    assert len(misbehave(0, "ok", 1.0)) == 1  # nlhs = 0 still returns plhs[0] (MATLAB's `ans`)


def test_host_error_carries_id_and_formatted_text_and_frees(misbehave):
    before = misbehave.live_arrays()
    with pytest.raises(MexError) as e:
        misbehave(1, "error_after_create")
    assert (e.value.id, e.value.msg) == ("mis:boom", "value 42 and 'text'")
    assert misbehave.live_arrays() == before, "arrays alive at the error are freed by the host"


def test_host_lock_and_exit(misbehave):
    n = misbehave.lock_count()
    misbehave(1, "lock")
    misbehave(1, "lock")
    assert misbehave.lock_count() == n + 2 and not misbehave.has_exit_fcn()
    misbehave.unload()
    assert misbehave.lock_count() == 0


# ---- the shims: compile, link, validate ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHIMS)
def test_shim_compiles_and_links(mex_shims, name):
    """g++ -std=c++17 -Wall -Werror -shared -fPIC of the shim + host against libsnmf_hip.so; loaded after _lib.load(), one
    libsnmf_hip.so in the process (asserted in mexhost.Mex)."""
    assert os.path.exists(mex_shims[name].path)


F, T, R = 6, 9, 4
N_FFT, N_S = 64, 700
_rs = np.random.RandomState(3)
V, W0, H0 = _rs.rand(F, T) + .1, _rs.rand(F, R) + .1, _rs.rand(R, T) + .1
OPTS = dict(beta=1.0, max_iter=3, conv_eps=0.0, cost_check=1.0, floor_v=1.0)
WIN = np.sqrt(np.hanning(N_FFT + 1)[:N_FFT])
P = dict(framelength=64.0, frameshift=16.0, fftlength=64.0, DCbin=1.0, Splice=0.0, preemph=0.0, pow=2.0, nonzerofloor=1e-9, win_STFT=WIN,
         R_x=3.0, R_d=2.0, cf="kl", sparsity=5.0, max_iter=3.0, conv_eps=0.0, cost_check=1.0, random_seed=1.0)
S = _rs.randn(N_S)
NB = N_FFT // 2 + 1
T_S = -(-(N_S - N_FFT - 1) // 16)  # frames of S (src/stft_fft.m:21; test_nframes_matches_the_binding checks the rule), no library needed here
MEL = _rs.rand(7, NB)
B_D, B_M = _rs.rand(NB, 5) + .1, _rs.rand(7, 5) + .1
OP = dict(P, overlapscale=0.5, delay=3.0, win_ISTFT=WIN, adapt_train_N=1.0, R_a=3.0, m_a=4.0)
BX, BD, OH0, AD = _rs.rand(NB, 3) + .1, _rs.rand(NB, 2) + .1, _rs.rand(5), _rs.rand(3, 4)


def without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731

# (shim, case name, expected id, nlhs, args): every path that is decided before the device
VALIDATION = [
    # ---- sparse_nmf_mex(v, w0, h0, sparsity, opts)
    ("sparse_nmf_mex", "nargin", "snmf:nargin", 1, (V, W0, H0, 5.0)),
    ("sparse_nmf_mex", "nargout", "snmf:nargout", 6, (V, W0, H0, 5.0, OPTS)),
    ("sparse_nmf_mex", "type-v-single", "snmf:type", 1, (f32(V), W0, H0, 5.0, OPTS)),
    ("sparse_nmf_mex", "type-w0-logical", "snmf:type", 1, (V, W0 > .5, H0, 5.0, OPTS)),
    ("sparse_nmf_mex", "type-h0-char", "snmf:type", 1, (V, W0, "ones", 5.0, OPTS)),
    ("sparse_nmf_mex", "type-sparsity-single", "snmf:type", 1, (V, W0, H0, f32(5), OPTS)),
    ("sparse_nmf_mex", "type-opts", "snmf:type", 1, (V, W0, H0, 5.0, 1.0)),
    ("sparse_nmf_mex", "dim-w0-rows", "snmf:dim", 1, (V, W0[:-1], H0, 5.0, OPTS)),
    ("sparse_nmf_mex", "dim-h0-cols", "snmf:dim", 1, (V, W0, H0[:, :-1], 5.0, OPTS)),
    ("sparse_nmf_mex", "dim-h0-transposed", "snmf:dim", 1, (V, W0, H0.T, 5.0, OPTS)),
    ("sparse_nmf_mex", "dim-sparsity-rows", "snmf:dim", 1, (V, W0, H0, np.ones(R - 1), OPTS)),
    ("sparse_nmf_mex", "dim-sparsity-row-vector", "snmf:dim", 1, (V, W0, H0, np.ones((1, R)), OPTS)),
    ("sparse_nmf_mex", "dim-mask-w", "snmf:dim", 1, (V, W0, H0, 5.0, dict(OPTS, w_update_ind=np.ones(R + 1, bool)))),
    ("sparse_nmf_mex", "dim-mask-h", "snmf:dim", 1, (V, W0, H0, 5.0, dict(OPTS, h_update_ind=np.ones(R - 1)))),
    ("sparse_nmf_mex", "type-mask-int16", "snmf:type", 1, (V, W0, H0, 5.0, dict(OPTS, h_update_ind=np.ones(R, np.int16)))),
    ("sparse_nmf_mex", "type-devices", "snmf:type", 1, (V, W0, H0, 5.0, dict(OPTS, devices=f32([0, 0])))),
    ("sparse_nmf_mex", "type-precision-number", "snmf:type", 1, (V, W0, H0, 5.0, dict(OPTS, precision=64.0))),
    ("sparse_nmf_mex", "type-precision-other", "snmf:type", 1, (V, W0, H0, 5.0, dict(OPTS, precision="fp16"))),
    ("sparse_nmf_mex", "type-precision-long", "snmf:type", 1, (V, W0, H0, 5.0, dict(OPTS, precision="fp64-but-much-too-long"))),
    ("sparse_nmf_mex", "unsupported-fp64-devices", "snmf:unsupported", 1, (V, W0, H0, 5.0, dict(OPTS, precision="fp64", devices=[0.0, 0.0]))),
    # ---- snmf_mdi_mex(v, mask, w0, h0, sparsity, opts)
    ("snmf_mdi_mex", "nargin", "snmf:nargin", 1, (V, V > .5, W0, H0, 0.0)),
    ("snmf_mdi_mex", "nargout", "snmf:nargout", 7, (V, V * 0 + 1, W0, H0, 0.0, OPTS)),
    ("snmf_mdi_mex", "type-mask-logical", "snmf:type", 1, (V, V > .5, W0, H0, 0.0, OPTS)),
    ("snmf_mdi_mex", "type-v-single", "snmf:type", 1, (f32(V), V * 0 + 1, W0, H0, 0.0, OPTS)),
    ("snmf_mdi_mex", "type-w0-single", "snmf:type", 1, (V, V * 0 + 1, f32(W0), H0, 0.0, OPTS)),
    ("snmf_mdi_mex", "type-h0-single", "snmf:type", 1, (V, V * 0 + 1, W0, f32(H0), 0.0, OPTS)),
    ("snmf_mdi_mex", "type-sparsity-struct", "snmf:type", 1, (V, V * 0 + 1, W0, H0, {"a": 1.0}, OPTS)),
    ("snmf_mdi_mex", "type-opts", "snmf:type", 1, (V, V * 0 + 1, W0, H0, 0.0, "opts")),
    ("snmf_mdi_mex", "dim-mask", "snmf:dim", 1, (V, V.T * 0 + 1, W0, H0, 0.0, OPTS)),
    ("snmf_mdi_mex", "dim-w0", "snmf:dim", 1, (V, V * 0 + 1, W0[1:], H0, 0.0, OPTS)),
    ("snmf_mdi_mex", "dim-h0", "snmf:dim", 1, (V, V * 0 + 1, W0, H0[:, 1:], 0.0, OPTS)),
    ("snmf_mdi_mex", "dim-sparsity-vector", "snmf:dim", 1, (V, V * 0 + 1, W0, H0, np.ones(R), OPTS)),
    ("snmf_mdi_mex", "dim-mask-ind", "snmf:dim", 1, (V, V * 0 + 1, W0, H0, 0.0, dict(OPTS, w_update_ind=np.ones(R + 2, bool)))),
    ("snmf_mdi_mex", "type-mask-ind-single", "snmf:type", 1, (V, V * 0 + 1, W0, H0, 0.0, dict(OPTS, h_update_ind=f32(np.ones(R))))),
    # ---- snmf_frontend_mex('stft', s, p, DC_bin) / ('mel', TF_mag, melmat, K[, precision])
    ("snmf_frontend_mex", "nargin-none", "snmf:nargin", 1, ()),
    ("snmf_frontend_mex", "nargin-not-char", "snmf:nargin", 1, (1.0, S, P, 1.0)),
    ("snmf_frontend_mex", "nargout", "snmf:nargout", 2, ("stft", S, P, 1.0)),
    ("snmf_frontend_mex", "cmd", "snmf:cmd", 1, ("istft", S, P, 1.0)),
    ("snmf_frontend_mex", "nargin-stft", "snmf:nargin", 1, ("stft", S, P)),
    ("snmf_frontend_mex", "nargin-stft-p", "snmf:nargin", 1, ("stft", S, 1.0, 1.0)),
    ("snmf_frontend_mex", "type-s-single", "snmf:type", 1, ("stft", f32(S), P, 1.0)),
    ("snmf_frontend_mex", "type-s-single-fp64", "snmf:type", 1, ("stft", f32(S), dict(P, snmf_precision="fp64"), 1.0)),
    ("snmf_frontend_mex", "type-precision-other", "snmf:type", 1, ("stft", S, dict(P, snmf_precision="double"), 1.0)),
    ("snmf_frontend_mex", "type-precision-number", "snmf:type", 1, ("stft", S, dict(P, snmf_precision=1.0), 1.0)),
    ("snmf_frontend_mex", "field-win-absent", "snmf:field", 1, ("stft", S, without(P, "win_STFT"), 1.0)),
    ("snmf_frontend_mex", "field-win-single", "snmf:field", 1, ("stft", S, dict(P, win_STFT=f32(WIN)), 1.0)),
    ("snmf_frontend_mex", "field-framelength", "snmf:field", 1, ("stft", S, without(P, "framelength"), 1.0)),
    ("snmf_frontend_mex", "field-pow-empty", "snmf:field", 1, ("stft", S, dict(P, pow=None), 1.0)),
    ("snmf_frontend_mex", "dim-win", "snmf:dim", 1, ("stft", S, dict(P, win_STFT=WIN[:-1]), 1.0)),
    ("snmf_frontend_mex", "dim-s-matrix", "snmf:dim", 1, ("stft", S.reshape(2, -1), P, 1.0)),
    ("snmf_frontend_mex", "dim-dcbin-empty", "snmf:dim", 1, ("stft", S, P, None)),
    ("snmf_frontend_mex", "nargin-mel-3", "snmf:nargin", 1, ("mel", np.ones((NB, 4)), MEL)),
    ("snmf_frontend_mex", "nargin-mel-6", "snmf:nargin", 1, ("mel", np.ones((NB, 4)), MEL, 1.0, "fp32", 0.0)),
    ("snmf_frontend_mex", "type-tfmag-single", "snmf:type", 1, ("mel", f32(np.ones((NB, 4))), MEL, 1.0)),
    ("snmf_frontend_mex", "type-tfmag-single-fp64", "snmf:type", 1, ("mel", f32(np.ones((NB, 4))), MEL, 1.0, "fp64")),
    ("snmf_frontend_mex", "type-melmat-single", "snmf:type", 1, ("mel", np.ones((NB, 4)), f32(MEL), 1.0)),
    ("snmf_frontend_mex", "type-mel-precision", "snmf:type", 1, ("mel", np.ones((NB, 4)), MEL, 1.0, "fp8")),
    ("snmf_frontend_mex", "dim-mel-rows", "snmf:dim", 1, ("mel", np.ones((NB + 1, 4)), MEL, 1.0)),
    ("snmf_frontend_mex", "dim-mel-transposed", "snmf:dim", 1, ("mel", np.ones((NB, 4)), MEL.T, 1.0)),
    ("snmf_frontend_mex", "dim-mel-K", "snmf:dim", 1, ("mel", np.ones((3 * NB, 4)), MEL, 2.0)),
    ("snmf_frontend_mex", "dim-mel-K0", "snmf:dim", 1, ("mel", np.ones((NB, 4)), MEL, 0.0)),
    ("snmf_frontend_mex", "dim-mel-K-empty", "snmf:dim", 1, ("mel", np.ones((NB, 4)), MEL, None)),
    ("snmf_frontend_mex", "dim-melmat-empty", "snmf:dim", 1, ("mel", np.ones((0, 4)), np.zeros((7, 0)), 1.0)),
    # ---- snmf_dnmf_mex
    ("snmf_dnmf_mex", "nargin-none", "snmf:nargin", 1, ()),
    ("snmf_dnmf_mex", "nargin-not-char", "snmf:nargin", 1, (P,)),
    ("snmf_dnmf_mex", "cmd", "snmf:cmd", 1, ("adapt", S, S)),
    ("snmf_dnmf_mex", "nargin-nframes", "snmf:nargin", 1, ("nframes", 100.0)),
    ("snmf_dnmf_mex", "nargin-nframes-p", "snmf:nargin", 1, ("nframes", 100.0, 3.0)),
    ("snmf_dnmf_mex", "field-nframes-frameshift", "snmf:field", 1, ("nframes", 100.0, without(P, "frameshift"))),
    ("snmf_dnmf_mex", "field-nframes-win", "snmf:field", 1, ("nframes", 100.0, dict(P, win_STFT=WIN[:10]))),
    ("snmf_dnmf_mex", "dim-nframes-n-empty", "snmf:dim", 1, ("nframes", None, P)),
    ("snmf_dnmf_mex", "nargin-dnmf", "snmf:nargin", 1, ("dnmf", S, S, B_D, None, P)),
    ("snmf_dnmf_mex", "nargin-dnmf-p", "snmf:nargin", 1, ("dnmf", S, S, B_D, None, 1.0, None)),
    ("snmf_dnmf_mex", "type-dnmf-precision", "snmf:type", 1, ("dnmf", S, S, B_D, None, dict(P, snmf_precision="fp65"), None)),
    ("snmf_dnmf_mex", "type-dnmf-x-single", "snmf:type", 1, ("dnmf", f32(S), S, B_D, None, P, None)),
    ("snmf_dnmf_mex", "type-dnmf-d-single-fp64", "snmf:type", 1, ("dnmf", S, f32(S), B_D, None, dict(P, snmf_precision="fp64"), None)),
    ("snmf_dnmf_mex", "dim-dnmf-x-matrix", "snmf:dim", 1, ("dnmf", S.reshape(-1, 2), S, B_D, None, P, None)),
    ("snmf_dnmf_mex", "dim-dnmf-d-matrix", "snmf:dim", 1, ("dnmf", S, S.reshape(2, -1), B_D, None, P, None)),
    ("snmf_dnmf_mex", "field-dnmf-DCbin", "snmf:field", 1, ("dnmf", S, S, B_D, None, without(P, "DCbin"), None)),
    ("snmf_dnmf_mex", "field-dnmf-win", "snmf:field", 1, ("dnmf", S, S, B_D, None, dict(P, win_STFT=WIN[1:]), None)),
    ("snmf_dnmf_mex", "dim-dnmf-melmat-cols", "snmf:dim", 1, ("dnmf", S, S, B_M, None, P, MEL[:, :-1])),
    ("snmf_dnmf_mex", "dim-dnmf-melmat-transposed", "snmf:dim", 1, ("dnmf", S, S, B_M, None, P, MEL.T)),
    ("snmf_dnmf_mex", "dim-dnmf-melmat-single", "snmf:dim", 1, ("dnmf", S, S, B_M, None, P, f32(MEL))),
    ("snmf_dnmf_mex", "field-dnmf-R_x", "snmf:field", 1, ("dnmf", S, S, B_D, None, without(P, "R_x"), None)),
    ("snmf_dnmf_mex", "field-dnmf-cost_check", "snmf:field", 1, ("dnmf", S, S, B_D, None, without(P, "cost_check"), None)),
    ("snmf_dnmf_mex", "dim-dnmf-sparsity", "snmf:dim", 1, ("dnmf", S, S, B_D, None, dict(P, sparsity=np.ones(5)), None)),
    ("snmf_dnmf_mex", "dim-dnmf-B-rows", "snmf:dim", 1, ("dnmf", S, S, B_D[:-1], None, P, None)),
    ("snmf_dnmf_mex", "dim-dnmf-B-is-Mel", "snmf:dim", 1, ("dnmf", S, S, B_M, None, P, None)),
    ("snmf_dnmf_mex", "dim-dnmf-B-cols", "snmf:dim", 1, ("dnmf", S, S, B_D[:, :-1], None, P, None)),
    ("snmf_dnmf_mex", "dim-dnmf-H0", "snmf:dim", 1, ("dnmf", S, S, B_D, np.ones((5, T_S + 1)), P, None)),
    ("snmf_dnmf_mex", "dim-dnmf-H0-transposed", "snmf:dim", 1, ("dnmf", S, S, B_D, np.ones((T_S, 5)), P, None)),
    ("snmf_dnmf_mex", "field-dnmf-seed", "snmf:field", 1, ("dnmf", S, S, B_D, None, dict(P, random_seed=0.0), None)),
    ("snmf_dnmf_mex", "nargin-multi", "snmf:nargin", 1, ("dnmf_multi", V, V, V, W0, None, P)),
    ("snmf_dnmf_mex", "unsupported-multi-fp64", "snmf:unsupported", 1, ("dnmf_multi", V, V, V, W0[:, :5], None, dict(P, snmf_precision="fp64"), [0.0])),
    ("snmf_dnmf_mex", "dim-multi-X", "snmf:dim", 1, ("dnmf_multi", V, V[:, 1:], V, np.ones((F, 5)), None, P, [0.0])),
    ("snmf_dnmf_mex", "dim-multi-D-single", "snmf:dim", 1, ("dnmf_multi", V, V, f32(V), np.ones((F, 5)), None, P, [0.0])),
    ("snmf_dnmf_mex", "dim-multi-B", "snmf:dim", 1, ("dnmf_multi", V, V, V, np.ones((F, 4)), None, P, [0.0])),
    ("snmf_dnmf_mex", "dim-multi-H0", "snmf:dim", 1, ("dnmf_multi", V, V, V, np.ones((F, 5)), np.ones((5, T + 1)), P, [0.0])),
    ("snmf_dnmf_mex", "dim-multi-devices-empty", "snmf:dim", 1, ("dnmf_multi", V, V, V, np.ones((F, 5)), np.ones((5, T)), P, None)),
    ("snmf_dnmf_mex", "dim-multi-devices-17", "snmf:dim", 1, ("dnmf_multi", V, V, V, np.ones((F, 5)), np.ones((5, T)), P, np.zeros(17))),
    ("snmf_dnmf_mex", "field-multi-seed", "snmf:field", 1, ("dnmf_multi", V, V, V, np.ones((F, 5)), None, dict(P, random_seed=-1.0), [0.0])),
    ("snmf_dnmf_mex", "nargin-train", "snmf:nargin", 1, ("train", S, [1.0, 2.0], None, P, MEL)),
    ("snmf_dnmf_mex", "type-train-s-single", "snmf:type", 1, ("train", f32(S), [1.0, 2.0], None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-s-matrix", "snmf:dim", 1, ("train", S.reshape(-1, 2), [1.0, 2.0], None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-dcbin-empty", "snmf:dim", 1, ("train", S, [1.0, 2.0], None, P, MEL, None)),
    ("snmf_dnmf_mex", "dim-train-melmat-absent", "snmf:dim", 1, ("train", S, [1.0, 2.0], None, P, None, 1.0)),
    ("snmf_dnmf_mex", "dim-train-idx-empty", "snmf:dim", 1, ("train", S, None, None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-idx-int32", "snmf:dim", 1, ("train", S, np.array([1, 2], np.int32), None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-idx-zero", "snmf:dim", 1, ("train", S, [0.0, 2.0], None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-idx-past-end", "snmf:dim", 1, ("train", S, [1.0, T_S + 1.0], None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-idx-fraction", "snmf:dim", 1, ("train", S, [1.5, 2.0], None, P, MEL, 1.0)),
    ("snmf_dnmf_mex", "dim-train-H0", "snmf:dim", 1, ("train", S, [1.0, 2.0], np.ones((3, T_S)), P, MEL, 1.0)),
    ("snmf_dnmf_mex", "field-train-alpha_eta", "snmf:field", 1, ("train", S, [1.0, 2.0], np.ones((2, T_S)), dict(P, domain_DD=1.0), MEL, 1.0)),
    ("snmf_dnmf_mex", "field-train-seed", "snmf:field", 1, ("train", S, [1.0, 2.0], None, dict(P, random_seed=0.5), MEL, 1.0)),
    # ---- snmf_online_mex
    ("snmf_online_mex", "usage-none", "snmf:usage", 1, ()),
    ("snmf_online_mex", "usage-not-char", "snmf:usage", 1, (1.0,)),
    ("snmf_online_mex", "usage-unknown", "snmf:usage", 1, ("reset", 1.0)),
    ("snmf_online_mex", "nargout", "snmf:nargout", 2, ("create", BX, BD, OH0, AD, OP)),
    ("snmf_online_mex", "usage-create", "snmf:usage", 1, ("create", BX, BD, OH0, OP)),
    ("snmf_online_mex", "usage-set_mel", "snmf:usage", 1, ("set_mel", 1.0, MEL, B_M[:, :3], B_M[:, :2])),
    ("snmf_online_mex", "usage-process", "snmf:usage", 1, ("process", 1.0, S)),
    ("snmf_online_mex", "usage-basis", "snmf:usage", 1, ("basis", 1.0, 33.0)),
    ("snmf_online_mex", "usage-destroy", "snmf:usage", 1, ("destroy",)),
    ("snmf_online_mex", "type-p", "snmf:type", 1, ("create", BX, BD, OH0, AD, 1.0)),
    ("snmf_online_mex", "precision-other", "snmf:precision", 1, ("create", BX, BD, OH0, AD, dict(OP, precision="fp16"))),
    ("snmf_online_mex", "precision-number", "snmf:precision", 1, ("create", BX, BD, OH0, AD, dict(OP, precision=64.0))),
    ("snmf_online_mex", "precision-long", "snmf:precision", 1, ("create", BX, BD, OH0, AD, dict(OP, precision="fp64fp64"))),
    ("snmf_online_mex", "unsupported-splice", "snmf:unsupported", 1, ("create", BX, BD, OH0, AD, dict(OP, Splice=1.0))),
    ("snmf_online_mex", "unsupported-blk_len", "snmf:unsupported", 1, ("create", BX, BD, OH0, AD, dict(OP, blk_len_sep=2.0))),
    ("snmf_online_mex", "unsupported-mode", "snmf:unsupported", 1, ("create", BX, BD, OH0, AD, dict(OP, B_sep_mode="MFCC"))),
    ("snmf_online_mex", "field-fftlength", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "fftlength"))),
    ("snmf_online_mex", "field-framelength", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "framelength"))),
    ("snmf_online_mex", "field-frameshift", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "frameshift"))),
    ("snmf_online_mex", "field-DCbin", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "DCbin"))),
    ("snmf_online_mex", "field-delay", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "delay"))),
    ("snmf_online_mex", "field-overlapscale", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "overlapscale"))),
    ("snmf_online_mex", "field-cost_check", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "cost_check"))),
    ("snmf_online_mex", "field-win_ISTFT", "snmf:field", 1, ("create", BX, BD, OH0, AD, without(OP, "win_ISTFT"))),
    ("snmf_online_mex", "type-Bx-single", "snmf:type", 1, ("create", f32(BX), BD, OH0, AD, OP)),
    ("snmf_online_mex", "type-win-single", "snmf:type", 1, ("create", BX, BD, OH0, AD, dict(OP, win_STFT=f32(WIN)))),
    ("snmf_online_mex", "type-Ad-logical-no-adapt", "snmf:type", 1, ("create", BX, BD, OH0, AD > .5, dict(OP, adapt_train_N=0.0))),
    ("snmf_online_mex", "dim-Bx-rows", "snmf:dim", 1, ("create", BX[:-1], BD, OH0, AD, OP)),
    ("snmf_online_mex", "dim-Bd-rows", "snmf:dim", 1, ("create", BX, np.vstack([BD, BD[:1]]), OH0, AD, OP)),
    ("snmf_online_mex", "dim-Bd-empty", "snmf:dim", 1, ("create", BX, np.zeros((NB, 0)), OH0[:3], AD, OP)),
    ("snmf_online_mex", "dim-fftlength-vs-bases", "snmf:dim", 1, ("create", BX, BD, OH0, AD, dict(OP, fftlength=128.0))),
    ("snmf_online_mex", "dim-H0-short", "snmf:dim", 1, ("create", BX, BD, OH0[:-1], AD, OP)),
    ("snmf_online_mex", "dim-H0-long", "snmf:dim", 1, ("create", BX, BD, np.ones(6), AD, OP)),
    ("snmf_online_mex", "dim-Ad-transposed", "snmf:dim", 1, ("create", BX, BD, OH0, AD.T, OP)),
    ("snmf_online_mex", "dim-Ad-empty-with-adapt", "snmf:dim", 1, ("create", BX, BD, OH0, None, OP)),
    ("snmf_online_mex", "dim-win_STFT", "snmf:dim", 1, ("create", BX, BD, OH0, AD, dict(OP, win_STFT=WIN[:-1]))),
    ("snmf_online_mex", "dim-win_ISTFT", "snmf:dim", 1, ("create", BX, BD, OH0, AD, dict(OP, win_ISTFT=np.ones(N_FFT + 16)))),
    ("snmf_online_mex", "dim-framelength-vs-windows", "snmf:dim", 1, ("create", BX, BD, OH0, AD, dict(OP, framelength=48.0))),
    ("snmf_online_mex", "handle-process-0", "snmf:handle", 1, ("process", 0.0, S, 1.0)),
    ("snmf_online_mex", "handle-process-99", "snmf:handle", 1, ("process", 99.0, S, 1.0)),
    ("snmf_online_mex", "handle-process-nan", "snmf:handle", 1, ("process", float("nan"), S, 1.0)),
    ("snmf_online_mex", "handle-process-negative", "snmf:handle", 1, ("process", -1.0, S, 1.0)),
    ("snmf_online_mex", "handle-process-empty", "snmf:handle", 1, ("process", None, S, 1.0)),
    ("snmf_online_mex", "handle-basis", "snmf:handle", 1, ("basis", 1e9, 33.0, 2.0)),
    ("snmf_online_mex", "handle-set_mel", "snmf:handle", 1, ("set_mel", 0.5, MEL, B_M[:, :3], B_M[:, :2], 1.0)),
]
assert len({(s, n) for s, n, *_ in VALIDATION}) == len(VALIDATION)


@pytest.mark.parametrize("shim,case,want,nlhs,args", VALIDATION, ids=[f"{s.replace('_mex', '').replace('snmf_', '')}-{n}" for s, n, *_ in VALIDATION])
def test_validation(mex_shims, shim, case, want, nlhs, args):
    """A wrong call is refused with the id of its kind before any device work: these run where there is no device, and the
    shim has made no context (nothing locked) when it raises."""
    m = mex_shims[shim]
    locks = m.lock_count()
    with pytest.raises(MexError) as e:
        m(nlhs, *args)
    assert e.value.id == want, (e.value.id, e.value.msg)
    assert e.value.msg and "%" not in e.value.msg, e.value.msg
    assert m.lock_count() == locks, "an argument error must come before the device context is made"


def test_online_destroy_of_no_handle_is_a_no_op(mex_shims):
    for h in (0.0, 5.0, -3.0, float("nan")):
        mex_shims["snmf_online_mex"](0, "destroy", h)


def test_frontend_mel_without_frames(mex_shims):
    """T = 0: K*M x 0 in both precisions, without the device (the fp32 path used to fail in the library: T < 1)."""
    for extra in ((), ("fp32",), ("fp64",)):
        (o,) = mex_shims["snmf_frontend_mex"](1, "mel", np.zeros((3 * NB, 0)), MEL, 3.0, *extra)
        assert o.shape == (21, 0) and o.dtype == np.float64


FRAME_GRID = [(n, fl, fs, nfft) for (fl, fs, nfft) in ((64, 16, 64), (640, 160, 1024), (48, 16, 64), (100, 37, 128))
              for n in (0, 1, fl - 1, fl, nfft, nfft + 1, nfft + 2, nfft + fs + 1, nfft + fs + 2, 3001, 16000)]


@pytest.mark.parametrize("n,fl,fs,nfft", FRAME_GRID)
def test_nframes_matches_the_binding(mex_shims, n, fl, fs, nfft):
    """snmf_dnmf_mex('nframes', n, p) is frontend.num_frames(n, p): what integration/*.m size H0 and sample_idx by."""
    p = dict(P, framelength=float(fl), frameshift=float(fs), fftlength=float(nfft), win_STFT=np.ones(fl))
    (o,) = mex_shims["snmf_dnmf_mex"](1, "nframes", float(n), p)
    assert o.shape == (1, 1) and o[0, 0] == frontend.num_frames(n, dict(p, DCbin=1))
    if n <= nfft + 1:
        assert o[0, 0] == 0


REACHES_DEVICE = [
    ("sparse_nmf_mex", (V, W0, H0, 5.0, OPTS)),
    ("snmf_mdi_mex", (V, (V > .3) * 1.0, W0, H0, 0.0, OPTS)),
    ("snmf_frontend_mex", ("stft", S, P, 1.0)),
    ("snmf_frontend_mex", ("mel", np.ones((NB, 4)), MEL, 1.0)),
    ("snmf_dnmf_mex", ("dnmf", S, S, B_D, None, P, None)),
    ("snmf_dnmf_mex", ("train", S, [1.0, 2.0], None, dict(P, F_order=7.0), MEL, 1.0)),
    ("snmf_online_mex", ("create", BX, BD, OH0, AD, OP)),
]


@pytest.mark.parametrize("shim,args", REACHES_DEVICE, ids=[f"{s}-{a[0] if isinstance(a[0], str) else 'solve'}" for s, a in REACHES_DEVICE])
def test_no_device_is_an_error_not_a_crash(mex_shims, lib, shim, args):
    if lib.snmf_device_count() > 0:
        pytest.skip("a device is present: the same calls run in tests/test_gpu_mex.py")
    m = mex_shims[shim]
    with pytest.raises(MexError) as e:
        m(1, *args)
    assert e.value.id == "snmf:device", (e.value.id, e.value.msg)
    assert m.lock_count() == 0 and not m.has_exit_fcn()


# ---- the MATLAB wrappers: call arity -------------------------------------------------------------------------------------
def top_level_args(text):
    """Number of top-level comma-separated arguments of the call whose text (between its parentheses) is `text`."""
    if not text.strip():
        return 0
    depth, n, in_str = 0, 1, False
    for i, c in enumerate(text):
        if in_str:
            in_str = c != "'"
        elif c == "'" and (i == 0 or not (text[i - 1].isalnum() or text[i - 1] in ")]}_.'")):  # a quote, not a transpose
            in_str = True
        elif c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
        elif c == "," and depth == 0:
            n += 1
    return n


def matlab_call_sites():
    """(file, line, shim, command or None, number of arguments) of every NAME_mex( ... ) call in integration/*.m."""
    sites = []
    for path in sorted(glob.glob(os.path.join(ROOT, "integration", "*.m"))):
        src = open(path).read()
        code = "\n".join(line if line.lstrip()[:1] != "%" else "" for line in src.split("\n"))
        for mt in re.finditer(r"\b(\w+_mex)\(", code):
            i, depth, in_str = mt.end(), 1, False
            while depth:
                c = code[i]
                if in_str:
                    in_str = c != "'"
                elif c == "'" and not (code[i - 1].isalnum() or code[i - 1] in ")]}_.'"):
                    in_str = True
                elif c in "([{":
                    depth += 1
                elif c in ")]}":
                    depth -= 1
                i += 1
            text = code[mt.end():i - 1]
            cmd = re.match(r"\s*'(\w+)'", text)
            sites.append((os.path.basename(path), code[:mt.start()].count("\n") + 1, mt.group(1), cmd.group(1) if cmd else None,
                          top_level_args(text)))
    return sites


def shim_arity(shim, cmd):
    """The nrhs values the shim's own test accepts for `cmd` (None: the shim has no commands), read from its source."""
    src = open(os.path.join(ROOT, "integration", shim + ".cpp")).read()
    if cmd is None:
        body = src[src.index("void mexFunction"):]
    else:
        mt = re.search(r'(strcmp\(cmd, "%s"\)|std::string\(cmd\) == "%s")' % (cmd, cmd), src)
        assert mt, f"{shim} has no command '{cmd}'"
        body = src[mt.end():]
    test = re.search(r"if \((nrhs != \d+[^)]*)\)", body)
    return {int(v) for v in re.findall(r"nrhs != (\d+)", test.group(1))}


def test_top_level_args_counter():
    assert top_level_args("") == 0 and top_level_args("x") == 1
    assert top_level_args("'stft', x(:) + d(:), p, p.DCbin") == 4
    assert top_level_args("'dnmf_multi', Y, X, D, double(B), H0, p, double(p.snmf_devices(:)')") == 8
    assert top_level_args("'basis', h, size(B_DFT_d,1), size(B_DFT_d,2)") == 4
    assert top_level_args("'a,b', [1, 2; 3, 4], {5, 6}, x'") == 4
    assert shim_arity("sparse_nmf_mex", None) == {5} and shim_arity("snmf_mdi_mex", None) == {6}
    assert shim_arity("snmf_frontend_mex", "mel") == {4, 5} and shim_arity("snmf_online_mex", "set_mel") == {6}


SITES = matlab_call_sites()


def test_every_matlab_call_site_is_found():
    """All *_mex calls of integration/*.m: 15 sites, every shim with a wrapper and every command a wrapper uses."""
    assert len(SITES) == 15, SITES
    assert {(s, c) for _, _, s, c, _ in SITES} == {
        ("sparse_nmf_mex", None), ("snmf_online_mex", "create"), ("snmf_online_mex", "process"), ("snmf_online_mex", "basis"),
        ("snmf_online_mex", "destroy"), ("snmf_dnmf_mex", "nframes"), ("snmf_dnmf_mex", "train"), ("snmf_dnmf_mex", "dnmf"),
        ("snmf_dnmf_mex", "dnmf_multi"), ("snmf_frontend_mex", "stft")}


@pytest.mark.parametrize("site", SITES, ids=[f"{f}:{ln}" for f, ln, *_ in SITES])
def test_matlab_call_arity(site):
    """The number of arguments at the call site is one the shim's nrhs test accepts for that command."""
    fname, line, shim, cmd, nargs = site
    assert shim in SHIMS
    assert nargs in shim_arity(shim, cmd), f"{fname}:{line}: {shim}('{cmd}', ...) is called with {nargs} arguments"
