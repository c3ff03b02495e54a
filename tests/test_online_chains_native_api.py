"""The chain driver behind the C ABI (snmf_online_batch_out_capacity, snmf_online_batch_run_chains_f32 / _f64) and its
MEX shim integration/snmf_online_batch_mex.cpp, as far as both are decided without a device: the symbols and their
argtypes, the NULL-handle answers, the shim compiled and linked with the test host, and for every command of the shim
the refusals that come before the device is touched -- a wrong number of arguments, a wrong class, a wrong size, a count
vector that does not sum to the PCM it describes.  What the device computes is tests/test_gpu_online_chains_native.py.

Commands on a handle ('set_mel', 'process', 'restart', 'basis', 'mel_basis', 'chains') check what does not depend on the
handle first (argument count, classes, counts that must add up), then the handle, then the sizes the handle fixes.  No
handle exists without a device, so here the first group is asserted by its identifier and the handle check by
snmf:handle; the sizes a handle fixes are asserted on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mexhost
from mexhost import MexError
from se_snmf_nat_amd import _lib

NAME = "snmf_online_batch_mex"
NEW = ("snmf_online_batch_out_capacity", "snmf_online_batch_run_chains_f32", "snmf_online_batch_run_chains_f64")


@pytest.fixture(scope="module")
def shim(tmp_path_factory, lib):
    m = mexhost.Mex(mexhost.build_shim(NAME, tmp_path_factory.mktemp("batch_mex")))
    yield m
    m.unload()


def test_symbols_are_bound_with_argtypes(lib):
    assert lib.snmf_abi_version() == 5  # added within 5
    for name in NEW:
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (2 if name.endswith("capacity") else 15), name
    assert lib.snmf_online_batch_out_capacity.restype is C.c_int64
    assert lib.snmf_online_batch_run_chains_f32.restype is C.c_int


def test_null_handle(lib):
    for n in (0, 1, 160, 10 ** 9):
        assert lib.snmf_online_batch_out_capacity(None, n) == 0
    for name in NEW[1:]:
        assert getattr(lib, name)(None, 0, None, None, None, None, None, None, None, 0, None, None, None, None, None) == 1  # SNMF_ERR_INVALID
        assert b"NULL" in lib.snmf_last_error()


def test_shim_compiles_and_links(shim):
    """g++ -std=c++17 -Wall -Werror of the shim + host against libsnmf_hip.so (one library in the process: mexhost.Mex)."""
    assert shim.live_arrays() == 0 and not shim.has_exit_fcn()  # no context was made


def test_scheduler_against_a_simulated_batch_under_sanitizers(tmp_path):
    """tests/chains_host/chains_sim_main.cpp: csrc/snmf_online_batch_chains.h alone, as a stand-alone host program built with
    the address and undefined-behaviour sanitizers, on 400 seeded corpora with chunk_hops from 0 to INT32_MAX.  A scratch
    buffer sized by chunk_hops instead of by the files would end this program (hundreds of GB); an index or a count that is
    off by one is caught by the sanitizer or by the sample-by-sample comparison."""
    exe = str(tmp_path / "chains_sim")
    src = os.path.join(mexhost.HOST_DIR, "..", "chains_host", "chains_sim_main.cpp")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(mexhost.ROOT, "include"), "-I" + os.path.join(mexhost.ROOT, "se_snmf_nat_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "400 simulated corpora ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


# ---- argument checks -------------------------------------------------------------------------------------------------------
_rs = np.random.RandomState(5)
NB, RX, RD, RA, MA, S = 33, 5, 4, 3, 4, 2
WIN = np.sqrt(np.hanning(65)[:64])
P = dict(framelength=64.0, frameshift=16.0, fftlength=64.0, DCbin=1.0, Splice=0.0, preemph=0.0, pow=2.0, nonzerofloor=1e-9, win_STFT=WIN,
         win_ISTFT=WIN, overlapscale=0.5, delay=3.0, cf="kl", sparsity=5.0, max_iter=3.0, conv_eps=0.0, cost_check=1.0, adapt_train_N=1.0,
         R_a=float(RA), m_a=float(MA))
BX, BD, H0, AD = _rs.rand(NB, RX) + .1, _rs.rand(NB, RD) + .1, _rs.rand(RX + RD, 1), _rs.rand(RA, MA)
BDS, H0S, ADS = _rs.rand(NB, RD * S) + .1, _rs.rand(RX + RD, S), _rs.rand(RA, MA * S)
MEL, BMX, BMD = _rs.rand(12, NB), _rs.rand(12, RX), _rs.rand(12, RD)
PCM = _rs.randn(100)
f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
without = lambda d, *keys: {k: v for k, v in d.items() if k not in keys}  # noqa: E731
H = 1.0  # a handle that was never made

# (case, expected id, nlhs, args): every path that is decided before the device
CASES = [
    ("usage-no-command", "snmf:usage", 1, ()),
    ("usage-command-not-char", "snmf:usage", 1, (1.0,)),
    ("usage-unknown", "snmf:usage", 1, ("resume", H)),
    # ---- create: B_DFT_x, B_DFT_d, H0, Ad_blk0, p, S
    ("create-nrhs", "snmf:usage", 1, ("create", BX, BD, H0, AD, P)),
    ("create-nlhs", "snmf:nargout", 2, ("create", BX, BD, H0, AD, P, float(S))),
    ("create-p-not-struct", "snmf:type", 1, ("create", BX, BD, H0, AD, 1.0, float(S))),
    ("create-precision", "snmf:precision", 1, ("create", BX, BD, H0, AD, dict(P, precision="fp16"), float(S))),
    ("create-field-fftlength", "snmf:field", 1, ("create", BX, BD, H0, AD, without(P, "fftlength"), float(S))),
    ("create-field-cost_check", "snmf:field", 1, ("create", BX, BD, H0, AD, without(P, "cost_check"), float(S))),
    ("create-field-windows", "snmf:field", 1, ("create", BX, BD, H0, AD, without(P, "win_ISTFT"), float(S))),
    ("create-S-zero", "snmf:dim", 1, ("create", BX, BD, H0, AD, P, 0.0)),
    ("create-S-fraction", "snmf:dim", 1, ("create", BX, BD, H0, AD, P, 1.5)),
    ("create-S-vector", "snmf:dim", 1, ("create", BX, BD, H0, AD, P, np.ones(2))),
    ("create-S-single", "snmf:type", 1, ("create", BX, BD, H0, AD, P, f32(2))),
    ("create-Bx-single", "snmf:type", 1, ("create", f32(BX), BD, H0, AD, P, float(S))),
    ("create-Bd-single", "snmf:type", 1, ("create", BX, f32(BD), H0, AD, P, float(S))),
    ("create-H0-single", "snmf:type", 1, ("create", BX, BD, f32(H0), AD, P, float(S))),
    ("create-Ad-logical", "snmf:type", 1, ("create", BX, BD, H0, AD > .5, P, float(S))),
    ("create-window-single", "snmf:type", 1, ("create", BX, BD, H0, AD, dict(P, win_STFT=f32(WIN)), float(S))),
    ("create-Bx-rows", "snmf:dim", 1, ("create", BX[:-1], BD, H0, AD, P, float(S))),
    ("create-Bd-rows", "snmf:dim", 1, ("create", BX, BD[:-1], H0, AD, P, float(S))),
    ("create-Bd-neither-one-nor-S", "snmf:dim", 1, ("create", BX, np.tile(BD, (1, 3)), H0, AD, P, float(S))),
    ("create-H0-row-vector", "snmf:dim", 1, ("create", BX, BD, H0.T, AD, P, float(S))),
    ("create-H0-too-short-for-R_x", "snmf:dim", 1, ("create", BX, BD, H0[:RX], AD, P, float(S))),
    ("create-H0-three-columns", "snmf:dim", 1, ("create", BX, BD, np.tile(H0, (1, 3)), AD, P, float(S))),
    ("create-Ad-shape", "snmf:dim", 1, ("create", BX, BD, H0, AD.T, P, float(S))),
    ("create-Ad-empty-but-adapting", "snmf:dim", 1, ("create", BX, BD, H0, None, P, float(S))),
    ("create-window-length", "snmf:dim", 1, ("create", BX, BD, H0, AD, dict(P, win_ISTFT=WIN[:-1]), float(S))),
    ("create-unsupported-splice", "snmf:unsupported", 1, ("create", BX, BD, H0, AD, dict(P, Splice=1.0), float(S))),
    # ---- set_mel: handle, melmat, B_Mel_x, B_Mel_d, MelConv
    ("set_mel-nrhs", "snmf:usage", 1, ("set_mel", H, MEL, BMX, BMD)),
    ("set_mel-melmat-single", "snmf:type", 1, ("set_mel", H, f32(MEL), BMX, BMD, 1.0)),
    ("set_mel-BMx-single", "snmf:type", 1, ("set_mel", H, MEL, f32(BMX), BMD, 1.0)),
    ("set_mel-BMd-char", "snmf:type", 1, ("set_mel", H, MEL, BMX, "mel", 1.0)),
    ("set_mel-MelConv-vector", "snmf:dim", 1, ("set_mel", H, MEL, BMX, BMD, np.ones(2))),
    ("set_mel-no-handle", "snmf:handle", 1, ("set_mel", H, MEL, BMX, BMD, 1.0)),
    # ---- process: handle, pcm, n, flush
    ("process-nrhs", "snmf:usage", 1, ("process", H, PCM, [60.0, 40.0])),
    ("process-nlhs", "snmf:nargout", 4, ("process", H, PCM, [60.0, 40.0], [1.0, 1.0])),
    ("process-pcm-int16", "snmf:type", 1, ("process", H, PCM.astype(np.int16), [60.0, 40.0], [1.0, 1.0])),
    ("process-pcm-matrix", "snmf:dim", 1, ("process", H, PCM.reshape(10, 10), [60.0, 40.0], [1.0, 1.0])),
    ("process-n-single", "snmf:type", 1, ("process", H, PCM, f32([60, 40]), [1.0, 1.0])),
    ("process-flush-logical", "snmf:type", 1, ("process", H, PCM, [60.0, 40.0], np.array([True, True]))),
    ("process-n-negative", "snmf:dim", 1, ("process", H, PCM, [110.0, -10.0], [1.0, 1.0])),
    ("process-n-fraction", "snmf:dim", 1, ("process", H, PCM, [60.5, 39.5], [1.0, 1.0])),
    ("process-n-does-not-sum", "snmf:dim", 1, ("process", H, PCM, [60.0, 39.0], [1.0, 1.0])),
    ("process-flush-length", "snmf:dim", 1, ("process", H, PCM, [60.0, 40.0], [1.0])),
    ("process-no-handle", "snmf:handle", 1, ("process", H, PCM, [60.0, 40.0], [1.0, 1.0])),
    # ---- restart: handle, slots, B_DFT_d, H0, Ad_blk0[, B_Mel_d]
    ("restart-nrhs", "snmf:usage", 1, ("restart", H, [1.0], BD, H0)),
    ("restart-nrhs-long", "snmf:usage", 1, ("restart", H, [1.0], BD, H0, AD, BMD, 1.0)),
    ("restart-slots-single", "snmf:type", 1, ("restart", H, f32([1]), BD, H0, AD)),
    ("restart-slots-matrix", "snmf:dim", 1, ("restart", H, np.ones((2, 2)), BD, H0, AD)),
    ("restart-Bd-single", "snmf:type", 1, ("restart", H, [1.0], f32(BD), H0, AD)),
    ("restart-H0-single", "snmf:type", 1, ("restart", H, [1.0], BD, f32(H0), AD)),
    ("restart-Ad-logical", "snmf:type", 1, ("restart", H, [1.0], BD, H0, AD > .5)),
    ("restart-BMd-single", "snmf:type", 1, ("restart", H, [1.0], BD, H0, AD, f32(BMD))),
    ("restart-no-handle", "snmf:handle", 1, ("restart", H, [1.0], None, None, None)),
    # ---- basis / mel_basis: handle, k
    ("basis-nrhs", "snmf:usage", 1, ("basis", H)),
    ("basis-k-vector", "snmf:dim", 1, ("basis", H, [1.0, 2.0])),
    ("basis-k-single", "snmf:type", 1, ("basis", H, f32(1))),
    ("basis-no-handle", "snmf:handle", 1, ("basis", H, 1.0)),
    ("mel_basis-nrhs", "snmf:usage", 1, ("mel_basis", H, 1.0, 2.0)),
    ("mel_basis-k-struct", "snmf:dim", 1, ("mel_basis", H, {"k": 1.0})),
    ("mel_basis-no-handle", "snmf:handle", 1, ("mel_basis", H, 1.0)),
    # ---- chains: handle, pcm, n_samples, n_files, B_DFT_d, H0, Ad_blk0, chunk_hops[, B_Mel_d]
    ("chains-nrhs", "snmf:usage", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD)),
    ("chains-nlhs", "snmf:nargout", 5, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD, 0.0)),
    ("chains-pcm-single", "snmf:type", 1, ("chains", H, f32(PCM), [60.0, 40.0], [2.0], BD, H0, AD, 0.0)),
    ("chains-pcm-matrix", "snmf:dim", 1, ("chains", H, PCM.reshape(4, 25), [60.0, 40.0], [2.0], BD, H0, AD, 0.0)),
    ("chains-n_samples-int32", "snmf:type", 1, ("chains", H, PCM, np.array([60, 40], np.int32), [2.0], BD, H0, AD, 0.0)),
    ("chains-n_files-single", "snmf:type", 1, ("chains", H, PCM, [60.0, 40.0], f32([2]), BD, H0, AD, 0.0)),
    ("chains-Bd-single", "snmf:type", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], f32(BD), H0, AD, 0.0)),
    ("chains-H0-single", "snmf:type", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, f32(H0), AD, 0.0)),
    ("chains-Ad-single", "snmf:type", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, f32(AD), 0.0)),
    ("chains-BMd-single", "snmf:type", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD, 0.0, f32(BMD))),
    ("chains-chunk_hops-single", "snmf:type", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD, f32(0))),
    ("chains-chunk_hops-vector", "snmf:dim", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD, [1.0, 2.0])),
    ("chains-chunk_hops-negative", "snmf:dim", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD, -1.0)),
    ("chains-chunk_hops-fraction", "snmf:dim", 1, ("chains", H, PCM, [60.0, 40.0], [2.0], BD, H0, AD, 2.5)),
    ("chains-n_samples-does-not-sum", "snmf:dim", 1, ("chains", H, PCM, [60.0, 41.0], [2.0], BD, H0, AD, 0.0)),
    ("chains-n_samples-negative", "snmf:dim", 1, ("chains", H, PCM, [110.0, -10.0], [2.0], BD, H0, AD, 0.0)),
    ("chains-n_files-does-not-sum", "snmf:dim", 1, ("chains", H, PCM, [60.0, 40.0], [1.0, 2.0], BDS, H0S, ADS, 0.0)),
    ("chains-n_files-fraction", "snmf:dim", 1, ("chains", H, PCM, [60.0, 40.0], [1.5, 0.5], BDS, H0S, ADS, 0.0)),
    ("chains-no-handle", "snmf:handle", 1, ("chains", H, PCM, [60.0, 40.0], [1.0, 1.0], BDS, H0S, ADS, 0.0)),
    # ---- destroy: handle
    ("destroy-nrhs", "snmf:usage", 1, ("destroy",)),
    ("destroy-vector", "snmf:dim", 1, ("destroy", [1.0, 2.0])),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refused_before_the_device(shim, case):
    _, want, nlhs, args = case
    with pytest.raises(MexError) as e:
        shim(nlhs, *args)
    assert e.value.id == want, (e.value.id, e.value.msg)
    assert not shim.has_exit_fcn() and shim.lock_count() == 0, "a context was made: the check came after the device"
    assert shim.live_arrays() == 0


def test_every_command_is_covered():
    cmds = {c[3][0] for c in CASES if c[3] and isinstance(c[3][0], str)}
    assert {"create", "set_mel", "process", "restart", "basis", "mel_basis", "chains", "destroy"} <= cmds


@pytest.mark.parametrize("h", [0.0, 1.0, 7.0, -3.0, 2.5])
def test_destroy_of_no_handle_is_a_noop(shim, h):
    shim(0, "destroy", h)
    assert not shim.has_exit_fcn() and shim.live_arrays() == 0
