"""integration/snmf_batch_mex.cpp -- the MEX shim over the batch engines -- as far as it is decided without a device: the shim
compiled and linked with the test host under -Wall -Werror, and for every command the refusals that come before the context
is created, each judged by its identifier: a wrong number of arguments or outputs, a wrong class, a packed array one element
short or long of what its count vectors give, count vectors that disagree or hold no count, a 1-based index off either end,
a settings matrix that is not n x 4, an unknown precision, ranks or settings per problem on the fp32 engine, a transposed Mel
table, a handle that was never made.  A valid call of every command must pass all of this and stop at the device.  The same
table is replayed through a stand-alone program built with the address and undefined-behaviour sanitizers, and the MEX calls
of the wrappers under integration/batch/ are checked for their arity.  What the device computes: tests/test_gpu_batch_mex.py.

Commands on a signals handle check what does not depend on the handle first, then the handle; no handle exists without a
device, so the sizes a handle fixes ('train_signals': H0 and sample_idx against the resident lengths) are asserted on the GPU."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import dnmf_audio_batch_cases as dac
import dnmf_batch_cases as dc
import mexhost
import train_batch_cases as tc
from batch_mex_cases import COMMANDS, NAME, col, long, pack, short, side, swap, without
from mexhost import MexError
from se_snmf_nat_amd import frontend
from test_mexhost import shim_arity, top_level_args


@pytest.fixture(scope="module")
def shim(tmp_path_factory, lib):
    m = mexhost.Mex(mexhost.build_shim(NAME, tmp_path_factory.mktemp("batch_mex")))
    yield m
    m.unload()


@pytest.fixture(scope="module")
def shim_dev(tmp_path_factory, lib):
    """A second copy of the shim (state of its own) for the calls that go on to the device."""
    m = mexhost.Mex(mexhost.build_shim(NAME, tmp_path_factory.mktemp("batch_mex_dev")))
    yield m
    m.unload()


# ---- a valid call of every command ---------------------------------------------------------------------------------------
_rs = np.random.RandomState(11)
f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
N3 = 3
H = 7.0  # a handle that was never made
first = lambda a, n: np.asarray(a, dtype=np.float64).reshape(-1, order="F")[:n].copy()  # noqa: E731

# 'solve': V, T, W0, H0, p, settings
F, TS, RS = 5, [3, 4, 6], [2, 3, 1]
V = side([_rs.rand(F, T) + .1 for T in TS])
T = col(TS)
W0, H0 = side([_rs.rand(F, 2) for _ in TS]), side([_rs.rand(2, t) for t in TS])
W0M, H0M = pack([_rs.rand(F, r) for r in RS]), pack([_rs.rand(r, t) for r, t in zip(RS, TS)])
P = dict(r=2.0, cf="kl", sparsity=5.0, max_iter=4.0, conv_eps=0.0, cost_check=1.0)
P64 = dict(P, snmf_precision="fp64")
PMIX = dict(P64, r=col(RS))
ST = np.array([[1.0, 5.0, 0.0, 4.0], [2.0, 0.5, 1e-3, 3.0], [0.0, 0.1, 0.0, 2.0]])
SOLVE = ("solve", V, T, W0, H0, P, None)
SOLVE_MIX = ("solve", V, T, W0M, H0M, PMIX, None)

# 'dnmf': Y, X, D, T, B, H0, p, settings
_E = dc.edges()[:N3]
DT = col(dc.TS[:N3])
PD = dict(dc.P_EDGES, R_x=dc.R_X, R_d=dc.R_D)
PDMIX = dict(PD, R_x=col([5, 2, 3]), R_d=col([7, 1, 4]), snmf_precision="fp64")
DNMF = ("dnmf", side([e[0] for e in _E]), side([e[1] for e in _E]), side([e[2] for e in _E]), DT, side([e[3] for e in _E]),
        pack([e[4] for e in _E]), PD, None)

# 'dnmf_audio': x, n_x, d, n_d, B, H0, p, melmat, settings
_W = dac.waves()[:N3]
MEL = np.asfortranarray(frontend.mel_matrix(dac.TINY["fs"], dac.TINY["F_order"], dac.N, 1.0, dac.TINY["fs"] / 2).T)  # F_order x (N/2+1)
assert MEL.shape == (8, 33)
PA = dict(dac.P_STOP)
AUDIO = ("dnmf_audio", pack([w[0] for w in _W]), col([w[0].size for w in _W]), pack([w[1] for w in _W]), col([w[1].size for w in _W]),
         side(dac.bases()[:N3]), pack(dac.given_h0()[:N3]), PA, None, None)
AUDIO_MEL = swap(swap(AUDIO, 5, side(dac.bases(8)[:N3])), 8, MEL)

# 'train': s, n_samples, sample_idx, n_atoms, H0, p, melmat, DC_bin, settings
_S = tc.signals()[:N3]
IDX = pack(tc.sample_idx()[:N3])
PT = dict(tc.P_STOP)
TRAIN = ("train", pack(_S), col([s.size for s in _S]), IDX, float(tc.R), pack([tc.host_h0(t) for t in tc.TS[:N3]]), PT, MEL, 1.0, None)
assert tc.TS[0] in tc.sample_idx()[0], "the valid call holds sample_idx = T_k, the 1-based upper edge"
ATOMS_MIX = col([6, 3, 1])
IDX_MIX = pack([ix[:a] for ix, a in zip(tc.sample_idx()[:N3], (6, 3, 1))])
H0_MIX = pack([tc.host_h0(t, n_ex=a) for t, a in zip(tc.TS[:N3], (6, 3, 1))])


def _idx_with(k, j, v):
    ix = [np.array(a, dtype=np.float64) for a in tc.sample_idx()[:N3]]
    ix[k][j] = v
    return pack(ix)


# 'assemble': clips, clip_len, n_clips, mode, range, p
CLIPS = [_rs.randn(30) * 3000, _rs.randn(40) * 3000, _rs.randn(50) * 3000, _rs.randn(60) * 3000]
PASM = dict(fs=1000.0, train_seq_len_max=6000.0, train_file_len_max=1500.0)
RANGE = np.array([[1, 1, 3, 1], [30, 40, 40, 60]], dtype=np.float64)
ASM = ("assemble", pack(CLIPS), col([30, 40, 50, 60]), col([2, 1, 1]), col([0, 2, 1]), RANGE, PASM)

# 'train_signals': handle, sample_idx, n_atoms, H0, p, melmat, DC_bin, settings
TSIG = ("train_signals", H, IDX, float(tc.R), None, PT, MEL, 1.0, None)

VALID = {"solve": SOLVE, "dnmf": DNMF, "dnmf_audio": AUDIO, "train": TRAIN, "assemble": ASM}
VALID_MORE = [("solve-ranks", SOLVE_MIX), ("solve-settings", swap(swap(SOLVE, 5, P64), 6, ST)),
              ("solve-fp64", swap(SOLVE, 5, P64)), ("dnmf-fp64", swap(DNMF, 7, dict(PD, snmf_precision="fp64"))),
              ("dnmf-single", swap(DNMF, 7, dict(PD, snmf_single=1.0))),
              ("dnmf_audio-mel-device-draw", swap(AUDIO_MEL, 6, None)), ("dnmf_audio-settings", swap(swap(AUDIO, 7, dict(PA, snmf_precision="fp64")), 9, ST)),
              ("train-exemplar", swap(swap(TRAIN, 5, None), 6, dict(PT, train_Exemplar=1))),
              ("train-dd-device-draw", swap(swap(TRAIN, 5, None), 6, dict(PT, domain_DD=1, alpha_eta=0.4))),
              ("train-ranks", swap(swap(swap(swap(TRAIN, 3, IDX_MIX), 4, ATOMS_MIX), 5, H0_MIX), 6, dict(PT, snmf_precision="fp64"))),
              ("train-settings", swap(swap(TRAIN, 6, dict(PT, snmf_precision="fp64")), 9, ST)),
              ("assemble-no-range", swap(swap(ASM, 4, col([0, 0, 1])), 5, None))]


def _common(name, valid, packed_at, struct_at, double_at, nlhs_max):
    """The refusals every command has: argument and output counts, a wrong class for every argument, every packed argument one
    element short and one long."""
    out = [(f"{name}-nrhs-short", "snmf:usage", 1, valid[:-1]), (f"{name}-nrhs-long", "snmf:usage", 1, valid + (1.0,)),
           (f"{name}-nlhs", "snmf:nargout", nlhs_max + 1, valid)]
    for i in struct_at:
        out.append((f"{name}-arg{i}-not-struct", "snmf:type", 1, swap(valid, i, 1.0)))
    for i in double_at:
        out.append((f"{name}-arg{i}-single", "snmf:type", 1, swap(valid, i, f32(valid[i] if valid[i] is not None else 1.0))))
    for i in packed_at:
        out.append((f"{name}-arg{i}-short", "snmf:dim", 1, swap(valid, i, short(valid[i]))))
        out.append((f"{name}-arg{i}-long", "snmf:dim", 1, swap(valid, i, long(valid[i]))))
    return out


# (case, expected id, nlhs, args): every path that is decided before the device
CASES = [
    ("usage-no-command", "snmf:usage", 1, ()),
    ("usage-command-not-char", "snmf:usage", 1, (1.0,)),
    ("usage-unknown", "snmf:usage", 1, ("mdi", V, T)),
    ("usage-command-too-long", "snmf:usage", 1, ("signals_destroy_all_of_them", H)),
]
# ---- solve
CASES += _common("solve", SOLVE, packed_at=(1, 3, 4), struct_at=(5,), double_at=(1, 2, 3, 4, 6), nlhs_max=5)
CASES += _common("solve-ranks", SOLVE_MIX, packed_at=(3, 4), struct_at=(), double_at=(), nlhs_max=5)[3:]
CASES += [
    ("solve-T-logical", "snmf:type", 1, swap(SOLVE, 2, np.array([[True], [True], [True]]))),
    ("solve-V-transposed", "snmf:dim", 1, swap(SOLVE, 1, np.asfortranarray(V.T))),
    ("solve-T-matrix", "snmf:dim", 1, swap(SOLVE, 2, np.ones((2, 2)))),
    ("solve-T-fraction", "snmf:dim", 1, swap(SOLVE, 2, col([3, 4.5, 5.5]))),
    ("solve-T-negative", "snmf:dim", 1, swap(SOLVE, 2, col([3, -4, 14]))),
    ("solve-T-zero", "snmf:dim", 1, swap(SOLVE, 2, col([3, 0, 10]))),
    ("solve-T-nan", "snmf:dim", 1, swap(SOLVE, 2, col([3, np.nan, 6]))),
    ("solve-T-beyond-int32", "snmf:dim", 1, swap(SOLVE, 2, col([3, 2.0 ** 31, 6]))),
    ("solve-empty-batch", "snmf:dim", 1, ("solve", None, None, None, None, P, None)),
    ("solve-r-length", "snmf:dim", 1, swap(SOLVE_MIX, 5, dict(PMIX, r=col(RS[:2])))),
    ("solve-r-zero", "snmf:dim", 1, swap(SOLVE, 5, dict(P, r=0.0))),
    ("solve-r-fraction", "snmf:dim", 1, swap(SOLVE, 5, dict(P, r=2.5))),
    ("solve-r-single", "snmf:type", 1, swap(SOLVE, 5, dict(P, r=f32(2)))),
    ("solve-r-missing", "snmf:field", 1, swap(SOLVE, 5, without(P, "r"))),
    ("solve-cost_check-missing", "snmf:field", 1, swap(SOLVE, 5, without(P, "cost_check"))),
    ("solve-max_iter-fraction", "snmf:field", 1, swap(SOLVE, 5, dict(P, max_iter=2.5))),
    ("solve-cf-not-char", "snmf:type", 1, swap(SOLVE, 5, dict(P, cf=1.0))),
    ("solve-precision", "snmf:precision", 1, swap(SOLVE, 5, dict(P, snmf_precision="fp16"))),
    ("solve-precision-not-char", "snmf:precision", 1, swap(SOLVE, 5, dict(P, snmf_precision=64.0))),
    ("solve-settings-3-columns", "snmf:dim", 1, swap(swap(SOLVE, 5, P64), 6, ST[:, :3])),
    ("solve-settings-transposed", "snmf:dim", 1, swap(swap(SOLVE, 5, P64), 6, np.asfortranarray(ST.T))),
    ("solve-settings-2-rows", "snmf:dim", 1, swap(swap(SOLVE, 5, P64), 6, ST[:2])),
    ("solve-settings-max_iter-fraction", "snmf:dim", 1, swap(swap(SOLVE, 5, P64), 6, ST + np.array([0, 0, 0, .5]))),
    ("solve-ranks-fp32", "snmf:unsupported", 1, swap(SOLVE_MIX, 5, without(PMIX, "snmf_precision"))),
    ("solve-settings-fp32", "snmf:unsupported", 1, swap(SOLVE, 6, ST)),
    ("solve-ranks-partial-mask", "snmf:unsupported", 1, swap(SOLVE_MIX, 5, dict(PMIX, w_update_ind=np.array([1.0, 0.0, 1.0])))),
    ("solve-ranks-vector-sparsity", "snmf:unsupported", 1, swap(SOLVE_MIX, 5, dict(PMIX, sparsity=np.ones(3)))),
    ("solve-mask-length", "snmf:dim", 1, swap(SOLVE, 5, dict(P, h_update_ind=np.ones(3)))),
    ("solve-mask-single", "snmf:type", 1, swap(SOLVE, 5, dict(P, h_update_ind=f32(np.ones(2))))),
    ("solve-sparsity-length", "snmf:dim", 1, swap(SOLVE, 5, dict(P, sparsity=np.ones(3)))),
    ("solve-sparsity-matrix", "snmf:dim", 1, swap(SOLVE, 5, dict(P, sparsity=np.ones((2, 13))))),
]
# ---- dnmf
CASES += _common("dnmf", DNMF, packed_at=(1, 2, 3, 5, 6), struct_at=(7,), double_at=(1, 2, 3, 4, 5, 6, 8), nlhs_max=3)
CASES += [
    ("dnmf-X-rows", "snmf:dim", 1, swap(DNMF, 2, DNMF[2][:-1])),
    ("dnmf-T-does-not-sum", "snmf:dim", 1, swap(DNMF, 4, col([1, 31, 33]))),
    ("dnmf-T-zero", "snmf:dim", 1, swap(DNMF, 4, col([0, 32, 32]))),
    ("dnmf-T-fraction", "snmf:dim", 1, swap(DNMF, 4, col([1.5, 30.5, 32]))),
    ("dnmf-H0-required", "snmf:dim", 1, swap(DNMF, 6, None)),
    ("dnmf-R_x-length", "snmf:dim", 1, swap(DNMF, 7, dict(PDMIX, R_x=col([5, 2])))),
    ("dnmf-R_d-zero", "snmf:dim", 1, swap(DNMF, 7, dict(PD, R_d=0.0))),
    ("dnmf-R_x-missing", "snmf:field", 1, swap(DNMF, 7, without(PD, "R_x"))),
    ("dnmf-cost_check-missing", "snmf:field", 1, swap(DNMF, 7, without(PD, "cost_check"))),
    ("dnmf-vector-sparsity", "snmf:dim", 1, swap(DNMF, 7, dict(PD, sparsity=np.ones(12)))),
    ("dnmf-precision", "snmf:precision", 1, swap(DNMF, 7, dict(PD, snmf_precision="double"))),
    ("dnmf-ranks-fp32", "snmf:unsupported", 1, swap(swap(swap(DNMF, 5, first(DNMF[5], 33 * (12 + 3 + 7))), 6, first(DNMF[6], 12 * 1 + 3 * 31 + 7 * 32)),
                                                    7, without(PDMIX, "snmf_precision"))),
    ("dnmf-settings-fp32", "snmf:unsupported", 1, swap(DNMF, 8, ST)),
    ("dnmf-single-fp64", "snmf:unsupported", 1, swap(DNMF, 7, dict(PD, snmf_precision="fp64", snmf_single=1.0))),
    ("dnmf-settings-5-columns", "snmf:dim", 1, swap(DNMF, 8, np.ones((3, 5)))),
    ("dnmf-settings-4-rows", "snmf:dim", 1, swap(DNMF, 8, np.ones((4, 4)))),
]
# ---- dnmf_audio
CASES += _common("dnmf_audio", AUDIO, packed_at=(1, 3, 5, 6), struct_at=(7,), double_at=(1, 2, 3, 4, 5, 6, 8, 9), nlhs_max=3)
CASES += _common("dnmf_audio-mel", AUDIO_MEL, packed_at=(5,), struct_at=(), double_at=(8,), nlhs_max=3)[3:]
CASES += [
    ("dnmf_audio-n_d-length", "snmf:dim", 1, swap(AUDIO, 4, col([AUDIO[4][0, 0] + AUDIO[4][1, 0], AUDIO[4][2, 0]]))),
    ("dnmf_audio-n_x-zero", "snmf:dim", 1, swap(AUDIO, 2, col([0, AUDIO[2][0, 0] + AUDIO[2][1, 0], AUDIO[2][2, 0]]))),
    ("dnmf_audio-n_x-fraction", "snmf:dim", 1, swap(AUDIO, 2, AUDIO[2] + np.array([[.5], [-.5], [0]]))),
    ("dnmf_audio-n_x-negative", "snmf:dim", 1, swap(AUDIO, 2, AUDIO[2] + np.array([[AUDIO[2][1, 0] + 1], [-AUDIO[2][1, 0] - 1], [0]]))),
    ("dnmf_audio-no-frame", "snmf:dim", 1, swap(AUDIO, 2, AUDIO[2] + np.array([[AUDIO[2][1, 0] - 10], [10 - AUDIO[2][1, 0]], [0]]))),
    ("dnmf_audio-melmat-transposed", "snmf:dim", 1, swap(AUDIO_MEL, 8, np.asfortranarray(MEL.T))),
    ("dnmf_audio-mel-basis-has-dft-rows", "snmf:dim", 1, swap(AUDIO, 8, MEL)),
    ("dnmf_audio-window-length", "snmf:field", 1, swap(AUDIO, 7, dict(PA, win_STFT=PA["win_STFT"][:-1]))),
    ("dnmf_audio-fftlength-missing", "snmf:field", 1, swap(AUDIO, 7, without(PA, "fftlength"))),
    ("dnmf_audio-DCbin-missing", "snmf:field", 1, swap(AUDIO, 7, without(PA, "DCbin"))),
    ("dnmf_audio-device-draw-without-seed", "snmf:field", 1, swap(swap(AUDIO, 6, None), 7, dict(PA, random_seed=0))),
    ("dnmf_audio-precision", "snmf:precision", 1, swap(AUDIO, 7, dict(PA, snmf_precision="FP64"))),
    ("dnmf_audio-ranks-fp32", "snmf:unsupported", 1, swap(swap(swap(AUDIO, 5, first(AUDIO[5], 33 * (12 + 11 + 6))), 6, first(AUDIO[6], 12 * 1 + 11 * 2 + 6 * 31)),
                                                          7, dict(PA, R_x=col([5, 4, 5]), R_d=col([7, 7, 1])))),
    ("dnmf_audio-settings-fp32", "snmf:unsupported", 1, swap(AUDIO, 9, ST)),
    ("dnmf_audio-settings-3-columns", "snmf:dim", 1, swap(AUDIO, 9, ST[:, 1:])),
]
# ---- train
CASES += _common("train", TRAIN, packed_at=(1, 3, 5), struct_at=(6,), double_at=(1, 2, 3, 4, 5, 7, 8, 9), nlhs_max=5)
CASES += [
    ("train-sample_idx-zero", "snmf:dim", 1, swap(TRAIN, 3, _idx_with(1, 2, 0.0))),
    ("train-sample_idx-T-plus-1", "snmf:dim", 1, swap(TRAIN, 3, _idx_with(1, 2, tc.TS[1] + 1.0))),
    ("train-sample_idx-T-plus-1-last-problem", "snmf:dim", 1, swap(TRAIN, 3, _idx_with(2, 5, tc.TS[2] + 1.0))),
    ("train-sample_idx-fraction", "snmf:dim", 1, swap(TRAIN, 3, _idx_with(0, 0, 1.5))),
    ("train-n_samples-length", "snmf:dim", 1, swap(TRAIN, 2, col([TRAIN[2][0, 0] + TRAIN[2][1, 0], TRAIN[2][2, 0]]))),
    ("train-n_samples-zero", "snmf:dim", 1, swap(TRAIN, 2, col([0, TRAIN[2][0, 0] + TRAIN[2][1, 0], TRAIN[2][2, 0]]))),
    ("train-n_samples-fraction", "snmf:dim", 1, swap(TRAIN, 2, TRAIN[2] + np.array([[.25], [-.25], [0]]))),
    ("train-no-frame", "snmf:dim", 1, swap(TRAIN, 2, TRAIN[2] + np.array([[TRAIN[2][1, 0] - 10], [10 - TRAIN[2][1, 0]], [0]]))),
    ("train-empty-batch", "snmf:dim", 1, swap(swap(TRAIN, 1, None), 2, None)),
    ("train-n_atoms-length", "snmf:dim", 1, swap(TRAIN, 4, col([6, 6]))),
    ("train-n_atoms-zero", "snmf:dim", 1, swap(TRAIN, 4, 0.0)),
    ("train-n_atoms-fraction", "snmf:dim", 1, swap(TRAIN, 4, 5.5)),
    ("train-melmat-missing", "snmf:dim", 1, swap(TRAIN, 7, None)),
    ("train-melmat-transposed", "snmf:dim", 1, swap(TRAIN, 7, np.asfortranarray(MEL.T))),
    ("train-DC_bin-vector", "snmf:dim", 1, swap(TRAIN, 8, np.ones(2))),
    ("train-precision", "snmf:precision", 1, swap(TRAIN, 6, dict(PT, snmf_precision="fp8"))),
    ("train-ranks-fp32", "snmf:unsupported", 1, swap(swap(swap(TRAIN, 3, IDX_MIX), 4, ATOMS_MIX), 5, H0_MIX)),
    ("train-settings-fp32", "snmf:unsupported", 1, swap(TRAIN, 9, ST)),
    ("train-settings-2-rows", "snmf:dim", 1, swap(swap(TRAIN, 6, dict(PT, snmf_precision="fp64")), 9, ST[:2])),
    ("train-settings-not-4-columns", "snmf:dim", 1, swap(swap(TRAIN, 6, dict(PT, snmf_precision="fp64")), 9, np.ones((3, 2)))),
    ("train-dd-without-alpha_eta", "snmf:field", 1, swap(TRAIN, 6, dict(PT, domain_DD=1))),
    ("train-pow-missing", "snmf:field", 1, swap(TRAIN, 6, without(PT, "pow"))),
    ("train-cost_check-missing", "snmf:field", 1, swap(TRAIN, 6, without(PT, "cost_check"))),
    ("train-device-draw-without-seed", "snmf:field", 1, swap(swap(TRAIN, 5, None), 6, dict(PT, random_seed=-1))),
]
# ---- assemble
CASES += _common("assemble", ASM, packed_at=(1, 5), struct_at=(6,), double_at=(1, 2, 3, 4, 5), nlhs_max=1)
CASES += [
    ("assemble-clip_len-count", "snmf:dim", 1, swap(ASM, 3, col([2, 1, 2]))),
    ("assemble-mode-length", "snmf:dim", 1, swap(ASM, 4, col([0, 2]))),
    ("assemble-mode-3", "snmf:dim", 1, swap(ASM, 4, col([0, 3, 1]))),
    ("assemble-mode-fraction", "snmf:dim", 1, swap(ASM, 4, col([0, 1.5, 1]))),
    ("assemble-n_clips-zero", "snmf:dim", 1, swap(ASM, 3, col([3, 0, 1]))),
    ("assemble-clip_len-zero", "snmf:dim", 1, swap(ASM, 2, col([30, 0, 90, 60]))),
    ("assemble-clip_len-negative", "snmf:dim", 1, swap(ASM, 2, col([30, -10, 100, 60]))),
    ("assemble-empty", "snmf:dim", 1, ("assemble", None, None, None, None, None, PASM)),
    ("assemble-mode-2-without-range", "snmf:dim", 1, swap(ASM, 5, None)),
    ("assemble-range-start-zero", "snmf:dim", 1, swap(ASM, 5, RANGE - np.array([[0, 0, 3, 0], [0, 0, 0, 0]]))),
    ("assemble-range-end-beyond", "snmf:dim", 1, swap(ASM, 5, RANGE + np.array([[0, 0, 0, 0], [0, 0, 11, 0]]))),
    ("assemble-range-reversed", "snmf:dim", 1, swap(ASM, 5, RANGE + np.array([[0, 0, 40, 0], [0, 0, 0, 0]]))),
    ("assemble-range-fraction", "snmf:dim", 1, swap(ASM, 5, RANGE + np.array([[0, 0, .5, 0], [0, 0, 0, 0]]))),
    ("assemble-vad-clip-shorter-than-bg_len", "snmf:dim", 1, swap(ASM, 4, col([1, 2, 1]))),
    ("assemble-fs-missing", "snmf:field", 1, swap(ASM, 6, without(PASM, "fs"))),
    ("assemble-odd-frame_len", "snmf:field", 1, swap(ASM, 6, dict(PASM, fs=1050.0))),
    ("assemble-fractional-frame_len", "snmf:field", 1, swap(ASM, 6, dict(PASM, fs=1010.0))),
    ("assemble-seq_len-negative", "snmf:field", 1, swap(ASM, 6, dict(PASM, train_seq_len_max=-1.0))),
    ("assemble-seq_len-missing", "snmf:field", 1, swap(ASM, 6, without(PASM, "train_seq_len_max"))),
]
# ---- the commands on a handle
for _h, _what in ((H, "never-made"), (0.0, "zero"), (-1.0, "negative"), (1.5, "fraction"), (np.ones(2), "vector"), ({"h": 1.0}, "struct"),
                  (f32(1), "single"), (None, "empty")):
    CASES += [(f"signals_info-handle-{_what}", "snmf:handle", 1, ("signals_info", _h)),
              (f"signals_get-handle-{_what}", "snmf:handle", 1, ("signals_get", _h, 1.0)),
              (f"signals_destroy-handle-{_what}", "snmf:handle", 0, ("signals_destroy", _h)),
              (f"train_signals-handle-{_what}", "snmf:handle", 1, swap(TSIG, 1, _h))]
CASES += [
    ("signals_info-nrhs", "snmf:usage", 1, ("signals_info",)),
    ("signals_info-nrhs-long", "snmf:usage", 1, ("signals_info", H, 1.0)),
    ("signals_info-nlhs", "snmf:nargout", 3, ("signals_info", H)),
    ("signals_get-nrhs", "snmf:usage", 1, ("signals_get", H)),
    ("signals_get-nlhs", "snmf:nargout", 2, ("signals_get", H, 1.0)),
    ("signals_get-k-vector", "snmf:dim", 1, ("signals_get", H, np.ones(2))),
    ("signals_get-k-single", "snmf:type", 1, ("signals_get", H, f32(1))),
    ("signals_destroy-nrhs", "snmf:usage", 0, ("signals_destroy",)),
    ("signals_destroy-nlhs", "snmf:nargout", 1, ("signals_destroy", H)),
]
CASES += _common("train_signals", TSIG, packed_at=(), struct_at=(5,), double_at=(2, 3, 4, 6, 7, 8), nlhs_max=5)
CASES += [
    ("train_signals-sample_idx-short-of-n_atoms", "snmf:dim", 1, swap(swap(TSIG, 2, short(IDX_MIX)), 3, ATOMS_MIX)),
    ("train_signals-sample_idx-long-of-n_atoms", "snmf:dim", 1, swap(swap(TSIG, 2, long(IDX_MIX)), 3, ATOMS_MIX)),
    ("train_signals-n_atoms-zero", "snmf:dim", 1, swap(TSIG, 3, 0.0)),
    ("train_signals-n_atoms-fraction", "snmf:dim", 1, swap(TSIG, 3, col([6, 2.5, 1]))),
    ("train_signals-n_atoms-empty", "snmf:dim", 1, swap(TSIG, 3, None)),
    ("train_signals-melmat-transposed", "snmf:dim", 1, swap(TSIG, 6, np.asfortranarray(MEL.T))),
    ("train_signals-melmat-missing", "snmf:dim", 1, swap(TSIG, 6, None)),
    ("train_signals-DC_bin-vector", "snmf:dim", 1, swap(TSIG, 7, np.ones(3))),
    ("train_signals-settings-3-columns", "snmf:dim", 1, swap(TSIG, 8, ST[:, :3])),
    ("train_signals-precision", "snmf:precision", 1, swap(TSIG, 5, dict(PT, snmf_precision="half"))),
    ("train_signals-window-missing", "snmf:field", 1, swap(TSIG, 5, without(PT, "win_STFT"))),
]
assert len({c[0] for c in CASES}) == len(CASES), "case names are ids"


def test_shim_compiles_and_links(shim):
    """g++ -std=c++17 -Wall -Werror of the shim + host against libsnmf_hip.so (one library in the process: mexhost.Mex); loading
    it makes no context, and it is none of the five shims of the session fixture."""
    assert shim.live_arrays() == 0 and not shim.has_exit_fcn() and shim.lock_count() == 0
    assert len(mexhost.SHIMS) == 5 and NAME not in mexhost.SHIMS


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refused_before_the_device(shim, case):
    _, want, nlhs, args = case
    with pytest.raises(MexError) as e:
        shim(nlhs, *args)
    assert e.value.id == want, (e.value.id, e.value.msg)
    assert not shim.has_exit_fcn() and shim.lock_count() == 0, "a context was made: the check came after the device"
    assert shim.live_arrays() == 0


def test_every_command_and_every_kind_of_refusal_is_covered():
    by_cmd = {}
    for _, want, _, args in CASES:
        if args and isinstance(args[0], str):
            by_cmd.setdefault(args[0], set()).add(want)
    assert set(COMMANDS) <= set(by_cmd)
    for cmd in ("solve", "dnmf", "dnmf_audio", "train"):
        assert {"snmf:usage", "snmf:nargout", "snmf:type", "snmf:dim", "snmf:field", "snmf:precision", "snmf:unsupported"} <= by_cmd[cmd], cmd
    assert {"snmf:usage", "snmf:nargout", "snmf:type", "snmf:dim", "snmf:field"} <= by_cmd["assemble"]
    assert {"snmf:usage", "snmf:nargout", "snmf:type", "snmf:dim", "snmf:field", "snmf:precision", "snmf:handle"} <= by_cmd["train_signals"]
    for cmd in ("signals_info", "signals_get", "signals_destroy"):
        assert {"snmf:usage", "snmf:nargout", "snmf:handle"} <= by_cmd[cmd], cmd


@pytest.mark.parametrize("name,args", list(VALID.items()) + VALID_MORE, ids=list(VALID) + [n for n, _ in VALID_MORE])
def test_a_valid_call_stops_only_at_the_device(shim_dev, lib, name, args):
    """Every check passes: without a device the call ends in snmf:device, made no context and left no array; with one it returns."""
    nlhs = {"solve": 5, "dnmf": 3, "dnmf_audio": 3, "train": 5, "assemble": 1}[args[0]]
    if lib.snmf_device_count() > 0:
        assert len(shim_dev(nlhs, *args)) == nlhs
    else:
        with pytest.raises(MexError) as e:
            shim_dev(nlhs, *args)
        assert e.value.id == "snmf:device", (e.value.id, e.value.msg)
        assert shim_dev.lock_count() == 0 and not shim_dev.has_exit_fcn()
    assert shim_dev.live_arrays() == 0


def test_sample_idx_upper_edge_passes(shim_dev, lib):
    """sample_idx = T_k in every problem is the last valid column: only T_k + 1 is refused (CASES)."""
    idx = pack([np.full(tc.R, t, dtype=np.float64) for t in tc.TS[:N3]])
    try:
        shim_dev(5, *swap(TRAIN, 3, idx))
        assert lib.snmf_device_count() > 0
    except MexError as e:
        assert e.id == "snmf:device" and lib.snmf_device_count() == 0, (e.id, e.msg)
    assert shim_dev.live_arrays() == 0


# ---- the wrappers under integration/batch/: call arity ---------------------------------------------------------------------
def _batch_call_sites():
    """(file, line, shim, command, number of arguments) of every snmf_batch_mex( / snmf_dnmf_mex( call in integration/batch/*.m."""
    sites = []
    for path in sorted(glob.glob(os.path.join(mexhost.ROOT, "integration", "batch", "*.m"))):
        src = open(path).read()
        code = "\n".join(line if line.lstrip()[:1] != "%" else "" for line in src.split("\n"))
        for mt in re.finditer(r"\b(snmf_batch_mex|snmf_dnmf_mex)\(", code):
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
            sites.append((os.path.basename(path), code[:mt.start()].count("\n") + 1, mt.group(1), cmd.group(1) if cmd else None, top_level_args(text)))
    return sites


BATCH_SITES = _batch_call_sites()


def test_the_wrappers_use_every_command():
    files = {f for f, *_ in BATCH_SITES}
    assert {"sparse_nmf_batch.m", "run_basis_train_batch.m", "run_basis_DNMF_batch.m"} <= files
    used = {c for _, _, s, c, _ in BATCH_SITES if s == NAME}
    assert {"solve", "dnmf_audio", "assemble", "signals_info", "signals_get", "train_signals", "signals_destroy"} <= used, used
    assert ("snmf_dnmf_mex", "nframes") in {(s, c) for _, _, s, c, _ in BATCH_SITES}


@pytest.mark.parametrize("site", BATCH_SITES, ids=[f"{f}:{ln}" for f, ln, *_ in BATCH_SITES])
def test_wrapper_call_arity(site):
    """The number of arguments at the call site is one the shim's own nrhs test accepts for that command."""
    fname, line, shim_name, cmd, nargs = site
    assert cmd is not None, f"{fname}:{line}: the command must be a literal"
    assert nargs in shim_arity(shim_name, cmd), f"{fname}:{line}: {shim_name}('{cmd}', ...) is called with {nargs} arguments"


def test_shim_arity_reads_every_command():
    want = {"solve": 7, "dnmf": 9, "dnmf_audio": 10, "train": 10, "assemble": 7, "signals_info": 2, "signals_get": 3, "train_signals": 9,
            "signals_destroy": 2}
    assert {c: shim_arity(NAME, c) for c in COMMANDS} == {c: {n} for c, n in want.items()}


# ---- the same table under the sanitizers, as a program of its own -----------------------------------------------------------
def test_refusals_under_sanitizers(tmp_path, lib):
    """tests/mexhost/replay_main.cpp + the shim + the host as ONE stand-alone program built with the address and
    undefined-behaviour sanitizers (the recipe of that file's header), fed the table above as mexhost.dump_cases writes it.  Exit
    status 0: every case ended in its recorded identifier, without a host error, a sanitizer report or a live array.  Nothing
    sanitized is loaded into this interpreter."""
    cases = str(tmp_path / "cases.txt")
    mexhost.dump_cases(cases, [(NAME, name, want, nlhs, args) for name, want, nlhs, args in CASES])
    exe = str(tmp_path / "replay_batch")
    lp = mexhost.lib_path()
    cmd = ["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",  # (-Wall -Werror: mexhost.build_shim)
           "-I" + os.path.join(mexhost.ROOT, "integration", "mex_stub"), "-I" + os.path.join(mexhost.ROOT, "include"),
           os.path.join(mexhost.HOST_DIR, "replay_main.cpp"), os.path.join(mexhost.ROOT, "integration", NAME + ".cpp"),
           os.path.join(mexhost.HOST_DIR, "mexhost.cpp"), "-L" + os.path.dirname(lp), "-l:" + os.path.basename(lp),
           "-Wl,-rpath," + os.path.dirname(lp), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, NAME, cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{NAME}: {len(CASES)} cases replayed, 0 wrong" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
