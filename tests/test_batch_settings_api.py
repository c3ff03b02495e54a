"""CPU tests of the fp64 batch with settings per problem (snmf_batch_create_settings_fp64,
snmf_run_basis_train_*_batch_settings_fp64; BatchPlan64(settings=...), sparse_nmf_batch_fp64 with a list of settings dicts and the
three batched basis-training calls with settings=...): every argument error fires before the library is loaded, with its status;
valid forms reach the library; the three C names stand in the header and in the binding; the C entries refuse NULL arguments without
a device; and the sweep case of the GPU tests stops on the oracle where those tests need it to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_settings_cases as sc
import train_batch_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ["snmf_batch_create_settings_fp64", "snmf_run_basis_train_audio_batch_settings_fp64",
           "snmf_run_basis_train_signals_batch_settings_fp64"]


@pytest.fixture
def no_device(monkeypatch):
    from se_snmf_nat_amd import _lib, batch, frontend, train

    def refuse(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", refuse)
    for mod in (batch, train, frontend):
        monkeypatch.setattr(mod, "default_context", refuse)


def _vs(F=6, Ts=(5, 3, 8)):
    rs = np.random.RandomState(0)
    return [rs.rand(F, T) + 0.1 for T in Ts]


def _status(call):
    from se_snmf_nat_amd import SnmfError
    with pytest.raises(SnmfError) as e:
        call()
    return e.value.status


def _reaches(call):
    with pytest.raises(AssertionError, match="reached the device"):
        call()


S3 = [dict(cf="kl", sparsity=5), dict(cf="ed", max_iter=4), dict(beta=0.5, conv_eps=1e-3)]


def test_plan_refusals_come_before_the_library(no_device):
    from se_snmf_nat_amd import BatchPlan, BatchPlan64, BatchPlanMdi64
    Ts = (5, 3, 8)
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=S3[:2])) == 3                      # not one per problem
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=S3 + S3[:1])) == 3
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=dict(cf="kl"))) == 3               # a dict is not a list of dicts
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=[dict(cf="kl"), dict(r=3), dict()])) == 1   # an unknown key
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=[dict(), dict(cost_check=1), dict()])) == 1
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=[dict(), dict(sparsity=np.ones(3)), dict()])) == 8  # a vector sparsity
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, sparsity=np.ones(3), settings=[dict(sparsity=1), dict(), dict(sparsity=2)])) == 8
    assert _status(lambda: BatchPlan64(None, 6, 3, Ts, settings=[dict(), dict(max_iter=-1), dict()])) == 1
    # the engines without the form: status 8
    assert _status(lambda: BatchPlan(None, 6, 3, Ts, settings=S3)) == 8
    assert _status(lambda: BatchPlanMdi64(None, 6, 3, Ts, settings=S3)) == 8
    # with ranks, the rules of the ranks handle apply unchanged
    assert _status(lambda: BatchPlan64(None, 6, [2, 3, 4], Ts, settings=S3, w_update_ind=np.array([1, 0, 1, 1]))) == 8
    assert _status(lambda: BatchPlan64(None, 6, [2, 3], Ts, settings=S3)) == 3
    # valid forms pass every check and only then reach the library
    _reaches(lambda: BatchPlan64(None, 6, 3, Ts, settings=S3))
    _reaches(lambda: BatchPlan64(None, 6, 3, Ts, settings=[dict(), dict(), dict()]))
    _reaches(lambda: BatchPlan64(None, 6, [2, 3, 4], Ts, settings=S3, h_update_ind=False))
    _reaches(lambda: BatchPlan64(None, 6, 3, Ts, settings=S3, w_update_ind=np.array([1, 0, 1])))
    _reaches(lambda: BatchPlan64(None, 6, 3, Ts, sparsity=np.ones(3), settings=[dict(sparsity=k) for k in range(3)]))
    _reaches(lambda: BatchPlan64(None, 6, 3, Ts))


def test_a_missing_key_takes_the_plans_shared_value():
    from se_snmf_nat_amd.batch import _problem_settings, _settings_array
    shared = dict(beta=2.0, sparsity=0.25, max_iter=17, conv_eps=1e-4)
    got = _problem_settings([dict(), dict(cf="is"), dict(beta=1.5, max_iter=3), dict(cf="beta", beta=0.5, sparsity=[7.0], conv_eps=0)], 4, shared)
    assert got == [(2.0, 0.25, 17, 1e-4), (0.0, 0.25, 17, 1e-4), (1.5, 0.25, 3, 1e-4), (0.5, 7.0, 17, 0.0)]
    arr = _settings_array(got)
    assert [(a.beta, a.sparsity, a.max_iter, a.conv_eps, a.reserved) for a in arr] == [(b, s, m, e, 0) for b, s, m, e in got]
    assert C.sizeof(arr) == 4 * 32  # include/snmf.h: three doubles and two int32


def test_solve_refusals_come_before_the_library(no_device):
    from se_snmf_nat_amd import sparse_nmf_batch, sparse_nmf_batch_fp64
    vs = _vs()
    base = dict(cf="kl", cost_check=1, max_iter=3, r=3)
    ps = [dict(base), dict(base, cf="ed", sparsity=0.5), dict(base, cf="beta", beta=0.5, max_iter=2)]
    assert _status(lambda: sparse_nmf_batch_fp64(vs, ps[:2])) == 3                                            # not one per problem
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], dict(ps[1], sparsity=np.ones(3)), ps[2]])) == 8  # a vector sparsity
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], {k: v for k, v in ps[1].items() if k != "cost_check"}, ps[2]])) == 4
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], dict(ps[1], cost_check=0), ps[2]])) == 3         # shared, and equal
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], dict(ps[1], random_seed=2), ps[2]])) == 3
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], dict(ps[1], w_update_ind=np.array([1, 0, 1])), ps[2]])) == 3
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], dict(ps[1], r=None), ps[2]])) == 2               # neither r nor init_w
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [ps[0], dict(ps[1], init_h=np.ones((2, 3))), ps[2]])) == 3
    # differing ranks go through the ranks rules
    mixed = [dict(q, r=r) for q, r in zip(ps, (2, 3, 4))]
    assert _status(lambda: sparse_nmf_batch_fp64(vs, [dict(q, w_update_ind=np.array([1, 0])) for q in mixed])) == 8
    # the fp32 batch has one settings struct
    assert _status(lambda: sparse_nmf_batch(vs, ps)) == 8
    # valid calls reach the library
    _reaches(lambda: sparse_nmf_batch_fp64(vs, ps))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, mixed))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, [dict(q, w_update_ind=np.zeros(q["r"])) for q in mixed]))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, [dict(q, w_update_ind=np.array([1, 0, 1])) for q in ps]))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, [dict(ps[0], init_w=np.ones((6, 2))), ps[1], dict(ps[2], init_h=np.ones((3, 8)))]))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, dict(base)))  # the dict call, as before


def test_training_refusals_come_before_the_library(no_device):
    from se_snmf_nat_amd import run_basis_train_assembled_batch, run_basis_train_clips_batch, run_basis_train_signal_batch
    p = tc.P_STOP
    sigs = tc.signals()
    two = [sigs[3], sigs[0]]  # T = 32 and T = 6
    s2 = [dict(cf="ed", sparsity=0.5), dict(max_iter=7)]

    def st(sg, R, settings, pq=p, **kw):
        return _status(lambda: run_basis_train_signal_batch(sg, R, pq, settings=settings, **kw))

    assert st(two, 3, s2[:1], precision="fp64") == 3
    assert st(two, 3, s2 + s2, precision="fp64") == 3
    assert st(two, 3, [dict(), dict(R=3)], precision="fp64") == 1
    assert st(two, 3, [dict(sparsity=np.ones(3)), dict()], precision="fp64") == 8
    assert st(two, 3, s2, precision="fp32") == 8          # the fp32 engine has one settings struct
    assert st(two, 3, s2) == 8
    assert st(two, [3, 2], s2, precision="fp32") == 8
    _reaches(lambda: run_basis_train_signal_batch(two, 3, p, precision="fp64", settings=s2))
    _reaches(lambda: run_basis_train_signal_batch(two, [3, 2], p, precision="fp64", settings=s2, h0="device"))
    _reaches(lambda: run_basis_train_signal_batch(two, 3, p, precision="fp64"))
    # the clips form: refused before the assembly
    clips = [[np.arange(400, dtype=np.float64)], [np.arange(300, dtype=np.float64)]]
    pc = dict(p, train_seq_len_max=700, train_file_len_max=300)
    assert _status(lambda: run_basis_train_clips_batch(clips, 3, pc, precision="fp64", settings=s2[:1])) == 3
    assert _status(lambda: run_basis_train_clips_batch(clips, 3, pc, precision="fp64", settings=[dict(x=1), dict()])) == 1
    assert _status(lambda: run_basis_train_clips_batch(clips, 3, pc, settings=s2)) == 8
    _reaches(lambda: run_basis_train_clips_batch(clips, 3, pc, precision="fp64", settings=s2))
    assert _status(lambda: run_basis_train_assembled_batch(object(), 3, pc, precision="fp64", settings=s2)) == 1


def test_c_names_stand_in_the_header_and_in_the_binding_once():
    from se_snmf_nat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snmf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for nm in C_NAMES:
        m = re.findall(r"\b%s\s*\(([^;]*)\)\s*;" % nm, txt)
        assert len(m) == 1, nm
        assert "const snmf_problem_settings*" in m[0], nm
        assert _lib.SYMBOLS.count(nm) == 1, nm
    assert len(re.findall(r"\}\s*snmf_problem_settings\s*;", txt)) == 1
    assert re.search(r"#define\s+SNMF_ABI_VERSION\s+5\b", hdr)


def test_c_entries_refuse_null_arguments_without_a_device(lib):
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd._lib import SnmfProblemSettings
    from se_snmf_nat_amd.api import _make_params
    sp, _win = fe._params(tc.TINY)
    q = _make_params(tc.F, 1, 6, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    T = np.array([5, 7], np.int32)
    r = np.array([6, 2], np.int32)
    s = (SnmfProblemSettings * 2)()
    h = C.c_void_p()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    fc = lib.snmf_batch_create_settings_fp64
    assert fc(None, C.byref(q), 2, vp(T), vp(r), s, C.byref(h)) == 1       # no context
    assert fc(None, C.byref(q), 2, vp(T), None, None, C.byref(h)) == 1     # no settings
    assert fc(None, None, 2, None, None, None, None) == 1
    fa = lib.snmf_run_basis_train_audio_batch_settings_fp64
    assert fa(None, C.byref(q), C.byref(sp), -1.0, None, 0, 2, None, None, vp(r), None, 0, None, None, None, None, None, None, None, s) == 1
    assert fa(None, C.byref(q), C.byref(sp), -1.0, None, 0, 2, None, None, None, None, 0, None, None, None, None, None, None, None, None) == 1
    fs = lib.snmf_run_basis_train_signals_batch_settings_fp64
    assert fs(None, C.byref(q), C.byref(sp), -1.0, None, 0, None, vp(r), None, 0, None, None, None, None, None, None, None, s) == 1
    assert fs(None, C.byref(q), C.byref(sp), -1.0, None, 0, None, None, None, 0, None, None, None, None, None, None, None, None) == 1


def test_the_sweep_case_stops_where_the_gpu_tests_need_it_to():
    """On the fp64 oracle with max_iter = 40 for all: the conditions, not the numbers."""
    n = sc.oracle_stop_indices(40)
    print("oracle stop indices of the sweep case at max_iter = 40:", n, "own max_iter:", sc.MAX_ITER)
    own = [min(a, mi) for a, mi in zip(n, sc.MAX_ITER)]  # where each problem ends with its own limit
    print("n_iter with the own limits:", own)
    largest = max(sc.MAX_ITER)
    assert len(set(own)) >= 4, own
    assert sum(1 for a, mi in zip(n, sc.MAX_ITER) if mi < largest and a > mi) >= 2, (n, sc.MAX_ITER)
    assert sum(1 for a, mi in zip(n, sc.MAX_ITER) if a < mi) >= 3, (n, sc.MAX_ITER)
