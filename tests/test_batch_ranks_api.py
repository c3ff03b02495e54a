"""CPU tests of the mixed-rank fp64 batch (snmf_batch_create_ranks_fp64, snmf_run_basis_train_*_batch_ranks_fp64; BatchPlan64,
sparse_nmf_batch_fp64 and the three batched basis-training calls with a rank per problem): every argument error fires before the
library is loaded, with its status; the fp32 error for differing ranks is unchanged; the three C names stand in the header and in
the binding; the C entries refuse NULL arguments without a device; and the signals of the GPU training test stop where that test
needs them to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_ranks_cases as rc
import train_batch_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ["snmf_batch_create_ranks_fp64", "snmf_run_basis_train_audio_batch_ranks_fp64", "snmf_run_basis_train_signals_batch_ranks_fp64"]


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


def test_plan_refusals_come_before_the_library(no_device):
    from se_snmf_nat_amd import BatchPlan, BatchPlan64, BatchPlanMdi64
    Ts = (5, 3, 8)
    assert _status(lambda: BatchPlan64(None, 6, [2, 3], Ts)) == 3                       # a list that is not one per problem
    assert _status(lambda: BatchPlan64(None, 6, [2, 3, 4, 5], Ts)) == 3
    assert _status(lambda: BatchPlan64(None, 6, [2, 0, 4], Ts)) == 1                    # an entry below 1
    assert _status(lambda: BatchPlan64(None, 6, [2, 3, 4], Ts, sparsity=np.ones(4))) == 8   # an r-vector across ranks
    assert _status(lambda: BatchPlan64(None, 6, [2, 3, 4], Ts, w_update_ind=np.array([1, 0, 1, 1]))) == 8
    assert _status(lambda: BatchPlan64(None, 6, [2, 3, 4], Ts, h_update_ind=np.array([0, 0, 1, 0]))) == 8
    # the fp32 engine shares the rank: status 3, as for init_w arrays of different widths; so does a missing-data batch (8)
    assert _status(lambda: BatchPlan(None, 6, [2, 3, 4], Ts)) == 3
    assert _status(lambda: BatchPlanMdi64(None, 6, [2, 3, 4], Ts)) == 8
    _reaches(lambda: BatchPlanMdi64(None, 6, [3, 3, 3], Ts))
    # valid forms pass every check and only then reach the library
    for kw in (dict(), dict(w_update_ind=np.zeros(4)), dict(h_update_ind=False), dict(sparsity=0.5), dict(sparsity=np.array([0.5]))):
        _reaches(lambda: BatchPlan64(None, 6, [2, 3, 4], Ts, **kw))
    _reaches(lambda: BatchPlan64(None, 6, (3, 3, 3), Ts))
    _reaches(lambda: BatchPlan64(None, 6, np.array([3, 3, 3]), Ts, sparsity=np.ones(3)))  # equal ranks: the int form takes the vector
    _reaches(lambda: BatchPlan(None, 6, [3, 3, 3], Ts))
    _reaches(lambda: BatchPlan64(None, 6, 3, Ts))


def test_solve_refusals_come_before_the_library(no_device):
    from se_snmf_nat_amd import sparse_nmf_batch, sparse_nmf_batch_fp64
    vs = _vs()
    ws = [np.ones((6, r)) for r in (2, 3, 4)]
    base = dict(cf="kl", cost_check=1, max_iter=3)
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, r=[2, 3]))) == 3
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, r=[2, 3, 0]))) == 1
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, r=[2, 3, 4], sparsity=np.ones(4)))) == 8
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws, sparsity=np.ones((4, 1))))) == 8
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws, w_update_ind=np.array([1, 1, 0, 0])))) == 8
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws, h_update_ind=np.array([1, 1, 0, 0])))) == 8
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws, init_h=[np.ones((2, 5)), np.ones((2, 3)), np.ones((4, 8))]))) == 3
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(cf="kl", init_w=ws))) == 4           # src/sparse_nmf.m:260
    assert _status(lambda: sparse_nmf_batch_fp64(vs, dict(base))) == 2                          # neither r nor init_w
    # the fp32 error for differing ranks is unchanged
    assert _status(lambda: sparse_nmf_batch(vs, dict(base, init_w=ws))) == 3
    assert _status(lambda: sparse_nmf_batch(vs, dict(base, r=[2, 3, 4]))) == 3
    # valid calls reach the library: a list for r, init_w of different widths, init_w narrower than r[k] (the rest is drawn)
    _reaches(lambda: sparse_nmf_batch_fp64(vs, dict(base, r=[2, 3, 4])))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws)))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws, r=[2, 5, 1], init_h=[np.ones((2, 5)), np.ones((5, 3)), np.ones((4, 8))])))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, dict(base, init_w=ws, w_update_ind=np.zeros(4), h_update_ind=np.ones(2))))
    _reaches(lambda: sparse_nmf_batch_fp64(vs, dict(base, r=[3, 3, 3], sparsity=np.ones(3))))
    _reaches(lambda: sparse_nmf_batch(vs, dict(base, r=[3, 3, 3])))


def test_the_draws_stay_in_list_order_each_of_its_own_shape():
    """w then h per problem from one generator: what a loop of single solves sharing that generator would draw."""
    from se_snmf_nat_amd.batch import _batch_draws, _batch_inits
    vs = _vs()
    w1 = np.ones((6, 1))
    rs, iws, ihs = _batch_inits(dict(r=[2, 3, 4], init_w=[w1, np.ones((6, 3)), w1]), vs, 6, per_problem=True)
    assert rs == [2, 3, 4] and ihs is None
    w0s, h0s = _batch_draws(vs, 6, rs, iws, ihs, np.random.RandomState(7), np.dtype(np.float64))
    g = np.random.RandomState(7)
    for k, (v, r) in enumerate(zip(vs, rs)):
        ri = iws[k].shape[1]
        assert w0s[k].shape == (6, r) and h0s[k].shape == (r, v.shape[1])
        assert np.array_equal(w0s[k][:, :ri], iws[k])
        if ri < r:
            assert np.array_equal(w0s[k][:, ri:], g.random_sample((6, r - ri)))
        assert np.array_equal(h0s[k], g.random_sample((r, v.shape[1])))
    rs, _, _ = _batch_inits(dict(init_w=[w1, np.ones((6, 3)), w1], r=2), vs, 6, per_problem=True)  # :125: r only where it is larger
    assert rs == [2, 3, 2]


def test_training_refusals_come_before_the_library(no_device):
    from se_snmf_nat_amd import run_basis_train_assembled_batch, run_basis_train_clips_batch, run_basis_train_signal_batch
    p = tc.P_STOP
    sigs = tc.signals()
    two = [sigs[3], sigs[0]]  # T = 32 and T = 6

    def st(sg, R, pq=p, **kw):
        return _status(lambda: run_basis_train_signal_batch(sg, R, pq, **kw))

    for prec in ("fp32", "fp64"):
        assert st(two, [3], precision=prec) == 3                 # not one entry per problem
        assert st(two, [3, 3, 3], precision=prec) == 3
        assert st(two, [3, 0], precision=prec) == 1              # an entry below 1
    assert st(two, [3, 2], precision="fp32") == 8                # differing ranks need the fp64 engine
    assert st(two, [3, 2]) == 8
    from se_snmf_nat_amd import SnmfError
    with pytest.raises(SnmfError, match="problem 1 has 6 frames") as e:   # n_ex_k > T_k, naming k
        run_basis_train_signal_batch(two, [8, 7], p, precision="fp64")
    assert e.value.status == 3
    assert st(two, [5, 4], pq=dict(p, cluster_buff=2), precision="fp64") == 3
    assert st(two, [3, 2], precision="fp64", sample_idx=[np.arange(1, 4), np.arange(1, 4)]) == 3  # sample_idx[k] holds n_ex_k indices
    _reaches(lambda: run_basis_train_signal_batch(two, [3, 2], p, precision="fp64"))
    _reaches(lambda: run_basis_train_signal_batch(two, [3, 2], p, precision="fp64", h0="device",
                                                  sample_idx=[np.arange(1, 4), np.arange(1, 3)]))
    _reaches(lambda: run_basis_train_signal_batch(two, np.array([3, 2]), dict(p, cluster_buff=2), precision="fp64"))
    for prec in ("fp32", "fp64"):  # equal entries are the scalar call
        _reaches(lambda: run_basis_train_signal_batch(two, [3, 3], p, precision=prec))
    # the clips form: what needs no assembled length is refused before the assembly
    clips = [[np.arange(400, dtype=np.float64)], [np.arange(300, dtype=np.float64)]]
    pc = dict(p, train_seq_len_max=700, train_file_len_max=300)
    assert _status(lambda: run_basis_train_clips_batch(clips, [3], pc, precision="fp64")) == 3
    assert _status(lambda: run_basis_train_clips_batch(clips, [3, 0], pc, precision="fp64")) == 1
    assert _status(lambda: run_basis_train_clips_batch(clips, [3, 2], pc)) == 8
    _reaches(lambda: run_basis_train_clips_batch(clips, [3, 2], pc, precision="fp64"))
    assert _status(lambda: run_basis_train_assembled_batch(object(), [3, 2], pc, precision="fp64")) == 1


def test_c_names_stand_in_the_header_and_in_the_binding_once():
    from se_snmf_nat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snmf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for nm in C_NAMES:
        m = re.findall(r"\b%s\s*\(([^;]*)\)\s*;" % nm, txt)
        assert len(m) == 1, nm
        assert not re.search(r"\bld[A-Za-z_]*\b", m[0]), nm   # no leading dimension in a new prototype: every matrix is tight
        assert _lib.SYMBOLS.count(nm) == 1, nm
    assert re.search(r"#define\s+SNMF_ABI_VERSION\s+5\b", hdr)


def test_c_entries_refuse_null_arguments_without_a_device(lib):
    from se_snmf_nat_amd import frontend as fe
    from se_snmf_nat_amd.api import _make_params
    sp, _win = fe._params(tc.TINY)
    q = _make_params(tc.F, 1, 6, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    T = np.array([5, 7], np.int32)
    r = np.array([6, 2], np.int32)
    h = C.c_void_p()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.snmf_batch_create_ranks_fp64(None, C.byref(q), 2, vp(T), vp(r), C.byref(h)) == 1
    assert lib.snmf_batch_create_ranks_fp64(None, None, 2, None, None, None) == 1
    fa = lib.snmf_run_basis_train_audio_batch_ranks_fp64
    assert fa(None, C.byref(q), C.byref(sp), -1.0, None, 0, 2, None, None, vp(r), None, 0, None, None, None, None, None, None, None) == 1
    assert fa(None, C.byref(q), C.byref(sp), -1.0, None, 0, 2, None, None, None, None, 0, None, None, None, None, None, None, None) == 1
    fs = lib.snmf_run_basis_train_signals_batch_ranks_fp64
    assert fs(None, C.byref(q), C.byref(sp), -1.0, None, 0, None, vp(r), None, 0, None, None, None, None, None, None, None) == 1


def test_the_signals_stop_where_the_gpu_test_needs_them_to():
    """The DFT solves of the six problems at their own ranks, on the oracle from the H0 the GPU test uses: one runs to max_iter and
    the others stop on their own at no fewer than two different iterations."""
    n = rc.oracle_stop_indices()
    print("oracle stop indices [n_dft, n_mel] per problem at ranks", rc.RANKS, ":", n)
    assert tc.stops_are_spread([a for a, _ in n], tc.P_STOP["max_iter"]), n
