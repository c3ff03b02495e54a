"""CPU tests of the DNMF batches with a rank pair and settings per problem (run_basis_dnmf_batch, run_basis_DNMF_batch,
run_basis_DNMF_Mel_batch with sequences for R_x / R_d and settings=[...]): every argument error carries its status and is raised
before the library is loaded, the fp32 engine refuses, scalar arguments still reach the uniform entry, the host H0 draw for equal
ranks is the uniform draw, the two C entries stand in the header and the binding and refuse without a device, and the problems of
the GPU tests stop on the oracle where those tests need them to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dnmf_audio_batch_cases as ac
import dnmf_batch_cases as dc
import dnmf_batch_ranks_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_NAMES = ["snmf_run_basis_dnmf_batch_ranks_fp64", "snmf_run_basis_dnmf_audio_batch_ranks_fp64"]


class Reached(Exception):
    def __init__(self, name, args):
        super().__init__(name)
        self.name, self.args_ = name, args


class FakeLib:
    """Stands in the library's place: the first entry that is called ends the call and says which one it was."""

    def __getattr__(self, name):
        def entry(*args):
            raise Reached(name, args)
        return entry


def no_device(*a, **k):
    raise AssertionError("reached the library")


def test_matrix_form_argument_errors_come_before_any_library_call(monkeypatch):
    from se_snmf_nat_amd import _lib, batch
    from se_snmf_nat_amd.batch import run_basis_dnmf_batch
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(batch, "default_context", no_device)
    F, T = 6, 5
    V, V2 = np.ones((F, T)), np.ones((F, T + 1))
    Bs = [np.ones((F, 5)), np.ones((F, 3))]
    Hs = [np.ones((5, T)), np.ones((3, T + 1))]
    p = dict(cf="kl", sparsity=0.1, max_iter=3, cost_check=1)
    good = dict(Ys=[V, V2], Bq=Bs, Rx=[2, 1], Rd=[3, 2], h0=Hs, precision="fp64")

    def call(pq=p, **kw):
        a = dict(good, **kw)
        Ys, Bq, Rx, Rd = (a.pop(k) for k in ("Ys", "Bq", "Rx", "Rd"))
        return run_basis_dnmf_batch(Ys, Ys, Ys, Bq, Rx, Rd, pq, **a)

    def status(**kw):
        with pytest.raises(_lib.SnmfError) as e:
            call(**kw)
        return e.value.status

    assert status(Rx=[2]) == 3 and status(Rd=[3, 2, 1]) == 3                 # a rank list of another length
    assert status(Rx=np.array([2, 1, 1])) == 3
    assert status(Rx=[2, 0]) == 1 and status(Rd=[-1, 2]) == 1                # a rank below 1
    assert status(Rx=0, Rd=[3, 2], Bq=[np.ones((F, 3)), np.ones((F, 2))]) == 1  # (also as the scalar beside a sequence)
    assert status(Bq=[Bs[0]]) == 3                                           # B of the wrong list length
    assert status(Bq=Bs[0]) == 3                                             # one B for pairs that differ
    assert status(Bq=[Bs[0], Bs[0]]) == 3                                    # B_k that does not fit problem k's own ranks
    assert status(Bq=[Bs[0], np.ones((F + 1, 3))]) == 3
    assert status(h0=[Hs[0]]) == 3                                           # h0 of the wrong list length
    assert status(h0=[Hs[0], np.ones((5, T + 1))]) == 3                      # H0_k that does not fit problem k's own ranks
    assert status(h0=[Hs[0], np.ones((3, T))]) == 3
    assert status(h0="device") == 3
    assert status(precision="fp32") == 8                                     # the fp32 engine: lists ...
    assert status(Rx=(2, 2), Rd=(3, 3), Bq=Bs[0], h0="host", precision="fp32") == 8  # ... also equal ones ...
    assert status(Rx=2, Rd=3, Bq=Bs[0], h0="host", precision="fp32", settings=[{}, {}]) == 8  # ... and settings
    assert status(dtype=np.float32) == 1                                     # the fp64 mode takes doubles
    assert status(pq=dict(cf="kl", sparsity=0.1)) == 4                       # no cost_check (src/sparse_nmf.m:260)
    assert status(pq=dict(p, sparsity=np.ones(5))) == 3                      # a non-scalar sparsity of p
    assert status(settings=[{}]) == 3 and status(settings={}) == 3           # the rules of _problem_settings
    assert status(settings=[{}, 1]) == 1
    assert status(settings=[{}, dict(tol=1)]) == 1
    assert status(settings=[{}, dict(max_iter=-1)]) == 1
    assert status(settings=[{}, dict(sparsity=[1.0, 2.0])]) == 8
    assert status(Ys=[V, np.ones((F + 1, T + 1))]) == 3                      # (the uniform call's own errors stay)
    assert status(Ys=[]) == 1
    with pytest.raises(ValueError):
        run_basis_dnmf_batch([V], [V], [V], Bs[:1], [2], [3], p, precision="bf16")
    # valid calls pass every check and only then reach the library
    for kw in (dict(), dict(settings=[dict(cf="ed"), dict(max_iter=2, sparsity=1.0)]), dict(h0="host"), dict(Rx=[2, 2], Rd=[3, 3], Bq=Bs[0], h0="host"),
               dict(Rx=2, Rd=[3, 1], h0="host"), dict(Rx=2, Rd=3, Bq=Bs[0], h0="host", settings=[{}, {}])):
        with pytest.raises(AssertionError, match="reached the library"):
            call(**kw)


def test_waveform_form_argument_errors_come_before_any_library_call(monkeypatch):
    from se_snmf_nat_amd import _lib, frontend, train
    from se_snmf_nat_amd.train import run_basis_DNMF_batch, run_basis_DNMF_Mel_batch
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(train, "default_context", no_device)
    monkeypatch.setattr(frontend, "default_context", no_device)
    w = ac.waves()
    xs, ds = [w[2][0], w[0][0]], [w[2][1], w[0][1]]
    Ts = [ac.TS[2], ac.TS[0]]
    Rx, Rd = [3, 1], [2, 4]
    p = dict(ac.P_STOP, R_x=Rx, R_d=Rd)

    def bases(rows):
        return [np.ones((rows, 5)), np.ones((rows, 5))]

    def status(fn=run_basis_DNMF_batch, Bq=None, pq=p, precision="fp64", **kw):
        rows = ac.F if fn is run_basis_DNMF_batch else ac.TINY["F_order"]
        with pytest.raises(_lib.SnmfError) as e:
            fn(xs, ds, bases(rows) if Bq is None else Bq, pq, precision=precision, **kw)
        return e.value.status

    for fn in (run_basis_DNMF_batch, run_basis_DNMF_Mel_batch):
        rows = ac.F if fn is run_basis_DNMF_batch else ac.TINY["F_order"]
        assert status(fn, pq=dict(p, R_x=[3])) == 3 and status(fn, pq=dict(p, R_d=[2, 4, 1])) == 3
        assert status(fn, pq=dict(p, R_x=[3, 0])) == 1
        assert status(fn, precision="fp32") == 8
        assert status(fn, pq=dict(p, R_x=3, R_d=2), precision="fp32", settings=[{}, {}]) == 8
        assert status(fn, pq=dict(p, R_d=[2, 3])) == 3                       # B_k that does not fit problem k's own ranks
        assert status(fn, Bq=np.ones((rows, 5)), pq=dict(p, R_d=[2, 3])) == 3  # one B for pairs that differ
        assert status(fn, Bq=bases(rows)[:1]) == 3
        assert status(fn, h0=[np.ones((5, Ts[0]))]) == 3
        assert status(fn, h0=[np.ones((5, Ts[0])), np.ones((4, Ts[1]))]) == 3
        assert status(fn, h0="gpu") == 3
        assert status(fn, settings=[{}]) == 3 and status(fn, settings=[{}, dict(sparsity=[1.0, 2.0])]) == 8
        assert status(fn, dtype=np.float32) == 1
        for kw in (dict(), dict(h0="device"), dict(h0=[np.ones((5, Ts[0])), np.ones((5, Ts[1]))]), dict(settings=[dict(cf="is"), dict(max_iter=1)])):
            with pytest.raises(AssertionError, match="reached the library"):
                fn(xs, ds, bases(rows), p, precision="fp64", **kw)


def test_scalars_reach_the_uniform_entries_and_sequences_the_new_ones(monkeypatch):
    from se_snmf_nat_amd import _lib, batch, train
    monkeypatch.setattr(_lib, "load", lambda: FakeLib())

    class Ctx:
        _h = None
    F, T = 6, 5
    V, B = np.ones((F, T)), np.ones((F, 5))
    p = dict(cf="kl", sparsity=0.1, max_iter=3, cost_check=1)

    def reached(fn, *a, **k):
        with pytest.raises(Reached) as e:
            fn(*a, ctx=Ctx(), **k)
        return e.value

    for prec, name in (("fp32", "snmf_run_basis_dnmf_batch_f64"), ("fp64", "snmf_run_basis_dnmf_batch_fp64")):
        e = reached(batch.run_basis_dnmf_batch, [V, V], [V, V], [V, V], B, 2, 3, p, precision=prec)
        assert e.name == name and e.args_[2:5] == (2, 3, 2)  # (R_x, R_d, n_problems: the uniform argument list)
    e = reached(batch.run_basis_dnmf_batch, [V, V], [V, V], [V, V], B, [2, 2], [3, 3], p, precision="fp64")
    assert e.name == "snmf_run_basis_dnmf_batch_ranks_fp64" and e.args_[4] is None and e.args_[5] == 2  # s = NULL, n_problems
    e = reached(batch.run_basis_dnmf_batch, [V, V], [V, V], [V, V], B, 2, 3, p, precision="fp64", settings=[dict(max_iter=7), dict(cf="ed")])
    assert e.name == "snmf_run_basis_dnmf_batch_ranks_fp64"
    s = e.args_[4]
    assert [(q.beta, q.sparsity, q.conv_eps, q.max_iter, q.reserved) for q in s] == [(1.0, 0.1, 0.0, 7, 0), (2.0, 0.1, 0.0, 3, 0)]
    assert e.args_[1]._obj.max_iter == 7 and e.args_[1]._obj.r == 5  # params: the largest limit, the largest R_x + R_d

    w = ac.waves()
    xs, ds = [w[2][0], w[0][0]], [w[2][1], w[0][1]]
    Bw = np.ones((ac.F, ac.R_X + ac.R_D))
    for prec, name in (("fp32", "snmf_run_basis_dnmf_audio_batch_f64"), ("fp64", "snmf_run_basis_dnmf_audio_batch_fp64")):
        assert reached(train.run_basis_DNMF_batch, xs, ds, Bw, ac.P_STOP, precision=prec).name == name
    pl = dict(ac.P_STOP, R_x=[ac.R_X] * 2, R_d=[ac.R_D] * 2)
    assert reached(train.run_basis_DNMF_batch, xs, ds, Bw, pl, precision="fp64").name == "snmf_run_basis_dnmf_audio_batch_ranks_fp64"
    bm = np.ones((ac.TINY["F_order"], ac.R_X + ac.R_D))
    assert reached(train.run_basis_DNMF_Mel_batch, xs, ds, bm, pl, precision="fp64", h0="device").name == "snmf_run_basis_dnmf_audio_batch_ranks_fp64"


def test_host_h0_draw_for_equal_ranks_is_the_uniform_draw(monkeypatch):
    """The H0 arrays the two paths hand to the library are the same for equal pairs, and with differing ranks the draw is
    rand(r_k, T_k) per problem in list order from one generator."""
    from se_snmf_nat_amd import _lib, batch
    monkeypatch.setattr(_lib, "load", lambda: FakeLib())

    class Ctx:
        _h = None
    F = 6
    Ts = [5, 1, 8]
    Vs = [np.ones((F, T)) for T in Ts]
    p = dict(cf="kl", sparsity=0.1, max_iter=3, cost_check=1, random_seed=7)

    def h0_of(R_x, R_d, B, at, rs):
        with pytest.raises(Reached) as e:
            batch.run_basis_dnmf_batch(Vs, Vs, Vs, B, R_x, R_d, p, precision="fp64", ctx=Ctx())
        ptrs = e.value.args_[at]
        return [np.ctypeslib.as_array(C.cast(ptrs[k], C.POINTER(C.c_double)), (Ts[k] * rs[k],)).reshape((rs[k], Ts[k]), order="F").copy()
                for k in range(3)]

    uni = h0_of(2, 3, np.ones((F, 5)), 10, [5] * 3)
    lst = h0_of([2, 2, 2], [3, 3, 3], np.ones((F, 5)), 11, [5] * 3)
    rng = np.random.RandomState(7)
    for a, b, T in zip(uni, lst, Ts):
        assert np.array_equal(a, b) and np.array_equal(a, rng.random_sample((5, T)))
    rs = [3, 5, 2]
    mixed = h0_of([2, 1, 1], [1, 4, 1], [np.ones((F, r)) for r in rs], 11, rs)
    rng = np.random.RandomState(7)
    for a, r, T in zip(mixed, rs, Ts):
        assert np.array_equal(a, rng.random_sample((r, T)))


def test_c_names_stand_in_the_header_and_in_the_binding_once():
    from se_snmf_nat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snmf.h")).read(), flags=re.S)
    for nm in C_NAMES:
        assert len(re.findall(r"\b%s\s*\(" % nm, txt)) == 1, nm
        assert _lib.SYMBOLS.count(nm) == 1, nm
    whole = open(os.path.join(ROOT, "include", "snmf.h")).read()
    assert "no DNMF form" not in whole


def test_c_entries_refuse_bad_arguments_without_a_device(lib):
    """What the entries refuse comes before the device is touched, so it can be checked where there is none: here, what comes
    before the context is looked at."""
    from se_snmf_nat_amd.api import _make_params
    sp = _make_params(8, 1, 5, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    assert lib.snmf_run_basis_dnmf_batch_ranks_fp64(None, C.byref(sp), None, None, None, 1, None, None, None, None, None, None, None, None, None) == 1
    assert lib.snmf_run_basis_dnmf_audio_batch_ranks_fp64(None, C.byref(sp), None, None, None, None, 1, None, None, None, None, None, 0, None, None,
                                                          None, None, None, None) == 1


def test_the_problems_stop_where_the_gpu_tests_need_them_to():
    """On the oracle: with the shared settings the solve-1 counts hold max_iter, a smaller odd and a smaller even count; with the
    settings per problem one problem ends at a limit of its own below the largest and one after a single iteration."""
    shared = [n for _, _, n in rc.oracle(False)]
    own = [n for _, _, n in rc.oracle(True)]
    print("oracle, shared settings:", shared)
    print("oracle, settings per problem:", own)
    assert shared == rc.TRIPLES_SHARED and own == rc.TRIPLES_SETTINGS
    assert dc.covers_both_buffers([n[0] for n in shared], rc.P_EDGES["max_iter"])
    mi = [s["max_iter"] for s in rc.SETTINGS]
    assert own[3] == [13] * 3 and mi[3] == 13 < max(mi) and rc.SETTINGS[3]["conv_eps"] == 0
    assert own[5] == [1, 1, 1]
    for res in (rc.oracle(False), rc.oracle(True)):
        assert all(np.isfinite(b).all() and np.isfinite(a).all() for b, a, _ in res)
