"""GPU tests of the snmf_batch handle's state machine (include/snmf.h: snmf_batch_*), the same in the fp32 mode (BatchPlan) and
in the fp64 mode (BatchPlan64): what is refused before a run, run(n) and its continuation, a new batch on a used handle, and
the sparsity vector.  The host driver of the two modes is one (csrc/snmf_batch_host.h), and these are the cases that run it.

Nothing is compared across the modes or against an oracle here (test_gpu_batch.py and test_gpu_batch_f64.py do that): every
comparison is between two runs of the same mode, in bytes.  F = 65, r = 8 and the frame counts (7, 31, 100) are the smallest
shapes with a second row tile, a one-tile and a multi-tile problem and a ragged last tile; with conv_eps = 1e-3 and
max_iter = 31 (the problems of the stop cases of the two files above) two problems stop early and one reaches max_iter."""
import ctypes as C

import numpy as np
import pytest

from oracle.sparse_nmf_oracle import synth_problem

pytestmark = pytest.mark.gpu

F, R, TS = 65, 8, (7, 31, 100)
PS = dict(beta=1.0, max_iter=31, conv_eps=1e-3, sparsity=5)
MODES = ["BatchPlan", "BatchPlan64"]
STATE = 7  # SNMF_ERR_STATE


def _problems(other=False):
    if other:
        return [synth_problem(F, T, R, seed_data=500 + k, seed_init=600 + k, r_true=4) for k, T in enumerate(TS)]
    return [synth_problem(F, T, R, seed_data=10 * b, seed_init=10 * b + 1, r_true=4) for b, T in ((5, 7), (1, 31), (3, 100))]


def _plan(mode, ctx, **kw):
    import se_snmf_nat_amd
    return getattr(se_snmf_nat_amd, mode)(ctx, F, R, TS, **dict(PS, **kw))


def _fill(bp, probs):
    for k, q in enumerate(probs):
        bp.set_problem(k, *q)


def _results(bp):
    return [bp.get(k) for k in range(len(TS))]


def _refused(call):
    from se_snmf_nat_amd import SnmfError
    with pytest.raises(SnmfError) as e:
        call()
    assert e.value.status == STATE, e.value
    return e.value.message


def _same_bytes(a, b, what):
    (w, h, o), (w2, h2, o2) = a, b
    assert o["n_iter"] == o2["n_iter"], (what, o["n_iter"], o2["n_iter"])
    assert w.dtype == w2.dtype and h.dtype == h2.dtype and w.shape == w2.shape and h.shape == h2.shape
    assert w.tobytes() == w2.tobytes(), (what, "W")
    assert h.tobytes() == h2.tobytes(), (what, "H")
    assert o["div"].tobytes() == o2["div"].tobytes(), (what, "div")
    assert o["cost"].tobytes() == o2["cost"].tobytes(), (what, "cost")


_ONE_RUN = {}


def _one_run(mode, ctx, other=False):
    """Every problem of a fresh plan after one run(): the reference of the mode, computed once."""
    if (mode, other) not in _ONE_RUN:
        bp = _plan(mode, ctx)
        _fill(bp, _problems(other))
        bp.run()
        _ONE_RUN[mode, other] = _results(bp)
        bp.close()
    return _ONE_RUN[mode, other]


@pytest.mark.parametrize("mode", MODES)
def test_run_and_get_are_refused_before_their_time(gpu_ctx, mode):
    probs = _problems()
    bp = _plan(mode, gpu_ctx)
    _refused(bp.run)  # no problem is set
    for k, q in enumerate(probs):
        _refused(bp.run)  # k of 3 are set
        _refused(lambda: bp.get(0))
        bp.set_problem(k, *q)
    _refused(lambda: bp.get(0))  # every problem is set, nothing has run
    bp.run()
    for k, (x, y) in enumerate(zip(_results(bp), _one_run(mode, gpu_ctx))):
        _same_bytes(x, y, f"{mode} after the refusals[{k}]")
    bp.close()


@pytest.mark.parametrize("mode", MODES)
def test_continuation_and_a_new_batch_on_the_same_handle(gpu_ctx, mode):
    base = _one_run(mode, gpu_ctx)
    n_iters = [o["n_iter"] for _, _, o in base]
    print(mode, "n_iter", n_iters)
    assert min(n_iters) < PS["max_iter"] and all(n > 3 for n in n_iters)  # a problem stops early, none within the first run(3)
    bp = _plan(mode, gpu_ctx)
    _fill(bp, _problems())
    bp.run(3)
    for k, ((_, _, o), (_, _, ob)) in enumerate(zip(_results(bp), base)):
        assert o["n_iter"] == 3, (k, o["n_iter"])
        assert len(o["cost"]) == 3 and len(o["div"]) == 3, k
        assert o["cost"].tobytes() == ob["cost"][:3].tobytes() and o["div"].tobytes() == ob["div"][:3].tobytes(), k
    bp.run()
    for k, (x, y) in enumerate(zip(_results(bp), base)):
        _same_bytes(x, y, f"{mode} run(3) + run()[{k}]")
    # a set_problem after a run starts a new batch: run is refused until every problem is set again, then other data in the
    # same slots give what a fresh plan gives
    other = _problems(other=True)
    for k, q in enumerate(other):
        bp.set_problem(k, *q)
        if k + 1 < len(other):
            assert "problems are set" in _refused(bp.run)
            _refused(lambda: bp.get(0))
    bp.run()
    fresh = _one_run(mode, gpu_ctx, other=True)
    for k, (x, y) in enumerate(zip(_results(bp), fresh)):
        _same_bytes(x, y, f"{mode} reuse[{k}]")
    assert fresh[0][0].tobytes() != base[0][0].tobytes()
    bp.close()


@pytest.mark.parametrize("mode", MODES)
def test_the_sparsity_vector_before_and_after_a_run(gpu_ctx, lib, mode):
    from se_snmf_nat_amd.api import _make_params, _ptr
    probs = _problems()
    vec = np.linspace(0.0, 9.0, R)
    # after a run the vector is fixed
    bp = _plan(mode, gpu_ctx, sparsity=vec)
    _fill(bp, probs)
    bp.run(2)
    assert lib.snmf_batch_set_sparsity_f64(bp._h, _ptr(vec)) == STATE
    assert b"after snmf_batch_run" in lib.snmf_last_error()
    bp.run()
    done = _results(bp)
    bp.close()
    # a handle made for an r-vector that was never given one does not run (BatchPlan sets the vector itself: the C entries)
    sp = _make_params(F, 1, R, 1.0, PS["max_iter"], PS["conv_eps"], 1, 1, 1, 0.0, None, None)
    T = np.array(TS, np.int32)
    h = C.c_void_p()
    create = lib.snmf_batch_create if mode == "BatchPlan" else lib.snmf_batch_create_fp64
    assert create(gpu_ctx._h, C.byref(sp), len(TS), _ptr(T), C.byref(h)) == 0
    try:
        arrs = [[np.asfortranarray(a, dtype=np.float64) for a in q] for q in probs]
        for k, (V, W0, H0) in enumerate(arrs):
            assert lib.snmf_batch_set_problem_f64(h, k, _ptr(V), F, _ptr(W0), _ptr(H0)) == 0
        gpu_ctx.sync()
        assert lib.snmf_batch_run(h, 0) == STATE
        assert b"sparsity vector is not set" in lib.snmf_last_error()
        # and with the vector it runs, to the results of the plan above
        assert lib.snmf_batch_set_sparsity_f64(h, _ptr(vec)) == 0
        assert lib.snmf_batch_run(h, 0) == 0
        for k, (w, hh, o) in enumerate(done):
            W, H = np.empty_like(w), np.empty_like(hh)
            ni = C.c_int32()
            assert lib.snmf_batch_get_f64(h, k, _ptr(W), _ptr(H), None, None, C.byref(ni)) == 0
            assert ni.value == o["n_iter"] and W.tobytes() == w.tobytes() and H.tobytes() == hh.tobytes(), k
    finally:
        lib.snmf_batch_destroy(h)
