"""GPU tests of the DNMF batches with a rank pair and settings per problem (snmf_run_basis_dnmf_batch_ranks_fp64,
snmf_run_basis_dnmf_audio_batch_ranks_fp64; run_basis_dnmf_batch / run_basis_DNMF_batch / run_basis_DNMF_Mel_batch with sequences
for R_x / R_d and settings=[...]).

The contract is bit equality (np.array_equal) with the single fp64 loop run alone on problem k at its own ranks and settings --
whatever the ranks, settings, sizes and order of the problems around it -- and, for equal pairs, with the uniform batch.  Against
the oracle the bound is the imported one of the fp64 DNMF batch tests (tests/test_gpu_dnmf_batch.py: REL_SOLVE).  The problems
are those of dnmf_batch_ranks_cases.py; test_dnmf_batch_ranks_api.py checks on the oracle that they stop where these tests need.
"""
import ctypes as C

import numpy as np
import pytest

import dnmf_audio_batch_cases as ac
import dnmf_batch_cases as dc
import dnmf_batch_ranks_cases as rc
from test_gpu_train_f64 import REL_SOLVE

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def same_bits(res, ref):
    assert len(res) == len(ref)
    for k, ((b, a, n), (br, ar, nr)) in enumerate(zip(res, ref)):
        assert list(n) == list(nr), (k, n, nr)
        assert b.shape == br.shape and a.shape == ar.shape, (k, b.shape, br.shape, a.shape, ar.shape)
        assert np.array_equal(b, br), (k, "B_hat", float(np.abs(b - br).max()))
        assert np.array_equal(a, ar), (k, "A_hat", float(np.abs(a - ar).max()))


def run_batch(ctx, order, settings=False, pairs=None, probs=None, **kw):
    """-> [(B_hat, A_hat, [n1, n2, n3])] of ONE run_basis_dnmf_batch call on the problems `order` of the cases."""
    from se_snmf_nat_amd import run_basis_dnmf_batch
    probs = rc.problems() if probs is None else probs
    pairs = rc.PAIRS if pairs is None else pairs
    q = [probs[k] for k in order]
    info = {}
    out = run_basis_dnmf_batch([v[0] for v in q], [v[1] for v in q], [v[2] for v in q], [v[3] for v in q], [pairs[k][0] for k in order],
                               [pairs[k][1] for k in order], rc.P_EDGES, ctx=ctx, h0=[v[4] for v in q], precision="fp64", info=info,
                               settings=[rc.SETTINGS[k] for k in order] if settings else None, **kw)
    return [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
        for b, a, _ in _cache[key]:
            b.setflags(write=False)
            a.setflags(write=False)
    return _cache[key]


def whole_batch(ctx, settings=False):
    return cached(("batch", settings), lambda: run_batch(ctx, range(len(rc.PAIRS)), settings))


def alone(ctx, settings=False):
    """run_basis_dnmf(..., precision="fp64", h0=H0_k) per problem at its own ranks (and settings): the contract's reference."""
    from se_snmf_nat_amd import run_basis_dnmf

    def make():
        out = []
        for k, ((Y, X, D, B, H0), (rx, rd)) in enumerate(zip(rc.problems(), rc.PAIRS)):
            info = {}
            b, a = run_basis_dnmf(Y, X, D, B, rx, rd, rc.p_of(k) if settings else rc.P_EDGES, ctx=ctx, precision="fp64", h0=H0, info=info)
            out.append((b, a, info["n_iter"]))
        return out
    return cached(("alone", settings), make)


def test_mixed_pairs_equal_the_single_loop_bit_for_bit(gpu_ctx):
    res = whole_batch(gpu_ctx)
    print("n_iter per problem:", [n for _, _, n in res])
    for k, ((b, a, n), (bo, ao, no)) in enumerate(zip(res, rc.oracle(False))):
        print(f"problem {k} pair {rc.PAIRS[k]} T={rc.TS[k]}: n_iter {n} (oracle {no}) relB={rel(b, bo):.2e} relA={rel(a, ao):.2e}")
    same_bits(res, alone(gpu_ctx))
    for (b, a, _), (rx, rd), T in zip(res, rc.PAIRS, rc.TS):
        assert b.shape == (rc.F, rx + rd) and a.shape == (rx + rd, T)
        assert b.dtype == a.dtype == np.float64 and np.isfinite(b).all() and np.isfinite(a).all()
    for k, ((b, a, _), (bo, ao, _)) in enumerate(zip(res, rc.oracle(False))):
        assert rel(b, bo) < REL_SOLVE and rel(a, ao) < REL_SOLVE, k


def test_a_problem_does_not_depend_on_the_batch_around_it(gpu_ctx):
    res = whole_batch(gpu_ctx)
    n = len(rc.PAIRS)
    same_bits(run_batch(gpu_ctx, range(n)[::-1])[::-1], res)
    sub = [1, 4, 2]
    same_bits(run_batch(gpu_ctx, sub), [res[k] for k in sub])


def test_equal_pairs_as_lists_equal_the_uniform_batch(gpu_ctx):
    from se_snmf_nat_amd import run_basis_dnmf_batch
    probs = dc.edges()
    n = len(probs)
    info = {}
    out = run_basis_dnmf_batch([q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs], [q[3] for q in probs], dc.R_X, dc.R_D,
                               dc.P_EDGES, ctx=gpu_ctx, h0=[q[4] for q in probs], precision="fp64", info=info)
    uniform = [(b, a, m) for (b, a), m in zip(out, info["n_iter"])]
    lists = run_batch(gpu_ctx, range(n), pairs=[(dc.R_X, dc.R_D)] * n, probs=probs)
    same_bits(lists, uniform)
    assert dc.covers_both_buffers([m[0] for _, _, m in lists], dc.P_EDGES["max_iter"])


def test_settings_per_problem_equal_the_single_loop_with_its_own_settings(gpu_ctx):
    res = whole_batch(gpu_ctx, settings=True)
    print("n_iter per problem:", [n for _, _, n in res])
    same_bits(res, alone(gpu_ctx, settings=True))
    assert res[3][2] == [13, 13, 13] and res[5][2] == [1, 1, 1]
    for k, ((b, a, n), (bo, ao, no)) in enumerate(zip(res, rc.oracle(True))):
        print(f"problem {k} {rc.SETTINGS[k]}: n_iter {n} (oracle {no}) relB={rel(b, bo):.2e} relA={rel(a, ao):.2e}")
        assert np.isfinite(b).all() and np.isfinite(a).all()
    assert not np.array_equal(res[1][0], whole_batch(gpu_ctx)[1][0])  # (the settings are read: other settings, another result)
    same_bits(run_batch(gpu_ctx, [5, 3, 0], settings=True), [res[k] for k in (5, 3, 0)])  # (and they travel with their problem)


# ---- waveforms ---------------------------------------------------------------------------------------------------------------
W_KS = [2, 0, 4]                   # of dnmf_audio_batch_cases.waves(): 31 frames, ONE frame, 33 frames
W_PAIRS = [(3, 2), (1, 4), (5, 1)]
W_SETTINGS = [dict(cf="ed", sparsity=0.5, max_iter=9), dict(cf="kl", sparsity=2.0, max_iter=13, conv_eps=0), dict(cf="x", beta=1.5, sparsity=0.1)]


def wave_bases(rows):
    rng = np.random.default_rng(3)
    return [rng.random((rows, rx + rd)) + 0.05 for rx, rd in W_PAIRS]


@pytest.mark.parametrize("mel,h0,settings", [(False, "host", False), (False, "device", False), (True, "host", False), (True, "device", False),
                                             (False, "host", True), (True, "given", True)])
def test_waveforms_equal_the_single_callers_bit_for_bit(gpu_ctx, mel, h0, settings):
    from se_snmf_nat_amd import train
    if h0 == "given":
        h0 = [np.random.RandomState(20 + i).random_sample((rx + rd, ac.TS[k])) for i, (k, (rx, rd)) in enumerate(zip(W_KS, W_PAIRS))]
    xs, ds = [ac.waves()[k][0] for k in W_KS], [ac.waves()[k][1] for k in W_KS]
    Bs = wave_bases(ac.TINY["F_order"] if mel else ac.F)
    p = dict(ac.P_STOP, R_x=[a for a, _ in W_PAIRS], R_d=[b for _, b in W_PAIRS])
    info = {}
    fn = train.run_basis_DNMF_Mel_batch if mel else train.run_basis_DNMF_batch
    out = fn(xs, ds, Bs, p, ctx=gpu_ctx, h0=h0, precision="fp64", info=info, settings=W_SETTINGS if settings else None)
    assert info["T"] == [ac.TS[k] for k in W_KS]
    print("n_iter per problem:", info["n_iter"])
    seed = ac.P_STOP["random_seed"]
    rng = np.random.RandomState(seed)  # the list-order draw of h0="host"
    ref = []
    for i, (rx, rd) in enumerate(W_PAIRS):
        q = dict(ac.P_STOP, R_x=rx, R_d=rd, **(W_SETTINGS[i] if settings else {}))
        if isinstance(h0, list):
            h = h0[i]
        elif h0 == "host":
            h = rng.random_sample((rx + rd, ac.TS[W_KS[i]]))
        else:
            h, q = "device", dict(q, random_seed=seed + i)
        one = {}
        b, a = train._run_basis_dnmf_audio(xs[i], ds[i], Bs[i], q, ctx=gpu_ctx, mel=mel, h0=h, want_a=True, precision="fp64", info=one)
        ref.append((b, a, one["n_iter"]))
    same_bits([(b, a, n) for (b, a), n in zip(out, info["n_iter"])], ref)
    if settings:
        assert info["n_iter"][1] == [13, 13, 13]  # (conv_eps = 0: the problem's own limit, below the largest)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_with_the_documented_status_and_leaves_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import _lib
    from se_snmf_nat_amd.api import _make_params
    F, T = 33, 40
    Rx, Rd = [5, 1, 3], [7, 2, 3]

    def call(*, Rx=Rx, Rd=Rd, r=12, max_iter=3, s=None, null=(), kind=0, ctx=gpu_ctx._h):
        n = 3
        sp = _make_params(F, 1, r, 1.0, max_iter, 0.0, 1, True, kind, 0.1, None, None)
        rs = [max(a + b, 1) for a, b in zip(Rx, Rd)]
        shapes = dict(Y=lambda r_: (F, T), X=lambda r_: (F, T), D=lambda r_: (F, T), B=lambda r_: (F, r_), H0=lambda r_: (r_, T),
                      B_hat=lambda r_: (F, r_), A_hat=lambda r_: (r_, T))
        keep = {k: [np.ones(f(r_), order="F") for r_ in rs] for k, f in shapes.items()}
        ptr = {k: (C.c_void_p * n)(*[a.ctypes.data for a in v]) for k, v in keep.items()}
        Tv, rx, rd = np.full(n, T, np.int32), np.array(Rx, np.int32), np.array(Rd, np.int32)
        sarr = None
        if s is not None:
            sarr = (_lib.SnmfProblemSettings * n)()
            for a, (beta, lam, eps, mi, res) in zip(sarr, s):
                a.beta, a.sparsity, a.conv_eps, a.max_iter, a.reserved = beta, lam, eps, mi, res
        n_iter = np.zeros(3 * n, np.int32)
        vp = lambda v: C.c_void_p(v.ctypes.data)  # noqa: E731
        return lib.snmf_run_basis_dnmf_batch_ranks_fp64(ctx, C.byref(sp), None if "R_x" in null else vp(rx), None if "R_d" in null else vp(rd), sarr,
                                                        n, vp(Tv), ptr["Y"], ptr["X"], ptr["D"], ptr["B"], ptr["H0"], ptr["B_hat"],
                                                        None if "A_hat" in null else ptr["A_hat"], vp(n_iter))

    ok = [(1.0, 0.1, 0.0, 3, 0), (2.0, 0.5, 0.0, 2, 0), (0.0, 0.1, 1e-3, 3, 0)]
    before = whole_batch(gpu_ctx)

    def still_usable():
        same_bits(run_batch(gpu_ctx, range(len(rc.PAIRS))), before)

    assert call() == 0 and call(s=ok) == 0 and call(null=("A_hat",)) == 0
    refusals = [
        (dict(null=("R_x",)), 3, None), (dict(null=("R_d",)), 3, None),       # as the uniform entry refuses a bad scalar
        (dict(Rd=[7, 0, 3]), 3, None), (dict(Rx=[5, 1, -2]), 3, None),
        (dict(kind=1), 3, None),                                              # an r-vector sparsity: likewise
        (dict(r=13), 3, b"largest"), (dict(r=11), 3, b"largest"),             # p->r is not the largest R_x[k] + R_d[k]
        (dict(s=ok, max_iter=4), 3, b"largest max_iter"),                     # p->max_iter is not the largest limit
        (dict(s=ok[:2] + [(0.0, 0.1, 1e-3, 3, 1)]), 1, b"problem 2"),         # a non-zero reserved
        (dict(s=[ok[0], (1.0, 0.1, 0.0, -1, 0), ok[2]]), 1, b"problem 1"),    # a field snmf_params would be refused for
        (dict(ctx=None), 1, None),
    ]
    for kw, status, msg in refusals:
        assert call(**kw) == status, kw
        if msg:
            assert msg in lib.snmf_last_error(), (kw, lib.snmf_last_error())
        still_usable()  # a valid call after the refusal gives the earlier bits
