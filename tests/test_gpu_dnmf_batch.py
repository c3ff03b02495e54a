"""GPU tests of run_basis_dnmf_batch (snmf_run_basis_dnmf_batch_*): many DNMF re-trainings in three resident batches.

The contract is bit equality with what is already shipped.  In the fp64 mode problem k is run_basis_dnmf(..., precision="fp64",
h0=H0_k) alone; in the fp32 mode it is three chained sparse_nmf_batch calls, A_hat going through the host.  The "edges" batch
(dnmf_batch_cases.py) puts the hand-off of A_hat on every edge of the two layouts.  Against the oracle the bounds are the
imported ones of the single DNMF tests.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dnmf_batch_cases as dc
from test_gpu_parity import REL_WH
from test_gpu_train_f64 import REL_SOLVE

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = ["fp32", "fp64"]
SETTINGS = {"kl": dc.P_EDGES, "ed": dict(dc.P_EDGES, cf="ed"), "b05": dict(dc.P_EDGES, cf="beta", beta=0.5)}


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def run_batch(ctx, probs, p, mode, B=None, **kw):
    """-> [(B_hat, A_hat, [n1, n2, n3])] of one run_basis_dnmf_batch call on [(Y, X, D, B, H0)]."""
    from se_snmf_nat_amd import run_basis_dnmf_batch
    info = {}
    out = run_basis_dnmf_batch([q[0] for q in probs], [q[1] for q in probs], [q[2] for q in probs],
                               [q[3] for q in probs] if B is None else B, dc.R_X, dc.R_D, p, ctx=ctx, h0=[q[4] for q in probs],
                               precision=mode, info=info, **kw)
    return [(b, a, n) for (b, a), n in zip(out, info["n_iter"])]


def reference(ctx, probs, p, mode, R_x=dc.R_X, R_d=dc.R_D):
    """What the contract names: the single fp64 loop per problem, or three chained sparse_nmf_batch calls."""
    from se_snmf_nat_amd import run_basis_dnmf, sparse_nmf_batch
    r = R_x + R_d
    if mode == "fp64":
        out = []
        for Y, X, D, B, H0 in probs:
            info = {}
            b, a = run_basis_dnmf(Y, X, D, B, R_x, R_d, p, ctx=ctx, precision="fp64", h0=H0, info=info)
            out.append((b, a, info["n_iter"]))
        return out
    Ys, Xs, Ds, Bs, H0s = (list(c) for c in zip(*probs))
    s1 = sparse_nmf_batch(Ys, dict(p, init_w=Bs, init_h=H0s, w_update_ind=np.zeros(r, bool), h_update_ind=np.ones(r, bool)), ctx=ctx)
    A = [h for _, h, _ in s1]
    s2 = sparse_nmf_batch(Xs, dict(p, init_w=[b[:, :R_x] for b in Bs], init_h=[a[:R_x] for a in A], w_update_ind=np.ones(R_x, bool),
                                   h_update_ind=np.zeros(R_x, bool)), ctx=ctx)
    s3 = sparse_nmf_batch(Ds, dict(p, init_w=[b[:, R_x:] for b in Bs], init_h=[a[R_x:] for a in A], w_update_ind=np.ones(R_d, bool),
                                   h_update_ind=np.zeros(R_d, bool)), ctx=ctx)
    return [(np.concatenate([w2, w3], axis=1), a, [o1["n_iter"], o2["n_iter"], o3["n_iter"]])
            for (_, a, o1), (w2, _, o2), (w3, _, o3) in zip(s1, s2, s3)]


_cache = {}


def edges_batch(ctx, mode, setting="kl"):
    """The "edges" batch on the device, once per (mode, setting); the arrays are shared and read only."""
    key = (mode, setting)
    if key not in _cache:
        _cache[key] = run_batch(ctx, edges(), SETTINGS[setting], mode)
        for b, a, _ in _cache[key]:
            b.setflags(write=False)
            a.setflags(write=False)
    return _cache[key]


@functools.lru_cache(maxsize=None)
def edges():
    return dc.edges()


def same_bits(res, ref):
    assert len(res) == len(ref)
    for k, ((b, a, n), (br, ar, nr)) in enumerate(zip(res, ref)):
        assert list(n) == list(nr), (k, n, nr)
        assert b.shape == br.shape and a.shape == ar.shape
        assert np.array_equal(b, br), (k, "B_hat", float(np.abs(b - br).max()))
        assert np.array_equal(a, ar), (k, "A_hat", float(np.abs(a - ar).max()))


@pytest.mark.parametrize("mode", MODES)
def test_edges_equal_the_shipped_paths_bit_for_bit(gpu_ctx, mode):
    res = edges_batch(gpu_ctx, mode)
    n1 = [n[0] for _, _, n in res]
    print(f"{mode}: n_iter per problem {[n for _, _, n in res]}")
    assert dc.covers_both_buffers(n1, dc.P_EDGES["max_iter"]), n1  # the stop iterate lies in either H buffer
    same_bits(res, reference(gpu_ctx, edges(), dc.P_EDGES, mode))
    for b, a, _ in res:
        assert b.dtype == a.dtype == np.float64 and np.isfinite(b).all() and np.isfinite(a).all()


@pytest.mark.parametrize("mode", MODES)
def test_a_problem_does_not_depend_on_the_batch_around_it(gpu_ctx, mode):
    res = edges_batch(gpu_ctx, mode)
    alone = [run_batch(gpu_ctx, [q], dc.P_EDGES, mode)[0] for q in edges()]
    same_bits(alone, res)
    rev = run_batch(gpu_ctx, edges()[::-1], dc.P_EDGES, mode)
    same_bits(rev[::-1], res)


@pytest.mark.parametrize("mode", MODES)
def test_one_basis_equals_a_list_of_equal_bases(gpu_ctx, mode):
    B0 = edges()[0][3]
    one = run_batch(gpu_ctx, edges(), dc.P_EDGES, mode, B=B0)
    many = run_batch(gpu_ctx, edges(), dc.P_EDGES, mode, B=[B0.copy() for _ in edges()])
    same_bits(one, many)
    assert not np.array_equal(one[1][0], edges_batch(gpu_ctx, mode)[1][0])  # (and B is read: another basis, another result)


@pytest.mark.parametrize("setting", ["ed", "b05"])
@pytest.mark.parametrize("mode", MODES)
def test_two_image_modes_equal_the_shipped_paths_bit_for_bit(gpu_ctx, mode, setting):
    same_bits(edges_batch(gpu_ctx, mode, setting), reference(gpu_ctx, edges(), SETTINGS[setting], mode))


@pytest.mark.parametrize("mode", MODES)
def test_golden_loop_as_one_problem_of_three(gpu_ctx, mode):
    """tests/golden/dnmf_loop_513x64_r20_20.npz as problem 1; problems 0 and 2 are its first 33 columns and its columns reversed."""
    from se_snmf_nat_amd import run_basis_dnmf_batch
    ref = dict(np.load(os.path.join(GOLD, "ref_data.npz")))
    d = dict(np.load(os.path.join(GOLD, "dnmf_loop_513x64_r20_20.npz")))
    Y = ref["Y"]
    X = (Y * d["mask"] + 1e-9).astype(np.float32)
    D = (Y - X + 2e-9).astype(np.float32)
    Bs = np.concatenate([ref["B"][:, :20], ref["B"][:, 100:120]], axis=1)
    p = dict(cf="kl", sparsity=5, max_iter=30, conv_eps=1e-3, cost_check=1)
    H0 = np.random.RandomState(1).random_sample((40, Y.shape[1]))  # the draw of the single loop (random_seed = 1)
    cut = [lambda M: M[:, :33], lambda M: M, lambda M: M[:, ::-1]]
    Ys, Xs, Ds, H0s = ([np.asarray(c(M), dtype=np.float64) for c in cut] for M in (Y, X, D, H0))
    info = {}
    out = run_basis_dnmf_batch(Ys, Xs, Ds, Bs, 20, 20, p, ctx=gpu_ctx, h0=H0s, precision=mode, info=info)
    bound = REL_WH if mode == "fp32" else REL_SOLVE
    orc = [dc.oracle_dnmf(Ys[k], Xs[k], Ds[k], np.asarray(Bs, dtype=np.float64), H0s[k], 20, 20, p) for k in range(3)]
    assert rel(orc[1][0], d["B_hat"]) < 1e-12 and rel(orc[1][1], d["A_hat"]) < 1e-12  # (the oracle restated here IS the golden file's)
    for k, ((b, a), (br, ar, nr)) in enumerate(zip(out, orc)):
        print(f"{mode} golden problem {k}: n_iter {info['n_iter'][k]} (oracle {nr}) relB={rel(b, br):.2e} relA={rel(a, ar):.2e}")
    for k, ((b, a), (br, ar, _)) in enumerate(zip(out, orc)):
        assert rel(b, br) < bound and rel(a, ar) < bound, k
    assert rel(out[1][0], d["B_hat"]) < bound and rel(out[1][1], d["A_hat"]) < bound


def test_host_types_of_the_fp32_engine_agree(gpu_ctx):
    """_f32 with float32 arrays equals _f64 with the same values widened: A_hat exactly (the engine's H is fp32), B_hat as the
    fp64 master copy rounded once."""
    probs32 = [tuple(np.asarray(m, dtype=np.float32) for m in q) for q in edges()]
    wide = run_batch(gpu_ctx, [tuple(m.astype(np.float64) for m in q) for q in probs32], dc.P_EDGES, "fp32")
    narrow = run_batch(gpu_ctx, probs32, dc.P_EDGES, "fp32", dtype=np.float32)
    for (b, a, n), (bw, aw, nw) in zip(narrow, wide):
        assert b.dtype == a.dtype == np.float32 and n == nw
        assert np.array_equal(b, bw.astype(np.float32))
        assert np.array_equal(a.astype(np.float64), aw)


def test_c_entries_refuse_with_the_documented_status_and_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd.api import _make_params
    F, T, Rx, Rd = 33, 40, 5, 7
    r = Rx + Rd

    def call(ty, *, F=F, Rx=Rx, Rd=Rd, r=r, n=2, Ts=(T, T), kind=0, null=None, null_entry=None, ctx=gpu_ctx._h):
        dt = np.float32 if ty == "f32" else np.float64
        sp = _make_params(F, 1, r, 1.0, 3, 0.0, 1, True, kind, 0.1, None, None)
        Tv = np.array(Ts, np.int32)
        m = max(n, 1)
        Tm = max(max(Ts), 1)
        arr = dict(Y=(F, Tm), X=(F, Tm), D=(F, Tm), B=(F, max(r, 1)), H0=(max(r, 1), Tm), B_hat=(F, max(r, 1)), A_hat=(max(r, 1), Tm))
        keep = {k: [np.ones(s, dtype=dt, order="F") for _ in range(m)] for k, s in arr.items()}
        ptr = {k: (C.c_void_p * m)(*[a.ctypes.data for a in v]) for k, v in keep.items()}
        if null_entry:
            ptr[null_entry][m - 1] = None
        args = [None if null == k else ptr[k] for k in ("Y", "X", "D", "B", "H0", "B_hat", "A_hat")]
        n_iter = np.zeros(3 * m, np.int32)
        return getattr(lib, f"snmf_run_basis_dnmf_batch_{ty}")(ctx, None if null == "p" else C.byref(sp), Rx, Rd, n,
                                                                None if null == "T" else C.c_void_p(Tv.ctypes.data), *args,
                                                                C.c_void_p(n_iter.ctypes.data))

    before = {m: edges_batch(gpu_ctx, m) for m in MODES}
    for ty in ("f64", "f32", "fp64"):
        assert call(ty, ctx=None) == 1
        for nm in ("p", "T", "Y", "X", "D", "B", "H0", "B_hat"):
            assert call(ty, null=nm) == 1, (ty, nm)
        for nm in ("Y", "X", "D", "B", "H0", "B_hat"):
            assert call(ty, null_entry=nm) == 1, (ty, nm)
        assert call(ty, n=0) == 1
        assert call(ty, Ts=(T, 0)) == 1
        assert call(ty, Rx=0, r=Rd) == 3
        assert call(ty, Rd=0, r=Rx) == 3
        assert call(ty, r=r + 1) == 3
        assert call(ty, kind=1) == 3 and call(ty, kind=2) == 3  # an r-vector and an r x n sparsity
        assert call(ty, null="A_hat") == 0 and call(ty, null_entry="A_hat") == 0  # A_hat is optional, whole or per problem
    for ty in ("f64", "f32"):  # the fp32 batch's envelope, with its message
        assert call(ty, F=600) == 8 and b"limit of 513 rows" in lib.snmf_last_error()
        assert call(ty, Rx=150, Rd=150, r=300) == 8 and b"limit of 200 components" in lib.snmf_last_error()
    assert call("fp64", F=600) == 0  # (no such limit in the fp64 mode)
    for m in MODES:  # a valid batch afterwards still gives the earlier bits
        same_bits(run_batch(gpu_ctx, edges(), dc.P_EDGES, m), before[m])
