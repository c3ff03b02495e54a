"""GPU tests of the batched offline solve (include/snmf.h: snmf_batch_*, snmf_sparse_nmf_batch_*; se_snmf_nat_amd/batch.py).

Every problem of a batch is held to the fp64 oracle with the single solve's bounds (test_gpu_parity: REL_WH = 1e-4 on W and
H, REL_COST = 1e-5 on every recorded cost and divergence, the exact stop index), and the batch is held to being a batch of
INDEPENDENT solves: per-problem stop indices, and bits that do not depend on the company a problem is solved in.
Shapes are the smallest that still reach every path: partial last tiles, one-frame tiles (T = 1, 33), the extra row
(F = 32n+1), unaligned F and r, two row groups (F = 513), the W'*ratio product cut 1, 2, 4 and 8 ways (r = 200 .. 8)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem
from test_gpu_parity import REL_COST, REL_WH, rel

pytestmark = pytest.mark.gpu


def _problems(F, Ts, r, seeds=None):
    seeds = seeds if seeds is not None else [10 * b for b in range(len(Ts))]
    return [synth_problem(F, T, r, seed_data=s, seed_init=s + 1, r_true=max(1, r // 2)) for T, s in zip(Ts, seeds)]


def _oracle(probs, ps, **kw):
    return [oracle_nmf(V, dict(ps, init_w=W0, init_h=H0), **kw) for V, W0, H0 in probs]


def _batch(probs, ps, ctx, **kw):
    from se_snmf_nat_amd import sparse_nmf_batch
    p = dict(ps, init_w=[q[1] for q in probs], init_h=[q[2] for q in probs])
    return sparse_nmf_batch([q[0] for q in probs], p, ctx=ctx, **kw)


def _check(res, refs, *, objective=True):
    assert len(res) == len(refs)
    for b, ((w, h, o), (wr, hr, orf)) in enumerate(zip(res, refs)):
        ew, eh = rel(w, wr), rel(h, hr)
        print(f"problem {b}: n_iter {o['n_iter']} (oracle {orf['n_iter']}) relW {ew:.2e} relH {eh:.2e}", end="")
        assert o["n_iter"] == orf["n_iter"], (b, o["n_iter"], orf["n_iter"])
        assert np.isfinite(w).all() and np.isfinite(h).all()
        assert ew < REL_WH, (b, ew)
        assert eh < REL_WH, (b, eh)
        assert np.abs(np.linalg.norm(w, axis=0) - 1.0).max() < 1e-6, b  # unit columns (:242)
        if objective:
            assert o["cost"].shape == orf["cost"].shape and o["div"].shape == orf["div"].shape, b
            if o["cost"].size:
                ec = np.max(np.abs(o["cost"] - orf["cost"]) / np.abs(orf["cost"]))
                ed = np.max(np.abs(o["div"] - orf["div"]) / np.abs(orf["div"]))
                print(f" relcost {ec:.2e} reldiv {ed:.2e}", end="")
                assert ec < REL_COST, (b, ec)
                assert ed < REL_COST, (b, ed)
        print()


def _same_bits(a, b):
    (w, h, o), (w2, h2, o2) = a, b
    assert o["n_iter"] == o2["n_iter"]
    assert np.array_equal(w, w2) and np.array_equal(h, h2)
    assert np.array_equal(o["cost"], o2["cost"]) and np.array_equal(o["div"], o2["div"])


# ---- 1. ragged batches against the oracle ---------------------------------------------------------------------------------
RAGGED = [
    ("kl_extra_row", 65, (1, 7, 31, 33, 100), 8, dict(cf="kl", sparsity=5, max_iter=80, conv_eps=1e-3)),
    ("kl_257", 257, (96, 200, 33, 640, 1), 40, dict(cf="kl", sparsity=5, max_iter=15)),
    ("ed_unaligned", 37, (131, 17, 64, 50), 13, dict(cf="ed", sparsity=0.5, max_iter=15)),
    ("is_129", 129, (300, 45, 96), 24, dict(cf="is", sparsity=0.1, max_iter=15)),
    ("kl_513", 513, (100, 300, 63), 100, dict(cf="kl", sparsity=5, max_iter=10)),
    ("kl_mel_64", 64, (200, 90, 33), 100, dict(cf="kl", sparsity=5, max_iter=10)),
    ("kl_513_r200", 513, (33, 257, 100), 200, dict(cf="kl", sparsity=5, max_iter=10)),
]


@pytest.mark.parametrize("case", RAGGED, ids=[c[0] for c in RAGGED])
def test_ragged_batch_against_the_oracle(gpu_ctx, case):
    _, F, Ts, r, ps = case
    ps = dict(ps, cost_check=1)
    probs = _problems(F, Ts, r)
    _check(_batch(probs, ps, gpu_ctx), _oracle(probs, ps))


# ---- 2. update patterns ---------------------------------------------------------------------------------------------------
P257 = dict(F=257, Ts=(96, 200, 33), r=40)
KL257 = dict(cf="kl", sparsity=5, max_iter=12, cost_check=1)


@functools.lru_cache(maxsize=None)
def _p257():
    return _problems(P257["F"], P257["Ts"], P257["r"])


PATTERNS = {
    "w_only": dict(h_update_ind=np.zeros(40, bool)),
    "h_only": dict(w_update_ind=np.zeros(40, bool)),
    "neither": dict(w_update_ind=np.zeros(40, bool), h_update_ind=np.zeros(40, bool), conv_eps=1e-3),
    "semi_supervised": dict(w_update_ind=np.arange(40) >= 20),
    "rvec_sparsity": dict(sparsity=np.linspace(0.0, 9.0, 40)),
    "rvec_sparsity_column_ed": dict(sparsity=np.linspace(0.0, 2.0, 40).reshape(-1, 1), cf="ed"),
}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_update_patterns_against_the_oracle(gpu_ctx, name):
    ps = dict(KL257, **PATTERNS[name])
    _check(_batch(_p257(), ps, gpu_ctx), _oracle(_p257(), ps))


def test_no_cost_check_records_nothing_and_runs_to_the_end(gpu_ctx):
    ps = dict(KL257, cost_check=0, conv_eps=1e-2)  # (conv_eps is not looked at without the objective, :260-285)
    res = _batch(_p257(), ps, gpu_ctx)
    _check(res, _oracle(_p257(), ps), objective=False)
    for _, _, o in res:
        assert o["n_iter"] == 12 and not o["cost"].any() and not o["div"].any() and o["cost"].shape == (12,)


def test_floor_v_off_through_the_c_entry(gpu_ctx):
    """floor_v = 0 (sparse_nmf_GPU.m: no max(v, 1e-9)) through the resident C entry, on a V with entries below the floor.
    The oracle's gpu_variant leaves the objective vectors zero, so the factors and n_iter are judged."""
    from se_snmf_nat_amd import BatchPlan
    probs = [(np.where(V < 0.02, 1e-12, V), W0, H0) for V, W0, H0 in _p257()]
    ps = dict(cf="kl", sparsity=5, max_iter=12)
    refs = _oracle(probs, ps, gpu_variant=True)
    bp = BatchPlan(gpu_ctx, 257, 40, P257["Ts"], beta=1.0, max_iter=12, sparsity=5, floor_v=False)
    for k, (V, W0, H0) in enumerate(probs):
        bp.set_problem(k, V, W0, H0)
    bp.run()
    res = [bp.get(k) for k in range(3)]
    bp.close()
    _check(res, refs, objective=False)


# ---- 3. different stop indices in one batch -------------------------------------------------------------------------------
def _stop_margin(obj, conv_eps):
    c = obj["cost"]
    e = np.abs(np.diff(c)) / c[:-1]
    return np.min(np.abs(e - conv_eps) / conv_eps)


def _gen_dictionary(F, r, seed):
    return np.random.default_rng(seed).gamma(0.5, 1.0, size=(F, r))  # the dictionary synth_problem(seed_data=seed) drew V from


def _stop_cases():
    kl = dict(cf="kl", sparsity=5, max_iter=80, conv_eps=1e-3, cost_check=1)
    # positions in the list (1, 31, 33, 100, 64, 7); T = 64 (position 4) sits 0.0004 from the threshold and is left out
    kl65 = [synth_problem(65, T, 8, seed_data=10 * b, seed_init=10 * b + 1, r_true=4) for b, T in ((0, 1), (1, 31), (2, 33), (3, 100), (5, 7))]
    # seeds found by a search on the CPU oracle for a stop test at least 0.02 away from its threshold at every iteration
    wonly = [synth_problem(257, T, 40, seed_data=s, seed_init=s + 1, r_true=20) for T, s in ((96, 20), (200, 10), (33, 260))]
    honly = []
    for T, s in ((96, 70), (200, 20), (33, 0)):  # a trained dictionary held fixed: W0 = the one the data were drawn from
        V, _, H0 = synth_problem(257, T, 40, seed_data=s, seed_init=s + 1)
        honly.append((V, _gen_dictionary(257, 40, s), H0))
    return {
        "kl_65": (kl65, kl, [10, 32, 29, 30, 23]),
        "w_only_257": (wonly, dict(kl, h_update_ind=np.zeros(40, bool)), [21, 18, 24]),
        "h_only_257": (honly, dict(kl, conv_eps=1e-2, w_update_ind=np.zeros(40, bool)), [7, 8, 8]),
    }


@functools.lru_cache(maxsize=None)
def _stop_case(name):
    probs, ps, idx = _stop_cases()[name]
    return probs, ps, idx, _oracle(probs, ps)


@pytest.mark.parametrize("name", ["kl_65", "w_only_257", "h_only_257"])
def test_every_problem_stops_at_its_own_iteration(gpu_ctx, name):
    probs, ps, idx, refs = _stop_case(name)
    # the condition on the inputs, on the oracle's side: no stop decision within 2 * REL_COST / conv_eps of its threshold
    for ref, n in zip(refs, idx):
        assert ref[2]["n_iter"] == n
        assert _stop_margin(ref[2], ps["conv_eps"]) >= 0.02
    res = _batch(probs, ps, gpu_ctx)
    assert [o["n_iter"] for _, _, o in res] == idx
    _check(res, refs)
    # a problem that stopped early holds the factors of its own stop iteration: the bits of a batch that ends there
    for b, n in enumerate(idx):
        if n < max(idx):
            short = _batch(probs, dict(ps, max_iter=n), gpu_ctx)
            assert short[b][2]["n_iter"] == n
            _same_bits(short[b], res[b])


# ---- 4. company and slot independence, bit for bit ---------------------------------------------------------------------------
def _resident(probs, ps, ctx, runs=(None,), F=65, r=8):
    from se_snmf_nat_amd import BatchPlan
    bp = BatchPlan(ctx, F, r, [q[0].shape[1] for q in probs], beta=1.0, max_iter=ps["max_iter"], conv_eps=ps["conv_eps"],
                   sparsity=ps["sparsity"])
    assert "k_bh" in bp.describe()
    for k, (V, W0, H0) in enumerate(probs):
        bp.set_problem(k, V, W0, H0)
    for n in runs:
        bp.run(n)
    out = [bp.get(k) for k in range(len(probs))]
    bp.close()
    return out


def test_bits_do_not_depend_on_the_company(gpu_ctx):
    probs, ps, idx, _ = _stop_case("kl_65")
    base = _batch(probs, ps, gpu_ctx)
    assert [o["n_iter"] for _, _, o in base] == idx
    for b in range(len(probs)):  # each problem as a batch of one
        _same_bits(_batch([probs[b]], ps, gpu_ctx)[0], base[b])
    for a, b in zip(_batch(probs[::-1], ps, gpu_ctx)[::-1], base):  # reversed order
        _same_bits(a, b)
    # among 27 others of other sizes; nine of them start from a converged pair of factors and stop at once (iteration 2)
    rs = np.random.RandomState(7)
    others = []
    for i in range(27):
        T = int(rs.randint(1, 300))
        V, W0, H0 = synth_problem(65, T, 8, seed_data=1000 + i, seed_init=2000 + i, r_true=4)
        if i % 3 == 0:
            W0, H0, _ = oracle_nmf(V, dict(ps, init_w=W0, init_h=H0, max_iter=150, conv_eps=0))
        others.append((V, W0, H0))
    slots = [0, 6, 13, 20, 31]
    mixed = list(others)
    for s, q in zip(slots, probs):
        mixed.insert(s, q)
    res = _batch(mixed, ps, gpu_ctx)
    assert sum(res[i][2]["n_iter"] == 2 for i in range(len(mixed)) if i not in slots) >= 9
    for s, b in zip(slots, base):
        _same_bits(res[s], b)
    for a, b in zip(_resident(probs, ps, gpu_ctx), base):  # resident entry against the one-shot entry
        _same_bits(a, b)
    for a, b in zip(_resident(probs, ps, gpu_ctx, runs=(10, 0)), base):  # run(10) + run(0) against one run
        _same_bits(a, b)
    for a, b in zip(_batch(probs, ps, gpu_ctx), base):  # two identical runs
        _same_bits(a, b)
    for a, b in zip(_batch(probs, ps, gpu_ctx, dtype=np.float32), base):  # fp32 host arrays of the same numbers: n_iter and cost
        assert a[2]["n_iter"] == b[2]["n_iter"] and a[0].dtype == np.float32


# ---- 5. fixed-seed fuzz -----------------------------------------------------------------------------------------------------
def _fuzz_case(i):
    rs = np.random.RandomState(4200 + i)
    F, r, B = int(rs.randint(1, 514)), int(rs.randint(1, 201)), int(rs.randint(1, 13))
    if i == 0:
        F, r = 513, 200  # the corner of the envelope
    if i == 1:
        F, r = 1, 1
    Ts = [int(rs.randint(1, 401)) for _ in range(B)]
    beta = [0.0, 0.5, 1.0, 1.5, 2.0][i % 5]
    ps = dict(cf={0.0: "is", 1.0: "kl", 2.0: "ed"}.get(beta, "beta"), beta=beta, sparsity=float(rs.choice([0.0, 0.3, 2.0])), max_iter=6,
              cost_check=1)
    wp, hp = int(rs.randint(0, 3)), int(rs.randint(0, 4))
    if wp == 1:
        ps["w_update_ind"] = rs.rand(r) < 0.5
    elif wp == 2:
        ps["w_update_ind"] = np.zeros(r, bool)
    if hp == 0:
        ps["h_update_ind"] = np.zeros(r, bool)
    probs = [synth_problem(F, T, r, seed_data=100 * i + b, seed_init=100 * i + 50 + b, r_true=max(1, r // 2)) for b, T in enumerate(Ts)]
    return probs, ps


@pytest.mark.parametrize("i", range(20))
def test_fuzz_against_the_oracle(gpu_ctx, i):
    probs, ps = _fuzz_case(i)
    print(f"F={probs[0][0].shape[0]} r={probs[0][1].shape[1]} T={[q[0].shape[1] for q in probs]} "
          f"{ {k: v for k, v in ps.items() if not isinstance(v, np.ndarray)} }")
    _check(_batch(probs, ps, gpu_ctx), _oracle(probs, ps))


# ---- 6. refusals and recovery -----------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu_ctx, lib):
    from se_snmf_nat_amd import BatchPlan, SnmfError
    from se_snmf_nat_amd.api import _make_params
    with pytest.raises(SnmfError, match="513") as e:
        BatchPlan(gpu_ctx, 600, 8, [5, 3])
    assert e.value.status == 8
    with pytest.raises(SnmfError, match="200") as e:
        BatchPlan(gpu_ctx, 64, 300, [5, 3])
    assert e.value.status == 8
    probs = _problems(65, (7, 31), 8)
    # a NULL problem through the one-shot entry
    sp = _make_params(65, 1, 8, 1.0, 5, 0.0, 1, 1, 0, 5.0, None, None)
    T = np.array([7, 31], np.int32)
    ld = np.array([65, 65], np.int64)
    arrs = [[np.asfortranarray(q[i]) for q in probs] for i in range(3)]
    W = [np.empty((65, 8), order="F") for _ in probs]
    H = [np.empty((8, t), order="F") for t in (7, 31)]
    ptrs = lambda xs: (C.c_void_p * 2)(*[None if x is None else x.ctypes.data for x in xs])  # noqa: E731
    ni = np.zeros(2, np.int32)
    args = lambda V: (gpu_ctx._h, C.byref(sp), 2, C.c_void_p(T.ctypes.data), ptrs(V), C.c_void_p(ld.ctypes.data), ptrs(arrs[1]),  # noqa: E731
                      ptrs(arrs[2]), None, ptrs(W), ptrs(H), None, None, C.c_void_p(ni.ctypes.data))
    assert lib.snmf_sparse_nmf_batch_f64(*args([arrs[0][0], None])) == 1
    assert b"NULL" in lib.snmf_last_error()
    # run before every problem is set, get before run
    bp = BatchPlan(gpu_ctx, 65, 8, [7, 31], max_iter=5, sparsity=5)
    bp.set_problem(0, *probs[0])
    with pytest.raises(SnmfError) as e:
        bp.run()
    assert e.value.status == 7
    with pytest.raises(SnmfError) as e:
        bp.get(0)
    assert e.value.status == 7
    # the same handle, and the same context through the one-shot entry, then solve correctly
    bp.set_problem(1, *probs[1])
    bp.run()
    ps = dict(cf="kl", sparsity=5, max_iter=5, cost_check=1)
    refs = _oracle(probs, ps)
    _check([bp.get(0), bp.get(1)], refs)
    bp.close()
    assert lib.snmf_sparse_nmf_batch_f64(*args(arrs[0])) == 0
    assert list(ni) == [5, 5] and rel(W[1], refs[1][0]) < REL_WH and rel(H[0], refs[0][1]) < REL_WH
