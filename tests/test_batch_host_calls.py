"""CPU tests that pin what the batched offline calls hand to the library: which C entry each form reaches, its params struct,
its arrays and their contents, NULL where it is NULL, the host draws (order and number), and which of two violated rules fires
first.  A recording stand-in takes the library's place (the FakeLib / Reached idea of test_dnmf_batch_ranks_api.py, but every
entry returns 0 and the call goes on): it notes (name, args) and, because the host arrays of a call die with it, what a reader
given for that entry decodes from the pointers at the time of the call.  Expected values come from the documented rules
(np.random.RandomState, the docstrings), never from the package's private helpers.

Shapes: F = 6, frame counts (5, 1, 8) -- T = 1 is where the leading-dimension rule can go wrong -- ranks (2, 3, 4) and (3, 3, 3);
the waveforms are the first three of dnmf_audio_batch_cases / train_batch_cases."""
import ctypes as C

import numpy as np
import pytest

import dnmf_audio_batch_cases as ac
import train_batch_cases as tc

F, TS = 6, (5, 1, 8)
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)


# ---------------------------------------------------------------- the recording stand-in
class Rec:
    """The library's stand-in: .lib has every attribute as an entry that appends (name, args, readers[name](args) or None) to
    .calls and returns 0.  An entry with "create" in its name fills the handle its last argument points to."""

    def __init__(self, **readers):
        self.calls, self.readers = [], readers
        rec = self

        class Lib:
            def __getattr__(self, name):
                if name.startswith("__"):
                    raise AttributeError(name)

                def entry(*args):
                    rec.calls.append((name, args, rec.readers[name](args) if name in rec.readers else None))
                    if "create" in name:
                        args[-1]._obj.value = 0xB0
                    return 0
                return entry
        self.lib = Lib()

    def names(self):
        return [c[0] for c in self.calls]

    def only(self):
        assert len(self.calls) == 1, self.names()
        return self.calls[0]


class Ctx:
    """The context's stand-in.  _h is None as a rule; the handle tests give it a value, since a plan destroys its handle only on
    a live context."""

    def __init__(self, h=None):
        self._h, self._plans = h, set()

    def sync(self):
        pass


@pytest.fixture
def rec(monkeypatch):
    from se_snmf_nat_amd import _lib, batch, frontend, train
    r = Rec()
    monkeypatch.setattr(_lib, "load", lambda: r.lib)

    def no_default(*a, **k):
        raise AssertionError("took the default context")
    for mod in (batch, train, frontend):
        monkeypatch.setattr(mod, "default_context", no_default)
    return r


def mat(p, shape, dt=F64):
    """A copy of the column-major array of `shape` and dtype `dt` at the address p."""
    addr = p.value if isinstance(p, C.c_void_p) else p
    n = int(np.prod(shape)) * np.dtype(dt).itemsize
    return np.frombuffer((C.c_char * n).from_address(addr), dtype=dt).reshape(shape, order="F").copy()


def mats(ptrs, shapes, dt=F64):
    return [mat(ptrs[k], s, dt) for k, s in enumerate(shapes)]


def vec(p, n, dt):
    return mat(p, (n,), dt).tolist()


def params(ref):
    """The fields of the snmf_params a byref points to; the masks as lists of r flags."""
    s = ref._obj
    d = {f: getattr(s, f) for f, _ in s._fields_}
    for k in ("w_update_ind", "h_update_ind"):
        d[k] = None if d[k] is None else vec(d[k], s.r, np.uint8)
    return d


def settings_of(arr):
    return [(q.beta, q.sparsity, q.conv_eps, q.max_iter, q.reserved) for q in arr]


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)


def problems(seed=0):
    g = np.random.RandomState(seed)
    return [g.rand(F, T) + 0.1 for T in TS]


def draws(seed, rs, Ts=TS, rows=F, iws=None):
    """w then h per problem, list order, one generator; an init_w narrower than r gets only its missing columns drawn."""
    g = np.random.RandomState(seed) if isinstance(seed, int) else seed
    w0s, h0s = [], []
    for k, (r, T) in enumerate(zip(rs, Ts)):
        iw = None if iws is None else iws[k]
        if iw is None:
            w0s.append(g.random_sample((rows, r)))
        elif iw.shape[1] < r:
            w0s.append(np.concatenate([iw, g.random_sample((rows, r - iw.shape[1]))], axis=1))
        else:
            w0s.append(iw)
        h0s.append(g.random_sample((r, T)))
    return w0s, h0s


def h_draws(seed, rs, Ts):
    g = np.random.RandomState(seed)
    return [g.random_sample((r, T)) for r, T in zip(rs, Ts)]


# ---------------------------------------------------------------- sparse_nmf_batch, sparse_nmf_batch_fp64
def read_solve(rs, dt):
    """snmf_sparse_nmf_batch_*(ctx, params, B, Ts, v, ldv, w0, h0, sparsity, W, H, div, cost, n_iter)."""
    def reader(a):
        B = a[2]
        return dict(params=params(a[1]), B=B, Ts=vec(a[3], B, np.int32), v=mats(a[4], [(F, T) for T in TS], dt),
                    ldv=vec(a[5], B, np.int64), w0=mats(a[6], [(F, r) for r in rs], dt),
                    h0=mats(a[7], [(r, T) for r, T in zip(rs, TS)], dt), sparsity=None if a[8] is None else vec(a[8], rs[0], F64))
    return reader


def test_sparse_nmf_batch_float64_scalar_sparsity(rec):
    from se_snmf_nat_amd import sparse_nmf_batch
    vs = problems()
    rec.readers = {"snmf_sparse_nmf_batch_f64": read_solve([3] * 3, F64)}
    out = sparse_nmf_batch(vs, dict(r=3, cf="kl", sparsity=0.5, max_iter=7, conv_eps=1e-3, cost_check=1, random_seed=5), ctx=Ctx())
    name, a, got = rec.only()
    assert name == "snmf_sparse_nmf_batch_f64" and a[0] is None and len(a) == 14 and len(out) == 3
    assert got["params"] == dict(F=F, T=1, r=3, beta=1.0, max_iter=7, conv_eps=1e-3, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.5, w_update_ind=[1, 1, 1], h_update_ind=[1, 1, 1])
    assert got["B"] == 3 and got["Ts"] == list(TS) and got["ldv"] == [F, F, F] and got["sparsity"] is None
    w0s, h0s = draws(5, [3] * 3)
    same(got["v"], vs), same(got["w0"], w0s), same(got["h0"], h0s)
    assert [o[0].shape for o in out] == [(F, 3)] * 3 and [o[1].shape for o in out] == [(3, T) for T in TS]


def test_sparse_nmf_batch_float32_vector_sparsity_masks_and_a_narrow_init_w(rec):
    from se_snmf_nat_amd import sparse_nmf_batch
    vs = problems()
    iw = np.random.RandomState(3).rand(F, 2)
    rec.readers = {"snmf_sparse_nmf_batch_f32": read_solve([3] * 3, F32)}
    p = dict(r=[3, 3, 3], init_w=iw, cf="ed", sparsity=[0.1, 0.2, 0.3], max_iter=4, cost_check=0, w_update_ind=[0, 0, 1],
             h_update_ind=np.zeros(3))
    sparse_nmf_batch(vs, p, ctx=Ctx(), dtype=np.float32, rng=np.random.RandomState(11))
    name, a, got = rec.only()
    assert name == "snmf_sparse_nmf_batch_f32"
    assert got["params"] == dict(F=F, T=1, r=3, beta=2.0, max_iter=4, conv_eps=0.0, cost_check=0, floor_v=1, sparsity_kind=1,
                                 sparsity_scalar=0.0, w_update_ind=[0, 0, 1], h_update_ind=[0, 0, 0])
    assert got["sparsity"] == [0.1, 0.2, 0.3] and got["ldv"] == [F, F, F]
    w0s, h0s = draws(np.random.RandomState(11), [3] * 3, iws=[iw] * 3)  # only the third column of every w is drawn
    same(got["v"], [v.astype(F32) for v in vs])
    same(got["w0"], [w.astype(F32) for w in w0s]), same(got["h0"], [h.astype(F32) for h in h0s])


@pytest.mark.parametrize("r", [3, [3, 3, 3], (3, 3, 3)])
def test_fp64_solve_with_one_rank_is_the_one_shot_entry(rec, r):
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    vs = problems()
    rec.readers = {"snmf_sparse_nmf_batch_fp64": read_solve([3] * 3, F64)}
    sparse_nmf_batch_fp64(vs, dict(r=r, cf="is", max_iter=2, cost_check=1), ctx=Ctx())
    name, a, got = rec.only()
    assert name == "snmf_sparse_nmf_batch_fp64"
    assert got["params"]["beta"] == 0.0 and got["params"]["r"] == 3 and got["sparsity"] is None
    w0s, h0s = draws(1, [3] * 3)  # random_seed defaults to 1
    same(got["w0"], w0s), same(got["h0"], h0s)


def handle_readers(rs):
    """The handle's entries: create*(ctx, params, B, Ts, [r], [settings], &h), set_problem(h, k, v, ld, w0, h0)."""
    def create(a):
        B = a[2]
        d = dict(params=params(a[1]), B=B, Ts=vec(a[3], B, np.int32))
        if len(a) == 6:  # _ranks
            d["r"] = vec(a[4], B, np.int32)
        if len(a) == 7:  # _settings
            d["r"] = None if a[4] is None else vec(a[4], B, np.int32)
            d["settings"] = settings_of(a[5])
        return d

    def set_problem(a):
        k = a[1]
        return dict(k=k, v=mat(a[2], (F, TS[k])), ld=a[3], w0=mat(a[4], (F, rs[k])), h0=mat(a[5], (rs[k], TS[k])))
    return {"snmf_batch_create_fp64": create, "snmf_batch_create_ranks_fp64": create, "snmf_batch_create_settings_fp64": create,
            "snmf_batch_set_problem_f64": set_problem}


def check_handle_sequence(rec, create, vs, w0s, h0s):
    B = len(vs)
    assert rec.names() == [create] + ["snmf_batch_set_problem_f64"] * B + ["snmf_batch_run"] + ["snmf_batch_get_f64"] * B + ["snmf_batch_destroy"]
    sets = [c[2] for c in rec.calls[1:1 + B]]
    assert [s["k"] for s in sets] == list(range(B)) and [s["ld"] for s in sets] == [F] * B
    same([s["v"] for s in sets], vs), same([s["w0"] for s in sets], w0s), same([s["h0"] for s in sets], h0s)
    assert rec.calls[1 + B][1][1] == 0  # run to the end
    assert [c[1][1] for c in rec.calls[2 + B:2 + 2 * B]] == list(range(B))


def test_fp64_solve_with_differing_ranks_goes_through_the_handle(rec):
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    vs, rs = problems(), [2, 3, 4]
    rec.readers = handle_readers(rs)
    out = sparse_nmf_batch_fp64(vs, dict(r=rs, cf="kl", sparsity=0.25, max_iter=6, conv_eps=1e-5, cost_check=1, random_seed=9,
                                         h_update_ind=np.ones(2)), ctx=Ctx(h=C.c_void_p(1)))
    w0s, h0s = draws(9, rs)
    check_handle_sequence(rec, "snmf_batch_create_ranks_fp64", vs, w0s, h0s)
    got = rec.calls[0][2]
    assert got["r"] == rs and got["Ts"] == list(TS)
    assert got["params"] == dict(F=F, T=1, r=4, beta=1.0, max_iter=6, conv_eps=1e-5, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.25, w_update_ind=[1] * 4, h_update_ind=[1] * 4)
    assert [o[0].shape for o in out] == [(F, r) for r in rs]


@pytest.mark.parametrize("rs", [[3, 3, 3], [2, 3, 4]])
def test_fp64_solve_with_a_list_of_dicts_goes_through_the_settings_handle(rec, rs):
    from se_snmf_nat_amd import sparse_nmf_batch_fp64
    vs = problems()
    iw = np.random.RandomState(4).rand(F, 1)  # narrower than r_0: its other columns are drawn
    ps = [dict(r=rs[0], init_w=iw, cf="kl", sparsity=0.5, max_iter=4, cost_check=1),
          dict(r=rs[1], cf="is", max_iter=9, conv_eps=1e-4, cost_check=1),
          dict(r=rs[2], cf="ed", sparsity=[2.0], max_iter=6, cost_check=1)]
    rec.readers = handle_readers(rs)
    out = sparse_nmf_batch_fp64(vs, ps, ctx=Ctx(h=C.c_void_p(1)))
    w0s, h0s = draws(1, rs, iws=[iw, None, None])
    check_handle_sequence(rec, "snmf_batch_create_settings_fp64", vs, w0s, h0s)
    got = rec.calls[0][2]
    assert got["r"] == (None if len(set(rs)) == 1 else rs)  # NULL for one rank
    assert got["settings"] == [(1.0, 0.5, 0.0, 4, 0), (0.0, 0.0, 1e-4, 9, 0), (2.0, 2.0, 0.0, 6, 0)]
    r = max(rs)
    assert got["params"] == dict(F=F, T=1, r=r, beta=1.0, max_iter=9, conv_eps=0.0, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.5, w_update_ind=[1] * r, h_update_ind=[1] * r)  # max_iter: the largest limit
    assert [len(o[2]["div"]) for o in out] == [0, 0, 0] and [o[0].shape for o in out] == [(F, r) for r in rs]


# ---------------------------------------------------------------- the constructors
PLANS = [("BatchPlan", "snmf_batch_create"), ("BatchPlan64", "snmf_batch_create_fp64"), ("BatchPlanMdi64", "snmf_batch_create_mdi_fp64")]


def plan_readers():
    rd = handle_readers([3] * 3)
    for _, nm in PLANS:
        rd[nm] = rd["snmf_batch_create_fp64"]
    rd["snmf_batch_set_sparsity_f64"] = lambda a: vec(a[1], 3, F64)
    return rd


@pytest.mark.parametrize("cls,create", PLANS)
def test_plan_with_an_int_rank_and_a_vector_sparsity(rec, cls, create):
    import se_snmf_nat_amd as pkg
    rec.readers = plan_readers()
    ctx = Ctx()
    plan = getattr(pkg, cls)(ctx, F, 3, TS, beta=2.0, max_iter=5, conv_eps=1e-2, cost_check=False, sparsity=[0.1, 0.2, 0.3])
    assert rec.names() == [create, "snmf_batch_set_sparsity_f64"] and rec.calls[1][2] == [0.1, 0.2, 0.3]
    a, got = rec.calls[0][1:]
    assert len(a) == 5 and got["B"] == 3 and got["Ts"] == list(TS)
    assert got["params"] == dict(F=F, T=1, r=3, beta=2.0, max_iter=5, conv_eps=1e-2, cost_check=0, floor_v=1, sparsity_kind=1,
                                 sparsity_scalar=0.0, w_update_ind=[1, 1, 1], h_update_ind=[1, 1, 1])
    assert plan in ctx._plans and plan.ranks is None and plan.settings is None
    assert (plan.r, plan.max_iter, plan.rank(2), plan.max_iter_of(1)) == (3, 5, 3, 5)


@pytest.mark.parametrize("cls,create", PLANS)
@pytest.mark.parametrize("kw", [dict(sparsity=[0.1, 0.2, 0.3]), dict(w_update_ind=[1, 0, 1])])
def test_equal_ranks_with_a_vector_or_a_partial_mask_take_the_int_form(rec, cls, create, kw):
    import se_snmf_nat_amd as pkg
    rec.readers = plan_readers()
    plan = getattr(pkg, cls)(Ctx(), F, (3, 3, 3), TS, **kw)
    assert rec.names()[0] == create and plan.ranks is None and plan.r == 3
    assert rec.calls[0][2]["params"]["w_update_ind"] == kw.get("w_update_ind", [1, 1, 1])
    assert rec.calls[0][2]["params"]["sparsity_kind"] == (1 if "sparsity" in kw else 0)


def test_equal_ranks_that_the_ranks_rules_allow(rec):
    """BatchPlan64 takes the ranks entry for a sequence whenever sparsity and masks allow it; the two engines with one rank take
    the int entry."""
    from se_snmf_nat_amd import BatchPlan, BatchPlan64, BatchPlanMdi64
    rec.readers = plan_readers()
    plan = BatchPlan64(Ctx(), F, [3, 3, 3], TS, h_update_ind=False)
    assert rec.names() == ["snmf_batch_create_ranks_fp64"] and plan.ranks == [3, 3, 3] and plan.r == 3
    assert rec.calls[0][2]["r"] == [3, 3, 3] and rec.calls[0][2]["params"]["h_update_ind"] == [0, 0, 0]
    for cls, create in ((BatchPlan, "snmf_batch_create"), (BatchPlanMdi64, "snmf_batch_create_mdi_fp64")):
        rec.calls.clear()
        plan = cls(Ctx(), F, np.array([3, 3, 3]), TS)
        assert rec.names() == [create] and plan.ranks is None and plan.r == 3


@pytest.mark.parametrize("r", [3, [2, 3, 4]])
def test_settings_plan_takes_bool_masks(rec, r):
    from se_snmf_nat_amd import BatchPlan64
    rec.readers = handle_readers([3] * 3)
    plan = BatchPlan64(Ctx(), F, r, TS, beta=0.0, max_iter=3, conv_eps=1e-3, sparsity=0.75, w_update_ind=True, h_update_ind=False,
                       settings=[{}, dict(max_iter=5, cf="ed"), dict(sparsity=1.5, conv_eps=0)])
    name, a, got = rec.only()
    rmax = 3 if r == 3 else 4
    assert name == "snmf_batch_create_settings_fp64" and got["r"] == (None if r == 3 else r)
    assert got["settings"] == [(0.0, 0.75, 1e-3, 3, 0), (2.0, 0.75, 1e-3, 5, 0), (0.0, 1.5, 0.0, 3, 0)]
    assert got["params"] == dict(F=F, T=1, r=rmax, beta=0.0, max_iter=5, conv_eps=1e-3, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.75, w_update_ind=[1] * rmax, h_update_ind=[0] * rmax)
    assert plan.settings == [(0.0, 0.75, 3, 1e-3), (2.0, 0.75, 5, 1e-3), (0.0, 1.5, 3, 0.0)]
    assert (plan.max_iter, plan.max_iter_of(0), plan.max_iter_of(1), plan.r) == (5, 3, 5, rmax)
    assert plan.ranks == (None if r == 3 else r) and plan.rank(0) == (3 if r == 3 else 2)


def test_set_problem_of_a_plan_picks_the_entry_by_the_dtype_of_v(rec):
    from se_snmf_nat_amd import BatchPlan64
    plan = BatchPlan64(Ctx(), F, 3, TS)
    v = problems()[1]
    w0, h0 = np.ones((F, 3)), np.ones((3, 1))
    rec.readers = {"snmf_batch_set_problem_f32": lambda a: (a[1], mat(a[2], (F, 1), F32), a[3], mat(a[4], (F, 3), F32), mat(a[5], (3, 1), F32))}
    plan.set_problem(1, v.astype(F32), w0, h0)
    plan.set_problem(1, v, w0, h0)
    assert rec.names() == ["snmf_batch_create_fp64", "snmf_batch_set_problem_f32", "snmf_batch_set_problem_f64"]
    k, vv, ld, w, h = rec.calls[1][2]
    assert (k, ld) == (1, F) and np.array_equal(vv, v.astype(F32)) and np.array_equal(w, w0) and np.array_equal(h, h0)


# ---------------------------------------------------------------- the missing-data batch
def read_mdi(a):
    """snmf_mdi_batch_fp64(ctx, params, B, Ts, v, ldv, m, ldm, w0, h0, sparsity, v_mdi, NULL, W, H, div, cost, n_iter)."""
    B, shapes = a[2], [(F, T) for T in TS]
    return dict(params=params(a[1]), Ts=vec(a[3], B, np.int32), v=mats(a[4], shapes), ldv=vec(a[5], B, np.int64), m=mats(a[6], shapes),
                ldm=vec(a[7], B, np.int64), w0=mats(a[8], [(F, 3)] * B), h0=mats(a[9], [(3, T) for T in TS]),
                sparsity=None if a[10] is None else vec(a[10], 3, F64))


@pytest.mark.parametrize("soft", [False, True])
def test_mdi_batches_reach_one_entry_and_hand_the_mask_over_as_doubles(rec, soft):
    from se_snmf_nat_amd import snmf_mdi_batch, snmf_mdi_Sm_batch
    vs = problems()
    g = np.random.RandomState(2)
    masks = [g.rand(F, T) for T in TS] if soft else [g.rand(F, T) > 0.3 for T in TS]
    rec.readers = {"snmf_mdi_batch_fp64": read_mdi}
    info = {}
    p = dict(r=3, cf="kl", cost_check=1, max_iter=4, sparsity_mdi=0.5, conv_eps_mdi=1e-3, sparsity=9, conv_eps=1, random_seed=6)
    out = (snmf_mdi_Sm_batch if soft else snmf_mdi_batch)(vs, masks, p, ctx=Ctx(), info=info)
    name, a, got = rec.only()
    assert name == "snmf_mdi_batch_fp64" and len(a) == 18 and a[12] is None and got["sparsity"] is None
    assert got["params"] == dict(F=F, T=1, r=3, beta=1.0, max_iter=4, conv_eps=1e-3, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.5, w_update_ind=[1, 1, 1], h_update_ind=[1, 1, 1])
    assert got["Ts"] == list(TS) and got["ldv"] == [F] * 3 and got["ldm"] == [F] * 3  # (T = 1: the row count)
    same(got["v"], vs)
    same(got["m"], masks if soft else [m.astype(F64) for m in masks])  # hard: 0/1 doubles; soft: unchanged
    w0s, h0s = draws(6, [3] * 3)
    same(got["w0"], w0s), same(got["h0"], h0s)
    assert len(out) == 3 and [w.shape for w in info["w"]] == [(F, 3)] * 3


def test_mdi_plan_set_problem(rec):
    from se_snmf_nat_amd import BatchPlanMdi64
    plan = BatchPlanMdi64(Ctx(), F, 3, TS)
    v = problems()[1]
    m = np.random.RandomState(2).rand(F, 1)
    w0, h0 = np.random.RandomState(3).rand(F, 3), np.random.RandomState(4).rand(3, 1)
    rec.readers = {"snmf_batch_set_problem_mdi_f64": lambda a: (a[1], mat(a[2], (F, 1)), a[3], mat(a[4], (F, 1)), a[5], mat(a[6], (F, 3)),
                                                                mat(a[7], (3, 1)))}
    plan.set_problem(1, v.astype(F32), m, w0, h0)  # (float32 is widened: the missing-data batch has one entry)
    assert rec.names() == ["snmf_batch_create_mdi_fp64", "snmf_batch_set_problem_mdi_f64"]
    k, vv, ldv, mm, ldm, w, h = rec.calls[1][2]
    assert (k, ldv, ldm) == (1, F, F)
    assert np.array_equal(vv, v.astype(F32).astype(F64)) and np.array_equal(mm, m) and np.array_equal(w, w0) and np.array_equal(h, h0)


# ---------------------------------------------------------------- run_basis_dnmf_batch
P_DNMF = dict(cf="kl", sparsity=0.1, max_iter=3, conv_eps=1e-4, cost_check=1, random_seed=7)


def dnmf_problems():
    g = np.random.RandomState(8)
    return tuple([g.rand(F, T) + 0.1 for T in TS] for _ in range(3))


def read_dnmf(rs, dt):
    """snmf_run_basis_dnmf_batch_*(ctx, params, R_x, R_d, n, Ts, Y, X, D, B, H0, B_hat, A_hat, n_iter)."""
    def reader(a):
        n, shapes = a[4], [(F, T) for T in TS]
        return dict(params=params(a[1]), head=a[2:5], Ts=vec(a[5], n, np.int32), Y=mats(a[6], shapes, dt), X=mats(a[7], shapes, dt),
                    D=mats(a[8], shapes, dt), B=mats(a[9], [(F, r) for r in rs], dt), H0=mats(a[10], [(r, T) for r, T in zip(rs, TS)], dt))
    return reader


def read_dnmf_ranks(rs):
    """snmf_run_basis_dnmf_batch_ranks_fp64(ctx, params, R_x[], R_d[], settings, n, Ts, Y, X, D, B, H0, B_hat, A_hat, n_iter)."""
    def reader(a):
        n, shapes = a[5], [(F, T) for T in TS]
        return dict(params=params(a[1]), rx=vec(a[2], n, np.int32), rd=vec(a[3], n, np.int32), settings=None if a[4] is None else settings_of(a[4]),
                    n=n, Ts=vec(a[6], n, np.int32), Y=mats(a[7], shapes), X=mats(a[8], shapes), D=mats(a[9], shapes),
                    B=mats(a[10], [(F, r) for r in rs]), H0=mats(a[11], [(r, T) for r, T in zip(rs, TS)]))
    return reader


@pytest.mark.parametrize("precision,dtype,entry,dt", [("fp32", np.float64, "snmf_run_basis_dnmf_batch_f64", F64),
                                                      ("fp32", np.float32, "snmf_run_basis_dnmf_batch_f32", F32),
                                                      ("fp64", np.float64, "snmf_run_basis_dnmf_batch_fp64", F64)])
@pytest.mark.parametrize("h0", ["host", "list"])
def test_dnmf_batch_uniform_forms(rec, precision, dtype, entry, dt, h0):
    from se_snmf_nat_amd import run_basis_dnmf_batch
    Ys, Xs, Ds = dnmf_problems()
    B = np.random.RandomState(9).rand(F, 5)
    given = h_draws(21, [5] * 3, TS)
    rec.readers = {entry: read_dnmf([5] * 3, dt)}
    info = {}
    out = run_basis_dnmf_batch(Ys, Xs, Ds, B, 2, 3, P_DNMF, ctx=Ctx(), dtype=dtype, precision=precision, info=info,
                               h0="host" if h0 == "host" else given)
    name, a, got = rec.only()
    assert name == entry and len(a) == 14 and got["head"] == (2, 3, 3) and got["Ts"] == list(TS)
    assert got["params"] == dict(F=F, T=1, r=5, beta=1.0, max_iter=3, conv_eps=1e-4, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.1, w_update_ind=None, h_update_ind=None)
    # every array crosses in the call's dtype (read back as that dtype, so another one would not compare equal)
    for key, want in (("Y", Ys), ("X", Xs), ("D", Ds), ("B", [B] * 3), ("H0", h_draws(7, [5] * 3, TS) if h0 == "host" else given)):
        same(got[key], [w.astype(dt) for w in want])
    assert [(b.shape, b.dtype, x.shape, x.dtype) for b, x in out] == [((F, 5), dt, (5, T), dt) for T in TS]
    assert info["n_iter"] == [[0, 0, 0]] * 3


@pytest.mark.parametrize("h0", ["host", "list"])
def test_dnmf_batch_with_a_rank_pair_per_problem(rec, h0):
    from se_snmf_nat_amd import run_basis_dnmf_batch
    Ys, Xs, Ds = dnmf_problems()
    Rx, Rd, rs = [2, 1, 1], (1, 4, 1), [3, 5, 2]
    Bs = [np.random.RandomState(9 + r).rand(F, r) for r in rs]
    given = h_draws(21, rs, TS)
    rec.readers = {"snmf_run_basis_dnmf_batch_ranks_fp64": read_dnmf_ranks(rs)}
    out = run_basis_dnmf_batch(Ys, Xs, Ds, Bs, Rx, Rd, P_DNMF, ctx=Ctx(), precision="fp64", h0="host" if h0 == "host" else given)
    name, a, got = rec.only()
    assert name == "snmf_run_basis_dnmf_batch_ranks_fp64" and len(a) == 15
    assert (got["rx"], got["rd"], got["settings"], got["n"], got["Ts"]) == (Rx, list(Rd), None, 3, list(TS))
    assert got["params"]["r"] == 5 and got["params"]["max_iter"] == 3
    same(got["Y"], Ys), same(got["X"], Xs), same(got["D"], Ds), same(got["B"], Bs)
    same(got["H0"], h_draws(7, rs, TS) if h0 == "host" else given)
    assert [(b.shape, x.shape) for b, x in out] == [((F, r), (r, T)) for r, T in zip(rs, TS)]


def test_dnmf_batch_with_settings_only(rec):
    from se_snmf_nat_amd import run_basis_dnmf_batch
    Ys, Xs, Ds = dnmf_problems()
    B = np.random.RandomState(9).rand(F, 5)
    rec.readers = {"snmf_run_basis_dnmf_batch_ranks_fp64": read_dnmf_ranks([5] * 3)}
    run_basis_dnmf_batch(Ys, Xs, Ds, B, 2, 3, P_DNMF, ctx=Ctx(), precision="fp64", settings=[dict(max_iter=7), {}, dict(cf="ed", sparsity=2)])
    name, a, got = rec.only()
    assert name == "snmf_run_basis_dnmf_batch_ranks_fp64"
    assert (got["rx"], got["rd"], got["n"]) == ([2] * 3, [3] * 3, 3)  # the scalars arrive as arrays
    assert got["settings"] == [(1.0, 0.1, 1e-4, 7, 0), (1.0, 0.1, 1e-4, 3, 0), (2.0, 2.0, 1e-4, 3, 0)]
    assert got["params"] == dict(F=F, T=1, r=5, beta=1.0, max_iter=7, conv_eps=1e-4, cost_check=1, floor_v=1, sparsity_kind=0,
                                 sparsity_scalar=0.1, w_update_ind=None, h_update_ind=None)
    same(got["B"], [B] * 3), same(got["H0"], h_draws(7, [5] * 3, TS))


# ---------------------------------------------------------------- run_basis_DNMF_batch, run_basis_DNMF_Mel_batch
W_TS = ac.TS[:3]


def wave_lists():
    w = ac.waves()[:3]
    return [x for x, _ in w], [d for _, d in w]


def read_audio_dnmf(rows, rs, sdt, ranks):
    """snmf_run_basis_dnmf_audio_batch_*(ctx, params, stft, R_x, R_d, n, x, n_x, d, n_d, mel, M, B, H0, seeds, B_hat, A_hat, n_iter);
    the _ranks_fp64 entry has (R_x[], R_d[], settings) in the place of (R_x, R_d)."""
    def reader(a):
        o = 6 if ranks else 5
        n = a[o]
        n_x, n_d = vec(a[o + 2], n, np.int64), vec(a[o + 4], n, np.int64)
        d = dict(params=params(a[1]), n=n, n_x=n_x, n_d=n_d, x=mats(a[o + 1], [(s,) for s in n_x], sdt), d=mats(a[o + 3], [(s,) for s in n_d], sdt),
                 mel=a[o + 5] is not None, M=a[o + 6], B=mats(a[o + 7], [(rows, r) for r in rs]),
                 H0=None if a[o + 8] is None else mats(a[o + 8], [(r, T) for r, T in zip(rs, W_TS)]),
                 seeds=None if a[o + 9] is None else vec(a[o + 9], n, np.uint64), n_args=len(a))
        if ranks:
            d.update(rx=vec(a[3], n, np.int32), rd=vec(a[4], n, np.int32), settings=None if a[5] is None else settings_of(a[5]))
        else:
            d["head"] = a[3:5]
        return d
    return reader


@pytest.mark.parametrize("mel", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("h0", ["host", "device", "list"])
def test_waveform_dnmf_batch_uniform_forms(rec, mel, precision, h0):
    from se_snmf_nat_amd import train
    fn = train.run_basis_DNMF_Mel_batch if mel else train.run_basis_DNMF_batch
    rows, r = (ac.TINY["F_order"] if mel else ac.F), ac.R_X + ac.R_D
    xs, ds = wave_lists()
    sdt = F64 if precision == "fp64" else F32
    entry = "snmf_run_basis_dnmf_audio_batch_" + ("fp64" if precision == "fp64" else "f64")
    Bs = list(ac.bases(rows)[:3])
    given = list(ac.given_h0()[:3])
    rec.readers = {entry: read_audio_dnmf(rows, [r] * 3, sdt, False)}
    info = {}
    out = fn(xs, ds, Bs, ac.P_STOP, ctx=Ctx(), precision=precision, info=info, h0=given if h0 == "list" else h0)
    name, a, got = rec.only()
    assert name == entry and got["n_args"] == 18 and got["head"] == (ac.R_X, ac.R_D) and got["n"] == 3
    assert got["n_x"] == [x.size for x in xs] and got["n_d"] == [d.size for d in ds]
    same(got["x"], [x.astype(sdt) for x in xs]), same(got["d"], [d.astype(sdt) for d in ds]), same(got["B"], Bs)
    assert (got["mel"], got["M"]) == ((True, ac.TINY["F_order"]) if mel else (False, 0))
    pr = got["params"]
    assert (pr["F"], pr["T"], pr["r"], pr["beta"], pr["max_iter"], pr["conv_eps"], pr["sparsity_scalar"]) == (rows, 1, r, 1.0, 20, 1.5e-3, 5.0)
    if h0 == "device":
        assert got["H0"] is None and got["seeds"] == [1, 2, 3]  # random_seed + k
    else:
        assert got["seeds"] is None
        same(got["H0"], h_draws(1, [r] * 3, W_TS) if h0 == "host" else given)
    assert info["T"] == W_TS and [(b.shape, x.shape) for b, x in out] == [((rows, r), (r, T)) for T in W_TS]


@pytest.mark.parametrize("mel", [False, True])
@pytest.mark.parametrize("h0", ["host", "device", "list"])
@pytest.mark.parametrize("form", ["pairs", "settings"])
def test_waveform_dnmf_batch_with_ranks_or_settings(rec, mel, h0, form):
    from se_snmf_nat_amd import train
    fn = train.run_basis_DNMF_Mel_batch if mel else train.run_basis_DNMF_batch
    rows = ac.TINY["F_order"] if mel else ac.F
    xs, ds = wave_lists()
    Rx, Rd = ([5, 3, 2], [7, 1, 2]) if form == "pairs" else (ac.R_X, ac.R_D)
    rs = [12, 4, 4] if form == "pairs" else [12] * 3
    settings = None if form == "pairs" else [{}, dict(max_iter=25, cf="is"), dict(conv_eps=0)]
    Bs = [np.random.RandomState(30 + k).rand(rows, r) + 0.05 for k, r in enumerate(rs)]
    given = h_draws(21, rs, W_TS)
    rec.readers = {"snmf_run_basis_dnmf_audio_batch_ranks_fp64": read_audio_dnmf(rows, rs, F64, True)}
    fn(xs, ds, Bs, dict(ac.P_STOP, R_x=Rx, R_d=Rd, random_seed=4), ctx=Ctx(), precision="fp64", settings=settings,
       h0=given if h0 == "list" else h0)
    name, a, got = rec.only()
    assert name == "snmf_run_basis_dnmf_audio_batch_ranks_fp64" and got["n_args"] == 19 and got["n"] == 3
    assert got["rx"] == (Rx if form == "pairs" else [ac.R_X] * 3) and got["rd"] == (Rd if form == "pairs" else [ac.R_D] * 3)
    if form == "pairs":
        assert got["settings"] is None and got["params"]["max_iter"] == 20
    else:
        assert got["settings"] == [(1.0, 5.0, 1.5e-3, 20, 0), (0.0, 5.0, 1.5e-3, 25, 0), (1.0, 5.0, 0.0, 20, 0)] and got["params"]["max_iter"] == 25
    assert got["params"]["r"] == 12 and got["params"]["F"] == rows
    same(got["x"], [np.asarray(x, F64) for x in xs]), same(got["B"], Bs)
    if h0 == "device":
        assert got["H0"] is None and got["seeds"] == [4, 5, 6]
    else:
        assert got["seeds"] is None
        same(got["H0"], h_draws(4, rs, W_TS) if h0 == "host" else given)


# ---------------------------------------------------------------- the batched training calls
S_TS = tc.TS[:3]
TRAIN_FORMS = {  # form -> (precision, R, settings, the entry's suffix, n_atoms as handed over)
    "fp32": ("fp32", 6, None, "f64", "absent"),
    "fp64": ("fp64", [6, 6, 6], None, "fp64", "absent"),
    "ranks": ("fp64", [6, 5, 4], None, "ranks_fp64", [6, 5, 4]),
    "settings": ("fp64", 6, [dict(max_iter=30), {}, dict(cf="ed", sparsity=1)], "settings_fp64", None),
    "settings+ranks": ("fp64", (6, 5, 4), [dict(max_iter=30), {}, dict(cf="ed", sparsity=1)], "settings_fp64", [6, 5, 4]),
}


def train_call(source, R, p, **kw):
    """The call of `source` on the first three training signals -> what it returns."""
    from se_snmf_nat_amd import train
    sigs = list(tc.signals()[:3])
    if source == "audio":
        return train.run_basis_train_signal_batch(sigs, R, p, ctx=Ctx(), **kw)

    class Signals(train.TrainSignals):  # (a stand-in: nothing on a device to give back)
        def close(self):
            self._h = None
    return train.run_basis_train_assembled_batch(Signals("the handle", Ctx(), [s.size for s in sigs], [1] * 3), R, p, **kw)


def read_train(source, sdt, n_exs, atoms, with_settings, exemplar=False):
    """snmf_run_basis_train_audio_batch_*(ctx, params, stft, alpha, mel, M, n, signals, lengths, [n_atoms], idx, exemplar, H0,
    seeds, B_DFT, A_DFT, B_Mel, A_Mel, n_iter, [settings]); the _signals_ entries have the resident handle for (n, signals, lengths)."""
    def reader(a):
        d = dict(params=params(a[1]), alpha=a[3], mel=mat(a[4], (tc.F_MEL, tc.N // 2 + 1), sdt).shape, M=a[5], n_args=len(a))
        if source == "audio":
            d.update(n=a[6], lens=vec(a[8], 3, np.int64))
            d["signals"] = mats(a[7], [(s,) for s in d["lens"]], sdt)
            o = 9
        else:
            d["handle"] = a[6]
            o = 7
        if atoms:
            d["atoms"] = None if a[o] is None else vec(a[o], 3, np.int32)
            o += 1
        d.update(idx=mats(a[o], [(n,) for n in n_exs], np.int64), exemplar=a[o + 1],
                 H0=None if a[o + 2] is None else mats(a[o + 2], [(n, T) for n, T in zip(n_exs, S_TS)]),
                 seeds=None if a[o + 3] is None else vec(a[o + 3], 3, np.uint64), A=(a[o + 5] is not None, a[o + 7] is not None))
        assert a[o + 4] is not None and a[o + 6] is not None and a[o + 8] is not None
        if with_settings:
            d["settings"] = settings_of(a[o + 9])
        assert len(a) == o + 9 + (1 if with_settings else 0)
        return d
    return reader


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (the host epilogue runs on output arrays nothing has filled)
@pytest.mark.parametrize("source", ["audio", "signals"])
@pytest.mark.parametrize("form", list(TRAIN_FORMS))
@pytest.mark.parametrize("h0", ["host", "device"])
def test_batched_training_forms(rec, source, form, h0):
    precision, R, settings, suffix, atoms = TRAIN_FORMS[form]
    entry = f"snmf_run_basis_train_{source}_batch_{suffix}"
    sdt = F64 if precision == "fp64" else F32
    n_exs = atoms if isinstance(atoms, list) else [6, 6, 6]
    rec.readers = {entry: read_train(source, sdt, n_exs, atoms != "absent", settings is not None)}
    info = {}
    out = train_call(source, R, dict(tc.P_STOP, random_seed=3), h0=h0, precision=precision, settings=settings, info=info)
    name, a, got = rec.only()
    assert name == entry and got["M"] == tc.F_MEL and got["alpha"] == -1.0 and got["exemplar"] == 0 and got["A"] == (True, True)
    sigs = tc.signals()[:3]
    if source == "audio":
        assert got["n"] == 3 and got["lens"] == [s.size for s in sigs]
        same(got["signals"], [s.astype(sdt) for s in sigs])
    else:
        assert got["handle"] == "the handle"
    if atoms != "absent":
        assert got["atoms"] == atoms  # NULL for one dictionary size
    same(got["idx"], [np.random.RandomState(1).choice(T, size=n, replace=False) for T, n in zip(S_TS, n_exs)])  # 0-based
    if h0 == "host":  # every problem: the single call's own draw, the same seed
        assert got["seeds"] is None
        same(got["H0"], [np.random.RandomState(3).random_sample((n, T)) for n, T in zip(n_exs, S_TS)])
    else:
        assert got["H0"] is None and got["seeds"] == [3, 3, 3]
    pr = got["params"]
    assert (pr["F"], pr["T"], pr["r"], pr["beta"], pr["conv_eps"], pr["cost_check"], pr["sparsity_scalar"]) == (tc.F, 1, 6, 1.0, 5e-4, 1, 5.0)
    assert pr["max_iter"] == (30 if settings else 20)  # the largest limit
    if settings:
        assert got["settings"] == [(1.0, 5.0, 5e-4, 30, 0), (1.0, 5.0, 5e-4, 20, 0), (2.0, 1.0, 5e-4, 20, 0)]
    assert info["T"] == S_TS and [o["A_DFT_sub"].shape for o in out] == [(n, T) for n, T in zip(n_exs, S_TS)]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("source", ["audio", "signals"])
def test_batched_training_in_exemplar_mode_ignores_the_settings(rec, source):
    entry = f"snmf_run_basis_train_{source}_batch_fp64"
    rec.readers = {entry: read_train(source, F64, [6] * 3, False, False)}
    out = train_call(source, 6, dict(tc.P_STOP, train_Exemplar=1), precision="fp64", settings=[dict(max_iter=30), {}, {}])
    name, a, got = rec.only()
    assert name == entry and got["exemplar"] == 1 and got["H0"] is None and got["seeds"] is None and got["A"] == (False, False)
    pr = got["params"]
    assert (pr["beta"], pr["max_iter"], pr["conv_eps"], pr["cost_check"], pr["sparsity_scalar"], pr["r"]) == (1.0, 1, 0.0, 0, 0.0, 6)
    assert [o["A_DFT_sub"] for o in out] == [0, 0, 0]


# ---------------------------------------------------------------- which of two violated rules fires first
VS, OK = problems(), dict(cf="kl", cost_check=1, max_iter=3)
ONES = [np.ones_like(v) for v in VS]
W2 = np.ones((F, 2))
YS, XS_, DS_ = dnmf_problems()
B5 = np.ones((F, 5))
XS, DS = wave_lists()
BW = np.ones((ac.F, ac.R_X + ac.R_D))
SIGS = list(tc.signals()[:3])
BAD_MASKS = [np.ones((F, 4)), np.ones((F, 1)), np.ones((F, 8))]


def signals_stand_in(train):
    class Signals(train.TrainSignals):  # (a stand-in: nothing on a device to give back)
        def close(self):
            self._h = None
    return Signals("the handle", Ctx(), [s.size for s in SIGS], [1] * 3)


# Doubly wrong inputs: (the call, what the parent commit gives).  Every expected status (or exception) was read off the parent
# commit of the pull request that added this test, two or more rows per public name.
PRECEDENCE = [
    # sparse_nmf_batch
    (lambda pkg, train: pkg.sparse_nmf_batch(VS, dict(r=[2, 3])), 3),                                  # a short rank list; no cost_check (4)
    (lambda pkg, train: pkg.sparse_nmf_batch(VS, dict(OK, r=[2, 3, 4], sparsity=np.ones((2, 2)))), 3),  # differing ranks; a matrix sparsity (8)
    (lambda pkg, train: pkg.sparse_nmf_batch(VS, [OK] * 3, precision="fp64"), ValueError),             # precision; settings per problem (8)
    (lambda pkg, train: pkg.sparse_nmf_batch(VS + [np.ones((F + 1, 2))], dict(OK, r=2), dtype=np.int32), 1),  # dtype; a row count (3)
    # sparse_nmf_batch_fp64
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, dict(r=[2, 3, 4], sparsity=np.ones(4))), 8),     # a vector across ranks; no cost_check (4)
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS[:2] + [np.ones(F)], [dict(OK, r=2)] * 2), 3),     # two dicts for three; a 1-D v (1)
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, [OK, dict(OK, r=2, sparsity=[1, 2]), dict(OK, r=2)]), 2),  # no rank in problem 0; a vector in 1 (8)
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, [dict(OK, r=0), dict(OK, r=2, max_iter=-1), dict(OK, r=2)]), 1),  # (both are status 1)
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, [dict(cf="kl", r=2, w_update_ind=[1, 0])] + [dict(OK, r=2)] * 2), 4),  # no cost_check; masks differ (3)
    # the plans
    (lambda pkg, train: pkg.BatchPlan(None, F, 3, [], settings=[{}]), 1),                              # no problem; settings in fp32 (8)
    (lambda pkg, train: pkg.BatchPlan(None, F, [2, 3, 4], TS, settings=[{}] * 3), 8),                  # settings in fp32; differing ranks (3)
    (lambda pkg, train: pkg.BatchPlan(None, F, 3, TS, precision="fp64", settings=[{}]), ValueError),
    (lambda pkg, train: pkg.BatchPlan64(None, F, [2, 0, 4], TS, settings=[{}]), 3),                    # one dict for three; a rank of 0 (1)
    (lambda pkg, train: pkg.BatchPlan64(None, F, [2, 3], TS, sparsity=np.ones(4)), 3),                 # a short rank list; a vector across ranks (8)
    (lambda pkg, train: pkg.BatchPlan64(None, F, 3, TS, w_update_ind=[1, 0], sparsity=np.ones((3, 2))), 3),  # a short mask; a matrix sparsity (8)
    (lambda pkg, train: pkg.BatchPlanMdi64(None, F, [2, 3, 4], TS, settings=[{}] * 3), 8),
    # the missing-data batches
    (lambda pkg, train: pkg.snmf_mdi_batch(VS, [np.ones((F, 5))] * 2, dict(r=3)), 3),                  # two masks for three; no cost_check (KeyError)
    (lambda pkg, train: pkg.snmf_mdi_batch(VS[:2] + [np.ones(F)], BAD_MASKS[:2] + [np.ones(F)], dict(OK, r=3)), 3),  # the mask of problem 0; a 1-D v after it (1)
    (lambda pkg, train: pkg.snmf_mdi_Sm_batch(VS, [np.ones_like(v) for v in VS], dict(cf="kl")), KeyError),  # no cost_check; neither r nor init_w (2)
    (lambda pkg, train: pkg.snmf_mdi_batch(VS, [np.ones_like(v) for v in VS], dict(OK, r=[2, 3, 4], sparsity_mdi=np.ones((2, 2)))), 3),
    # run_basis_dnmf_batch
    (lambda pkg, train: pkg.run_basis_dnmf_batch(YS, XS_, DS_, np.ones((F, 4)), 2, 3, dict(cf="kl")), 3),  # B's shape; no cost_check (4)
    (lambda pkg, train: pkg.run_basis_dnmf_batch(YS, XS_, DS_, B5, [2, 2], 3, P_DNMF, settings=[{}]), 8),  # lists in fp32; a short list (3)
    (lambda pkg, train: pkg.run_basis_dnmf_batch(YS, XS_, DS_, B5, 2, 3, P_DNMF, precision="fp64", settings=[{}], dtype=np.float32), 3),  # settings; dtype (1)
    (lambda pkg, train: pkg.run_basis_dnmf_batch(YS, XS_, DS_, B5, 2, 3, dict(P_DNMF, sparsity=[1, 2]), h0="device"), 3),
    (lambda pkg, train: pkg.run_basis_dnmf_batch(YS, XS_[:2], DS_, B5, [2, 0, 2], 3, P_DNMF, precision="fp64"), 1),  # (both are status 1)
    (lambda pkg, train: pkg.run_basis_dnmf_batch(YS, XS_, DS_, B5, 2, 3, dict(cf="kl"), precision="fp64", dtype=np.float32), 4),  # no cost_check; dtype (1)
    # run_basis_DNMF_batch, run_basis_DNMF_Mel_batch
    (lambda pkg, train: train.run_basis_DNMF_batch(XS, DS, BW, ac.P_STOP, settings=[{}]), 8),          # settings in fp32; one dict for three (3)
    (lambda pkg, train: train.run_basis_DNMF_batch(XS, DS, BW, dict(ac.TINY, cf="kl"), h0="gpu"), 3),  # h0; no cost_check (4)
    (lambda pkg, train: train.run_basis_DNMF_Mel_batch(XS, DS, BW, dict(ac.TINY, cf="kl"), precision="fp64", dtype=np.float32), 3),  # B's rows; the rest
    (lambda pkg, train: train.run_basis_DNMF_batch(XS, DS, BW, dict(ac.TINY, cf="kl"), precision="fp64", dtype=np.float32), 4),  # no cost_check; dtype (1)
    (lambda pkg, train: train.run_basis_DNMF_batch(XS, DS[:2], BW, dict(ac.P_STOP, R_x=[5, 5])), 1),   # two noise waveforms; lists in fp32 (8)
    # the batched training calls
    (lambda pkg, train: train.run_basis_train_signal_batch(SIGS, 6, tc.P_STOP, settings=[{}]), 8),     # settings in fp32; one dict for three (3)
    (lambda pkg, train: train.run_basis_train_signal_batch(SIGS, [6, 0, 6], tc.P_STOP, h0="gpu"), 3),  # h0; a size of 0 (1)
    (lambda pkg, train: train.run_basis_train_signal_batch(SIGS, [6, 5], tc.P_STOP, settings=[{}], precision="fp64"), 3),  # (both are status 3)
    (lambda pkg, train: train.run_basis_train_signal_batch(SIGS, [6, 5, 4], dict(tc.P_STOP, cluster_buff=2, train_Exemplar=1)), 3),  # exemplars; fp32 ranks (8)
    (lambda pkg, train: train.run_basis_train_signal_batch(SIGS, [6, 5, 7], tc.P_STOP, precision="fp64", settings=[dict(tol=1)] * 3), 1),  # a key; 7 > T_0 (3)
    (lambda pkg, train: train.run_basis_train_assembled_batch(None, [6, 0, 6], tc.P_STOP), 1),          # no TrainSignals; (both are status 1)
    (lambda pkg, train: train.run_basis_train_clips_batch([[SIGS[0]]] * 3, [6, 5, 4], tc.P_STOP, h0="gpu"), 3),  # h0; fp32 ranks (8)
    (lambda pkg, train: train.run_basis_train_clips_batch([[SIGS[0]]] * 3, [6, 5, 4], dict(tc.P_STOP, cost_check=None, sparsity=[1, 2])), 3),  # sparsity; ranks (8)
    (lambda pkg, train: train.run_basis_train_clips_batch([[SIGS[0]]] * 3, 6, {k: v for k, v in tc.P_STOP.items() if k != "cost_check"}, settings=[{}]), 4),
    # a None entry in the list forms of init_w / init_h is no matrix (only an absent key means "none given")
    (lambda pkg, train: pkg.sparse_nmf_batch(VS, dict(r=3, init_w=[None, W2, W2])), 3),           # the entry; no cost_check (4)
    (lambda pkg, train: pkg.sparse_nmf_batch(VS, dict(r=3, init_w=[W2, W2, None])), 3),
    (lambda pkg, train: pkg.sparse_nmf_batch(VS, dict(r=2, init_h=[None] * 3)), 3),
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, dict(r=3, init_w=[None, W2, W2])), 3),
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, dict(r=[2, 3, 4], init_w=[None] * 3)), 3),
    (lambda pkg, train: pkg.sparse_nmf_batch_fp64(VS, dict(r=2, init_h=[None, np.ones((2, 1)), np.ones((2, 8))])), 3),
    (lambda pkg, train: pkg.snmf_mdi_batch(VS, ONES, dict(r=2, init_w=[W2, None, W2])), KeyError),  # no cost_check comes first there
    (lambda pkg, train: pkg.snmf_mdi_batch(VS, ONES, dict(OK, r=2, init_h=[None] * 3, sparsity_mdi=np.ones((2, 2)))), 3),  # a matrix sparsity (8)
    # a second row for the names that share a body with a sibling above
    (lambda pkg, train: pkg.snmf_mdi_Sm_batch(VS, ONES[:2], dict(OK, r=[2, 3, 4])), 3),           # two masks for three; differing ranks (3)
    (lambda pkg, train: pkg.snmf_mdi_Sm_batch(VS, ONES, dict(OK, r=3, h_update_ind=[1, 0, 1], sparsity_mdi=np.ones((3, 2)))), 3),  # mask; matrix (8)
    (lambda pkg, train: pkg.BatchPlanMdi64(None, F, [2, 3, 4], TS, sparsity=np.ones((2, 2))), 8),  # differing ranks (8 here); a matrix (8)
    (lambda pkg, train: pkg.BatchPlanMdi64(None, F, [3, 3], TS, h_update_ind=[1, 0, 1]), 3),        # a short rank list; a partial mask (3)
    (lambda pkg, train: pkg.BatchPlanMdi64(None, F, 3, [], sparsity=np.ones((3, 2))), 1),           # no problem; a matrix sparsity (8)
    (lambda pkg, train: train.run_basis_DNMF_Mel_batch(XS, DS, BW, ac.P_STOP, settings=[{}]), 8),  # settings in fp32; B's rows (3)
    (lambda pkg, train: train.run_basis_DNMF_Mel_batch(XS, DS, np.ones((8, 12)), dict(ac.TINY, cf="kl"), h0=[np.ones((12, 1))]), 3),  # h0; cost_check (4)
    (lambda pkg, train: train.run_basis_train_assembled_batch("ts", 6, tc.P_STOP, precision="bf16"), 1),  # no TrainSignals; precision (ValueError)
    (lambda pkg, train: train.run_basis_train_assembled_batch(signals_stand_in(train), [6, 5, 4], tc.P_STOP, h0="gpu"), 3),  # h0; fp32 ranks (8)
    (lambda pkg, train: train.run_basis_train_assembled_batch(signals_stand_in(train), 6, tc.P_STOP, settings=[{}], sample_idx=[[1]]), 8),  # settings; idx (3)
]


@pytest.mark.parametrize("row", range(len(PRECEDENCE)))
def test_error_precedence(monkeypatch, row):
    """Which of two violated rules fires first, and that it does before the library is loaded."""
    import se_snmf_nat_amd as pkg
    from se_snmf_nat_amd import _lib, batch, frontend, train

    def refuse(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_lib, "load", refuse)
    for mod in (batch, train, frontend):
        monkeypatch.setattr(mod, "default_context", refuse)
    call, want = PRECEDENCE[row]
    if isinstance(want, int):
        with pytest.raises(_lib.SnmfError) as e:
            call(pkg, train)
        assert e.value.status == want, (e.value.status, want)
    else:
        with pytest.raises(want):
            call(pkg, train)
