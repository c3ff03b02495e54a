"""The C ABI's matrix boundary, bit for bit (include/snmf.h: every `int64_t ld*` parameter that tests/boundary.py maps to this
file): leading dimensions above the row count, both host types, host and device residency, and the chunked host transfer
pipeline of csrc/snmf_tu_xfer.hip with one to five chunks.

Every buffer holds exactly (cols - 1) * ld + rows elements and a guard band behind them.  Input padding and guards are NaN
(a read of padding poisons a result), output padding and guards a negative sentinel (compared as integers).  Every assertion
on data is equality of bits or of status codes: there is no tolerance in this file.

  A  set -> get round trips through a plan: types x residencies x leading dimensions, three shapes
  B  the pipeline: 1, 2, 3, 4, 5 chunks, contiguous and per-column host copies, overwrite after return, back-to-back calls,
     the fp64-staged path, two host threads
  C  every computing entry: NaN-padded strided arguments give the bits of tight ones
  D  (inside C's driver and A) ld = rows - 1 is SNMF_ERR_INVALID and writes nothing, ld = rows is accepted, and the same
     handle then gives the same bits; a leading dimension of rows + 2^20
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import boundary as bd
from boundary import INVALID, OK, same_bits, strided, strided_out
from oracle.sparse_nmf_oracle import synth_problem

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NP = {"f32": F32, "f64": F64, "fp64": F64}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def vp(x):
    if x is None:
        return None
    return C.c_void_p(x.ptr if isinstance(x, bd.Strided) else x.ctypes.data)


def ptrs(xs):
    return (C.c_void_p * len(xs))(*[None if x is None else (x.ptr if isinstance(x, bd.Strided) else x.ctypes.data) for x in xs])


def col(a, dt):
    return np.asfortranarray(np.asarray(a), dtype=dt)


def inp(a, ld, dt=None):
    """A NaN-padded input with leading dimension ld."""
    a = np.asarray(a)
    return strided(col(a, a.dtype if dt is None else dt), ld)


def inout(a, dt):
    """A tight array the entry reads and overwrites: sentinel guard, `initial` = what a refused call must leave."""
    s = bd.Strided(a.shape[0], a.shape[1], a.shape[0], dt, bd.sentinel(dt), col(a, dt))
    s.initial = s.values()
    return s


def unwritten(s):
    if getattr(s, "initial", None) is None:
        return s.untouched()
    return same_bits(s.values(), s.initial) and s.intact()


def params(F, T, r, *, max_iter=3, w_ind=None, h_ind=None, sparsity=5.0, floor_v=True):
    from se_snmf_nat_amd.api import _make_params
    return _make_params(F, T, r, 1.0, max_iter, 0.0, 1, floor_v, 0, sparsity, w_ind, h_ind)


def err(lib):
    return lib.snmf_last_error()


def outs_same(got, ref, what=""):
    assert sorted(got) == sorted(ref)
    for n in got:
        g, w = got[n], ref[n]
        assert g.intact(), (what, n, "padding or guard band written")
        v = g.values()
        assert not np.isnan(v).any(), (what, n, "NaN in an output: padding was read")
        assert same_bits(v, w.values()), (what, n, "first difference (row, column)", bd.first_difference(v, w.values()))


def check_entry(lib, call, rows, extra=()):
    """call(ld, layout) -> (status, {name: Strided output}) passes ld[name] for every leading dimension and lays the buffers out
    with layout[name].  Sections C and D for one entry: strided == tight, padding and guards intact, no NaN; then for every
    leading dimension rows - 1 is refused with nothing written, and the valid call still gives the same bits."""
    tight = dict(rows)
    rc, ref = call(tight, tight)  # ld = rows exactly is accepted
    assert rc == OK, err(lib)
    for o in ref.values():
        assert o.intact() and not np.isnan(o.values()).any()
    lds = {n: rows[n] + 1 + 2 * i for i, n in enumerate(rows)}  # a different padding for every argument
    assert len(set(v - rows[n] for n, v in lds.items())) == len(rows)
    rc, got = call(lds, lds)
    assert rc == OK, err(lib)
    outs_same(got, ref, "strided")
    for lay in extra:
        rc, g = call(lay, lay)
        assert rc == OK, (lay, err(lib))
        outs_same(g, ref, lay)
    for n in rows:
        bad = dict(lds)
        bad[n] = rows[n] - 1
        rc, out = call(bad, lds)
        assert rc == INVALID, (n, rc, err(lib))
        for k, o in out.items():
            assert unwritten(o), (n, k, "a refused call wrote an output")
        rc, again = call(lds, lds)
        assert rc == OK, (n, err(lib))
        outs_same(again, got, f"after refusing {n}")


# =============================================================================================================================
# A. round trips through a plan
# =============================================================================================================================
def _round_trip(lib, ctx, pl, name, a64, dev_type, in_ty, out_ty, in_dev, out_dev, ld_in, ld_out):
    a = col(a64, NP[in_ty])
    src = strided(a, ld_in)
    dst = strided_out(a.shape[0], a.shape[1], ld_out, NP[out_ty])
    if in_dev:
        src.to_device()
    if out_dev:
        dst.to_device()
    what = (name, a.shape, in_ty, out_ty, "dev" if in_dev else "host", "dev" if out_dev else "host", ld_in, ld_out)
    assert getattr(lib, f"snmf_plan_set_{name}_{in_ty}")(pl._h, vp(src), ld_in, int(in_dev)) == OK, (what, err(lib))
    assert getattr(lib, f"snmf_plan_get_{name}_{out_ty}")(pl._h, vp(dst), ld_out, int(out_dev)) == OK, (what, err(lib))
    ctx.sync()
    dst.fetch()  # (a synchronising copy for a device output)
    want = bd.expect(a, NP[in_ty], dev_type, NP[out_ty])
    assert dst.intact(), (what, "padding or guard band written")
    assert same_bits(dst.values(), want), (what, bd.first_difference(dst.values(), want))
    if in_dev:
        before = src.buf.copy()
        assert same_bits(src.fetch().buf, before), (what, "the device input was written")


@pytest.mark.parametrize("name", ["w", "h"])
@pytest.mark.parametrize("shape", bd.ROUND_TRIP_SHAPES, ids=lambda s: "F%d-r%d-T%d" % s)
def test_a_round_trip_types_residency_and_leading_dimensions(gpu_ctx, lib, shape, name):
    """snmf_plan_set_w -> get_w (the fp64 master Wc) and set_h -> get_h (fp32; get_h before init reads the buffer set_h
    wrote): the full cross of host types, residencies and leading dimensions; then the refusals on the same plan."""
    from se_snmf_nat_amd import Plan
    F, r, T = shape
    rows, cols, dev_type = (F, r, F64) if name == "w" else (r, T, F32)
    a64 = bd.round_trip_values(rows, cols, 100 + F)
    pl = Plan(gpu_ctx, F, T, r, max_iter=1)
    try:
        n = 0
        for in_ty in ("f32", "f64"):
            for out_ty in ("f32", "f64"):
                for in_dev in (False, True):
                    for out_dev in (False, True):
                        for ld_in in bd.ld_steps(rows):
                            for ld_out in bd.ld_steps(rows):
                                _round_trip(lib, gpu_ctx, pl, name, a64, dev_type, in_ty, out_ty, in_dev, out_dev, ld_in, ld_out)
                                n += 1
        assert n == 144
        # D: rows - 1 is refused on either side, host and device, and nothing is written; the plan then works as before
        for ty in ("f32", "f64"):
            for dev in (False, True):
                src = strided(col(a64, NP[ty]), rows + 1)
                dst = strided_out(rows, cols, rows + 1, NP[ty])
                if dev:
                    src.to_device(), dst.to_device()
                assert getattr(lib, f"snmf_plan_set_{name}_{ty}")(pl._h, vp(src), rows - 1, int(dev)) == INVALID
                assert b"leading dimension" in err(lib)
                assert getattr(lib, f"snmf_plan_get_{name}_{ty}")(pl._h, vp(dst), rows - 1, int(dev)) == INVALID
                gpu_ctx.sync()
                assert dst.fetch().untouched()
                _round_trip(lib, gpu_ctx, pl, name, a64, dev_type, ty, ty, dev, dev, rows + 1, rows + 1)
    finally:
        pl.close()


def test_d_a_huge_leading_dimension_on_three_columns(gpu_ctx, lib):
    """ld = rows + 2^20 on a 3-column matrix: the buffer holds 2 * ld + rows elements and not one more that may be touched."""
    from se_snmf_nat_amd import Plan
    F, r, T = 65, 3, 3
    pl = Plan(gpu_ctx, F, T, r, max_iter=1)
    try:
        for name, rows, cols, dev_type in (("w", F, r, F64), ("h", r, T, F32)):
            a64 = bd.round_trip_values(rows, cols, 9)
            ld = rows + 2 ** 20
            assert strided(a64, ld).n == 2 * ld + rows
            for in_dev, out_dev in ((False, False), (True, True), (False, True), (True, False)):
                _round_trip(lib, gpu_ctx, pl, name, a64, dev_type, "f64", "f32", in_dev, out_dev, ld, ld)
                _round_trip(lib, gpu_ctx, pl, name, a64, dev_type, "f32", "f64", in_dev, out_dev, ld, rows)
    finally:
        pl.close()


# =============================================================================================================================
# B. the chunked pipeline
# =============================================================================================================================
R = bd.CHUNK_R


def _where(got, want, host_dt=F64, dev_dt=F32):
    d = bd.first_difference(got, want)
    if d is None:
        return None
    chunk, buffer = bd.chunk_of(d[1], got.shape[0], host_dt, dev_dt)
    return dict(row=d[0], column=d[1], chunk=chunk, bounce_buffer=buffer, got=got[d], want=want[d])


def _h_plan(ctx, T):
    from se_snmf_nat_amd import Plan
    return Plan(ctx, 5, T, R, max_iter=1)


def _set_h(lib, pl, src):
    assert lib.snmf_plan_set_h_f64(pl._h, vp(src), src.ld, 0) == OK, err(lib)


def _get_h(lib, pl, T, ld):
    dst = strided_out(R, T, ld, F64)
    assert lib.snmf_plan_get_h_f64(pl._h, vp(dst), ld, 0) == OK, err(lib)
    return dst


@pytest.mark.parametrize("T", sorted(bd.CHUNK_CASES))
def test_b_one_to_five_chunks_contiguous_and_per_column(gpu_ctx, lib, T):
    """H (128 x T, fp32 on the device) from and to an fp64 host array: 32768 columns per chunk, so 1, 2 (one-column tail), 3, 4
    and 5 chunks; bounce buffers are reused from the fourth chunk on.  ld = r: one contiguous copy per pool item; ld = r + 3:
    column by column.  value(row, column) is unique, so a wrong element names the chunk it sits in."""
    a = bd.placed_values(R, T)
    want = a.astype(F32).astype(F64)
    assert same_bits(want, a)  # (exact in fp32: the narrowing on the way in loses nothing here)
    pl = _h_plan(gpu_ctx, T)
    try:
        for ld in bd.CHUNK_LDS:
            src = strided(a, ld)
            _set_h(lib, pl, src)
            dst = _get_h(lib, pl, T, ld)
            assert dst.intact(), (T, ld, "padding or guard band written")
            assert same_bits(dst.values(), want), (T, ld, _where(dst.values(), want))
            assert src.intact() and same_bits(src.values(), a)  # the source is read only
    finally:
        pl.close()


T4 = 98305  # 4 chunks


def test_b1_the_source_may_be_overwritten_after_set_returns(gpu_ctx, lib):
    """xfer_pack_in returns once the last chunk has left the caller's array (the tail of the pipeline is still in flight)."""
    a = bd.placed_values(R, T4)
    pl = _h_plan(gpu_ctx, T4)
    try:
        for ld in bd.CHUNK_LDS:
            src = strided(a, ld)
            _set_h(lib, pl, src)
            src.buf[:] = np.nan
            dst = _get_h(lib, pl, T4, ld)
            assert dst.intact() and same_bits(dst.values(), a), (ld, _where(dst.values(), a))
    finally:
        pl.close()


def test_b2_back_to_back_calls_without_a_synchronisation(gpu_ctx, lib):
    """set_h(A), get_h, set_h(B), get_h, set_w, get_w on one context with nothing between them: every get returns what the
    preceding set stored (H at the 4-chunk size; the bounce buffers and their events carry over from call to call)."""
    a = bd.placed_values(R, T4)
    b = np.asfortranarray(a[::-1, ::-1])
    w = bd.round_trip_values(5, R, 4)
    pl = _h_plan(gpu_ctx, T4)
    try:
        sa, sb, sw = strided(a, R + 3), strided(b, R), strided(w, 5 + 2)
        da, db, dw = strided_out(R, T4, R, F64), strided_out(R, T4, R + 3, F64), strided_out(5, R, 5 + 1, F64)
        rcs = [lib.snmf_plan_set_h_f64(pl._h, vp(sa), sa.ld, 0), lib.snmf_plan_get_h_f64(pl._h, vp(da), da.ld, 0),
               lib.snmf_plan_set_h_f64(pl._h, vp(sb), sb.ld, 0), lib.snmf_plan_get_h_f64(pl._h, vp(db), db.ld, 0),
               lib.snmf_plan_set_w_f64(pl._h, vp(sw), sw.ld, 0), lib.snmf_plan_get_w_f64(pl._h, vp(dw), dw.ld, 0)]
        assert rcs == [OK] * 6, err(lib)
        assert da.intact() and same_bits(da.values(), a), _where(da.values(), a)
        assert db.intact() and same_bits(db.values(), b), _where(db.values(), b)
        assert dw.intact() and same_bits(dw.values(), w)
    finally:
        pl.close()


def test_b3_the_fp64_staged_path_with_four_chunks_each_way(gpu_ctx, lib):
    """One masked fp64 batch problem (snmf_batch_create_mdi_fp64): V and M go up and V_mdi comes back staged as fp64, 8160
    columns per chunk, 4 chunks, all three with leading dimension F + 3.  The check is the IDENTITY V_mdi == V: with M == 1
    everywhere and V >= 1e-9 the imputation is v * 1 + Nt * max(w h, flr) * 0 = v and max(v, 1e-9) = v exactly
    (tests/test_boundary_rules.py shows it on oracle/mdi_oracle.py), whatever the one iteration does to W and H."""
    m = bd.MDI_CHUNK
    F, T, r = m["F"], m["T"], m["r"]
    rs = np.random.RandomState(5)
    V = np.asfortranarray(rs.gamma(0.5, 1.0, (F, T)) + 1e-3)
    assert V.min() >= 1e-9
    W0, H0 = col(rs.random_sample((F, r)) + 0.1, F64), col(rs.random_sample((r, T)) + 0.1, F64)
    sp = params(F, T, r, max_iter=1, sparsity=0.1)
    Ts = np.array([T], np.int32)
    b = C.c_void_p()
    assert lib.snmf_batch_create_mdi_fp64(gpu_ctx._h, C.byref(sp), 1, vp(Ts), C.byref(b)) == OK, err(lib)
    try:
        ld = F + 3
        sv, sm = strided(V, ld), strided(np.ones((F, T), order="F"), ld)
        out = strided_out(F, T, ld, F64)
        assert lib.snmf_batch_set_problem_mdi_f64(b, 0, vp(sv), ld, vp(sm), ld, vp(W0), vp(H0)) == OK, err(lib)
        assert lib.snmf_batch_run(b, 0) == OK, err(lib)
        assert lib.snmf_batch_get_v_mdi_f64(b, 0, vp(out), ld) == OK, err(lib)
        assert out.intact()
        assert same_bits(out.values(), V), _where(out.values(), V, F64, F64)
    finally:
        lib.snmf_batch_destroy(b)


def test_b4_two_host_threads_each_with_a_context(lib, gpu_ctx):
    """Two callers of the host worker pool at once (as the ranks of snmf_multi_* and the downloader thread of
    snmf_run_basis_dnmf_* are): each thread owns a context and moves a 4 MB matrix with ld != rows there and back."""
    from se_snmf_nat_amd import Context
    T = 4099
    assert R * T * 8 > bd.POOL_MIN_BYTES
    res = {}

    def work(i):
        try:
            ctx = Context(0)
            pl = _h_plan(ctx, T)
            ok = True
            for rep in range(3):
                a = bd.placed_values(R, T) + np.float64(i * 2 ** 20 + rep)
                src = strided(np.asfortranarray(a), R + 1 + i)
                _set_h(lib, pl, src)
                dst = _get_h(lib, pl, T, R + 5 - i)
                ok = ok and dst.intact() and same_bits(dst.values(), a)
            pl.close()
            ctx.close()
            res[i] = ok
        except BaseException as e:  # noqa: BLE001 (reported by the asserting thread)
            res[i] = e

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert res == {0: True, 1: True}, res


# =============================================================================================================================
# C / D. every computing entry: strided == tight, refusals
# =============================================================================================================================
F, T, r = 65, 45, 8


def _problem(dt=F64):
    V, W0, H0 = synth_problem(F, T, r, r_true=4)
    return col(V, dt), col(W0, dt), col(H0, dt)


@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_one_shot_in_place(gpu_ctx, lib, ty):
    dt = NP[ty]
    V, W0, H0 = _problem(dt)
    sp = params(F, T, r)
    fn = getattr(lib, f"snmf_sparse_nmf_{ty}")

    def call(ld, lay):
        v, w, h = inp(V, lay["V"]), inout(W0, dt), inout(H0, dt)
        n = C.c_int32()
        return fn(gpu_ctx._h, C.byref(sp), vp(v), ld["V"], vp(w), vp(h), None, None, None, C.byref(n)), dict(W=w, H=h)

    check_entry(lib, call, dict(V=F))


@pytest.mark.parametrize("entry", ["snmf_sparse_nmf_oop_f64", "snmf_sparse_nmf_oop_f32", "snmf_sparse_nmf_fp64"])
def test_c_one_shot_out_of_place_and_fp64(gpu_ctx, lib, entry):
    dt = F32 if entry.endswith("f32") else F64
    V, W0, H0 = _problem(dt)
    sp = params(F, T, r)
    fn = getattr(lib, entry)

    def call(ld, lay):
        v, w0, h0 = inp(V, lay["V"]), inp(W0, F), inp(H0, r)
        w, h = strided_out(F, r, F, dt), strided_out(r, T, r, dt)
        n = C.c_int32()
        rc = fn(gpu_ctx._h, C.byref(sp), vp(v), ld["V"], vp(w0), vp(h0), None, vp(w), vp(h), None, None, C.byref(n))
        return rc, dict(W=w, H=h)

    check_entry(lib, call, dict(V=F))


def _mask(rows, cols, seed=3):
    return col(np.random.RandomState(seed).random_sample((rows, cols)) > 0.3, F64)


def test_c_mdi_fp64_three_leading_dimensions(gpu_ctx, lib):
    V, W0, H0 = _problem()
    M = _mask(F, T)
    sp = params(F, T, r, sparsity=0.1)

    def call(ld, lay):
        v, m, w0, h0 = inp(V, lay["V"]), inp(M, lay["M"]), inp(W0, F), inp(H0, r)
        vm, w, h = strided_out(F, T, lay["Vm"], F64), strided_out(F, r, F, F64), strided_out(r, T, r, F64)
        n = C.c_int32()
        rc = lib.snmf_mdi_fp64(gpu_ctx._h, C.byref(sp), vp(v), ld["V"], vp(m), ld["M"], vp(w0), vp(h0), None, vp(vm), ld["Vm"], vp(w),
                               vp(h), None, None, C.byref(n))
        return rc, dict(Vm=vm, W=w, H=h)

    check_entry(lib, call, dict(V=F, M=F, Vm=F))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_plan_v_mask_and_v_mdi(gpu_ctx, lib, ty, dev):
    """snmf_plan_set_mask_*, snmf_plan_set_v_* and snmf_plan_get_v_mdi_* of a missing-data plan, host and device pointers."""
    from se_snmf_nat_amd import Plan
    dt = NP[ty]
    V, W0, H0 = _problem(dt)
    M = _mask(F, T).astype(dt)
    pl = Plan(gpu_ctx, F, T, r, max_iter=3, sparsity=0.1)

    def call(ld, lay):
        m, v = inp(M, lay["M"]), inp(V, lay["V"])
        vm, w, h = strided_out(F, T, lay["Vm"], dt), strided_out(F, r, F, dt), strided_out(r, T, r, dt)
        outs = dict(Vm=vm, W=w, H=h)
        if dev:
            m.to_device(), v.to_device(), vm.to_device()

        def done(rc):
            gpu_ctx.sync()
            vm.fetch()
            return rc, outs

        for step in (lambda: getattr(lib, f"snmf_plan_set_mask_{ty}")(pl._h, vp(m), ld["M"], int(dev)),
                     lambda: getattr(lib, f"snmf_plan_set_v_{ty}")(pl._h, vp(v), ld["V"], int(dev)),
                     lambda: getattr(lib, f"snmf_plan_set_w_{ty}")(pl._h, vp(W0), F, 0),
                     lambda: getattr(lib, f"snmf_plan_set_h_{ty}")(pl._h, vp(H0), r, 0),
                     lambda: lib.snmf_plan_init(pl._h),
                     lambda: lib.snmf_plan_run(pl._h, 3, None),
                     lambda: getattr(lib, f"snmf_plan_get_v_mdi_{ty}")(pl._h, vp(vm), ld["Vm"], int(dev)),
                     lambda: getattr(lib, f"snmf_plan_get_w_{ty}")(pl._h, vp(w), F, 0),
                     lambda: getattr(lib, f"snmf_plan_get_h_{ty}")(pl._h, vp(h), r, 0)):
            rc = step()
            if rc != OK:
                return done(rc)
        return done(OK)

    try:
        check_entry(lib, call, dict(M=F, V=F, Vm=F))
    finally:
        pl.close()


@pytest.mark.parametrize("tps", [1, 4])
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_solve_frames(gpu_ctx, lib, ty, tps):
    """snmf_plan_solve_frames_*: 6 solves of 1 and of 4 frames; the entry copies (ncols - 1) * ldV + F elements, padding
    included, and packs on the device."""
    from se_snmf_nat_amd import Plan
    dt = NP[ty]
    n_solves = 6
    V, W0, H0 = _problem(dt)
    V, H0 = col(V[:, :n_solves * tps], dt), col(H0[:, :tps], dt)
    pl = Plan(gpu_ctx, F, 24, r, max_iter=3, sparsity=5.0, w_update_ind=np.zeros(r, bool))
    pl.set_w(W0)
    fn = getattr(lib, f"snmf_plan_solve_frames_{ty}")

    def call(ld, lay):
        v, h0 = inp(V, lay["V"]), inp(H0, r)
        h = strided_out(r, n_solves * tps, r, dt)
        nit, cost = np.full(n_solves, -1, np.int32), np.zeros(n_solves)
        return fn(pl._h, tps, vp(v), ld["V"], n_solves, vp(h0), vp(h), vp(nit), vp(cost)), dict(H=h)

    try:
        check_entry(lib, call, dict(V=F))
    finally:
        pl.close()


# ---- DNMF ------------------------------------------------------------------------------------------------------------------
RX, RD = 5, 3
DNMF_ROWS = dict(Y=F, X=F, D=F, B=F, Bh=F, A=r)


def _dnmf_problem(dt, rows=F, cols=T):
    rs = np.random.default_rng(3)
    X = rs.gamma(0.5, 1.0, (rows, RX)) @ rs.gamma(0.3, 1.0, (RX, cols)) + 1e-9
    D = rs.gamma(0.5, 1.0, (rows, RD)) @ rs.gamma(0.3, 1.0, (RD, cols)) + 1e-9
    B = rs.random((rows, RX + RD)) + 0.05
    H0 = rs.random((RX + RD, cols)) + 0.05
    return tuple(col(a, dt) for a in (X + D, X, D, B, H0))


def _dnmf_call(lib, fn, head, sp, dt):
    Y, X, D, B, H0 = _dnmf_problem(dt)

    def call(ld, lay):
        y, x, d, b, h0 = inp(Y, lay["Y"]), inp(X, lay["X"]), inp(D, lay["D"]), inp(B, lay["B"]), inp(H0, r)
        bh, ah = strided_out(F, r, lay["Bh"], dt), strided_out(r, T, lay["A"], dt)
        nit = np.zeros(3, np.int32)
        rc = fn(*head, C.byref(sp), RX, RD, vp(y), ld["Y"], vp(x), ld["X"], vp(d), ld["D"], vp(b), ld["B"], vp(h0), 1, vp(bh), ld["Bh"],
                vp(ah), ld["A"], vp(nit))
        return rc, dict(Bh=bh, A=ah)

    return call


def _a_tight(rows):
    """Every argument strided but A_hat (ldA = r): the downloader thread then takes the contiguous copy."""
    lay = {n: rows[n] + 1 + 2 * i for i, n in enumerate(rows)}
    lay["A"] = rows["A"]
    return lay


@pytest.mark.parametrize("entry", ["snmf_run_basis_dnmf_f64", "snmf_run_basis_dnmf_f32", "snmf_run_basis_dnmf_fp64"])
def test_c_dnmf_six_leading_dimensions(gpu_ctx, lib, entry):
    dt = F32 if entry.endswith("f32") else F64
    call = _dnmf_call(lib, getattr(lib, entry), (gpu_ctx._h,), params(F, T, r), dt)
    check_entry(lib, call, DNMF_ROWS, extra=[_a_tight(DNMF_ROWS)])


@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_dnmf_over_a_device_list(gpu_ctx, lib, ty):
    devs = np.zeros(2, np.int32)
    call = _dnmf_call(lib, getattr(lib, f"snmf_run_basis_dnmf_multi_{ty}"), (vp(devs), 2), params(F, T, r), NP[ty])
    check_entry(lib, call, DNMF_ROWS, extra=[_a_tight(DNMF_ROWS)])


@pytest.mark.parametrize("entry", ["snmf_run_basis_dnmf_audio_f64", "snmf_run_basis_dnmf_audio_fp64"])
def test_c_dnmf_from_audio(gpu_ctx, lib, entry):
    """The waveform forms: ldB, ldBh, ldA (x, d are vectors)."""
    from se_snmf_nat_amd import frontend as fe
    sdt = F64 if entry.endswith("fp64") else F32
    n = np.arange(40)
    stft = dict(fftlength=64, framelength=40, frameshift=10, DCbin=1, win_STFT=np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / 40)))
    sp_stft, _win = fe._params(stft)
    L = 510
    Fa, Ta = 33, fe.num_frames(L, stft)
    assert Ta == T
    rs = np.random.RandomState(8)
    x, d = (np.ascontiguousarray(rs.standard_normal(L) * 1000, dtype=sdt) for _ in range(2))
    B, H0 = _dnmf_problem(F64, Fa, Ta)[3:]
    sp = params(Fa, Ta, r)
    fn = getattr(lib, entry)

    def call(ld, lay):
        b, h0 = inp(B, lay["B"]), inp(H0, r)
        bh, ah = strided_out(Fa, r, lay["Bh"], F64), strided_out(r, Ta, lay["A"], F64)
        nit = np.zeros(3, np.int32)
        rc = fn(gpu_ctx._h, C.byref(sp), C.byref(sp_stft), RX, RD, vp(x), L, vp(d), L, None, 0, vp(b), ld["B"], vp(h0), 1, vp(bh),
                ld["Bh"], vp(ah), ld["A"], vp(nit))
        return rc, dict(Bh=bh, A=ah)

    rows = dict(B=Fa, Bh=Fa, A=r)
    check_entry(lib, call, rows, extra=[_a_tight(rows)])


# ---- batch -------------------------------------------------------------------------------------------------------------------
BT = (7, 31)


def _batch_problems(dt):
    return [tuple(col(a, dt) for a in synth_problem(F, t, r, seed_data=10 * k, seed_init=10 * k + 1, r_true=4)) for k, t in enumerate(BT)]


@pytest.mark.parametrize("engine", ["fp32", "fp64"])
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_batch_set_problem(gpu_ctx, lib, ty, engine):
    dt = NP[ty]
    probs = _batch_problems(dt)
    sp = params(F, 1, r)
    Ts = np.array(BT, np.int32)
    b = C.c_void_p()
    create = lib.snmf_batch_create if engine == "fp32" else lib.snmf_batch_create_fp64
    assert create(gpu_ctx._h, C.byref(sp), 2, vp(Ts), C.byref(b)) == OK, err(lib)
    setp, get = getattr(lib, f"snmf_batch_set_problem_{ty}"), getattr(lib, f"snmf_batch_get_{ty}")

    def call(ld, lay):
        outs = {}
        for k, t in enumerate(BT):
            outs[f"W{k}"], outs[f"H{k}"] = strided_out(F, r, F, dt), strided_out(r, t, r, dt)
        for k, (V, W0, H0) in enumerate(probs):
            v, w0, h0 = inp(V, lay[f"V{k}"]), inp(W0, F), inp(H0, r)
            rc = setp(b, k, vp(v), ld[f"V{k}"], vp(w0), vp(h0))
            if rc != OK:
                return rc, outs
        rc = lib.snmf_batch_run(b, 0)
        for k in range(2):
            n = C.c_int32()
            rc = rc or get(b, k, vp(outs[f"W{k}"]), vp(outs[f"H{k}"]), None, None, C.byref(n))
        return rc, outs

    try:
        check_entry(lib, call, dict(V0=F, V1=F))
    finally:
        lib.snmf_batch_destroy(b)


@pytest.mark.parametrize("entry", ["snmf_sparse_nmf_batch_f64", "snmf_sparse_nmf_batch_f32", "snmf_sparse_nmf_batch_fp64"])
def test_c_batch_one_shot(gpu_ctx, lib, entry):
    dt = F32 if entry.endswith("f32") else F64
    probs = _batch_problems(dt)
    sp = params(F, 1, r)
    Ts = np.array(BT, np.int32)
    fn = getattr(lib, entry)

    def call(ld, lay):
        v = [inp(q[0], lay[f"V{k}"]) for k, q in enumerate(probs)]
        w0, h0 = [inp(q[1], F) for q in probs], [inp(q[2], r) for q in probs]
        w, h = [strided_out(F, r, F, dt) for _ in BT], [strided_out(r, t, r, dt) for t in BT]
        lds = np.array([ld["V0"], ld["V1"]], np.int64)
        nit = np.zeros(2, np.int32)
        rc = fn(gpu_ctx._h, C.byref(sp), 2, vp(Ts), ptrs(v), vp(lds), ptrs(w0), ptrs(h0), None, ptrs(w), ptrs(h), None, None, vp(nit))
        return rc, dict(W0=w[0], W1=w[1], H0=h[0], H1=h[1])

    check_entry(lib, call, dict(V0=F, V1=F))


def _mdi_batch_inputs():
    probs = _batch_problems(F64)
    return probs, [_mask(F, t, 20 + k) for k, t in enumerate(BT)]


MDI_B_ROWS = dict(V0=F, M0=F, Vm0=F, V1=F, M1=F, Vm1=F)


def test_c_batch_mdi_resident(gpu_ctx, lib):
    probs, masks = _mdi_batch_inputs()
    sp = params(F, 1, r, sparsity=0.1)
    Ts = np.array(BT, np.int32)
    b = C.c_void_p()
    assert lib.snmf_batch_create_mdi_fp64(gpu_ctx._h, C.byref(sp), 2, vp(Ts), C.byref(b)) == OK, err(lib)

    def call(ld, lay):
        outs = {}
        for k, t in enumerate(BT):
            outs[f"Vm{k}"], outs[f"H{k}"] = strided_out(F, t, lay[f"Vm{k}"], F64), strided_out(r, t, r, F64)
        for k, (V, W0, H0) in enumerate(probs):
            v, m, w0, h0 = inp(V, lay[f"V{k}"]), inp(masks[k], lay[f"M{k}"]), inp(W0, F), inp(H0, r)
            rc = lib.snmf_batch_set_problem_mdi_f64(b, k, vp(v), ld[f"V{k}"], vp(m), ld[f"M{k}"], vp(w0), vp(h0))
            if rc != OK:
                return rc, outs
        rc = lib.snmf_batch_run(b, 0)
        if rc != OK:
            return rc, outs
        for k in range(2):  # every leading dimension is looked at before a result is read, as a one-shot entry would
            if ld[f"Vm{k}"] < F:
                return lib.snmf_batch_get_v_mdi_f64(b, k, vp(outs[f"Vm{k}"]), ld[f"Vm{k}"]), outs
        for k in range(2):
            n = C.c_int32()
            rc = rc or lib.snmf_batch_get_f64(b, k, None, vp(outs[f"H{k}"]), None, None, C.byref(n))
            rc = rc or lib.snmf_batch_get_v_mdi_f64(b, k, vp(outs[f"Vm{k}"]), ld[f"Vm{k}"])
        return rc, outs

    try:
        check_entry(lib, call, MDI_B_ROWS)
    finally:
        lib.snmf_batch_destroy(b)


def test_c_batch_mdi_one_shot(gpu_ctx, lib):
    """snmf_mdi_batch_fp64 with per-problem ldV[], ldM[], ldVm[]; a refused ldVm[] of EITHER problem writes no output of any
    problem; ldVm = NULL means tight."""
    probs, masks = _mdi_batch_inputs()
    sp = params(F, 1, r, sparsity=0.1)
    Ts = np.array(BT, np.int32)

    def run(ld, lay, null_ldvm=False):
        v, m = [inp(q[0], lay[f"V{k}"]) for k, q in enumerate(probs)], [inp(masks[k], lay[f"M{k}"]) for k in range(2)]
        w0, h0 = [inp(q[1], F) for q in probs], [inp(q[2], r) for q in probs]
        vm = [strided_out(F, t, lay[f"Vm{k}"], F64) for k, t in enumerate(BT)]
        w, h = [strided_out(F, r, F, F64) for _ in BT], [strided_out(r, t, r, F64) for t in BT]
        lv, lm, lo = (np.array([ld[f"{n}0"], ld[f"{n}1"]], np.int64) for n in ("V", "M", "Vm"))
        nit = np.zeros(2, np.int32)
        rc = lib.snmf_mdi_batch_fp64(gpu_ctx._h, C.byref(sp), 2, vp(Ts), ptrs(v), vp(lv), ptrs(m), vp(lm), ptrs(w0), ptrs(h0), None, ptrs(vm),
                                     None if null_ldvm else vp(lo), ptrs(w), ptrs(h), None, None, vp(nit))
        return rc, dict(Vm0=vm[0], Vm1=vm[1], W0=w[0], W1=w[1], H0=h[0], H1=h[1])

    check_entry(lib, run, MDI_B_ROWS)
    rc, ref = run(MDI_B_ROWS, MDI_B_ROWS)
    assert rc == OK
    lay = {n: v + 1 + 2 * i for i, (n, v) in enumerate(MDI_B_ROWS.items())}
    lay["Vm0"] = lay["Vm1"] = F
    rc, got = run(lay, lay, null_ldvm=True)
    assert rc == OK, err(lib)
    outs_same(got, ref, "ldVm = NULL")


# ---- multi-rank: two ranks on device 0, T odd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_multi_handle(gpu_ctx, lib, ty):
    """snmf_multi_set_v / set_w / set_h / get_w / get_w_rank_f64 / get_h: rank 1's shard starts at col[1] * ld."""
    dt = NP[ty]
    V, W0, H0 = _problem(dt)
    sp = params(F, T, r)
    devs = np.zeros(2, np.int32)
    h = C.c_void_p()
    assert lib.snmf_multi_create(vp(devs), 2, C.byref(sp), None, C.byref(h)) == OK, err(lib)
    f = lambda nm: getattr(lib, f"snmf_multi_{nm}_{ty}")  # noqa: E731

    def call(ld, lay):
        v, w0, h0 = inp(V, lay["V"]), inp(W0, lay["W0"]), inp(H0, lay["H0"])
        outs = dict(W=strided_out(F, r, lay["W"], dt), Wr=strided_out(F, r, lay["Wr"], F64), H=strided_out(r, T, lay["H"], dt))
        done = C.c_int32()
        for step in (lambda: f("set_v")(h, vp(v), ld["V"]), lambda: f("set_w")(h, vp(w0), ld["W0"]), lambda: f("set_h")(h, vp(h0), ld["H0"]),
                     lambda: lib.snmf_multi_init(h), lambda: lib.snmf_multi_run(h, 3, C.byref(done))):
            rc = step()
            if rc != OK:
                return rc, outs
        gets = dict(W=lambda: f("get_w")(h, vp(outs["W"]), ld["W"]), Wr=lambda: lib.snmf_multi_get_w_rank_f64(h, 1, vp(outs["Wr"]), ld["Wr"]),
                    H=lambda: f("get_h")(h, vp(outs["H"]), ld["H"]))
        for n, rows_n in (("W", F), ("Wr", F), ("H", r)):  # the three readers are calls of their own: a refused one is made alone
            if ld[n] < rows_n:
                return gets[n](), outs
        rc = gets["W"]() or gets["Wr"]() or gets["H"]()
        if rc == OK and ty == "f64":
            assert same_bits(outs["W"].values(), outs["Wr"].values())  # the replicas
        return rc, outs

    try:
        check_entry(lib, call, dict(V=F, W0=F, H0=r, W=F, Wr=F, H=r))
    finally:
        lib.snmf_multi_destroy(h)


@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_c_multi_one_shot(gpu_ctx, lib, ty):
    dt = NP[ty]
    V, W0, H0 = _problem(dt)
    sp = params(F, T, r)
    devs = np.zeros(2, np.int32)
    fn = getattr(lib, f"snmf_sparse_nmf_multi_{ty}")

    def call(ld, lay):
        v, w, h = inp(V, lay["V"]), inout(W0, dt), inout(H0, dt)
        n = C.c_int32()
        return fn(vp(devs), 2, C.byref(sp), vp(v), ld["V"], vp(w), vp(h), None, None, None, C.byref(n)), dict(W=w, H=h)

    check_entry(lib, call, dict(V=F))


# ---- online basis readers ----------------------------------------------------------------------------------------------------
ONLINE = dict(fft=64, sz=64, hop=16, R_x=8, R_d=12, over=dict(R_a=6, m_a=12, overlap_m_a=0.2, Ar_up=2.0, P_len_k=8, P_len_l=4, init_N_len=4,
                                                             DCbin=1, DCbin_back=1, delay=2))  # tests/test_online.py's smallest geometry
N_MEL = 12


def _online_setup(mel):
    from oracle.online_oracle import default_params
    from se_snmf_nat_amd.online import default_settings
    g = ONLINE
    rs = np.random.RandomState(g["fft"])
    Fo = g["fft"] // 2 + 1
    B = rs.gamma(0.6, 1.0, (Fo, g["R_x"] + g["R_d"])) + 1e-3
    B = B / np.sqrt((B ** 2).sum(0)) + 1e-9
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(g["sz"]) / g["sz"]))
    p = dict(default_params(), fftlength=g["fft"], framelength=g["sz"], frameshift=g["hop"], win_STFT=win, win_ISTFT=win.copy(),
             overlapscale=2 * g["hop"] / g["sz"])
    p.update(g["over"])
    ps = dict(default_settings(), **{k: v for k, v in p.items() if k in default_settings()})
    ps["fs"] = p["fs"]
    kw = {}
    if mel:
        from se_snmf_nat_amd.frontend import mel_matrix
        ps.update(B_sep_mode="Mel", MelConv=1, F_order=N_MEL)
        mm = mel_matrix(ps["fs"], N_MEL, g["fft"], 1.0, ps["fs"] / 2).T
        assert mm.shape == (N_MEL, Fo) and (mm.sum(1) > 0).all()
        BM = mm @ B
        BM = BM / np.sqrt((BM ** 2).sum(0)) + 1e-9
        kw = dict(B_Mel_x=BM[:, :g["R_x"]], B_Mel_d=BM[:, g["R_x"]:])
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"][:g["hop"] * 44]
    rs = np.random.RandomState(7)
    H0, Ad0 = rs.random_sample(g["R_x"] + g["R_d"]), rs.random_sample((ps["R_a"], ps["m_a"]))
    return s, B[:, :g["R_x"]], B[:, g["R_x"]:], ps, H0, Ad0, kw


def _reader(fn, handle, rows, cols, dt):
    def call(ld, lay):
        out = strided_out(rows, cols, lay["B"], dt)
        return fn(*handle, vp(out), ld["B"]), dict(B=out)
    return call


def _moved(call, rows, start, dt):
    """The basis the reader returns is no longer the one the separator started with (an adaptation solve ran)."""
    rc, out = call(dict(B=rows), dict(B=rows))
    assert rc == OK
    return not same_bits(out["B"].values(), col(start, dt))


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_c_online_basis_readers(gpu_ctx, lib, precision):
    """snmf_online_get_basis_f32 / _f64 on an fp32 and on an fp64 separator after 44 hops with adaptation on (the f64 entry on
    an fp32 separator reads its fp64 master; the f32 entry on an fp64 separator rounds)."""
    from se_snmf_nat_amd.online import OnlineSeparator
    s, Bx, Bd, ps, H0, Ad0, _ = _online_setup(False)
    sep = OnlineSeparator(Bx, Bd, ps, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, precision=precision)
    try:
        sep.process(s)
        assert sum(t["solved"] for t in sep.trace()) > 0
        Fo, Rd = Bd.shape
        for fn, dt in ((lib.snmf_online_get_basis_f32, F32), (lib.snmf_online_get_basis_f64, F64)):
            call = _reader(fn, (sep._h,), Fo, Rd, dt)
            assert _moved(call, Fo, Bd, dt)
            check_entry(lib, call, dict(B=Fo))
    finally:
        sep.close()


def test_c_online_mel_basis_reader(gpu_ctx, lib):
    from se_snmf_nat_amd.online import OnlineSeparator
    s, Bx, Bd, ps, H0, Ad0, kw = _online_setup(True)
    sep = OnlineSeparator(Bx, Bd, ps, H0=H0, Ad_blk0=Ad0, ctx=gpu_ctx, **kw)
    try:
        sep.process(s)
        call = _reader(lib.snmf_online_get_mel_basis_f32, (sep._h,), N_MEL, Bd.shape[1], F32)
        if sum(t["solved"] for t in sep.trace()) > 0:
            assert _moved(call, N_MEL, kw["B_Mel_d"], F32)
        check_entry(lib, call, dict(B=N_MEL))
    finally:
        sep.close()


@pytest.mark.parametrize("mode", ["fp32", "fp64", "mel"])
def test_c_online_batch_basis_readers(gpu_ctx, lib, mode):
    """The batch forms, stream 1 of 2: get_basis_f32 / _f64 on an fp32 and an fp64 batch, get_mel_basis_f32 / _f64 on a Mel batch."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    s, Bx, Bd, ps, H0, Ad0, kw = _online_setup(mode == "mel")
    Bd2 = [Bd, Bd[:, ::-1].copy()]
    if kw:
        kw["B_Mel_d"] = [kw["B_Mel_d"], kw["B_Mel_d"][:, ::-1].copy()]
    sep = OnlineBatchSeparator(Bx, Bd2, ps, 2, H0=[H0, H0[::-1].copy()], Ad_blk0=[Ad0, Ad0[::-1].copy()], ctx=gpu_ctx,
                               precision="fp64" if mode == "fp64" else "fp32", **kw)
    try:
        sep.process([s, s[:s.size // 2]])
        solved = sum(t["solved"] for t in sep.trace(1)) > 0
        Fo, Rd = Bd.shape
        if mode == "mel":
            readers = ((lib.snmf_online_batch_get_mel_basis_f32, F32, N_MEL, kw["B_Mel_d"][1]),
                       (lib.snmf_online_batch_get_mel_basis_f64, F64, N_MEL, kw["B_Mel_d"][1]))
        else:
            readers = ((lib.snmf_online_batch_get_basis_f32, F32, Fo, Bd2[1]), (lib.snmf_online_batch_get_basis_f64, F64, Fo, Bd2[1]))
        for fn, dt, rows, start in readers:
            call = _reader(fn, (sep._h, 1), rows, Rd, dt)
            if solved:
                assert _moved(call, rows, start, dt)
            check_entry(lib, call, dict(B=rows))
    finally:
        sep.close()
