"""CPU checks of the boundary tests' own tools (tests/boundary.py): the header coverage table, the strided buffers, the
comparator against five mutants, and the mirrored chunk arithmetic of csrc/snmf_tu_xfer.hip.  tests/test_gpu_boundary.py is
only as good as these."""
import os
import re

import numpy as np
import pytest

import boundary as bd


# ---- header coverage -------------------------------------------------------------------------------------------------------
def test_every_leading_dimension_of_the_header_is_mapped_to_a_test():
    lds = bd.header_ld_parameters()
    n_params = sum(len(v) for v in lds.values())
    print(f"include/snmf.h: {n_params} leading dimensions in {len(lds)} entries")
    assert n_params >= 75 and len(lds) >= 60
    assert sorted(set(lds) - set(bd.ENTRIES)) == [], "an ld parameter without a row in boundary.ENTRIES"
    assert sorted(set(bd.ENTRIES) - set(lds)) == [], "a row of boundary.ENTRIES for an entry without an ld parameter"
    for fn, where in bd.ENTRIES.items():
        assert where == bd.HERE or os.path.isfile(os.path.join(bd.ROOT, where)), (fn, where)
    # the multi-parameter entries are parsed whole
    assert lds["snmf_run_basis_dnmf_f64"] == ["ldY", "ldX", "ldD", "ldB", "ldBh", "ldA"]
    assert lds["snmf_mdi_batch_fp64"] == ["ldV", "ldM", "ldVm"] and lds["snmf_mel_features_fp64"] == ["ldv", "ldo"]


def test_entries_marked_here_are_called_by_the_gpu_file():
    src = open(os.path.join(bd.ROOT, "tests", "test_gpu_boundary.py")).read()
    names = set(re.findall(r"snmf_\w+", src))
    # names the file builds from a stem and a type suffix: f"snmf_plan_set_w_{ty}" ...
    stems = [re.escape(s).replace(r"\{\}", r"\w+") for s in re.findall(r"""["'](snmf_[\w{}]*\{\}[\w{}]*)["']""", re.sub(r"\{\w+\}", "{}", src))]
    missing = [fn for fn, where in bd.ENTRIES.items()
               if where == bd.HERE and fn not in names and not any(re.fullmatch(s, fn) for s in stems)]
    assert missing == []


def test_the_front_end_file_passes_leading_dimensions_above_the_row_count():
    """The front-end rows of the table point at tests/test_gpu_frontend_envelope.py: it calls each of the three entry families
    in both modes with a padded leading dimension and checks the padding."""
    src = open(os.path.join(bd.ROOT, bd.FRONTEND)).read()
    assert re.search(r'MODES\s*=\s*\(?\[?\s*"f32",\s*"fp64"', src)
    for stem in ("snmf_stft_features_", "snmf_mel_features_", "snmf_tf_dd_"):
        assert f'getattr(lib, "{stem}" + mode)' in src, stem
        assert any(fn.startswith(stem) and where == bd.FRONTEND for fn, where in bd.ENTRIES.items())
    assert "(False, F + 3), (True, F), (True, F + 5)" in src            # stft: ld = F + 3 host, F + 5 device
    assert "(rv + 2, ro + 3, False)" in src and "(rv + 2, ro + 3, True)" in src  # mel: ldv, ldo
    assert '(F + 2, F + 3, "host")' in src and '(F + 2, F + 3, "dev")' in src    # tf_dd: ldx, ldo
    assert "only_sentinel(rest)" in src and "np.nan" in src


# ---- the buffers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("rows,cols,ld", [(5, 4, 5), (5, 4, 6), (5, 1, 66), (1, 7, 3), (3, 3, 3 + 2 ** 20)])
def test_strided_has_the_blas_size_padding_and_guard(dt, rows, cols, ld):
    a = bd.placed_values(rows, cols, dt)
    s = bd.strided(a, ld)
    assert s.n == (cols - 1) * ld + rows and s.buf.size == s.n + bd.GUARD and s.buf.dtype == dt
    assert bd.same_bits(s.values(), a) and s.intact() and not s.untouched()
    flat = s.buf
    for c in range(cols):
        assert bd.same_bits(flat[c * ld:c * ld + rows], a[:, c])
        if c < cols - 1:
            assert np.isnan(flat[c * ld + rows:(c + 1) * ld]).all()
    assert np.isnan(flat[s.n:]).all() and flat[s.n:].size == bd.GUARD
    assert s.rest().size == (ld - rows) * (cols - 1) + bd.GUARD
    o = bd.strided_out(rows, cols, ld, dt)
    assert o.untouched() and o.intact() and o.buf.size == s.buf.size
    assert (bd.ubits(o.buf) == bd.SENT_BITS[np.dtype(dt)]).all()
    assert bd.sentinel(dt) < 0 and np.isfinite(bd.sentinel(dt))  # no non-negative result equals it
    o.buf[0] = 1
    assert not o.untouched() and o.intact()


# ---- the comparator against its mutants ------------------------------------------------------------------------------------
def _filled(want, ld):
    o = bd.strided_out(want.shape[0], want.shape[1], ld, want.dtype)
    o._matrix(o.buf)[...] = want
    return o


@pytest.mark.parametrize("ld", [6, 9])
def test_the_comparator_rejects_shifts_stray_writes_and_truncation(ld):
    a64 = bd.round_trip_values(6, 5, 3)
    want = bd.expect(a64, np.float64, np.float32, np.float32)
    assert bd.matches(_filled(want, ld), want)
    assert not bd.matches(_filled(np.roll(want, 1, axis=1), ld), want)  # one column off
    assert not bd.matches(_filled(np.roll(want, 1, axis=0), ld), want)  # one row off
    assert bd.first_difference(np.roll(want, 1, axis=1), want) == (0, 0)
    o = _filled(want, ld)
    o.buf[o.n] = want[0, 0]  # the first guard element
    assert not bd.matches(o, want)
    o = _filled(want, ld)
    o.buf[o.n + bd.GUARD - 1] = 0.0  # the last one
    assert not bd.matches(o, want)
    if ld > 6:
        o = _filled(want, ld)
        o.buf[6] = want[0, 0]  # row `rows` of column 0: padding
        assert not bd.matches(o, want)
        o = _filled(want, ld)
        o.buf[3 * ld + ld - 1] = np.float32(0)  # the last padding row of column 3
        assert not bd.matches(o, want)
    # truncation in place of round-to-nearest, on an input where the two differ: 1 + 0.75 ulp(fp32) rounds up, truncates down
    x = np.full((6, 5), 1.0 + 0.75 * 2.0 ** -23, order="F")
    rn, tr = bd.expect(x, np.float64, np.float32, np.float32), bd.truncate_to_f32(x)
    assert rn[0, 0] == np.float32(1.0) + np.float32(2.0 ** -23) and tr[0, 0] == np.float32(1.0)
    assert bd.matches(_filled(rn, ld), rn) and not bd.matches(_filled(tr, ld), rn)
    # ... and on the round-trip values themselves (ties go to even: half of them round up)
    assert not bd.same_bits(bd.truncate_to_f32(a64), want)
    # a NaN is told from the same NaN only by its bits; the sentinel never equals a result
    assert not bd.matches(bd.strided_out(6, 5, ld, np.float32), want)


def test_expect_rounds_once_and_widens_exactly():
    a = bd.round_trip_values(7, 9, 5)
    assert a.min() > 0 and a.min() < 1e-25 and a.max() > 1e25
    lo = a.astype(np.float32)
    ties = (np.arange(63).reshape(9, 7).T % 3) == 0
    mid = lambda other: (lo.astype(np.float64) + np.nextafter(lo, np.float32(other)).astype(np.float64)) / 2  # noqa: E731
    assert ((a == mid(np.inf)) | (a == mid(0)))[ties].all() and (a != lo)[ties].all()  # exact midpoints of two fp32 neighbours
    assert ((a == mid(np.inf)) & ties).any() and ((a == mid(0)) & ties).any()            # rounded down here, up there
    assert (bd.ubits(lo[ties]) & np.uint32(1) == 0).all()  # round-to-nearest-even took the even neighbour
    assert bd.same_bits(bd.expect(a, np.float64, np.float64, np.float64), a)            # the fp64 master of W: identity
    assert bd.same_bits(bd.expect(a, np.float64, np.float64, np.float32), lo)           # one rounding on the way out
    assert bd.same_bits(bd.expect(a, np.float64, np.float32, np.float64), lo.astype(np.float64))  # H: one on the way in, exact out
    assert bd.same_bits(bd.expect(a, np.float32, np.float64, np.float32), lo)           # f32 -> master -> f32 is exact


# ---- the chunk arithmetic --------------------------------------------------------------------------------------------------
def test_the_mirror_has_the_constants_of_the_source():
    assert bd.xfer_constants_in_source() == (bd.CHUNK_BYTES, bd.N_BUFFERS, bd.POOL_MIN_BYTES)
    lines = open(bd.XFER_SRC).read().split("\n")
    assert "kChunkBytes" in lines[28] and "kNB" in lines[29] and "kPoolMinBytes" in lines[30]  # the lines boundary.py names


def test_chunk_cases_claim_what_the_arithmetic_gives():
    assert sorted(n for n, _ in bd.CHUNK_CASES.values()) == [1, 2, 3, 4, 5]
    for T, (n, last) in bd.CHUNK_CASES.items():
        cpc, got_n, got_last, host_bytes = bd.chunking(bd.CHUNK_R, T, np.float64, np.float32)
        assert (cpc, got_n, got_last) == (32768, n, last), T
        assert host_bytes >= bd.POOL_MIN_BYTES  # the pool copies it (snmf_tu_xfer.hip: host_to_pinned)
    assert bd.CHUNK_CASES[32769][1] == 1 and bd.CHUNK_CASES[98304] == (3, 32768)  # a one-column tail; exactly kNB chunks
    assert max(bd.CHUNK_CASES) * bd.CHUNK_LDS[1] * 8 < 140e6  # the largest host array
    assert bd.chunk_of(98304, bd.CHUNK_R, np.float64, np.float32) == (3, 0)  # the fourth chunk reuses buffer 0
    assert bd.chunk_of(131072, bd.CHUNK_R, np.float64, np.float32) == (4, 1)
    m = bd.MDI_CHUNK
    cpc, n, last, host_bytes = bd.chunking(m["F"], m["T"], np.float64, np.float64)
    assert (cpc, n, last) == (8160, m["chunks"], m["last"]) and host_bytes >= bd.POOL_MIN_BYTES
    assert bd.staged_size(np.float32, np.float64) == 4 and bd.staged_size(np.float64, np.float64) == 8
    # section A stays in one chunk, below the pool threshold
    for F, r, T in bd.ROUND_TRIP_SHAPES:
        assert bd.chunking(F, r, np.float64, np.float64)[1] == 1 and bd.chunking(r, T, np.float64, np.float32)[1] == 1


def test_a_full_mask_makes_the_imputation_the_identity_in_the_oracle():
    """B3 of test_gpu_boundary.py asserts V_mdi == V bit for bit for M == 1 and V >= 1e-9: the oracle shows the identity
    (v .* 1 + Nt .* max(w*h, flr) .* 0 = v exactly, and max(v, 1e-9) = v)."""
    from oracle.mdi_oracle import snmf_mdi
    rs = np.random.RandomState(2)
    F, T, r = 33, 21, 2
    V = np.maximum(rs.gamma(0.5, 1.0, (F, T)), 1e-9)
    p = dict(cf="kl", sparsity_mdi=0.1, max_iter=1, conv_eps_mdi=0.0, cost_check=1, init_w=rs.random_sample((F, r)) + 0.1,
             init_h=rs.random_sample((r, T)) + 0.1, r=r)
    v_mdi = snmf_mdi(V, np.ones((F, T)), p)[0]
    assert bd.same_bits(np.asfortranarray(v_mdi), np.asfortranarray(V))
