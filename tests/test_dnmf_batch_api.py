"""CPU tests of run_basis_dnmf_batch: its errors fire before the library is loaded, its names are exported, its three C entries
are bound once each and carry no leading dimension, and the "edges" batch of the GPU tests stops where those tests need it to."""
import numpy as np
import pytest

import boundary
import dnmf_batch_cases as dc


def test_every_argument_error_is_raised_before_any_library_call(monkeypatch):
    from se_snmf_nat_amd import _lib, batch
    from se_snmf_nat_amd.batch import run_basis_dnmf_batch

    def no_device(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(batch, "default_context", no_device)
    F, T, Rx, Rd = 6, 5, 2, 3
    r = Rx + Rd
    V, V2 = np.ones((F, T)), np.ones((F, T + 1))
    B, H = np.ones((F, r)), np.ones((r, T))
    p = dict(cf="kl", sparsity=0.1, max_iter=3, cost_check=1)

    def status(Ys, Xs, Ds, Bq=B, pq=p, **kw):
        with pytest.raises(_lib.SnmfError) as e:
            run_basis_dnmf_batch(Ys, Xs, Ds, Bq, Rx, Rd, pq, **kw)
        return e.value.status

    assert status([], [], []) == 1                                   # an empty batch
    assert status([V, V], [V], [V, V]) == 1                          # lists of different lengths
    assert status([V, V], [V, V], [V]) == 1
    assert status([V, np.ones((F + 1, T))], [V, np.ones((F + 1, T))], [V, np.ones((F + 1, T))]) == 3  # row counts differ
    assert status([V], [V2], [V]) == 3                               # X_k not the shape of Y_k
    assert status([V], [V], [V2]) == 3                               # D_k not the shape of Y_k
    assert status([V], [V], [V], Bq=np.ones((F, r + 1))) == 3        # B of the wrong shape
    assert status([V, V], [V, V], [V, V], Bq=[B]) == 3               # B of the wrong list length
    assert status([V, V], [V, V], [V, V], Bq=[B, B[:-1]]) == 3
    assert status([V], [V], [V], h0=[np.ones((r, T + 1))]) == 3      # h0 of the wrong shape
    assert status([V, V], [V, V], [V, V], h0=[H]) == 3               # h0 of the wrong list length
    assert status([V], [V], [V], h0="device") == 3
    assert status([V], [V], [V], pq=dict(cf="kl", sparsity=0.1)) == 4                # no cost_check (src/sparse_nmf.m:260)
    assert status([V], [V], [V], pq=dict(p, sparsity=np.ones(r))) == 3               # a non-scalar sparsity
    assert status([V], [V], [V], precision="fp64", dtype=np.float32) == 1            # the fp64 mode takes doubles
    with pytest.raises(ValueError):
        run_basis_dnmf_batch([V], [V], [V], B, Rx, Rd, p, precision="bf16")
    # a valid call passes every check and only then reaches the library
    with pytest.raises(AssertionError, match="reached the library"):
        run_basis_dnmf_batch([V, V2], [V, V2], [V, V2], [B, B], Rx, Rd, p, h0=[H, np.ones((r, T + 1))], precision="fp64")


def test_names_are_exported():
    import se_snmf_nat_amd
    from se_snmf_nat_amd import batch
    assert "run_basis_dnmf_batch" in batch.__all__
    assert se_snmf_nat_amd.run_basis_dnmf_batch is batch.run_basis_dnmf_batch


def test_c_entries_are_bound_once_and_take_no_leading_dimension():
    from se_snmf_nat_amd import _lib
    for ty in ("f64", "f32", "fp64"):
        assert _lib.SYMBOLS.count(f"snmf_run_basis_dnmf_batch_{ty}") == 1
    assert not [k for k in boundary.header_ld_parameters() if k.startswith("snmf_run_basis_dnmf_batch")]


def test_c_entries_refuse_bad_arguments_without_a_device(lib):
    """What the driver refuses comes before the device is touched, so it can be checked where there is none."""
    import ctypes as C

    from se_snmf_nat_amd.api import _make_params
    sp = _make_params(8, 1, 5, 1.0, 3, 0.0, 1, True, 0, 0.1, None, None)
    for ty in ("f64", "f32", "fp64"):
        fn = getattr(lib, f"snmf_run_basis_dnmf_batch_{ty}")
        assert fn(None, C.byref(sp), 2, 3, 1, None, None, None, None, None, None, None, None, None) == 1


def test_edges_stop_iterates_lie_in_both_buffers():
    """Solve 1 of the "edges" problems on the oracle: one runs to max_iter, the others stop at odd and at even iterates."""
    n1 = [dc.oracle_dnmf(*q, dc.R_X, dc.R_D, dc.P_EDGES)[2][0] for q in dc.edges()]
    print("oracle solve-1 stop indices:", n1)
    assert dc.covers_both_buffers(n1, dc.P_EDGES["max_iter"])
