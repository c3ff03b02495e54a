"""GPU tests of assemble_training_signals (snmf_train_signals_*): every class's training signal formed on the device from its
clips, against the NumPy restatement of run_basis_train.m:16-57 in tests/assemble_cases.py.

Judged per case: lengths and clips_used equal; the kept-sample pattern equal, read through the signal (every output sample's
sign and its rank among its clip's absolute values are the restatement's); every sample within TOL = 1e-12 * 30000 of the
restatement's.  test_assemble_api.py asserts on the CPU that no frame quotient of these cases is within 1e-9 of the threshold,
so a different summation order cannot move a decision.  The cases (assemble_cases.CASES): all three modes in one call with
every stop and clip-length edge, a call without the file cut, the two committed recordings at 16 kHz, and single VAD clips of one
below, at and one above the work blocks a workgroup folds per pass and a scan group holds.  The tests print their figures before
they assert; measured on an MI355X: at most 7.3e-12 (one ulp of 30000) in every case."""
import ctypes as C

import numpy as np
import pytest

import assemble_cases as ac

pytestmark = pytest.mark.gpu
_cache = {}


def assembled(ctx, name, as_double=False):
    """-> (lengths, clips_used, [s_full per class]) of one case, computed once per (case, entry)."""
    key = (name, as_double)
    if key not in _cache:
        from se_snmf_nat_amd import assemble_training_signals
        case = ac.CASES[name]()
        classes = [[ac.pcm_to_double(c) for c in cl] for cl in case["classes"]] if as_double else case["classes"]
        with assemble_training_signals(classes, case["p"], vad=case["vad"], ranges=case["ranges"], ctx=ctx) as ts:
            sigs = [ts.signal(k) for k in range(len(classes))]
            for s in sigs:
                s.setflags(write=False)
            _cache[key] = (list(ts.lengths), list(ts.clips_used), sigs)
    return _cache[key]


def dense_rank(x):
    return np.unique(x, return_inverse=True)[1]


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_signals_are_the_restatements(gpu_ctx, name):
    lengths, used, sigs = assembled(gpu_ctx, name)
    ref = ac.reference(name)
    print(name, "lengths", lengths, "clips_used", used)
    assert lengths == [len(s) for s, _, _ in ref]
    assert used == [u for _, u, _ in ref]
    worst = 0.0
    for k, (got, (want, _, seg)) in enumerate(zip(sigs, ref)):
        assert got.dtype == np.float64 and got.shape == want.shape, k
        assert np.isfinite(got).all(), k
        assert np.array_equal(np.sign(got), np.sign(want)), k
        for i, (a, b) in enumerate(seg):
            assert np.array_equal(dense_rank(np.abs(got[a:b])), dense_rank(np.abs(want[a:b]))), (k, i)
        if len(want):
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"{name}: largest |device - restatement| {worst:.3e} (bound {ac.TOL:.1e})")
    assert worst <= ac.TOL


@pytest.mark.parametrize("name", ["mixed", "recordings"])
def test_int16_and_double_clips_give_the_same_bits(gpu_ctx, name):
    a, b = assembled(gpu_ctx, name), assembled(gpu_ctx, name, as_double=True)
    assert a[0] == b[0] and a[1] == b[1]
    for k, (x, y) in enumerate(zip(a[2], b[2])):
        assert np.array_equal(x, y), k


def test_two_runs_give_the_same_bits(gpu_ctx):
    from se_snmf_nat_amd import assemble_training_signals
    case = ac.case_mixed()
    first = assembled(gpu_ctx, "mixed")
    with assemble_training_signals(case["classes"], case["p"], vad=case["vad"], ranges=case["ranges"], ctx=gpu_ctx) as ts:
        assert ts.lengths == first[0] and ts.clips_used == first[1]
        for k, s in enumerate(first[2]):
            assert np.array_equal(ts.signal(k), s), k


def test_a_class_does_not_depend_on_the_classes_around_it(gpu_ctx):
    """Alone, a class's clips lie elsewhere in the input slab (another alignment of the 8-sample vectors) and its work blocks
    are the first of every launch."""
    from se_snmf_nat_amd import assemble_training_signals
    case = ac.case_mixed()
    for k in (0, 4, 1):
        with assemble_training_signals([case["classes"][k][1:]], case["p"], vad=[case["vad"][k]],
                                       ranges=[case["ranges"][k][1:] if case["ranges"][k] is not None else None], ctx=gpu_ctx) as ts:
            want = ac.assemble_class(case["classes"][k][1:], ac.modes(case)[k], case["ranges"][k][1:] if case["ranges"][k] is not None else None,
                                     1000, 6000, 1500)
            assert ts.lengths == [len(want[0])] and ts.clips_used == [want[1]]
            assert float(np.abs(ts.signal(0) - want[0]).max()) <= ac.TOL


def test_a_clip_without_variance_fails_the_call_and_names_the_clip(gpu_ctx, lib):
    from se_snmf_nat_amd import SnmfError, assemble_training_signals
    rs = np.random.RandomState(9)
    ok = ac.plain_clip(rs, 300)
    p = dict(fs=1000, train_seq_len_max=5000, train_file_len_max=0)
    one = np.array([5, 7, 9], np.int16)
    for classes, kw, cls, clip in (
            ([[ok], [ok, one]], dict(ranges=[None, [(1, 300), (2, 2)]]), 1, 1),            # one kept sample: 0 / 0
            ([[ok, np.full(64, 321, np.int16)]], dict(), 0, 1),                             # a constant clip of power-of-two length: var = 0 exactly
            ([[np.full(64, 321.5)], [ok]], dict(), 0, 0)):                                  # the same through the double entry
        with pytest.raises(SnmfError) as e:
            assemble_training_signals(classes, p, ctx=gpu_ctx, **kw)
        assert e.value.status == 1 and f"clip {clip} of class {cls}" in e.value.message, e.value.message
    # behind the stop the reference never looks at a clip: no error
    with assemble_training_signals([[ok, ok, np.full(64, 321, np.int16)]], dict(p, train_seq_len_max=400), ctx=gpu_ctx) as ts:
        assert ts.lengths == [400] and ts.clips_used == [2]
    # and the context still works
    got = assembled(gpu_ctx, "mixed")
    with assemble_training_signals([[ok]], p, ctx=gpu_ctx) as ts:
        assert float(np.abs(ts.signal(0) - ac.normalise(ac.pcm_to_double(ok))).max()) <= ac.TOL
    assert got[0] == [len(s) for s, _, _ in ac.reference("mixed")]


def test_handle_entries_and_refusals_through_ctypes(gpu_ctx, lib):
    from se_snmf_nat_amd import assemble_training_signals
    rs = np.random.RandomState(10)
    with assemble_training_signals([[ac.plain_clip(rs, 100)], [ac.plain_clip(rs, 40), ac.plain_clip(rs, 50)]],
                                   dict(fs=1000, train_seq_len_max=60, train_file_len_max=0), ctx=gpu_ctx) as ts:
        n, length, used = C.c_int32(), np.zeros(2, np.int64), np.zeros(2, np.int32)
        assert lib.snmf_train_signals_info(ts._h, C.byref(n), C.c_void_p(length.ctypes.data), C.c_void_p(used.ctypes.data)) == 0
        assert n.value == 2 and list(length) == [60, 60] == ts.lengths and list(used) == [1, 2] == ts.clips_used
        buf = np.zeros(60)
        assert lib.snmf_train_signals_get_f64(ts._h, 2, C.c_void_p(buf.ctypes.data)) == 3
        assert lib.snmf_train_signals_get_f64(ts._h, -1, C.c_void_p(buf.ctypes.data)) == 3
        assert lib.snmf_train_signals_get_f64(ts._h, 1, None) == 1
        assert lib.snmf_train_signals_get_f64(ts._h, 1, C.c_void_p(buf.ctypes.data)) == 0 and np.abs(buf).max() == 30000.0
    assert ts._h is None
    ts.close()  # (twice is fine)


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_create_and_destroy_fifty_times_returns_all_device_memory(gpu_ctx):
    from se_snmf_nat_amd import assemble_training_signals
    case = ac.case_recordings()

    def cycle():
        with assemble_training_signals(case["classes"], case["p"], vad=case["vad"], ranges=case["ranges"], ctx=gpu_ctx) as ts:
            assert ts.lengths[1] == 114912
    cycle()
    gpu_ctx.sync()
    before = _free_bytes()
    for _ in range(50):
        cycle()
    gpu_ctx.sync()
    after = _free_bytes()
    # the driver hands memory out in 2 MiB granules; a handle's slab is 1 MiB here and anything that leaks shows up 50-fold
    assert before - after < (8 << 20), f"device memory shrank by {(before - after) / 2**20:.1f} MiB over 50 cycles"
