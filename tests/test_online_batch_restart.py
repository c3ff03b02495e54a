"""Restarting streams of the batched online separator (snmf_online_batch_restart / _get_basis_f64 in include/snmf.h,
OnlineBatchSeparator.restart / basis_f64, ntf_sep_event_rt_chains): a stream that finished one recording starts the next
one in place, with a new noise dictionary or with the one it adapted (src/NTF_sep_event_RT.m:27-38, :137-140, run file
after file by run_ntf_sep_RT.m:10-41).  A restarted stream must give the bits a new separator gives, its batch-mates
must not notice, and a chain of files must follow the fp64 oracle (oracle/online_oracle.py) carrying its own dictionary."""
import ctypes as C

import numpy as np
import pytest

from oracle.online_oracle import default_params, ntf_sep_event_rt
from test_online_batch import REL_OUT, REL_OUT_GEN, _decisions, _fixture, _geo_streams, _settings, _streams


def _noisy(n_hops, seed, scale=1.0, noise=200.0):
    """n_hops hops of the fixture audio (tiled) from a seeded offset, plus seeded white noise: enough noise-dominated
    frames that the adaptation triggers often."""
    s, _, _ = _fixture()
    rs = np.random.RandomState(seed)
    n = n_hops * 160
    t = np.tile(s, n // len(s) + 2)
    off = rs.randint(len(s))
    return np.round(t[off:off + n] * scale + rs.randn(n) * noise)


def _file(sep, k, x):
    """Stream k of `sep` runs the whole recording x (the other streams get nothing): outputs, trace, basis."""
    S = sep.S
    pcms = [np.zeros(0)] * S
    pcms[k] = x
    flush = [False] * S
    flush[k] = True
    out = sep.process(pcms, flush)[k]
    return out, sep.trace(k), sep.basis(k)


def _fresh(ctx, x, Bx, Bd, p, H0, Ad, cls=False):
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    sep = OnlineBatchSeparator(Bx, [Bd], p, 1, H0=[H0], Ad_blk0=[Ad], ctx=ctx, class_outputs=cls)
    r = _file(sep, 0, x) + (sep.basis_f64(0),)
    sep.close()
    return r


def _same(a, b, keys=("x_tilde_f", "x_tilde")):
    for key in keys:
        assert np.array_equal(a[0][key], b[0][key]), key
    assert a[1] == b[1]
    assert np.array_equal(a[2], b[2])


def _f32(B):
    return np.asarray(B, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------- CPU ----------------------------------------------
def test_restart_and_chain_arguments_raise_before_any_device_call(monkeypatch):
    """restart() checks streams and shapes, ntf_sep_event_rt_chains its chains, dictionaries and draws, in Python before
    any call reaches the library (here a stand-in whose only working entry is create)."""
    from se_snmf_nat_amd import _lib, online
    from se_snmf_nat_amd.online import OnlineBatchSeparator, ntf_sep_event_rt_chains

    class NoDevice:
        def snmf_online_batch_create(self, *a):
            return 0

        def __getattr__(self, name):
            raise AssertionError(f"reached the device: {name}")

    class Ctx:
        _h = C.c_void_p(1)
        _plans = set()

    monkeypatch.setattr(_lib, "load", lambda *a, **k: NoDevice())
    monkeypatch.setattr(online, "default_context", lambda *a, **k: Ctx())
    _, Bx, Bd = _fixture()
    p = _settings(default_params())
    sep = OnlineBatchSeparator(Bx, Bd, p, 3)
    for args, kw in (((3,), {}), ((-1,), {}), (([0, 0],), {}), (([0, 3],), {}),
                     ((0,), dict(B_DFT_d=Bd[:-1])),
                     ((0,), dict(B_DFT_d=Bd[:, :50])),
                     (([0, 1],), dict(B_DFT_d=[Bd])),
                     (([0, 1],), dict(B_DFT_d=[Bd, Bd, Bd])),
                     ((1,), dict(H0=np.ones(199))),
                     (([1, 2],), dict(H0=[np.ones(200)])),
                     ((2,), dict(Ad_blk0=np.ones((50, 99)))),
                     (([0, 2],), dict(Ad_blk0=[np.ones((50, 100)), np.ones((100, 50))]))):
        with pytest.raises(_lib.SnmfError) as e:
            sep.restart(*args, **kw)
        assert e.value.status == 1, (args, kw)  # SNMF_ERR_INVALID
    sep._h = None

    def no_device(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(online, "default_context", no_device)
    s, _, _ = _fixture()
    chains = [[s[:800], s[:320]], [s[:480]]]
    for kw in (dict(B_DFT_d=[Bd]), dict(B_DFT_d=Bd[:-1]), dict(B_DFT_d=[Bd, Bd[:, :50]]), dict(H0=[np.ones(200)] * 3),
               dict(H0=np.ones(201)), dict(Ad_blk0=[np.ones((50, 100)), np.ones((50, 10))]), dict(n_streams=0)):
        args = dict(B_DFT_d=Bd)
        args.update(kw)
        with pytest.raises(_lib.SnmfError) as e:
            ntf_sep_event_rt_chains(chains, Bx, args.pop("B_DFT_d"), p, **args)
        assert e.value.status == 1, kw
    assert ntf_sep_event_rt_chains([], Bx, Bd, p) == []


# ---------------------------------------------------------------- GPU ----------------------------------------------
@pytest.mark.gpu
def test_restart_equals_a_fresh_stream(gpu_ctx):
    """Slot 1 runs a recording long enough that the rings fill (more pushes than m_a), the adaptation runs, and
    update_switch and the overlap-add tails (class outputs included) move.  Restarted, its next recording is bit for bit
    what a new S = 1 batch gives: with an explicit dictionary, H0 and Ad_blk0, and with NULL H0 / Ad_blk0 (the values
    the stream last started with).  (Explicit dictionaries are fp32 values here: creation takes fp32.)"""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = _settings(default_params())
    _, Bx, Bds, H0s, Ads = _streams(10, S=3, seed=21)
    x0, x1, y, z = _noisy(300, 1), _noisy(320, 2), _noisy(70, 3, 0.7), _noisy(50, 4, 1.3, 50.0)
    sep = OnlineBatchSeparator(Bx, Bds[:2], p, 2, H0=H0s[:2], Ad_blk0=Ads[:2], ctx=gpu_ctx, class_outputs=True)
    out = sep.process([x0, x1], flush=True)
    tr = sep.trace(1)
    assert sum(t["trig"] for t in tr) > p["m_a"] and sum(t["solved"] for t in tr) >= 2
    keys = ("x_tilde_f", "x_tilde", "x_hat", "d_hat")
    # explicit dictionary, H0, Ad_blk0
    Bn = _f32(Bds[2])
    sep.restart(1, B_DFT_d=Bn, H0=H0s[2], Ad_blk0=Ads[2])
    got = _file(sep, 1, y) + (sep.basis_f64(1),)
    ref = _fresh(gpu_ctx, y, Bx, Bn, p, H0s[2], Ads[2], cls=True)
    _same(got, ref, keys)
    assert np.array_equal(got[3], ref[3])
    assert sum(t["solved"] for t in ref[1]) > 0
    # NULL H0 / Ad_blk0: the values of the last start (the restart above), here with a new dictionary
    sep.restart([1], B_DFT_d=[_f32(Bds[0])])
    _same(_file(sep, 1, z), _fresh(gpu_ctx, z, Bx, Bds[0], p, H0s[2], Ads[2], cls=True)[:3], keys)
    # slot 0, restarted for the first time: the creation values
    sep.restart(0, B_DFT_d=_f32(Bds[1]))
    _same(_file(sep, 0, y), _fresh(gpu_ctx, y, Bx, Bds[1], p, H0s[0], Ads[0], cls=True)[:3], keys)
    sep.close()


@pytest.mark.gpu
def test_carry_keeps_the_fp64_master(gpu_ctx):
    """A carried dictionary (restart with B_DFT_d = None) is the fp64 master: batch A carries it from file 1 to file 2;
    batch B, never fed, restarts with A.basis_f64(0) taken after file 1.  File 2 is bit-identical in both.  (k_obassemble
    reads the fixed columns for j >= R_a only, and after an adaptation those columns of the dictionary are exact copies
    of them, so B's new fixed columns change nothing.)"""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = _settings(default_params())
    _, Bx, Bds, H0s, Ads = _streams(10, S=2, seed=22)
    x1, x2 = _noisy(150, 5), _noisy(90, 6, 0.8)
    A = OnlineBatchSeparator(Bx, Bds[:1], p, 1, H0=H0s[:1], Ad_blk0=Ads[:1], ctx=gpu_ctx)
    _, tr1, b32 = _file(A, 0, x1)
    assert sum(t["solved"] for t in tr1) > 0
    Bc = A.basis_f64(0)
    assert np.array_equal(b32, Bc.astype(np.float32).astype(np.float64))
    assert not np.array_equal(Bc, b32)  # the fp32 mirror would lose bits
    A.restart(0)
    ra = _file(A, 0, x2)
    B = OnlineBatchSeparator(Bx, Bds[1:2], p, 1, H0=H0s[:1], Ad_blk0=Ads[:1], ctx=gpu_ctx)
    B.restart(0, B_DFT_d=Bc)
    rb = _file(B, 0, x2)
    _same(ra, rb)
    assert np.array_equal(A.basis_f64(0), B.basis_f64(0))
    A.close()
    B.close()


@pytest.mark.gpu
def test_batch_mates_are_untouched(gpu_ctx):
    """Slots 1 and 3 finish short recordings and restart (one new dictionary, one carry) while 0, 2 and 4 are in the
    middle of theirs: the bits of 0, 2 and 4 equal a run without restarts."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = _settings(default_params())
    pcms, Bx, Bds, H0s, Ads = _streams(40, S=5, seed=23)
    pcms[1], pcms[3] = pcms[1][:800], pcms[3][:1200]
    whole = OnlineBatchSeparator(Bx, Bds, p, 5, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    ref = whole.process(pcms, flush=True)
    ref_tr = [whole.trace(k) for k in range(5)]
    ref_b = [whole.basis_f64(k) for k in range(5)]
    whole.close()
    sep = OnlineBatchSeparator(Bx, Bds, p, 5, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    acc = [[] for _ in range(5)]
    e = np.zeros(0)
    cut = 2400
    outs = sep.process([pcms[0][:cut], pcms[1], pcms[2][:cut], pcms[3], pcms[4][:cut]], [False, True, False, True, False])
    for k in (0, 2, 4):
        acc[k].append(outs[k]["x_tilde_f"])
    sep.restart([3, 1], B_DFT_d=[Bds[0], Bds[4]])
    sep.process([e, pcms[2][:700], e, pcms[0][:900], e])
    sep.process([e, e, e, e, e], [False, True, False, True, False])
    sep.restart(1)
    outs = sep.process([pcms[0][cut:], pcms[4][:500], pcms[2][cut:], e, pcms[4][cut:]], [True, True, True, False, True])
    for k in (0, 2, 4):
        acc[k].append(outs[k]["x_tilde_f"])
        assert np.array_equal(np.concatenate(acc[k]), ref[k]["x_tilde_f"])
        assert sep.trace(k) == ref_tr[k]
        assert np.array_equal(sep.basis_f64(k), ref_b[k])
    sep.close()


def _chain_vs_oracle(ctx, p, geo=None):
    """A 3-file chain on slot 0 of a batch of 2 (slot 1 finished a recording first), the dictionary carried on the device.
    Per file, the device against two oracle runs: one started from the device's carried fp64 dictionary ("file") and
    the chain the oracle carries itself ("chain").  Returns per (file, kind): the frames whose decisions differ, the
    relative error of x_tilde_f and of the final B_DFT_d, and the largest int16 difference.  `geo`: the shipped
    transform and dictionaries, else a tests/test_online.py geometry (test_online_batch._geo_streams)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    if geo is None:
        pcms, Bx, Bds, H0s, Ads = _streams(40, S=2, seed=24)
        files = [pcms[0], _noisy(38, 7, 0.6, 80.0), _noisy(36, 8, 1.1, 120.0)]
    else:
        p, files, Bx, Bds, H0s, Ads = _geo_streams(geo, 36, S=3, seed=24)
        pcms = [None, files[1][:5 * p["frameshift"]]]
    sep = OnlineBatchSeparator(Bx, Bds[:2], _settings(p), 2, H0=H0s[:2], Ad_blk0=Ads[:2], ctx=ctx)
    sep.process([np.zeros(0), pcms[1]], [False, True])  # company that finished
    B_dev, B_orc = Bds[0], Bds[0]
    rows, solved = [], 0
    for i, x in enumerate(files):
        if i:
            sep.restart(0)
        out, tr, Bn = _file(sep, 0, x)
        solved += sum(t["solved"] for t in tr)
        chain = None
        for kind, B0 in (("file", B_dev), ("chain", B_orc)):
            ref = ntf_sep_event_rt(x, Bx, B0, p, H0s[0], Ads[0], return_trace=True)
            o16, of, Bdn, rtr = ref[:4]
            dd, dr = _decisions(tr), _decisions(rtr)
            diff = sorted({j for u, v in zip(dd, dr) for j in range(max(len(u), len(v))) if u[j:j + 1] != v[j:j + 1]})
            dev = out["x_tilde_f"]
            assert len(dev) == len(of) and np.isfinite(dev).all()
            rows.append(dict(file=i, kind=kind, n_frames=len(tr), diff=diff, rel_out=np.linalg.norm(dev - of) / np.linalg.norm(of),
                             rel_B=np.linalg.norm(Bn - Bdn) / np.linalg.norm(Bdn),
                             i16=int(np.abs(out["x_tilde"].astype(int) - o16.astype(int)).max(initial=0))))
            if kind == "chain":
                chain = Bdn
        B_dev, B_orc = sep.basis_f64(0), chain
    sep.close()
    assert solved > 0
    return rows


# The chain the oracle carries itself drifts from the device's: each file's adaptation amplifies the start dictionary's
# difference (3.4e-5 after file 1 on the MI355X, 7.9e-4 after file 2), and in file 3 the decisions part (11 of 40
# frames).  So the whole chain is checked over its first two files, x_tilde_f within REL_OUT_CHAIN (measured: 1.07e-4
# in file 2); every file is checked against the oracle started from the dictionary the device carried.
REL_OUT_CHAIN = 2e-4
# beta = 1.5 at test_online_batch.py's WADAPT_CASES transform and ring (R_a = m_a = 72): at the shipped 50 x 100 ring an
# all-zero flush frame's trigger moves with fp32 rounding at the 1e-9 floor, and the solve it starts moves the final
# dictionary by 35 % (measured; the same cancellation tests/test_online_batch.py's generic-beta notes describe)
GEO_BETA15 = (1024, 640, 160, 72, 128, dict(overlap_m_a=0.05, Ar_up=2.0, sparsity=1.0, R_a=72, m_a=72, cf="x", beta_div=1.5,
                                              conv_eps=0.0, max_iter=30))


def _check_chain(rows, tol, tol_chain):
    for r in rows:
        if r["kind"] == "chain" and r["file"] >= 2:
            continue
        bound = tol if r["kind"] == "file" else tol_chain
        assert r["diff"] == [], r
        assert r["rel_out"] < bound and r["rel_B"] < 10 * bound, r


@pytest.mark.gpu
def test_chain_matches_the_oracle_file_by_file_and_whole(gpu_ctx):
    """A 3-file chain with the shipped settings (adaptation on): every file against the oracle started from the device's
    carried fp64 dictionary within REL_OUT (measured: 2.4e-6), the first two against the oracle that carries its own
    within REL_OUT_CHAIN, all with equal decision traces."""
    rows = _chain_vs_oracle(gpu_ctx, default_params())
    _check_chain(rows, REL_OUT, REL_OUT_CHAIN)
    assert all(r["i16"] <= 1 for r in rows if r["kind"] == "file")


@pytest.mark.gpu
def test_chain_matches_the_oracle_generic_beta(gpu_ctx):
    """beta = 1.5 (k_hsolve_frame / k_wadapt_batch BM_GEN) with adaptation, without a stop test as the other generic-beta
    variants (GEO_BETA15): every file within tests/test_online_batch.py's REL_OUT_GEN (measured: 8.0e-7), the first two
    of the oracle's own chain within REL_OUT_CHAIN (measured: 2.2e-5), equal decision traces."""
    _check_chain(_chain_vs_oracle(gpu_ctx, default_params(), geo=GEO_BETA15), REL_OUT_GEN, REL_OUT_CHAIN)


def _uneven_chains():
    s, _, _ = _fixture()
    rs = np.random.RandomState(25)
    lens = [[31, 12, 26], [8], [17, 0, 22], [40, 9], [5, 28, 3, 15]]  # hops; chain 2 holds an empty file
    chains = []
    for c, ls in enumerate(lens):
        files = []
        for i, n in enumerate(ls):
            m = n * 160 + (37 * (c + i)) % 160
            if n == 0:
                m = 0
            files.append(np.round(_noisy(n + 2, 100 + 10 * c + i, 0.5 + 0.2 * c, 40.0 + 30 * i)[:m]))
        chains.append(files)
    return chains


@pytest.mark.gpu
def test_chain_driver_does_not_depend_on_scheduling(gpu_ctx):
    """Five uneven chains (one with an empty file): identical bits for n_streams 1, 2, 5 and two chunk_hops values; one-
    file chains with n_streams = len(chains) equal ntf_sep_event_rt_batch bit for bit."""
    from se_snmf_nat_amd.online import ntf_sep_event_rt_batch, ntf_sep_event_rt_chains
    p = _settings(default_params())
    _, Bx, Bds, _, _ = _streams(10, S=5, seed=26)
    chains = _uneven_chains()
    base = ntf_sep_event_rt_chains(chains, Bx, Bds, p, ctx=gpu_ctx)
    assert [len(r) for r in base] == [len(c) for c in chains]
    assert len(base[2][1][0]) == len(base[2][1][1])
    for n_streams in (1, 2, 5):
        for hops in (None, 7):
            if n_streams == 5 and hops is None:
                continue
            got = ntf_sep_event_rt_chains(chains, Bx, Bds, p, n_streams=n_streams, chunk_hops=hops, ctx=gpu_ctx)
            for rc, gc in zip(base, got):
                for a, b in zip(rc, gc):
                    assert all(np.array_equal(u, v) for u, v in zip(a, b)), (n_streams, hops)
    pcms = [c[0] for c in chains]
    one = ntf_sep_event_rt_chains([[x] for x in pcms], Bx, Bds, p, n_streams=len(pcms), ctx=gpu_ctx)
    bat = ntf_sep_event_rt_batch(pcms, Bx, Bds, p, ctx=gpu_ctx)
    for (a,), b in zip(one, bat):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.gpu
def test_restart_error_codes(gpu_ctx):
    """Mid-file restart: SNMF_ERR_STATE, and the stream runs on unchanged; slots out of range, listed twice or a negative
    count: SNMF_ERR_INVALID from the C entry; feeding a flushed stream without a restart: SNMF_ERR_STATE."""
    from se_snmf_nat_amd import _lib
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = _settings(default_params())
    pcms, Bx, Bds, H0s, Ads = _streams(30, S=2, seed=27)
    ref = OnlineBatchSeparator(Bx, Bds, p, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    want = ref.process(pcms, flush=True)
    want_tr = ref.trace(0)
    ref.close()
    sep = OnlineBatchSeparator(Bx, Bds, p, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    sep.restart([0, 1])  # never fed: allowed
    parts = [sep.process([pcms[0][:1000], pcms[1][:100]])[0]["x_tilde_f"]]
    for k in (0, 1, [1, 0]):  # 0 has consumed hops, 1 holds a partial hop
        with pytest.raises(_lib.SnmfError) as e:
            sep.restart(k)
        assert e.value.status == 7
    lib = _lib.load()
    for n, sl in ((1, [2]), (1, [-1]), (2, [1, 1]), (-1, [0]), (3, [0, 1, 0])):
        arr = np.array(sl, dtype=np.int32)
        assert lib.snmf_online_batch_restart(sep._h, n, arr.ctypes.data, None, None, None) == 1, sl
    outs = sep.process([pcms[0][1000:], pcms[1][100:]], flush=True)
    parts.append(outs[0]["x_tilde_f"])
    assert np.array_equal(np.concatenate(parts), want[0]["x_tilde_f"]) and sep.trace(0) == want_tr
    assert np.array_equal(outs[1]["x_tilde_f"], want[1]["x_tilde_f"])
    for flush in (False, True):
        with pytest.raises(_lib.SnmfError) as e:
            sep.process([pcms[0][:160], np.zeros(0)], flush=[flush, False])
        assert e.value.status == 7
    with pytest.raises(_lib.SnmfError) as e:
        sep.process([np.zeros(0), np.zeros(0)], flush=[True, False])
    assert e.value.status == 7
    sep.restart(0, B_DFT_d=_f32(Bds[0]))  # (a carry would start from the adapted dictionary)
    assert np.array_equal(sep.process([pcms[0], np.zeros(0)], flush=[True, False])[0]["x_tilde_f"], want[0]["x_tilde_f"])
    sep.close()


@pytest.mark.gpu
def test_restart_with_more_streams_than_cus(gpu_ctx):
    """S = 300: every stream finishes a short recording, all restart at once with new dictionaries, H0 and Ad_blk0 (one
    k_obrestart over 300 streams), and each second recording equals a new S = 1 batch's."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p = _settings(default_params())
    pcms, Bx, Bds, H0s, Ads = _streams(12, S=3, seed=28)
    pcms = [x[:12 * 160] for x in pcms]
    S = 300
    sep = OnlineBatchSeparator(Bx, [Bds[k % 3] for k in range(S)], p, S, H0=[H0s[k % 3] for k in range(S)],
                               Ad_blk0=[Ads[k % 3] for k in range(S)], ctx=gpu_ctx)
    sep.process([pcms[k % 3] for k in range(S)], flush=True)
    j = [(k + 1) % 3 for k in range(S)]
    sep.restart(list(range(S))[::-1], B_DFT_d=[_f32(Bds[j[k]]) for k in range(S)][::-1], H0=[H0s[j[k]] for k in range(S)][::-1],
                Ad_blk0=[Ads[j[k]] for k in range(S)][::-1])
    ys = [pcms[(k + 2) % 3] for k in range(S)]
    outs = sep.process(ys, flush=True)
    singles = {}
    for k in range(S):
        key = (j[k], (k + 2) % 3)
        if key not in singles:
            singles[key] = _fresh(gpu_ctx, ys[k], Bx, Bds[j[k]], p, H0s[j[k]], Ads[j[k]])
        a = singles[key]
        assert np.array_equal(outs[k]["x_tilde_f"], a[0]["x_tilde_f"]) and np.array_equal(outs[k]["x_tilde"], a[0]["x_tilde"])
        assert sep.trace(k) == a[1]
        assert np.array_equal(sep.basis(k), a[2])
    sep.close()
