"""Settings and an event dictionary per stream in the fp64 batched online separator (snmf_online_batch_create_streams_f64 /
_restart_streams_f64 / _get_settings; OnlineBatchSeparator(settings=[...], B_DFT_x=[...]); the per-stream settings table of
csrc/snmf_online_batch_f64.h).

The yardstick is the batch of one made through the interface that was there before, OnlineBatchSeparator(Bx_k, Bd_k, p_k, 1,
precision="fp64"): stream k of a mixed batch must give its bits -- signals, class outputs, trace, final B_DFT_d -- whatever the
other streams run, whichever slot it has and however it is fed.  Against the oracle the module keeps the bounds of
tests/test_online_batch_f64.py (FIX_OVERALL, FIX_BASIS, every decision equal).

Geometry: GEO_CASES[0] of tests/test_online_batch_f64.py (fftlength 128, frame 100, hop 25, R_x 16, R_d 20, ring 8 x 12, 36 hops):
every stream crosses the row-block remainder (F = 65), the ring wrap and the adaptation trigger; one test runs the shipped
geometry.  Every test prints its figures before it asserts (pytest -s).

Not tested, because it cannot be built: "a ring inside the KL budget but outside the beta != 1 budget".  No such ring exists: with
R_a <= 64 and m_a <= 128 the beta != 1 image is at most 159120 bytes <= 163840 (wbatch64_lds), and beyond R_a = 64 / m_a = 128
every class is refused.  What can be shown of the per-class check is shown instead: a ring outside the envelope is refused
only when a stream adapts, and the refusal reports the LDS of the class that adapts.
"""
import ctypes as C
import re

import numpy as np
import pytest

from test_online_batch import _geo_streams
from test_online_batch_f64 import FIX_BASIS, FIX_OVERALL, GEO_CASES, HOP, KB, KEYS, _judge, _oracle, _run_batch, _settings, _streams, wbatch64_lds

pytestmark = pytest.mark.gpu

GEO, N_HOPS = GEO_CASES[0]
# shipped, Wiener, no adaptation, ED with sparsity 50, no stop test with 12 iterations, generic beta
SETTINGS = [dict(), dict(ENHANCE_METHOD="Wiener"), dict(adapt_train_N=0), dict(cf="ed", sparsity=50.0), dict(conv_eps=0.0, max_iter=12),
            dict(cf="x", beta_div=1.5)]
# the generic-beta stream is fed without the flush and judged on its signal frames, as tests/test_online_batch_f64.py's VARIANTS
FLUSH = [True, True, True, True, True, False]
BX_OF = [0, 1, 0, 1, 1, 0]  # which of the two event dictionaries a stream has
SEEDS = (11, 23)


def _setup():
    """S = 6 streams of the small geometry: two draws of _geo_streams (signals, lengths, H0 / Ad_blk0 and noise dictionaries all
    differ), two event dictionaries (the second: the first's columns permuted and rescaled)."""
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(GEO, N_HOPS, S=3, seed=SEEDS[0])
    _, pcms2, _, Bds2, H0s2, Ads2 = _geo_streams(GEO, N_HOPS, S=3, seed=SEEDS[1])
    rs = np.random.RandomState(5)
    Bx2 = Bx[:, rs.permutation(Bx.shape[1])] * (1.0 + 0.3 * rs.random_sample(Bx.shape))
    return p, pcms + pcms2, [Bx, Bx2], Bds + Bds2, H0s + H0s2, Ads + Ads2


def _run_mixed(ctx, data, order=None, feed=None, settings=SETTINGS, bx_of=BX_OF, flush=FLUSH):
    """The streams order[...] of `data` as ONE batch with settings and B_x per stream -> per stream (outputs, trace, basis)."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p, pcms, Bxs, Bds, H0s, Ads = data
    order = list(range(len(pcms))) if order is None else order
    sep = OnlineBatchSeparator([Bxs[bx_of[i]] for i in order], [Bds[i] for i in order], _settings(p), len(order), H0=[H0s[i] for i in order],
                               Ad_blk0=[Ads[i] for i in order], ctx=ctx, class_outputs=True, precision="fp64",
                               settings=[settings[i] for i in order])
    keys = ["x_tilde", "x_tilde_f", "x_hat", "d_hat"]
    acc = [{k: [] for k in keys} for _ in order]
    for chunk_list, fl in (feed if feed is not None else [([pcms[i] for i in order], [flush[i] for i in order])]):
        for a, o in zip(acc, sep.process(chunk_list, flush=fl)):
            for k in keys:
                a[k].append(o[k])
    res = [({key: np.concatenate(acc[j][key]) for key in keys}, sep.trace(j), sep.basis(j)) for j in range(len(order))]
    sets = [sep.settings(j) for j in range(len(order))]
    sep.close()
    return res, sets


def _single(ctx, data, i, settings=SETTINGS, bx_of=BX_OF, flush=FLUSH):
    """Stream i as a batch of one through the interface that has no settings list."""
    p, pcms, Bxs, Bds, H0s, Ads = data
    return _run_batch(ctx, [pcms[i]], Bxs[bx_of[i]], [Bds[i]], dict(p, **settings[i]), [H0s[i]], [Ads[i]], class_outputs=True, flush=flush[i])[0]


def _same(a, b, label=""):
    for key in ("x_tilde_f", "x_tilde", "x_hat", "d_hat"):
        assert a[0][key].dtype == b[0][key].dtype and np.array_equal(a[0][key], b[0][key], equal_nan=True), (label, key)
    assert len(a[1]) == len(b[1]), (label, "trace")
    for i, (ta, tb) in enumerate(zip(a[1], b[1])):  # (a silent flush frame has beta = NaN on both sides: NaN equals NaN here)
        assert ta.keys() == tb.keys() and all(ta[k] == tb[k] or (ta[k] != ta[k] and tb[k] != tb[k]) for k in ta), (label, "trace", i + 1)
    assert np.array_equal(a[2], b[2]), (label, "B_DFT_d")


@pytest.fixture(scope="module")
def data():
    return _setup()


@pytest.fixture(scope="module")
def mixed(gpu_ctx, data):
    """The six streams as one mixed batch, once."""
    res, sets = _run_mixed(gpu_ctx, data)
    return res, sets


@pytest.fixture(scope="module")
def singles(gpu_ctx, data):
    return [_single(gpu_ctx, data, i) for i in range(len(SETTINGS))]


def test_mixed_batch_equals_batches_of_one_bit_for_bit(mixed, singles):
    res, sets = mixed
    solved = [sum(t["solved"] for t in r[1]) for r in res]
    print("mixed batch of %d: solves per stream %s, frames %s" % (len(res), solved, [len(r[1]) for r in res]))
    for i in range(len(SETTINGS)):
        _same(res[i], singles[i], "stream %d %s" % (i, SETTINGS[i]))
    assert solved[2] == 0 and not any(t["trig"] for t in res[2][1])  # the stream that does not adapt never triggers
    assert sum(1 for i in (0, 1, 3, 4, 5) if solved[i] > 0) >= 3
    assert sets[1]["enhance_method"] == 0 and sets[0]["enhance_method"] == 1 and sets[2]["adapt_train_N"] == 0
    assert sets[3]["beta_div"] == 2.0 and sets[3]["sparsity"] == 50.0 and sets[5]["beta_div"] == 1.5
    assert sets[4]["conv_eps"] == 0.0 and sets[4]["max_iter"] == 12 and sets[0]["overlap_m_a"] == GEO[5]["overlap_m_a"]


def test_mixed_batch_streams_hold_their_oracle_runs(data, mixed):
    p, pcms, Bxs, Bds, H0s, Ads = data
    res, _ = mixed
    classes = set()
    for i, var in enumerate(SETTINGS):
        pk = dict(p, **var)
        ref = _oracle(pcms[i], Bxs[BX_OF[i]], Bds[i], pk, H0s[i], Ads[i])
        n_fr = None
        if not FLUSH[i]:
            n_fr = len(pcms[i]) // GEO[2]
            assert not any(int(t["trig"]) for t in ref[3][n_fr:])  # the oracle's dictionary after the last signal frame is its final one
        n_solves = sum(int(t["adapt_iters"] > 0) for t in ref[3])
        if n_solves:
            classes.add("kl" if pk["cf"] == "kl" else "ed" if pk["cf"] == "ed" else "gen")
        _judge("mixed stream %d %s" % (i, var), *res[i], ref, n_fr=n_fr)
    print("oracle adaptation solves in the divergence classes", sorted(classes))
    assert len(classes) >= 2  # the oracle alone runs adaptation solves in at least two divergence classes


def test_bits_do_not_depend_on_company_slot_or_feeding(gpu_ctx, data, mixed, singles):
    res, _ = mixed  # (company: test_mixed_batch_equals_batches_of_one_bit_for_bit holds every stream alone against the six)
    pcms = data[1]
    order = [4, 2, 5, 0, 3, 1]  # another slot, other neighbours
    perm, _ = _run_mixed(gpu_ctx, data, order=order)
    for j, i in enumerate(order):
        _same(perm[j], res[i], "slot %d <- stream %d" % (j, i))
    S, sizes, pos, feed, rnd = len(pcms), [160, 1000, 57, 160, 57, 1000], [0] * len(pcms), [], 0  # 160- / 1000- / 57-sample chunks
    while any(pos[k] < len(pcms[k]) for k in range(S)):
        chunk = []
        for k in range(S):
            if (rnd + k) % 4 == 3:  # some streams get nothing in some calls
                chunk.append(pcms[k][:0])
                continue
            chunk.append(pcms[k][pos[k]:pos[k] + sizes[k]])
            pos[k] += sizes[k]
        feed.append((chunk, False))
        rnd += 1
    feed.append(([x[:0] for x in pcms], [FLUSH[k] and k % 2 == 1 for k in range(S)]))  # staggered flushes
    feed.append(([x[:0] for x in pcms], [FLUSH[k] and k % 2 == 0 for k in range(S)]))
    fed, _ = _run_mixed(gpu_ctx, data, feed=feed)
    for k in range(S):
        _same(fed[k], res[k], "fed in chunks, stream %d" % k)


def test_uniform_settings_given_as_lists_are_the_uniform_call(gpu_ctx, data):
    p, pcms, Bxs, Bds, H0s, Ads = data
    for var in (dict(), dict(cf="ed", sparsity=50.0)):
        pk = dict(p, **var)
        uni = _run_batch(gpu_ctx, pcms[:3], Bxs[0], Bds[:3], pk, H0s[:3], Ads[:3], class_outputs=True)
        # once as overrides on the shipped settings, once as empty overrides on the variant's own dict
        a, _ = _run_mixed(gpu_ctx, data, order=[0, 1, 2], settings=[var] * 3, bx_of=[0] * 3, flush=[True] * 3)
        b, _ = _run_mixed(gpu_ctx, (pk,) + tuple(data[1:]), order=[0, 1, 2], settings=[{}] * 3, bx_of=[0] * 3, flush=[True] * 3)
        assert sum(t["solved"] for r in uni for t in r[1]) > 0
        for k in range(3):
            _same(a[k], uni[k], "list of equal settings, stream %d" % k)
            _same(b[k], uni[k], "list of empty overrides, stream %d" % k)


def _file(sep, k, x, S, flush=True):
    pcms = [x[:0]] * S
    pcms[k] = x
    fl = [False] * S
    fl[k] = flush
    o = sep.process(pcms, flush=fl)[k]
    return ({key: o[key] for key in ("x_tilde", "x_tilde_f", "x_hat", "d_hat")}, sep.trace(k), sep.basis(k))


def test_restart_with_another_dictionary_and_other_settings(gpu_ctx, data, singles):
    """Slot 0 goes from no adaptation to the shipped settings (off -> on) and another B_x, slot 1 from KL to ED; then a batch of
    ONE that never adapted (no ring allocated) turns adaptation on.  Each restarted file equals a fresh batch of one."""
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    p, pcms, Bxs, Bds, H0s, Ads = data
    sep = OnlineBatchSeparator([Bxs[0], Bxs[1]], [Bds[2], Bds[1]], _settings(p), 2, H0=[H0s[2], H0s[1]], Ad_blk0=[Ads[2], Ads[1]], ctx=gpu_ctx,
                               class_outputs=True, precision="fp64", settings=[SETTINGS[2], SETTINGS[1]])
    first = sep.process([pcms[2], pcms[1]], flush=True)
    assert np.array_equal(first[0]["x_tilde_f"], singles[2][0]["x_tilde_f"]) and np.array_equal(first[1]["x_tilde_f"], singles[1][0]["x_tilde_f"])
    with pytest.raises(SnmfError) as e:  # a shared key in a restart's entry: refused on the host, the batch untouched
        sep.restart(0, settings=dict(R_a=4))
    assert e.value.status == 1
    sep.restart([0, 1], B_DFT_d=[Bds[4], Bds[3]], H0=[H0s[4], H0s[3]], Ad_blk0=[Ads[4], Ads[3]], B_DFT_x=[Bxs[1], Bxs[1]],
                settings=[SETTINGS[4], SETTINGS[3]])
    assert sep.settings(0)["adapt_train_N"] == 1 and sep.settings(0)["max_iter"] == 12 and sep.settings(1)["beta_div"] == 2.0
    outs = sep.process([pcms[4], pcms[3]], flush=True)
    got = [({key: outs[j][key] for key in ("x_tilde", "x_tilde_f", "x_hat", "d_hat")}, sep.trace(j), sep.basis(j)) for j in range(2)]
    sep.close()
    _same(got[0], singles[4], "slot 0: off -> on, new B_x")
    _same(got[1], singles[3], "slot 1: KL -> ED")
    assert sum(t["solved"] for t in got[0][1]) > 0 and sum(t["solved"] for t in got[1][1]) > 0
    # a batch of one created without any adapting stream: the rings come with the restart
    one = OnlineBatchSeparator([Bxs[0]], [Bds[2]], _settings(p), 1, H0=[H0s[2]], ctx=gpu_ctx, class_outputs=True, precision="fp64",
                               settings=[SETTINGS[2]])
    _same(_file(one, 0, pcms[2], 1), singles[2], "one stream, no adaptation")
    with pytest.raises(SnmfError) as e:  # adaptation on, and no Ad_blk0 was ever given
        one.restart(0, settings=SETTINGS[0])
    assert e.value.status == 1
    one.restart(0, B_DFT_d=Bds[0], H0=H0s[0], Ad_blk0=Ads[0], settings=SETTINGS[0])
    _same(_file(one, 0, pcms[0], 1), singles[0], "one stream, off -> on")
    one.restart(0, B_DFT_d=Bds[3], H0=H0s[3], Ad_blk0=Ads[3], B_DFT_x=Bxs[1], settings=SETTINGS[3])  # and KL -> ED: P comes with it
    _same(_file(one, 0, pcms[3], 1), singles[3], "one stream, KL -> ED")
    one.close()


def test_chains_with_settings_per_chain_do_not_depend_on_the_slots(gpu_ctx, data):
    from se_snmf_nat_amd.online import ntf_sep_event_rt_chains
    p, pcms, Bxs, Bds, H0s, Ads = data
    chains = [[pcms[0], pcms[1]], [pcms[3], pcms[2]]]
    kw = dict(H0=[H0s[0], H0s[3]], Ad_blk0=[Ads[0], Ads[3]], ctx=gpu_ctx, precision="fp64", settings=[SETTINGS[0], SETTINGS[3]])
    runs = [ntf_sep_event_rt_chains(chains, [Bxs[0], Bxs[1]], [Bds[0], Bds[3]], _settings(p), n_streams=n, **kw) for n in (2, 1)]
    for c in range(2):
        for i in range(2):
            for a, b in zip(runs[0][c][i], runs[1][c][i]):
                assert np.array_equal(a, b), (c, i)
    # each chain's first file is its batch of one (x_tilde, x_tilde_f, final B_DFT_d)
    for c, k in ((0, 0), (1, 3)):
        ref = _single(gpu_ctx, data, k)
        d16, df, dB = runs[0][c][0]
        assert np.array_equal(d16, ref[0]["x_tilde"]) and np.array_equal(df, ref[0]["x_tilde_f"]) and np.array_equal(dB, ref[2])
    # the two chains really ran different things: the second chain's first file under the first chain's settings differs
    other = ntf_sep_event_rt_chains([[pcms[3]]], Bxs[1], Bds[3], _settings(p), H0=H0s[3], Ad_blk0=Ads[3], ctx=gpu_ctx, precision="fp64")
    assert not np.array_equal(other[0][0][1], runs[0][1][0][1])


def test_shipped_geometry_once(gpu_ctx):
    """F = 513, r = 200, the 50 x 100 ring, S = 3: KL, ED and a stream that does not adapt, about 30 hops."""
    from oracle.online_oracle import default_params
    p = default_params()
    pcms, Bx, Bds, H0s, Ads = _streams([30 * HOP, 27 * HOP + 57, 28 * HOP], seed=7)
    rs = np.random.RandomState(3)
    Bx2 = Bx[:, rs.permutation(Bx.shape[1])] * (1.0 + 0.2 * rs.random_sample(Bx.shape))
    sets = [dict(), dict(cf="ed", sparsity=50.0, alpha_eta=0.5, alpha_d=0.7, beta=2.0), dict(adapt_train_N=0, ENHANCE_METHOD="Wiener")]
    d = (p, pcms, [Bx, Bx2], Bds, H0s, Ads)
    res, got = _run_mixed(gpu_ctx, d, settings=sets, bx_of=[0, 1, 1], flush=[True] * 3)
    solved = [sum(t["solved"] for t in r[1]) for r in res]
    print("shipped geometry: solves per stream", solved)
    for k in range(3):
        _same(res[k], _single(gpu_ctx, d, k, settings=sets, bx_of=[0, 1, 1], flush=[True] * 3), "shipped geometry, stream %d" % k)
    assert solved[0] > 0 and solved[1] > 0 and solved[2] == 0
    # snmf_online_batch_get_settings returns what was set
    from se_snmf_nat_amd.online import default_settings
    ds = default_settings()
    want = [dict(beta_div=1.0, sparsity=float(ds["sparsity"]), enhance_method=1, adapt_train_N=1, alpha_eta=ds["alpha_eta"], alpha_d=ds["alpha_d"],
                 beta=ds["beta"]),
            dict(beta_div=2.0, sparsity=50.0, enhance_method=1, adapt_train_N=1, alpha_eta=0.5, alpha_d=0.7, beta=2.0),
            dict(beta_div=1.0, sparsity=float(ds["sparsity"]), enhance_method=0, adapt_train_N=0, alpha_eta=ds["alpha_eta"], alpha_d=ds["alpha_d"],
                 beta=ds["beta"])]
    for k in range(3):
        for key, v in want[k].items():
            assert got[k][key] == v, (k, key)
        for key in ("conv_eps", "max_iter", "init_N_len", "beta_max", "blk_sparse", "P_len_k", "blk_gap", "alpha_p", "overlap_m_a", "Ar_up"):
            assert got[k][key] == ds[key], (k, key)


def test_refusals_through_the_c_abi_and_a_valid_batch_afterwards(gpu_ctx, lib, data):
    from se_snmf_nat_amd import SnmfError
    from se_snmf_nat_amd._lib import SnmfOnlineStreamSettings
    from se_snmf_nat_amd.online import OnlineBatchSeparator, default_settings
    good, _ = _run_mixed(gpu_ctx, data, order=[0, 3, 2])
    # a ring outside k_wadapt_batch64's envelope (R_a = 80 > 64 column lanes): refused only when a stream adapts, and the
    # refusal reports the LDS image of the divergence class that adapts
    ps = default_settings()
    rs = np.random.RandomState(0)
    Bx3, Bd3 = rs.random_sample((513, 72)) + 1e-3, rs.random_sample((513, 128)) + 1e-3
    pr = dict(ps, R_a=80, m_a=100)
    kw = dict(ctx=gpu_ctx, precision="fp64", Ad_blk0=[np.ones((80, 100))] * 2)
    x = [np.round(rs.randn(8 * HOP) * 300.0)] * 2
    off = dict(adapt_train_N=0)
    sep = OnlineBatchSeparator(Bx3, Bd3, pr, 2, settings=[off, dict(off, cf="ed")], **kw)  # nobody adapts: accepted, and it runs
    before = [o["x_tilde_f"] for o in sep.process(x, flush=True)]
    for entry, beta in ((dict(), 1.0), (dict(cf="ed"), 2.0), (dict(cf="x", beta_div=1.5), 1.5)):
        with pytest.raises(SnmfError, match="R_a <= 64, m_a <= 128") as e:
            OnlineBatchSeparator(Bx3, Bd3, pr, 2, settings=[off, entry], **kw)
        assert e.value.status == 8
        need, limit = (int(v) for v in re.search(r"(\d+) bytes of LDS <= (\d+)", e.value.message).groups())
        print("refused ring 80 x 100 with one adapting stream, beta %g: %d bytes of LDS (limit %d)" % (beta, need, limit))
        assert need == wbatch64_lds(80, 100, beta) and limit == 160 * KB
        with pytest.raises(SnmfError, match="R_a <= 64, m_a <= 128") as e:  # ... and so is the restart that would turn one on
            sep.restart(1, Ad_blk0=np.ones((80, 100)), settings=entry)
        assert e.value.status == 8
    assert sep.settings(1)["adapt_train_N"] == 0 and sep.settings(1)["beta_div"] == 2.0  # the refused restarts changed nothing
    sep.restart([0, 1])
    after = [o["x_tilde_f"] for o in sep.process(x, flush=True)]
    sep.close()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # an entry that ob_validate refuses for p itself is refused with the same status
    for entry, status in ((dict(max_iter=0), 1), (dict(blk_gap=4), 1), (dict(P_len_k=7), 1)):
        with pytest.raises(SnmfError) as e:
            OnlineBatchSeparator(Bx3, Bd3, dict(ps, adapt_train_N=0), 2, ctx=gpu_ctx, precision="fp64", settings=[{}, entry])
        assert e.value.status == status, entry
    # the _streams_f64 entries and _get_settings on an fp32 batch: SNMF_ERR_STATE (7), the batch not harmed
    pcms, Bx, Bds, H0s, Ads = _streams([12 * HOP, 10 * HOP], seed=2)
    ref32 = [o["x_tilde_f"] for o in OnlineBatchSeparator(Bx, Bds, ps, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx).process(pcms, flush=True)]
    sep32 = OnlineBatchSeparator(Bx, Bds, ps, 2, H0=H0s, Ad_blk0=Ads, ctx=gpu_ctx)
    sl = np.zeros(1, np.int32)
    st = SnmfOnlineStreamSettings()
    Bx64 = np.asfortranarray(Bx, dtype=np.float64)
    assert lib.snmf_online_batch_restart_streams_f64(sep32._h, 1, sl.ctypes.data, Bx64.ctypes.data, None, None, None, None) == 7
    assert lib.snmf_online_batch_restart_streams_f64(sep32._h, 1, sl.ctypes.data, None, None, None, None, C.cast(C.byref(st), C.c_void_p)) == 7
    assert lib.snmf_online_batch_get_settings(sep32._h, 0, C.byref(st)) == 7
    o32 = sep32.process(pcms, flush=True)
    sep32.close()
    assert all(np.array_equal(o32[k]["x_tilde_f"], ref32[k]) for k in range(2))
    # a slot out of range or listed twice, and a stream in the middle of a recording: the existing restart's statuses
    p, pc, Bxs, Bds6, H0s6, Ads6 = data
    sep = OnlineBatchSeparator([Bxs[0]] * 2, Bds6[:2], _settings(p), 2, H0=H0s6[:2], Ad_blk0=Ads6[:2], ctx=gpu_ctx, precision="fp64",
                               settings=SETTINGS[:2])
    two = np.array([0, 0], np.int32)
    assert lib.snmf_online_batch_restart_streams_f64(sep._h, 3, two.ctypes.data, None, None, None, None, None) == 1
    assert lib.snmf_online_batch_restart_streams_f64(sep._h, 2, two.ctypes.data, None, None, None, None, None) == 1
    assert lib.snmf_online_batch_get_settings(sep._h, 2, C.byref(st)) == 1
    sep.process([pc[0][:100], pc[1][:0]], flush=False)
    assert lib.snmf_online_batch_restart_streams_f64(sep._h, 1, sl.ctypes.data, None, None, None, None, None) == 7
    sep.close()
    # afterwards a valid mixed batch gives the bits it gave before
    again, _ = _run_mixed(gpu_ctx, data, order=[0, 3, 2])
    for a, b in zip(again, good):
        _same(a, b, "after the refusals")
