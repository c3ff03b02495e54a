"""Get-state / set-state of the batched online separator on the device (snmf_online_batch_get_state / _set_state,
OnlineBatchSeparator.get_state / set_state; kernels k_obstate_get / _put and their fp64 twins).

A stream's state g leaves the device as a value and comes back into any slot of any batch of the same configuration; the
resumed stream's signals, trace and dictionary have the BITS of the uninterrupted run.  The small geometry is the smallest
at which a ring wraps (F = 65, an 8 x 12 ring, P_len_l = 5): cut after 557 samples = 22 hops and 7 pending samples, the three
streams stand at n_push 22 / 11 / 22 in the fp64 oracle.  Every test asserts what makes its case non-trivial from the
device's own returned state (ring phases, wrapped rings, update_switch, pending samples, solves on both sides of the cut).

The fp64 layout test holds the fp64 mode's own bounds (tests/test_online_batch_f64.py: FIX_OVERALL, FIX_BASIS)."""
import numpy as np
import pytest

from oracle.online_oracle import default_params, init_buff, ntf_sep_event_rt, sep_frame
from test_online_batch import _geo_streams, _settings
from test_online_batch_f64 import FIX_BASIS, FIX_OVERALL, _rel
from test_online_batch_f64 import _streams as _streams_f64
from test_online_batch_mel import _mel_params, _mel_streams

pytestmark = pytest.mark.gpu

GEO = (128, 100, 25, 16, 20, dict(P_len_k=12, P_len_l=5, init_N_len=5, DCbin=2, DCbin_back=2, R_a=8, m_a=12, overlap_m_a=0.3))
CUT_SMALL = 557            # 22 hops of 25 and 7 pending samples
CUT_SHIPPED = 22 * 160 + 7
PARTITION = dict(EVENT_NUM=2, EVENT_RANK=[1, 9], NOISE_NUM=2, NOISE_RANK=[1, 11])
SLOTS = (4, 0, 2)          # where the three states go in the batch of five
ORDER5 = (1, 0, 2, 1, 0)   # whose configuration each slot of that batch has (slots 1 and 3: the company)


# ---------------------------------------------------------------- inputs ------------------------------------------------
def _small(precision="fp32", cls=False, streams=False):
    p, pcms, Bx, Bds, H0s, Ads = _geo_streams(GEO, 48)
    p = _settings(p)
    d = dict(p=p, pcms=pcms, Bx=Bx, Bds=Bds, H0s=H0s, Ads=Ads, precision=precision, cls=cls, cut=CUT_SMALL, settings=None, mel=False)
    if streams:  # settings per stream and two event dictionaries (snmf_online_batch_create_streams_f64)
        rs = np.random.RandomState(5)
        d["Bx"] = [Bx, Bx * (1.0 + 0.05 * rs.random_sample(Bx.shape)), Bx]
        d["settings"] = [{}, dict(alpha_d=0.65), dict(sparsity=4)]
    return d


def _shipped(precision):
    pcms, Bx, Bds, H0s, Ads = _streams_f64([40 * 160, 33 * 160 + 53, 37 * 160])
    return dict(p=_settings(default_params()), pcms=pcms, Bx=Bx, Bds=Bds, H0s=H0s, Ads=Ads, precision=precision, cls=False, cut=CUT_SHIPPED,
                settings=None, mel=False)


def _mel(melconv, cls=False):
    p = _mel_params(melconv)
    pcms, Bx, Bds, H0s, Ads, BMx, BMds = _mel_streams(40, S=5, p=p)
    pick = lambda v: [v[k] for k in (0, 2, 3)]  # noqa: E731  (the three long streams: 40, 40 + 57 samples and 33 hops)
    return dict(p=_settings(p), pcms=pick(pcms), Bx=Bx, Bds=pick(Bds), H0s=pick(H0s), Ads=pick(Ads), BMx=BMx, BMds=pick(BMds), precision="fp32",
                cls=cls, cut=CUT_SHIPPED, settings=None, mel=True)


def _make(ctx, d, order, wrong=False):
    """A batch whose slot i has stream order[i]'s configuration (event dictionary, settings).  wrong: the slots start from
    another stream's noise dictionary and draws, which a set_state must replace."""
    from se_snmf_nat_amd.online import OnlineBatchSeparator
    src = [(k + 1) % 3 if wrong else k for k in order]
    p = dict(d["p"], **PARTITION) if d["cls"] else d["p"]
    kw = {}
    if d["mel"]:
        kw.update(B_Mel_x=d["BMx"], B_Mel_d=[d["BMds"][k] for k in src])
    if d["settings"] is not None:
        kw.update(settings=[d["settings"][k] for k in order])
    Bx = [d["Bx"][k] for k in order] if isinstance(d["Bx"], list) else d["Bx"]
    return OnlineBatchSeparator(Bx, [d["Bds"][k] for k in src], p, len(order), H0=[d["H0s"][k] for k in src],
                                Ad_blk0=[d["Ads"][k] for k in src], ctx=ctx, class_outputs=d["cls"], precision=d["precision"], **kw)


def _keys(d):
    return ("x_tilde", "x_tilde_f") + (("x_hat", "d_hat", "x_hat_i", "d_hat_i") if d["cls"] else ())


def _final(sep, d, k):
    return [sep.basis_f64(k)] + ([sep.mel_basis_f64(k)] if d["mel"] else [])


def _whole(ctx, d):
    """Every stream run whole: per stream (outputs, trace, final masters)."""
    sep = _make(ctx, d, (0, 1, 2))
    outs = sep.process(d["pcms"], flush=True)
    res = [({key: outs[k][key] for key in _keys(d)}, sep.trace(k), _final(sep, d, k)) for k in range(3)]
    sep.close()
    return res


def _head(ctx, d, get=True):
    """The first d['cut'] samples of every stream: (outputs, traces, states, the open batch)."""
    sep = _make(ctx, d, (0, 1, 2))
    outs = sep.process([x[:d["cut"]] for x in d["pcms"]])
    return outs, [sep.trace(k) for k in range(3)], sep.get_state([0, 1, 2]) if get else None, sep


def _assert_same(d, whole, parts, traces, finals):
    """parts: per stream the list of output dicts in feeding order; traces: likewise lists of trace lists."""
    for k in range(3):
        for key in _keys(d):
            got = np.concatenate([o[key] for o in parts[k]], axis=-1)
            assert got.dtype == whole[k][0][key].dtype and np.array_equal(got, whole[k][0][key], equal_nan=True), (k, key)
        assert sum(traces[k], []) == whole[k][1], k
        for a, b in zip(finals[k], whole[k][2]):
            assert np.array_equal(a, b), k


def _assert_not_trivial(d, states, tr1, tr2, small):
    ma, Pl = states[0]["lambda_d_blk"].shape[1], states[0]["r_blk"].shape[1]
    assert all(st["n_push"] % ma != 0 for st in states), [st["n_push"] for st in states]
    assert all((st["l"] - 1) % Pl != 0 for st in states)
    assert all(st["pending"].size == 7 for st in states)
    solved = lambda tr: sum(int(t["solved"]) for t in tr)  # noqa: E731
    if small:  # a wrapped ring and a count in the middle of its cycle
        assert any(st["n_push"] > ma for st in states) and any(st["update_switch"] > 1 for st in states)
    if small and d["settings"] is None:  # (the shared settings: the oracle stands at 22 / 11 / 22 pushes, 7 / 3 / 7 solves)
        assert any(st["n_push"] < ma for st in states)
        assert all(solved(a) > 0 and solved(b) > 0 for a, b in zip(tr1, tr2)), ([solved(a) for a in tr1], [solved(b) for b in tr2])
    else:
        assert sum(map(solved, tr1)) > 0 and sum(map(solved, tr2)) > 0


def _resume(ctx, d, states):
    """The states into slots SLOTS of a batch of five whose other two streams are running; the rest of every stream, flushed."""
    hop = d["p"]["frameshift"]
    sep = _make(ctx, d, ORDER5, wrong=True)
    company = {1: d["pcms"][0][::-1][:30 * hop].copy(), 3: d["pcms"][1][::-1][:20 * hop].copy()}
    empty = np.zeros(0)
    sep.process([company[s][:10 * hop] if s in company else empty for s in range(5)])
    sep.set_state(list(SLOTS), states)
    assert all(sep.trace(s) == [] for s in SLOTS)  # the trace goes on from frame l
    feed = [company[s][10 * hop:] if s in company else d["pcms"][SLOTS.index(s)][d["cut"]:] for s in range(5)]
    outs = sep.process(feed, flush=True)
    res = [(outs[s], sep.trace(s), _final(sep, d, s)) for s in SLOTS]
    sep.close()
    return res


CASES = {
    "fp32-dft": lambda cls: _small("fp32", cls),
    "fp32-mel-conv1": lambda cls: _mel(1, cls),
    "fp32-mel-conv0": lambda cls: _mel(0, cls),
    "fp64": lambda cls: _small("fp64", cls),
    "fp64-streams": lambda cls: _small("fp64", cls, streams=True),
    "fp32-shipped": lambda cls: _shipped("fp32"),
    "fp64-shipped": lambda cls: _shipped("fp64"),
}
_cache = {}


def _case(ctx, name, cls=False):
    """(inputs, whole run, head outputs, head traces, states) of a case, computed once."""
    if (name, cls) not in _cache:
        d = CASES[name](cls)
        o1, tr1, states, sep = _head(ctx, d)
        sep.close()
        _cache[(name, cls)] = (d, _whole(ctx, d), o1, tr1, states)
    return _cache[(name, cls)]


# ---------------------------------------------------------------- 1. resume, bit for bit --------------------------------
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "classes"])
@pytest.mark.parametrize("name", ["fp32-dft", "fp32-mel-conv1", "fp32-mel-conv0", "fp64", "fp64-streams"])
def test_a_resumed_stream_has_the_bits_of_the_whole_run(gpu_ctx, name, cls):
    d, whole, o1, tr1, states = _case(gpu_ctx, name, cls)
    res = _resume(gpu_ctx, d, states)
    _assert_not_trivial(d, states, tr1, [r[1] for r in res], small=not d["mel"])
    if cls:
        assert states[0]["class_tails"].shape[0] == 4 and all(np.any(st["class_tails"] != 0) and np.any(st["x_hat_tail"] != 0) for st in states)
    _assert_same(d, whole, [[o1[k], res[k][0]] for k in range(3)], [[tr1[k], res[k][1]] for k in range(3)], [r[2] for r in res])


@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_resume_through_the_raw_bytes_of_a_file(gpu_ctx, tmp_path, name):
    d, whole, o1, tr1, states = _case(gpu_ctx, name)
    path = tmp_path / "streams.state"
    path.write_bytes(b"".join(st["record"] for st in states))
    blob = path.read_bytes()
    n = len(blob) // 3
    res = _resume(gpu_ctx, d, [blob[i * n:(i + 1) * n] for i in range(3)])
    _assert_same(d, whole, [[o1[k], res[k][0]] for k in range(3)], [[tr1[k], res[k][1]] for k in range(3)], [r[2] for r in res])


@pytest.mark.parametrize("name", ["fp32-shipped", "fp64-shipped"])
def test_resume_at_the_shipped_geometry(gpu_ctx, name):
    d, whole, o1, tr1, states = _case(gpu_ctx, name)
    assert states[0]["lambda_d_blk"].shape == (513, 100) and states[0]["Ad_blk"].shape == (50, 100)
    res = _resume(gpu_ctx, d, states)
    _assert_not_trivial(d, states, tr1, [r[1] for r in res], small=False)
    _assert_same(d, whole, [[o1[k], res[k][0]] for k in range(3)], [[tr1[k], res[k][1]] for k in range(3)], [r[2] for r in res])


# ---------------------------------------------------------------- 2. round trip ------------------------------------------
@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_set_then_get_returns_the_record_and_a_get_disturbs_nothing(gpu_ctx, name):
    from se_snmf_nat_amd import _lib
    d, whole, o1, tr1, states = _case(gpu_ctx, name)
    ma = states[0]["lambda_d_blk"].shape[1]
    sep = _make(gpu_ctx, d, (0, 1, 2), wrong=True)
    _, lay = sep._state_layout(_lib.load())
    off = lay["n_push"][0]
    for n_push in (2 * ma, ma + 1, 2 * ma - 1):  # ring phases 0, 1 and m_a - 1
        want = bytearray(states[0]["record"])
        want[off:off + 4] = np.int32(n_push).tobytes()
        sep.set_state(1, dict(states[0], n_push=n_push))
        got = sep.get_state(1)
        assert got["record"] == bytes(want) and got["n_push"] == n_push
        for key in ("lambda_d_blk", "Ad_blk", "r_blk", "B_DFT_d", "x_tilde_tail", "pending"):
            assert np.array_equal(got[key], states[0][key]), key
    sep.close()
    # two gets with nothing in between; the stream goes on with the bits of the whole run
    o1b, tr1b, first, sep = _head(gpu_ctx, d)
    second = sep.get_state([0, 1, 2])
    assert [st["record"] for st in first] == [st["record"] for st in second] == [st["record"] for st in states]
    outs = sep.process([x[d["cut"]:] for x in d["pcms"]], flush=True)
    _assert_same(d, whole, [[o1b[k], outs[k]] for k in range(3)], [[sep.trace(k)] for k in range(3)], [_final(sep, d, k) for k in range(3)])
    sep.close()


# ---------------------------------------------------------------- 3. / 4. the layout is the reference's ------------------
def _oracle_head(d, k, n_frames):
    """oracle.online_oracle's driver loop (ntf_sep_event_rt:271-302) for the first n_frames frames of stream k ->
    (g, y, x_tilde, number of triggered frames)."""
    p = dict(d["p"])
    sz, hop = p["framelength"], p["frameshift"]
    g = init_buff(d["Bx"], d["Bds"][k], p, d["Ads"][k])
    y, x_tilde, pushes = np.zeros(sz), np.zeros(sz), 0
    for l in range(1, n_frames + 1):
        y[:sz - hop] = y[hop:].copy()
        y[sz - hop:] = d["pcms"][k][(l - 1) * hop:l * hop]
        frame, _, _, tr = sep_frame(y, l, g, p, d["H0s"][k])
        pushes += int(tr["trig"])
        if l > p["delay"]:
            x_tilde[:sz - hop] = x_tilde[hop:].copy()
            x_tilde[sz - hop:] = 0.0
            x_tilde = x_tilde + frame
    return g, y, x_tilde, pushes


@pytest.fixture(scope="module")
def oracle22():
    d = _small("fp64")
    return [_oracle_head(d, k, 22) for k in range(3)]


def test_the_fp64_state_is_the_oracles_g(gpu_ctx, oracle22):
    d, whole, o1, tr1, states = _case(gpu_ctx, "fp64")
    hop = d["p"]["frameshift"]
    for k, (st, (g, y, x_tilde, pushes)) in enumerate(zip(states, oracle22)):
        errs = {key: _rel(st[key], g[key]) for key in ("Xm_tilde", "lambda_dav", "r_blk", "lambda_d_blk", "Ad_blk")}
        print("stream %d: %s; B_DFT_d %.3g" % (k, ", ".join("%s %.3g" % kv for kv in errs.items()), _rel(st["B_DFT_d"], g["B_DFT_d"])))
        assert max(errs.values()) <= FIX_OVERALL, (k, errs)
        assert _rel(st["B_DFT_d"], g["B_DFT_d"]) <= FIX_BASIS
        assert (st["n_push"], st["update_switch"], st["l"]) == (pushes, g["update_switch"], 23)
        assert np.array_equal(st["B_fix"], g["B_Mel_d"]) and np.array_equal(st["H0"], d["H0s"][k]) and np.array_equal(st["Ad_blk0"], d["Ads"][k])
        assert np.array_equal(st["y_hist"], y[hop:]) and np.array_equal(st["pending"], d["pcms"][k][22 * hop:CUT_SMALL])


def test_a_state_built_from_the_oracles_g_runs_on_as_the_oracle(gpu_ctx, oracle22):
    d = _small("fp64")
    p, hop, sz = d["p"], d["p"]["frameshift"], d["p"]["framelength"]
    sep = _make(gpu_ctx, d, (0, 1, 2), wrong=True)
    shapes = sep._state_shapes()
    states = []
    for k, (g, y, x_tilde, pushes) in enumerate(oracle22):
        tail = np.zeros(shapes["x_tilde_tail"][0])
        tail[-sz:] = x_tilde  # the newest kept frame carries the accumulated buffer: the overlap-add is a sum
        states.append(dict(Xm_tilde=g["Xm_tilde"], lambda_dav=g["lambda_dav"], r_blk=g["r_blk"], lambda_d_blk=g["lambda_d_blk"], Ad_blk=g["Ad_blk"],
                           n_push=pushes, update_switch=g["update_switch"], B_DFT_d=g["B_DFT_d"], B_fix=g["B_Mel_d"], H0=d["H0s"][k],
                           Ad_blk0=d["Ads"][k], l=23, y_hist=y[hop:], pending=d["pcms"][k][22 * hop:CUT_SMALL], x_tilde_tail=tail))
    sep.set_state([0, 1, 2], states)
    outs = sep.process([x[CUT_SMALL:] for x in d["pcms"]], flush=True)
    for k in range(3):
        _, of, Bdn, rtr = ntf_sep_event_rt(d["pcms"][k], d["Bx"], d["Bds"][k], dict(p), d["H0s"][k], d["Ads"][k], return_trace=True)
        tr = sep.trace(k)
        for key in ("n_iter", "trig", "n_up", "adapt_iters"):
            assert [int(t[key]) for t in tr] == [int(t[key]) for t in rtr[22:]], (k, key)
        ref = of[(22 - p["delay"]) * hop:]
        got = outs[k]["x_tilde_f"]
        ok = np.isfinite(ref)
        assert len(got) == len(ref) and np.array_equal(np.isfinite(got), ok)
        print("stream %d: signal %.3g, B_DFT_d %.3g" % (k, _rel(got[ok], ref[ok]), _rel(sep.basis_f64(k), Bdn)))
        assert _rel(got[ok], ref[ok]) <= FIX_OVERALL and _rel(sep.basis_f64(k), Bdn) <= FIX_BASIS
    sep.close()


def test_the_fp32_rings_stand_in_the_oracles_column_order(gpu_ctx, oracle22):
    d, whole, o1, tr1, states = _case(gpu_ctx, "fp32-dft")
    for k, (st, (g, _, _, pushes)) in enumerate(zip(states, oracle22)):
        assert st["n_push"] == pushes
        for key in ("lambda_d_blk", "Ad_blk"):
            dev, ref = st[key].astype(np.float64), g[key]
            def rel(a, b):  # (a ring that has not wrapped still holds init_buff's zero columns)
                na, nb = np.linalg.norm(a - b), np.linalg.norm(b)
                return na / nb if nb > 0 else (0.0 if na == 0 else np.inf)
            dist = np.array([[rel(dev[:, c], ref[:, j]) for j in range(ref.shape[1])] for c in range(dev.shape[1])])
            assert np.array_equal(dist.argmin(axis=1), np.arange(dev.shape[1])), (k, key)


# ---------------------------------------------------------------- 5. refusals --------------------------------------------
def _refused(call, status, match):
    from se_snmf_nat_amd import SnmfError
    with pytest.raises(SnmfError, match=match) as e:
        call()
    assert e.value.status == status, match


@pytest.mark.parametrize("what", ["other-precision", "other-m_a", "truncated", "flushed-get", "duplicate-slots"])
def test_a_refused_call_changes_nothing(gpu_ctx, lib, what):
    d, whole, _, _, states = _case(gpu_ctx, "fp32-dft")
    sep = _make(gpu_ctx, d, (0, 1, 2))
    cut = [len(x) if (what == "flushed-get" and k == 1) else d["cut"] for k, x in enumerate(d["pcms"])]
    o1 = sep.process([x[:c] for x, c in zip(d["pcms"], cut)], flush=[what == "flushed-get" and k == 1 for k in range(3)])
    if what == "other-precision":
        rec = _case(gpu_ctx, "fp64")[4][0]["record"]
        _refused(lambda: sep.set_state(1, rec), 3, "elem_size")
    elif what == "other-m_a":
        d10 = dict(d, p=dict(d["p"], m_a=10), Ads=[a[:, :10] for a in d["Ads"]])
        other = _make(gpu_ctx, d10, (0, 1, 2))
        rec = other.get_state(0)["record"]
        other.close()
        _refused(lambda: sep.set_state(1, rec), 3, "m_a")
    elif what == "truncated":
        _refused(lambda: sep.set_state(1, states[1]["record"][:-8]), 1, "bytes")
        _refused(lambda: sep.set_state(1, states[1]["record"][:40]), 1, "header")
        _refused(lambda: sep.set_state(1, b"\0" * 8 + states[1]["record"][8:]), 1, "magic")
    elif what == "flushed-get":
        _refused(lambda: sep.get_state(1), 7, "flushed")
        _refused(lambda: sep.get_state([0, 1]), 7, "flushed")
    else:
        blob = np.frombuffer(states[1]["record"] * 2, dtype=np.uint8).copy()
        sl = np.array([1, 1], dtype=np.int32)
        assert lib.snmf_online_batch_set_state(sep._h, 2, sl.ctypes.data, blob.ctypes.data, blob.size) == 1
        assert lib.snmf_online_batch_get_state(sep._h, 2, sl.ctypes.data, blob.ctypes.data, blob.size) == 1
        sl[1] = 3
        assert lib.snmf_online_batch_set_state(sep._h, 2, sl.ctypes.data, blob.ctypes.data, blob.size) == 1
    outs = sep.process([x[c:] for x, c in zip(d["pcms"], cut)], flush=[c < len(x) for x, c in zip(d["pcms"], cut)])
    _assert_same(d, whole, [[o1[k], outs[k]] for k in range(3)], [[sep.trace(k)] for k in range(3)], [_final(sep, d, k) for k in range(3)])
    sep.close()
