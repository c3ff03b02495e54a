"""The single-stream online separator's state g as a value, and its restart in place, on the device
(snmf_online_get_state / _set_state / _restart_f32 / _f64, OnlineSeparator.get_state / set_state / restart,
ntf_sep_event_rt_chain; kernels k_ostate_get / _put and their fp64 twins).

The inputs are those of tests/test_gpu_online_batch_state.py, one stream at a time.  The small geometry is the smallest at
which a ring wraps (F = 65, an 8 x 12 ring, P_len_l = 5): cut after 557 samples = 22 hops and 7 pending samples, stream 0
stands at n_push 22 (a wrapped ring, update_switch 2) and stream 1 at n_push 11 (an unwrapped ring, update_switch 3) in the
fp64 oracle, with 7 / 3 adaptation solves before the cut and 9 / 4 behind it (oracle/online_oracle.py, run on the CPU).
Every resume test asserts what makes its case non-trivial from the device's own returned state.

A resumed, restarted or refused separator is compared BIT FOR BIT with the uninterrupted run on the same kernels.  Where
the two kinds of separator meet (a record continued on the other kind) and where the oracle is the reference, the fp64
mode's own bounds hold (tests/test_online_f64.py: FIX_OVERALL, FIX_BASIS) and the per-frame decisions are equal."""
import numpy as np
import pytest

from oracle.online_oracle import ntf_sep_event_rt
from test_gpu_online_batch_state import CUT_SMALL, PARTITION, _head as _batch_head
from test_gpu_online_batch_state import _make as _make_batch
from test_gpu_online_batch_state import _mel, _oracle_head, _shipped, _small
from test_online_batch_f64 import FIX_BASIS, FIX_OVERALL, _rel

pytestmark = pytest.mark.gpu

DECISIONS = ("n_iter", "trig", "n_up", "adapt_iters")


# ---------------------------------------------------------------- one stream of a configuration --------------------------
def _make(ctx, d, k, src=None, **over):
    """An OnlineSeparator with stream k's configuration; src: the stream whose noise dictionary and draws it starts from (a
    set_state must replace them)."""
    from se_snmf_nat_amd.online import OnlineSeparator
    src = k if src is None else src
    p = dict(d["p"], **PARTITION) if d["cls"] else d["p"]
    kw = dict(B_Mel_x=d["BMx"], B_Mel_d=d["BMds"][src]) if d["mel"] else {}
    kw.update(over)
    return OnlineSeparator(d["Bx"], kw.pop("B_DFT_d", d["Bds"][src]), p, H0=kw.pop("H0", d["H0s"][src]), Ad_blk0=kw.pop("Ad_blk0", d["Ads"][src]),
                           ctx=ctx, class_outputs=kw.pop("class_outputs", d["cls"]), precision=d["precision"], **kw)


def _keys(d):
    return ("x_tilde", "x_tilde_f") + (("x_hat", "d_hat", "x_hat_i", "d_hat_i") if d["cls"] else ())


def _final(sep, d):
    return [sep.basis_f64()] + ([sep.mel_basis()] if d["mel"] else [])


def _run(sep, d, pieces, flush=True):
    """Feed the pieces in turn (the last one with the flush) -> (outputs concatenated, trace, final dictionaries)."""
    outs = [sep.process(x, flush=flush and i == len(pieces) - 1) for i, x in enumerate(pieces)]
    return {key: np.concatenate([o[key] for o in outs], axis=-1) for key in _keys(d)}, sep.trace(), _final(sep, d)


def _assert_same(d, got, want):
    """(outputs, trace, finals) against (outputs, trace, finals): equal bits, equal dtypes."""
    for key in _keys(d):
        assert got[0][key].dtype == want[0][key].dtype and np.array_equal(got[0][key], want[0][key], equal_nan=True), key
    assert got[1] == want[1]
    assert len(got[2]) == len(want[2]) and all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))


def _join(d, o1, tr1, res):
    """The head's outputs and trace in front of a tail's (outputs, trace, finals)."""
    return {key: np.concatenate([o1[key], res[0][key]], axis=-1) for key in _keys(d)}, tr1 + res[1], res[2]


def _solved(tr):
    return sum(int(t["solved"]) for t in tr)


def _assert_not_trivial(st, tr1, tr2, small, k):
    ma, Pl = st["lambda_d_blk"].shape[1], st["r_blk"].shape[1]
    assert st["n_push"] % ma != 0 and (st["l"] - 1) % Pl != 0 and st["pending"].size == 7, (st["n_push"], st["l"], st["pending"].size)
    if small:  # stream 0: a wrapped ring; stream 1: one that has not wrapped; both in the middle of the update cycle
        assert st["update_switch"] > 1 and (st["n_push"] > ma if k == 0 else st["n_push"] < ma), (k, st["n_push"], st["update_switch"])
    assert _solved(tr1) > 0 and _solved(tr2) > 0, (_solved(tr1), _solved(tr2))


CASES = {
    "fp32-dft": lambda cls: _small("fp32", cls),
    "fp32-mel-conv1": lambda cls: _mel(1, cls),
    "fp32-mel-conv0": lambda cls: _mel(0, cls),
    "fp64": lambda cls: _small("fp64", cls),
    "fp32-shipped": lambda cls: _shipped("fp32"),
    "fp64-shipped": lambda cls: _shipped("fp64"),
}
_inputs, _cache = {}, {}


def _input(name, cls=False):
    if (name, cls) not in _inputs:
        _inputs[(name, cls)] = CASES[name](cls)
    return _inputs[(name, cls)]


def _case(ctx, name, k=0, cls=False):
    """(inputs, whole run, head outputs, head trace, state at the cut) of stream k of a case, computed once."""
    if (name, k, cls) not in _cache:
        d = _input(name, cls)
        sep = _make(ctx, d, k)
        whole = _run(sep, d, [d["pcms"][k]])
        sep.close()
        sep = _make(ctx, d, k)
        o1 = sep.process(d["pcms"][k][:d["cut"]])
        tr1, st = sep.trace(), sep.get_state()
        sep.close()
        _cache[(name, k, cls)] = (d, whole, o1, tr1, st)
    return _cache[(name, k, cls)]


def _resume(ctx, d, k, state):
    """A new separator created from another stream's dictionary and draws takes the state and runs the rest, flushed."""
    sep = _make(ctx, d, k, src=(k + 1) % 3)
    sep.set_state(state)
    assert sep.trace() == []  # the trace goes on from frame l
    res = _run(sep, d, [d["pcms"][k][d["cut"]:]])
    sep.close()
    return res


# ---------------------------------------------------------------- 1. resume, bit for bit --------------------------------
@pytest.mark.parametrize("cls", [False, True], ids=["plain", "classes"])
@pytest.mark.parametrize("k", [0, 1], ids=["wrapped", "unwrapped"])
@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_a_resumed_separator_has_the_bits_of_the_whole_run(gpu_ctx, name, k, cls):
    d, whole, o1, tr1, st = _case(gpu_ctx, name, k, cls)
    res = _resume(gpu_ctx, d, k, st)
    _assert_not_trivial(st, tr1, res[1], True, k)
    if cls:
        assert st["class_tails"].shape[0] == 4 and np.any(st["class_tails"] != 0) and np.any(st["x_hat_tail"] != 0)
    _assert_same(d, _join(d, o1, tr1, res), whole)


@pytest.mark.parametrize("name", ["fp32-mel-conv1", "fp32-mel-conv0", "fp32-shipped", "fp64-shipped"])
def test_resume_at_the_shipped_geometry(gpu_ctx, name):
    d, whole, o1, tr1, st = _case(gpu_ctx, name)
    assert st["lambda_d_blk"].shape == (513, 100) and st["Ad_blk"].shape == (50, 100)
    if d["mel"]:
        assert st["B_Mel_d"].shape == (64, 100) and not np.array_equal(st["B_Mel_d"], np.asarray(d["BMds"][0], dtype=np.float32))  # adapted
    res = _resume(gpu_ctx, d, 0, st)
    _assert_not_trivial(st, tr1, res[1], False, 0)
    _assert_same(d, _join(d, o1, tr1, res), whole)


@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_resume_through_the_raw_bytes_of_a_file(gpu_ctx, tmp_path, name):
    d, whole, o1, tr1, st = _case(gpu_ctx, name)
    path = tmp_path / "stream.state"
    path.write_bytes(st["record"])
    res = _resume(gpu_ctx, d, 0, path.read_bytes())
    _assert_same(d, _join(d, o1, tr1, res), whole)


# ---------------------------------------------------------------- 2. get_state disturbs nothing ---------------------------
@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_set_then_get_returns_the_record(gpu_ctx, name):
    from se_snmf_nat_amd import _lib
    d, whole, o1, tr1, st = _case(gpu_ctx, name)
    ma = st["lambda_d_blk"].shape[1]
    sep = _make(gpu_ctx, d, 0, src=1)
    _, lay = sep._state_layout(_lib.load())
    off = lay["n_push"][0]
    for n_push in (st["n_push"], 2 * ma, ma + 1, 2 * ma - 1):  # the cut's phase, and ring phases 0, 1 and m_a - 1
        want = bytearray(st["record"])
        want[off:off + 4] = np.int32(n_push).tobytes()
        sep.set_state(dict(st, n_push=n_push))
        got = sep.get_state()
        assert got["record"] == bytes(want) and got["n_push"] == n_push
        for key in ("lambda_d_blk", "Ad_blk", "r_blk", "B_DFT_d", "x_tilde_tail", "pending"):
            assert np.array_equal(got[key], st[key]), key
    sep.close()


@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_a_get_between_process_calls_disturbs_nothing(gpu_ctx, name):
    d, whole, o1, tr1, st = _case(gpu_ctx, name)
    x, cut = d["pcms"][0], d["cut"]
    sep = _make(gpu_ctx, d, 0)
    before = sep.get_state()  # before the first process call
    assert before["l"] == 1 and before["n_push"] == 0 and before["pending"].size == 0 and np.array_equal(before["Ad_blk"], before["Ad_blk0"])
    parts = [sep.process(x[:cut])]
    first, second = sep.get_state(), sep.get_state()
    assert first["record"] == second["record"] == st["record"]
    parts.append(sep.process(x[cut:cut + 300]))
    assert sep.get_state()["l"] > first["l"]
    parts.append(sep.process(x[cut + 300:], flush=True))
    got = ({key: np.concatenate([o[key] for o in parts], axis=-1) for key in _keys(d)}, sep.trace(), _final(sep, d))
    sep.close()
    _assert_same(d, got, whole)


# ---------------------------------------------------------------- 3. the fp64 layout is the reference's -----------------
@pytest.fixture(scope="module")
def oracle22():
    d = _small("fp64")
    return [_oracle_head(d, k, 22) for k in range(2)]


@pytest.mark.parametrize("k", [0, 1])
def test_the_fp64_state_is_the_oracles_g(gpu_ctx, oracle22, k):
    d, whole, o1, tr1, st = _case(gpu_ctx, "fp64", k)
    hop = d["p"]["frameshift"]
    g, y, x_tilde, pushes = oracle22[k]
    errs = {key: _rel(st[key], g[key]) for key in ("Xm_tilde", "lambda_dav", "r_blk", "lambda_d_blk", "Ad_blk")}
    print("stream %d: %s; B_DFT_d %.3g" % (k, ", ".join("%s %.3g" % kv for kv in errs.items()), _rel(st["B_DFT_d"], g["B_DFT_d"])))
    assert max(errs.values()) <= FIX_OVERALL, errs
    assert _rel(st["B_DFT_d"], g["B_DFT_d"]) <= FIX_BASIS
    assert (st["n_push"], st["update_switch"], st["l"]) == (pushes, g["update_switch"], 23) and pushes == (22, 11)[k]
    assert np.array_equal(st["B_fix"], g["B_Mel_d"]) and np.array_equal(st["H0"], d["H0s"][k]) and np.array_equal(st["Ad_blk0"], d["Ads"][k])
    assert np.array_equal(st["y_hist"], y[hop:]) and np.array_equal(st["pending"], d["pcms"][k][22 * hop:CUT_SMALL])
    # the rings are in time order: every column is nearest its own column of the oracle's ring
    for key in ("lambda_d_blk", "Ad_blk"):
        dev, ref = st[key], g[key]
        dist = np.array([[np.linalg.norm(dev[:, c] - ref[:, j]) for j in range(ref.shape[1])] for c in range(dev.shape[1])])
        live = np.linalg.norm(ref, axis=0) > 0  # (a ring that has not wrapped still holds init_buff's zero columns in lambda_d_blk)
        assert np.array_equal(dist.argmin(axis=1)[live], np.arange(dev.shape[1])[live]), key


@pytest.mark.parametrize("k", [0, 1])
def test_a_state_built_from_the_oracles_g_runs_on_as_the_oracle(gpu_ctx, oracle22, k):
    d = _input("fp64")
    p, hop, sz = d["p"], d["p"]["frameshift"], d["p"]["framelength"]
    g, y, x_tilde, pushes = oracle22[k]
    sep = _make(gpu_ctx, d, k, src=(k + 1) % 3)
    tail = np.zeros(sep._state_shapes()["x_tilde_tail"][0])
    tail[-sz:] = x_tilde  # the newest kept frame carries the accumulated buffer: the overlap-add is a sum
    sep.set_state(dict(Xm_tilde=g["Xm_tilde"], lambda_dav=g["lambda_dav"], r_blk=g["r_blk"], lambda_d_blk=g["lambda_d_blk"], Ad_blk=g["Ad_blk"],
                       n_push=pushes, update_switch=g["update_switch"], B_DFT_d=g["B_DFT_d"], B_fix=g["B_Mel_d"], H0=d["H0s"][k],
                       Ad_blk0=d["Ads"][k], l=23, y_hist=y[hop:], pending=d["pcms"][k][22 * hop:CUT_SMALL], x_tilde_tail=tail))
    out = sep.process(d["pcms"][k][CUT_SMALL:], flush=True)
    _, of, Bdn, rtr = ntf_sep_event_rt(d["pcms"][k], d["Bx"], d["Bds"][k], dict(p), d["H0s"][k], d["Ads"][k], return_trace=True)
    tr = sep.trace()
    for key in DECISIONS:
        assert [int(t[key]) for t in tr] == [int(t[key]) for t in rtr[22:]], key
    ref, got = of[(22 - p["delay"]) * hop:], out["x_tilde_f"]
    ok = np.isfinite(ref)
    assert len(got) == len(ref) and np.array_equal(np.isfinite(got), ok)
    print("stream %d: signal %.3g, B_DFT_d %.3g" % (k, _rel(got[ok], ref[ok]), _rel(sep.basis_f64(), Bdn)))
    assert _rel(got[ok], ref[ok]) <= FIX_OVERALL and _rel(sep.basis_f64(), Bdn) <= FIX_BASIS
    sep.close()


# ---------------------------------------------------------------- 4. interchange with the batch -------------------------
@pytest.mark.parametrize("name", ["fp32-dft", "fp32-mel-conv1", "fp64"])
def test_a_record_is_the_same_bytes_on_either_kind_of_separator(gpu_ctx, name):
    d, whole, o1, tr1, st = _case(gpu_ctx, name)
    batch = _make_batch(gpu_ctx, d, (0, 1, 2), wrong=True)
    batch.set_state(1, st["record"])
    back = batch.get_state(1)
    assert back["record"] == st["record"]
    for key in st:
        assert np.array_equal(back[key], st[key]) if key != "record" else True, key
    batch.close()
    # the other way round: a record taken from a batch's stream, through a single separator
    _, _, states, batch = _batch_head(gpu_ctx, d)
    batch.close()
    sep = _make(gpu_ctx, d, 0, src=1)
    for k in (2, 0):
        sep.set_state(states[k])
        assert sep.get_state()["record"] == states[k]["record"], k
    sep.close()


@pytest.mark.parametrize("direction", ["single-to-batch", "batch-to-single"])
def test_a_stream_continues_on_the_other_kind_within_the_fp64_bounds(gpu_ctx, direction):
    d, whole, o1, tr1, st = _case(gpu_ctx, "fp64")
    x, cut, p, hop = d["pcms"][0], d["cut"], d["p"], d["p"]["frameshift"]
    empty = np.zeros(0)
    if direction == "single-to-batch":
        batch = _make_batch(gpu_ctx, d, (0, 1, 2), wrong=True)
        batch.set_state(1, st)
        o2 = batch.process([empty, x[cut:], empty], flush=[False, True, False])[1]
        tr, Bn = tr1 + batch.trace(1), batch.basis_f64(1)
        batch.close()
    else:
        outs, trs, states, batch = _batch_head(gpu_ctx, d)
        batch.close()
        o1, sep = outs[0], _make(gpu_ctx, d, 0, src=1)
        sep.set_state(states[0])
        o2 = sep.process(x[cut:], flush=True)
        tr, Bn = trs[0] + sep.trace(), sep.basis_f64()
        sep.close()
    _, of, Bdn, rtr = ntf_sep_event_rt(x, d["Bx"], d["Bds"][0], dict(p), d["H0s"][0], d["Ads"][0], return_trace=True)
    assert _solved(tr[:22]) > 0 and _solved(tr[22:]) > 0
    for key in DECISIONS:
        assert [int(t[key]) for t in tr] == [int(t[key]) for t in rtr], key
    got = np.concatenate([o1["x_tilde_f"], o2["x_tilde_f"]])
    ok = np.isfinite(of)
    assert len(got) == len(of) and np.array_equal(np.isfinite(got), ok)
    print("%s: signal %.3g, B_DFT_d %.3g" % (direction, _rel(got[ok], of[ok]), _rel(Bn, Bdn)))
    assert _rel(got[ok], of[ok]) <= FIX_OVERALL and _rel(Bn, Bdn) <= FIX_BASIS


# ---------------------------------------------------------------- 5. restart --------------------------------------------
@pytest.mark.parametrize("name", ["fp32-dft", "fp64"])
def test_a_restart_with_everything_given_is_a_fresh_separator(gpu_ctx, name):
    d = _input(name, True)
    X = np.asarray(d["Bds"][1], dtype=np.float32).astype(np.float64)  # fp32-representable: creation takes it in fp32 in that mode
    h, a, file2 = d["H0s"][1], d["Ads"][1], d["pcms"][1]
    sep = _make(gpu_ctx, d, 0)
    r1 = _run(sep, d, [d["pcms"][0]])
    assert _solved(r1[1]) > 0 and not np.array_equal(r1[2][0], d["Bds"][0])  # the first file left an adapted state behind
    sep.restart(B_DFT_d=X, H0=h, Ad_blk0=a)
    assert sep.trace() == [] and np.array_equal(sep.basis_f64(), X)
    got = _run(sep, d, [file2])
    sep.close()
    fresh = _make(gpu_ctx, d, 0, B_DFT_d=X, H0=h, Ad_blk0=a)
    want = _run(fresh, d, [file2])
    fresh.close()
    assert _solved(want[1]) > 0
    _assert_same(d, got, want)


def test_a_carry_in_fp64_is_a_fresh_separator_created_with_the_master(gpu_ctx):
    d = _input("fp64")
    Ra = d["p"]["R_a"]
    sep = _make(gpu_ctx, d, 0)
    r1 = _run(sep, d, [d["pcms"][0]])
    M = sep.basis_f64()
    # the fixed columns of :328 never change, so a fresh separator that takes M for them too holds the same ones
    assert _solved(r1[1]) > 0 and not np.array_equal(M[:, :Ra], d["Bds"][0][:, :Ra]) and np.array_equal(M[:, Ra:], d["Bds"][0][:, Ra:])
    sep.restart()
    got = _run(sep, d, [d["pcms"][1]])
    sep.close()
    fresh = _make(gpu_ctx, d, 0, B_DFT_d=M)
    want = _run(fresh, d, [d["pcms"][1]])
    fresh.close()
    assert _solved(want[1]) > 0
    _assert_same(d, got, want)


@pytest.mark.parametrize("name", ["fp32-dft", "fp64", "fp32-mel-conv1"])
def test_a_carry_restart_is_a_fresh_state_with_the_carried_masters(gpu_ctx, name):
    d = _input(name, name != "fp32-mel-conv1")
    file2 = d["pcms"][1]
    sep = _make(gpu_ctx, d, 0)
    r1 = _run(sep, d, [d["pcms"][0]])
    M = sep.basis_f64()
    assert _solved(r1[1]) > 0
    sep.restart()
    assert np.array_equal(sep.basis_f64(), M) and sep.trace() == []  # unchanged, to the bit
    after = sep.get_state()  # (a restarted separator was never fed: its state is there to read)
    got = _run(sep, d, [file2])
    sep.close()
    fresh = _make(gpu_ctx, d, 0)
    st = fresh.get_state()
    for key in st:  # every piece of state is what creation gives, the carried masters aside
        if key not in ("record", "B_DFT_d", "B_Mel_d"):
            assert np.array_equal(after[key], st[key]), key
    assert np.array_equal(after["B_DFT_d"], M)
    if d["mel"]:
        assert not np.array_equal(after["B_Mel_d"], st["B_Mel_d"]) and np.array_equal(after["B_DFT_d"], st["B_DFT_d"])  # Mel mode adapts B_Mel_d
        assert np.array_equal(after["B_Mel_d"].astype(np.float32).astype(np.float64), r1[2][1])
        st["B_Mel_d"] = after["B_Mel_d"]
    else:
        assert not np.array_equal(M, st["B_DFT_d"])
    st["B_DFT_d"] = M
    fresh.set_state(st)
    want = _run(fresh, d, [file2])
    fresh.close()
    assert _solved(want[1]) > 0
    _assert_same(d, got, want)


def test_a_chain_of_two_files_follows_the_oracle_with_the_dictionary_carried(gpu_ctx):
    from se_snmf_nat_amd.online import ntf_sep_event_rt_chain
    d = _input("fp64")
    p, hop = d["p"], d["p"]["frameshift"]
    files = [d["pcms"][0][:24 * hop], d["pcms"][1][:24 * hop]]
    results, final = ntf_sep_event_rt_chain(files, d["Bx"], d["Bds"][0], p, H0=d["H0s"][0], Ad_blk0=d["Ads"][0], ctx=gpu_ctx, precision="fp64")
    split, _ = ntf_sep_event_rt_chain(files, d["Bx"], d["Bds"][0], p, H0=d["H0s"][0], Ad_blk0=d["Ads"][0], ctx=gpu_ctx, precision="fp64", chunk=557)
    Bd = d["Bds"][0]
    for i, x in enumerate(files):
        o16, of, Bdn, rtr = ntf_sep_event_rt(x, d["Bx"], Bd, dict(p), d["H0s"][0], d["Ads"][0], return_trace=True)
        i16, f, Bn = results[i]
        tr = final["traces"][i]
        assert _solved(tr) > 0
        for key in DECISIONS:
            assert [int(t[key]) for t in tr] == [int(t[key]) for t in rtr], (i, key)
        ok = np.isfinite(of)
        assert i16.dtype == np.int16 and len(f) == len(of) and np.array_equal(np.isfinite(f), ok)
        print("file %d: signal %.3g, B_DFT_d %.3g" % (i, _rel(f[ok], of[ok]), _rel(Bn, Bdn)))
        assert _rel(f[ok], of[ok]) <= FIX_OVERALL and _rel(Bn, Bdn) <= FIX_BASIS
        assert all(np.array_equal(u, v) for u, v in zip(split[i], results[i]))  # how a file is fed changes nothing
        Bd = Bdn  # the carry (B_D_u.mat)
    assert np.array_equal(final["B_DFT_d"], results[1][2]) and final["B_Mel_d"] is None


# ---------------------------------------------------------------- 6. refusals change nothing ------------------------------
def _refused(call, status, match):
    from se_snmf_nat_amd import SnmfError
    with pytest.raises(SnmfError, match=match) as e:
        call()
    assert e.value.status == status, match


def _patched(rec, lay, field, value):
    b = bytearray(rec)
    off = lay[field][0]
    b[off:off + 4] = np.int32(value).tobytes()
    return bytes(b)


@pytest.mark.parametrize("what", ["restart-unfinished", "restart-other-precision", "other-precision", "other-R_d", "other-mode", "other-class-count",
                                  "bad-magic", "truncated", "pending-is-frameshift", "bad-counters"])
def test_a_refused_call_changes_nothing(gpu_ctx, lib, what):
    cls = what == "other-class-count"
    d, whole, _, _, st = _case(gpu_ctx, "fp32-dft", 0, cls)
    x, cut = d["pcms"][0], d["cut"]
    sep = _make(gpu_ctx, d, 0)
    o1 = sep.process(x[:cut])
    before = sep.get_state()["record"]
    assert before == st["record"]
    _, lay = sep._state_layout(lib)
    if what == "restart-unfinished":
        _refused(lambda: sep.restart(), 7, "middle of a recording")
        _refused(lambda: sep.restart(B_DFT_d=d["Bds"][1]), 7, "middle of a recording")
    elif what == "restart-other-precision":
        assert lib.snmf_online_restart_f64(sep._h, None, None, None, None) == 7
        d64 = _input("fp64")
        s64 = _make(gpu_ctx, d64, 0)
        assert lib.snmf_online_restart_f32(s64._h, None, None, None, None) == 7
        Bm = np.ones((64, 20))
        assert lib.snmf_online_restart_f64(s64._h, None, Bm.ctypes.data, None, None) == 7  # B_Mel_d outside Mel mode
        assert lib.snmf_online_restart_f32(sep._h, None, Bm.ctypes.data, None, None) == 7
        s64.close()
    elif what == "other-precision":
        _refused(lambda: sep.set_state(_case(gpu_ctx, "fp64")[4]["record"]), 3, "elem_size")
    elif what == "other-R_d":
        other = _make(gpu_ctx, d, 0, B_DFT_d=d["Bds"][0][:, :19], H0=d["H0s"][0][:35])
        rec = other.get_state()["record"]
        other.close()
        _refused(lambda: sep.set_state(rec), 3, "R_d")
    elif what == "other-mode":
        _refused(lambda: sep.set_state(_case(gpu_ctx, "fp32-mel-conv1")[4]["record"]), 3, "mel")
    elif what == "other-class-count":  # class outputs on both sides, a partition (four classes) only here
        other = _make(gpu_ctx, dict(d, cls=False), 0, class_outputs=True)
        rec = other.get_state()["record"]
        other.close()
        _refused(lambda: sep.set_state(rec), 3, "n_classes")
    elif what == "bad-magic":
        _refused(lambda: sep.set_state(b"\0" * 8 + before[8:]), 1, "magic")
        _refused(lambda: sep.set_state(before[:4] + np.uint32(2).tobytes() + before[8:]), 1, "version")
    elif what == "truncated":
        _refused(lambda: sep.set_state(before[:-8]), 1, "bytes")
        _refused(lambda: sep.set_state(before[:40]), 1, "header")
    elif what == "pending-is-frameshift":
        _refused(lambda: sep.set_state(_patched(before, lay, "pending_count", d["p"]["frameshift"])), 1, "pending")
    else:
        _refused(lambda: sep.set_state(_patched(before, lay, "n_push", -1)), 1, "n_push")
        _refused(lambda: sep.set_state(_patched(before, lay, "update_switch", 0)), 1, "update_switch")
        _refused(lambda: sep.set_state(before[:lay["l"][0]] + np.int64(0).tobytes() + before[lay["l"][0] + 8:]), 1, "l = 0")
    assert sep.get_state()["record"] == before
    res = _run(sep, d, [x[cut:]])
    _assert_same(d, ({key: np.concatenate([o1[key], res[0][key]], axis=-1) for key in _keys(d)}, res[1], res[2]), whole)
    sep.close()


def test_a_flushed_separator_has_no_state_until_it_is_restarted(gpu_ctx):
    d, whole, _, _, st = _case(gpu_ctx, "fp32-dft")
    sep = _make(gpu_ctx, d, 0)
    got = _run(sep, d, [d["pcms"][0]])
    _refused(lambda: sep.get_state(), 7, "flushed")
    _assert_same(d, (got[0], sep.trace(), _final(sep, d)), whole)  # the refusal touched nothing a finished stream still has
    sep.set_state(st)  # a finished separator takes a state ...
    res = _run(sep, d, [d["pcms"][0][d["cut"]:]])
    assert np.array_equal(res[0]["x_tilde_f"], whole[0]["x_tilde_f"][len(whole[0]["x_tilde_f"]) - len(res[0]["x_tilde_f"]):])
    sep.restart()  # ... and a restarted one has one again
    assert sep.get_state()["l"] == 1
    sep.close()
