"""GPU tests of the single-stream online separator's handle (include/snmf.h: snmf_online_*), the same in the fp32 mode
(snmf_online_create) and in the fp64 mode (snmf_online_create_f64): the hop queue between calls, the flush, the roll-back of a
call whose outputs have too little room, the order set_classes asks for, what is refused after a flush, the trace read, and
what each precision's entry does on the other precision's handle.  The host driver of the two modes is one
(csrc/snmf_online_host.h), and these are the cases that run its state machine.

Nothing is compared across the modes or against an oracle here (test_online.py and test_online_f64.py do that): every
comparison is between two runs of the same mode, in bytes.  The geometry is the smallest one test_online.py runs (fft 64,
frame 64, hop 16, R_x = 8, R_d = 12, R_a = 6, m_a = 12, delay 2, _random_setup's dictionaries) on 44 hops of
frontend_audio.npz plus 9 samples: with the 9 samples a partial hop is queued when the flush comes, in the one-call run as in
the runs fed in pieces, and the flush drops it."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FFT, SZ, HOP, R_X, R_D, DELAY = 64, 64, 16, 8, 12, 2
N_HOPS, EXTRA = 44, 9
PRECISIONS = ["fp32", "fp64"]
INVALID, STATE = 1, 7  # SNMF_ERR_INVALID, SNMF_ERR_STATE
PART = ([1, 5], [1, 7])    # EVENT_RANK / NOISE_RANK: 2 event and 2 noise classes
PART_B = ([1, 4], [1, 5])
SIGNALS = ("xt", "i16", "xh", "dh", "xhi", "dhi")


def _setup():
    from se_snmf_nat_amd.online import default_settings
    rs = np.random.RandomState(FFT)  # test_online.py: _random_setup(fft, fft, sz, hop, R_x, R_d)
    B = rs.gamma(0.6, 1.0, (FFT // 2 + 1, R_X + R_D)) + 1e-3
    B = B / np.sqrt((B ** 2).sum(0)) + 1e-9
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(SZ) / SZ))
    p = dict(default_settings(), fftlength=FFT, framelength=SZ, frameshift=HOP, win_STFT=win, win_ISTFT=win.copy(),
             overlapscale=2 * HOP / SZ, R_a=6, m_a=12, overlap_m_a=0.2, Ar_up=2.0, P_len_k=8, P_len_l=4, init_N_len=4, DCbin=1,
             DCbin_back=1, delay=DELAY)
    rs = np.random.RandomState(7)
    H0, Ad0 = rs.random_sample(R_X + R_D), rs.random_sample((p["R_a"], p["m_a"]))
    s = np.load(os.path.join(GOLD, "frontend_audio.npz"))["samples"][:HOP * N_HOPS + EXTRA]
    return B[:, :R_X], B[:, R_X:], p, H0, Ad0, np.asarray(s, dtype=np.float64)


class _Handle:
    """One separator, driven through the C entries: the caller chooses `cap` and sees the status and the whole buffers."""

    def __init__(self, ctx, prec, class_outputs=False, partition=None):
        from se_snmf_nat_amd.online import OnlineSeparator
        Bx, Bd, p, H0, Ad0, self.s = _setup()
        self.sep = OnlineSeparator(Bx, Bd, p, H0=H0, Ad_blk0=Ad0, ctx=ctx, class_outputs=class_outputs, precision=prec)
        self.lib, self.h, self.prec = self.sep._lib, self.sep._h, prec
        self.dt = np.float64 if prec == "fp64" else np.float32
        self.co, self.E, self.N, self.pend, self.l = class_outputs, 1, 1, 0, 0  # (pend: samples queued, l: frames run)
        if partition:
            assert self.set_classes(*partition) == 0

    def set_classes(self, ev, nz):
        ev, nz = np.array(ev, np.int32), np.array(nz, np.int32)
        rc = self.lib.snmf_online_set_classes(self.h, ev.size, ev.ctypes.data, nz.size, nz.ctypes.data)
        if rc == 0:
            self.E, self.N = ev.size, nz.size
        return rc

    def frames(self, n, flush):
        return (self.pend + n) // HOP + (DELAY + 1 if flush else 0)

    def need(self, n, flush):
        """The room a call must offer: every frame it runs, one hop each."""
        return self.frames(n, flush) * HOP

    def returns(self, n, flush):
        """The samples a call returns: the stream's first `delay` frames give none."""
        return max(0, self.frames(n, flush) - max(0, DELAY - self.l)) * HOP

    def feed(self, x, flush=False, cap=None, fill=0, ask=None):
        """-> (status, n_out, {signal: whole buffer}).  `ask`: the outputs to pass (default: all the separator was made for)."""
        x = np.ascontiguousarray(x, dtype=self.dt)
        cap = self.need(x.size, flush) if cap is None else cap
        ask = ask or (SIGNALS if self.co else SIGNALS[:2])
        rows = dict(xhi=self.E, dhi=self.N)
        b = {k: np.full((rows.get(k, 1), max(cap, 1)), fill, np.int16 if k == "i16" else self.dt) for k in ask}
        ptr = lambda k: b[k].ctypes.data if k in b else None  # noqa: E731
        n = C.c_int64(-1)
        sfx = "f64" if self.prec == "fp64" else "f32"
        head = (self.h, x.ctypes.data if x.size else None, x.size, int(flush), ptr("xt"), ptr("i16"), ptr("xh"), ptr("dh"))
        if "xhi" in b or "dhi" in b:
            rc = getattr(self.lib, "snmf_online_process_classes_" + sfx)(*head, ptr("xhi"), ptr("dhi"), cap, C.byref(n))
        else:
            rc = getattr(self.lib, "snmf_online_process_" + sfx)(*head, cap, C.byref(n))
        if rc == 0:
            self.l += self.frames(x.size, flush)
            self.pend = 0 if flush else (self.pend + x.size) % HOP
        return rc, n.value, b

    def result(self, parts):
        """The calls' outputs joined, with the final basis and the trace."""
        out = {k: np.concatenate([q[k] for q in parts], axis=1) for k in parts[0]}
        out["basis"], out["trace"] = self.basis(), self.trace()
        return out

    def basis(self, sfx=None):
        sfx = sfx or ("f64" if self.prec == "fp64" else "f32")
        B = np.zeros((FFT // 2 + 1, R_D), np.float64 if sfx == "f64" else np.float32, order="F")
        assert getattr(self.lib, "snmf_online_get_basis_" + sfx)(self.h, B.ctypes.data, B.shape[0]) == 0
        return B

    def trace(self):
        """The whole trace, as bytes."""
        from se_snmf_nat_amd._lib import SnmfOnlineFrame
        n = C.c_int64(-1)
        assert self.lib.snmf_online_trace(self.h, None, 0, C.byref(n)) == 0  # out = NULL: the count alone
        arr = (SnmfOnlineFrame * max(1, n.value))()
        assert self.lib.snmf_online_trace(self.h, C.cast(arr, C.c_void_p), n.value, C.byref(n)) == 0
        return bytes(arr)[:n.value * C.sizeof(SnmfOnlineFrame)]

    def close(self):
        self.sep.close()


def _feed_checked(hd, x, flush):
    """A call that must succeed and return exactly the hops it completed."""
    want = hd.returns(len(x), flush)
    rc, n, b = hd.feed(x, flush)
    assert rc == 0, hd.lib.snmf_last_error()
    assert n == want, (n, want)
    return {k: v[:, :n] for k, v in b.items()}


def _run(hd, pieces=None, flush_alone=False):
    """The signal in `pieces`-sample calls (None: one call), the flush with the last samples or in a call with n = 0."""
    s = hd.s
    cuts = [s] if pieces is None else [s[i:i + pieces] for i in range(0, len(s), pieces)]
    calls = [(x, not flush_alone and i == len(cuts) - 1) for i, x in enumerate(cuts)] + ([(s[:0], True)] if flush_alone else [])
    return hd.result([_feed_checked(hd, x, fl) for x, fl in calls])


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "trace":
            assert a[k] == b[k], (what, k)
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


KINDS = {"plain": dict(), "one-class-per-side": dict(class_outputs=True), "partition": dict(class_outputs=True, partition=PART)}
_ONE_CALL = {}


def _one_call(ctx, prec, kind="plain"):
    """The whole signal with flush=True on a fresh separator: the reference of the mode, computed once and left unchanged."""
    if (prec, kind) not in _ONE_CALL:
        hd = _Handle(ctx, prec, **KINDS[kind])
        _ONE_CALL[prec, kind] = _run(hd)
        hd.close()
    return _ONE_CALL[prec, kind]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_pieces_give_the_bits_of_one_call(gpu_ctx, prec, kind):
    from se_snmf_nat_amd._lib import SnmfOnlineFrame
    ref = _one_call(gpu_ctx, prec, kind)
    n_frames = N_HOPS + DELAY + 1
    assert ref["xt"].shape == (1, (N_HOPS + 1) * HOP) and len(ref["trace"]) == n_frames * C.sizeof(SnmfOnlineFrame)
    tr = (SnmfOnlineFrame * n_frames).from_buffer_copy(ref["trace"])
    print(prec, kind, "adaptation solves:", sum(t.solved for t in tr))
    assert sum(t.solved for t in tr) > 0 and np.abs(ref["xt"]).max() > 0  # the run adapts its dictionary and is not silent
    if kind != "plain":
        assert ref["xhi"].shape[0] == (2 if kind == "partition" else 1)
        assert np.abs(ref["xh"]).max() > 0 and np.abs(ref["dhi"]).max() > 0
    if kind == "one-class-per-side":  # without a partition the class signals are x_hat / d_hat
        assert ref["xhi"].tobytes() == ref["xh"].tobytes() and ref["dhi"].tobytes() == ref["dh"].tobytes()
    for pieces in (16, 57, 1000):  # whole hops; a partial hop queued between the calls and at the flush; everything, then the flush
        hd = _Handle(gpu_ctx, prec, **KINDS[kind])
        got = _run(hd, pieces, flush_alone=True)
        hd.close()
        _same(got, ref, f"{prec} {kind} pieces of {pieces}")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_a_short_cap_is_refused_and_rolls_the_queue_back(gpu_ctx, prec):
    ref = _one_call(gpu_ctx, prec, "partition")
    hd = _Handle(gpu_ctx, prec, **KINDS["partition"])
    first = _feed_checked(hd, hd.s[:57], False)  # leaves 9 samples queued
    rest = hd.s[57:]
    need = hd.need(len(rest), True)
    fill = 77
    rc, n, b = hd.feed(rest, True, cap=need - 1, fill=fill)
    assert rc == INVALID and n == 0
    assert b"output capacity" in hd.lib.snmf_last_error()
    for k, v in b.items():
        assert (v == fill).all(), k  # nothing was written
    # without the flush too: the refusal looks at what this call would write
    rc, n, b = hd.feed(rest, False, cap=hd.need(len(rest), False) - 1, fill=fill)
    assert rc == INVALID and n == 0 and all((v == fill).all() for v in b.values())
    second = _feed_checked(hd, rest, True)  # the same samples again: had they stayed queued, they would now be there twice
    got = hd.result([first, second])
    hd.close()
    _same(got, ref, f"{prec} after two short caps")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_class_pointers_without_class_outputs_are_refused(gpu_ctx, prec):
    ref = _one_call(gpu_ctx, prec)
    hd = _Handle(gpu_ctx, prec)
    for ask in (("xt", "xh"), ("xt", "dh"), ("xt", "i16", "xhi"), ("dhi",)):
        rc, n, b = hd.feed(hd.s, True, fill=77, ask=ask)
        assert rc == STATE and n == 0, ask
        assert b"class outputs were not requested" in hd.lib.snmf_last_error()
        assert all((v == 77).all() for v in b.values())
    assert hd.set_classes(*PART) == STATE
    got = _run(hd)
    hd.close()
    _same(got, ref, f"{prec} after the refusals")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_set_classes_must_precede_the_first_sample(gpu_ctx, prec):
    msg = b"must precede the first sample"
    hd = _Handle(gpu_ctx, prec, class_outputs=True)
    _feed_checked(hd, hd.s[:HOP], False)  # one frame ran
    assert hd.set_classes(*PART) == STATE and msg in hd.lib.snmf_last_error()
    hd.close()
    hd = _Handle(gpu_ctx, prec, class_outputs=True)
    _feed_checked(hd, hd.s[:5], False)  # a partial hop is queued, no frame ran
    assert hd.set_classes(*PART) == STATE and msg in hd.lib.snmf_last_error()
    hd.close()
    # before the first sample: twice in a row, and the second partition holds
    fresh = _Handle(gpu_ctx, prec, class_outputs=True, partition=PART_B)
    want = _run(fresh)
    fresh.close()
    hd = _Handle(gpu_ctx, prec, class_outputs=True)
    assert hd.set_classes(*PART) == 0 and hd.set_classes(*PART_B) == 0
    got = _run(hd)
    assert hd.set_classes(*PART) == STATE and msg in hd.lib.snmf_last_error()  # and not after the flush
    hd.close()
    _same(got, want, f"{prec} second partition")
    ref = _one_call(gpu_ctx, prec, "partition")
    assert got["xhi"].tobytes() != ref["xhi"].tobytes() and got["xh"].tobytes() == ref["xh"].tobytes()  # other classes, same sums


@pytest.mark.parametrize("prec", PRECISIONS)
def test_after_the_flush_only_the_reads_work(gpu_ctx, prec):
    ref = _one_call(gpu_ctx, prec)
    hd = _Handle(gpu_ctx, prec)
    got = _run(hd)
    for x, fl in ((hd.s[:HOP], False), (hd.s[:0], False), (hd.s[:0], True)):
        rc, n, b = hd.feed(x, fl, cap=10 * HOP, fill=77)
        assert rc == STATE and n == 0 and b"the stream was flushed" in hd.lib.snmf_last_error()
        assert all((v == 77).all() for v in b.values())
    again = dict(got, basis=hd.basis(), trace=hd.trace())
    hd.close()
    _same(got, ref, f"{prec} one call")
    _same(again, ref, f"{prec} reads after the refusals")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_bad_arguments_are_refused_and_harm_nothing(gpu_ctx, prec):
    ref = _one_call(gpu_ctx, prec)
    hd = _Handle(gpu_ctx, prec)
    first = _feed_checked(hd, hd.s[:57], False)
    sfx = "f64" if prec == "fp64" else "f32"
    process = getattr(hd.lib, "snmf_online_process_" + sfx)
    of = np.full(100 * HOP, 77, hd.dt)
    x = np.ascontiguousarray(hd.s[57:], dtype=hd.dt)
    for pcm, n_in in ((x.ctypes.data, -1), (None, x.size)):
        n = C.c_int64(-1)
        assert process(hd.h, pcm, n_in, 0, of.ctypes.data, None, None, None, of.size, C.byref(n)) == INVALID
        assert n.value == 0 and (of == 77).all()
    got = hd.result([first, _feed_checked(hd, hd.s[57:], True)])
    hd.close()
    _same(got, ref, f"{prec} after the refusals")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_trace_count_and_a_short_read(gpu_ctx, prec):
    from se_snmf_nat_amd._lib import SnmfOnlineFrame
    ref = _one_call(gpu_ctx, prec)
    rec = C.sizeof(SnmfOnlineFrame)
    hd = _Handle(gpu_ctx, prec)
    n = C.c_int64(-1)
    assert hd.lib.snmf_online_trace(hd.h, None, 0, C.byref(n)) == 0 and n.value == 0  # nothing ran yet
    _run(hd)
    assert hd.lib.snmf_online_trace(hd.h, None, 10, C.byref(n)) == 0 and n.value == N_HOPS + DELAY + 1
    arr = (SnmfOnlineFrame * 12)()
    C.memset(arr, 0x5A, C.sizeof(arr))
    assert hd.lib.snmf_online_trace(hd.h, C.cast(arr, C.c_void_p), 10, C.byref(n)) == 0
    assert n.value == N_HOPS + DELAY + 1  # the count, not what was copied
    assert bytes(arr)[:10 * rec] == ref["trace"][:10 * rec] and bytes(arr)[10 * rec:] == b"\x5a" * (2 * rec)
    assert hd.lib.snmf_online_trace(hd.h, C.cast(arr, C.c_void_p), 12, None) == 0  # n = NULL
    assert bytes(arr) == ref["trace"][:12 * rec]
    hd.close()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_the_other_precisions_entries(gpu_ctx, prec):
    """Pinned as it is: process_f64 wants an fp64 handle; process_f32 on an fp64 handle rounds the fp64 outputs; both
    get_basis entries work on both kinds."""
    ref = _one_call(gpu_ctx, prec)
    hd = _Handle(gpu_ctx, prec)
    need = hd.need(len(hd.s), True)
    n = C.c_int64(-1)
    if prec == "fp32":
        x = np.ascontiguousarray(hd.s, dtype=np.float64)
        of = np.full(need, 77.0)
        assert hd.lib.snmf_online_process_f64(hd.h, x.ctypes.data, x.size, 1, of.ctypes.data, None, None, None, need, C.byref(n)) == STATE
        assert n.value == 0 and (of == 77).all()
        xhi = np.full(need, 77.0)
        assert hd.lib.snmf_online_process_classes_f64(hd.h, x.ctypes.data, x.size, 1, of.ctypes.data, None, None, None, xhi.ctypes.data,
                                                      None, need, C.byref(n)) == STATE
        assert n.value == 0 and (of == 77).all() and (xhi == 77).all()
        got = _run(hd)
        _same(got, ref, "fp32 after process_f64 was refused")
        B64 = hd.basis("f64")  # the fp32 separator's fp64 master
        assert B64.dtype == np.float64 and B64.astype(np.float32).tobytes() == ref["basis"].tobytes()
    else:
        x = np.ascontiguousarray(hd.s, dtype=np.float32)  # (integer-valued PCM: exact in fp32)
        of, o16 = np.zeros(need, np.float32), np.zeros(need, np.int16)
        assert hd.lib.snmf_online_process_f32(hd.h, x.ctypes.data, x.size, 1, of.ctypes.data, o16.ctypes.data, None, None, need, C.byref(n)) == 0
        m = n.value
        assert m == ref["xt"].shape[1] == need - DELAY * HOP
        assert of[:m].tobytes() == ref["xt"][0].astype(np.float32).tobytes() and o16[:m].tobytes() == ref["i16"][0].tobytes()
        assert hd.basis("f32").tobytes() == np.asfortranarray(ref["basis"].astype(np.float32)).tobytes()
        assert hd.basis("f64").tobytes() == ref["basis"].tobytes() and hd.trace() == ref["trace"]
    hd.close()
