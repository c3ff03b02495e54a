"""The spectrogram front-end over everything its C ABI accepts, in both modes (snmf_*_f32 and snmf_*_fp64 of include/snmf.h):
every FFT size, padded leading dimensions, host- and device-resident samples / matrices, in-place TF_DD, every refusal of
validate_stft.  The entries are called with ctypes, as the training callers and the MEX shims call them; device buffers are
torch tensors.  Cases, signals and CPU references: tests/frontend_envelope.py (checked on the CPU by
tests/test_frontend_envelope_cpu.py).

Which kernel instantiation a case reaches: every case of frontend_envelope.STFT_CASES runs with f32 and with fp64, so the
case named n<N>_... launches k_stft<log2 N> and k_stft64<log2 N>:
    k_stft<6>  / k_stft64<6>    n64_full_shift9_pow2  n64_len1_shift1_pow1  n64_splice1_T1  n64_splice2_T1  (+ frame-count edges,
                                 refusals, snmf_plan_set_v_from_audio_f32 at F = 33 and 99)
    k_stft<7>  / k_stft64<7>    n128_alldc  n128_splice2_T2
    k_stft<8>  / k_stft64<8>    n256_shiftN_pow07_splice1_T5
    k_stft<9>  / k_stft64<9>    n512_pow05_splice2_T5  (+ frame-count edges)
    k_stft<10> / k_stft64<10>   n1024_odd_len_shift1_pow1
    k_stft<11> / k_stft64<11>   n2048_splice1_T2  n2048_len1_shiftN_pow05
    k_stft<12> / k_stft64<12>   n4096_full_shift513_pow2  n4096_odd_len_shiftN_pow05   (64 KB static / 128 KB dynamic LDS)

Bounds.  None is read off the device.
    STFT f32     |err| <= 1e-4 |ref| + 2e-6 colmax, the bound of tests/test_frontend.py.  A single-precision restatement of the chain
                 (float32 window, complex64 FFT) stays within 0.046 of it on every case (tests/test_frontend_envelope_cpu.py).
    STFT fp64    |err| <= a |ref| + b colmax, (a, b) = (8e-14, 8e-14): the smallest response of the fp64 reference to a 1e-12
                 relative perturbation of the samples over these cases (scripts/train_f64_sensitivity.py --envelope ->
                 profiles/train_f64_sensitivity.md: a >= 8.4e-14, b >= 8.5e-14).  n128_alldc (every bin is the DC value) has no
                 response; it is held to the same figures, four orders above the spacing of doubles.
    Mel          all terms are non-negative, so a sequential sum of w terms is within (w + 1) eps ref of the exact one: w = the
                 widest filter's non-zero count, from the table; eps = 2^-23 (f32: covers the table rounded to float) / 2^-52.
    TF_DD        f32: 2e-7 |ref| + 1e-7 rowmax (tests/test_frontend.py); fp64: AB_TFDD of tests/test_gpu_train_f64.py.
    bit-equal    padded == tight, device-resident == host, in place == out of place, set_v_from_audio == set_v(features), the
                 output with the unread tail of the samples replaced by NaN, pad rows == the sentinel: every sum has a fixed order.
The reference of the cases with T <= Splice is frontend_envelope.features: the oracle's splice loop cannot index them.

Measured: every test prints max err/bound before it asserts.  No figure from an MI355X is recorded here yet.  The same
arithmetic restated on the CPU (radix-2 Stockham butterflies with twiddles rounded to the mode's type) gives, as an expectation
and not a measurement: STFT f32 <= 0.081 of the bound (n4096_odd_len_shiftN_pow05), STFT fp64 <= 0.013 (same case), Mel <= 0.13 of
the bound, TF_DD fp64 0.
"""
import ctypes as C

import numpy as np
import pytest

import frontend_envelope as env
from oracle import frontend_oracle as fo

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 8  # SNMF_OK, SNMF_ERR_INVALID, SNMF_ERR_UNSUPPORTED (include/snmf.h)
MODES = ("f32", "fp64")
AB_STFT = {"f32": (1e-4, 2e-6), "fp64": (8e-14, 8e-14)}
AB_TFDD = {"f32": (2e-7, 1e-7), "fp64": (2.7e-12, 1.2e-12)}
EPS = {"f32": 2.0 ** -23, "fp64": 2.0 ** -52}
SENT = -777.25  # what every buffer holds before a call; no feature is negative


def np_t(mode):
    return np.float32 if mode == "f32" else np.float64


def judge(what, got, ref, scale, ab):
    """|err| <= a |ref| + b scale, element-wise; prints the error in units of the bound first."""
    a, b = ab
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    bound = a * np.abs(ref) + b * scale
    print(f"front-end envelope {what}: max err/bound = {float((err / bound).max()):.2e}  max err/scale = {float((err / scale).max()):.2e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), float((err / bound).max())


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def ptr(a):
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def sync():
    import torch
    torch.cuda.synchronize()


def filled(n, dt):
    return np.full(n, SENT, dtype=dt)


def columns(buf, rows, ld, T):
    """(the rows x T matrix of a flat column-major buffer with leading dimension ld, everything else of the buffer)"""
    buf = np.asarray(buf)
    keep = np.zeros(buf.size, bool)
    for t in range(T):
        keep[t * ld:t * ld + rows] = True
    return buf[keep].reshape(T, rows).T, buf[~keep]


def only_sentinel(rest):
    return rest.size > 0 and (rest == SENT).all()


class Stft:
    """snmf_stft_features_<mode> through ctypes; host or device samples / output, any leading dimension."""

    def __init__(self, lib, ctx, mode, p):
        from se_snmf_nat_amd import frontend as fe
        self.fn = getattr(lib, "snmf_stft_features_" + mode)
        self.ctx, self.dt, self.p = ctx, np_t(mode), p
        self.sp, self._win = fe._params(p)
        self.F = (2 * p["Splice"] + 1) * (p["fftlength"] // 2 + 1)

    def __call__(self, s, ld=None, dev=False, cols=None):
        """-> (status, n_frames_out, the flat output buffer of ld * cols + 7 elements)"""
        ld = self.F if ld is None else ld
        cols = max(self.p.get("T", 1), 1) if cols is None else cols
        s = np.ascontiguousarray(s, dtype=self.dt)
        out = filled(ld * cols + 7, self.dt)
        n = C.c_int32(-5)
        if dev:
            ds, do = to_dev(s), to_dev(out)
            sync()
            rc = self.fn(self.ctx._h, C.byref(self.sp), ptr(ds), s.size, 1, ptr(do), ld, 1, C.byref(n))
            out = do.cpu().numpy()
        else:
            sync()
            rc = self.fn(self.ctx._h, C.byref(self.sp), ptr(s), s.size, 0, ptr(out), ld, 0, C.byref(n))
        return rc, n.value, out


# ---- 1. / 2. STFT: every size, both modes, layouts and residency ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(env.STFT_CASES))
@pytest.mark.parametrize("mode", MODES)
def test_stft_at_every_size_layout_and_residency(gpu_ctx, lib, mode, name):
    p, s, ref = env.STFT_CASES[name], env.case_signal(name), env.case_reference(name)
    call = Stft(lib, gpu_ctx, mode, p)
    F, T = ref.shape
    rc, n, buf = call(s)
    assert (rc, n) == (OK, T) and buf.dtype == np_t(mode)
    got, rest = columns(buf, F, F, T)
    assert only_sentinel(rest)
    judge(f"stft {mode} {name}", got, ref, env.colmax(ref, p), AB_STFT[mode])
    for dev, ld in ((False, F + 3), (True, F), (True, F + 5)):
        rc, n, buf = call(s, ld=ld, dev=dev)
        assert (rc, n) == (OK, T), (dev, ld)
        again, rest = columns(buf, F, ld, T)
        assert bits(again) == bits(got), (dev, ld)
        assert only_sentinel(rest), (dev, ld)  # rows F .. ld-1 of every column and everything after the last column's F entries
    tail = s.copy()
    tail[(T - 1) * p["frameshift"] + p["framelength"]:] = np.nan  # the samples no frame reads
    assert np.isnan(tail).sum() >= 2
    rc, n, buf = call(tail)
    assert (rc, n) == (OK, T) and bits(columns(buf, F, F, T)[0]) == bits(got)


@pytest.mark.parametrize("N", [64, 512])
@pytest.mark.parametrize("mode", MODES)
def test_stft_frame_count_edges(gpu_ctx, lib, mode, N):
    """L - N = 1, 2, 1 + shift, 2 + shift, 3 + shift: 0, 1, 1, 2 and 2 frames (a frame starts wherever 1 + i * shift < L - N, so
    the second one appears at 2 + shift); the zero-frame call returns OK and writes nothing."""
    shift = N // 8 + 1
    p = env.case(N, N // 2 + 3, shift, 2, 0.92, 1, 0, 1)
    call = Stft(lib, gpu_ctx, mode, p)
    F = call.F
    for extra, T in ((1, 0), (2, 1), (1 + shift, 1), (2 + shift, 2), (3 + shift, 2)):
        s = env.signal(N + extra, 40 + extra)
        ref = env.features(s, p)
        assert ref.shape == (F, T)
        for dev in (False, True):
            rc, n, buf = call(s, dev=dev, cols=2)
            assert (rc, n) == (OK, T), (extra, dev)
            got, rest = columns(buf, F, F, T)
            assert only_sentinel(rest)
            if T:
                judge(f"stft {mode} N={N} L-N={extra} dev={dev}", got, ref, env.colmax(ref, p), AB_STFT[mode])
            else:
                assert rest.size == buf.size


@pytest.mark.parametrize("splice", [0, 1], ids=["F33", "F99"])
@pytest.mark.parametrize("full", [False, True], ids=["h_only", "full_update"])
def test_plan_v_from_audio_equals_set_v_at_small_f(gpu_ctx, lib, splice, full):
    """snmf_plan_set_v_from_audio_f32 at F = 33 and 99 (fftlength 64): W, H and the objective of a 5-iteration solve are the
    bits of the same plan fed by set_v(stft_features(...)); samples on the host and on the device."""
    from se_snmf_nat_amd import Plan, frontend as fe
    p = env.case(64, 64, 16, 2, 0.0, 2, splice, 45)
    s = np.ascontiguousarray(env.signal(env.n_samples(p), 77), dtype=np.float32)
    V = fe.stft_features(s, p, ctx=gpu_ctx)
    F, T, r = V.shape[0], V.shape[1], 6
    assert (F, T) == (33 * (2 * splice + 1), 45)
    rs = np.random.RandomState(9)
    W0, H0 = rs.rand(F, r) + 0.05, rs.rand(r, T)
    sp, _win = fe._params(p)

    def from_audio(plan, dev):
        ds = to_dev(s) if dev else s
        sync()
        assert lib.snmf_plan_set_v_from_audio_f32(plan._h, C.byref(sp), ptr(ds), s.size, int(dev)) == OK

    def solve(feed):
        plan = Plan(gpu_ctx, F, T, r, beta=1.0, max_iter=5, conv_eps=0.0, cost_check=True, sparsity=5.0,
                    w_update_ind=np.full(r, full, bool))
        feed(plan)
        plan.set_w(W0); plan.set_h(H0); plan.init(); plan.run()
        w, h = plan.get_w(), plan.get_h()
        div, cost, n = plan.get_objective()
        plan.close()
        return w, h, np.asarray(div)[:n], np.asarray(cost)[:n]

    base = solve(lambda plan: plan.set_v(V))
    assert np.isfinite(base[1]).all() and (not full or not np.array_equal(base[0], W0))
    for dev in (False, True):
        other = solve(lambda plan: from_audio(plan, dev))
        for a, b, what in zip(base, other, ("W", "H", "div", "cost")):
            assert bits(a) == bits(b), (what, dev)


# ---- 3. Mel projection ---------------------------------------------------------------------------------------------------
MEL_CASES = [(64, 80, 1, 7), (64, 1, 5, 1), (64, 23, 3, 7), (1024, 23, 3, 7), (1024, 64, 1, 1), (1024, 1, 5, 7),
             (4096, 64, 3, 7), (4096, 80, 5, 1), (4096, 1, 1, 7)]  # fftlength, M, K, T


@pytest.mark.parametrize("N,M,K,T", MEL_CASES)
@pytest.mark.parametrize("mode", MODES)
def test_mel_projection_layouts_and_residency(gpu_ctx, lib, mode, N, M, K, T):
    dt = np_t(mode)
    n = N // 2 + 1
    p = dict(fs=env.FS, fftlength=N, F_order=M, Splice=(K - 1) // 2)
    rs = np.random.RandomState(N + M + K + T)
    V = (rs.gamma(0.5, 1.0, (K * n, T)) * 10.0 ** rs.uniform(-2, 2, (K * n, 1))).astype(dt)
    table = fo.mel_matrix(env.FS, M, N, 1.0, env.FS / 2).T  # M x n, not the product's mel_matrix
    assert table.shape == (M, n) and table.min() >= 0
    w = int((table != 0).sum(1).max())
    ref = fo.mel_features(V.astype(np.float64), p)
    mel = np.ascontiguousarray(table, dtype=dt)
    fn = getattr(lib, "snmf_mel_features_" + mode)
    rv, ro = K * n, K * M

    def call(ldv, ldo, dev):
        vin = np.full(ldv * T, np.nan, dtype=dt)  # a pad row that is read poisons the output
        for t in range(T):
            vin[t * ldv:t * ldv + rv] = V[:, t]
        out = filled(ldo * T + 7, dt)
        if dev:
            dv, do = to_dev(vin), to_dev(out)
            sync()
            rc = fn(gpu_ctx._h, ptr(mel), M, n, K, ptr(dv), ldv, T, ptr(do), ldo, 1)
            assert bits(dv.cpu().numpy()) == bits(vin)
            out = do.cpu().numpy()
        else:
            sync()
            rc = fn(gpu_ctx._h, ptr(mel), M, n, K, ptr(vin), ldv, T, ptr(out), ldo, 0)
        assert rc == OK, (ldv, ldo, dev)
        got, rest = columns(out, ro, ldo, T)
        assert only_sentinel(rest), (ldv, ldo, dev)
        return got

    got = call(rv, ro, False)
    err = np.abs(got.astype(np.float64) - ref)
    bound = (w + 1) * EPS[mode] * ref
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"front-end envelope mel {mode} N={N} M={M} K={K} T={T}: widest filter {w}, max err/bound = {worst:.2e}")
    assert got.dtype == dt and ref.max() > 0 and (err <= bound).all(), worst
    for ldv, ldo, dev in ((rv + 2, ro + 3, False), (rv, ro, True), (rv + 2, ro + 3, True)):
        assert bits(call(ldv, ldo, dev)) == bits(got), (ldv, ldo, dev)


# ---- 4. TF_DD --------------------------------------------------------------------------------------------------------------
TFDD_SHAPES = [(1, 513), (255, 2), (256, 257), (257, 256), (257, 1), (256, 255), (255, 513), (1, 1)]


@pytest.mark.parametrize("F,T", TFDD_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_tf_dd_layouts_residency_and_in_place(gpu_ctx, lib, mode, F, T):
    dt = np_t(mode)
    rs = np.random.RandomState(F + T)
    X = (rs.gamma(0.5, 1.0, (F, T)) * 10.0 ** rs.uniform(-3, 3, (F, 1))).astype(dt)
    fn = getattr(lib, "snmf_tf_dd_" + mode)
    alpha = 0.95 if T > 500 else 0.4

    def strided(ld, pad):
        a = np.full(ld * T + 5, pad, dtype=dt)
        for t in range(T):
            a[t * ld:t * ld + F] = X[:, t]
        return a

    def call(a, ldx, ldo, where):
        """where: 'host', 'dev' (out of place) or 'inplace' (out == X on the device) -> the F x T result"""
        xin = strided(ldx, np.nan)
        out = filled(ldo * T + 5, dt)
        if where == "host":
            sync()
            rc = fn(gpu_ctx._h, a, F, T, ptr(xin), ldx, ptr(out), ldo, 0)
        elif where == "dev":
            dx, do = to_dev(xin), to_dev(out)
            sync()
            rc = fn(gpu_ctx._h, a, F, T, ptr(dx), ldx, ptr(do), ldo, 1)
            assert bits(dx.cpu().numpy()) == bits(xin)  # X is read only
            out = do.cpu().numpy()
        else:
            assert ldx == ldo
            xin = strided(ldx, SENT)
            dx = to_dev(xin)
            sync()
            rc = fn(gpu_ctx._h, a, F, T, ptr(dx), ldx, ptr(dx), ldx, 1)
            out = dx.cpu().numpy()
        assert rc == OK, (a, ldx, ldo, where)
        got, rest = columns(out, F, ldo, T)
        assert only_sentinel(rest), (a, ldx, ldo, where)
        assert bits(got[:, 0]) == bits(X[:, 0]), (a, ldx, ldo, where)  # the first column is the input's
        return got

    ref = fo.tf_dd(X.astype(np.float64), {"alpha_eta": alpha})
    got = call(alpha, F, F, "host")
    judge(f"tf_dd {mode} {F}x{T}", got, ref, np.abs(ref).max(axis=1, keepdims=True), AB_TFDD[mode])
    for ldx, ldo, where in ((F + 2, F + 3, "host"), (F, F, "dev"), (F + 2, F + 3, "dev"), (F, F, "inplace"), (F + 2, F + 2, "inplace")):
        assert bits(call(alpha, ldx, ldo, where)) == bits(got), (ldx, ldo, where)
    for where in ("host", "inplace"):
        assert bits(call(0.0, F, F, where)) == bits(X), where  # alpha_eta = 0: the input itself
        assert bits(call(1.0, F, F, where)) == bits(np.repeat(X[:, :1], T, axis=1)), where  # alpha_eta = 1: the first column, held


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_refusal_names_its_code_and_leaves_the_context_usable(gpu_ctx, lib, mode):
    dt = np_t(mode)
    N = 64
    good = env.case(N, 35, 9, 2, 0.92, 0.7, 1, 4)
    s = env.signal(env.n_samples(good), 5)
    F = 3 * (N // 2 + 1)

    def stft(ld=None, **over):
        p = dict(good, **over)
        if "win_STFT" not in over:
            p["win_STFT"] = env.window(p["framelength"])
        call = Stft(lib, gpu_ctx, mode, p)
        if over.get("null_window"):
            call.sp.window = None
        big = env.signal(8192 + 40, 5) if p["fftlength"] > N else s
        return call(big, ld=F if ld is None else ld, cols=8)

    before = stft()
    assert before[:2] == (OK, 4)
    for N_bad in (32, 96, 8192):
        assert stft(fftlength=N_bad, framelength=16, DCbin=1)[0] == UNSUPPORTED, N_bad
    assert stft(framelength=N + 1)[0] == INVALID
    assert stft(frameshift=0)[0] == INVALID
    assert stft(DCbin=N // 2 + 2)[0] == INVALID
    assert stft(Splice=-1)[0] == INVALID
    assert stft(null_window=True)[0] == INVALID
    assert stft(ld=F - 1)[0] == INVALID
    assert stft(DCbin=0)[0] == UNSUPPORTED

    mel_fn, dd_fn = getattr(lib, "snmf_mel_features_" + mode), getattr(lib, "snmf_tf_dd_" + mode)
    n, M, K, T = 33, 23, 3, 4
    table = np.ascontiguousarray(fo.mel_matrix(env.FS, M, N, 1.0, env.FS / 2).T, dtype=dt)
    V = np.ones(K * n * T, dtype=dt)
    out = filled(K * M * T, dt)
    sync()
    assert mel_fn(gpu_ctx._h, ptr(table), M, n, K, ptr(V), K * n - 1, T, ptr(out), K * M, 0) == INVALID
    assert mel_fn(gpu_ctx._h, ptr(table), 0, n, K, ptr(V), K * n, T, ptr(out), K * M, 0) == INVALID
    X = np.ones(7 * 5, dtype=dt)
    o2 = filled(7 * 5, dt)
    assert dd_fn(gpu_ctx._h, float("nan"), 7, 5, ptr(X), 7, ptr(o2), 7, 0) == INVALID
    assert dd_fn(gpu_ctx._h, 0.4, 7, 5, ptr(X), 6, ptr(o2), 7, 0) == INVALID
    assert (out == SENT).all() and (o2 == SENT).all()  # a refused call writes nothing

    after = stft()
    assert after[:2] == (OK, 4) and bits(after[2]) == bits(before[2])
    assert mel_fn(gpu_ctx._h, ptr(table), M, n, K, ptr(V), K * n, T, ptr(out), K * M, 0) == OK
    np.testing.assert_allclose(columns(out, K * M, K * M, T)[0][:M, 0], table.sum(1), rtol=(n + 1) * EPS[mode])
