"""Host-side mirror of the online separation path (BASELINE config 3).

    g = init_buff(B_Mel_x, B_Mel_d, B_DFT_x, B_DFT_d, p)                   <->  src/init_buff.m:1
    [x_hat_i, d_hat_i, x_tilde, g] = bnmf_sep_event_RT_IS16(y, l, g, p)     <->  src/bnmf_sep_event_RT_IS16.m:1
    NTF_sep_event_RT(path_in, ..., B_DFT_x, B_DFT_d, p)                     <->  src/NTF_sep_event_RT.m:1

`OnlineSeparator` owns the state `g` on the device (snmf_online in include/snmf.h); `process(pcm)` is
the frame loop of the driver for as many hops as `pcm` holds -- framing, STFT, the per-frame solve, the
gain, the noise-dictionary adaptation, inverse STFT and overlap-add all run in libsnmf_hip.so.
`ntf_sep_event_rt` is the file-level call.  Parameter names are the reference's
(settings/initial_setting_SNMF_NAT.m); `default_settings()` returns the shipped values.

Scope = the configuration the reference ships: blk_len_sep = 1, Splice = 0, one channel; B_sep_mode 'DFT'
(shipped) or 'Mel' (MelConv 0/1); supervised or semi-supervised frame solve.  Anything else raises.
MATLAB's global-RNG draws (rand(r,1) per frame solve, rand(R_a, m_a) in init_buff) are explicit
arguments `H0` / `Ad_blk0` (default: numpy RandomState(random_seed) stand-ins).

Class outputs: `p.EVENT_RANK` / `p.NOISE_RANK` (optional `p.EVENT_NUM` / `p.NOISE_NUM`; settings/initial_setting_SNMF_NAT.m:40-44)
cut the two dictionaries into classes of consecutive columns, and with `class_outputs=True` every separator here also
returns the per-class estimates `x_hat_i` [E, n] / `d_hat_i` [N, n] (src/bnmf_sep_event_RT_IS16.m:158-202, :350-361).  The
shipped partition -- one class per side -- is x_hat / d_hat themselves and runs nothing extra.

`OnlineSeparator(..., precision="fp64")` is the fp64 mode (snmf_online_create_f64): every array crosses in float64 and every
step from PCM to the fed-back dictionary runs in fp64 on the device, so the separator holds the fp64 reference's per-frame
decisions over whole recordings (docs/WIDENING.md, "Parity horizon").  DFT mode and the supervised frame solve only.

`OnlineBatchSeparator(..., precision="fp64")`, `ntf_sep_event_rt_batch(..., precision="fp64")` and
`ntf_sep_event_rt_chains(..., precision="fp64")` are the same mode for many streams (snmf_online_batch_create_f64): every
stream holds its own fp64 reference run's decisions, also over a chain of files with the adapted dictionary carried.  It
covers B_sep_mode 'DFT', the supervised frame solve, every cf / beta_div, Wiener / MMSE, block sparsity, adaptation on or
off, class outputs, restart and chains; it refuses (SnmfError 8) B_sep_mode 'Mel', basis_update_N / basis_update_E and, with
adaptation, a ring beyond R_a <= 64, m_a <= 128.

Settings per stream (fp64 batch only): `OnlineBatchSeparator(..., precision="fp64", settings=[...])` takes a list of S dicts of
overrides on `p`, and `B_DFT_x` as a list of S event dictionaries, so that one batch enhances a corpus under several settings
files, or with the (B_x, B_d) pairs run_basis_dnmf_batch re-trained per noise type.  A stream may have its own cf / beta_div,
sparsity, conv_eps, max_iter, ENHANCE_METHOD, init_N_len, alpha_eta, alpha_d, beta, beta_max, blk_sparse, P_len_k, blk_gap,
alpha_p, adapt_train_N, overlap_m_a and Ar_up; every other key is the batch's geometry and an entry that changes one raises
SnmfError(1) naming it.  Each stream's bits are those of a batch of one with its pair and its settings.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SnmfError, SnmfOnlineFrame, SnmfOnlineParams, SnmfOnlineStreamSettings
from .api import default_context

__all__ = ["default_settings", "OnlineSeparator", "ntf_sep_event_rt", "ntf_sep_event_rt_chain", "OnlineBatchSeparator",
           "ntf_sep_event_rt_batch", "ntf_sep_event_rt_chains"]


def default_settings():
    """settings/initial_setting_SNMF_NAT.m: the fields the online path reads."""
    fs = 16000
    framelength = int(round(0.040 * fs))
    frameshift = int(round(0.010 * fs))
    fftlength = 2 ** int(np.ceil(np.log2(framelength)))
    n = np.arange(framelength)
    win = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / framelength))  # sqrt(hann(N,'periodic'))
    dcbin = int(np.floor(80 / (fs / fftlength) + 0.5))
    return dict(
        fs=fs, framelength=framelength, frameshift=frameshift, fftlength=fftlength, win_STFT=win, win_ISTFT=win.copy(),
        overlapscale=2 * frameshift / framelength, pow=2, preemph=0.0, DCbin=dcbin, DCbin_back=dcbin,
        nonzerofloor=1e-9, Splice=0, blk_len_sep=1, delay=0 + 1 + int(np.floor(0.040 / 0.010 / 2 + 0.5)),
        B_sep_mode="DFT", MelConv=1, F_order=64, basis_update_N=0, basis_update_E=0,
        adapt_train_N=1, init_N_len=15, R_a=50, m_a=100, overlap_m_a=0.01, Ar_up=1.0,
        blk_sparse=1, P_len_k=60, P_len_l=20, alpha_p=0.4, blk_gap=3,
        ENHANCE_METHOD="MMSE", alpha_eta=0.4, alpha_d=0.6, beta=1.0, beta_max=1000.0,
        cf="kl", sparsity=5, max_iter=100, conv_eps=1e-3, cost_check=1, random_seed=1,
        EVENT_NUM=1, EVENT_RANK=[1], NOISE_NUM=1, NOISE_RANK=[1],  # :40-44: one class per side
    )


def _beta_div(p):
    cf = p.get("cf", "kl")
    return {"is": 0.0, "kl": 1.0, "ed": 2.0}.get(cf, float(p.get("beta_div", 1.0)))  # src/sparse_nmf.m:99-110


def _online_params(p, R_x, R_d, adapt, R_a, m_a, method, class_outputs):
    """settings/initial_setting_SNMF_NAT.m -> snmf_online_params (shared by OnlineSeparator and OnlineBatchSeparator)."""
    q = SnmfOnlineParams()
    q.fftlength, q.framelength, q.frameshift = int(p["fftlength"]), int(p["framelength"]), int(p["frameshift"])
    q.dcbin, q.dcbin_back, q.delay = int(p["DCbin"]), int(p.get("DCbin_back", p["DCbin"])), int(p["delay"])
    q.preemph, q.pow, q.nonzerofloor = float(p.get("preemph", 0.0)), float(p.get("pow", 2)), float(p.get("nonzerofloor", 1e-9))
    q.overlapscale = float(p["overlapscale"])
    q.R_x, q.R_d = R_x, R_d
    q.beta_div, q.sparsity = _beta_div(p), float(p.get("sparsity", 0))
    q.max_iter, q.cost_check, q.conv_eps = int(p.get("max_iter", 100)), int(bool(p["cost_check"])), float(p.get("conv_eps", 0))
    q.enhance_method = 0 if method == "Wiener" else 1
    q.init_N_len = int(p.get("init_N_len", 0))
    q.alpha_eta, q.alpha_d = float(p.get("alpha_eta", 0.4)), float(p.get("alpha_d", 0.6))
    q.beta, q.beta_max = float(p.get("beta", 1.0)), float(p.get("beta_max", 1000.0))
    q.blk_sparse = int(bool(p.get("blk_sparse", 0)))
    q.P_len_k, q.P_len_l, q.blk_gap = int(p.get("P_len_k", 60)), int(p.get("P_len_l", 20)), int(p.get("blk_gap", 3))
    q.alpha_p = float(p.get("alpha_p", 0.4))
    q.adapt_train_N, q.R_a, q.m_a = adapt, R_a, m_a
    q.overlap_m_a, q.Ar_up = float(p.get("overlap_m_a", 0.01)), float(p.get("Ar_up", 1.0))
    q.class_outputs = int(bool(class_outputs))
    q.basis_update_N, q.basis_update_E = int(bool(p.get("basis_update_N", 0))), int(bool(p.get("basis_update_E", 0)))
    return q


# the keys of p a stream of an fp64 batch may have of its own (snmf_online_stream_settings); every other key is shared
_STREAM_KEYS = ("cf", "beta_div", "sparsity", "conv_eps", "max_iter", "ENHANCE_METHOD", "init_N_len", "alpha_eta", "alpha_d", "beta",
                "beta_max", "blk_sparse", "P_len_k", "blk_gap", "alpha_p", "adapt_train_N", "overlap_m_a", "Ar_up")
_STREAM_FIELDS = tuple(f for f, _ in SnmfOnlineStreamSettings._fields_)


def _stream_settings(p, settings, n, what="stream"):
    """`settings` (None, one dict for all, or a list of n dicts of overrides on `p`) -> n merged settings dicts.  Raised here,
    before the library is loaded: SnmfError(8) for an entry that asks for what the fp64 batch does not run, SnmfError(1) for
    one that changes a key the streams share (the message names it)."""
    if settings is None:
        entries = [{}] * n
    elif isinstance(settings, dict):
        entries = [settings] * n
    else:
        entries = list(settings)
        if len(entries) != n:
            raise _invalid(f"settings: {len(entries)} entries for {n} {what}s")
    out = []
    for k, e in enumerate(entries):
        if not isinstance(e, dict):
            raise _invalid(f"settings of {what} {k} is not a dict")
        for key in ("basis_update_N", "basis_update_E"):
            if e.get(key, 0):
                raise SnmfError(8, f"settings of {what} {k}: semi-supervised frame solves ({key}) are not supported")
        if e.get("B_sep_mode", "DFT") == "Mel":
            raise SnmfError(8, f"settings of {what} {k}: B_sep_mode 'Mel' is not supported")
        for key, v in e.items():
            if key in _STREAM_KEYS:
                continue
            if key not in p or not np.array_equal(np.asarray(v), np.asarray(p[key])):
                raise _invalid(f"settings of {what} {k} change the shared key {key!r}")
        m = dict(p)
        m.update(e)
        if m.get("ENHANCE_METHOD", "MMSE") not in ("Wiener", "MMSE"):
            raise ValueError("ENHANCE_METHOD must be 'Wiener' or 'MMSE'")
        out.append(m)
    return out


def _settings_struct(m, q):
    """One merged settings dict -> snmf_online_stream_settings, through the conversions of _online_params (q: the batch's)."""
    qk = _online_params(m, q.R_x, q.R_d, int(bool(m.get("adapt_train_N", 0))), q.R_a, q.m_a, m.get("ENHANCE_METHOD", "MMSE"), q.class_outputs)
    st = SnmfOnlineStreamSettings()
    for f in _STREAM_FIELDS:
        setattr(st, f, getattr(qk, f))
    return st


_MAX_CLASSES = 32  # per side (kOClassMax, csrc/snmf_online.h)


def _class_partition(p, R_x, R_d):
    """p.EVENT_RANK / p.NOISE_RANK (1-based class starts, src/bnmf_sep_event_RT_IS16.m:158-163, :180-185) and the optional
    p.EVENT_NUM / p.NOISE_NUM, checked as snmf_online_set_classes checks them -- SnmfError(1) / (8) before anything reaches
    the device.  Returns (event starts, noise starts) as int32 arrays, or None for one class per side (also: keys absent)."""
    sides = []
    for num_key, rank_key, R in (("EVENT_NUM", "EVENT_RANK", R_x), ("NOISE_NUM", "NOISE_RANK", R_d)):
        raw = np.asarray(p.get(rank_key, [1])).reshape(-1)
        if raw.size < 1 or not np.all(np.isfinite(raw.astype(np.float64))) or np.any(raw != np.round(raw)):
            raise _invalid(f"{rank_key} must hold at least one integer rank")
        rk = [int(v) for v in raw]
        for i, v in enumerate(rk):
            if not 1 <= v <= R:
                raise _invalid(f"{rank_key}({i + 1}) = {v} outside [1, {R}]")
            if i and v <= rk[i - 1]:
                raise _invalid(f"{rank_key} must be strictly ascending")
        if p.get(num_key) is not None and int(p[num_key]) != len(rk):
            raise _invalid(f"{num_key} = {p[num_key]} but {rank_key} lists {len(rk)} classes")
        sides.append(rk)
    for rank_key, rk in zip(("EVENT_RANK", "NOISE_RANK"), sides):
        if rk[0] != 1:  # the sum over the classes feeds the gain (:201)
            raise SnmfError(8, f"{rank_key}(1) = {rk[0]}: the classes must cover the dictionary from column 1")
        if len(rk) > _MAX_CLASSES:
            raise SnmfError(8, f"{len(rk)} classes on a side, at most {_MAX_CLASSES}")
    if len(sides[0]) == 1 and len(sides[1]) == 1:
        return None
    return np.array(sides[0], dtype=np.int32), np.array(sides[1], dtype=np.int32)


# ---- the state g as a value: what OnlineSeparator and OnlineBatchSeparator share (include/snmf.h: snmf_online_state_info) ----
def _state_shapes(q, dt, F, R_x, R_d, adapt, R_a, m_a, blk_ring, n1, class_outputs, classes):
    """Field name -> (shape, dtype) of one stream's state: the rows of include/snmf.h's snmf_online_state_field_id that exist
    in the separator's mode (n1: F_order in Mel mode, else None).  Computed from the constructor's arguments alone."""
    dt = np.dtype(dt)
    r = R_x + R_d
    Ra, ma = (R_a, m_a) if adapt else (1, 1)
    Pl = int(q.P_len_l) if blk_ring else 1
    sz, hop = int(q.framelength), int(q.frameshift)
    ntail = max(1, (sz + hop - 1) // hop - 1) * sz
    f8, i4, i8 = np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.int64)
    sh = {"Xm_tilde": ((F,), dt), "lambda_dav": ((F,), dt), "r_blk": ((F, Pl), dt), "lambda_d_blk": ((F, ma), dt),
          "Ad_blk": ((Ra, ma), dt), "n_push": ((), i4), "update_switch": ((), i4), "B_DFT_d": ((F, R_d), f8), "B_fix": ((F, R_d), f8)}
    if n1 is not None:
        sh["B_Mel_d"] = ((n1, R_d), f8)
    sh.update({"H0": ((r,), dt), "Ad_blk0": ((Ra, ma), dt), "l": ((), i8), "y_hist": ((sz - hop,), dt), "pending": (None, dt),
               "x_tilde_tail": ((ntail,), dt)})
    if class_outputs:
        sh["x_hat_tail"], sh["d_hat_tail"] = ((ntail,), dt), ((ntail,), dt)
    if classes is not None:
        sh["class_tails"] = ((classes[0].size + classes[1].size, ntail), dt)
    return sh


def _state_layout(lib, info):
    """{field: (offset, count, numpy dtype)} of a record under `info` (snmf_online_state_field)."""
    lay = {}
    for f, name in enumerate(_lib.STATE_FIELDS):
        off, cnt, typ = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(lib.snmf_online_state_field(C.byref(info), f, C.byref(off), C.byref(cnt), C.byref(typ)))
        lay[name] = (off.value, cnt.value, np.dtype(_lib.STATE_TYPES[typ.value]))
    return lay


def _state_from_record(rec, info, lay, shapes):
    """One record (uint8 array of info.bytes) -> the dict get_state returns."""
    st = {}
    cnt_p = int(rec[lay["pending_count"][0]:lay["pending_count"][0] + 4].view("<i4")[0])
    for name in shapes:
        off, cnt, dt = lay[name]
        a = rec[off:off + cnt * dt.itemsize].view(dt).copy()
        if name == "pending":
            st[name] = a[:cnt_p]
        elif name == "class_tails":  # one tail per class, class-major in the record
            st[name] = a.reshape(-1, int(info.ntail))
        elif name in ("n_push", "update_switch", "l"):
            st[name] = int(a[0])
        else:
            dims = {"r_blk": (info.F, info.P_len_l), "lambda_d_blk": (info.F, info.m_a), "Ad_blk": (info.R_a, info.m_a),
                    "Ad_blk0": (info.R_a, info.m_a), "B_DFT_d": (info.F, info.R_d), "B_fix": (info.F, info.R_d),
                    "B_Mel_d": (info.F_order, info.R_d)}.get(name)
            st[name] = a.reshape(dims, order="F") if dims else a
    st["record"] = rec.tobytes()
    return st


def _state_checked(st, shapes, hop, who, owner):
    """A state as set_state takes it (a get_state dict or the bytes of a record) -> (record bytes or None, {field: flat
    array}).  Unknown or missing keys raise SnmfError(1) and wrong shapes SnmfError(3), naming the field; nothing here needs
    the library.  who: "state of stream 3" / "state"; owner: "batch" / "separator"."""
    if isinstance(st, (bytes, bytearray, memoryview)):
        return bytes(st), {}
    if not isinstance(st, dict):
        raise _invalid(f"{who}: a dict or the bytes of a record, not {type(st).__name__}")
    unknown = [key for key in st if key != "record" and key not in shapes]
    if unknown:
        raise _invalid(f"{who}: no field {unknown[0]!r} in this {owner}'s mode")
    if st.get("record") is None:
        missing = [key for key in shapes if key not in st]
        if missing:
            raise _invalid(f"{who}: field {missing[0]!r} is missing (and there is no 'record')")
    fields = {}
    for key, (shape, dt) in shapes.items():
        if key not in st:
            continue
        a = np.asarray(st[key])
        if key == "pending":
            a = a.reshape(-1)
            if a.size >= hop:
                raise _invalid(f"{who}: 'pending' holds {a.size} samples, frameshift is {hop}")
        elif a.size == int(np.prod(shape)) and len(shape) <= 1:
            a = a.reshape(shape)
        if key != "pending" and a.shape != tuple(shape):
            raise SnmfError(3, f"{who}: {key!r} is {a.shape}, expected {tuple(shape)}")  # SNMF_ERR_DIM
        fields[key] = np.asarray(a, dtype=dt).ravel(order="C" if key == "class_tails" else "F")
    for key, lo in (("n_push", 0), ("update_switch", 1), ("l", 1)):
        if key in fields and int(fields[key][0]) < lo:
            raise _invalid(f"{who}: {key!r} = {int(fields[key][0])}")
    return (bytes(st["record"]) if st.get("record") is not None else None), fields


def _state_records(parsed, info, lay, owner):
    """The checked states of _state_checked -> the bytes set_state hands to the library: raw records as they are (the library
    judges them), dicts as their record (a hand-built one: the header of this separator) with the fields written over it."""
    rb = int(info.bytes)
    buf = np.zeros(len(parsed) * rb, dtype=np.uint8)
    at = 0
    for rec, fields in parsed:
        if rec is None:  # a hand-built state: the header of this separator
            head = np.zeros(_lib.STATE_HEADER_BYTES, dtype=np.uint8)
            head[:8].view("<u4")[:] = (_lib.STATE_MAGIC, _lib.STATE_VERSION)
            head[8:] = np.frombuffer(bytes(info), dtype=np.uint8)
            rec = head.tobytes()
        if not fields:  # raw bytes go as they are: the library judges them
            if at + len(rec) > buf.size:
                buf = np.concatenate([buf, np.zeros(at + len(rec) - buf.size, dtype=np.uint8)])
            buf[at:at + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
            at += len(rec)
            continue
        m = min(len(rec), rb)
        row = buf[at:at + rb]
        row[:m] = np.frombuffer(rec, dtype=np.uint8)[:m]
        for key, a in fields.items():
            off, cnt, dt = lay[key]
            if key == "pending":
                o2 = lay["pending_count"][0]
                row[o2:o2 + 4].view("<i4")[0] = a.size
                row[off:off + cnt * dt.itemsize] = 0
            elif a.size != cnt:
                raise SnmfError(3, f"state: {key!r} holds {a.size} elements, the {owner}'s record {cnt}")
            row[off:off + a.size * dt.itemsize] = np.ascontiguousarray(a, dtype=dt).view(np.uint8).reshape(-1)
        at += rb
    return buf, at


class OnlineSeparator:
    """State `g` of src/init_buff.m + the per-frame function, resident on the GPU."""

    def __init__(self, B_DFT_x, B_DFT_d, p, H0=None, Ad_blk0=None, ctx=None, class_outputs=False, B_Mel_x=None, B_Mel_d=None,
                 precision="fp32"):
        if precision not in ("fp32", "fp64"):
            raise ValueError("precision must be 'fp32' or 'fp64'")
        self.precision = precision
        dt = np.float64 if precision == "fp64" else np.float32  # what crosses the C ABI
        self._dt = dt
        mode = p.get("B_sep_mode", "DFT")
        if mode not in ("DFT", "Mel") or p.get("Splice", 0) != 0 or p.get("blk_len_sep", 1) != 1:
            raise NotImplementedError("online path: only Splice=0, blk_len_sep=1 (the shipped settings), B_sep_mode 'DFT' or 'Mel'")
        if mode == "Mel" and precision == "fp64":
            raise SnmfError(8, "fp64 online separator: B_sep_mode 'Mel' is not supported")  # SNMF_ERR_UNSUPPORTED, as snmf_online_set_mel
        if mode == "Mel" and (B_Mel_x is None or B_Mel_d is None):
            raise ValueError("B_sep_mode='Mel' needs B_Mel_x and B_Mel_d")
        if "cost_check" not in p:
            raise KeyError("Reference to non-existent field 'cost_check'.")  # src/sparse_nmf.m:260
        method = p.get("ENHANCE_METHOD", "MMSE")
        if method not in ("Wiener", "MMSE"):
            raise ValueError("ENHANCE_METHOD must be 'Wiener' or 'MMSE'")
        shx, shd = np.shape(B_DFT_x), np.shape(B_DFT_d)
        self._classes = _class_partition(p, shx[1], shd[1]) if len(shx) == 2 and len(shd) == 2 else None
        self._lib = _lib.load()
        self.ctx = ctx or default_context()
        Bx = np.asfortranarray(B_DFT_x, dtype=dt)
        Bd = np.asfortranarray(B_DFT_d, dtype=dt)
        F = p["fftlength"] // 2 + 1
        if Bx.shape[0] != F or Bd.shape[0] != F:
            raise ValueError(f"dictionaries must have fftlength/2+1 = {F} rows")
        self.F, self.R_x, self.R_d = F, Bx.shape[1], Bd.shape[1]
        r = self.R_x + self.R_d
        rs = np.random.RandomState(int(p.get("random_seed", 1)) or None)
        if H0 is None:
            H0 = rs.random_sample(r)  # stand-in for rand(r,1), src/sparse_nmf.m:133-134
        adapt = int(bool(p.get("adapt_train_N", 0)))
        R_a, m_a = int(p.get("R_a", 1)), int(p.get("m_a", 1))
        if adapt and Ad_blk0 is None:
            Ad_blk0 = rs.random_sample((R_a, m_a))  # stand-in for rand(R_a, m_a), src/init_buff.m:39
        H0 = np.ascontiguousarray(np.asarray(H0, dtype=dt).reshape(-1))
        if H0.size != r:
            raise ValueError("H0 must have R_x + R_d entries")
        Ad = None
        if adapt:
            Ad = np.asfortranarray(Ad_blk0, dtype=dt)
            if Ad.shape != (R_a, m_a):
                raise ValueError("Ad_blk0 must be R_a x m_a")
        ws = np.ascontiguousarray(p["win_STFT"], dtype=dt)
        wi = np.ascontiguousarray(p["win_ISTFT"], dtype=dt)
        q = _online_params(p, self.R_x, self.R_d, adapt, R_a, m_a, method, class_outputs)
        self._q = q
        self.class_outputs = bool(class_outputs)
        self.hop, self.delay = q.frameshift, q.delay
        self.adapt, self.R_a, self.m_a = adapt, R_a, m_a
        self._blk_ring = bool(p.get("blk_sparse", 0))  # the r_blk ring exists at P_len_l columns
        h = C.c_void_p()
        create = self._lib.snmf_online_create_f64 if precision == "fp64" else self._lib.snmf_online_create
        _lib.check(create(self.ctx._h, C.byref(q), Bx.ctypes.data, Bd.ctypes.data, H0.ctypes.data,
                          Ad.ctypes.data if Ad is not None else None, ws.ctypes.data, wi.ctypes.data, C.byref(h)))
        self._h = h
        self.ctx._plans.add(self)  # destroyed before the context
        self.mel = mode == "Mel"
        if self.mel:
            from .frontend import mel_matrix
            n1 = int(p.get("F_order", 64))
            melmat = np.ascontiguousarray(mel_matrix(p["fs"], n1, p["fftlength"], 1.0, p["fs"] / 2).T, dtype=np.float32)  # init_buff.m:46
            BMx = np.asfortranarray(B_Mel_x, dtype=np.float32)
            BMd = np.asfortranarray(B_Mel_d, dtype=np.float32)
            if BMx.shape != (n1, self.R_x) or BMd.shape != (n1, self.R_d):
                raise ValueError("B_Mel_x / B_Mel_d must be F_order x R_x / R_d")
            self.n1 = n1
            _lib.check(self._lib.snmf_online_set_mel(self._h, n1, int(bool(p.get("MelConv", 1))), melmat.ctypes.data, BMx.ctypes.data,
                                                     BMd.ctypes.data))
        if not self.class_outputs:
            self._classes = None  # (checked all the same; nothing to return them through)
        if self._classes is not None:
            ev, nz = self._classes
            _lib.check(self._lib.snmf_online_set_classes(self._h, ev.size, ev.ctypes.data, nz.size, nz.ctypes.data))

    def process(self, pcm, flush=False):
        """Feed PCM (int16 or int16-valued floats).  Returns a dict with the hops the driver writes for the
        frames completed by this call: 'x_tilde' (int16, what fwrite(...,'int16') stores), 'x_tilde_f'
        (float, before rounding) and with class_outputs 'x_hat' / 'd_hat' and the per-class 'x_hat_i' [E, n] / 'd_hat_i'
        [N, n] of p.EVENT_RANK / p.NOISE_RANK.  The float arrays are float32, or float64 with precision="fp64"."""
        dt = self._dt
        x = np.ascontiguousarray(np.asarray(pcm).reshape(-1), dtype=dt)
        cap = (x.size // self.hop + self.delay + 3) * self.hop
        of = np.zeros(cap, dt)
        o16 = np.zeros(cap, np.int16)
        xh = np.zeros(cap, dt) if self.class_outputs else None
        dh = np.zeros(cap, dt) if self.class_outputs else None
        n = C.c_int64()
        f64 = self.precision == "fp64"
        head = (self._h, x.ctypes.data if x.size else None, x.size, 1 if flush else 0, of.ctypes.data, o16.ctypes.data,
                xh.ctypes.data if xh is not None else None, dh.ctypes.data if dh is not None else None)
        if self._classes is None:  # one class per side: exactly the call a separator without classes makes
            process = self._lib.snmf_online_process_f64 if f64 else self._lib.snmf_online_process_f32
            _lib.check(process(*head, cap, C.byref(n)))
        else:
            xhi, dhi = np.zeros((self._classes[0].size, cap), dt), np.zeros((self._classes[1].size, cap), dt)
            process = self._lib.snmf_online_process_classes_f64 if f64 else self._lib.snmf_online_process_classes_f32
            _lib.check(process(*head, xhi.ctypes.data, dhi.ctypes.data, cap, C.byref(n)))
        out = {"x_tilde": o16[:n.value], "x_tilde_f": of[:n.value]}
        if self.class_outputs:
            out["x_hat"], out["d_hat"] = xh[:n.value], dh[:n.value]
            if self._classes is None:
                out["x_hat_i"], out["d_hat_i"] = out["x_hat"][None], out["d_hat"][None]
            else:
                out["x_hat_i"], out["d_hat_i"] = xhi[:, :n.value], dhi[:, :n.value]
        return out

    def basis(self):
        """Current B_DFT_d (g.B_DFT_d; saved to B_D_u.mat by src/NTF_sep_event_RT.m:138-140); with precision="fp64" the
        fp64 master."""
        if self.precision == "fp64":
            return self.basis_f64()
        B = np.zeros((self.F, self.R_d), dtype=np.float32, order="F")
        _lib.check(self._lib.snmf_online_get_basis_f32(self._h, B.ctypes.data, self.F))
        return B.astype(np.float64)

    def basis_f64(self):
        """The fp64 master of the current B_DFT_d (snmf_online_get_basis_f64; both precisions hold one)."""
        B = np.zeros((self.F, self.R_d), dtype=np.float64, order="F")
        _lib.check(self._lib.snmf_online_get_basis_f64(self._h, B.ctypes.data, self.F))
        return B

    def mel_basis(self):
        """Current B_Mel_d (Mel mode: the dictionary the adaptation updates, :318)."""
        B = np.zeros((self.n1, self.R_d), dtype=np.float32, order="F")
        _lib.check(self._lib.snmf_online_get_mel_basis_f32(self._h, B.ctypes.data, self.n1))
        return B.astype(np.float64)

    # ---- the state g as a value (snmf_online_get_state / _set_state), the next file in place (snmf_online_restart_*) ----
    def _state_shapes(self):
        """Field name -> (shape, dtype) of the state as this separator holds it: what a batch of one with the same arguments
        reports.  Computed from the constructor's arguments alone."""
        return _state_shapes(self._q, self._dt, self.F, self.R_x, self.R_d, self.adapt, self.R_a, self.m_a, self._blk_ring,
                             self.n1 if self.mel else None, self.class_outputs, self._classes)

    def _state_layout(self, lib):
        """The separator's snmf_online_state_info and {field: (offset, count, numpy dtype)} of a record under it."""
        info = _lib.SnmfOnlineStateInfo()
        _lib.check(lib.snmf_online_stream_state_info(self._h, C.byref(info)))
        return info, _state_layout(lib, info)

    def get_state(self):
        """The state g as a value: the dict OnlineBatchSeparator.get_state(k) returns for a stream (the fields of
        snmf_online_state_field_id under their names, matrices F-ordered, rings in time order, plus 'record', the raw
        self-describing bytes).  Allowed between process calls, also before the first; a flushed separator raises
        SnmfError(7).  The separator is not disturbed.  The record is the batch's: either kind of separator of the same
        configuration takes it."""
        shapes = self._state_shapes()
        lib = _lib.load()
        info, lay = self._state_layout(lib)
        buf = np.zeros(max(1, int(info.bytes)), dtype=np.uint8)
        _lib.check(lib.snmf_online_get_state(self._h, buf.ctypes.data, buf.size))
        return _state_from_record(buf[:int(info.bytes)], info, lay, shapes)

    def set_state(self, state):
        """The separator (fresh, running or finished) takes `state` -- what get_state returns here or on a batch, or the raw
        bytes of a record -- and is then a running stream at frame l with an empty trace whose next frames have the bits of
        the stream the state came from.  OnlineBatchSeparator.set_state's rules: in a dict the fields override its 'record';
        a hand-built g (no 'record') needs every field; unknown or missing keys raise SnmfError(1) and wrong shapes
        SnmfError(3), naming the field, before the library is reached; a record of another precision, mode, geometry or class
        count is refused by the library with SnmfError(3) and changes nothing."""
        parsed = [_state_checked(state, self._state_shapes(), int(self._q.frameshift), "state", "separator")]
        lib = _lib.load()
        info, lay = self._state_layout(lib)
        buf, at = _state_records(parsed, info, lay, "separator")
        _lib.check(lib.snmf_online_set_state(self._h, buf.ctypes.data, at))

    def restart(self, B_DFT_d=None, H0=None, Ad_blk0=None, B_Mel_d=None):
        """The next file in place (src/NTF_sep_event_RT.m:27-38 + init_buff) on a flushed or never-fed separator: every piece
        of state as a new separator gives it.  `B_DFT_d` (F x R_d, fp64; Mel mode also `B_Mel_d`, F_order x R_d) None keeps
        the current, adapted dictionary at full fp64 precision and the fixed columns; `H0` / `Ad_blk0` None keep the draws
        the separator last started with.  Wrong shapes raise SnmfError(1) before the library is reached, as in
        OnlineBatchSeparator.restart; a separator in the middle of a recording raises SnmfError(7), and so does a B_Mel_d
        outside Mel mode."""
        def arr(x, shape, name, dt):
            if x is None:
                return None
            a = np.asarray(x, dtype=np.float64)
            if len(shape) == 1 and a.size == shape[0]:
                a = a.reshape(-1)
            if a.shape != tuple(shape):
                raise _invalid(f"{name} is {a.shape}, expected {tuple(shape)}")
            return np.ascontiguousarray(np.asarray(a, dtype=dt).ravel(order="F"))
        Bd = arr(B_DFT_d, (self.F, self.R_d), "B_DFT_d", np.float64)
        H = arr(H0, (self.R_x + self.R_d,), "H0", self._dt)
        Ad = arr(Ad_blk0, (self.R_a, self.m_a), "Ad_blk0", self._dt) if self.adapt else None
        if B_Mel_d is not None and not self.mel:
            raise SnmfError(7, "B_Mel_d given to a separator that is not in Mel mode")  # SNMF_ERR_STATE, as the C entry
        Bm = arr(B_Mel_d, (self.n1, self.R_d), "B_Mel_d", np.float64) if self.mel else None
        lib = _lib.load()
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        restart = lib.snmf_online_restart_f64 if self.precision == "fp64" else lib.snmf_online_restart_f32
        _lib.check(restart(self._h, ptr(Bd), ptr(Bm), ptr(H), ptr(Ad)))

    def trace(self):
        """Per-frame diagnostics: list of dicts (n_iter, trig, solved, n_up, adapt_iters, beta, A_x_mag, ...)."""
        n = C.c_int64()
        _lib.check(self._lib.snmf_online_trace(self._h, None, 0, C.byref(n)))
        arr = (SnmfOnlineFrame * max(1, n.value))()
        _lib.check(self._lib.snmf_online_trace(self._h, C.cast(arr, C.c_void_p), n.value, C.byref(n)))
        return [{k: getattr(arr[i], k) for k, _ in SnmfOnlineFrame._fields_} for i in range(n.value)]

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.snmf_online_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ntf_sep_event_rt(pcm, B_DFT_x, B_DFT_d, p, H0=None, Ad_blk0=None, ctx=None, chunk=None, B_Mel_x=None, B_Mel_d=None,
                     precision="fp32"):
    """src/NTF_sep_event_RT.m for one channel with p.NMF_algorithm = 'SNMF': pcm = the int16 samples after the
    wav header.  Returns (denoised int16, denoised float, final B_DFT_d).  `chunk` (samples per process() call)
    only changes how the stream is fed, not the result.  precision="fp64": the fp64 mode of OnlineSeparator."""
    sep = OnlineSeparator(B_DFT_x, B_DFT_d, p, H0=H0, Ad_blk0=Ad_blk0, ctx=ctx, B_Mel_x=B_Mel_x, B_Mel_d=B_Mel_d, precision=precision)
    try:
        x = np.asarray(pcm).reshape(-1)
        if chunk is None:
            o = sep.process(x, flush=True)
            i16, f32 = o["x_tilde"], o["x_tilde_f"]
        else:
            parts = [sep.process(x[i:i + chunk]) for i in range(0, len(x), chunk)]
            parts.append(sep.process(x[:0], flush=True))
            i16 = np.concatenate([q["x_tilde"] for q in parts])
            f32 = np.concatenate([q["x_tilde_f"] for q in parts])
        return i16.copy(), f32.astype(np.float64), (sep.mel_basis() if sep.mel else sep.basis())
    finally:
        sep.close()


def ntf_sep_event_rt_chain(files, B_DFT_x, B_DFT_d, p, H0=None, Ad_blk0=None, ctx=None, chunk=None, B_Mel_x=None, B_Mel_d=None,
                           precision="fp32", class_outputs=False):
    """run_ntf_sep_RT.m on one separator: `files` (a list of PCM arrays) enhanced in turn by src/NTF_sep_event_RT.m, every file
    after the first starting from the dictionary its predecessor adapted, carried on the device in fp64 by
    OnlineSeparator.restart() (:27-38, :137-140; Mel mode carries B_Mel_d too) with the chain's H0 / Ad_blk0.  It is
    ntf_sep_event_rt_chains for one chain on the single-stream kernels.  Returns (results, final): results[i] is file i's
    (int16, float, final B_DFT_d) triple as ntf_sep_event_rt returns it (Mel mode: the final B_Mel_d; with class_outputs a
    fourth entry, the dict of 'x_hat', 'd_hat', 'x_hat_i', 'd_hat_i'), and final = {'B_DFT_d': the fp64 master after the last
    file, 'B_Mel_d': the Mel dictionary or None, 'traces': every file's OnlineSeparator.trace()}.  `chunk` (samples per
    process() call) only changes how a file is fed."""
    files = [np.asarray(x).reshape(-1) for x in files]
    sep = OnlineSeparator(B_DFT_x, B_DFT_d, p, H0=H0, Ad_blk0=Ad_blk0, ctx=ctx, class_outputs=class_outputs, B_Mel_x=B_Mel_x,
                          B_Mel_d=B_Mel_d, precision=precision)
    try:
        results, traces = [], []
        for i, x in enumerate(files):
            if i:
                sep.restart()  # the carry
            step = len(x) if chunk is None else int(chunk)
            parts = [sep.process(x[j:j + step]) for j in range(0, len(x), max(1, step))]
            parts.append(sep.process(x[:0], flush=True))
            cat = lambda key: np.concatenate([q[key] for q in parts], axis=-1)  # noqa: E731
            res = (cat("x_tilde").astype(np.int16), cat("x_tilde_f").astype(np.float64), sep.mel_basis() if sep.mel else sep.basis())
            if class_outputs:
                res += ({key: cat(key) for key in ("x_hat", "d_hat", "x_hat_i", "d_hat_i")},)
            results.append(res)
            traces.append(sep.trace())
        return results, {"B_DFT_d": sep.basis_f64(), "B_Mel_d": sep.mel_basis() if sep.mel else None, "traces": traces}
    finally:
        sep.close()


def _invalid(msg):
    return SnmfError(1, msg)  # SNMF_ERR_INVALID, raised before anything reaches the device


def _per_stream(x, S, shape, name, order, dtype=np.float32):
    """One array for every stream, a list of S arrays or an array stacked along the last axis -> dtype [S, ...]."""
    if isinstance(x, (list, tuple)):
        if len(x) != S:
            raise _invalid(f"{name}: {len(x)} entries for {S} streams")
        arrs = [np.asarray(a, dtype=np.float64) for a in x]
    else:
        a = np.asarray(x, dtype=np.float64)
        if a.shape == tuple(shape) + (S,):
            arrs = [a[..., k] for k in range(S)]
        else:
            arrs = [a] * S
    out = []
    for k, a in enumerate(arrs):
        if a.size == int(np.prod(shape)) and len(shape) == 1:
            a = a.reshape(-1)
        if a.shape != tuple(shape):
            raise _invalid(f"{name} of stream {k} is {a.shape}, expected {tuple(shape)}")
        out.append(np.asarray(a, dtype=dtype).ravel(order=order))
    return np.ascontiguousarray(np.concatenate(out))


class OnlineBatchSeparator:
    """S independent online streams (snmf_online_batch in include/snmf.h) sharing one set of settings `p`: each stream
    has its own PCM, noise dictionary and state `g`, and they all advance frame by frame in shared launches.  Stream k's
    output is what `OnlineSeparator` produces for it alone.  `B_DFT_d` is one F x R_d array (copied to every stream) or
    a list of S arrays; `H0` / `Ad_blk0` are lists or arrays stacked along the last axis, by default drawn per stream
    from RandomState(random_seed + k).  B_sep_mode 'DFT', or 'Mel' with `B_Mel_x` (F_order x R_x, shared) and `B_Mel_d`
    (one F_order x R_d array or S of them, like B_DFT_d); the supervised frame solve only (SNMF_ERR_UNSUPPORTED otherwise).
    In DFT mode the Mel arguments are ignored, as in OnlineSeparator.  p.EVENT_RANK / p.NOISE_RANK: one class partition for
    all streams (with class_outputs each stream's dict also holds 'x_hat_i' / 'd_hat_i').
    precision="fp64" is the fp64 mode (snmf_online_batch_create_f64): every array crosses in float64, the signals come back
    as float64 and basis(k) is the fp64 dictionary; DFT mode only ('Mel' raises SnmfError(8) before any device call).
    In that mode `settings` (a list of S dicts of overrides on `p`, the keys of _STREAM_KEYS) and `B_DFT_x` as a list of S
    arrays give every stream its own settings and event dictionary (snmf_online_batch_create_streams_f64); stream k's output
    is then what a batch of one with its dictionaries and `dict(p, **settings[k])` produces.  `Ad_blk0` is needed when any
    stream adapts and holds an entry for every stream.  Without either, the call is the uniform one, unchanged."""

    def __init__(self, B_DFT_x, B_DFT_d, p, n_streams, H0=None, Ad_blk0=None, ctx=None, class_outputs=False, B_Mel_x=None,
                 B_Mel_d=None, precision="fp32", settings=None):
        if precision not in ("fp32", "fp64"):
            raise ValueError("precision must be 'fp32' or 'fp64'")
        Bx_list = list(B_DFT_x) if isinstance(B_DFT_x, (list, tuple)) else None
        per_stream = settings is not None or Bx_list is not None
        if per_stream and precision != "fp64":
            raise SnmfError(8, "batched separator: settings and B_DFT_x per stream need precision='fp64'")
        self.precision = precision
        dt = np.float64 if precision == "fp64" else np.float32  # what crosses the C ABI
        self._dt = dt
        S = int(n_streams)
        if S < 1:
            raise _invalid("n_streams must be >= 1")
        if p.get("Splice", 0) != 0 or p.get("blk_len_sep", 1) != 1:
            raise NotImplementedError("online path: only Splice=0, blk_len_sep=1 (the shipped settings)")
        mode = p.get("B_sep_mode", "DFT")
        if mode not in ("DFT", "Mel"):
            raise SnmfError(8, f"batched separator: B_sep_mode {mode!r} is not supported")  # SNMF_ERR_UNSUPPORTED
        if mode == "Mel" and precision == "fp64":
            raise SnmfError(8, "fp64 batched separator: B_sep_mode 'Mel' is not supported")  # as snmf_online_batch_set_mel
        if mode == "Mel" and (B_Mel_x is None or B_Mel_d is None):
            raise SnmfError(8, "batched separator: B_sep_mode 'Mel' needs B_Mel_x and B_Mel_d")
        if "cost_check" not in p:
            raise KeyError("Reference to non-existent field 'cost_check'.")  # src/sparse_nmf.m:260
        method = p.get("ENHANCE_METHOD", "MMSE")
        if method not in ("Wiener", "MMSE"):
            raise ValueError("ENHANCE_METHOD must be 'Wiener' or 'MMSE'")
        F = p["fftlength"] // 2 + 1
        if Bx_list is not None and len(Bx_list) != S:
            raise _invalid(f"B_DFT_x: {len(Bx_list)} entries for {S} streams")
        Bx = np.asfortranarray(Bx_list[0] if Bx_list is not None else B_DFT_x, dtype=dt)
        if Bx.ndim != 2 or Bx.shape[0] != F:
            raise _invalid(f"B_DFT_x must have fftlength/2+1 = {F} rows")
        R_x = Bx.shape[1]
        Bd_list = B_DFT_d if isinstance(B_DFT_d, (list, tuple)) else None
        Bd_first = np.asarray(Bd_list[0] if Bd_list else B_DFT_d)
        if Bd_first.ndim not in (2, 3) or Bd_first.shape[0] != F:
            raise _invalid(f"B_DFT_d must have fftlength/2+1 = {F} rows")
        R_d = Bd_first.shape[1]
        r = R_x + R_d
        adapt = int(bool(p.get("adapt_train_N", 0)))
        self._p, self._stream_p = dict(p), None
        if per_stream:  # the rings exist when any stream adapts; Ad_blk0 then holds an entry for every stream
            self._stream_p = _stream_settings(p, settings, S)
            adapt = int(any(bool(m.get("adapt_train_N", 0)) for m in self._stream_p))
            Bx = _per_stream(Bx_list if Bx_list is not None else B_DFT_x, S, (F, R_x), "B_DFT_x", "F", dt)
        # the r_blk ring exists at P_len_l columns once any stream is block-sparse (the rings only grow)
        self._blk_ring = any(bool(m.get("blk_sparse", 0)) for m in (self._stream_p or [p]))
        R_a, m_a = int(p.get("R_a", 1)), int(p.get("m_a", 1))
        seed = int(p.get("random_seed", 1))
        if H0 is None or (adapt and Ad_blk0 is None):
            draws_h, draws_a = [], []
            for k in range(S):  # OnlineSeparator's stand-ins, seeded per stream
                rs = np.random.RandomState(seed + k)
                draws_h.append(rs.random_sample(r))
                if adapt:
                    draws_a.append(rs.random_sample((R_a, m_a)))
            H0 = draws_h if H0 is None else H0
            Ad_blk0 = draws_a if (adapt and Ad_blk0 is None) else Ad_blk0
        Bd = _per_stream(B_DFT_d, S, (F, R_d), "B_DFT_d", "F", dt)
        H = _per_stream(H0, S, (r,), "H0", "F", dt)
        Ad = _per_stream(Ad_blk0, S, (R_a, m_a), "Ad_blk0", "F", dt) if adapt else None
        self.mel = mode == "Mel"
        if self.mel:
            n1 = int(p.get("F_order", 64))
            if not 2 <= n1 <= F:
                raise _invalid(f"F_order = {n1} outside [2, fftlength/2+1 = {F}]")
            BMx = np.asfortranarray(B_Mel_x, dtype=np.float32)
            if BMx.shape != (n1, R_x):
                raise _invalid(f"B_Mel_x is {BMx.shape}, expected {(n1, R_x)}")
            BMd = _per_stream(B_Mel_d, S, (n1, R_d), "B_Mel_d", "F")
            self.n1 = n1
        self._classes = _class_partition(p, R_x, R_d)
        self._lib = _lib.load()
        self.ctx = ctx or default_context()
        self.F, self.R_x, self.R_d, self.S = F, R_x, R_d, S
        self.adapt, self.R_a, self.m_a = adapt, R_a, m_a
        ws = np.ascontiguousarray(p["win_STFT"], dtype=dt)
        wi = np.ascontiguousarray(p["win_ISTFT"], dtype=dt)
        q = _online_params(p, R_x, R_d, adapt, R_a, m_a, method, class_outputs)
        self._q = q
        self.class_outputs = bool(class_outputs)
        self.hop, self.delay = q.frameshift, q.delay
        h = C.c_void_p()
        if per_stream:
            sts = (SnmfOnlineStreamSettings * S)(*[_settings_struct(m, q) for m in self._stream_p])
            _lib.check(self._lib.snmf_online_batch_create_streams_f64(
                self.ctx._h, C.byref(q), S, Bx.ctypes.data, Bd.ctypes.data, H.ctypes.data, Ad.ctypes.data if Ad is not None else None,
                C.cast(sts, C.c_void_p), ws.ctypes.data, wi.ctypes.data, C.byref(h)))
        else:
            create = self._lib.snmf_online_batch_create_f64 if precision == "fp64" else self._lib.snmf_online_batch_create
            _lib.check(create(self.ctx._h, C.byref(q), S, Bx.ctypes.data, Bd.ctypes.data, H.ctypes.data,
                              Ad.ctypes.data if Ad is not None else None, ws.ctypes.data, wi.ctypes.data, C.byref(h)))
        self._h = h
        self.ctx._plans.add(self)  # destroyed before the context
        if self.mel:
            from .frontend import mel_matrix
            melmat = np.ascontiguousarray(mel_matrix(p["fs"], self.n1, p["fftlength"], 1.0, p["fs"] / 2).T, dtype=np.float32)  # init_buff.m:46
            _lib.check(self._lib.snmf_online_batch_set_mel(self._h, self.n1, int(bool(p.get("MelConv", 1))), melmat.ctypes.data,
                                                           BMx.ctypes.data, BMd.ctypes.data))
        if not self.class_outputs:
            self._classes = None  # (checked all the same; nothing to return them through)
        if self._classes is not None:  # one partition for all streams
            ev, nz = self._classes
            _lib.check(self._lib.snmf_online_batch_set_classes(self._h, ev.size, ev.ctypes.data, nz.size, nz.ctypes.data))

    def process(self, pcms, flush=False):
        """Feed every stream: `pcms` is a list of S sample arrays (any may be empty); `flush` a bool for all or a list of
        S bools.  Returns a list of S dicts, each as OnlineSeparator.process returns (float64 signals with precision="fp64")."""
        S, dt, f64 = self.S, self._dt, self.precision == "fp64"
        if len(pcms) != S:
            raise _invalid(f"{len(pcms)} PCM arrays for {S} streams")
        fl = [bool(flush)] * S if np.isscalar(flush) or flush is None else [bool(x) for x in flush]
        if len(fl) != S:
            raise _invalid(f"{len(fl)} flush flags for {S} streams")
        xs = [np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=dt) for x in pcms]
        caps = np.array([(x.size // self.hop + self.delay + 3) * self.hop for x in xs], dtype=np.int64)
        of = [np.zeros(c, dt) for c in caps]
        o16 = [np.zeros(c, np.int16) for c in caps]
        xh = [np.zeros(c, dt) for c in caps] if self.class_outputs else None
        dh = [np.zeros(c, dt) for c in caps] if self.class_outputs else None
        P = C.c_void_p * S
        ptrs = lambda arrs: P(*[a.ctypes.data if a.size else None for a in arrs])  # noqa: E731
        n = np.array([x.size for x in xs], dtype=np.int64)
        f32 = np.array(fl, dtype=np.int32)
        n_out = np.zeros(S, dtype=np.int64)
        head = (self._h, ptrs(xs), n.ctypes.data, f32.ctypes.data, P(*[a.ctypes.data for a in of]), P(*[a.ctypes.data for a in o16]),
                P(*[a.ctypes.data for a in xh]) if xh else None, P(*[a.ctypes.data for a in dh]) if dh else None)
        if self._classes is None:  # one class per side: exactly the call a batch without classes makes
            process = self._lib.snmf_online_batch_process_f64 if f64 else self._lib.snmf_online_batch_process_f32
            _lib.check(process(*head, caps.ctypes.data, n_out.ctypes.data))
        else:
            xhi = [np.zeros((self._classes[0].size, c), dt) for c in caps]
            dhi = [np.zeros((self._classes[1].size, c), dt) for c in caps]
            process = self._lib.snmf_online_batch_process_classes_f64 if f64 else self._lib.snmf_online_batch_process_classes_f32
            _lib.check(process(
                *head, P(*[a.ctypes.data for a in xhi]), P(*[a.ctypes.data for a in dhi]), caps.ctypes.data, n_out.ctypes.data))
        outs = []
        for k in range(S):
            m = int(n_out[k])
            o = {"x_tilde": o16[k][:m], "x_tilde_f": of[k][:m]}
            if self.class_outputs:
                o["x_hat"], o["d_hat"] = xh[k][:m], dh[k][:m]
                if self._classes is None:
                    o["x_hat_i"], o["d_hat_i"] = o["x_hat"][None], o["d_hat"][None]
                else:
                    o["x_hat_i"], o["d_hat_i"] = xhi[k][:, :m], dhi[k][:, :m]
            outs.append(o)
        return outs

    def restart(self, streams, B_DFT_d=None, H0=None, Ad_blk0=None, B_Mel_d=None, B_DFT_x=None, settings=None):
        """Streams `streams` (an index or a list of distinct indices) start a new recording: src/NTF_sep_event_RT.m:27-38
        + init_buff, every piece of their state as a new separator gives it, the other streams untouched.  Each of
        `B_DFT_d` (F x R_d, fp64), `B_Mel_d` (Mel mode: F_order x R_d, fp64), `H0` and `Ad_blk0` is None, one array for all
        listed streams or one per stream.  None keeps the stream's current, adapted dictionary at full fp64 precision
        (load('B_D_u.mat'), :27-38 load both) and the H0 / Ad_blk0 it last started with.  A stream that has consumed
        samples and was not flushed raises SnmfError(7), and so does a B_Mel_d outside Mel mode.
        fp64 batch: `B_DFT_x` (F x R_x, one array or one per listed stream) and `settings` (one dict of overrides on `p` or
        one per listed stream) also replace the streams' event dictionaries and settings (snmf_online_batch_restart_streams_f64);
        None keeps each stream's own.  A stream that adapts from now on needs an `Ad_blk0`, here or from an earlier call."""
        ks = [int(streams)] if np.isscalar(streams) else [int(k) for k in streams]
        n = len(ks)
        bad = [k for k in ks if not 0 <= k < self.S]
        if bad:
            raise _invalid(f"stream {bad[0]} out of range [0, {self.S})")
        if len(set(ks)) != n:
            raise _invalid("a stream is listed twice")
        per_stream = B_DFT_x is not None or settings is not None
        if per_stream and (self.precision != "fp64" or self.mel):
            raise SnmfError(8, "batched separator: settings and B_DFT_x per stream need precision='fp64'")
        new_p = _stream_settings(self._p, settings, n, "listed stream") if settings is not None else None
        Bxn = None if B_DFT_x is None else _per_stream(B_DFT_x, n, (self.F, self.R_x), "B_DFT_x", "F", np.float64)
        if new_p is not None and any(bool(m.get("adapt_train_N", 0)) for m in new_p):
            self.adapt = 1
        if new_p is not None and any(bool(m.get("blk_sparse", 0)) for m in new_p):
            self._blk_ring = True
        Bd = None if B_DFT_d is None else _per_stream(B_DFT_d, n, (self.F, self.R_d), "B_DFT_d", "F", np.float64)
        H = None if H0 is None else _per_stream(H0, n, (self.R_x + self.R_d,), "H0", "F", self._dt)
        Ad = None if (Ad_blk0 is None or not self.adapt) else _per_stream(Ad_blk0, n, (self.R_a, self.m_a), "Ad_blk0", "F", self._dt)
        if B_Mel_d is not None and not self.mel:
            raise SnmfError(7, "B_Mel_d given to a batch that is not in Mel mode")  # SNMF_ERR_STATE, as the C entry
        Bm = None if B_Mel_d is None else _per_stream(B_Mel_d, n, (self.n1, self.R_d), "B_Mel_d", "F", np.float64)
        if n == 0:
            return
        sl = np.array(ks, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        if per_stream:
            sts = None if new_p is None else (SnmfOnlineStreamSettings * n)(*[_settings_struct(m, self._q) for m in new_p])
            _lib.check(self._lib.snmf_online_batch_restart_streams_f64(self._h, n, sl.ctypes.data, ptr(Bxn), ptr(Bd), ptr(H), ptr(Ad),
                                                                       C.cast(sts, C.c_void_p) if sts is not None else None))
            if new_p is not None:
                if self._stream_p is None:
                    self._stream_p = [dict(self._p) for _ in range(self.S)]
                for k, m in zip(ks, new_p):
                    self._stream_p[k] = m
        elif self.mel:
            _lib.check(self._lib.snmf_online_batch_restart_mel(self._h, n, sl.ctypes.data, ptr(Bd), ptr(Bm), ptr(H), ptr(Ad)))
        elif self.precision == "fp64":  # H0 / Ad_blk0 cross in fp64 too
            _lib.check(self._lib.snmf_online_batch_restart_f64(self._h, n, sl.ctypes.data, ptr(Bd), ptr(H), ptr(Ad)))
        else:
            _lib.check(self._lib.snmf_online_batch_restart(self._h, n, sl.ctypes.data, ptr(Bd), ptr(H), ptr(Ad)))

    def basis(self, k):
        """Current B_DFT_d of stream k; with precision="fp64" the fp64 dictionary."""
        if self.precision == "fp64":
            return self.basis_f64(k)
        B = np.zeros((self.F, self.R_d), dtype=np.float32, order="F")
        _lib.check(self._lib.snmf_online_batch_get_basis_f32(self._h, int(k), B.ctypes.data, self.F))
        return B.astype(np.float64)

    def basis_f64(self, k):
        """Stream k's fp64 master of B_DFT_d: what a carry (restart with B_DFT_d=None) keeps."""
        B = np.zeros((self.F, self.R_d), dtype=np.float64, order="F")
        _lib.check(self._lib.snmf_online_batch_get_basis_f64(self._h, int(k), B.ctypes.data, self.F))
        return B

    def mel_basis(self, k):
        """Current B_Mel_d of stream k (Mel mode: the dictionary the adaptation updates, :318)."""
        if not self.mel:
            raise SnmfError(7, "not in Mel mode")
        B = np.zeros((self.n1, self.R_d), dtype=np.float32, order="F")
        _lib.check(self._lib.snmf_online_batch_get_mel_basis_f32(self._h, int(k), B.ctypes.data, self.n1))
        return B.astype(np.float64)

    def mel_basis_f64(self, k):
        """Stream k's fp64 master of B_Mel_d: what a carry (restart with B_Mel_d=None) keeps."""
        if not self.mel:
            raise SnmfError(7, "not in Mel mode")
        B = np.zeros((self.n1, self.R_d), dtype=np.float64, order="F")
        _lib.check(self._lib.snmf_online_batch_get_mel_basis_f64(self._h, int(k), B.ctypes.data, self.n1))
        return B

    def settings(self, k):
        """Stream k's settings as the batch holds them (snmf_online_batch_get_settings; fp64 batch): a dict of the fields
        of snmf_online_stream_settings."""
        st = SnmfOnlineStreamSettings()
        _lib.check(self._lib.snmf_online_batch_get_settings(self._h, int(k), C.byref(st)))
        return {f: getattr(st, f) for f in _STREAM_FIELDS}

    # ---- a stream's state g as a value (snmf_online_batch_get_state / _set_state) ----
    def _state_shapes(self):
        """Field name -> (shape, dtype) of one stream's state as this batch holds it: the rows of include/snmf.h's
        snmf_online_state_field_id that exist in its mode.  Computed from the constructor's arguments alone."""
        return _state_shapes(self._q, self._dt, self.F, self.R_x, self.R_d, self.adapt, self.R_a, self.m_a, self._blk_ring,
                             self.n1 if self.mel else None, self.class_outputs, self._classes)

    def _stream_list(self, streams):
        ks = [int(streams)] if np.isscalar(streams) else [int(k) for k in streams]
        bad = [k for k in ks if not 0 <= k < self.S]
        if bad:
            raise _invalid(f"stream {bad[0]} out of range [0, {self.S})")
        if len(set(ks)) != len(ks):
            raise _invalid("a stream is listed twice")
        return ks

    def _state_layout(self, lib):
        """The batch's snmf_online_state_info and {field: (offset, count, numpy dtype)} of a record under it."""
        info = _lib.SnmfOnlineStateInfo()
        _lib.check(lib.snmf_online_batch_state_info(self._h, C.byref(info)))
        return info, _state_layout(lib, info)

    def get_state(self, streams):
        """The state g of stream `streams` (an index: one dict; a list of distinct indices: a list of dicts), as the fourth
        result of bnmf_sep_event_RT_IS16 with the driver's variables around it: the fields of snmf_online_state_field_id under
        their names there ('Xm_tilde', 'lambda_dav', 'r_blk', 'lambda_d_blk', 'Ad_blk', 'n_push', 'update_switch', 'B_DFT_d',
        'B_fix', 'B_Mel_d', 'H0', 'Ad_blk0', 'l', 'y_hist', 'pending', 'x_tilde_tail', 'x_hat_tail', 'd_hat_tail',
        'class_tails'), matrices as F-ordered arrays with the rings in time order (oldest column first), plus 'record', the raw
        bytes (self-describing; what set_state and a file take).  Allowed between process calls on a stream that was not
        flushed (a flushed one raises SnmfError(7)); the stream is not disturbed."""
        one = np.isscalar(streams)
        ks = self._stream_list(streams)
        shapes = self._state_shapes()
        lib = _lib.load()
        info, lay = self._state_layout(lib)
        n, rb = len(ks), int(info.bytes)
        buf = np.zeros(max(1, n * rb), dtype=np.uint8)
        sl = np.array(ks, dtype=np.int32)
        if n:
            _lib.check(lib.snmf_online_batch_get_state(self._h, n, sl.ctypes.data, buf.ctypes.data, buf.size))
        out = [_state_from_record(buf[i * rb:(i + 1) * rb], info, lay, shapes) for i in range(n)]
        return out[0] if one else out

    def set_state(self, streams, states):
        """Streams `streams` (an index or a list of distinct indices; any slot, fresh, running or finished) take the given
        states and are then running streams at frame l with an empty trace: the next frames have the bits of the stream
        the state came from.  A state is what get_state returns (a dict; with `streams` a list, a list of them), or the raw
        bytes of a record.  In a dict the field arrays override its 'record', so a hand-built g works: without a 'record'
        every field of the batch's mode must be there.  Unknown or missing keys raise SnmfError(1) and wrong shapes
        SnmfError(3), naming the field, before the library is reached; a record of another precision, mode, geometry or
        class count is refused by the library with SnmfError(3) and changes nothing.  B_DFT_x, the settings and the class
        partition are configuration: the slot has them from create or restart."""
        ks = self._stream_list(streams)
        sts = [states] if (np.isscalar(streams) or isinstance(states, (dict, bytes, bytearray, memoryview))) else list(states)
        if len(sts) != len(ks):
            raise _invalid(f"{len(sts)} states for {len(ks)} streams")
        shapes = self._state_shapes()
        hop = int(self._q.frameshift)
        parsed = [_state_checked(st, shapes, hop, f"state of stream {k}", "batch") for k, st in zip(ks, sts)]
        lib = _lib.load()
        info, lay = self._state_layout(lib)
        n = len(ks)
        if n == 0:
            return
        buf, at = _state_records(parsed, info, lay, "batch")
        sl = np.array(ks, dtype=np.int32)
        _lib.check(lib.snmf_online_batch_set_state(self._h, n, sl.ctypes.data, buf.ctypes.data, at))

    def out_capacity(self, n_samples):
        """Output samples that hold one flushed recording of `n_samples` (snmf_online_batch_out_capacity)."""
        return int(self._lib.snmf_online_batch_out_capacity(self._h, int(n_samples)))

    def run_chains(self, chains, B_DFT_d, H0=None, Ad_blk0=None, B_Mel_d=None, chunk_hops=None, masters=False):
        """ntf_sep_event_rt_chains on this batch's slots in ONE library call (snmf_online_batch_run_chains_f32 / _f64): the
        queue of chains, the carries and the restarts run in the library's host code.  `chains` is a list of chains, each a
        list of PCM arrays; `B_DFT_d` (Mel mode also `B_Mel_d`) one start dictionary for all chains or one per chain, rounded
        to fp32 on an fp32 batch as the Python driver rounds them; `H0` / `Ad_blk0` one array or one per chain, by default
        drawn from RandomState(random_seed + c).  Returns what ntf_sep_event_rt_chains returns, bit for bit: per chain the
        list of its files' (int16, float, final dictionary) triples (Mel mode: the final B_Mel_d); with `masters` the
        dictionaries are the fp64 masters instead of their fp32 images (an fp64 batch returns the masters either way).
        The batch must be idle (every fed stream flushed: SnmfError(7) otherwise) and is idle again afterwards; a batch with
        settings per stream raises SnmfError(8)."""
        chains = [[np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=self._dt) for x in c] for c in chains]
        nc = len(chains)
        f64 = self.precision == "fp64"
        r = self.R_x + self.R_d
        Bds = _per_chain(B_DFT_d, nc, (self.F, self.R_d), "B_DFT_d", np.float64 if f64 else np.float32)
        if B_Mel_d is not None and not self.mel:
            raise SnmfError(7, "B_Mel_d given to a batch that is not in Mel mode")  # SNMF_ERR_STATE, as the C entry
        if self.mel and B_Mel_d is None:
            raise _invalid("a Mel batch needs every chain's start B_Mel_d")
        Bms = _per_chain(B_Mel_d, nc, (self.n1, self.R_d), "B_Mel_d", np.float32) if self.mel else None
        if H0 is not None:
            H0 = _per_chain(H0, nc, (r,), "H0", np.float64)
        if self.adapt and Ad_blk0 is not None:
            Ad_blk0 = _per_chain(Ad_blk0, nc, (self.R_a, self.m_a), "Ad_blk0", np.float64)
        if chunk_hops and int(chunk_hops) < 1:  # (None or 0: the default, as in ntf_sep_event_rt_chains and the C entry)
            raise _invalid("chunk_hops must be >= 1")
        seed = int(self._p.get("random_seed", 1))
        hs, ads = [], []
        for c in range(nc):  # ntf_sep_event_rt_chains' draws for chain c
            rs = np.random.RandomState(seed + c)
            h = rs.random_sample(r)
            a = rs.random_sample((self.R_a, self.m_a)) if self.adapt else None
            hs.append(h if H0 is None else H0[c])
            if self.adapt:
                ads.append(a if Ad_blk0 is None else Ad_blk0[c])
        flat = lambda arrs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=dt).ravel(order="F") for x in arrs]) if arrs  # noqa: E731
                                                     else np.zeros(0, dt))
        Bd_all, H_all = flat(Bds, np.float64), flat(hs, self._dt)
        Bm_all = flat(Bms, np.float64) if self.mel else None
        Ad_all = flat(ads, self._dt) if self.adapt else None
        files = [x for c in chains for x in c]
        nf = len(files)
        n_files = np.array([len(c) for c in chains], dtype=np.int32)
        n_samples = np.array([x.size for x in files], dtype=np.int64)
        caps = np.array([self.out_capacity(x.size) for x in files], dtype=np.int64)
        o16 = [np.zeros(c, np.int16) for c in caps]
        of = [np.zeros(c, self._dt) for c in caps]
        rows = self.n1 if self.mel else self.F
        Bo = [np.zeros((rows, self.R_d), dtype=np.float64, order="F") for _ in files]
        n_out = np.zeros(max(nf, 1), dtype=np.int64)
        P = C.c_void_p * max(nf, 1)
        ptrs = lambda arrs: P(*[a.ctypes.data if a.size else None for a in arrs])  # noqa: E731
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        run = self._lib.snmf_online_batch_run_chains_f64 if f64 else self._lib.snmf_online_batch_run_chains_f32
        _lib.check(run(self._h, nc, ptr(n_files), ptrs(files), ptr(n_samples), ptr(Bd_all), ptr(Bm_all), ptr(H_all), ptr(Ad_all),
                       int(chunk_hops or 0), ptrs(o16), ptrs(of), ptr(caps), n_out.ctypes.data, ptrs(Bo)))
        results, i = [], 0
        for c in chains:
            res = []
            for _ in c:
                m = int(n_out[i])
                B = Bo[i] if (f64 or masters) else Bo[i].astype(np.float32).astype(np.float64)  # basis(k) / mel_basis(k) of the fp32 batch
                res.append((o16[i][:m].copy(), of[i][:m].astype(np.float64), B))
                i += 1
            results.append(res)
        return results

    def trace(self, k):
        """Per-frame diagnostics of stream k, as OnlineSeparator.trace."""
        n = C.c_int64()
        _lib.check(self._lib.snmf_online_batch_trace(self._h, int(k), None, 0, C.byref(n)))
        arr = (SnmfOnlineFrame * max(1, n.value))()
        _lib.check(self._lib.snmf_online_batch_trace(self._h, int(k), C.cast(arr, C.c_void_p), n.value, C.byref(n)))
        return [{f: getattr(arr[i], f) for f, _ in SnmfOnlineFrame._fields_} for i in range(n.value)]

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.snmf_online_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ntf_sep_event_rt_batch(pcms, B_DFT_x, B_DFT_d, p, H0=None, Ad_blk0=None, ctx=None, B_Mel_x=None, B_Mel_d=None,
                           precision="fp32", settings=None):
    """src/NTF_sep_event_RT.m for several recordings at once (the per-target loop of Do_MultiBatch_IS16_20160324.m:183-205
    as one batch): returns a list of the (int16, float, final B_DFT_d) triples ntf_sep_event_rt returns (Mel mode: the
    final B_Mel_d).  precision="fp64": the fp64 mode of OnlineBatchSeparator, which also takes `settings` (one dict of
    overrides on `p` per recording) and `B_DFT_x` as a list (one event dictionary per recording)."""
    sep = OnlineBatchSeparator(B_DFT_x, B_DFT_d, p, len(pcms), H0=H0, Ad_blk0=Ad_blk0, ctx=ctx, B_Mel_x=B_Mel_x, B_Mel_d=B_Mel_d,
                               precision=precision, settings=settings)
    try:
        outs = sep.process(list(pcms), flush=True)
        fin = sep.mel_basis if sep.mel else sep.basis
        return [(o["x_tilde"].copy(), o["x_tilde_f"].astype(np.float64), fin(k)) for k, o in enumerate(outs)]
    finally:
        sep.close()


_B_CHUNK_SLOTS = 16384  # (frame, stream) slots of one device chunk (kBChunkSlots, csrc/snmf_online_batch_host.h)


def _per_chain(x, n, shape, name, dtype):
    """One array for every chain or a list of n arrays -> a list of n fp64 arrays of `shape` holding `dtype` values (a
    shared array is checked and converted once)."""
    if isinstance(x, (list, tuple)):
        if len(x) != n:
            raise _invalid(f"{name}: {len(x)} entries for {n} chains")
        arrs = list(x)
    else:
        arrs = [x] * n
    done, out = {}, []
    for c, a in enumerate(arrs):
        if id(a) not in done:
            b = np.asarray(a, dtype=dtype)
            if len(shape) == 1 and b.size == shape[0]:
                b = b.reshape(-1)
            if b.shape != tuple(shape):
                raise _invalid(f"{name} of chain {c} is {b.shape}, expected {tuple(shape)}")
            done[id(a)] = np.asfortranarray(b, dtype=np.float64)
        out.append(done[id(a)])
    return out


def ntf_sep_event_rt_chains(chains, B_DFT_x, B_DFT_d, p, n_streams=None, H0=None, Ad_blk0=None, ctx=None, chunk_hops=None,
                            B_Mel_x=None, B_Mel_d=None, precision="fp32", settings=None):
    """Do_MultiBatch_IS16_20160324.m:183-205 + run_ntf_sep_RT.m:10-41 on one batch: `chains` is a list of chains, each a
    list of PCM arrays enhanced in turn by src/NTF_sep_event_RT.m.  Chain c starts from B_DFT_d (one array or one per
    chain; the delete('B_D_u.mat') of :187), and every later file starts from the dictionary its predecessor adapted,
    carried on the device in fp64 (:27-38, :137-140).  Returns, per chain, the list of its files' (int16, float, final
    B_DFT_d) triples, as ntf_sep_event_rt_batch returns them.

    `n_streams` slots (default min(len(chains), 256)) take chains from a queue; each call feeds every busy slot at most
    `chunk_hops` hops (default one device chunk), and a slot whose file ended is restarted at the next call -- with the
    carried dictionary or with its next chain's.  Chain c uses its own H0 / Ad_blk0 (one array or one per chain; by
    default drawn from RandomState(random_seed + c), as OnlineBatchSeparator draws for stream k) for all its files, so
    its bits depend neither on its slot, `n_streams` or `chunk_hops` nor on the other chains.  Start dictionaries enter
    in fp32, as in ntf_sep_event_rt_batch.  In Mel mode (B_Mel_x, and B_Mel_d as one array or one per chain) a chain
    carries both dictionaries (:137-139) and its triples hold the final B_Mel_d.
    precision="fp64": the fp64 mode of OnlineBatchSeparator; start dictionaries, H0 and Ad_blk0 then enter as float64 (not
    rounded to fp32 first), the float signals and final dictionaries are the fp64 ones, and the slot-independence above holds.
    In that mode `B_DFT_x` may be a list with one event dictionary per chain and `settings` a list with one dict of overrides
    on `p` per chain: a slot takes its chain's pair and settings when the chain starts on it, and the independence holds."""
    if precision not in ("fp32", "fp64"):
        raise ValueError("precision must be 'fp32' or 'fp64'")
    Bx_list = list(B_DFT_x) if isinstance(B_DFT_x, (list, tuple)) else None
    per_chain = settings is not None or Bx_list is not None
    if per_chain and precision != "fp64":
        raise SnmfError(8, "batched separator: settings and B_DFT_x per chain need precision='fp64'")
    chains = [[np.asarray(x).reshape(-1) for x in c] for c in chains]
    nc = len(chains)
    if nc == 0:
        return []
    S = min(nc, 256) if n_streams is None else int(n_streams)
    if S < 1:
        raise _invalid("n_streams must be >= 1")
    F = p["fftlength"] // 2 + 1
    if Bx_list is not None and len(Bx_list) != nc:
        raise _invalid(f"B_DFT_x: {len(Bx_list)} entries for {nc} chains")
    Bx = np.asarray(Bx_list[0] if Bx_list is not None else B_DFT_x)
    if Bx.ndim != 2 or Bx.shape[0] != F:
        raise _invalid(f"B_DFT_x must have fftlength/2+1 = {F} rows")
    Bd_first = np.asarray(B_DFT_d[0] if isinstance(B_DFT_d, (list, tuple)) and len(B_DFT_d) else B_DFT_d)
    if Bd_first.ndim != 2 or Bd_first.shape[0] != F:
        raise _invalid(f"B_DFT_d must have fftlength/2+1 = {F} rows")
    R_x, R_d = Bx.shape[1], Bd_first.shape[1]
    r = R_x + R_d
    adapt = int(bool(p.get("adapt_train_N", 0)))
    sets = Bxs = None
    if per_chain:  # checked here, before the library is loaded; the draws follow "any chain adapts"
        sets = [{k: m[k] for k in m if k in _STREAM_KEYS} for m in _stream_settings(p, settings, nc, "chain")]
        adapt = int(any(bool(m.get("adapt_train_N", p.get("adapt_train_N", 0))) for m in sets))
        Bxs = _per_chain(Bx_list if Bx_list is not None else B_DFT_x, nc, (F, R_x), "B_DFT_x", np.float64)
    R_a, m_a = int(p.get("R_a", 1)), int(p.get("m_a", 1))
    # (fp32 mode: fp32 values, restarted with in fp64; fp64 mode: the doubles as they are)
    Bds = _per_chain(B_DFT_d, nc, (F, R_d), "B_DFT_d", np.float64 if precision == "fp64" else np.float32)
    mel = p.get("B_sep_mode", "DFT") == "Mel"
    if mel and precision == "fp64":
        raise SnmfError(8, "fp64 batched separator: B_sep_mode 'Mel' is not supported")
    Bms = None
    if mel:
        if B_Mel_x is None or B_Mel_d is None:
            raise SnmfError(8, "batched separator: B_sep_mode 'Mel' needs B_Mel_x and B_Mel_d")
        Bms = _per_chain(B_Mel_d, nc, (int(p.get("F_order", 64)), R_d), "B_Mel_d", np.float32)
    if H0 is not None:
        H0 = _per_chain(H0, nc, (r,), "H0", np.float64)
    if adapt and Ad_blk0 is not None:
        Ad_blk0 = _per_chain(Ad_blk0, nc, (R_a, m_a), "Ad_blk0", np.float64)
    seed = int(p.get("random_seed", 1))

    def draws(c):  # OnlineBatchSeparator's stand-ins for stream c
        rs = np.random.RandomState(seed + c)
        h = rs.random_sample(r)
        a = rs.random_sample((R_a, m_a)) if adapt else None
        if H0 is not None:
            h = H0[c]
        if adapt and Ad_blk0 is not None:
            a = Ad_blk0[c]
        return h, a

    results = [[] for _ in range(nc)]
    queue = [c for c in range(nc) if chains[c]][::-1]  # popped from the end: chain order
    if not queue:
        return results
    first = [queue.pop() for _ in range(min(S, len(queue)))]
    init = [first[k] if k < len(first) else first[0] for k in range(S)]
    dr = {c: draws(c) for c in set(init)}
    sep = OnlineBatchSeparator([Bxs[c] for c in init] if per_chain else Bx, [Bds[c] for c in init], p, S, H0=[dr[c][0] for c in init],
                               Ad_blk0=[dr[c][1] for c in init] if adapt else None, ctx=ctx, B_Mel_x=B_Mel_x,
                               B_Mel_d=[Bms[c] for c in init] if mel else None, precision=precision,
                               settings=[sets[c] for c in init] if per_chain else None)
    fin = sep.mel_basis if mel else sep.basis
    hop = sep.hop
    step = int(chunk_hops) if chunk_hops else max(1, min(4096, _B_CHUNK_SLOTS // S))
    if step < 1:
        raise _invalid("chunk_hops must be >= 1")
    try:
        # slot -> [chain, file, samples fed, int16 parts, float parts]
        busy = {k: [c, 0, 0, [], []] for k, c in enumerate(first)}
        carry, fresh = [], []
        while busy:
            if carry:
                sep.restart(carry)  # same chain: the adapted fp64 dictionaries, the chain's own H0 / Ad_blk0
            if fresh:
                cs = [busy[k][0] for k in fresh]
                ds = [draws(c) for c in cs]
                sep.restart(fresh, [Bds[c] for c in cs], [d[0] for d in ds], [d[1] for d in ds] if adapt else None,
                            B_Mel_d=[Bms[c] for c in cs] if mel else None, B_DFT_x=[Bxs[c] for c in cs] if per_chain else None,
                            settings=[sets[c] for c in cs] if per_chain else None)
            carry, fresh = [], []
            pcms, flush = [np.zeros(0, sep._dt)] * S, [False] * S
            for k, st in busy.items():
                x = chains[st[0]][st[1]]
                pcms[k] = x[st[2]:st[2] + step * hop]
                st[2] += len(pcms[k])
                flush[k] = st[2] >= len(x)
            outs = sep.process(pcms, flush)
            for k in list(busy):
                st = busy[k]
                st[3].append(outs[k]["x_tilde"])
                st[4].append(outs[k]["x_tilde_f"])
                if not flush[k]:
                    continue
                c, i = st[0], st[1]
                results[c].append((np.concatenate(st[3]).astype(np.int16), np.concatenate(st[4]).astype(np.float64), fin(k)))
                if i + 1 < len(chains[c]):
                    busy[k] = [c, i + 1, 0, [], []]
                    carry.append(k)
                elif queue:
                    busy[k] = [queue.pop(), 0, 0, [], []]
                    fresh.append(k)
                else:
                    del busy[k]
        return results
    finally:
        sep.close()
