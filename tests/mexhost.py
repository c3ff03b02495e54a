"""Runs the MATLAB MEX shims (integration/*_mex.cpp) without MATLAB: each shim is compiled together with the test host
tests/mexhost/mexhost.cpp -- a real implementation of the prototypes in integration/mex_stub/mex.h -- into a shared object
of its own, and driven through ctypes.

    shims = build_all(tmpdir)                 # or the session fixture `mex_shims`
    w, h = shims["sparse_nmf_mex"](2, v, w0, h0, 5.0, dict(beta=1.0, ...))

`mex(nlhs, *args)` converts as MATLAB would hold the values: numpy float64 <-> double matrix (column-major), float32 <->
single, bool <-> logical, int16 / int32 <-> the integer classes, str <-> char row, dict <-> 1 x 1 struct, None or an empty
array <-> [].  A Python float / int is a double scalar, a 1-D array a column.  It returns the list of results (max(nlhs, 1)
of them, as MATLAB fills `ans`).  mexErrMsgIdAndTxt raises MexError(id, msg); anything the host itself objects to (see
mexhost.cpp: double destroy, modified input, broken guard zone, wrong typed accessor, ...) raises HostError, so a test
that makes the call fails.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST_DIR = os.path.join(HERE, "mexhost")
SHIMS = ("sparse_nmf_mex", "snmf_mdi_mex", "snmf_frontend_mex", "snmf_dnmf_mex", "snmf_online_mex")

# mxClassID of integration/mex_stub/mex.h
LOGICAL, CHAR, DOUBLE, SINGLE, INT16, INT32, STRUCT = 3, 4, 6, 7, 10, 12, -1
_NP_OF = {LOGICAL: np.bool_, CHAR: np.uint16, DOUBLE: np.float64, SINGLE: np.float32, INT16: np.int16, INT32: np.int32}
_CLS_OF = {np.dtype(v): k for k, v in _NP_OF.items() if k != CHAR}


class MexError(Exception):
    """mexErrMsgIdAndTxt(id, msg) left the call."""

    def __init__(self, id, msg):
        super().__init__(f"{id}: {msg}")
        self.id, self.msg = id, msg


class HostError(AssertionError):
    """The test host saw the MEX file break the MEX contract."""


def lib_path():
    """The libsnmf_hip.so that _lib.load() maps."""
    from se_snmf_nat_amd import _lib
    return os.path.abspath(os.environ.get("SNMF_LIB_PATH") or _lib.LIB_PATH)


def compile_cmd(sources, out, link_lib=True, extra=()):
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", *extra,
           "-I" + os.path.join(ROOT, "integration", "mex_stub"), "-I" + os.path.join(ROOT, "include"), *sources, "-o", out]
    if link_lib:  # the library file itself, found again at run time through the rpath: one libsnmf_hip.so per process
        lp = lib_path()
        cmd += ["-L" + os.path.dirname(lp), "-l:" + os.path.basename(lp), "-Wl,-rpath," + os.path.dirname(lp)]
    return cmd


def build_shim(name, outdir):
    """integration/<name>.cpp + the host -> <outdir>/<name>_host.so (g++ -Wall -Werror; no HIP runtime on the link line)."""
    out = os.path.join(str(outdir), name + "_host.so")
    src = os.path.join(ROOT, "integration", name + ".cpp")
    r = subprocess.run(compile_cmd([src, os.path.join(HOST_DIR, "mexhost.cpp")], out), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{name}: compile / link failed\n{r.stderr}")
    return out


def build_misbehave(outdir):
    out = os.path.join(str(outdir), "misbehave_host.so")
    srcs = [os.path.join(HOST_DIR, "misbehave_mex.cpp"), os.path.join(HOST_DIR, "mexhost.cpp")]
    r = subprocess.run(compile_cmd(srcs, out, link_lib=False), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"misbehave_mex: compile failed\n{r.stderr}")
    return out


def mapped_libsnmf():
    """The distinct libsnmf_hip.so files this process maps."""
    seen = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libsnmf_hip.so"):
                seen.add(parts[5].strip())
    return sorted(seen)


class Mex:
    """One loaded shim-with-host shared object."""

    def __init__(self, path, needs_lib=True):
        if needs_lib:
            from se_snmf_nat_amd import _lib
            _lib.load()  # first: it decides which HIP runtime the process holds; the shim then binds to the mapped library
        self.path = path
        h = self._h = C.CDLL(path)
        vp, sz = C.c_void_p, C.c_size_t
        for name, res, args in (
                ("mh_make", vp, [C.c_int, sz, sz, vp]), ("mh_make_struct", vp, []), ("mh_set_field", C.c_int, [vp, C.c_char_p, vp]),
                ("mh_free", None, [vp]), ("mh_class", C.c_int, [vp]), ("mh_m", sz, [vp]), ("mh_n", sz, [vp]), ("mh_bytes", sz, [vp]),
                ("mh_data", vp, [vp]), ("mh_nfields", C.c_int, [vp]), ("mh_field_name", C.c_char_p, [vp, C.c_int]),
                ("mh_field_value", vp, [vp, C.c_int]), ("mh_guard_bytes", sz, []), ("mh_call", C.c_int, [C.c_int, C.c_int, C.POINTER(vp)]),
                ("mh_nout", C.c_int, []), ("mh_out", vp, [C.c_int]), ("mh_take_out", vp, [C.c_int]), ("mh_err_id", C.c_char_p, []),
                ("mh_err_msg", C.c_char_p, []), ("mh_lock_count", C.c_int, []), ("mh_has_exit_fcn", C.c_int, []),
                ("mh_unload", C.c_int, []), ("mh_error_count", C.c_int, []), ("mh_error_get", C.c_char_p, [C.c_int]),
                ("mh_error_clear", None, []), ("mh_live_count", sz, [])):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        if needs_lib:
            maps = mapped_libsnmf()
            assert len(maps) == 1 and os.path.samefile(maps[0], lib_path()), f"the process must map one libsnmf_hip.so: {maps}"

    # -- Python -> mxArray ------------------------------------------------------------------------------------------
    def to_mx(self, x):
        h = self._h
        if isinstance(x, dict):
            s = h.mh_make_struct()
            for k, v in x.items():
                assert h.mh_set_field(s, k.encode(), self.to_mx(v)) == 0
            return s
        if x is None:
            return h.mh_make(DOUBLE, 0, 0, None)
        if isinstance(x, str):
            a = np.frombuffer(x.encode("utf-16-le"), dtype=np.uint16)
            return h.mh_make(CHAR, 1 if a.size else 0, a.size, a.ctypes.data if a.size else None)
        a = np.asarray(x)
        if a.dtype not in _CLS_OF:  # Python numbers and lists: doubles, as MATLAB literals are
            a = a.astype(np.float64)
        if a.ndim == 0:
            a = a.reshape(1, 1)
        elif a.ndim == 1:
            a = a.reshape(-1, 1)
        assert a.ndim == 2, "matrices only"
        f = np.asfortranarray(a)
        p = h.mh_make(_CLS_OF[f.dtype], f.shape[0], f.shape[1], f.ctypes.data if f.size else None)
        assert p, "the host refused the array"
        return p

    # -- mxArray -> Python ------------------------------------------------------------------------------------------
    def from_mx(self, p):
        h = self._h
        cls = h.mh_class(p)
        if cls == STRUCT:
            return {h.mh_field_name(p, i).decode(): (self.from_mx(h.mh_field_value(p, i)) if h.mh_field_value(p, i) else None)
                    for i in range(h.mh_nfields(p))}
        m, n, nb = h.mh_m(p), h.mh_n(p), h.mh_bytes(p)
        dt = np.dtype(_NP_OF[cls])
        assert nb == m * n * dt.itemsize
        flat = np.frombuffer(C.string_at(h.mh_data(p), nb), dtype=dt) if nb else np.zeros(0, dt)
        if cls == CHAR:
            return flat.tobytes().decode("utf-16-le")
        return flat.reshape((m, n), order="F").copy(order="F")

    # -- the call ---------------------------------------------------------------------------------------------------
    def __call__(self, nlhs, *args):
        h = self._h
        h.mh_error_clear()
        mx = [self.to_mx(a) for a in args]
        try:
            arr = (C.c_void_p * max(len(mx), 1))(*mx)
            st = h.mh_call(int(nlhs), len(mx), arr)
            errs = self.host_errors()
            if errs:
                raise HostError("; ".join(errs))
            if st == 1:
                raise MexError(h.mh_err_id().decode(), h.mh_err_msg().decode())
            assert st == 0, f"mh_call returned {st} without a host error"
            return [self.from_mx(h.mh_out(i)) for i in range(h.mh_nout())]
        finally:
            for i in range(h.mh_nout()):  # the results were copied (or the call failed): nothing stays with the host
                h.mh_free(h.mh_take_out(i))
            for p in mx:
                h.mh_free(p)

    def host_errors(self):
        return [self._h.mh_error_get(i).decode() for i in range(self._h.mh_error_count())]

    def lock_count(self):
        return self._h.mh_lock_count()

    def has_exit_fcn(self):
        return bool(self._h.mh_has_exit_fcn())

    def unload(self):
        """What MATLAB does at `clear mex` of an unlocked file or at exit: the mexAtExit function runs."""
        assert self._h.mh_unload() == 0
        errs = self.host_errors()
        if errs:
            raise HostError("; ".join(errs))

    def live_arrays(self):
        """Arrays the host still holds (between calls: none)."""
        return self._h.mh_live_count()


def _dump_arg(x, out):
    """One argument in the token format of tests/mexhost/replay_main.cpp (the conversions of Mex.to_mx)."""
    if isinstance(x, dict):
        out.append(f"S {len(x)}")
        for k, v in x.items():
            out.append(k)
            _dump_arg(v, out)
        return
    if x is None:
        out.append(f"A {DOUBLE} 0 0 -")
        return
    if isinstance(x, str):
        a = np.frombuffer(x.encode("utf-16-le"), dtype=np.uint16)
        out.append(f"A {CHAR} {1 if a.size else 0} {a.size} {a.tobytes().hex() or '-'}")
        return
    a = np.asarray(x)
    if a.dtype not in _CLS_OF:
        a = a.astype(np.float64)
    a = a.reshape(1, 1) if a.ndim == 0 else a.reshape(-1, 1) if a.ndim == 1 else a
    out.append(f"A {_CLS_OF[a.dtype]} {a.shape[0]} {a.shape[1]} {np.asfortranarray(a).tobytes(order='F').hex() or '-'}")


def dump_cases(path, cases):
    """(shim, name, expected id, nlhs, args) cases -> the file tests/mexhost/replay_main.cpp replays (a sanitizer pass by hand)."""
    out = []
    for shim, _name, want, nlhs, args in cases:
        out.append(f"CASE {shim} {nlhs} {want} {len(args)}")
        for x in args:
            _dump_arg(x, out)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def build_all(outdir):
    return {name: Mex(build_shim(name, outdir)) for name in SHIMS}


@pytest.fixture(scope="session")
def mex_shims(tmp_path_factory, lib):
    """The five shims, each built with the host into a temp directory and loaded (after the library itself).  Their
    contexts are released at the end of the session, before the interpreter tears the library down."""
    shims = build_all(tmp_path_factory.mktemp("mexhost"))
    yield shims
    for m in shims.values():
        m.unload()


@pytest.fixture(scope="session")
def misbehave(tmp_path_factory):
    return Mex(build_misbehave(tmp_path_factory.mktemp("misbehave")), needs_lib=False)
