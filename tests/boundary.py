"""Helpers of the boundary tests (tests/test_boundary_rules.py on the CPU, tests/test_gpu_boundary.py on the GPU): strided
column-major buffers with poisoned padding and a guard band, the bits a round trip through the library must return, a mirror
of the transfer pipeline's chunk arithmetic, and the table that maps every `int64_t ld*` parameter of include/snmf.h to the
test file that passes it a leading dimension larger than the row count.  No test functions live here.

The element-count convention (BLAS): a rows x cols matrix with leading dimension ld occupies (cols - 1) * ld + rows elements.
Every buffer built here has exactly that many, followed by a guard band: a library path that assumed cols * ld elements would
read or write the guard."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snmf.h")
XFER_SRC = os.path.join(ROOT, "se_snmf_nat_amd", "csrc", "snmf_tu_xfer.hip")

OK, INVALID = 0, 1
GUARD = 64  # elements after the last element the convention grants

# Output padding and guard: negative finite numbers, so no result of a non-negative factorization (nor a rounded or widened
# one) can equal them; compared as integers.
SENT_BITS = {np.dtype(np.float32): np.uint32(0xC2F7A5C3), np.dtype(np.float64): np.uint64(0xC05EDD2F1A9FBE77)}
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def sentinel(dt):
    dt = np.dtype(dt)
    return np.array([SENT_BITS[dt]]).view(dt)[0]


def ubits(a):
    """The integer view of a float array (what every comparison of padding, guards and results is made on)."""
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype])


class Strided:
    """A rows x cols column-major matrix with leading dimension ld inside an allocation of (cols - 1) * ld + rows elements plus
    GUARD more.  `buf` is the whole allocation; the matrix starts at buf[0]."""

    def __init__(self, rows, cols, ld, dt, pad, a=None):
        assert ld >= rows >= 1 and cols >= 1
        self.rows, self.cols, self.ld, self.dt = int(rows), int(cols), int(ld), np.dtype(dt)
        self.n = (self.cols - 1) * self.ld + self.rows
        self.pad = np.asarray(pad, dtype=self.dt)
        self.buf = np.full(self.n + GUARD, self.pad, dtype=self.dt)
        self.dev = None
        if a is not None:
            a = np.asarray(a)
            assert a.shape == (rows, cols) and a.dtype == self.dt, (a.shape, a.dtype)
            self._matrix(self.buf)[...] = a

    def _matrix(self, buf):
        it = self.dt.itemsize
        return np.lib.stride_tricks.as_strided(buf, shape=(self.rows, self.cols), strides=(it, self.ld * it))

    def _padding(self, buf):
        it = self.dt.itemsize
        if self.cols < 2 or self.ld == self.rows:
            return buf[:0]
        return np.lib.stride_tricks.as_strided(buf[self.rows:], shape=(self.ld - self.rows, self.cols - 1), strides=(it, self.ld * it))

    # -- residency: the same allocation as a torch tensor on the device ----------------------------------------------------
    def to_device(self):
        import torch
        self.dev = torch.from_numpy(self.buf).to("cuda:0")
        torch.cuda.synchronize()
        return self

    def fetch(self):
        """Device allocation -> buf (a synchronising copy)."""
        if self.dev is not None:
            self.buf = self.dev.cpu().numpy()
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() if self.dev is not None else self.buf.ctypes.data

    # -- what the tests read -------------------------------------------------------------------------------------------------
    def values(self):
        return np.array(self._matrix(self.buf), order="F")

    def rest(self):
        """Padding rows and guard band, as integers."""
        return np.concatenate([ubits(np.array(self._padding(self.buf)).ravel()), ubits(self.buf[self.n:])])

    def intact(self):
        """Every element between rows and ld, and every element of the guard band, still holds the fill's bits."""
        r = self.rest()
        return r.size >= GUARD and bool((r == ubits(self.pad.reshape(1))[0]).all())

    def untouched(self):
        """Nothing at all was written (a refused call)."""
        return bool((ubits(self.buf) == ubits(self.pad.reshape(1))[0]).all())


def strided(a, ld, pad=np.nan):
    """The matrix `a` with leading dimension ld; the rows between a.shape[0] and ld and the guard band hold `pad`.  Inputs take
    NaN (any read of padding poisons a result), outputs the sentinel."""
    a = np.asarray(a)
    return Strided(a.shape[0], a.shape[1], ld, a.dtype, pad, a)


def strided_out(rows, cols, ld, dt):
    """An output buffer: matrix, padding and guard all hold the sentinel."""
    return Strided(rows, cols, ld, dt, sentinel(dt))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((ubits(a) == ubits(b)).all())


def first_difference(got, want):
    """(row, column) of the first element, in column-major order, whose bits differ; None when there is none."""
    d = ubits(np.asfortranarray(got)) != ubits(np.asfortranarray(want))
    if not d.any():
        return None
    c = int(np.argmax(d.any(axis=0)))
    return int(np.argmax(d[:, c])), c


def matches(buf, want):
    """The comparator of the round-trip tests: the matrix in `buf` (a Strided) has the bits of `want`, and its padding and
    guard are intact."""
    return same_bits(buf.values(), want) and buf.intact()


# ---- what a round trip returns ---------------------------------------------------------------------------------------------
def expect(a, in_type, dev_type, out_type):
    """The bits a set -> get round trip returns for host values `a`: each narrowing is ONE round-to-nearest-even to fp32, each
    widening is exact.  W is kept on the device as an fp64 master (dev_type float64: f64 in, f64 out is the identity), H in
    fp32 (dev_type float32)."""
    x = np.asarray(a).astype(in_type)
    return x.astype(dev_type).astype(out_type)


def truncate_to_f32(a):
    """f64 -> f32 by truncation (round toward zero): the mutant the comparator must tell from round-to-nearest."""
    b = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) & ~np.uint64((1 << 29) - 1)
    return b.view(np.float64).astype(np.float32)


def round_trip_values(rows, cols, seed):
    """Non-negative fp64 values over the fp32 range (1e-30 .. 1e30); every third one is an exact tie of the f64 -> f32 rounding
    (the midpoint of two neighbouring fp32 numbers, which an fp64 holds exactly)."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(1.0, 2.0, (rows, cols)) * 10.0 ** rs.uniform(-30, 30, (rows, cols))
    lo = a.astype(np.float32)
    tie = (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) / 2
    pick = (np.arange(rows * cols).reshape(cols, rows).T % 3) == 0
    return np.asfortranarray(np.where(pick, tie, a))


def placed_values(rows, cols, dt=np.float64):
    """value(row, column) = 1 + row + rows * column: a misplaced element names the place it came from.  Every value is exact in
    fp32 and no two are equal: past 2^24 - 1 the count goes on in half-integers (0.5, 1.5, ...)."""
    lim = 2 ** 24 - 1
    assert rows * cols < 2 * lim
    idx = np.arange(rows * cols, dtype=np.float64)
    v = np.where(idx < lim, idx + 1.0, idx - lim + 0.5)
    return v.reshape(cols, rows).T.astype(dt, order="F")


# ---- the chunk arithmetic of the host transfer pipeline --------------------------------------------------------------------
CHUNK_BYTES = 16 << 20     # kChunkBytes, se_snmf_nat_amd/csrc/snmf_tu_xfer.hip:29
N_BUFFERS = 3              # kNB, snmf_tu_xfer.hip:30
POOL_MIN_BYTES = 1 << 20   # kPoolMinBytes, snmf_tu_xfer.hip:31


def xfer_constants_in_source():
    """(kChunkBytes, kNB, kPoolMinBytes) as csrc/snmf_tu_xfer.hip defines them."""
    src = open(XFER_SRC).read()
    sh = lambda name: (lambda m: int(m.group(1)) << int(m.group(2)))(re.search(name + r"\s*=\s*\(size_t\)(\d+)\s*<<\s*(\d+)", src))  # noqa: E731
    return sh("kChunkBytes"), int(re.search(r"kNB\s*=\s*(\d+)", src).group(1)), sh("kPoolMinBytes")


def staged_size(host_dt, dev_dt):
    """Bytes per element in the bounce buffers: 4 when either side is fp32, else 8 (staged_t, snmf_tu_xfer.hip:217-219, :265)."""
    return 4 if 4 in (np.dtype(host_dt).itemsize, np.dtype(dev_dt).itemsize) else 8


def chunking(rows, cols, host_dt, dev_dt):
    """-> (columns per chunk, number of chunks, columns of the last chunk, host bytes of a full chunk)"""
    cpc = max(1, CHUNK_BYTES // (rows * staged_size(host_dt, dev_dt)))
    n = -(-cols // cpc)
    return cpc, n, cols - (n - 1) * cpc, min(cpc, cols) * rows * np.dtype(host_dt).itemsize


def chunk_of(col, rows, host_dt, dev_dt):
    """-> (chunk index, bounce buffer index) of a column"""
    i = col // chunking(rows, col + 1, host_dt, dev_dt)[0]
    return i, i % N_BUFFERS


# Section B of test_gpu_boundary.py: H (r = 128 rows, fp32 on the device) from an fp64 host array.
CHUNK_R = 128
CHUNK_CASES = {  # T: (chunks, columns of the last chunk)
    32768: (1, 32768),
    32769: (2, 1),
    98304: (3, 32768),
    98305: (4, 1),
    131073: (5, 1),
}
CHUNK_LDS = (CHUNK_R, CHUNK_R + 3)  # the contiguous copy, the per-column copy (both through the pool: a chunk is 32 MiB of host data)
# B3: one masked fp64 batch problem, fp64 staged: 8160 columns per chunk, 4 chunks each way
MDI_CHUNK = dict(F=257, T=24481, r=2, chunks=4, last=1)

# Section A
ROUND_TRIP_SHAPES = [(513, 37, 70), (5, 1, 33), (257, 40, 1)]  # (F, r, T)
TYPES = {"f32": np.float32, "f64": np.float64}


def ld_steps(rows):
    return (rows, rows + 1, rows + 61)


# ---- every leading dimension of the C ABI ----------------------------------------------------------------------------------
HERE = "here"  # tests/test_gpu_boundary.py
FRONTEND = "tests/test_gpu_frontend_envelope.py"
ENTRIES = {
    # one-shot solves
    "snmf_sparse_nmf_f64": HERE, "snmf_sparse_nmf_f32": HERE, "snmf_sparse_nmf_oop_f64": HERE, "snmf_sparse_nmf_oop_f32": HERE,
    "snmf_sparse_nmf_fp64": HERE, "snmf_mdi_fp64": HERE,
    # resident plan
    "snmf_plan_set_v_f64": HERE, "snmf_plan_set_v_f32": HERE, "snmf_plan_set_w_f64": HERE, "snmf_plan_set_w_f32": HERE,
    "snmf_plan_set_h_f64": HERE, "snmf_plan_set_h_f32": HERE, "snmf_plan_get_w_f64": HERE, "snmf_plan_get_w_f32": HERE,
    "snmf_plan_get_h_f64": HERE, "snmf_plan_get_h_f32": HERE, "snmf_plan_set_mask_f64": HERE, "snmf_plan_set_mask_f32": HERE,
    "snmf_plan_get_v_mdi_f64": HERE, "snmf_plan_get_v_mdi_f32": HERE,
    "snmf_plan_solve_frames_f64": HERE, "snmf_plan_solve_frames_f32": HERE,
    # front-end (layouts, residency and refusals are that file's sections 1-5)
    "snmf_stft_features_f32": FRONTEND, "snmf_stft_features_fp64": FRONTEND, "snmf_mel_features_f32": FRONTEND,
    "snmf_mel_features_fp64": FRONTEND, "snmf_tf_dd_f32": FRONTEND, "snmf_tf_dd_fp64": FRONTEND,
    # training callers
    "snmf_run_basis_dnmf_f64": HERE, "snmf_run_basis_dnmf_f32": HERE, "snmf_run_basis_dnmf_fp64": HERE,
    "snmf_run_basis_dnmf_audio_f64": HERE, "snmf_run_basis_dnmf_audio_fp64": HERE,
    # online basis readers
    "snmf_online_get_basis_f32": HERE, "snmf_online_get_basis_f64": HERE, "snmf_online_get_mel_basis_f32": HERE,
    "snmf_online_batch_get_basis_f32": HERE, "snmf_online_batch_get_basis_f64": HERE,
    "snmf_online_batch_get_mel_basis_f32": HERE, "snmf_online_batch_get_mel_basis_f64": HERE,
    # multi-rank
    "snmf_multi_set_v_f64": HERE, "snmf_multi_set_v_f32": HERE, "snmf_multi_set_w_f64": HERE, "snmf_multi_set_w_f32": HERE,
    "snmf_multi_set_h_f64": HERE, "snmf_multi_set_h_f32": HERE, "snmf_multi_get_w_f64": HERE, "snmf_multi_get_w_f32": HERE,
    "snmf_multi_get_w_rank_f64": HERE, "snmf_multi_get_h_f64": HERE, "snmf_multi_get_h_f32": HERE,
    "snmf_sparse_nmf_multi_f64": HERE, "snmf_sparse_nmf_multi_f32": HERE,
    "snmf_run_basis_dnmf_multi_f64": HERE, "snmf_run_basis_dnmf_multi_f32": HERE,
    # batched offline solve
    "snmf_batch_set_problem_f64": HERE, "snmf_batch_set_problem_f32": HERE, "snmf_sparse_nmf_batch_f64": HERE,
    "snmf_sparse_nmf_batch_f32": HERE, "snmf_sparse_nmf_batch_fp64": HERE, "snmf_batch_set_problem_mdi_f64": HERE,
    "snmf_batch_get_v_mdi_f64": HERE, "snmf_mdi_batch_fp64": HERE,
}


def header_ld_parameters(path=HEADER):
    """{function: [names of its `int64_t ld*` / `const int64_t* ld*` parameters]} of every prototype in the header."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(snmf_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        lds = re.findall(r"int64_t\s*\*?\s*(ld\w*)", m.group(2))
        if lds:
            out[m.group(1)] = lds
    return out
