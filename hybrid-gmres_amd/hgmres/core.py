"""Host-side mirror of the reference's MATLAB solver interface over libhgmres.

Every public solver keeps the reference's name, positional arguments and
output tuple (the MATLAB ``[x, error_norm, residual_norm, niters] = f(...)``
becomes a Python tuple), with histories truncated to ``1:niters`` exactly as
the ``.m`` files do.  Operators may be scipy sparse matrices, dense arrays, or
:class:`SparseOperator` handles already resident in HBM.

Reference signatures mirrored (file:line):
  hybrid_ab_gmres_rtp.m:1, hybrid_ba_gmres_rtp.m:1, lsqr_solver.m:1,
  lsmr_solver.m:1 (defaults :3,5), hybrid_lsqr_solver.m:1,
  hybrid_lsmr_solver.m:1, gcv_function.m:1, ABgmres_hybrid_bounds.m:1-2,
  ABgmres_nonhybrid_bounds.m:1-2, BAgmres_hybrid_bounds.m:1-2,
  BAgmres_nonhybrid_bounds.m:1-2.
Error behaviour: MATLAB errors (dimension mismatch, unassigned output) raise
ValueError / :class:`OutputNotAssigned`; Krylov breakdown is not an error.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np
import scipy.sparse as sp

from . import _lib as L


class HgmError(RuntimeError):
    pass


class OutputNotAssigned(HgmError):
    """MATLAB: 'Output argument "x" not assigned during call'."""


def _check(rc, ctx=None):
    if rc == L.HGM_OK:
        return
    msg = ""
    if ctx is not None and ctx._h:
        msg = L.load().hgm_last_error(ctx._h).decode(errors="replace")
    if rc == L.HGM_E_ARG:
        raise ValueError(msg or "invalid argument")
    if rc == L.HGM_E_NOT_ASSIGNED:
        raise OutputNotAssigned(msg)
    raise HgmError(f"libhgmres status {rc}: {msg}")


def _dp(a):
    return a.ctypes.data_as(L.dp) if a is not None else None


def _f64(v, n=None, name="vector"):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{name} has length {a.shape[0]}, expected {n}")
    return a


class Context:
    """One HIP device + stream (``hgm_ctx``).  ``world > 1`` contexts are made
    by :func:`hgmres.dist.init_context`."""

    def __init__(self, device: int = 0, _handle=None):
        lib = L.load()
        self.device = device
        if _handle is None:
            h = C.c_void_p()
            rc = lib.hgm_ctx_create(device, C.byref(h))
            if rc != L.HGM_OK:
                n, paths = L.runtime_check(lib)
                if n > 1:
                    raise HgmError(f"hgm_ctx_create refused: two HIP runtimes are mapped ({paths})")
                raise HgmError(f"hgm_ctx_create(device={device}) failed with status {rc} (is a GPU visible?)")
            _handle = h
        self._h = _handle
        self._keep = []          # callbacks kept alive

    @property
    def handle(self):
        return self._h

    def rank_world(self):
        r, w = C.c_int(), C.c_int()
        _check(L.load().hgm_ctx_rank(self._h, C.byref(r), C.byref(w)), self)
        return r.value, w.value

    def release_workspace(self):
        """Free this context's device workspace (hgm_ctx_release_workspace); returns the bytes freed."""
        b = C.c_int64()
        _check(L.load().hgm_ctx_release_workspace(self._h, C.byref(b)), self)
        return b.value

    def mem_info(self):
        """(free, total) bytes of device memory on this context's GPU (all processes)."""
        f, t = C.c_int64(), C.c_int64()
        _check(L.load().hgm_mem_info(self._h, C.byref(f), C.byref(t)), self)
        return f.value, t.value

    def solve_path(self):
        """Path decisions of the last solve on this context (``hgm_ctx_solve_path``):
        ``{"gram_monitor": [0/1 per GMRES iteration], "one_pass": 0/1 or None}``."""
        lib = L.load()
        out = {}
        for what, key in ((0, "gram_monitor"), (1, "one_pass")):
            n = C.c_int()
            _check(lib.hgm_ctx_solve_path(self._h, what, None, 0, C.byref(n)), self)
            buf = (C.c_int * max(n.value, 1))()
            _check(lib.hgm_ctx_solve_path(self._h, what, buf, n.value, C.byref(n)), self)
            out[key] = list(buf[:n.value])
        out["one_pass"] = out["one_pass"][0] if out["one_pass"] else None
        return out

    def set_option(self, name, value):
        """Per-context numerics option (``hgm_ctx_set_option``; names in ``_lib.OPTIONS`` and ``_lib.OPTIONS_37``),
        e.g. ``ctx.set_option("parity", 1)``.  Returns the previous value."""
        prev = self.get_option(name)
        _check(L.load().hgm_ctx_set_option(self._h, L.option_id(name), float(value)), self)
        return prev

    def get_option(self, name):
        v = C.c_double()
        _check(L.load().hgm_ctx_get_option(self._h, L.option_id(name), C.byref(v)), self)
        return v.value

    def options(self, **kw):
        """Context manager: set options for a block, restore them after."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            prev = {k: self.set_option(k, v) for k, v in kw.items()}
            try:
                yield self
            finally:
                for k, v in prev.items():
                    self.set_option(k, v)
        return _cm()

    def synchronize(self):
        _check(L.load().hgm_ctx_synchronize(self._h), self)

    def stream(self):
        return L.load().hgm_ctx_stream(self._h)

    def set_host_allreduce(self, rank, world, fn):
        """Route cross-rank sums through ``fn(np.ndarray) -> None`` (in place).
        Used for shard emulation (several processes on one device, gloo)."""
        def _cb(buf, count, _user):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(count,))
                fn(arr)
                return 0
            except Exception:   # noqa: BLE001 - reported as a comm error by the library
                return -1
        cb = L.ALLREDUCE_FN(_cb)
        self._keep.append(cb)
        _check(L.load().hgm_ctx_set_host_allreduce(self._h, rank, world, cb, None), self)

    def kernel_timing(self, enable=True):
        _check(L.load().hgm_kernel_timing(self._h, int(enable)), self)

    def kernel_timing_pause(self, paused=True):
        _check(L.load().hgm_kernel_timing_pause(self._h, int(paused)), self)

    def kernel_timing_read(self, cls):
        ms, calls, by = C.c_double(), C.c_int64(), C.c_double()
        _check(L.load().hgm_kernel_timing_read(self._h, cls, C.byref(ms), C.byref(calls), C.byref(by)), self)
        return ms.value, calls.value, by.value

    def close(self):
        if self._h:
            L.load().hgm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():       # HIP runtime may already be torn down at exit
            return
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass


_default_ctx = None
_ctx_lock = threading.Lock()


def default_context() -> Context:
    global _default_ctx
    with _ctx_lock:
        if _default_ctx is None:
            dev = int(os.environ.get("HGM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            _default_ctx = Context(dev)
        return _default_ctx


def auto_pixel_order(N):
    """Stored pixel order for an N x N image: 4 x 4 tiles (one 128-B
    line of fp64 per tile) whenever 4 | N.  Super-blocks (a second tiling level) are
    supported but measured no better once the banded kernel runs 4 lanes per segment
    (profiles/r1_spmv_sweep_c4_order.jsonl).  Returns (tile, super_block)."""
    return (4 if N % 4 == 0 else 1), 0


def stored_pixel_index(N, tile, super_block=0):
    """Stored position of every reference pixel p = r + c*N of an N x N image in the tiled
    order (N, tile, super_block) (csrc/ops.hip pixel_index): super x super blocks column-major,
    tile x tile tiles inside in tile-column-major order, column-major inside a tile."""
    p = np.arange(N * N, dtype=np.int64)
    r, c = p % N, p // N

    def tiled(S, rr, cc):
        if tile <= 1:
            return rr + cc * S
        tr, tc = rr // tile, cc // tile
        return ((tc * (S // tile) + tr) * tile + (cc % tile)) * tile + (rr % tile)

    if super_block <= 1:
        return tiled(N, r, c)
    S = super_block
    return ((c // S) * (N // S) + (r // S)) * S * S + tiled(S, r % S, c % S)


class SparseOperator:
    """A CSR operator resident in HBM (``hgm_mat``)."""

    def __init__(self, ctx: Context, handle, shape, nnz, dtype):
        self.ctx = ctx
        self._h = handle
        self.shape = shape
        self.nnz = nnz
        self.dtype = dtype
        self._T = None

    @classmethod
    def from_scipy(cls, M, ctx: Context | None = None, dtype=L.HGM_F64):
        ctx = ctx or default_context()
        if not sp.issparse(M):
            M = sp.csr_matrix(np.asarray(M, dtype=np.float64))
        M = M.tocsr()
        rp = np.ascontiguousarray(M.indptr, dtype=np.int64)
        ci = np.ascontiguousarray(M.indices, dtype=np.int32)
        va = np.ascontiguousarray(M.data, dtype=np.float64)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_csr(ctx.handle, M.shape[0], M.shape[1], M.nnz,
                                           rp.ctypes.data_as(L.ip64), ci.ctypes.data_as(L.ip32),
                                           _dp(va), dtype, C.byref(h)), ctx)
        return cls(ctx, h, M.shape, int(M.nnz), dtype)

    @classmethod
    def from_scipy_tiled(cls, M, N, tile, super_block=0, ctx: Context | None = None, dtype=L.HGM_F64):
        """A ray-major operator from a scipy matrix whose columns are the pixels of an ``N x N`` image
        in REFERENCE order, stored with the tiled pixel order ``(tile, super_block)`` (as
        :meth:`siddon` stores its own): prescribed values over a tiled grid."""
        ctx = ctx or default_context()
        M = sp.csr_matrix(M)
        pos = stored_pixel_index(N, tile, super_block)
        Ms = sp.csr_matrix((M.data.copy(), pos[M.indices], M.indptr.copy()), shape=M.shape)   # (sorted in place below)
        Ms.sort_indices()
        rp = np.ascontiguousarray(Ms.indptr, dtype=np.int64)
        ci = np.ascontiguousarray(Ms.indices, dtype=np.int32)
        va = np.ascontiguousarray(Ms.data, dtype=np.float64)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_csr_tiled(ctx.handle, Ms.shape[0], Ms.shape[1], Ms.nnz,
                                                 rp.ctypes.data_as(L.ip64), ci.ctypes.data_as(L.ip32), _dp(va),
                                                 dtype, int(N), int(tile), int(super_block), C.byref(h)), ctx)
        return cls._wrap(ctx, h)

    @classmethod
    def from_csc(cls, M, ctx: Context | None = None, dtype=L.HGM_F64):
        """MATLAB sparse hand-over (CSC, 64-bit indices), transposed on device."""
        ctx = ctx or default_context()
        M = sp.csc_matrix(M)
        M.sort_indices()
        jc = np.ascontiguousarray(M.indptr, dtype=np.int64)
        ir = np.ascontiguousarray(M.indices, dtype=np.int64)
        pr = np.ascontiguousarray(M.data, dtype=np.float64)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_csc(ctx.handle, M.shape[0], M.shape[1], M.nnz,
                                           jc.ctypes.data_as(L.ip64), ir.ctypes.data_as(L.ip64),
                                           _dp(pr), dtype, C.byref(h)), ctx)
        return cls(ctx, h, M.shape, int(M.nnz), dtype)

    @classmethod
    def siddon(cls, N, n_angles, ctx: Context | None = None, dtype=L.HGM_F64, det_offset=None,
               order="auto"):
        """Parallel-beam projector generated on the device.

        ``order`` is the STORED pixel order (invisible at the boundary: products,
        downloads and solves use the reference column-major ``x(:)``): ``"reference"``,
        ``(tile, super_block)``, or ``"auto"`` = :func:`auto_pixel_order`."""
        from .problems import DETECTOR_OFFSET
        ctx = ctx or default_context()
        off = DETECTOR_OFFSET if det_offset is None else det_offset
        tile, sup = auto_pixel_order(N) if order == "auto" else ((1, 0) if order == "reference" else order)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_siddon_ordered(ctx.handle, N, n_angles, off, dtype, int(tile), int(sup),
                                                      C.byref(h)), ctx)
        return cls._wrap(ctx, h)

    @classmethod
    def fanbeam(cls, N, n_angles, ctx: Context | None = None, R=None, span=None, dtype=L.HGM_F64, det_offset=None,
                order="auto"):
        """Fan-beam (curved detector) projector generated on the device, bit-identical to
        :func:`hgmres.problems.fanbeam_projector` (the 'fancurved' geometry of
        run_2D_phantom.m:12-13).  ``span=None``: the fan covering the image's circumscribed
        circle; ``order`` as for :meth:`siddon`."""
        from .problems import DETECTOR_OFFSET, FAN_R
        ctx = ctx or default_context()
        off = DETECTOR_OFFSET if det_offset is None else det_offset
        tile, sup = auto_pixel_order(N) if order == "auto" else ((1, 0) if order == "reference" else order)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_fanbeam(ctx.handle, N, n_angles, float(FAN_R if R is None else R),
                                               float(0.0 if span is None else span), off, dtype, int(tile), int(sup),
                                               C.byref(h)), ctx)
        return cls._wrap(ctx, h)

    @classmethod
    def pixel_backprojector(cls, N, n_angles, ctx: Context | None = None, dtype=L.HGM_F64, det_offset=None,
                            order="auto"):
        """Unmatched pixel-driven back-projector B (n x m) generated on the device, bit-identical
        to :func:`hgmres.problems.pixel_driven_backprojector`.  ``order``: stored pixel (row)
        order, as for :meth:`siddon` (pair it with an A of the same order)."""
        from .problems import DETECTOR_OFFSET
        ctx = ctx or default_context()
        off = DETECTOR_OFFSET if det_offset is None else det_offset
        tile, sup = auto_pixel_order(N) if order == "auto" else ((1, 0) if order == "reference" else order)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_backprojector(ctx.handle, N, n_angles, off, dtype, int(tile), int(sup),
                                                     C.byref(h)), ctx)
        return cls._wrap(ctx, h)

    @classmethod
    def fan_backprojector(cls, N, n_angles, ctx: Context | None = None, R=None, span=None, dtype=L.HGM_F64,
                          det_offset=None, order="auto"):
        """Unmatched pixel-driven back-projector B (n x m) of the fan-beam geometry generated on the
        device, bit-identical to :func:`hgmres.problems.fan_pixel_backprojector`: the ``B != A^T``
        partner of :meth:`fanbeam` with the same ``R``, ``span`` and ``det_offset``.  ``order``:
        stored pixel (row) order, as for :meth:`siddon` (pair it with an A of the same order)."""
        from .problems import DETECTOR_OFFSET, FAN_R
        ctx = ctx or default_context()
        off = DETECTOR_OFFSET if det_offset is None else det_offset
        tile, sup = auto_pixel_order(N) if order == "auto" else ((1, 0) if order == "reference" else order)
        h = C.c_void_p()
        _check(L.load().hgm_mat_create_fan_backprojector(ctx.handle, N, n_angles, float(FAN_R if R is None else R),
                                                         float(0.0 if span is None else span), off, dtype,
                                                         int(tile), int(sup), C.byref(h)), ctx)
        return cls._wrap(ctx, h)

    def pixel_order(self, which="cols"):
        """(N, tile, super_block) of the stored row/column index order; N = 0: reference order."""
        n_, t_, s_ = C.c_int(), C.c_int(), C.c_int()
        _check(L.load().hgm_mat_order(self._h, 0 if which == "rows" else 1, C.byref(n_), C.byref(t_),
                                      C.byref(s_)), self.ctx)
        return n_.value, t_.value, s_.value

    @classmethod
    def _wrap(cls, ctx, h):
        r, c_, nz, dt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        _check(L.load().hgm_mat_info(h, C.byref(r), C.byref(c_), C.byref(nz), C.byref(dt)), ctx)
        return cls(ctx, h, (r.value, c_.value), nz.value, dt.value)

    @property
    def T(self) -> "SparseOperator":
        """Device transpose (cached)."""
        if self._T is None:
            h = C.c_void_p()
            _check(L.load().hgm_mat_transpose(self.ctx.handle, self._h, C.byref(h)), self.ctx)
            self._T = SparseOperator._wrap(self.ctx, h)
            self._T._T = self
        return self._T

    def to_scipy(self) -> sp.csr_matrix:
        rows, cols = self.shape
        rp = np.empty(rows + 1, dtype=np.int64)
        ci = np.empty(max(self.nnz, 1), dtype=np.int32)
        va = np.empty(max(self.nnz, 1), dtype=np.float64)
        _check(L.load().hgm_mat_download(self.ctx.handle, self._h, rp.ctypes.data_as(L.ip64),
                                         ci.ctypes.data_as(L.ip32), _dp(va)), self.ctx)
        M = sp.csr_matrix((va[: self.nnz], ci[: self.nnz], rp), shape=self.shape)
        M.has_sorted_indices = False
        return M

    def row_ptr(self) -> np.ndarray:
        """The CSR row pointers only (rows + 1 int64; e.g. the nnz weights of a shard plan)."""
        rp = np.empty(self.shape[0] + 1, dtype=np.int64)
        _check(L.load().hgm_mat_download(self.ctx.handle, self._h, rp.ctypes.data_as(L.ip64), None, None),
               self.ctx)
        return rp

    def row_slice(self, lo: int, hi: int) -> "SparseOperator":
        """Rows [lo, hi) as a new device operator (pixel shard ``B(P_g,:)``)."""
        h = C.c_void_p()
        _check(L.load().hgm_mat_row_slice(self.ctx.handle, self._h, int(lo), int(hi), C.byref(h)), self.ctx)
        return SparseOperator._wrap(self.ctx, h)

    def tune(self, variant: int, group: int = 0):
        """Select the SpMV kernel variant (bits: 1 paired 16-B loads, 2 nontemporal,
        4 XCD-aware order) and lanes per row."""
        _check(L.load().hgm_mat_tune(self._h, int(variant), int(group)), self.ctx)

    def set_bands(self, band_width: int, group: int = 0):
        """Column banding of the x gather (0 = off, -1 = automatic)."""
        _check(L.load().hgm_mat_set_bands(self.ctx.handle, self._h, int(band_width), int(group)), self.ctx)

    def matvec_device(self, x_ptr: int, y_ptr: int):
        _check(L.load().hgm_spmv(self.ctx.handle, self._h, C.c_void_p(x_ptr), C.c_void_p(y_ptr)), self.ctx)

    def __matmul__(self, x):
        """Host convenience y = M @ x (copies through HBM)."""
        x = _f64(x, self.shape[1], "x")
        ctx = self.ctx
        lib = L.load()
        es = 8 if self.dtype == L.HGM_F64 else 4
        xd, yd = C.c_void_p(), C.c_void_p()
        _check(lib.hgm_dev_alloc(ctx.handle, es * max(1, self.shape[1]), C.byref(xd)), ctx)
        _check(lib.hgm_dev_alloc(ctx.handle, es * max(1, self.shape[0]), C.byref(yd)), ctx)
        try:
            xs = x if es == 8 else x.astype(np.float32)
            _check(lib.hgm_memcpy_h2d(ctx.handle, xd, xs.ctypes.data_as(C.c_void_p), es * self.shape[1]), ctx)
            _check(lib.hgm_spmv(ctx.handle, self._h, xd, yd), ctx)
            y = np.empty(self.shape[0], dtype=np.float64 if es == 8 else np.float32)
            _check(lib.hgm_memcpy_d2h(ctx.handle, y.ctypes.data_as(C.c_void_p), yd, es * self.shape[0]), ctx)
        finally:
            lib.hgm_dev_free(ctx.handle, xd)
            lib.hgm_dev_free(ctx.handle, yd)
        return y.astype(np.float64)

    def close(self):
        if self._T is not None and self._T is not self:
            T, self._T = self._T, None
            T._T = None
        if self._h:
            L.load().hgm_mat_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass


def _ld_view(M):
    """(flat array to upload, leading dimension) of a 2-D array: a column-major view with a leading
    dimension larger than its row count (``buf[:rows, :]`` of an ``ld x k`` Fortran array) is passed with
    that leading dimension and its padding rows (except past the last column); anything else is copied
    to a tight Fortran array."""
    rows, k = M.shape
    es = M.itemsize
    if not (M.strides[0] == es and (k == 1 or (M.strides[1] % es == 0 and M.strides[1] >= rows * es))):
        M = np.asfortranarray(M)
    ld = rows if k == 1 else M.strides[1] // es
    cnt = ld * (k - 1) + rows
    flat = np.lib.stride_tricks.as_strided(M, shape=(cnt,), strides=(es,)) if ld != rows else M.reshape(-1, order="F")
    return np.ascontiguousarray(flat), ld


class _DevArrays:
    """Device arrays of ``es``-byte elements for the device-pointer hooks (freed on exit)."""

    def __init__(self, ctx, es=8):
        self.ctx, self.lib, self.es, self.ptrs = ctx, L.load(), es, []

    def alloc(self, count):
        p = C.c_void_p()
        _check(self.lib.hgm_dev_alloc(self.ctx.handle, self.es * max(1, int(count)), C.byref(p)), self.ctx)
        self.ptrs.append(p)
        return p

    def upload(self, flat):
        p = self.alloc(flat.size)
        _check(self.lib.hgm_memcpy_h2d(self.ctx.handle, p, flat.ctypes.data_as(C.c_void_p), self.es * flat.size),
               self.ctx)
        return p

    def download(self, p, out):
        """Fill the host array ``out`` (contiguous in memory) from the device array ``p``."""
        _check(self.lib.hgm_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), p, self.es * out.size),
               self.ctx)
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            if p.value:
                self.lib.hgm_dev_free(self.ctx.handle, p)
        return False


def spmv_ab(A: "SparseOperator", B: "SparseOperator", q):
    """(B*q, A*(B*q)) through ``hgm_spmv_ab`` (host arrays in, host arrays out): the m-space
    operator of the AB solvers, one pass over B when B is A' value for value (fused.hip)."""
    ctx = A.ctx
    lib = L.load()
    m, n = A.shape
    es = 8 if A.dtype == L.HGM_F64 else 4
    dt = np.float64 if es == 8 else np.float32
    q = np.ascontiguousarray(np.asarray(q, dtype=dt).reshape(-1))
    if q.shape[0] != m:
        raise ValueError(f"q has length {q.shape[0]}, expected {m}")
    with _DevArrays(ctx, es) as dev:
        qd, bqd, abqd = dev.upload(q), dev.alloc(n), dev.alloc(m)
        _check(lib.hgm_spmv_ab(ctx.handle, A._h, B._h, qd, bqd, abqd), ctx)
        bq, abq = dev.download(bqd, np.empty(n, dtype=dt)), dev.download(abqd, np.empty(m, dtype=dt))
    return bq.astype(np.float64), abq.astype(np.float64)


def _mm_X(X, n, what):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"X has shape {X.shape}, expected ({n}, nvec)")
    nv = X.shape[1]
    if not 1 <= nv <= 8:
        raise ValueError(f"{what} takes 1 to 8 vectors, not {nv}")
    return X, nv


def _mm_device(ctx, m, n, nv, X, call):
    """Upload X (n x nv), run ``call(X_dev, Y_dev)``, download Y (m x nv)."""
    with _DevArrays(ctx) as dev:
        xd, yd = dev.upload(np.asfortranarray(X).reshape(-1, order="F")), dev.alloc(m * nv)
        _check(call(xd, yd), ctx)
        return dev.download(yd, np.empty((m, nv), order="F"))


def spmm(A: "SparseOperator", X):
    """``A @ X`` for an ``n x nvec`` host array ``X`` (``1 <= nvec <= 8``) through ``hgm_spmm``: the
    operator's entries are read once for all columns (spmm.hip).  fp64 operators.  A column's bits do not
    depend on ``nvec``, on its position, or on the other columns."""
    m, n = A.shape
    X, nv = _mm_X(X, n, "spmm")
    if A.dtype != L.HGM_F64:
        raise ValueError("spmm: fp64 operators only")
    ctx = A.ctx
    lib = L.load()
    return _mm_device(ctx, m, n, nv, X, lambda xd, yd: lib.hgm_spmm(ctx.handle, A._h, nv, xd, max(n, 1), yd, max(m, 1)))


class GaussianPerturbation:
    """``scale * randn(rows, cols)`` that is never stored: the dense Gaussian back-projector perturbation of
    ``plot_error_vs_mismatch_norm.m:16`` / ``run_2D_phantom.m:87`` (``E = randn(size(A'))``) as a pure function of
    ``(seed, i, j)``, regenerated on the device inside every product (``hgm_gauss_*``, csrc/gauss.hip;
    :func:`hgmres.problems.gaussian_entries` is the host twin).  Takes ``E``'s place in :func:`spmm_pert`,
    :func:`gmres_bounds_mismatch`, :func:`arnoldi_mismatch` and ``analysis.error_vs_mismatch_norm``.  ``seed`` is
    64-bit.  ``scale`` multiplies the coefficients on the host (one rounding); the device handle is unscaled."""

    ENTRIES_MAX = 1 << 27

    def __init__(self, rows, cols, seed=0, *, scale=1.0, ctx=None):
        rows, cols, seed, scale = int(rows), int(cols), int(seed), float(scale)
        if rows < 1 or cols < 1:
            raise ValueError(f"GaussianPerturbation: rows, cols >= 1, not ({rows}, {cols})")
        if not 0 <= seed < 1 << 64:
            raise ValueError("GaussianPerturbation: seed is an unsigned 64-bit integer")
        if not np.isfinite(scale):
            raise ValueError("GaussianPerturbation: scale must be finite")
        self.ctx = ctx or default_context()
        self.shape, self.seed, self.scale = (rows, cols), seed, scale
        h = C.c_void_p()
        _check(L.load().hgm_gauss_create(self.ctx.handle, rows, cols, seed, C.byref(h)), self.ctx)
        self._handle = h
        self._root = self          # the instance whose handle (and cached norm) this one uses

    def _with_scale(self, scale):
        G = object.__new__(GaussianPerturbation)
        G.ctx, G.shape, G.seed, G.scale = self.ctx, self.shape, self.seed, float(scale)
        G._root = self._root
        return G

    @property
    def _h(self):
        return self._root._handle

    def close(self):
        """Frees the handle; an instance made by :meth:`normalized` shares its parent's and frees nothing."""
        if getattr(self, "_root", None) is self and getattr(self, "_handle", None):
            L.load().hgm_gauss_destroy(self._handle)
            self._handle = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass

    def _fro_raw(self):
        f = C.c_double()
        _check(L.load().hgm_gauss_fro(self.ctx.handle, self._h, C.byref(f)), self.ctx)
        return f.value

    def fro(self):
        """``|scale| * ||G||_F`` (one generation pass on first use, then cached in the handle)."""
        return abs(self.scale) * self._fro_raw()

    def normalized(self):
        """The same seed with ``scale = 1 / ||G||_F``: ``E / norm(E, 'fro')`` of
        ``plot_error_vs_mismatch_norm.m:17``.  Shares this instance's handle."""
        return self._with_scale(1.0 / self._fro_raw())

    def entries(self, rows=slice(None), cols=slice(None)):
        """The block ``[rows, cols]`` (unit-step slices) of ``scale * G`` as a host array."""
        i0, i1, si = rows.indices(self.shape[0])
        j0, j1, sj = cols.indices(self.shape[1])
        if si != 1 or sj != 1:
            raise ValueError("entries: unit-step slices only")
        ni, nj = max(0, i1 - i0), max(0, j1 - j0)
        if ni * nj > self.ENTRIES_MAX:
            raise ValueError(f"entries: at most 2^27 entries per call, not {ni} x {nj}")
        out = np.empty((ni, nj), order="F")
        if ni and nj:
            _check(L.load().hgm_gauss_entries(self.ctx.handle, self._h, i0, ni, j0, nj, _dp(out), ni), self.ctx)
        return out if self.scale == 1.0 else out * self.scale

    def to_dense(self):
        if self.shape[0] * self.shape[1] > self.ENTRIES_MAX:
            raise ValueError(f"to_dense: {self.shape[0]} x {self.shape[1]} is above the 2^27-entry cap")
        return self.entries()

    def matmat(self, X, coefs=None):
        """``coefs[r] * scale * (G @ X[:, r])`` for a ``cols x nvec`` host array (``1 <= nvec <= 8``;
        ``coefs=None``: ones) through ``hgm_gauss_mm``.  A column's bits depend on its own data and coefficient
        only: not on ``nvec``, its position, the other columns or their coefficients."""
        m, n = self.shape
        X, nv = _mm_X(X, n, "matmat")
        cf = None
        if coefs is not None or self.scale != 1.0:
            cf = np.ones(nv) if coefs is None else _coefs(coefs, nv, nv, f"matmat of {nv} vectors")
            cf = _scaled_coefs(cf, self.scale, "matmat")
        lib = L.load()
        return _mm_device(self.ctx, m, n, nv, X,
                          lambda xd, yd: lib.hgm_gauss_mm(self.ctx.handle, self._h, nv, _dp(cf), xd, n, yd, m))


def _scaled_coefs(cf, scale, what):
    """``cf * scale`` (one rounding), refused when a product is not finite."""
    with np.errstate(over="ignore"):
        out = cf if scale == 1.0 else np.ascontiguousarray(cf * scale)
    if not np.all(np.isfinite(out)):
        raise ValueError(f"{what}: every coefficient times the scale must be finite")
    return out


def _spmm_pert_gauss(B0, G, coefs, X):
    if not isinstance(B0, SparseOperator):
        raise TypeError("B0 must be a SparseOperator (hgmres.as_operator)")
    if tuple(G.shape) != tuple(B0.shape):
        raise ValueError(f"G has shape {G.shape}, expected B0's {B0.shape}")
    if B0.dtype != L.HGM_F64:
        raise ValueError("perturbed product: fp64 operators only")
    m, n = B0.shape
    X, nv = _mm_X(X, n, "spmm_pert")
    cf = _scaled_coefs(_coefs(coefs, nv, nv, f"spmm_pert of {nv} vectors"), G.scale, "spmm_pert")
    ctx = B0.ctx
    lib = L.load()
    return _mm_device(ctx, m, n, nv, X,
                      lambda xd, yd: lib.hgm_spmm_pert_gauss(ctx.handle, B0._h, G._h, nv, _dp(cf), xd, n, yd, m))


def _pert_pair(B0, E):
    """The (B0, E) operator pair of a perturbed product, checked on the host."""
    if not isinstance(B0, SparseOperator) or not isinstance(E, SparseOperator):
        raise TypeError("B0 and E must be SparseOperators (hgmres.as_operator)")
    if E.shape != B0.shape:
        raise ValueError(f"E has shape {E.shape}, expected B0's {B0.shape}")
    if B0.dtype != L.HGM_F64 or E.dtype != L.HGM_F64:
        raise ValueError("perturbed product: fp64 operators only")


def _coefs(coefs, lo, hi, what):
    cf = np.ascontiguousarray(np.asarray(coefs, dtype=np.float64).reshape(-1))
    if not lo <= cf.size <= hi:
        raise ValueError(f"{what} takes {lo} to {hi} coefficients, not {cf.size}")
    if not np.all(np.isfinite(cf)):
        raise ValueError(f"{what}: every coefficient must be finite")
    return cf


def spmm_pert(B0: "SparseOperator", E: "SparseOperator", coefs, X):
    """``B0 @ X[:, r] + coefs[r] * (E @ X[:, r])`` for an ``n x nvec`` host array ``X`` (``1 <= nvec <= 8``) through
    ``hgm_spmm_pert``: column r is the product with ``B0 + coefs[r] * E``, which is never formed, and both
    operators' entries are read once for all columns (spmm.hip).  ``E`` has ``B0``'s shape; when it also has its
    sparsity pattern the index stream and the x gathers are shared.  A column's bits depend on its coefficient
    only: not on ``nvec``, its position, the other columns or their coefficients.

    ``E`` may be a :class:`GaussianPerturbation` (``hgm_spmm_pert_gauss``): column r is then bit for bit
    ``spmm(B0, X)[:, r] + (coefs[r] * E.scale) * (G @ X[:, r])`` with ``G @ X`` the bits of ``E.matmat``'s unscaled
    product."""
    if isinstance(E, GaussianPerturbation):
        return _spmm_pert_gauss(B0, E, coefs, X)
    _pert_pair(B0, E)
    m, n = B0.shape
    X, nv = _mm_X(X, n, "spmm_pert")
    cf = _coefs(coefs, nv, nv, f"spmm_pert of {nv} vectors")
    ctx = B0.ctx
    lib = L.load()
    return _mm_device(ctx, m, n, nv, X, lambda xd, yd: lib.hgm_spmm_pert(ctx.handle, B0._h, E._h, nv, _dp(cf), xd,
                                                                          max(n, 1), yd, max(m, 1)))


def fused_plan_info(A: "SparseOperator", B: "SparseOperator"):
    """The one-pass plan of (A, B) under the context's options (built if needed): dict with the
    build seconds, a checksum over every plan array, the partial slots and whether the device built
    the ray sets (``hgm_fused_plan_info``), and the compact value stream (``hgm_fused_vstream_info``):
    whether the pass reads it, the share of coded entries, its value bytes and the plan's device bytes."""
    ctx = A.ctx
    bs, ck, ns, dv = C.c_double(), C.c_uint64(), C.c_int64(), C.c_int()
    _check(L.load().hgm_fused_plan_info(ctx.handle, A._h, B._h, C.byref(bs), C.byref(ck), C.byref(ns), C.byref(dv)),
           ctx)
    va, cov, vb, pb = C.c_int(), C.c_double(), C.c_int64(), C.c_int64()
    _check(L.load().hgm_fused_vstream_info(ctx.handle, A._h, B._h, C.byref(va), C.byref(cov), C.byref(vb),
                                           C.byref(pb)), ctx)
    return {"build_s": bs.value, "checksum": ck.value, "nslot": ns.value, "device_built": bool(dv.value),
            "vstream": bool(va.value), "vstream_coverage": cov.value, "vstream_value_bytes": vb.value,
            "plan_bytes": pb.value}


def as_operator(M, ctx=None, dtype=L.HGM_F64) -> SparseOperator:
    if isinstance(M, SparseOperator):
        return M
    return SparseOperator.from_scipy(M, ctx=ctx, dtype=dtype)


def _ops(A, B, ctx):
    ctx = ctx or (A.ctx if isinstance(A, SparseOperator) else default_context())
    Ao = as_operator(A, ctx)
    if B is None:
        Bo = Ao.T
    else:
        Bo = as_operator(B, ctx, Ao.dtype)
    if Bo.shape != (Ao.shape[1], Ao.shape[0]):
        raise ValueError(f"dimension mismatch: A is {Ao.shape}, B is {Bo.shape} (expected size(A'))")
    return ctx, Ao, Bo


def _opts(orth="mgs", H_out=None, device_ptrs=False, explicit_residual=False):
    o = L.hgm_opts()
    o.flags = (L.HGM_DEVICE_PTRS if device_ptrs else 0) | (L.HGM_EXPLICIT_RESIDUAL if explicit_residual else 0)
    o.orth = L.HGM_CGS2 if str(orth).lower() == "cgs2" else L.HGM_MGS
    o.H_out = _dp(H_out) if H_out is not None else None
    return o


def _gmres_call(fn_name, A, B, b, x_true, tol, maxit, lam, ctx, orth, return_H, extra=(), explicit_residual=False):
    ctx, Ao, Bo = _ops(A, B, ctx)
    m, n = Ao.shape
    maxit = int(maxit)
    b = _f64(b, m, "b")
    xt = _f64(x_true, n, "x_true")
    x = np.zeros(n)
    err = np.zeros(maxit)
    res = np.zeros(maxit)
    it = C.c_int(0)
    H = np.zeros((maxit + 1) * maxit) if return_H else None
    o = _opts(orth, H, explicit_residual=explicit_residual)
    fn = getattr(L.load(), fn_name)
    if fn_name == "hgm_gmres_bounds_ex":
        lam_, side, hyb = extra
        rc = fn(ctx.handle, C.byref(o), Ao._h, Bo._h, _dp(b), _dp(xt), float(tol), maxit, float(lam_), side, hyb,
                _dp(x), _dp(err), _dp(res), C.byref(it))
    else:
        rc = fn(ctx.handle, C.byref(o), Ao._h, Bo._h, _dp(b), _dp(xt), float(tol), maxit, float(lam),
                _dp(x), _dp(err), _dp(res), C.byref(it))
    _check(rc, ctx)
    k = it.value
    out = (x, err[:k].copy(), res[:k].copy(), k)
    if return_H:
        out = out + (H.reshape(maxit, maxit + 1).T.copy(),)
    return out


# ---------------------------------------------------------------------------
# Reference solver signatures
# ---------------------------------------------------------------------------
def hybrid_ab_gmres_rtp(A, B, b, x_true, tol, maxit, lambda_, *, ctx=None, orth="mgs", return_H=False,
                        explicit_residual=False):
    """``[x, error_norm, residual_norm, niters] = hybrid_ab_gmres_rtp(A,B,b,x_true,tol,maxit,lambda)``
    (hybrid_ab_gmres_rtp.m:1-45): n-space Arnoldi on ``B*A + lambda*I``, projected
    Tikhonov ``(AQk'AQk + lambda I) y = AQk' b``.  ``explicit_residual`` monitors
    ``norm(b - A*x)`` with an SpMV of x instead of ``b - (A*Q) y`` (HGM_EXPLICIT_RESIDUAL)."""
    return _gmres_call("hgm_hybrid_ab_gmres_rtp_ex", A, B, b, x_true, tol, maxit, lambda_, ctx, orth, return_H,
                       explicit_residual=explicit_residual)


def hybrid_ba_gmres_rtp(A, B, b, x_true, tol, maxit, lambda_, *, ctx=None, orth="mgs", return_H=False,
                        explicit_residual=False):
    """``hybrid_ba_gmres_rtp.m:1-42``: Arnoldi on ``B*A + lambda*I``, ``yk = Hk \\ beta e1``."""
    return _gmres_call("hgm_hybrid_ba_gmres_rtp_ex", A, B, b, x_true, tol, maxit, lambda_, ctx, orth, return_H,
                       explicit_residual=explicit_residual)


def _delta_ops(DeltaM, ctx):
    """DeltaM as one device operator, or as a factored product (L, R) = L*R applied to vectors."""
    if isinstance(DeltaM, (tuple, list)):
        L_, R_ = DeltaM
        return as_operator(_sparse(L_), ctx), as_operator(_sparse(R_), ctx)
    return as_operator(_sparse(DeltaM), ctx), None


def _sparse(M):
    if isinstance(M, SparseOperator) or sp.issparse(M):
        return M
    return sp.csr_matrix(np.asarray(M, dtype=np.float64))


def _bounds(A, B, b, x_true, tol, maxit, lam, side, hybrid, ctx, orth, return_H, explicit_residual=False,
            DeltaM=None, ritz_steps=0, return_ritz=False):
    if DeltaM is None:
        out = _gmres_call("hgm_gmres_bounds_ex", A, B, b, x_true, tol, maxit, lam, ctx, orth, return_H,
                          extra=(lam, side, hybrid), explicit_residual=explicit_residual)
        # outputs 5-8 need DeltaM (the reference's 8th / 7th argument)
        return out[:4] + (None, None, None, None) + out[4:]
    # outputs 5-8: filter factors phi and their first-order perturbation dphi (*_bounds.m:42-81)
    ctx, Ao, Bo = _ops(A, B, ctx)
    DL, DR = _delta_ops(DeltaM, ctx)
    m, n = Ao.shape
    maxit = int(maxit)
    b = _f64(b, m, "b")
    xt = _f64(x_true, n, "x_true")
    x, err, res, it = np.zeros(n), np.zeros(maxit), np.zeros(maxit), C.c_int(0)
    phi = np.zeros(maxit * maxit)
    dphi = np.zeros(maxit * maxit)
    mu = np.zeros(maxit)
    rres = np.zeros(maxit)
    H = np.zeros((maxit + 1) * maxit)          # also tells a breakdown at iteration k (below)
    o = _opts(orth, H, explicit_residual=explicit_residual)
    _check(L.load().hgm_gmres_bounds_filter(ctx.handle, C.byref(o), Ao._h, Bo._h, _dp(b), _dp(xt), float(tol),
                                            maxit, float(lam), side, hybrid, DL._h, DR._h if DR else None,
                                            int(ritz_steps), _dp(x), _dp(err), _dp(res), C.byref(it), _dp(phi),
                                            _dp(dphi), _dp(mu), _dp(rres)), ctx)
    k = it.value
    P_ = phi.reshape(maxit, maxit)
    D_ = dphi.reshape(maxit, maxit)
    phi_iter = [P_[j, : j + 1].copy() for j in range(k)]
    dphi_iter = [D_[j, : j + 1].copy() for j in range(k)]
    Hm = H.reshape(maxit, maxit + 1).T
    if k and Hm[k, k - 1] == 0.0:   # breakdown at iteration k (*_bounds.m:31 before :80): phi_iter{k} = []
        phi_iter[-1] = np.zeros(0)
        dphi_iter[-1] = np.zeros(0)
    out = (x, err[:k].copy(), res[:k].copy(), k, phi_iter[-1], dphi_iter[-1], phi_iter, dphi_iter)
    if return_H:
        out = out + (Hm.copy(),)
    if return_ritz:
        out = out + (mu[:k].copy(), rres[:k].copy())
    return out


def ABgmres_hybrid_bounds(A, B, b, x_true, tol, maxit, lambda_, DeltaM=None, *, ctx=None, orth="mgs", return_H=False,
                             explicit_residual=False, ritz_steps=0, return_ritz=False):
    """``ABgmres_hybrid_bounds.m``: m-space Arnoldi on ``A*B``, PTR Tikhonov, ``x = B*z``; outputs 5-8
    (filter factors) when ``DeltaM`` (a matrix, or a factored pair ``(L, R)`` = L*R) is given."""
    return _bounds(A, B, b, x_true, tol, maxit, lambda_, L.HGM_SIDE_AB, 1, ctx, orth, return_H,
                   explicit_residual=explicit_residual,
                   DeltaM=DeltaM, ritz_steps=ritz_steps, return_ritz=return_ritz)


def ABgmres_nonhybrid_bounds(A, B, b, x_true, tol, maxit, DeltaM=None, *, ctx=None, orth="mgs", return_H=False,
                             explicit_residual=False, ritz_steps=0, return_ritz=False):
    """``ABgmres_nonhybrid_bounds.m`` (outputs 5-8 with ``DeltaM``)."""
    return _bounds(A, B, b, x_true, tol, maxit, 0.0, L.HGM_SIDE_AB, 0, ctx, orth, return_H,
                   explicit_residual=explicit_residual,
                   DeltaM=DeltaM, ritz_steps=ritz_steps, return_ritz=return_ritz)


def BAgmres_hybrid_bounds(A, B, b, x_true, tol, maxit, lambda_, DeltaM=None, *, ctx=None, orth="mgs", return_H=False,
                             explicit_residual=False, ritz_steps=0, return_ritz=False):
    """``BAgmres_hybrid_bounds.m``: n-space Arnoldi on ``B*A``, PTR Tikhonov (outputs 5-8 with ``DeltaM``)."""
    return _bounds(A, B, b, x_true, tol, maxit, lambda_, L.HGM_SIDE_BA, 1, ctx, orth, return_H,
                   explicit_residual=explicit_residual,
                   DeltaM=DeltaM, ritz_steps=ritz_steps, return_ritz=return_ritz)


def BAgmres_nonhybrid_bounds(A, B, b, x_true, tol, maxit, DeltaM=None, *, ctx=None, orth="mgs", return_H=False,
                             explicit_residual=False, ritz_steps=0, return_ritz=False):
    """``BAgmres_nonhybrid_bounds.m`` (outputs 5-8 with ``DeltaM``).  The reference forms ``M = B*A``
    explicitly (``:4``); here the operator is applied as ``B*(A*q)``."""
    return _bounds(A, B, b, x_true, tol, maxit, 0.0, L.HGM_SIDE_BA, 0, ctx, orth, return_H,
                   explicit_residual=explicit_residual,
                   DeltaM=DeltaM, ritz_steps=ritz_steps, return_ritz=return_ritz)


class SweepResult:
    """Outputs of :func:`gmres_lambda_sweep`.  ``err``, ``res``, ``sol``: ``maxit x nlam`` surfaces
    (row k-1 = iteration k, column l = ``lambdas[l]``; NaN past ``niters[l]``); ``niters``: per lambda;
    ``X`` (``n x nlam``) and ``H`` when requested, else None; ``ksteps``: Arnoldi steps performed."""

    def __init__(self, lambdas, err, res, sol, niters, X, H, ksteps):
        self.lambdas, self.err, self.res, self.sol = lambdas, err, res, sol
        self.niters, self.X, self.H, self.ksteps = niters, X, H, ksteps


def _side(side):
    if side in (L.HGM_SIDE_AB, L.HGM_SIDE_BA) and not isinstance(side, str):
        return int(side)
    s = str(side).lower()
    if s not in ("ab", "ba"):
        raise ValueError(f"side must be 'ab' or 'ba', not {side!r}")
    return L.HGM_SIDE_AB if s == "ab" else L.HGM_SIDE_BA


def gmres_lambda_sweep(A, B, b, x_true, tol, maxit, lambdas, side, *, ctx=None, orth="mgs", return_x=False,
                       return_H=False):
    """``ABgmres_hybrid_bounds`` / ``BAgmres_hybrid_bounds`` (``side`` 'ab' / 'ba') for every lambda of
    ``lambdas`` from ONE Arnoldi (``hgm_gmres_bounds_sweep``): lambda enters only the projected solve
    ``yk = (Hk'*Hk + lambda*eye(k)) \\ (Hk'*tk)`` (``*_hybrid_bounds.m:34-36``).  Column l of the result's
    surfaces is the history of the single solve at ``lambdas[l]``; ``sol`` adds ``||x_k||`` (the L-curve).
    ``x_true`` may be None (``err`` stays NaN)."""
    ctx, Ao, Bo = _ops(A, B, ctx)
    m, n = Ao.shape
    maxit = int(maxit)
    b = _f64(b, m, "b")
    xt = _f64(x_true, n, "x_true") if x_true is not None else None
    lam = np.ascontiguousarray(np.asarray(lambdas, dtype=np.float64).reshape(-1))
    nl = lam.size
    err, res, sol = (np.full(maxit * max(nl, 1), np.nan) for _ in range(3))
    X = np.zeros(n * max(nl, 1)) if return_x else None
    nit = np.zeros(max(nl, 1), dtype=np.int32)
    ks = C.c_int(0)
    H = np.zeros((maxit + 1) * maxit) if return_H else None
    o = _opts(orth, H)
    _check(L.load().hgm_gmres_bounds_sweep(ctx.handle, C.byref(o), Ao._h, Bo._h, _dp(b), _dp(xt), float(tol), maxit,
                                           _dp(lam), int(nl), _side(side), _dp(X), _dp(err), _dp(res), _dp(sol),
                                           nit.ctypes.data_as(C.POINTER(C.c_int)), C.byref(ks)), ctx)
    shp = (nl, maxit)
    return SweepResult(lam, err.reshape(shp).T.copy(), res.reshape(shp).T.copy(), sol.reshape(shp).T.copy(),
                       nit.astype(int), X.reshape(nl, n).T.copy() if return_x else None,
                       H.reshape(maxit, maxit + 1).T.copy() if return_H else None, ks.value)


def _col_lambdas(lambdas, ncols, noun):
    """``lambdas`` (or None) as a contiguous vector with one entry per ``noun`` (``ncols`` None: any length)."""
    if lambdas is None:
        return None
    lam = np.ascontiguousarray(np.asarray(lambdas, dtype=np.float64).reshape(-1))
    if ncols is not None and lam.size != ncols:
        raise ValueError(f"lambdas has {lam.size} entries, expected one per {noun} ({ncols})")
    return lam


def _col_x_true(x_true, n, ncols):
    """``(xt, ldxt)`` of a lockstep solve: none, one vector shared by every column (``ldxt`` 0) or ``n x ncols``."""
    if x_true is None:
        return None, 0
    xt = np.asarray(x_true, dtype=np.float64)
    if xt.ndim == 1 or (xt.ndim == 2 and xt.shape[1] == 1 and ncols != 1):
        return _f64(xt, n, "x_true"), 0                         # one column shared by every right-hand side
    if xt.shape != (n, ncols):
        raise ValueError(f"x_true has shape {xt.shape}, expected ({n},) or ({n}, {ncols})")
    return np.asfortranarray(xt), max(n, 1)


def _batch_outputs(n, maxit, ncols, nhist):
    """``(X, histories, niters)`` of a lockstep solve before the call: NaN, and no iterations."""
    return (np.full((n, ncols), np.nan, order="F"), [np.full((maxit, ncols), np.nan, order="F") for _ in range(nhist)],
            np.zeros(ncols, dtype=np.int32))


def _H_blocks(H, ncols, k):
    """``ncols`` consecutive column-major ``(k+1) x k`` blocks as an ``ncols x (k+1) x k`` array."""
    return H.reshape(ncols, k, k + 1).transpose(0, 2, 1).copy()


def _bounds_lockstep(ctx, n, maxit, ncols, orth, return_H, call):
    """The outputs of a lockstep ``*_bounds`` solve, ``call(opts, X, ldx, err, res, niters, status)`` and the
    :class:`BatchResult`; a column without an x (breakdown at k = 1) does not raise."""
    X, (err, res), nit = _batch_outputs(n, maxit, ncols, 2)
    st = np.zeros(ncols, dtype=np.int32)
    H = np.zeros((maxit + 1) * maxit * ncols) if return_H else None
    o = _opts(orth, H)
    ip = C.POINTER(C.c_int)
    rc = call(C.byref(o), _dp(X), max(n, 1), _dp(err), _dp(res), nit.ctypes.data_as(ip), st.ctypes.data_as(ip))
    if rc != L.HGM_E_NOT_ASSIGNED:
        _check(rc, ctx)
    return BatchResult(X, err, res, nit.astype(int), st.astype(int), _H_blocks(H, ncols, maxit) if return_H else None)


class BatchResult:
    """Outputs of :func:`gmres_bounds_batch`.  ``x``: ``n x nrhs`` (a column that broke down at k = 1 is
    NaN); ``error_norm``, ``residual_norm``: ``maxit x nrhs`` (row k-1 = iteration k; NaN past
    ``niters[j]``); ``niters``, ``status`` (``HGM_OK`` or ``HGM_E_NOT_ASSIGNED``): per column; ``H``:
    ``nrhs x (maxit+1) x maxit`` when requested, else None."""

    def __init__(self, x, error_norm, residual_norm, niters, status, H):
        self.x, self.error_norm, self.residual_norm = x, error_norm, residual_norm
        self.niters, self.status, self.H = niters, status, H


def gmres_bounds_batch(A, B, Bm, x_true, tol, maxit, side, *, lambdas=None, ctx=None, orth="mgs", return_H=False):
    """``nrhs`` lockstep solves of one ``*_bounds`` solver against one operator pair
    (``hgm_gmres_bounds_batch``): column j of every output is what ``{AB,BA}gmres_{hybrid,nonhybrid}_bounds``
    returns for ``b = Bm[:, j]``, ``x_true[:, j]`` and ``lambdas[j]``.  ``side`` is 'ab' or 'ba';
    ``lambdas=None`` selects the non-hybrid solver.  ``x_true`` is ``n x nrhs``, one vector shared by every
    column, or None (the error histories stay NaN).  The operators' entries are read once per group of up
    to 8 running columns and iteration; a finished column leaves the batch.  A column that breaks down at
    k = 1 does not raise: its ``status`` is ``HGM_E_NOT_ASSIGNED`` and the other columns finish."""
    sd = _side(side)
    m, n = A.shape
    maxit = int(maxit)
    Bm = np.asarray(Bm, dtype=np.float64)
    if Bm.ndim == 1:
        Bm = Bm.reshape(-1, 1)
    if Bm.ndim != 2 or Bm.shape[0] != m or Bm.shape[1] < 1:
        raise ValueError(f"Bm has shape {Bm.shape}, expected ({m}, nrhs)")
    nrhs = Bm.shape[1]
    if nrhs > 64:
        raise ValueError(f"at most 64 right-hand sides per call, not {nrhs}")
    lam = _col_lambdas(lambdas, nrhs, "right-hand side")
    xt, ldxt = _col_x_true(x_true, n, nrhs)
    if maxit < 1:
        raise ValueError("maxit must be >= 1")
    ctx, Ao, Bo = _ops(A, B, ctx)
    Bf = np.asfortranarray(Bm)
    fn = L.load().hgm_gmres_bounds_batch
    return _bounds_lockstep(ctx, n, maxit, nrhs, orth, return_H, lambda o, *out: fn(
        ctx.handle, o, Ao._h, Bo._h, _dp(Bf), max(m, 1), nrhs, _dp(xt), ldxt, float(tol), maxit, _dp(lam), sd,
        0 if lam is None else 1, *out))


def _mismatch_args(A, B0, E, coefs, b, what):
    """Host-side checks shared by the mismatch bindings (before anything is uploaded): shapes and
    coefficients.  Returns (m, n, coefs, b)."""
    m, n = A.shape
    if tuple(B0.shape) != (n, m):
        raise ValueError(f"dimension mismatch: A is {tuple(A.shape)}, B0 is {tuple(B0.shape)} (expected size(A'))")
    if tuple(E.shape) != (n, m):
        raise ValueError(f"E has shape {tuple(E.shape)}, expected B0's ({n}, {m})")
    cf = _coefs(coefs, 1, 64, what)
    return m, n, cf, _f64(b, m, "b")


def _mismatch_ops(A, B0, E, ctx):
    ctx, Ao, Bo = _ops(A, B0, ctx)
    if isinstance(E, GaussianPerturbation):
        return ctx, Ao, Bo, E
    return ctx, Ao, Bo, as_operator(E, ctx, Ao.dtype)


def gmres_bounds_mismatch(A, B0, E, coefs, b, x_true, tol, maxit, side, *, lambdas=None, ctx=None, orth="mgs",
                          return_H=False):
    """``len(coefs)`` lockstep solves of one ``*_bounds`` solver of ONE ``b`` against back-projectors that
    differ in a scalar (``hgm_gmres_bounds_mismatch``): column j of the returned :class:`BatchResult` is what
    ``{AB,BA}gmres_{hybrid,nonhybrid}_bounds`` returns with ``B = B0 + coefs[j] * E`` and ``lambdas[j]`` -- the
    loop over the mismatch levels of ``plot_error_vs_mismatch_norm.m:23-61``.  No ``B0 + c * E`` is formed or
    uploaded: ``B0`` and ``E`` (``B0``'s shape; its sparsity pattern, or one of its own) are read once per
    group of up to 8 running levels and iteration.  ``side`` is 'ab' or 'ba'; ``lambdas=None`` selects the
    non-hybrid solver; ``x_true`` may be None (the error histories stay NaN).  At most 64 levels per call.
    Per-column stopping and breakdown as :func:`gmres_bounds_batch`.

    ``E`` may be a :class:`GaussianPerturbation` (``hgm_gmres_bounds_mismatch_gauss``): the dense Gaussian
    ``E = randn(size(A'))`` of the reference, regenerated inside every B pass and never stored."""
    sd = _side(side)
    m, n, cf, b = _mismatch_args(A, B0, E, coefs, b, "gmres_bounds_mismatch")
    gauss = isinstance(E, GaussianPerturbation)
    if gauss:
        cf = _scaled_coefs(cf, E.scale, "gmres_bounds_mismatch")
    nc = cf.size
    maxit = int(maxit)
    if maxit < 1:
        raise ValueError("maxit must be >= 1")
    lam = _col_lambdas(lambdas, nc, "coefficient")
    xt = _f64(x_true, n, "x_true") if x_true is not None else None
    ctx, Ao, Bo, Eo = _mismatch_ops(A, B0, E, ctx)
    fn = L.load().hgm_gmres_bounds_mismatch_gauss if gauss else L.load().hgm_gmres_bounds_mismatch
    return _bounds_lockstep(ctx, n, maxit, nc, orth, return_H, lambda o, *out: fn(
        ctx.handle, o, Ao._h, Bo._h, Eo._h, _dp(cf), nc, _dp(b), _dp(xt), float(tol), maxit, _dp(lam), sd,
        0 if lam is None else 1, *out))


def arnoldi_mismatch(A, B0, E, coefs, b, k, gcv_type="ba", *, ctx=None, breakdown_tol=1e-12, orth="mgs"):
    """:func:`arnoldi` with the back-projector ``B0 + coefs[j] * E`` for every j in lockstep
    (``hgm_arnoldi_mismatch``; the GCV Arnoldis of ``plot_error_vs_mismatch_norm.m:46-50``): returns
    (H, beta, kdone) with ``H`` of shape ``ncoef x (k+1) x k`` and ``beta``, ``kdone`` of length ``ncoef``.
    ``E`` may be a :class:`GaussianPerturbation` (``hgm_arnoldi_mismatch_gauss``)."""
    sd = _side(gcv_type)
    m, n, cf, b = _mismatch_args(A, B0, E, coefs, b, "arnoldi_mismatch")
    gauss = isinstance(E, GaussianPerturbation)
    if gauss:
        cf = _scaled_coefs(cf, E.scale, "arnoldi_mismatch")
    nc = cf.size
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    ctx, Ao, Bo, Eo = _mismatch_ops(A, B0, E, ctx)
    H = np.zeros((k + 1) * k * nc)
    beta = np.zeros(nc)
    kd = np.zeros(nc, dtype=np.int32)
    o = L.HGM_CGS2 if str(orth).lower() == "cgs2" else L.HGM_MGS
    fn = L.load().hgm_arnoldi_mismatch_gauss if gauss else L.load().hgm_arnoldi_mismatch
    _check(fn(ctx.handle, Ao._h, Bo._h, Eo._h, _dp(cf), nc, _dp(b), k, sd, float(breakdown_tol), o, _dp(H), _dp(beta),
              kd.ctypes.data_as(C.POINTER(C.c_int))), ctx)
    return _H_blocks(H, nc, k), beta, kd.astype(int)


def proj_norms(V, Y, t=None, *, ctx=None, loop=False):
    """``(d, s)`` with ``d[l] = ||V @ Y[:, l] - t||^2`` and ``s[l] = ||V @ Y[:, l]||^2`` from the device
    primitive ``hgm_proj_norms`` (one pass over V, the product never stored).  ``V`` is used as given when
    it is Fortran-ordered, so a column-major view with a leading dimension larger than its row count
    (``buf[:rows, :]`` of an ``ld x k`` array) is passed with that leading dimension.
    ``loop``: the yardstick ``hgm_proj_norms_loop`` instead (the solvers' single-coefficient monitor, one
    launch per column; ``t`` required, even leading dimension); returns ``(d, None)``."""
    V = np.asarray(V, dtype=np.float64)
    Y = np.asfortranarray(np.asarray(Y, dtype=np.float64))
    if V.ndim != 2 or Y.ndim != 2 or Y.shape[0] != V.shape[1]:
        raise ValueError("proj_norms: V is rows x k and Y is k x L")
    rows, k = V.shape
    nl = Y.shape[1]
    if rows < 1 or k < 1 or nl < 1:
        raise ValueError("proj_norms: rows, k and L must be >= 1")
    ctx = ctx or default_context()
    lib = L.load()
    vflat, ldv = _ld_view(V)
    tt = _f64(t, rows, "t") if t is not None else None
    d, s = np.zeros(nl), np.zeros(nl)
    with _DevArrays(ctx) as dev:
        vd, yd = dev.upload(vflat), dev.upload(Y.reshape(-1, order="F"))
        td = dev.upload(tt) if tt is not None else None
        if loop:
            _check(lib.hgm_proj_norms_loop(ctx.handle, rows, k, vd, ldv, yd, k, nl, td, _dp(d)), ctx)
            s = None
        else:
            _check(lib.hgm_proj_norms(ctx.handle, rows, k, vd, ldv, yd, k, nl, td, _dp(d), _dp(s)), ctx)
    return d, s


def _gkb_ops(A, ctx, At=None, dtype=L.HGM_F64):
    ctx = ctx or (A.ctx if isinstance(A, SparseOperator) else default_context())
    Ao = as_operator(A, ctx, dtype)
    Ato = as_operator(At, ctx, Ao.dtype) if At is not None else Ao.T
    return ctx, Ao, Ato


def _gkb_solve(fn_name, A, b, x_true, tol, maxit, ctx, At, lambda_=None):
    """The one body of lsqr_solver (``lambda_`` None: the ``_ex`` signature with options) and the two hybrid
    solvers (lambda after maxit)."""
    ctx, Ao, Ato = _gkb_ops(A, ctx, At)
    m, n = Ao.shape
    maxit = int(maxit)
    b = _f64(b, m, "b")
    xt = _f64(x_true, n, "x_true")
    x, err, res, it = np.zeros(n), np.zeros(maxit), np.zeros(maxit), C.c_int(0)
    o = _opts()
    head, lam = ((C.byref(o),), ()) if lambda_ is None else ((), (float(lambda_),))
    _check(getattr(L.load(), fn_name)(ctx.handle, *head, Ao._h, Ato._h, _dp(b), _dp(xt), float(tol), maxit, *lam,
                                      _dp(x), _dp(err), _dp(res), C.byref(it)), ctx)
    k = it.value
    return x, err[:k].copy(), res[:k].copy(), k


def lsqr_solver(A, b, x_true, tol, maxit, *, ctx=None, At=None):
    """``[x, error_norm, residual_norm, niters] = lsqr_solver(A,b,x_true,tol,maxit)`` (lsqr_solver.m:1-54)."""
    return _gkb_solve("hgm_lsqr_solver_ex", A, b, x_true, tol, maxit, ctx, At)


def lsmr_solver(A, b, x_true=None, tol=None, maxit=None, *, ctx=None, At=None, explicit_residual=False):
    """``[x, err_hist, res_hist, ar_hist, iters] = lsmr_solver(A,b,x_true,tol,maxit)``
    (lsmr_solver.m:1-83; ``tol`` defaults to 1e-6, ``maxit`` to ``min(m,n)``).  The monitors
    ``b - A*x`` and ``A'*r`` come from kept products unless ``explicit_residual``."""
    ctx, Ao, Ato = _gkb_ops(A, ctx, At)
    m, n = Ao.shape
    tol = 1e-6 if tol is None else float(tol)
    maxit = min(m, n) if maxit is None else int(maxit)
    b = _f64(b, m, "b")
    xt = None if x_true is None or np.size(x_true) == 0 else _f64(x_true, n, "x_true")
    x = np.zeros(n)
    eh, rh, ah, it = np.zeros(maxit), np.zeros(maxit), np.zeros(maxit), C.c_int(0)
    o = _opts(explicit_residual=explicit_residual)
    _check(L.load().hgm_lsmr_solver_ex(ctx.handle, C.byref(o), Ao._h, Ato._h, _dp(b), _dp(xt), tol, maxit,
                                       _dp(x), _dp(eh), _dp(rh), _dp(ah), C.byref(it)), ctx)
    k = it.value
    return x, eh[:k].copy(), rh[:k].copy(), ah[:k].copy(), k


def hybrid_lsqr_solver(A, b, x_true, tol, maxit, lambda_, *, ctx=None, At=None):
    """``hybrid_lsqr_solver.m:1-52`` (LSQR on ``[A; sqrt(lambda) I]``, augmentation implicit)."""
    return _gkb_solve("hgm_hybrid_lsqr_solver", A, b, x_true, tol, maxit, ctx, At, lambda_)


def hybrid_lsmr_solver(A, b, x_true, tol, maxit, lambda_, *, ctx=None, At=None):
    """``hybrid_lsmr_solver.m:1-57``."""
    return _gkb_solve("hgm_hybrid_lsmr_solver", A, b, x_true, tol, maxit, ctx, At, lambda_)


class GKBatchResult:
    """Outputs of :func:`gk_batch`.  ``x``: ``n x nrhs``; ``error_norm``, ``residual_norm``, ``ar_norm``:
    ``maxit x nrhs`` (row k-1 = iteration k; NaN past ``niters[j]``; ``ar_norm`` is all NaN except for
    ``kind='lsmr'``); ``niters``: per column."""

    def __init__(self, x, error_norm, residual_norm, ar_norm, niters):
        self.x, self.error_norm, self.residual_norm, self.ar_norm = x, error_norm, residual_norm, ar_norm
        self.niters = niters


GK_KINDS = {"lsqr": (L.HGM_GK_LSQR, 0), "lsmr": (L.HGM_GK_LSMR, 0), "hybrid_lsqr": (L.HGM_GK_LSQR, 1),
            "hybrid_lsmr": (L.HGM_GK_LSMR, 1)}


def gk_batch(A, Bm, x_true, tol, maxit, kind, *, lambdas=None, At=None, ctx=None):
    """``nrhs`` lockstep solves of one Golub-Kahan solver against one operator (``hgm_gk_batch``): column j of
    every output is what ``lsqr_solver`` / ``lsmr_solver`` / ``hybrid_lsqr_solver`` / ``hybrid_lsmr_solver``
    (``kind`` 'lsqr', 'lsmr', 'hybrid_lsqr', 'hybrid_lsmr') returns for ``b = Bm[:, j]``, ``x_true[:, j]`` and
    ``lambdas[j]`` (the hybrid kinds need ``lambdas``).  A 1-D ``Bm`` with several lambdas is one ``b`` shared by
    every column: a hybrid solver's lambda sweep.  ``x_true`` is ``n x nrhs``, one vector shared by every column,
    or None (the error histories stay NaN).  ``At`` defaults to the device transpose of ``A``.  The operators'
    entries are read once per group of up to 8 running columns and pass; a finished column leaves the batch."""
    if str(kind).lower() not in GK_KINDS:
        raise ValueError(f"kind must be one of {sorted(GK_KINDS)}, not {kind!r}")
    kd, hybrid = GK_KINDS[str(kind).lower()]
    m, n = A.shape
    maxit = int(maxit)
    lam = _col_lambdas(lambdas, None, "column")
    if hybrid and lam is None:
        raise ValueError(f"kind {kind!r} needs lambdas (one per column)")
    Bm = np.asarray(Bm, dtype=np.float64)
    shared_b = Bm.ndim == 1 and lam is not None and lam.size > 1
    if shared_b:
        if Bm.shape[0] != m:
            raise ValueError(f"b has length {Bm.shape[0]}, expected {m}")
        nrhs = lam.size
    else:
        if Bm.ndim == 1:
            Bm = Bm.reshape(-1, 1)
        if Bm.ndim != 2 or Bm.shape[0] != m or Bm.shape[1] < 1:
            raise ValueError(f"Bm has shape {Bm.shape}, expected ({m}, nrhs)")
        nrhs = Bm.shape[1]
    if nrhs > 64:
        raise ValueError(f"at most 64 columns per call, not {nrhs}")
    lam = _col_lambdas(lam, nrhs, "column")
    if hybrid and not (np.all(np.isfinite(lam)) and np.all(lam >= 0)):
        raise ValueError("every lambda must be finite and >= 0")
    xt, ldxt = _col_x_true(x_true, n, nrhs)
    if maxit < 1:
        raise ValueError("maxit must be >= 1")
    if At is not None and tuple(At.shape) != (n, m):
        raise ValueError(f"At has shape {tuple(At.shape)}, expected ({n}, {m})")
    ctx, Ao, Ato = _gkb_ops(A, ctx, At)
    Bf = np.ascontiguousarray(Bm) if shared_b else np.asfortranarray(Bm)
    X, (err, res, ar), nit = _batch_outputs(n, maxit, nrhs, 3)
    o = _opts()
    _check(L.load().hgm_gk_batch(ctx.handle, C.byref(o), Ao._h, Ato._h, _dp(Bf), 0 if shared_b else max(m, 1), nrhs,
                                 _dp(xt), ldxt, float(tol), maxit, _dp(lam), kd, hybrid, _dp(X), max(n, 1), _dp(err),
                                 _dp(res), _dp(ar), nit.ctypes.data_as(C.POINTER(C.c_int))), ctx)
    return GKBatchResult(X, err, res, ar, nit.astype(int))


def mv_axpby_norms(a, X, b, Y, ctx=None):
    """``Out[:, r] = (a[r] * X[:, r]) + (b[r] * Y[:, r])`` for ``n x nvec`` host arrays (``1 <= nvec <= 8``) and
    ``sumsq[r] = sum_i Out[i, r]**2`` through ``hgm_mv_axpby_norms``, the interleaved vector kernel of
    :func:`gk_batch` (gkmv.hip): products and sum rounded separately, a fixed summation order, and a column's bits
    independent of ``nvec``, its position and the other columns.  Returns ``(Out, sumsq)``."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)
    if X.ndim != 2 or Y.shape != X.shape:
        raise ValueError(f"X and Y have shapes {X.shape} and {Y.shape}, expected the same (n, nvec)")
    n, nv = X.shape
    if not 1 <= nv <= 8:
        raise ValueError(f"mv_axpby_norms takes 1 to 8 vectors, not {nv}")
    af = _coefs_any(a, nv, "a")
    bf = _coefs_any(b, nv, "b")
    ctx = ctx or default_context()
    ss = np.zeros(nv)
    ld = max(n, 1)
    with _DevArrays(ctx) as dev:
        xd, yd = (dev.upload(np.asfortranarray(M).reshape(-1, order="F")) for M in (X, Y))
        od = dev.alloc(ld * nv)
        _check(dev.lib.hgm_mv_axpby_norms(ctx.handle, n, nv, _dp(af), xd, ld, _dp(bf), yd, ld, od, ld, _dp(ss)), ctx)
        Out = dev.download(od, np.empty((n, nv), order="F"))
    return Out, ss


def _coefs_any(v, nv, name):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if a.size != nv:
        raise ValueError(f"{name} has {a.size} entries, expected one per vector ({nv})")
    return a


def arnoldi(A, B, b, k, gcv_type="ba", *, ctx=None, breakdown_tol=1e-12, orth="mgs"):
    """Arnoldi part of ``gcv_function.m:3-33``: returns (H, beta, kdone)."""
    ctx, Ao, Bo = _ops(A, B, ctx)
    side = L.HGM_SIDE_AB if gcv_type == "ab" else L.HGM_SIDE_BA
    b = _f64(b, Ao.shape[0], "b")
    H = np.zeros((k + 1) * k)
    beta, kd = C.c_double(), C.c_int()
    o = L.HGM_CGS2 if orth == "cgs2" else L.HGM_MGS
    _check(L.load().hgm_arnoldi(ctx.handle, Ao._h, Bo._h, _dp(b), int(k), side, float(breakdown_tol), o,
                                _dp(H), C.byref(beta), C.byref(kd)), ctx)
    return H.reshape(k, k + 1).T.copy(), beta.value, kd.value


def gcv_from_H(H, beta, lambda_, trace_m):
    """λ-dependent part of ``gcv_function.m:35-58`` on a cached H ((k+1) x k)."""
    H = np.asarray(H, dtype=np.float64)
    k = H.shape[1]
    Hf = np.ascontiguousarray(H.T).reshape(-1)
    g = C.c_double()
    rc = L.load().hgm_gcv_from_H(_dp(Hf), k, float(beta), float(lambda_), float(trace_m), C.byref(g))
    if rc != L.HGM_OK:
        raise ValueError("hgm_gcv_from_H: invalid arguments")
    return g.value


def gcv_function(lambda_, A, B, b, m, k_gcv, gcv_type, *, ctx=None):
    """``gcv_val = gcv_function(lambda,A,B,b,m,k_gcv,gcv_type)`` (gcv_function.m:1-59)."""
    ctx, Ao, Bo = _ops(A, B, ctx)
    side = L.HGM_SIDE_AB if gcv_type == "ab" else L.HGM_SIDE_BA
    b = _f64(b, Ao.shape[0], "b")
    g = C.c_double()
    _check(L.load().hgm_gcv_function(ctx.handle, float(lambda_), Ao._h, Bo._h, _dp(b), int(m), int(k_gcv), side,
                                     C.byref(g)), ctx)
    return g.value


def gcv_fminbnd(H, beta, trace_m, lo=1e-9, hi=1e-1, tolx=1e-8):
    """``fminbnd(@(l) gcv_function(l,...), lo, hi, optimset('TolX',tolx))`` on ONE cached
    Arnoldi (analyze_regularization.m:37-46): returns (lambda_opt, gcv_opt)."""
    H = np.asarray(H, dtype=np.float64)
    k = H.shape[1]
    Hf = np.ascontiguousarray(H.T).reshape(-1)
    lo_, g = C.c_double(), C.c_double()
    rc = L.load().hgm_gcv_fminbnd(_dp(Hf), k, float(beta), float(trace_m), float(lo), float(hi), float(tolx),
                                  C.byref(lo_), C.byref(g))
    if rc != L.HGM_OK:
        raise ValueError("hgm_gcv_fminbnd: invalid arguments")
    return lo_.value, g.value


# ---------------------------------------------------------------------------
# Host-only spectral helpers of the filter-factor bounds (spectral.cpp)
# ---------------------------------------------------------------------------
def eig(M):
    """MATLAB ``[V, D] = eig(M)`` of a real square matrix (host): (w, V), complex, unit 2-norm columns."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    Mf = np.ascontiguousarray(M.T).reshape(-1)
    wr, wi, V = np.zeros(n), np.zeros(n), np.zeros(n * n)
    if L.load().hgm_eig(n, _dp(Mf), _dp(wr), _dp(wi), _dp(V)) != L.HGM_OK:
        raise HgmError("hgm_eig: QR iteration did not converge")
    V = V.reshape(n, n).T
    W = V.astype(np.complex128)
    j = 0
    while j < n:
        if wi[j] > 0 and j + 1 < n:
            W[:, j] = V[:, j] + 1j * V[:, j + 1]
            W[:, j + 1] = V[:, j] - 1j * V[:, j + 1]
            j += 2
        else:
            j += 1
    return wr + 1j * wi, W


def filter_factors(H, k, dK, mu, dmu, lambda_, side, hybrid):
    """phi / dphi of iteration k of the ``*_bounds.m`` files (``:42-78``) from H ((k+1) x k
    leading part), dK = Qk' DeltaM Qk, the k leading eigenvalues mu of M and dmu."""
    H = np.asarray(H, dtype=np.float64)
    Hf = np.ascontiguousarray(H.T).reshape(-1)
    dK = np.asarray(dK, dtype=np.float64)
    dKf = np.ascontiguousarray(dK.T).reshape(-1)
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    dmu = np.ascontiguousarray(dmu, dtype=np.float64)
    phi, dphi = np.zeros(k), np.zeros(k)
    sd = L.HGM_SIDE_AB if side == "ab" else L.HGM_SIDE_BA
    rc = L.load().hgm_filter_factors(_dp(Hf), H.shape[0], int(k), _dp(dKf), dK.shape[0], _dp(mu), _dp(dmu),
                                     float(lambda_), sd, int(bool(hybrid)), _dp(phi), _dp(dphi))
    if rc != L.HGM_OK:
        raise ValueError("hgm_filter_factors: invalid arguments")
    return phi, dphi


def ritz(Hp, h_next, G, nev):
    """Leading Ritz pairs of a p-step Arnoldi: (mu, dmu, resid) (descending real part)."""
    Hp = np.asarray(Hp, dtype=np.float64)
    p = Hp.shape[1]
    Hf = np.ascontiguousarray(Hp.T).reshape(-1)
    G = np.asarray(G, dtype=np.float64)
    Gf = np.ascontiguousarray(G.T).reshape(-1)
    mu, dmu, rr = np.zeros(nev), np.zeros(nev), np.zeros(nev)
    rc = L.load().hgm_ritz(_dp(Hf), Hp.shape[0], p, float(h_next), _dp(Gf), G.shape[0], int(nev), _dp(mu),
                           _dp(dmu), _dp(rr))
    if rc != L.HGM_OK:
        raise ValueError("hgm_ritz: invalid arguments")
    return mu, dmu, rr


# ---- leading singular triplets and empirical filter factors (plot_filter_factors.m:30-40) ----
def basis_project(Q, X, *, loop=False, ctx=None):
    """``C = Q.T @ X`` (k x nx) from the device primitive ``hgm_basis_project``: one pass over the basis
    ``Q`` (rows x k, k <= 256) per group of up to 8 columns of ``X`` (rows x nx).  Column-major views with
    a larger leading dimension are passed with it (their padding is uploaded and never read).
    ``loop``: the yardstick ``hgm_basis_project_loop`` instead (the solvers' one-vector projection, one pass
    over ``Q`` per column of ``X``)."""
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    if Q.ndim != 2 or X.ndim != 2 or X.shape[0] != Q.shape[0]:
        raise ValueError("basis_project: Q is rows x k and X is rows x nx")
    rows, k = Q.shape
    nx = X.shape[1]
    if rows < 1 or k < 1 or nx < 1:
        raise ValueError("basis_project: rows, k and nx must be >= 1")
    ctx = ctx or default_context()
    qf, ldq = _ld_view(Q)
    xf, ldx = _ld_view(X)
    Cm = np.zeros(k * nx)
    with _DevArrays(ctx) as d:
        qp, xp = d.upload(qf), d.upload(xf)
        fn = d.lib.hgm_basis_project_loop if loop else d.lib.hgm_basis_project
        _check(fn(ctx.handle, rows, k, qp, ldq, nx, xp, ldx, _dp(Cm)), ctx)
    return Cm.reshape(nx, k).T.copy()


def basis_rotate(Q, Y, *, ldw=None, return_sumsq=False, loop=False, ctx=None):
    """``W = Q @ Y`` (rows x p, p <= 64) from the device primitive ``hgm_basis_rotate``: one pass over the
    basis ``Q`` (rows x k, k <= 256).  ``ldw``: the leading dimension of the device result (>= rows; its
    padding is pre-filled with NaN and must come back untouched -- the padded array is returned).
    ``return_sumsq``: also ``sum_i W[i, l]**2`` as summed on the device.
    ``loop``: the yardstick ``hgm_basis_rotate_loop`` instead (the solvers' ``x = Q y``, one pass over ``Q`` per
    column of ``Y``; even leading dimensions, no sums)."""
    Q = np.asarray(Q, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Q.ndim != 2 or Y.ndim != 2 or Y.shape[0] != Q.shape[1]:
        raise ValueError("basis_rotate: Q is rows x k and Y is k x p")
    rows, k = Q.shape
    p = Y.shape[1]
    if rows < 1 or k < 1 or p < 1:
        raise ValueError("basis_rotate: rows, k and p must be >= 1")
    ldw = rows if ldw is None else int(ldw)
    if ldw < rows:
        raise ValueError("basis_rotate: ldw < rows")
    ctx = ctx or default_context()
    qf, ldq = _ld_view(Q)
    yf, ldy = _ld_view(Y)
    W = np.full(ldw * p, np.nan)
    ss = np.zeros(p)
    with _DevArrays(ctx) as d:
        qp, yp, wp = d.upload(qf), d.upload(yf), d.upload(W)
        if loop:
            if return_sumsq:
                raise ValueError("basis_rotate: the loop form returns no sums")
            _check(d.lib.hgm_basis_rotate_loop(ctx.handle, rows, k, qp, ldq, p, yp, ldy, wp, ldw), ctx)
        else:
            _check(d.lib.hgm_basis_rotate(ctx.handle, rows, k, qp, ldq, p, yp, ldy, wp, ldw,
                                          _dp(ss) if return_sumsq else None), ctx)
        _check(d.lib.hgm_memcpy_d2h(ctx.handle, W.ctypes.data_as(C.c_void_p), wp, 8 * W.size), ctx)
    Wm = W.reshape(p, ldw).T
    Wm = Wm if ldw != rows else Wm.copy()
    return (Wm, ss) if return_sumsq else Wm


def bidiag_svd(alpha, beta):
    """``(sigma, P, Q)`` with ``B = P @ diag(sigma) @ Q.T`` for the lower bidiagonal ``B`` ((k+1) x k, diagonal
    ``alpha``, subdiagonal ``beta``): the host one-sided Jacobi of ``hgm_bidiag_svd``."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    k = alpha.size
    if k < 1 or beta.size != k:
        raise ValueError("bidiag_svd: alpha and beta have the same length k >= 1")
    s, Pm, Qm = np.zeros(k), np.zeros((k + 1) * k), np.zeros(k * k)
    rc = L.load().hgm_bidiag_svd(k, _dp(alpha), _dp(beta), _dp(s), _dp(Pm), _dp(Qm))
    if rc != L.HGM_OK:
        raise ValueError("hgm_bidiag_svd: invalid arguments")
    return s, Pm.reshape(k, k + 1).T.copy(), Qm.reshape(k, k).T.copy()


class SvdsResult:
    """Leading singular triplets from ``svds``: ``sigma``, ``resid`` (= ||A'u - sigma v||), ``utb`` (= u'b >= 0),
    ``VtX`` (nsv x nx, or None), ``U`` / ``V`` (or None), ``steps_done``.  Entries past
    ``min(nsv, steps_done)`` are NaN."""
    __slots__ = ("sigma", "resid", "utb", "VtX", "U", "V", "steps_done")

    def __init__(self, sigma, resid, utb, VtX, U, V, steps_done):
        self.sigma, self.resid, self.utb, self.VtX, self.U, self.V = sigma, resid, utb, VtX, U, V
        self.steps_done = steps_done

    def nconv(self, tol=1e-10):
        """The leading run of triplets with ``resid <= tol * sigma[0]``."""
        n = 0
        for r in self.resid:
            if not (r <= tol * self.sigma[0]):
                break
            n += 1
        return n


def svds(A, b, steps, nsv, *, At=None, X=None, return_vectors=False, breakdown_tol=0, ctx=None):
    """Leading singular triplets of ``A`` by Golub-Kahan-Lanczos bidiagonalisation started at ``b`` with full
    reorthogonalisation (``hgm_svds``; the ``svd(A,'econ')`` of plot_filter_factors.m:30 restricted to the
    modes ``b`` excites).  ``b=None``: a fixed deterministic start vector.  ``X`` (n x nx, nx <= 64): also
    ``VtX = V.T @ X``.  Returns an ``SvdsResult``."""
    ctx, Ao, Ato = _gkb_ops(A, ctx, At, dtype=A.dtype if isinstance(A, SparseOperator) else L.HGM_F64)
    m, n = Ao.shape
    steps, nsv = int(steps), int(nsv)
    bb = _f64(b, m, "b") if b is not None else None
    Xf, nx = None, 0
    if X is not None:
        Xf = np.asarray(X, dtype=np.float64)
        if Xf.ndim == 1:
            Xf = Xf.reshape(-1, 1)
        if Xf.shape[0] != n:
            raise ValueError(f"X must have {n} rows")
        nx = Xf.shape[1]
        Xf = np.asfortranarray(Xf)
    ns = max(nsv, 1)
    sigma, resid, utb = np.zeros(ns), np.zeros(ns), np.zeros(ns)
    VtX = np.zeros((ns, nx), order="F") if Xf is not None else None
    U = np.zeros((m, ns), order="F") if return_vectors else None
    V = np.zeros((n, ns), order="F") if return_vectors else None
    done = C.c_int(0)
    _check(L.load().hgm_svds(ctx.handle, Ao._h, Ato._h, _dp(bb) if bb is not None else None, steps, nsv,
                             float(breakdown_tol), _dp(Xf) if Xf is not None else None, n, nx, _dp(sigma), _dp(resid),
                             _dp(utb), _dp(VtX) if VtX is not None else None, _dp(U) if U is not None else None, m,
                             _dp(V) if V is not None else None, n, C.byref(done)), ctx)
    return SvdsResult(sigma, resid, utb, VtX, U, V, done.value)


class EmpiricalFilterResult:
    """``sigma``, ``Phi`` (nsv x nx), ``resid``, ``nconv`` of ``empirical_filter_factors`` (and the ``svds``
    result they came from as ``svds``)."""
    __slots__ = ("sigma", "Phi", "resid", "nconv", "svds")

    def __init__(self, sigma, Phi, resid, nconv, svds_result):
        self.sigma, self.Phi, self.resid, self.nconv, self.svds = sigma, Phi, resid, nconv, svds_result

    def __iter__(self):
        return iter((self.sigma, self.Phi, self.resid, self.nconv))


def empirical_filter_factors(A, b, X, steps, nsv, *, At=None, breakdown_tol=0, tol=1e-10, ctx=None):
    """Empirical filter factors ``Phi[i, r] = sigma_i (v_i' x_r) / (u_i' b)`` of the solutions ``X`` (n x nx) on the
    leading singular triplets from ``svds`` (plot_filter_factors.m:31-40), with the reference's guard
    ``d(abs(d) < 1e-12) = 1`` on the denominators (:35).  ``nconv``: the leading run with
    ``resid <= tol * sigma[0]``."""
    r = svds(A, b, steps, nsv, At=At, X=X, breakdown_tol=breakdown_tol, ctx=ctx)
    d = r.utb.copy()
    d[np.abs(d) < 1e-12] = 1.0                                    # :35
    Phi = r.sigma[:, None] * r.VtX / d[:, None]                   # :31-36
    return EmpiricalFilterResult(r.sigma, Phi, r.resid, r.nconv(tol), r)
