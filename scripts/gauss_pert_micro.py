"""Measurements of the matrix-free Gaussian product.  Run on an MI355X:
    python scripts/gauss_pert_micro.py c2 [reps]      hgm_gauss_mm and hgm_spmm_pert_gauss at the c2 B shape
    python scripts/gauss_pert_micro.py small [reps]   hgm_gauss_mm against hgm_spmm on the explicit dense CSR
One JSON line per point.

c2: B0 = A' of the bench's c2 (512^2, 30 angles) tiled Siddon projector, 262,144 x 21,750, and G of its shape;
nvec 1, 4, 8.  hgm_gauss_mm (G X alone) and hgm_spmm_pert_gauss (B0 X + c G X), each warmed; host clock around
`inner` back-to-back calls that end in a device synchronise, per call, median of `reps`; and the device time of
one call's launches (kernel-timing class 5: pack, product(s), unpack and the pixel-order permutes).  Rates: Philox
calls (rows x ceil(cols / 4)) and generated entries per second over the device time.

small: the 64^2 / 90-angle B shape (4,096 rows): hgm_gauss_mm against hgm_spmm on the dense CSR of the same
entries (G.entries(), uploaded: 12 B per entry), nvec 1, 4, 8, alternating; the largest deviation between the two
over the largest value is printed with them.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hybrid-gmres_amd"), ROOT]
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402
import hgmres  # noqa: E402
from hgmres import _lib as L  # noqa: E402

KC_SPMM = 5
mode = sys.argv[1] if len(sys.argv) > 1 else "c2"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ctx = hgmres.Context(0)
lib = L.load()
dev = torch.device("cuda", 0)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def ok(rc):
    assert rc == 0, f"libhgmres status {rc}"


def clock(fn, inner):
    torch.cuda.synchronize()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def device_ms(fn):
    ctx.kernel_timing(True)
    fn()
    ms = ctx.kernel_timing_read(KC_SPMM)[0]
    ctx.kernel_timing(False)
    return ms


def c2():
    A = hgmres.SparseOperator.siddon(512, 30, ctx=ctx)
    B0 = A.T
    rows, cols = B0.shape
    G = hgmres.GaussianPerturbation(rows, cols, 21, ctx=ctx)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(cols * 8, dtype=torch.float64, device=dev, generator=g)
    Y = torch.zeros(rows * 8, dtype=torch.float64, device=dev)
    inner = 3
    for nv in (1, 4, 8):
        cf = np.ascontiguousarray(np.logspace(-3, 0, nv))
        routes = {
            "gauss_mm": lambda: ok(lib.hgm_gauss_mm(ctx.handle, G._h, nv, None, P(X), cols, P(Y), rows)),
            "spmm_pert_gauss": lambda: ok(lib.hgm_spmm_pert_gauss(ctx.handle, B0._h, G._h, nv, cf.ctypes.data_as(L.dp),
                                                                  P(X), cols, P(Y), rows)),
            "spmm_B0": lambda: ok(lib.hgm_spmm(ctx.handle, B0._h, nv, P(X), cols, P(Y), rows)),
        }
        for fn in routes.values():
            clock(fn, 1)
        t = {k: [] for k in routes}
        d = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():
                t[k].append(clock(fn, inner))
                d[k].append(device_ms(fn))
        out = dict(what="matrix-free Gaussian product", workload="c2 B shape", rows=rows, cols=cols, nvec=nv, reps=reps,
                   inner=inner, nnz_B0=B0.nnz)
        for k in routes:
            out[f"{k}_ms"] = round(statistics.median(t[k]), 3)
            out[f"{k}_ms_min"] = round(min(t[k]), 3)
            out[f"{k}_ms_max"] = round(max(t[k]), 3)
            out[f"{k}_device_ms"] = round(statistics.median(d[k]), 3)
        dm = out["gauss_mm_device_ms"] * 1e-3
        out["philox_calls_per_s"] = round(rows * ((cols + 3) // 4) / dm, 0)
        out["entries_per_s"] = round(rows * cols / dm, 0)
        print(json.dumps(out), flush=True)


def small():
    A = hgmres.SparseOperator.siddon(64, 90, ctx=ctx)
    rows, cols = A.shape[1], A.shape[0]
    G = hgmres.GaussianPerturbation(rows, cols, 21, ctx=ctx)
    t0 = time.perf_counter()
    E = hgmres.SparseOperator.from_scipy(sp.csr_matrix(G.to_dense()), ctx=ctx)
    ctx.synchronize()
    upload_s = time.perf_counter() - t0
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(cols * 8, dtype=torch.float64, device=dev, generator=g)
    Y, Z = (torch.zeros(rows * 8, dtype=torch.float64, device=dev) for _ in range(2))
    inner = 10
    for nv in (1, 4, 8):
        routes = {
            "gauss_mm": lambda: ok(lib.hgm_gauss_mm(ctx.handle, G._h, nv, None, P(X), cols, P(Y), rows)),
            "spmm_dense_csr": lambda: ok(lib.hgm_spmm(ctx.handle, E._h, nv, P(X), cols, P(Z), rows)),
        }
        for fn in routes.values():
            clock(fn, 1)
        t = {k: [] for k in routes}
        d = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():
                t[k].append(clock(fn, inner))
                d[k].append(device_ms(fn))
        torch.cuda.synchronize()
        dev_ = float((Y[: rows * nv] - Z[: rows * nv]).abs().max() / Z[: rows * nv].abs().max())
        out = dict(what="matrix-free Gaussian product vs hgm_spmm on the dense CSR", rows=rows, cols=cols, nvec=nv,
                   reps=reps, inner=inner, dense_csr_bytes=12 * E.nnz, dense_csr_build_upload_s=round(upload_s, 2),
                   max_dev_over_max=dev_)
        for k in routes:
            out[f"{k}_ms"] = round(statistics.median(t[k]), 3)
            out[f"{k}_ms_min"] = round(min(t[k]), 3)
            out[f"{k}_ms_max"] = round(max(t[k]), 3)
            out[f"{k}_device_ms"] = round(statistics.median(d[k]), 3)
        out["gauss_over_csr"] = round(out["gauss_mm_ms"] / out["spmm_dense_csr_ms"], 3)
        print(json.dumps(out), flush=True)


{"c2": c2, "small": small}[mode]()
