"""Measurements of the block kernels on a basis.  Run on an MI355X:
    python scripts/basis_micro.py [rows] [reps]
One JSON line per kernel.

rows = 2048^2 (C3's pixel count) by default, k = 60 basis vectors: basis_project with nx = 4 columns of X
against the loop of nx multidot launches (hgm_basis_project_loop), basis_rotate with p = 20 columns of Y
against the loop of p gemv launches (hgm_basis_rotate_loop), on the same buffers -- the loops are the
solvers' own one-vector kernels, the code before the block kernels.  Host clock around a call that ends in
a device synchronise (both hooks synchronise before they return), routes alternating, median of `reps`
(5) warmed calls; GB/s on the bytes a single pass needs, 8 rows (k + nx) / 8 rows (k + p), for both routes.
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
import torch  # noqa: E402,F401
import hgmres  # noqa: E402
from hgmres import _lib as L  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 2048 * 2048
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
k, nx, p = 60, 4, 20
ctx = hgmres.Context(0)
lib = L.load()
dev = torch.device("cuda", 0)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
g = torch.Generator(device=dev).manual_seed(0)
ld = rows + 64
Q = torch.randn(ld * k, dtype=torch.float64, device=dev, generator=g)
X = torch.randn(ld * nx, dtype=torch.float64, device=dev, generator=g)
Y = torch.randn(k * p, dtype=torch.float64, device=dev, generator=g)
W = [torch.zeros(ld * p, dtype=torch.float64, device=dev) for _ in range(2)]
Cb, Cl = np.zeros(k * nx), np.zeros(k * nx)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert fn() == 0
    return (time.perf_counter() - t0) * 1e3


def compare(name, block, loop, nbytes, check):
    block(), loop()                                   # warm both routes
    tb, tl = [], []
    for _ in range(reps):                             # alternating
        tb.append(wall(block))
        tl.append(wall(loop))
    mb, ml = statistics.median(tb), statistics.median(tl)
    print(json.dumps({"kernel": name, "rows": rows, "k": k, "nx": nx, "p": p, "reps": reps,
                      "block_ms": round(mb, 4), "loop_ms": round(ml, 4), "speedup": round(ml / mb, 3),
                      "block_GBps": round(nbytes / mb / 1e6, 1), "loop_GBps_same_bytes": round(nbytes / ml / 1e6, 1),
                      "block_ms_all": [round(v, 4) for v in tb], "loop_ms_all": [round(v, 4) for v in tl],
                      "max_rel_diff": check()}), flush=True)


compare("basis_project",
        lambda: lib.hgm_basis_project(ctx.handle, rows, k, P(Q), ld, nx, P(X), ld, Cb.ctypes.data_as(L.dp)),
        lambda: lib.hgm_basis_project_loop(ctx.handle, rows, k, P(Q), ld, nx, P(X), ld, Cl.ctypes.data_as(L.dp)),
        8.0 * rows * (k + nx), lambda: float(np.max(np.abs(Cb - Cl)) / np.max(np.abs(Cl))))
compare("basis_rotate",
        lambda: lib.hgm_basis_rotate(ctx.handle, rows, k, P(Q), ld, p, P(Y), k, P(W[0]), ld, None),
        lambda: lib.hgm_basis_rotate_loop(ctx.handle, rows, k, P(Q), ld, p, P(Y), k, P(W[1]), ld),
        8.0 * rows * (k + p), lambda: float((W[0] - W[1]).abs().max() / W[1].abs().max()))
ctx.close()
