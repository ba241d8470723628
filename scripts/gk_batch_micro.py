"""Measurements of the lockstep Golub-Kahan solves.  Run on an MI355X:
    python scripts/gk_batch_micro.py c3|c4 [reps] [kind ...]
One JSON line per point: hgm_gk_batch against the loop of the unchanged single solvers (hgm_lsqr_solver_ex,
hgm_hybrid_lsqr_solver, hgm_lsmr_solver_ex, hgm_hybrid_lsmr_solver: the route the library had before the
batch), on the same context and resident operators.

Operators: the bench's c3 (2048^2, 19 angles) and c4 (4096^2, 47 angles) tiled Siddon projectors A and their
device transposes.  All four kinds, 8 and 20 noisy right-hand sides, maxit 20, tol 0 (no column leaves early),
lambda 1e-3 for the hybrid kinds.  Host time around the calls, synchronised, the two routes alternating, median
of `reps` (>= 5) after one warm-up of each; then one timed batch for the split between the operator passes
(timing class 5) and the interleaved vector kernels (class 6); the rest is host work, transfers and, for hybrid
LSMR, the per-column x = V_k y.  Hybrid LSMR's bases take 8 * n * maxit * nrhs bytes (c4, 20 columns: 54 GB).
"""
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

GEOM = {"c3": (2048, 19), "c4": (4096, 47)}
KC_SPMM, KC_GKMV = 5, 6
SINGLE = {"lsqr": hgmres.lsqr_solver, "hybrid_lsqr": hgmres.hybrid_lsqr_solver, "lsmr": hgmres.lsmr_solver,
          "hybrid_lsmr": hgmres.hybrid_lsmr_solver}
PASSES = {"lsqr": 2, "hybrid_lsqr": 3, "lsmr": 4, "hybrid_lsmr": 3}     # operator passes per iteration of the batch

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
kinds = sys.argv[3:] or list(SINGLE)
N, na = GEOM[wl]
maxit, lam = 20, 1e-3
ctx = hgmres.Context(0)

from hgmres.problems import shepp_logan  # noqa: E402
A = hgmres.SparseOperator.siddon(N, na, ctx=ctx)
At = A.T
m, n = A.shape
x_true = shepp_logan(N).ravel(order="F")
b_exact = A @ x_true
rng = np.random.default_rng(0)
for kind in kinds:
    hybrid = kind.startswith("hybrid")
    for nrhs in (8, 20):
        Bm = np.empty((m, nrhs), order="F")
        for j, lv in enumerate(np.logspace(-4, -1, nrhs)):
            e = rng.standard_normal(m)
            Bm[:, j] = b_exact + e / np.linalg.norm(e) * lv * np.linalg.norm(b_exact)
        lams = np.full(nrhs, lam) if hybrid else None

        def batch():
            t0 = time.perf_counter()
            R = hgmres.gk_batch(A, Bm, x_true, 0.0, maxit, kind, lambdas=lams, At=At, ctx=ctx)
            ctx.synchronize()
            return time.perf_counter() - t0, R

        def loop():
            t0 = time.perf_counter()
            out = [SINGLE[kind](A, Bm[:, j], x_true, 0.0, maxit, *((lam,) if hybrid else ()), ctx=ctx, At=At)
                   for j in range(nrhs)]
            ctx.synchronize()
            return time.perf_counter() - t0, out

        batch(), loop()                                            # warm-up, both (plans, workspaces)
        tb, tl = [], []
        for _ in range(reps):                                      # alternating
            dt, R = batch()
            tb.append(dt)
            dt, out = loop()
            tl.append(dt)
        dev_ = max(float(np.max(np.abs(R.error_norm[:, j] - out[j][1]) / out[j][1])) for j in range(nrhs))
        ctx.kernel_timing(True)                                    # the split, from one more batch
        t0 = time.perf_counter()
        hgmres.gk_batch(A, Bm, x_true, 0.0, maxit, kind, lambdas=lams, At=At, ctx=ctx)
        ctx.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        op_ms, op_calls, op_bytes = ctx.kernel_timing_read(KC_SPMM)
        vk_ms, vk_calls, vk_bytes = ctx.kernel_timing_read(KC_GKMV)
        ctx.kernel_timing(False)
        ms, msl = statistics.median(tb) * 1e3, statistics.median(tl) * 1e3
        print(json.dumps(dict(
            what="gk_batch vs loop of single solves", workload=wl, kind=kind, maxit=maxit, nrhs=nrhs, reps=reps,
            batch_ms=round(ms, 2), batch_ms_min=round(min(tb) * 1e3, 2), loop_ms=round(msl, 2),
            loop_ms_min=round(min(tl) * 1e3, 2), loop_over_batch=round(msl / ms, 3),
            batch_ms_per_col_iter=round(ms / nrhs / maxit, 4), loop_ms_per_col_iter=round(msl / nrhs / maxit, 4),
            max_rel_dev_err_hist=dev_, timed_batch_ms=round(total, 2), operator_ms=round(op_ms, 2),
            operator_passes=op_calls, operator_GB=round(op_bytes / 1e9, 2), vector_ms=round(vk_ms, 2),
            vector_launch_groups=vk_calls, vector_GB=round(vk_bytes / 1e9, 2), rest_ms=round(total - op_ms - vk_ms, 2),
            passes_per_iteration=PASSES[kind],
            basis_GB=round(8.0 * n * maxit * nrhs / 1e9, 2) if kind == "hybrid_lsmr" else 0.0)), flush=True)
ctx.close()
del ctx
