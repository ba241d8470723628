"""Measurements of the multi-vector product and the batched solves.  Run on an MI355X:
    python scripts/spmm_micro.py products c3|c4 [reps]   hgm_spmm against loops of hgm_spmv / hgm_spmv_ab
    python scripts/spmm_micro.py solve c3|c4 [reps]      hgm_gmres_bounds_batch against a loop of hgm_gmres_bounds_ex
One JSON line per point.

The yardstick is always the route the library had before the batch: one hgm_spmv (hgm_spmv_ab) or one
single solve per column.  Operators: the bench's c3 (2048^2, 19 angles) and c4 (4096^2, 47 angles) tiled
Siddon projectors A and their device transposes B.

products: device time of one call's launches from the kernel-timing events (class 5 for hgm_spmm: pack,
product and unpack, and the pixel-order permutes around them; classes 0 / 1 / 3 for the yardsticks, which
time their product kernels alone, so the comparison leans towards the yardstick), median of `reps` warmed
calls, the two routes alternating.  Per column: ms, entries/s (nnz per column and second) and bytes/s on the
algorithmic bytes (12 nnz + 8 (rows + 1) once per call, 8 (rows + cols) per column).

solve: AB side, non-hybrid, maxit 20, tol 0 (no column leaves early), 8 and 20 noisy right-hand sides; host
time around the calls, synchronised, median of `reps`; then one timed batch for the step's split between the
operator passes (class 5), the orthogonalisation (class 2) and the rest (projected solves, monitors, host).
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

GEOM = {"c3": (2048, 19), "c4": (4096, 47)}
KC_A, KC_B, KC_MGS, KC_FUSED, KC_SPMM = 0, 1, 2, 3, 5

mode = sys.argv[1] if len(sys.argv) > 1 else "products"
wl = sys.argv[2] if len(sys.argv) > 2 else "c3"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 15
N, na = GEOM[wl]
ctx = hgmres.Context(0)
lib = L.load()
dev = torch.device("cuda", 0)
P = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)  # noqa: E731


def timed(fn, classes):
    """Device ms of the launches of fn() in the given timing classes."""
    ctx.kernel_timing(True)
    fn()
    ms = sum(ctx.kernel_timing_read(k)[0] for k in classes)
    ctx.kernel_timing(False)
    return ms


def point(what, op, nv, M, t_new, t_old, extra):
    ms, ms_old = statistics.median(t_new), statistics.median(t_old)
    m, n = M.shape
    bytes_ = 12.0 * M.nnz + 8.0 * (m + 1) + 8.0 * nv * (m + n)
    print(json.dumps(dict(
        what=what, workload=wl, operator=op, rows=m, cols=n, nnz=M.nnz, nvec=nv, reps=reps,
        spmm_ms=round(ms, 4), spmm_ms_min=round(min(t_new), 4), spmm_ms_max=round(max(t_new), 4),
        spmm_ms_per_col=round(ms / nv, 4), spmm_Gentries_per_s=round(M.nnz * nv / ms / 1e6, 1),
        spmm_GBps=round(bytes_ / ms / 1e6, 1), loop_ms=round(ms_old, 4), loop_ms_per_col=round(ms_old / nv, 4),
        loop_Gentries_per_s=round(M.nnz * nv / ms_old / 1e6, 1), loop_over_spmm=round(ms_old / ms, 3), **extra)),
        flush=True)


def products():
    A = hgmres.SparseOperator.siddon(N, na, ctx=ctx)
    B = A.T
    m, n = A.shape
    g = torch.Generator(device=dev).manual_seed(0)
    Xn = torch.randn(n * 8, dtype=torch.float64, device=dev, generator=g)
    Xm = torch.randn(m * 8, dtype=torch.float64, device=dev, generator=g)
    Yn = torch.zeros(n * 8, dtype=torch.float64, device=dev)
    Ym = torch.zeros(m * 8, dtype=torch.float64, device=dev)
    Y1n = torch.zeros(n, dtype=torch.float64, device=dev)
    Y1m = torch.zeros(m, dtype=torch.float64, device=dev)

    def ok(rc):
        assert rc == 0, f"libhgmres status {rc}"

    for op, M, X, Y, Y1 in (("A", A, Xn, Ym, Y1m), ("B=A'", B, Xm, Yn, Y1n)):
        rows, cols = M.shape
        for nv in (1, 2, 4, 8):
            new = lambda: ok(lib.hgm_spmm(ctx.handle, M._h, nv, P(X), cols, P(Y), rows))  # noqa: E731

            def old():
                for r in range(nv):
                    ok(lib.hgm_spmv(ctx.handle, M._h, P(X, r * cols), P(Y1)))

            for f in (new, old, new, old):
                f()
            t_new, t_old = [], []
            for _ in range(reps):
                t_new.append(timed(new, (KC_SPMM,)))
                t_old.append(timed(old, (KC_A, KC_B)))
            torch.cuda.synchronize()
            dev_ = float((Y[(nv - 1) * rows: nv * rows] - Y1).abs().max() / Y1.abs().max())
            point("spmm vs nvec x hgm_spmv", op, nv, M, t_new, t_old, {"max_dev_last_col_over_max": dev_})
    # A*(B*X): two multi-vector passes against nvec x hgm_spmv_ab (the one-pass plan where the pair has one)
    info = hgmres.fused_plan_info(A, B)
    for nv in (1, 2, 4, 8):
        def new():
            ok(lib.hgm_spmm(ctx.handle, B._h, nv, P(Xm), m, P(Yn), n))
            ok(lib.hgm_spmm(ctx.handle, A._h, nv, P(Yn), n, P(Ym), m))

        def old():
            for r in range(nv):
                ok(lib.hgm_spmv_ab(ctx.handle, A._h, B._h, P(Xm, r * m), P(Y1n), P(Y1m)))

        for f in (new, old, new, old):
            f()
        t_new, t_old = [], []
        for _ in range(reps):
            t_new.append(timed(new, (KC_SPMM,)))
            t_old.append(timed(old, (KC_A, KC_B, KC_FUSED)))
        torch.cuda.synchronize()
        dev_ = float((Ym[(nv - 1) * m: nv * m] - Y1m).abs().max() / Y1m.abs().max())

        class AB:            # the pair as one operator for the per-column figures
            shape = (m + n, m + n)
            nnz = A.nnz + B.nnz
        point("A*(B*X): two spmm passes vs nvec x hgm_spmv_ab", "A*B", nv, AB, t_new, t_old,
              {"fused_plan_slots": info["nslot"], "max_dev_last_col_over_max": dev_})


def solve():
    from hgmres.problems import shepp_logan
    maxit = 20
    A = hgmres.SparseOperator.siddon(N, na, ctx=ctx)
    B = A.T
    m, n = A.shape
    x_true = shepp_logan(N).ravel(order="F")
    b_exact = A @ x_true
    rng = np.random.default_rng(0)
    for nrhs in (8, 20):
        Bm = np.empty((m, nrhs), order="F")
        for j, lv in enumerate(np.logspace(-4, -1, nrhs)):
            e = rng.standard_normal(m)
            Bm[:, j] = b_exact + e / np.linalg.norm(e) * lv * np.linalg.norm(b_exact)

        def batch():
            t0 = time.perf_counter()
            R = hgmres.gmres_bounds_batch(A, B, Bm, x_true, 0.0, maxit, "ab", ctx=ctx)
            ctx.synchronize()
            return time.perf_counter() - t0, R

        def loop():
            t0 = time.perf_counter()
            out = [hgmres.ABgmres_nonhybrid_bounds(A, B, Bm[:, j], x_true, 0.0, maxit, ctx=ctx) for j in range(nrhs)]
            ctx.synchronize()
            return time.perf_counter() - t0, out

        batch(), loop()                                            # warm-up, both
        tb, tl = [], []
        for _ in range(reps):                                      # alternating
            dt, R = batch()
            tb.append(dt)
            dt, out = loop()
            tl.append(dt)
        dev_ = max(float(np.max(np.abs(R.error_norm[:, j] - out[j][1]) / out[j][1])) for j in range(nrhs))
        # the step's split, from one more batch with the kernel-timing events on
        ctx.kernel_timing(True)
        t0 = time.perf_counter()
        hgmres.gmres_bounds_batch(A, B, Bm, x_true, 0.0, maxit, "ab", ctx=ctx)
        ctx.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        op_ms, op_calls, _ = ctx.kernel_timing_read(KC_SPMM)
        mgs_ms, mgs_calls, _ = ctx.kernel_timing_read(KC_MGS)
        ctx.kernel_timing(False)
        ms, msl = statistics.median(tb) * 1e3, statistics.median(tl) * 1e3
        print(json.dumps(dict(
            what="batch solve vs loop of single solves", workload=wl, side="ab", hybrid=0, maxit=maxit, nrhs=nrhs,
            reps=reps, batch_ms=round(ms, 2), batch_ms_min=round(min(tb) * 1e3, 2), loop_ms=round(msl, 2),
            loop_ms_min=round(min(tl) * 1e3, 2), loop_over_batch=round(msl / ms, 3), max_rel_dev_err_hist=dev_,
            timed_batch_ms=round(total, 2), operator_ms=round(op_ms, 2), operator_groups=op_calls,
            mgs_ms=round(mgs_ms, 2), mgs_calls=mgs_calls, rest_ms=round(total - op_ms - mgs_ms, 2),
            operator_share=round(op_ms / total, 3), mgs_share=round(mgs_ms / total, 3),
            rest_share=round((total - op_ms - mgs_ms) / total, 3))), flush=True)


{"products": products, "solve": solve}[mode]()
ctx.close()
del ctx
