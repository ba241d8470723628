"""Measurements of the lambda sweep.  Run on an MI355X:
    python scripts/sweep_micro.py kernel [reps]     the monitor kernel hgm_proj_norms
    python scripts/sweep_micro.py solve [reps]      hgm_gmres_bounds_sweep against a loop of hgm_gmres_bounds
One JSON line per point.

kernel: rows = 2^24 and 2^18, k = 20, L in {1, 16, 100}; device time of the call's launches (events
around them on the context stream, hgm_kernel_timing class 4), median of `reps` warmed calls; GB/s on
the bytes of V (8 rows k), fp64 TFLOP/s on 2 rows k L (+ 5 rows L of the epilogue), and the bound each
point sits under from the MI355X peaks below.  The yardstick is hgm_proj_norms_loop on the same
buffers: the solvers' own single-coefficient monitor, L launches that read V L times.

solve: the bench's c2 geometry (512^2, 30 angles, tiled Siddon pair), AB side, maxit 20, tol 0,
L in {8, 100}; host time of a warmed call that ends in a device synchronise, median of `reps`.
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

HBM_GBPS = 8000.0        # MI355X peak HBM bandwidth
FP64_MATRIX_TF = 78.6    # MI355X peak fp64 matrix rate
KC_PNORM = 4

mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 25
ctx = hgmres.Context(0)
lib = L.load()
dev = torch.device("cuda", 0)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def timed_call(fn):
    """Device ms of the launches of one primitive call (timing class 4)."""
    ctx.kernel_timing(True)
    assert fn() == 0
    ms, calls, _ = ctx.kernel_timing_read(KC_PNORM)
    ctx.kernel_timing(False)
    assert calls == 1
    return ms


def kernel():
    k = 20
    g = torch.Generator(device=dev).manual_seed(0)
    for rows in (1 << 24, 1 << 18):
        ld = rows + 64
        V = torch.randn(ld * k, dtype=torch.float64, device=dev, generator=g)
        t = torch.randn(rows, dtype=torch.float64, device=dev, generator=g)
        for nl in (1, 16, 100):
            Y = torch.randn(k * nl, dtype=torch.float64, device=dev, generator=g)
            d, s, dl = np.zeros(nl), np.zeros(nl), np.zeros(nl)
            dpp = lambda a: a.ctypes.data_as(L.dp)  # noqa: E731
            one = lambda: lib.hgm_proj_norms(ctx.handle, rows, k, P(V), ld, P(Y), k, nl, P(t), dpp(d), dpp(s))  # noqa: E731
            loop = lambda: lib.hgm_proj_norms_loop(ctx.handle, rows, k, P(V), ld, P(Y), k, nl, P(t), dpp(dl))  # noqa: E731
            for f in (one, loop, one, loop):                       # warm-up, both
                assert f() == 0
            t_one, t_loop = [], []
            for _ in range(reps):                                  # alternating
                t_one.append(timed_call(one))
                t_loop.append(timed_call(loop))
            ms, ms_loop = statistics.median(t_one), statistics.median(t_loop)
            vbytes = 8.0 * rows * k
            flops = 2.0 * rows * k * nl + 5.0 * rows * nl
            t_bw, t_fl = vbytes / (HBM_GBPS * 1e9), flops / (FP64_MATRIX_TF * 1e12)
            print(json.dumps({
                "what": "kernel", "rows": rows, "k": k, "L": nl, "reps": reps,
                "ms": round(ms, 4), "ms_min": round(min(t_one), 4), "ms_max": round(max(t_one), 4),
                "V_GBps": round(vbytes / ms / 1e6, 1), "fp64_TFLOPs": round(flops / ms / 1e9, 2),
                "bound": "bandwidth" if t_bw >= t_fl else "fp64 issue",
                "share_of_bound": round(max(t_bw, t_fl) * 1e3 / ms, 3),
                "loop_ms": round(ms_loop, 4), "loop_over_one_pass": round(ms_loop / ms, 2),
                "rel_dev_vs_loop": float(np.max(np.abs(d - dl) / np.abs(dl)))}), flush=True)
        del V, t


def solve():
    N, na, maxit = 512, 30, 20
    from hgmres.problems import shepp_logan
    A = hgmres.SparseOperator.siddon(N, na, ctx=ctx)
    B = A.T
    x_true = shepp_logan(N).ravel(order="F")
    b_exact = A @ x_true
    e = np.random.default_rng(0).standard_normal(A.shape[0])
    b = b_exact + e / np.linalg.norm(e) * 1e-2 * np.linalg.norm(b_exact)
    info = hgmres.fused_plan_info(A, B)                            # the pair takes the one-pass route
    for nl in (8, 100):
        lams = np.logspace(-2, 5, nl)

        def sweep():
            t0 = time.perf_counter()
            S = hgmres.gmres_lambda_sweep(A, B, b, x_true, 0.0, maxit, lams, "ab", ctx=ctx)
            ctx.synchronize()
            return time.perf_counter() - t0, S

        def loop():
            t0 = time.perf_counter()
            out = [hgmres.ABgmres_hybrid_bounds(A, B, b, x_true, 0.0, maxit, lam, ctx=ctx) for lam in lams]
            ctx.synchronize()
            return time.perf_counter() - t0, out

        sweep(), loop()                                            # warm-up, both
        ts, tl = [], []
        for _ in range(reps):                                      # alternating
            dt, S = sweep()
            ts.append(dt)
            dt, out = loop()
            tl.append(dt)
        dev_ = max(float(np.max(np.abs(S.err[:, l] - out[l][1]) / out[l][1])) for l in range(nl))
        ms, msl = statistics.median(ts) * 1e3, statistics.median(tl) * 1e3
        print(json.dumps({"what": "solve", "N": N, "angles": na, "side": "ab", "maxit": maxit, "L": nl, "reps": reps,
                          "fused_plan_slots": info["nslot"], "sweep_ms": round(ms, 3),
                          "sweep_ms_min": round(min(ts) * 1e3, 3), "loop_ms": round(msl, 3),
                          "loop_ms_min": round(min(tl) * 1e3, 3), "loop_over_sweep": round(msl / ms, 2),
                          "max_rel_dev_err_hist": dev_}), flush=True)


{"kernel": kernel, "solve": solve}[mode]()
ctx.close()
del ctx
