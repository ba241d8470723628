"""Measurements of the perturbed multi-vector product and the mismatch sweep.  Run on an MI355X:
    python scripts/spmm_pert_micro.py products [reps]   hgm_spmm_pert (shared / general path) against two hgm_spmm + combine
    python scripts/spmm_pert_micro.py sweep [reps]      analysis.error_vs_mismatch_norm against the loop over explicit operators
One JSON line per point.

Operators: the bench's c2 (512^2, 30 angles) tiled Siddon projector A, B0 = A' (device transpose) and E = random
values on B0's pattern with ||E||_F = 1.

products, nvec 1, 4, 8, three routes alternating, each warmed:
  shared    hgm_spmm_pert (HGM_OPT_PERT_SHARED = 1: one index stream, one gather per entry);
  general   hgm_spmm_pert with option 39 = 0 (B0's row, then E's row);
  two       the route without the kernel: hgm_spmm(B0), hgm_spmm(E), then Y = YB + c * YE on the device (torch).
Host clock around `inner` back-to-back calls that end in a device synchronise, per call, median of `reps`: the same
clock for all three (the combine of `two` runs outside the library, so the kernel-timing events cannot see it).
For the two hgm_spmm_pert paths also the device time of the call's launches (class 5: pack, product, unpack and
the pixel-order permutes) and the GB/s of the kernel's algorithmic bytes over it: shared 20 nnz + 8 w (rows + cols),
general 12 (nnzB + nnzE) + 8 w (rows + cols), w = the interleaved width.

sweep: 20 levels c = logspace(-4, -1, 20) ||B0||_F, maxit 20, tol 1e-6, k_gcv 20, the hybrid AB and BA solvers with
GCV lambdas: error_vs_mismatch_norm (2 lockstep Arnoldis + 2 lockstep solves) against 20 x (2 hgm_arnoldi + 2 single
solves) on 20 uploaded explicit B0 + c E (their build and upload timed apart).  Host clock, synchronised.
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
from hgmres import analysis  # noqa: E402

N, NA = 512, 30
KC_SPMM = 5
mode = sys.argv[1] if len(sys.argv) > 1 else "products"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else (15 if mode == "products" else 3)
ctx = hgmres.Context(0)
lib = L.load()
dev = torch.device("cuda", 0)
P = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)  # noqa: E731


def operators():
    """A, B0 = A', E (B0's pattern and stored order, ||E||_F = 1), and A, E's transpose as scipy matrices."""
    A = hgmres.SparseOperator.siddon(N, NA, ctx=ctx)
    S = A.to_scipy()
    S.sort_indices()
    v = np.random.default_rng(21).standard_normal(S.nnz)
    Ev = sp.csr_matrix((v / np.linalg.norm(v), S.indices.copy(), S.indptr.copy()), shape=S.shape)
    return A, A.T, upload_like(A, Ev).T, S, Ev


def upload_like(A, M):
    """The scipy matrix M (reference pixel order) as a device operator in A's stored order."""
    n_, tile, sup = A.pixel_order("cols")
    if n_ == 0:
        return hgmres.SparseOperator.from_scipy(M, ctx=ctx)
    return hgmres.SparseOperator.from_scipy_tiled(M, n_, tile, sup, ctx=ctx)


def ok(rc):
    assert rc == 0, f"libhgmres status {rc}"


def products():
    A, B0, E, _, _ = operators()
    rows, cols = B0.shape
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(cols * 8, dtype=torch.float64, device=dev, generator=g)
    Y, YB, YE = (torch.zeros(rows * 8, dtype=torch.float64, device=dev) for _ in range(3))
    inner = 20
    for nv in (1, 4, 8):
        w = nv                                                           # 1, 4, 8 are interleaved widths
        cf = np.ascontiguousarray(np.logspace(-3, 0, nv))
        ct = torch.tensor(np.repeat(cf, rows), device=dev)               # column-major: c_r over column r

        def pert():
            ok(lib.hgm_spmm_pert(ctx.handle, B0._h, E._h, nv, cf.ctypes.data_as(L.dp), P(X), cols, P(Y), rows))

        def two():
            ok(lib.hgm_spmm(ctx.handle, B0._h, nv, P(X), cols, P(YB), rows))
            ok(lib.hgm_spmm(ctx.handle, E._h, nv, P(X), cols, P(YE), rows))
            ctx.synchronize()                                            # the combine runs on torch's stream
            torch.addcmul(YB[: rows * nv], ct, YE[: rows * nv], out=Y[: rows * nv])

        def clock(fn, shared):
            ctx.set_option("pert_shared", shared)
            torch.cuda.synchronize()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / inner

        def device_us(shared):
            ctx.set_option("pert_shared", shared)
            ctx.kernel_timing(True)
            pert()
            ms = ctx.kernel_timing_read(KC_SPMM)[0]
            ctx.kernel_timing(False)
            return ms * 1e3

        routes = (("shared", pert, 1), ("general", pert, 0), ("two", two, 1))
        for _, fn, sh in routes:                                         # warm every route
            clock(fn, sh)
        t = {k: [] for k, _, _ in routes}
        d = {"shared": [], "general": []}
        for _ in range(reps):                                            # alternating
            for k, fn, sh in routes:
                t[k].append(clock(fn, sh))
            d["shared"].append(device_us(1))
            d["general"].append(device_us(0))
        # the routes agree: shared == general bit for bit; `two` within a rounding of the combine (addcmul may fuse)
        two()
        torch.cuda.synchronize()
        ref = Y[: rows * nv].clone()
        ctx.set_option("pert_shared", 0)
        pert()
        ctx.synchronize()
        general = Y[: rows * nv].clone()
        ctx.set_option("pert_shared", 1)
        pert()
        ctx.synchronize()
        same = bool(torch.equal(Y[: rows * nv], general))
        dev_two = float((Y[: rows * nv] - ref).abs().max() / ref.abs().max())
        by = {"shared": 20.0 * B0.nnz + 8.0 * w * (rows + cols), "general": 12.0 * (B0.nnz + E.nnz) + 8.0 * w * (rows + cols)}
        out = dict(what="spmm_pert vs two spmm + combine", workload="c2", rows=rows, cols=cols, nnz=B0.nnz, nvec=nv,
                   reps=reps, inner=inner, shared_equals_general=same, max_dev_from_two_over_max=dev_two)
        for k in t:
            out[f"{k}_us"] = round(statistics.median(t[k]), 1)
            out[f"{k}_us_min"] = round(min(t[k]), 1)
            out[f"{k}_us_max"] = round(max(t[k]), 1)
        for k in d:
            us = statistics.median(d[k])
            out[f"{k}_device_us"] = round(us, 1)
            out[f"{k}_kernel_GBps"] = round(by[k] / us / 1e3, 1)
        out["two_over_shared"] = round(out["two_us"] / out["shared_us"], 3)
        out["two_over_general"] = round(out["two_us"] / out["general_us"], 3)
        print(json.dumps(out), flush=True)


def sweep():
    from hgmres.problems import shepp_logan
    A, B0, E, S, Ev = operators()
    m, n = A.shape
    x_true = shepp_logan(N).ravel(order="F")
    b_exact = A @ x_true
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(m)
    b = b_exact + noise / np.linalg.norm(noise) * 1e-2 * np.linalg.norm(b_exact)
    nl, maxit, tol, kg = 20, 20, 1e-6, 20
    cr = np.logspace(-4, -1, nl) * np.linalg.norm(S.data)
    t0 = time.perf_counter()
    Bc = [upload_like(A, sp.csr_matrix(S + c * Ev)).T for c in cr]       # the explicit operators, 12 B/entry each
    ctx.synchronize()
    upload_s = time.perf_counter() - t0

    def lockstep():
        t0 = time.perf_counter()
        M = analysis.error_vs_mismatch_norm(A, B0, E, b, x_true, cr, maxit=maxit, tol=tol, k_gcv=kg, ctx=ctx)
        ctx.synchronize()
        return time.perf_counter() - t0, M

    def loop():
        t0 = time.perf_counter()
        fin = {"ab": np.zeros(nl), "ba": np.zeros(nl)}
        for i in range(nl):
            for side, solver in (("ab", hgmres.ABgmres_hybrid_bounds), ("ba", hgmres.BAgmres_hybrid_bounds)):
                H, beta, _ = hgmres.arnoldi(A, Bc[i], b, kg, side, ctx=ctx)
                lam = hgmres.gcv_fminbnd(H, beta, m if side == "ab" else n, 1e-9, 1e-1, 1e-8)[0]
                fin[side][i] = solver(A, Bc[i], b, x_true, tol, maxit, lam, ctx=ctx)[1][-1]
        ctx.synchronize()
        return time.perf_counter() - t0, fin

    lockstep(), loop()                                                   # warm-up, both
    tl, to = [], []
    for _ in range(reps):                                                # alternating
        dt, M = lockstep()
        tl.append(dt)
        dt, fin = loop()
        to.append(dt)
    dev_ = max(float(np.max(np.abs(M[f"final_errors_h{s}"] - fin[s]) / fin[s])) for s in ("ab", "ba"))
    ms, mso = statistics.median(tl) * 1e3, statistics.median(to) * 1e3
    print(json.dumps(dict(
        what="error_vs_mismatch_norm vs loop over explicit operators", workload="c2", levels=nl, maxit=maxit,
        k_gcv=kg, reps=reps, nnz=B0.nnz, lockstep_ms=round(ms, 1), lockstep_ms_min=round(min(tl) * 1e3, 1),
        loop_ms=round(mso, 1), loop_ms_min=round(min(to) * 1e3, 1), loop_over_lockstep=round(mso / ms, 3),
        explicit_build_upload_s=round(upload_s, 2), explicit_operator_bytes=12 * B0.nnz * nl,
        max_rel_dev_final_error=dev_, niters_hab=[int(v) for v in M["niters_hab"]])), flush=True)


{"products": products, "sweep": sweep}[mode]()
ctx.close()
del ctx
