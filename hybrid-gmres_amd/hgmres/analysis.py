"""The numeric pipeline of ``analyze_regularization.m`` over the device solvers.

``analyze_regularization.m`` is the consumer the north star requires to "see identical
outputs" (SURVEY.md §3.4, §8(f)2).  This module runs its numeric part, with the figures
left out, through the same entry points a MATLAB caller would reach (``*_bounds`` and the GCV
split ``hgm_arnoldi`` + ``hgm_gcv_fminbnd``):

* the 100-point lambda sweep of ``ABgmres_hybrid_bounds`` / ``BAgmres_hybrid_bounds`` with the
  relative residual, solution norm and last error of each solve (``:19-33``);
* the GCV lambda of each method by ``fminbnd`` over ``gcv_function`` on [1e-9, 1e-1], TolX 1e-8
  (``:35-49``).  ``gcv_function`` re-runs the same deterministic Arnoldi at every evaluation, so
  one Arnoldi and the lambda-dependent part on its H give the same values (``plot_gcv_surface.m:58-122``);
* the "true optimal" lambdas (argmin of the error curves, ``:41-42,47-48``);
* the final solves at the GCV lambdas and the non-hybrid solves (``:106-107,122-123``).

The problem set-up of ``:3-15`` (``shaw(32)``, ``randn`` noise, the mismatch ``E``) is
:func:`regularization_problem`; MATLAB's ``rng(0); randn`` cannot be reproduced here, so the
noise comes from numpy and the golden fixture stores the arrays.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import core
from .regtools import generate_test_problem


@dataclass
class RegularizationProblem:
    A: np.ndarray
    b: np.ndarray
    b_exact: np.ndarray
    x_true: np.ndarray
    E: np.ndarray
    B_pert: np.ndarray       # A' + E
    DeltaM_AB: np.ndarray    # A * E
    DeltaM_BA: np.ndarray    # E * A


def regularization_problem(n: int = 32, problem: str = "shaw", noise_level: float = 1e-2,
                           mismatch: float = 1e-4, seed: int = 0) -> RegularizationProblem:
    """``analyze_regularization.m:3-15`` (numpy's generator in place of ``rng(0); randn``)."""
    A, b_exact, x_true = generate_test_problem(problem, n)     # :5
    rng = np.random.default_rng(seed)                          # :7
    noise = rng.standard_normal(b_exact.shape)                 # :9
    noise = noise / np.linalg.norm(noise) * noise_level * np.linalg.norm(b_exact)   # :10
    b = b_exact + noise                                        # :11
    E = mismatch * rng.standard_normal(A.T.shape)              # :12
    B_pert = A.T + E                                           # :13
    return RegularizationProblem(A, b, b_exact, x_true, E, B_pert, A @ E, E @ A)   # :14-15


def analyze_regularization(P: RegularizationProblem, *, maxit: int = 32, tol: float = 1e-6,
                           lambda_range=None, k_gcv: int = 20, ctx=None, DeltaM_factored: bool = False,
                           sweep: bool = False) -> dict:
    """Numeric outputs of ``analyze_regularization.m`` (no figures).

    ``DeltaM_factored``: pass DeltaM as the factor pair (A, E) / (E, A) instead of the
    formed product (the at-scale form; the bounds outputs used here do not depend on it).

    ``sweep``: take the six arrays of the lambda loop (``:22-33``) from two
    :func:`hgmres.core.gmres_lambda_sweep` calls, one Arnoldi per side instead of one solve per
    lambda and side (fp64 operators, single rank, not in parity mode)."""
    ctx = ctx or core.default_context()
    lam_range = np.logspace(-10, 0, 100) if lambda_range is None else np.asarray(lambda_range, dtype=np.float64)
    A = core.as_operator(P.A, ctx)                             # uploaded once, reused by every solve
    Bp = core.as_operator(P.B_pert, ctx)
    dm_ab = (P.A, P.E) if DeltaM_factored else P.DeltaM_AB
    dm_ba = (P.E, P.A) if DeltaM_factored else P.DeltaM_BA
    nb = np.linalg.norm(P.b)
    out = {k: np.zeros(lam_range.size) for k in
           ("res_norms_ab", "sol_norms_ab", "err_norms_ab", "res_norms_ba", "sol_norms_ba", "err_norms_ba")}
    if sweep:                                                  # :22-33 from one Arnoldi per side
        for side in ("ab", "ba"):
            S = core.gmres_lambda_sweep(A, Bp, P.b, P.x_true, tol, maxit, lam_range, side, ctx=ctx, return_x=True)
            out[f"res_norms_{side}"] = np.linalg.norm(P.b[:, None] - P.A @ S.X, axis=0) / nb   # :25 / :30
            out[f"sol_norms_{side}"] = np.linalg.norm(S.X, axis=0)                            # :26 / :31
            out[f"err_norms_{side}"] = S.err[S.niters - 1, np.arange(lam_range.size)]         # :27 / :32
    for i, lam in enumerate(lam_range if not sweep else ()):   # :22-33
        x_ab, err_ab = core.ABgmres_hybrid_bounds(A, Bp, P.b, P.x_true, tol, maxit, lam, ctx=ctx)[:2]   # :24
        out["res_norms_ab"][i] = np.linalg.norm(P.b - P.A @ x_ab) / nb                                  # :25
        out["sol_norms_ab"][i] = np.linalg.norm(x_ab)                                                   # :26
        out["err_norms_ab"][i] = err_ab[-1]                                                             # :27
        x_ba, err_ba = core.BAgmres_hybrid_bounds(A, Bp, P.b, P.x_true, tol, maxit, lam, ctx=ctx)[:2]   # :29
        out["res_norms_ba"][i] = np.linalg.norm(P.b - P.A @ x_ba) / nb                                  # :30
        out["sol_norms_ba"][i] = np.linalg.norm(x_ba)                                                   # :31
        out["err_norms_ba"][i] = err_ba[-1]                                                             # :32
    m = P.A.shape[0]                                           # :36
    for side in ("ab", "ba"):                                  # :39-40 / :45-46
        H, beta, _ = core.arnoldi(A, Bp, P.b, k_gcv, side, ctx=ctx)
        trace_m = m if side == "ab" else P.A.shape[1]          # gcv_function.m:46-50
        lam_gcv, g = core.gcv_fminbnd(H, beta, trace_m, 1e-9, 1e-1, 1e-8)
        out[f"lambda_gcv_{side}"] = lam_gcv
        out[f"gcv_min_{side}"] = g
        idx = int(np.argmin(out[f"err_norms_{side}"]))          # :41 / :47  [min_err, idx] = min(err_norms)
        out[f"lambda_true_optimal_{side}"] = lam_range[idx]    # :42 / :48
        out[f"min_err_{side}"] = out[f"err_norms_{side}"][idx]
    out["x_optimal_ab"] = core.ABgmres_hybrid_bounds(A, Bp, P.b, P.x_true, tol, maxit, out["lambda_gcv_ab"],
                                                     dm_ab, ctx=ctx)[0]          # :106
    out["x_optimal_ba"] = core.BAgmres_hybrid_bounds(A, Bp, P.b, P.x_true, tol, maxit, out["lambda_gcv_ba"],
                                                     dm_ba, ctx=ctx)[0]          # :107
    out["solution_nonhybrid_ab"] = core.ABgmres_nonhybrid_bounds(A, Bp, P.b, P.x_true, tol, maxit, dm_ab,
                                                                 ctx=ctx)[0]     # :122
    out["solution_nonhybrid_ba"] = core.BAgmres_nonhybrid_bounds(A, Bp, P.b, P.x_true, tol, maxit, dm_ba,
                                                                 ctx=ctx)[0]     # :123
    out["lambda_range"] = lam_range
    return out


def error_surface(A, B, b, x_true, lambdas, maxit, tol=1e-10, *, ctx=None) -> dict:
    """The numeric part of ``plot_error_surface.m:21-48``: the (k, lambda) error surfaces of
    ``ABgmres_hybrid_bounds`` and ``BAgmres_hybrid_bounds`` (``maxit x nlam``: the transpose of the
    reference's arrays; NaN past each lambda's stopping iteration, ``:32,36``) and the optimal point of
    each (``:45-48``, ``:69-72``: ``k`` 1-based, ``lambda``, ``error``; ties go to the smaller k, then the
    smaller lambda index, as MATLAB's ``min`` over the flattened array), from one Arnoldi per side
    (:func:`hgmres.core.gmres_lambda_sweep`) instead of one solve per lambda and side (``:28-42``)."""
    lam = np.asarray(lambdas, dtype=np.float64).reshape(-1)
    out = {"lambdas": lam, "iterations": np.arange(1, int(maxit) + 1)}
    for side in ("ab", "ba"):
        S = core.gmres_lambda_sweep(A, B, b, x_true, tol, maxit, lam, side, ctx=ctx)
        surf = S.err
        out[f"error_surface_{side}"] = surf
        out[f"residual_surface_{side}"] = S.res
        out[f"niters_{side}"] = S.niters
        k, l = np.unravel_index(int(np.nanargmin(surf)), surf.shape)     # :45-46
        out[f"optimal_{side}"] = {"k": int(k) + 1, "lambda": float(lam[l]), "error": float(surf[k, l])}
    return out


def error_vs_noise_level(A, B, b_exact, x_true, noise_levels, *, maxit, tol=1e-6, k_gcv=20, lambdas=None, seed=0,
                         ctx=None) -> dict:
    """The numeric part of ``plot_error_vs_noise_level.m:28-54``: the final errors of the four ``*_bounds``
    solvers over a range of data noise levels, every solver's loop over the levels as ONE batched solve
    (:func:`hgmres.core.gmres_bounds_batch`: the right-hand sides share the operator passes) instead of one
    device solve per level and solver.

    Right-hand side i is ``b_exact + noise_i / ||noise_i|| * noise_levels[i] * ||b_exact||`` (``:31-32``) with
    ``noise_i`` drawn in order from ``numpy.random.default_rng(seed).standard_normal`` (not MATLAB's
    ``rng(0); randn`` stream, which cannot be reproduced here).  The hybrid solvers' lambdas are the GCV
    minimisers of ``:38-39`` / ``:43-44`` (``arnoldi`` + ``gcv_fminbnd`` per level and side, on [1e-9, 1e-1]
    with TolX 1e-8) unless ``lambdas = (lambdas_ab, lambdas_ba)`` supplies them.  The GCV Arnoldis still run
    one right-hand side at a time (batching them is follow-up work).

    Returns ``noise_levels``, the noisy ``Bm`` (``m x nlevels``), ``lambda_gcv_ab`` / ``lambda_gcv_ba`` and the
    curves ``final_errors_hab``, ``final_errors_hba``, ``final_errors_nab``, ``final_errors_nba``
    (``err(end)`` of each solve, ``:41,46,49,52``) with the matching ``niters_*``."""
    levels = np.asarray(noise_levels, dtype=np.float64).reshape(-1)
    nl = levels.size
    if nl < 1:
        raise ValueError("noise_levels is empty")
    m, n = A.shape
    b_exact = np.asarray(b_exact, dtype=np.float64).reshape(-1)
    x_true = np.asarray(x_true, dtype=np.float64).reshape(-1)
    if b_exact.size != m or x_true.size != n:
        raise ValueError(f"b_exact / x_true have lengths {b_exact.size} / {x_true.size}, expected {m} / {n}")
    if lambdas is not None:
        lab, lba = (np.asarray(v, dtype=np.float64).reshape(-1) for v in lambdas)
        if lab.size != nl or lba.size != nl:
            raise ValueError(f"lambdas: one value per noise level ({nl}) and side")
    rng = np.random.default_rng(seed)
    nbe = np.linalg.norm(b_exact)
    Bm = np.empty((m, nl), order="F")
    for i, level in enumerate(levels):                         # :29-32
        noise = rng.standard_normal(m)
        Bm[:, i] = b_exact + noise / np.linalg.norm(noise) * level * nbe
    ctx = ctx or (A.ctx if isinstance(A, core.SparseOperator) else core.default_context())
    Ao = core.as_operator(A, ctx)                              # uploaded once, reused by every solve
    Bo = core.as_operator(B, ctx)
    if lambdas is None:                                        # :34-39 / :43-44
        lab, lba = np.zeros(nl), np.zeros(nl)
        for side, lam in (("ab", lab), ("ba", lba)):
            trace_m = m if side == "ab" else n                 # gcv_function.m:46-50
            for i in range(nl):
                H, beta, _ = core.arnoldi(Ao, Bo, Bm[:, i], k_gcv, side, ctx=ctx)
                lam[i] = core.gcv_fminbnd(H, beta, trace_m, 1e-9, 1e-1, 1e-8)[0]
    out = {"noise_levels": levels, "Bm": Bm, "lambda_gcv_ab": lab, "lambda_gcv_ba": lba}
    for key, side, lam in (("hab", "ab", lab), ("hba", "ba", lba), ("nab", "ab", None), ("nba", "ba", None)):
        fin, nit = np.full(nl, np.nan), np.zeros(nl, dtype=int)
        for lo in range(0, nl, 64):                            # at most 64 columns per call
            hi = min(nl, lo + 64)
            R = core.gmres_bounds_batch(Ao, Bo, Bm[:, lo:hi], x_true, tol, maxit, side,
                                        lambdas=None if lam is None else lam[lo:hi], ctx=ctx)
            ok = R.niters >= 1
            fin[lo:hi][ok] = R.error_norm[R.niters[ok] - 1, np.nonzero(ok)[0]]     # err(end), :41 / :46 / :49 / :52
            nit[lo:hi] = R.niters
        out[f"final_errors_{key}"] = fin
        out[f"niters_{key}"] = nit
    return out


def equivalence_vs_noise_level(A, b_exact, x_true, noise_levels, *, maxit, tol=1e-6, lam=1e-3, seed=0, ctx=None) -> dict:
    """``run_equivalence_plots.m:12-22`` (the same ``b`` through all eight solvers, ``B = A'``: AB-GMRES == LSQR and
    BA-GMRES == LSMR) over the noise levels of ``plot_error_vs_noise_level.m:28-32``, each solver's loop over the
    levels as ONE lockstep solve: four :func:`hgmres.core.gmres_bounds_batch` calls (the four ``*_bounds`` solvers,
    the hybrid ones at ``lam``) and four :func:`hgmres.core.gk_batch` calls (``lsqr``, ``lsmr``, ``hybrid_lsqr``,
    ``hybrid_lsmr``).  ``B`` is the device transpose of ``A``.  The right-hand sides are drawn exactly as
    :func:`error_vs_noise_level` draws them.  Calls take at most 64 levels each.

    Returns ``noise_levels``, the noisy ``Bm`` (``m x nlevels``), ``final_errors_<key>`` / ``niters_<key>`` for the
    keys 'ab', 'ba', 'hab', 'hba' (non-hybrid / hybrid GMRES) and 'lsqr', 'lsmr', 'hybrid_lsqr', 'hybrid_lsmr', and
    ``gap_ab_lsqr`` / ``gap_ba_lsmr``: the largest relative gap ``|e1 - e2| / |e2|`` between the two error
    histories of a pair, over every level and the iterations both solvers ran."""
    levels = np.asarray(noise_levels, dtype=np.float64).reshape(-1)
    nl = levels.size
    if nl < 1:
        raise ValueError("noise_levels is empty")
    m, n = A.shape
    b_exact = np.asarray(b_exact, dtype=np.float64).reshape(-1)
    x_true = np.asarray(x_true, dtype=np.float64).reshape(-1)
    if b_exact.size != m or x_true.size != n:
        raise ValueError(f"b_exact / x_true have lengths {b_exact.size} / {x_true.size}, expected {m} / {n}")
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError("lam must be finite and >= 0")
    maxit = int(maxit)
    if maxit < 1:
        raise ValueError("maxit must be >= 1")
    rng = np.random.default_rng(seed)
    nbe = np.linalg.norm(b_exact)
    Bm = np.empty((m, nl), order="F")
    for i, level in enumerate(levels):                         # plot_error_vs_noise_level.m:29-32
        noise = rng.standard_normal(m)
        Bm[:, i] = b_exact + noise / np.linalg.norm(noise) * level * nbe
    ctx = ctx or (A.ctx if isinstance(A, core.SparseOperator) else core.default_context())
    Ao = core.as_operator(A, ctx)                              # uploaded once, reused by every solve
    Bo = Ao.T                                                  # :5 B = A'
    out = {"noise_levels": levels, "Bm": Bm, "lambda": float(lam)}
    hist = {}
    for key in ("ba", "lsmr", "ab", "lsqr", "hba", "hybrid_lsmr", "hab", "hybrid_lsqr"):       # :12-22
        fin, nit = np.full(nl, np.nan), np.zeros(nl, dtype=int)
        eh = np.full((maxit, nl), np.nan)
        for lo in range(0, nl, 64):                            # at most 64 columns per call
            hi = min(nl, lo + 64)
            lams = np.full(hi - lo, float(lam))
            if key in core.GK_KINDS:
                R = core.gk_batch(Ao, Bm[:, lo:hi], x_true, tol, maxit, key, At=Bo, ctx=ctx,
                                  lambdas=lams if core.GK_KINDS[key][1] else None)
            else:
                R = core.gmres_bounds_batch(Ao, Bo, Bm[:, lo:hi], x_true, tol, maxit, key[-2:],
                                            lambdas=lams if key[0] == "h" else None, ctx=ctx)
            ok = R.niters >= 1
            fin[lo:hi][ok] = R.error_norm[R.niters[ok] - 1, np.nonzero(ok)[0]]     # err(end)
            nit[lo:hi] = R.niters
            eh[:, lo:hi] = R.error_norm
        out[f"final_errors_{key}"] = fin
        out[f"niters_{key}"] = nit
        hist[key] = eh
    for pair, k1, k2 in (("ab_lsqr", "ab", "lsqr"), ("ba_lsmr", "ba", "lsmr")):
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.abs(hist[k1] - hist[k2]) / np.abs(hist[k2])
        out["gap_" + pair] = float(np.nanmax(g)) if np.any(np.isfinite(g)) else float("nan")
    return out


def _fro(E):
    """``norm(E, 'fro')`` of a scipy matrix, an array, a device operator or a matrix-free Gaussian."""
    if isinstance(E, core.GaussianPerturbation):
        return float(E.fro())
    if isinstance(E, core.SparseOperator):
        E = E.to_scipy()
    if hasattr(E, "data") and hasattr(E, "tocsr"):
        return float(np.linalg.norm(E.tocsr().data))
    return float(np.linalg.norm(np.asarray(E, dtype=np.float64)))


def error_vs_mismatch_norm(A, B0, E, b, x_true, c_range, *, maxit, tol=1e-6, k_gcv=20, lambdas=None,
                           solvers=("hab", "hba"), ctx=None) -> dict:
    """The numeric part of ``plot_error_vs_mismatch_norm.m:23-61`` (and, with all four ``solvers``, of
    ``run_2D_phantom.m:79-102``): the final errors of the ``*_bounds`` solvers over a range of back-projector
    mismatch levels ``B_pert = B0 + c * E`` for one fixed ``E``, every solver's loop over the levels as ONE
    lockstep solve (:func:`hgmres.core.gmres_bounds_mismatch`) and the GCV Arnoldis of all levels as one
    lockstep Arnoldi per side (:func:`hgmres.core.arnoldi_mismatch`).  No ``B_pert`` is formed or uploaded:
    ``B0`` and ``E`` are read once per group of up to 8 levels.  ``E`` may be a
    :class:`hgmres.GaussianPerturbation`, the reference's own dense ``E = randn(size(A'))`` (``:16-17``:
    ``G.normalized()``), which is regenerated on the device and never stored.

    ``b`` is the (noisy) right-hand side shared by every level.  The hybrid solvers' lambdas are the GCV
    minimisers of ``:46-50`` (``gcv_fminbnd`` on [1e-9, 1e-1] with TolX 1e-8 on each level's H) unless
    ``lambdas = (lambdas_ab, lambdas_ba)`` supplies them.  ``solvers`` picks from 'hab', 'hba' (the hybrid
    solvers of ``:53-56``) and 'nab', 'nba' (the non-hybrid ones).  Calls take at most 64 levels each.

    Returns ``c_range``, ``mismatch_norms = |c| * ||E||_F`` (``:36``), ``lambda_gcv_ab`` / ``lambda_gcv_ba`` (NaN
    for a side no hybrid solver asked for and no ``lambdas`` gave) and, per solver key, ``final_errors_<key>``
    (``err(end)``, ``:54,57``) and ``niters_<key>``."""
    cr = np.asarray(c_range, dtype=np.float64).reshape(-1)
    nl = cr.size
    if nl < 1:
        raise ValueError("c_range is empty")
    if not np.all(np.isfinite(cr)):
        raise ValueError("c_range: every level must be finite")
    keys = {"hab": ("ab", True), "hba": ("ba", True), "nab": ("ab", False), "nba": ("ba", False)}
    solvers = tuple(solvers)
    if not solvers or any(s not in keys for s in solvers):
        raise ValueError(f"solvers: a non-empty choice of {sorted(keys)}, not {solvers!r}")
    m, n = A.shape
    if tuple(B0.shape) != (n, m) or tuple(E.shape) != (n, m):
        raise ValueError(f"B0 / E have shapes {tuple(B0.shape)} / {tuple(E.shape)}, expected ({n}, {m})")
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x_true = np.asarray(x_true, dtype=np.float64).reshape(-1)
    if b.size != m or x_true.size != n:
        raise ValueError(f"b / x_true have lengths {b.size} / {x_true.size}, expected {m} / {n}")
    lam = {"ab": np.full(nl, np.nan), "ba": np.full(nl, np.nan)}
    if lambdas is not None:
        lab, lba = (np.asarray(v, dtype=np.float64).reshape(-1) for v in lambdas)
        if lab.size != nl or lba.size != nl:
            raise ValueError(f"lambdas: one value per mismatch level ({nl}) and side")
        lam = {"ab": lab, "ba": lba}
    out = {"c_range": cr, "mismatch_norms": np.abs(cr) * _fro(E)}          # :33-36
    ctx = ctx or (A.ctx if isinstance(A, core.SparseOperator) else core.default_context())
    Ao = core.as_operator(A, ctx)                              # uploaded once, reused by every solve
    Bo = core.as_operator(B0, ctx)
    Eo = E if isinstance(E, core.GaussianPerturbation) else core.as_operator(E, ctx)
    chunks = [(lo, min(nl, lo + 64)) for lo in range(0, nl, 64)]            # at most 64 levels per call
    if lambdas is None:                                        # :42-50
        for side in sorted({keys[s][0] for s in solvers if keys[s][1]}):
            trace_m = m if side == "ab" else n                 # gcv_function.m:46-50
            for lo, hi in chunks:
                H, beta, _ = core.arnoldi_mismatch(Ao, Bo, Eo, cr[lo:hi], b, k_gcv, side, ctx=ctx)
                for i in range(lo, hi):
                    lam[side][i] = core.gcv_fminbnd(H[i - lo], beta[i - lo], trace_m, 1e-9, 1e-1, 1e-8)[0]
    out["lambda_gcv_ab"], out["lambda_gcv_ba"] = lam["ab"], lam["ba"]
    for key in solvers:
        side, hybrid = keys[key]
        fin, nit = np.full(nl, np.nan), np.zeros(nl, dtype=int)
        for lo, hi in chunks:
            R = core.gmres_bounds_mismatch(Ao, Bo, Eo, cr[lo:hi], b, x_true, tol, maxit, side,
                                           lambdas=lam[side][lo:hi] if hybrid else None, ctx=ctx)
            ok = R.niters >= 1
            fin[lo:hi][ok] = R.error_norm[R.niters[ok] - 1, np.nonzero(ok)[0]]     # err(end), :54 / :57
            nit[lo:hi] = R.niters
        out[f"final_errors_{key}"] = fin
        out[f"niters_{key}"] = nit
    return out


def filter_factor_comparison(A, B, b, x_true, *, maxit, tol, lam, DeltaM_AB=None, DeltaM_BA=None, steps, nsv,
                             ctx=None) -> dict:
    """The numeric part of ``plot_filter_factors.m:23-40`` (no figures): the four ``*_bounds`` solves with
    their theoretical filter factors ``phi_final`` (``:23-26``; outputs 5-8 need ``DeltaM_AB`` / ``DeltaM_BA``,
    else ``phi`` / ``dphi`` are None), and the empirical filter factors of the four solutions on the
    leading singular triplets of ``A`` (``:30-40``) from ONE :func:`hgmres.core.svds` run started at ``b``
    with the four solutions as ``X``, in place of ``svd(A,'econ')``.

    Per method ``ab``, ``ba`` (non-hybrid), ``hab``, ``hba`` (hybrid): ``x_*``, ``err_*``, ``res_*``, ``it_*``,
    ``phi_*`` (``phi_final``), ``dphi_*`` and ``Phi_emp_*`` (``nsv`` values, NaN past the triplets found);
    plus ``sigma``, ``resid``, ``utb``, ``nconv`` and ``steps_done`` of the triplets."""
    ctx = ctx or core.default_context()
    Ao = core.as_operator(A, ctx)
    Bo = core.as_operator(B, ctx)
    runs = (("ab", core.ABgmres_nonhybrid_bounds, (), DeltaM_AB),       # :23
            ("ba", core.BAgmres_nonhybrid_bounds, (), DeltaM_BA),       # :24
            ("hab", core.ABgmres_hybrid_bounds, (lam,), DeltaM_AB),     # :25
            ("hba", core.BAgmres_hybrid_bounds, (lam,), DeltaM_BA))     # :26
    out = {}
    for name, fn, extra, dm in runs:
        r = fn(Ao, Bo, b, x_true, tol, maxit, *extra, dm, ctx=ctx)
        out[f"x_{name}"], out[f"err_{name}"], out[f"res_{name}"], out[f"it_{name}"] = r[:4]
        out[f"phi_{name}"], out[f"dphi_{name}"] = r[4], r[5]
    X = np.column_stack([out[f"x_{name}"] for name, *_ in runs])
    E = core.empirical_filter_factors(Ao, b, X, steps, nsv, ctx=ctx)    # :30-40
    for j, (name, *_) in enumerate(runs):
        out[f"Phi_emp_{name}"] = E.Phi[:, j].copy()
    out.update(sigma=E.sigma, resid=E.resid, utb=E.svds.utb, nconv=E.nconv, steps_done=E.svds.steps_done)
    return out
