"""The lockstep multi-column solves at long, odd, non-square sizes.

gmres_bounds_batch, gmres_bounds_mismatch / arnoldi_mismatch, gk_batch and gmres_lambda_sweep are tested
elsewhere on the 24^2 tomography fixtures (n = 576, a ray count of the same order), where every vector kernel
under them takes one path: the padded one-workgroup MGS, one-launch reductions, one-block Golub-Kahan updates.
test_gpu_lengths.py walks the other paths with the single solvers; this file does with the lockstep ones:

  0. a CPU test that ties the shapes, column counts and budgets below to the constants of csrc/;
  1. gmres_bounds_batch against the oracle, columns leaving the batch at different iterations;
  2. bitwise composition where the per-column MGS workspace matters (batch = its columns alone = itself
     after an unrelated batch on the same context);
  3. the mismatch sweeps against the oracle on explicit B0 + c E;
  4. gk_batch against the oracle, its bitwise composition across a re-gather, and past the grid-stride cap;
  5. lockstep runs across step MGS1_MAXC = 120 under mgs_single = 0;
  6. the lambda sweep.

The operator is test_gpu_lengths.py's 1-D blur with B = A', the reference oracle/restatement.py (fp64 numpy)
called once per column, the right-hand sides noisy_rhs(A x_true, LEVELS).  Nothing is read from tests/golden.
Where the oracle's own spread under the rounding model (test_gpu_parity._Rounded, 8 seeds; a 1-ulp copy of the
operator values where B*A is formed explicitly) exceeds 1e-12, the 1e-10 bar no longer keeps the project's
100x margin: those cases (ENVELOPED) are judged per entry at max(1e-10, 100 x spread), computed in the test,
and no entry's bar may pass GKB_CAP.  The measured spreads are quoted at each section.
"""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import hgmres
from oracle import restatement as R   # checker only
from test_gpu_batch import CASES, ORACLE, SINGLE, hist_ok, noisy_rhs, rel, same_batch
from test_gpu_gkbatch import GRID_CAP, KINDS, NHIST, _envelope, _hists, same_gk
from test_gpu_lengths import (LAM, LONG_SHAPES, SHAPES, _csrc_constants, _device_ops, _kdone, _long_check,
                              _long_envelope, _problem, _ulp_copy, blur_problem)
from test_gpu_parity import GKB_CAP, TOL, H_ok, _gkb_check, _Rounded
from test_gpu_sweep import _oracle_sweep

gpu = pytest.mark.gpu

MAXIT = 12
NRHS = 5
LEVELS = np.logspace(-4, -1, NRHS)
# per-column lambdas of the hybrid solvers, distinct, around LAM (test_gpu_lengths.py says why 1e-4)
LAMS = LAM * np.array([0.5, 0.7, 1.0, 1.4, 2.0])
NCOMP = 9                                    # composition tests: the columns pack as groups of 8 + 1
LEVELS9 = np.logspace(-4, -1, NCOMP)
LAMS9 = LAM * np.logspace(-0.3, 0.3, NCOMP)
CAP_SHAPES = ((1537, GRID_CAP + 257), (GRID_CAP + 257, 1537))
LONG = LONG_SHAPES[1]
LONG_BUDGET = 124
SWEEP_LAMS = np.logspace(-4, -1, 6)
MISMATCH_COEFS = np.array([0.0, 1e-3, 1e-2, 3e-2, 1e-1])
ARNOLDI_K = 8
ids = lambda s: f"{s[0]}x{s[1]}"   # noqa: E731
case_id = lambda c: c[0] + ("p" if c[1] else "n")   # noqa: E731


@functools.lru_cache(maxsize=None)
def _rhs(shape, ncol=NRHS, seed=7):
    """noisy_rhs(A x_true, logspace(-4, -1, ncol)) of the shape's blur problem: read-only, shared."""
    A, _, _, xt = _problem(*shape)
    Bm = noisy_rhs(A @ xt, np.logspace(-4, -1, ncol), seed=seed)
    Bm.setflags(write=False)
    return Bm


# ---------------------------------------------------------------------------------------------
# 0. the shapes against the constants of csrc/
# ---------------------------------------------------------------------------------------------
def test_lockstep_shapes_cover_the_dispatch_edges():
    """The Krylov dimensions (n on the BA side, m on the AB side: every shape runs both), vector lengths, column
    counts and the long budget of this file against csrc/'s constants, read by regular expression.  A constant
    that moves fails this test instead of silently leaving its edge uncovered."""
    v, _ = _csrc_constants()
    with open(os.path.join(ROOT, "hybrid-gmres_amd", "csrc", "internal.h")) as fh:
        mt = re.search(r"constexpr\s+int\s+SPMM_MAXV\s*=\s*(\d+)\s*;", fh.read())
    assert mt, "SPMM_MAXV"
    maxv = int(mt.group(1))
    dims = sorted({d for s in SHAPES for d in s})
    assert any(d % 2 and d > v["MGS1_MAX"] for d in dims), dims            # past the one-workgroup MGS
    assert any(d % 2 and d > v["SINGLE_MAX"] for d in dims), dims          # past the one-launch reductions
    assert any(d <= v["MGS1_MAX"] for d in dims)                           # and a short side next to them
    # the composition tests need the one-reduction MGS (its Gram triangle kept per column): dim > MGS1_MAX by
    # default, any dim under mgs_single = 0
    assert SHAPES[0][1] > v["MGS1_MAX"] and SHAPES[1][0] > v["MGS1_MAX"] and SHAPES[2][1] > v["SINGLE_MAX"]
    assert GRID_CAP == v["BS"] * v["MAX_PARTS"]
    for s in CAP_SHAPES:                                                   # a thread strides over > 1 row
        assert max(s) > v["BS"] * v["MAX_PARTS"] and max(s) % 2 and min(s) <= v["MGS1_MAX"]
    assert NCOMP == maxv + 1 and NRHS < maxv                               # the last packed group: one column
    assert LONG_BUDGET > v["MGS1_MAXC"] + 1 and max(LONG) <= v["MGS1_MAX"]  # mgs_single = 0 decides the form
    assert MAXIT < v["MGS1_MAXC"] and ARNOLDI_K < MAXIT


# ---------------------------------------------------------------------------------------------
# solutions, envelopes and the comparison shared by sections 1, 3 and 6
# ---------------------------------------------------------------------------------------------
def _sol(x, k, H, **hists):
    return dict(x=np.asarray(x), k=int(k), H=np.asarray(H), hists={n: np.asarray(h) for n, h in hists.items()})


def _bounds_sol(o):
    """(x, err, res, niters, H) of a *_bounds solve."""
    return _sol(o[0], o[3], o[4], err=o[1], res=o[2])


def _batch_col(Rb, j):
    k = int(Rb.niters[j])
    for h in (Rb.error_norm, Rb.residual_norm):
        assert np.all(np.isnan(h[k:, j])) and np.all(np.isfinite(h[:k, j])), j   # NaN past niters, and only there
    return _sol(Rb.x[:, j], k, Rb.H[j], err=Rb.error_norm[:k, j], res=Rb.residual_norm[:k, j])


def _gm_envelope(run, A, B, explicit=False):
    """Per-entry bars max(TOL, 100 x spread) of the oracle run(A, B) -> _sol(...) under 8 seeds of the rounding
    model (a 1-ulp copy of the values where the oracle forms B*A explicitly), none past GKB_CAP."""
    ref = run(A, B)
    hmax = np.max(np.abs(ref["H"]))
    sH, sx = np.zeros_like(ref["H"]), 0.0
    sh = {n: np.zeros(h.shape) for n, h in ref["hists"].items()}
    for seed in range(1, 9):
        rng = np.random.default_rng(seed)
        Ap, Bp = (_ulp_copy(A, rng), _ulp_copy(B, rng)) if explicit else (_Rounded(A, rng), _Rounded(B, rng))
        p = run(Ap, Bp)
        assert p["k"] == ref["k"], (p["k"], ref["k"])
        sH = np.maximum(sH, np.abs(p["H"] - ref["H"]) / hmax)
        sx = max(sx, rel(p["x"], ref["x"]))
        for n, h in ref["hists"].items():
            sh[n] = np.maximum(sh[n], np.abs(p["hists"][n] - h) / np.abs(h))
    bar = dict(H=np.maximum(TOL, 100.0 * sH), x=max(TOL, 100.0 * sx),
               hists={n: np.maximum(TOL, 100.0 * s) for n, s in sh.items()})
    worst = max([float(np.max(bar["H"])), bar["x"]] + [float(np.max(t)) for t in bar["hists"].values()])
    assert worst <= GKB_CAP, ("an envelope past the cap", worst)
    spread = max([float(np.max(sH)), sx] + [float(np.max(s)) for s in sh.values()])
    return bar, spread


def _sol_ok(out, ref, bar=None, what=""):
    """niters equal; H against max|H|, x in norm, every history per entry: at TOL, or at the envelope `bar`.
    Returns the largest deviation of each."""
    assert out["k"] == ref["k"], (what, out["k"], ref["k"])
    hmax = np.max(np.abs(ref["H"]))
    dH = np.abs(out["H"] - ref["H"]) / hmax
    dx = rel(out["x"], ref["x"])
    dev = dict(H=float(np.max(dH)), x=float(dx))
    if bar is None:
        H_ok(out["H"], ref["H"], TOL)
        assert dx <= TOL, (what, dx)
    else:
        assert np.all(dH <= bar["H"]), (what, "H", float(np.max(dH / bar["H"])))
        assert dx <= bar["x"], (what, "x", dx, bar["x"])
    for n, h in ref["hists"].items():
        a = out["hists"][n]
        assert a.shape == h.shape, (what, n, a.shape, h.shape)
        d = np.abs(a - h) / np.abs(h)
        dev[n] = float(np.max(d))
        if bar is None:
            hist_ok(a, h, TOL)
        else:
            assert np.all(d <= bar["hists"][n]), (what, n, float(np.max(d / bar["hists"][n])))
    return dev


def _report(tag, devs, spread=None):
    worst = {k: max(d[k] for d in devs) for k in devs[0]}
    print(f"[lockstep {tag}] " + " ".join(f"{k}={v:.1e}" for k, v in worst.items())
          + (f" (enveloped: oracle spread {spread:.1e})" if spread is not None else ""))


def _spread_ok(nits, hists, tol, maxit=MAXIT):
    """The issue's conditions on the oracle's own result: at least two distinct niters, at least one below
    maxit, every deciding residual (each entry of each returned history was compared with tol) at least 2 %
    away from tol."""
    assert len(set(nits)) >= 2 and min(nits) < maxit, nits
    margin = min(float(np.min(np.abs(np.asarray(h) - tol))) for h in hists) / tol
    assert margin >= 0.02, (margin, nits)
    return margin


# ---------------------------------------------------------------------------------------------
# 1. gmres_bounds_batch against the oracle
#    5 columns (noise levels LEVELS, lambdas LAMS), 12 iterations.  Stopping tolerances picked on the CPU from the
#    oracle's tol = 0 residual histories: among the geometric midpoints of neighbouring history values, the one
#    with the most distinct niters, then the latest stops, with every deciding entry >= 3 % away.  Oracle niters
#    and oracle spread (8 seeds, largest over the columns and over H, x and both histories), measured on the CPU:
#                         abp                      bap                      abn                      ban
#      1537 x 24577   1.91e-2 [1,2,12,12,12]   1.91e-2 [1,2,12,12,12]   8.06e-4 [9,10,12,12,12]  3.0e-3 [3,3,5,12,12]
#                     4.7e-14                  1.7e-12 *                2.1e-13                  2.9e-13
#      24577 x 1537   4.47e-3 [6,6,8,12,12]    4.67e-3 [6,6,8,12,12]    4.47e-3 [6,6,8,12,12]    4.67e-3 [6,6,8,12,12]
#                     7.8e-13                  1.1e-12 *                5.4e-13                  4.4e-13
#      32769 x 32769  4.32e-3 [6,6,7,12,12]    3.89e-3 [7,7,9,12,12]    3.59e-3 [7,7,9,12,12]    3.83e-3 [7,7,9,12,12]
#                     4.1e-14                  4.5e-13                  4.5e-14                  2.4e-13
#    The hybrid histories flatten at the noise level after one or two steps at 1537 x 24577, so a column stops
#    there at once or never.  ban at 1537 x 24577: the tolerance 8.72e-4 ([9,10,12,12,12]) has spread 1.2e-12 and
#    the oracle, which forms the 24577^2 B*A, takes 0.5 s a run, so 3.0e-3 it is.  The two cases marked * stay
#    above 1e-12 at every tolerance tried (the columns that run all 12 iterations carry it: x spreads by 1.1e-12
#    whatever lambda is in 1e-5 .. 1e-1, H by 5e-13): they are judged at their envelope, not moved.
# ---------------------------------------------------------------------------------------------
BATCH_TOL = {(SHAPES[0], "ab", True): 1.91e-2, (SHAPES[0], "ba", True): 1.91e-2,
             (SHAPES[0], "ab", False): 8.06e-4, (SHAPES[0], "ba", False): 3.0e-3,
             (SHAPES[1], "ab", True): 4.47e-3, (SHAPES[1], "ba", True): 4.67e-3,
             (SHAPES[1], "ab", False): 4.47e-3, (SHAPES[1], "ba", False): 4.67e-3,
             (SHAPES[2], "ab", True): 4.32e-3, (SHAPES[2], "ba", True): 3.89e-3,
             (SHAPES[2], "ab", False): 3.59e-3, (SHAPES[2], "ba", False): 3.83e-3}
ENVELOPED = {("batch", SHAPES[0], "ba", True), ("batch", SHAPES[1], "ba", True),
             ("mismatch", SHAPES[0], "ba", True), ("sweep", SHAPES[0], "ba")}


def _bounds_run(side, hybrid, b, xt, tol, lam, maxit=MAXIT):
    def run(AA, BB):
        return _bounds_sol(ORACLE[(side, hybrid)](AA, BB, b, xt, tol, maxit, *((lam,) if hybrid else ()),
                                                  return_H=True))
    return run


@functools.lru_cache(maxsize=None)
def _oracle_batch(shape, side, hybrid):
    """The oracle once per column at the case's tolerance (computed once), the conditions on its own result,
    and the envelopes of an ENVELOPED case."""
    A, B, _, xt = _problem(*shape)
    Bm, tol = _rhs(shape), BATCH_TOL[shape, side, hybrid]
    runs = [_bounds_run(side, hybrid, Bm[:, j], xt, tol, LAMS[j]) for j in range(NRHS)]
    ref = [run(A, B) for run in runs]
    margin = _spread_ok([r["k"] for r in ref], [r["hists"]["res"] for r in ref], tol)
    bars, spread = [None] * NRHS, None
    if ("batch", shape, side, hybrid) in ENVELOPED:
        env = [_gm_envelope(run, A, B, explicit=(side, hybrid) == ("ba", False)) for run in runs]
        bars, spread = [e[0] for e in env], max(e[1] for e in env)
    return ref, bars, spread, margin


@gpu
@pytest.mark.parametrize("side,hybrid", CASES, ids=[case_id(c) for c in CASES])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_batch_matches_oracle_at_length(gpu_ctx, shape, side, hybrid):
    A, B, _, xt = _problem(*shape)
    ref, bars, spread, margin = _oracle_batch(shape, side, hybrid)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        Rb = hgmres.gmres_bounds_batch(Ao, Bo, _rhs(shape), xt, BATCH_TOL[shape, side, hybrid], MAXIT, side,
                                       lambdas=LAMS if hybrid else None, ctx=gpu_ctx, return_H=True)
    assert np.all(Rb.status == 0)
    assert [int(k) for k in Rb.niters] == [r["k"] for r in ref], (Rb.niters, [r["k"] for r in ref])
    devs = [_sol_ok(_batch_col(Rb, j), ref[j], bars[j], (shape, side, hybrid, j)) for j in range(NRHS)]
    _report(f"batch {case_id((side, hybrid))} {ids(shape)} niters {[r['k'] for r in ref]} margin {margin:.3f}", devs,
            spread)


# ---------------------------------------------------------------------------------------------
# 2. bitwise composition where the per-column workspace matters
#    Past MGS1_MAX mgs() runs the one-reduction sweep, which keeps its Gram triangle (mgs1_G / mgs1_h / mgs1_pr)
#    in the context's workspace from step to step: lockstep_core gives every column workspace names of its own.
#    9 columns (groups of 8 + 1), tolerances at which the oracle's columns stop at [1,1,2,12 x 6] (1537 x 24577,
#    both hybrid sides), [6,6,6,6,8,12 x 4] (24577 x 1537 abn) and [7,7,7,7,9,12 x 4] (32769^2 ban); the spread is
#    asserted on the device's own result.
# ---------------------------------------------------------------------------------------------
COMPOSE = {"bap-1537x24577": (SHAPES[0], "ba", True, 1.91e-2, {}, {}),
           "abn-24577x1537": (SHAPES[1], "ab", False, 4.47e-3, {}, {}),
           "ban-32769x32769": (SHAPES[2], "ba", False, 3.83e-3, {}, {}),
           "bap-1537x24577-mgs_form0": (SHAPES[0], "ba", True, 1.91e-2, dict(mgs_form=0), {}),
           "bap-1537x24577-cgs2": (SHAPES[0], "ba", True, 1.91e-2, {}, dict(orth="cgs2")),
           "abp-1537x24577-mgs_single0": (SHAPES[0], "ab", True, 1.91e-2, dict(mgs_single=0), {})}


@gpu
@pytest.mark.parametrize("name", list(COMPOSE))
def test_batch_composition_at_length(gpu_ctx, name):
    """The batch equals each of its 9 columns run alone, and itself repeated after an unrelated batch (other
    right-hand sides, 4 columns, 7 iterations) on the same context: columns overwriting one another's MGS
    workspace, or state left over from an earlier solve, change the bits.  The default options at the two
    non-square shapes also against the library's single solvers at 1e-10."""
    shape, side, hybrid, tol, opts, kw = COMPOSE[name]
    A, B, _, xt = _problem(*shape)
    Bm = _rhs(shape, NCOMP, 11)
    other = _rhs(shape, 4, 5)
    kw = dict(kw, ctx=gpu_ctx, return_H=True)

    def batch(cols, rhs=Bm, maxit=MAXIT, lams=LAMS9):
        return hgmres.gmres_bounds_batch(Ao, Bo, rhs[:, cols], xt, tol, maxit, side,
                                         lambdas=lams[cols] if hybrid else None, **kw)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo), gpu_ctx.options(**opts):
        Rb = batch(slice(None))
        assert len(set(Rb.niters)) >= 2 and min(Rb.niters) < MAXIT and max(Rb.niters) == MAXIT, Rb.niters
        assert np.all(Rb.status == 0) and np.all(np.isfinite(Rb.x))
        for j in range(NCOMP):
            same_batch(Rb, batch([j]), [j], [0])
        Ro = batch(slice(None), rhs=other, maxit=7, lams=LAMS9[::-1][:4])
        assert np.all(np.isfinite(Ro.x))
        same_batch(Rb, batch(slice(None)))
        if not opts and not kw.get("orth") and shape != SHAPES[2]:
            worst = 0.0
            for j in range(NCOMP):
                o = SINGLE[(side, hybrid)](Ao, Bo, Bm[:, j], xt, tol, MAXIT, *((LAMS9[j],) if hybrid else ()),
                                           ctx=gpu_ctx, return_H=True)
                d = _sol_ok(_batch_col(Rb, j), _sol(o[0], o[3], o[-1], err=o[1], res=o[2]), None, (name, "single", j))
                worst = max(worst, max(d.values()))
            print(f"[lockstep compose {name}] niters {[int(k) for k in Rb.niters]}; "
                  f"largest deviation from the single solver {worst:.1e}")


# ---------------------------------------------------------------------------------------------
# 3. mismatch sweeps at length
#    B0 = A', coefficients [0, 1e-3, 1e-2, 3e-2, 1e-1], b and x_true of the shape's blur problem, lambdas LAMS,
#    12 iterations, tol = 0.  E "same": B0's pattern, values B0.data * N(0, 1); "own": the pattern of the blur of
#    half-width 3, values mean|B0.data| * N(0, 1).  Oracle spread (8 seeds; largest over the five levels and over
#    H, x and both histories), measured on the CPU:
#                              abp      bap        abn      ban
#      1537 x 24577  same   3.5e-14  3.2e-12 *  3.5e-14  8.9e-13
#                    own    4.7e-14  2.6e-12 *  4.7e-14  8.9e-13
#      24577 x 1537  same   1.3e-13  9.9e-13    4.2e-14  9.0e-13
#                    own    1.7e-13  6.1e-13    3.7e-14  4.9e-13
#    * judged at the envelope (the same 12-iteration BA runs as the cases marked in section 1).
#    The Arnoldi alone (k = 8, c = 0, BA side of 1537 x 24577): H spreads by 4e-13 (in its last column).
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mismatch_E(shape, variant):
    _, B0, _, _ = _problem(*shape)
    if variant == "same":
        v = B0.data * np.random.default_rng(31).standard_normal(B0.nnz)
        E = sp.csr_matrix((v, B0.indices.copy(), B0.indptr.copy()), shape=B0.shape)
    else:
        P = blur_problem(shape[0], shape[1], half=3)[1]
        assert P.shape == B0.shape and P.nnz < B0.nnz
        v = np.mean(np.abs(B0.data)) * np.random.default_rng(32).standard_normal(P.nnz)
        E = sp.csr_matrix((v, P.indices.copy(), P.indptr.copy()), shape=P.shape)
    E.sort_indices()
    return E


@functools.lru_cache(maxsize=None)
def _mismatch_B(shape, variant):
    _, B0, _, _ = _problem(*shape)
    E = _mismatch_E(shape, variant)
    out = []
    for c in MISMATCH_COEFS:
        Bc = sp.csr_matrix(B0 + c * E)
        Bc.sort_indices()
        out.append(Bc)
    return out


@gpu
@pytest.mark.parametrize("side,hybrid", CASES, ids=[case_id(c) for c in CASES])
@pytest.mark.parametrize("variant", ["same", "own"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=ids)
def test_mismatch_matches_oracle_at_length(gpu_ctx, shape, variant, side, hybrid):
    """gmres_bounds_mismatch against the oracle's solver on the explicit B0 + c E, level by level; the c = 0
    level bitwise equal to the gmres_bounds_batch column for the same b; E on B0's pattern bitwise the same
    through the general kernel (pert_shared = 0)."""
    A, B0, b, xt = _problem(*shape)
    E, Bc = _mismatch_E(shape, variant), _mismatch_B(shape, variant)
    runs = [_bounds_run(side, hybrid, b, xt, 0.0, LAMS[j]) for j in range(NRHS)]
    ref = [run(A, Bc[j]) for j, run in enumerate(runs)]
    bars, spread = [None] * NRHS, None
    if ("mismatch", shape, side, hybrid) in ENVELOPED:
        env = [_gm_envelope(run, A, Bc[j]) for j, run in enumerate(runs)]
        bars, spread = [e[0] for e in env], max(e[1] for e in env)
    lam = LAMS if hybrid else None
    kw = dict(ctx=gpu_ctx, return_H=True)
    with _device_ops(gpu_ctx, A, B0) as (Ao, Bo):
        Eo = hgmres.SparseOperator.from_scipy(E, gpu_ctx)
        try:
            Rm = hgmres.gmres_bounds_mismatch(Ao, Bo, Eo, MISMATCH_COEFS, b, xt, 0.0, MAXIT, side, lambdas=lam, **kw)
            R0 = hgmres.gmres_bounds_batch(Ao, Bo, b[:, None], xt, 0.0, MAXIT, side,
                                           lambdas=LAMS[:1] if hybrid else None, **kw)
            if variant == "same":
                with gpu_ctx.options(pert_shared=0):
                    Rg = hgmres.gmres_bounds_mismatch(Ao, Bo, Eo, MISMATCH_COEFS, b, xt, 0.0, MAXIT, side, lambdas=lam,
                                                      **kw)
        finally:
            Eo.close()
    assert np.all(Rm.status == 0) and np.all(Rm.niters == MAXIT)
    devs = [_sol_ok(_batch_col(Rm, j), ref[j], bars[j], (shape, variant, side, hybrid, j)) for j in range(NRHS)]
    _report(f"mismatch {case_id((side, hybrid))} {variant} {ids(shape)}", devs, spread)
    same_batch(Rm, R0, [0], [0])
    if variant == "same":
        same_batch(Rm, Rg)


@gpu
@pytest.mark.parametrize("variant", ["same", "own"])
@pytest.mark.parametrize("shape,side", [(SHAPES[0], "ba"), (SHAPES[1], "ab")], ids=["ba-1537x24577", "ab-24577x1537"])
def test_arnoldi_mismatch_at_length(gpu_ctx, shape, side, variant):
    """The lockstep GCV Arnoldi, 8 steps, against R.arnoldi on the explicit B0 + c E per level: H at 1e-10 of
    max|H|, beta at 1e-13, kdone equal."""
    A, B0, b, _ = _problem(*shape)
    E, Bc = _mismatch_E(shape, variant), _mismatch_B(shape, variant)
    with _device_ops(gpu_ctx, A, B0) as (Ao, Bo):
        Eo = hgmres.SparseOperator.from_scipy(E, gpu_ctx)
        try:
            H, beta, kd = hgmres.arnoldi_mismatch(Ao, Bo, Eo, MISMATCH_COEFS, b, ARNOLDI_K, side, ctx=gpu_ctx)
        finally:
            Eo.close()
    assert H.shape == (NRHS, ARNOLDI_K + 1, ARNOLDI_K)
    worst = [0.0, 0.0]
    for j in range(NRHS):
        Hr, br = R.arnoldi(A, Bc[j], b, ARNOLDI_K, side)
        assert kd[j] == _kdone(Hr) == ARNOLDI_K, (j, kd[j])
        H_ok(H[j], Hr, TOL)
        assert abs(beta[j] - br) <= 1e-13 * br, (j, abs(beta[j] - br) / br)
        worst = [max(worst[0], float(np.max(np.abs(H[j] - Hr)) / np.max(np.abs(Hr)))), max(worst[1], abs(beta[j] - br) / br)]
    print(f"[lockstep arnoldi_mismatch {side} {variant} {ids(shape)}] |dH| {worst[0]:.1e} |dbeta| {worst[1]:.1e}")


# ---------------------------------------------------------------------------------------------
# 4. gk_batch at length
#    5 columns (LEVELS, LAMS), 12 iterations, each column judged by _gkb_check: max(1e-10, 100 x the oracle's spread
#    over 8 seeds), and every entry's envelope must lie under GKB_CAP.  Tolerances picked as in section 1; oracle
#    niters and spread (largest over the columns, x and the histories), measured on the CPU:
#                         lsqr                     lsmr                     hybrid_lsqr              hybrid_lsmr
#      1537 x 24577   8.06e-4 [9,10,12,12,12]  8.72e-4 [9,10,12,12,12]  1.59e-3 [6,7,12,12,12]   7.02e-2 [1,1,1,1,12]
#                     5.8e-14                  1.9e-13                  4.9e-14                  2.1e-14
#      24577 x 1537   4.47e-3 [6,6,8,12,12]    4.67e-3 [6,6,8,12,12]    4.47e-3 [6,6,8,12,12]    6.42e-2 [1,1,1,1,12]
#                     5.7e-15                  2.3e-14                  5.7e-15                  1.8e-13
#      32769 x 32769  3.59e-3 [7,7,9,12,12]    3.83e-3 [7,7,9,12,12]    3.60e-3 [7,7,9,12,12]    5.72e-2 [1,1,1,1,12]
#                     1.6e-14                  1.9e-14                  8.6e-15                  1.2e-13
#    The oracle's hybrid_lsmr residuals rise after the first iteration on these problems for every lambda in
#    1e-6 .. 1e-2 (at LAMS: 1.6e-2, 6.0e-2, 6.4e-2, ... in the first column of 1537 x 24577), so its columns stop
#    at iteration 1 or never; the spread stays ~1e-13 at LAMS, so LAMS it is for the hybrid kinds too.
# ---------------------------------------------------------------------------------------------
GK_TOL = {(SHAPES[0], "lsqr"): 8.06e-4, (SHAPES[0], "lsmr"): 8.72e-4, (SHAPES[0], "hybrid_lsqr"): 1.59e-3,
          (SHAPES[0], "hybrid_lsmr"): 7.02e-2,
          (SHAPES[1], "lsqr"): 4.47e-3, (SHAPES[1], "lsmr"): 4.67e-3, (SHAPES[1], "hybrid_lsqr"): 4.47e-3,
          (SHAPES[1], "hybrid_lsmr"): 6.42e-2,
          (SHAPES[2], "lsqr"): 3.59e-3, (SHAPES[2], "lsmr"): 3.83e-3, (SHAPES[2], "hybrid_lsqr"): 3.60e-3,
          (SHAPES[2], "hybrid_lsmr"): 5.72e-2}


class _Memo:
    """An oracle `fn(A)` that remembers its results: the exact operator, and each seed of the rounding model (a
    fresh _Rounded is known by its generator's state), so that the envelope and _gkb_check share the runs."""

    def __init__(self, fn):
        self.fn, self.cache = fn, {}

    def __call__(self, AA):
        key = repr(AA.rng.bit_generator.state) if isinstance(AA, _Rounded) else "exact"
        if key not in self.cache:
            self.cache[key] = self.fn(AA)
        return self.cache[key]


def _gk_fn(kind, b, xt, tol, maxit, lam):
    fn, hybrid = KINDS[kind][1], KINDS[kind][3]
    return _Memo(lambda AA: fn(AA, b, xt, tol, maxit, *((lam,) if hybrid else ())))


@functools.lru_cache(maxsize=None)
def _oracle_gk(shape, kind):
    """Per column: the memoised oracle at the case's tolerance.  Asserts the conditions on the oracle's own
    result: the niters spread, the 2 % margins, and x and every history entry judged under the cap."""
    A, _, _, xt = _problem(*shape)
    Bm, tol = _rhs(shape), GK_TOL[shape, kind]
    fns = [_gk_fn(kind, Bm[:, j], xt, tol, MAXIT, LAMS[j]) for j in range(NRHS)]
    ref = [fn(A) for fn in fns]
    margin = _spread_ok([r[-1] for r in ref], [r[2] for r in ref], tol)
    for j, fn in enumerate(fns):
        tx, th = _envelope(fn, A, NHIST[kind])
        assert tx <= GKB_CAP and all(np.all(t <= GKB_CAP) for t in th), (shape, kind, j, "envelope past the cap")
    return fns, ref, margin


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gk_batch_matches_oracle_at_length(gpu_ctx, shape, kind):
    A, B, _, xt = _problem(*shape)
    fns, ref, margin = _oracle_gk(shape, kind)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        Rb = hgmres.gk_batch(Ao, _rhs(shape), xt, GK_TOL[shape, kind], MAXIT, kind,
                             lambdas=LAMS if KINDS[kind][3] else None, At=Bo, ctx=gpu_ctx)
    assert [int(k) for k in Rb.niters] == [r[-1] for r in ref], (Rb.niters, [r[-1] for r in ref])
    print(f"[lockstep gk_batch {kind} {ids(shape)}] niters {[r[-1] for r in ref]} margin {margin:.3f}")
    for j in range(NRHS):
        k = ref[j][-1]
        _gkb_check(fns[j], A, _hists(Rb, kind, j), nhist=NHIST[kind], label=f"lockstep gk_batch {kind} {ids(shape)} col {j}")
        for h in (Rb.error_norm, Rb.residual_norm) + ((Rb.ar_norm,) if kind == "lsmr" else ()):
            assert np.all(np.isnan(h[k:, j])) and np.all(np.isfinite(h[:k, j]))


# 9 columns, tolerances at which the oracle's columns stop at [9,9,10,12 x 6] (lsqr), [1,1,1,12 x 6] (hybrid_lsmr),
# [6,6,6,6,8,12 x 4] (lsmr, hybrid_lsqr): 9 -> 8 or fewer running columns re-gathers 8 + 1 into one group
GK_COMPOSE = [("lsqr", SHAPES[0], 8.06e-4), ("hybrid_lsmr", SHAPES[0], 2.3e-2), ("lsmr", SHAPES[1], 4.67e-3),
              ("hybrid_lsqr", SHAPES[1], 4.47e-3)]


@gpu
@pytest.mark.parametrize("kind,shape,tol", GK_COMPOSE, ids=[f"{k}-{ids(s)}" for k, s, _ in GK_COMPOSE])
def test_gk_batch_composition_at_length(gpu_ctx, kind, shape, tol):
    A, B, _, xt = _problem(*shape)
    Bm = _rhs(shape, NCOMP, 11)
    hybrid = KINDS[kind][3]
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        run = lambda cols: hgmres.gk_batch(Ao, Bm[:, cols], xt, tol, MAXIT, kind,   # noqa: E731
                                           lambdas=LAMS9[cols] if hybrid else None, At=Bo, ctx=gpu_ctx)
        Rb = run(slice(None))
        # a column left while others ran on: the 8 + 1 groups were re-gathered into a narrower layout
        assert min(Rb.niters) < MAXIT and max(Rb.niters) > min(Rb.niters), Rb.niters
        assert np.all(np.isfinite(Rb.x))
        for j in range(NCOMP):
            same_gk(Rb, run([j]), [j], [0])
    print(f"[lockstep gk compose {kind} {ids(shape)}] niters {[int(k) for k in Rb.niters]}")


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", CAP_SHAPES, ids=ids)
def test_gk_batch_past_the_grid_stride_cap(gpu_ctx, shape, kind):
    """262,401 rows or pixels (half = 2 keeps the operator at ~1 M entries): every thread of the vector kernels
    on that space strides over more than one row.  3 columns, 4 iterations, tol = 0, one call with a shared
    x_true (MVS_DIFF_SHARED) and one with a column of its own for column 1 (MVS_DIFF).  Each column against the
    oracle by _gkb_check (oracle spread over the four kinds: <= 9e-14, so every entry is judged at the 1e-10
    floor); the batch equals its columns alone, bit for bit."""
    A, B, _, xt = blur_problem(*shape, half=2)
    Bm = noisy_rhs(A @ xt, LEVELS[[0, 2, 4]])
    hybrid, nh = KINDS[kind][3], NHIST[kind]
    lam = LAMS[:3] if hybrid else None
    xt2 = xt[::-1].copy()
    XT = np.stack([xt, xt2, xt], axis=1)
    kw = dict(At=None, ctx=gpu_ctx)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        kw["At"] = Bo
        Rs = hgmres.gk_batch(Ao, Bm, xt, 0.0, 4, kind, lambdas=lam, **kw)
        Rp = hgmres.gk_batch(Ao, Bm, XT, 0.0, 4, kind, lambdas=lam, **kw)
        alone = [hgmres.gk_batch(Ao, Bm[:, [j]], xt, 0.0, 4, kind, lambdas=None if lam is None else lam[[j]], **kw)
                 for j in range(3)]
        alone2 = hgmres.gk_batch(Ao, Bm[:, [1]], xt2[:, None], 0.0, 4, kind, lambdas=None if lam is None else lam[[1]], **kw)
    assert np.all(Rs.niters == 4) and np.all(Rp.niters == 4)
    def judged(fn, out, label):
        tx, th = _envelope(fn, A, nh)
        assert tx <= GKB_CAP and all(np.all(t <= GKB_CAP) for t in th), (label, "envelope past the cap")
        _gkb_check(fn, A, out, nhist=nh, label=label)
    for j in range(3):
        judged(_gk_fn(kind, Bm[:, j], xt, 0.0, 4, LAMS[j]), _hists(Rs, kind, j), f"lockstep cap {kind} {ids(shape)} col {j}")
        same_gk(Rs, alone[j], [j], [0])
    same_gk(Rs, Rp, err=False)
    same_gk(Rs, Rp, [0, 2], [0, 2])                         # the same x_true through MVS_DIFF: the same bits
    judged(_gk_fn(kind, Bm[:, 1], xt2, 0.0, 4, LAMS[1]), _hists(Rp, kind, 1),
           f"lockstep cap {kind} {ids(shape)} col 1, own x_true")
    same_gk(Rp, alone2, [1], [0])
    assert not np.array_equal(Rp.error_norm[:, 1], Rs.error_norm[:, 1])


# ---------------------------------------------------------------------------------------------
# 5. across step 120 in lockstep
# ---------------------------------------------------------------------------------------------
LONG_TAGS = {"ban": ("ba", False), "bap": ("ba", True), "abn": ("ab", False), "abp": ("ab", True)}


@gpu
@pytest.mark.parametrize("tag", list(LONG_TAGS))
def test_lockstep_across_step_120(gpu_ctx, tag):
    """4097^2 under mgs_single = 0, budget 124, tol = 0, 3 columns: each column's one-reduction sweep hands over
    to the pass form at step MGS1_MAXC = 120, with its own basis and Gram triangle.  Columns 0 and 2 carry
    _problem's b (and LAM): bitwise equal, and each inside test_gpu_lengths._long_envelope (100 x the oracle's
    spread, every entry from 118 on judged under the cap).  Column 1, another right-hand side and lambda
    between them, only has to be finite."""
    side, hybrid = LONG_TAGS[tag]
    A, B, b, xt = _problem(*LONG)
    ref, tol, _ = _long_envelope(LONG, tag)
    Bm = np.stack([b, _rhs(LONG)[:, 3], b], axis=1)
    lam = np.array([LAM, 3.0 * LAM, LAM]) if hybrid else None
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo), gpu_ctx.options(mgs_single=0):
        Rb = hgmres.gmres_bounds_batch(Ao, Bo, Bm, xt, 0.0, LONG_BUDGET, side, lambdas=lam, ctx=gpu_ctx, return_H=True)
    assert np.all(Rb.status == 0) and np.all(Rb.niters == LONG_BUDGET)
    same_batch(Rb, Rb, [0], [2])
    for j in (0, 2):
        out = (Rb.x[:, j], Rb.error_norm[:, j], Rb.residual_norm[:, j], int(Rb.niters[j]), Rb.H[j])
        _long_check(out, ref, tol, LONG_BUDGET, ("H", "x", "err", "res"), f"lockstep {tag} {ids(LONG)} col {j}")
    assert np.all(np.isfinite(Rb.x[:, 1])) and np.all(np.isfinite(Rb.H[1]))
    assert np.all(np.isfinite(Rb.residual_norm[:, 1])) and np.all(np.isfinite(Rb.error_norm[:, 1]))
    assert not np.array_equal(Rb.x[:, 1], Rb.x[:, 0])


# ---------------------------------------------------------------------------------------------
# 6. the lambda sweep at length
#    6 lambdas logspace(-4, -1, 6), 12 iterations, tol = 0, b of the shape's blur problem.  Oracle spread (8 seeds,
#    per lambda, largest over H, x and the three histories), measured on the CPU:
#      1537 x 24577 ba   9.5e-13 1.0e-12 1.1e-12 1.1e-12 1.1e-12 1.1e-12   (enveloped)
#      24577 x 1537 ab   1.2e-13 8.2e-14 9.1e-14 3.6e-14 1.5e-14 1.3e-14
#    Below lambda = 1e-4 the residual history's spread grows (4e-12 at 1e-5 on the BA side): not run.
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape,side", [(SHAPES[0], "ba"), (SHAPES[1], "ab")], ids=["ba-1537x24577", "ab-24577x1537"])
def test_lambda_sweep_at_length(gpu_ctx, shape, side):
    """gmres_lambda_sweep against the oracle's loop over the lambdas (test_gpu_sweep._oracle_sweep): x, the error,
    residual and ||x_k|| surfaces and H, at the bar of section 1."""
    A, B, b, xt = _problem(*shape)

    def run(lam):
        def one(AA, BB):
            x, e, r, k, sol, H = _oracle_sweep(AA, BB, b, xt, 0.0, side, lambdas=[lam], maxit=MAXIT)[0]
            return _sol(x, k, H, err=e, res=r, sol=sol)
        return one
    ref = [run(lam)(A, B) for lam in SWEEP_LAMS]
    bars, spread = [None] * SWEEP_LAMS.size, None
    if ("sweep", shape, side) in ENVELOPED:
        env = [_gm_envelope(run(lam), A, B) for lam in SWEEP_LAMS]
        bars, spread = [e[0] for e in env], max(e[1] for e in env)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        S = hgmres.gmres_lambda_sweep(Ao, Bo, b, xt, 0.0, MAXIT, SWEEP_LAMS, side, ctx=gpu_ctx, return_x=True,
                                      return_H=True)
    assert S.ksteps == MAXIT and np.all(S.niters == MAXIT)
    devs = [_sol_ok(_sol(S.X[:, l], S.niters[l], S.H, err=S.err[:, l], res=S.res[:, l], sol=S.sol[:, l]), ref[l], bars[l],
                    (shape, side, l)) for l in range(SWEEP_LAMS.size)]
    _report(f"sweep {side} {ids(shape)}", devs, spread)


# ---------------------------------------------------------------------------------------------
# the oracle-only conditions of sections 1 and 4, without a device
# ---------------------------------------------------------------------------------------------
def test_oracle_conditions_on_the_non_square_shapes():
    """What sections 1 and 4 require of the oracle alone, on the two non-square shapes: at every tolerance of
    BATCH_TOL and GK_TOL the columns' niters spread (two distinct values, one below 12), every deciding residual
    lies 2 % or more from the tolerance, the envelopes of the ENVELOPED cases and every Golub-Kahan envelope stay
    under GKB_CAP.  (32769^2 is asserted by the GPU tests through the same two functions, which keep their results.  27 s of
    oracle runs on 8 CPU cores, most of them the 8-seed Golub-Kahan envelopes.)"""
    for shape in SHAPES[:2]:
        for side, hybrid in CASES:
            ref, bars, spread, margin = _oracle_batch(shape, side, hybrid)
            assert (spread is not None) == (("batch", shape, side, hybrid) in ENVELOPED)
            print(f"[lockstep oracle batch {case_id((side, hybrid))} {ids(shape)}] niters {[r['k'] for r in ref]} "
                  f"margin {margin:.3f}" + (f" spread {spread:.1e}" if spread is not None else ""))
        for kind in KINDS:
            _, ref, margin = _oracle_gk(shape, kind)
            print(f"[lockstep oracle gk {kind} {ids(shape)}] niters {[r[-1] for r in ref]} margin {margin:.3f}")
