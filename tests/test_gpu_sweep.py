"""The lambda sweep of the hybrid PTR solvers (hgm_gmres_bounds_sweep) and its monitor kernel
(hgm_proj_norms, csrc/sweep.hip), on the device.

* the kernel against numpy, with a bound computed from the forward error of a length-k dot product;
* the sweep against the oracle's ``{AB,BA}gmres_hybrid_bounds`` called once per lambda (the loop of
  analyze_regularization.m:22-33 / plot_error_surface.m:28-42), at the project's bar 1e-10;
* the sweep against the device's own single-lambda solver;
* a tiled operator pair (the one-pass A*(B*q) route, pixel-order handling of X) and CGS2;
* refusals and breakdown; the analysis pipeline on top.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, golden_problem
import hgmres
from hgmres import _lib as L
from hgmres import analysis
from hgmres.problems import tomo_problem
from oracle import restatement as R   # checker only

pytestmark = pytest.mark.gpu

TOL = 1e-10
EPS = np.finfo(np.float64).eps
LAMBDAS = np.logspace(-2, 5, 15)
MAXIT = 12
FIXTURES = ("tomo24_matched.npz", "tomo24_pixel.npz")
ORACLE = {"ab": R.ABgmres_hybrid_bounds, "ba": R.BAgmres_hybrid_bounds}
SINGLE = {"ab": hgmres.ABgmres_hybrid_bounds, "ba": hgmres.BAgmres_hybrid_bounds}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def hist_ok(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    both_nan = np.isnan(a) & np.isnan(b)
    d = np.abs(a - b)[~both_nan]
    s = np.maximum(np.abs(b), 1e-300)[~both_nan]
    assert np.all(d <= tol * s + 1e-300), (d / s).max()


def H_ok(Hg, Hr, tol=TOL):
    assert np.max(np.abs(Hg - Hr)) <= tol * np.max(np.abs(Hr)), np.max(np.abs(Hg - Hr)) / np.max(np.abs(Hr))


# ---------------------------------------------------------------------------------------------
# 1. kernel against numpy
# ---------------------------------------------------------------------------------------------
ROWS = (1, 15, 16, 17, 1000, 70001)
KS = (1, 3, 4, 5, 32, 33)
LS = (1, 15, 16, 17, 100, 300)


def _kernel_cases():
    """A sample of the product rows x k x L x (ldv padding) x (t given): three rotations of the axes,
    so every value of each axis appears (three times), with both paddings and both t settings."""
    cases = []
    for rot in range(3):
        for i in range(6):
            j = len(cases)
            cases.append((ROWS[i], KS[(i + rot) % 6], LS[(i + 2 * rot + 1) % 6], 6 * (j % 2), (j // 2) % 2 == 0))
    return cases


def _padded(Vd, pad):
    """Vd as a column-major view with leading dimension rows + pad, the padding rows NaN."""
    rows, k = Vd.shape
    buf = np.full((rows + pad, k), np.nan, order="F")
    buf[:rows, :] = Vd
    return buf[:rows, :]


def _check_norms(V, Y, t, got_d, got_s):
    """|got - ref| <= 8 (k + 4) eps sum_i g_il^2 with g_il = sum_j |V_ij||Y_jl| + |t_i|: the forward error
    of the length-k dot product (k eps g), the subtraction, the square (a factor 2) and the row sum."""
    k = V.shape[1]
    P = V @ Y
    G = np.abs(V) @ np.abs(Y)
    tt = np.zeros(V.shape[0]) if t is None else t
    # (the row sums in extended precision: numpy adds the rows of a C-ordered array one after the other,
    # and 70 001 sequential fp64 additions would put tens of eps of the REFERENCE's own error into the check)
    ref_d = np.sum((P - tt[:, None]) ** 2, axis=0, dtype=np.longdouble).astype(np.float64)
    ref_s = np.sum(P ** 2, axis=0, dtype=np.longdouble).astype(np.float64)
    bd = 8 * (k + 4) * EPS * np.sum((G + np.abs(tt)[:, None]) ** 2, axis=0)
    bs = 8 * (k + 4) * EPS * np.sum(G ** 2, axis=0)
    ed, es = np.abs(got_d - ref_d), np.abs(got_s - ref_s)
    print(f"proj_norms rows={V.shape[0]} k={k} L={Y.shape[1]}: max err/bound d {np.max(ed / bd):.3g} "
          f"s {np.max(es / bs):.3g}")
    assert np.all(np.isfinite(got_d)) and np.all(np.isfinite(got_s))
    assert np.all(ed <= bd), np.max(ed / bd)
    assert np.all(es <= bs), np.max(es / bs)


@pytest.mark.parametrize("rows,k,nl,pad,with_t", _kernel_cases())
def test_proj_norms_against_numpy(gpu_ctx, rows, k, nl, pad, with_t):
    rng = np.random.default_rng(1000 * k + nl + rows)
    V = rng.standard_normal((rows, k))
    Y = rng.standard_normal((k, nl))
    t = rng.standard_normal(rows) if with_t else None
    d, s = hgmres.proj_norms(_padded(V, pad), Y, t, ctx=gpu_ctx)
    _check_norms(V, Y, t, d, s)
    if not with_t:
        assert np.array_equal(d, s)


def test_proj_norms_axes_covered():
    cases = _kernel_cases()
    assert {c[0] for c in cases} == set(ROWS) and {c[1] for c in cases} == set(KS) and {c[2] for c in cases} == set(LS)
    assert {c[3] for c in cases} == {0, 6} and {c[4] for c in cases} == {True, False}
    assert {(c[3], c[4]) for c in cases} == {(0, True), (6, True), (0, False), (6, False)}


def test_proj_norms_long_basis(gpu_ctx):
    """k > 64: the kernel variant that re-reads the operands per column block (k = 70, 130)."""
    rng = np.random.default_rng(7)
    for k in (70, 130):
        V = rng.standard_normal((333, k))
        Y = rng.standard_normal((k, 37))
        t = rng.standard_normal(333)
        d, s = hgmres.proj_norms(_padded(V, 6), Y, t, ctx=gpu_ctx)
        _check_norms(V, Y, t, d, s)


def test_proj_norms_loop_yardstick_agrees(gpu_ctx):
    """hgm_proj_norms_loop (the solvers' own single-coefficient monitor, once per column: the yardstick of
    scripts/sweep_micro.py) meets the same bound."""
    rng = np.random.default_rng(11)
    V, Y, t = rng.standard_normal((1001, 5)), rng.standard_normal((5, 17)), rng.standard_normal(1001)
    d, s = hgmres.proj_norms(_padded(V, 5), Y, t, ctx=gpu_ctx)
    dl, none = hgmres.proj_norms(_padded(V, 5), Y, t, ctx=gpu_ctx, loop=True)
    assert none is None
    _check_norms(V, Y, t, d, s)
    _check_norms(V, Y, t, dl, s)
    with pytest.raises(ValueError):
        hgmres.proj_norms(V, Y, None, ctx=gpu_ctx, loop=True)        # t is required there


def test_proj_norms_cancellation_and_bitwise(gpu_ctx):
    """Coefficients of magnitude 1e8 that cancel to O(1) (late PTR iterations on shaw): the same bound
    (it scales with |V||Y|), and two runs give the same bits (fixed summation order, no atomics)."""
    rng = np.random.default_rng(3)
    rows, k, nl = 1000, 6, 20
    u = rng.standard_normal((rows, k // 2))
    w = rng.standard_normal((rows, k // 2))
    V = np.hstack([u, u + 1e-8 * w])                       # nearly dependent column pairs
    a = rng.standard_normal((k // 2, nl))
    Y = 1e8 * np.vstack([a, -a])                           # V Y = -w a: O(1) from O(1e8) terms
    t = rng.standard_normal(rows)
    assert np.abs(Y).min() > 1e5 and np.abs(V @ Y).max() < 1e2
    d1, s1 = hgmres.proj_norms(V, Y, t, ctx=gpu_ctx)
    d2, s2 = hgmres.proj_norms(V, Y, t, ctx=gpu_ctx)
    _check_norms(V, Y, t, d1, s1)
    assert d1.tobytes() == d2.tobytes() and s1.tobytes() == s2.tobytes()


# ---------------------------------------------------------------------------------------------
# 2. solver against the oracle, 24^2 fixtures
# ---------------------------------------------------------------------------------------------
def _oracle_sweep(A, B, b, xt, tol, side, lambdas=LAMBDAS, maxit=MAXIT):
    """The reference's loop: one oracle solve per lambda.  Per lambda: x, err, res, niters, ||x_k|| of
    every iterate (re-formed from the oracle's own Q and H by its projected solve), H."""
    out = []
    for lam in lambdas:
        x, e, r, k, H, Q = ORACLE[side](A, B, b, xt, tol, maxit, lam, return_H=True, return_Q=True)
        beta = np.linalg.norm(b if side == "ab" else B @ b)
        sol = np.zeros(k)
        for kk in range(1, k + 1):
            Hk = H[: kk + 1, :kk]
            tk = np.zeros(kk + 1)
            tk[0] = beta
            yk = R.mldivide(Hk.T @ Hk + lam * np.eye(kk), Hk.T @ tk)
            zk = Q[:, :kk] @ yk
            sol[kk - 1] = np.linalg.norm(B @ zk if side == "ab" else zk)
        assert rel(B @ zk if side == "ab" else zk, x) <= 1e-13     # the re-formed last iterate is x
        out.append((x, e, r, k, sol, H))
    return out


@pytest.fixture(scope="module")
def problems():
    return {name: golden_problem(name)[:4] for name in FIXTURES}


@pytest.fixture(scope="module")
def oracle_ref(problems):
    """Computed once, shared, never modified: (fixture, side, tol) -> per-lambda oracle outputs."""
    ref = {}
    for name, (A, B, b, xt) in problems.items():
        for side in ("ab", "ba"):
            for tol in (0.0, 0.05):
                ref[name, side, tol] = _oracle_sweep(A, B, b, xt, tol, side)
    return ref


@pytest.mark.parametrize("side", ["ab", "ba"])
@pytest.mark.parametrize("name", FIXTURES)
def test_sweep_matches_oracle_full_histories(gpu_ctx, problems, oracle_ref, name, side):
    A, B, b, xt = problems[name]
    S = hgmres.gmres_lambda_sweep(A, B, b, xt, 0.0, MAXIT, LAMBDAS, side, ctx=gpu_ctx, return_x=True,
                                  return_H=True)
    assert S.err.shape == S.res.shape == S.sol.shape == (MAXIT, LAMBDAS.size)
    assert S.ksteps == MAXIT
    for l, (x, e, r, k, sol, H) in enumerate(oracle_ref[name, side, 0.0]):
        assert S.niters[l] == k == MAXIT
        hist_ok(S.res[:, l], r, TOL)
        hist_ok(S.err[:, l], e, TOL)
        hist_ok(S.sol[:, l], sol, TOL)
        assert rel(S.X[:, l], x) <= TOL, (l, rel(S.X[:, l], x))
    H_ok(S.H, oracle_ref[name, side, 0.0][0][5])


@pytest.mark.parametrize("side", ["ab", "ba"])
@pytest.mark.parametrize("name", FIXTURES)
def test_sweep_matches_oracle_stopping(gpu_ctx, problems, oracle_ref, name, side):
    """tol = 0.05: every lambda stops at its own iteration, as the oracle's solve at that lambda."""
    tol = 0.05
    A, B, b, xt = problems[name]
    ref = oracle_ref[name, side, tol]
    full = oracle_ref[name, side, 0.0]
    # no oracle residual lies within rounding of tol, so a rounding-level difference cannot flip a stop
    gap = min(np.min(np.abs(f[2] - tol) / tol) for f in full)
    print(f"{name} {side}: oracle niters {[f[3] for f in ref]}, closest residual to tol {gap:.3g} (relative)")
    assert gap > 1e-6, gap
    assert len({f[3] for f in ref}) > 1 and max(f[3] for f in ref) == MAXIT      # both kinds of stop occur
    S = hgmres.gmres_lambda_sweep(A, B, b, xt, tol, MAXIT, LAMBDAS, side, ctx=gpu_ctx, return_x=True)
    assert S.ksteps == max(f[3] for f in ref)
    for l, (x, e, r, k, sol, H) in enumerate(ref):
        assert S.niters[l] == k, (l, S.niters[l], k)
        hist_ok(S.res[:k, l], r, TOL)
        hist_ok(S.err[:k, l], e, TOL)
        hist_ok(S.sol[:k, l], sol, TOL)
        assert rel(S.X[:, l], x) <= TOL, (l, rel(S.X[:, l], x))
        for surf in (S.res, S.err, S.sol):
            assert np.all(np.isnan(surf[k:, l])) and not np.any(np.isnan(surf[:k, l]))


# ---------------------------------------------------------------------------------------------
# 3. sweep against the device's single-lambda solver
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["ab", "ba"])
def test_sweep_matches_single_solver(gpu_ctx, problems, side):
    A, B, b, xt = problems["tomo24_pixel.npz"]
    tol = 0.05
    Ao, Bo = hgmres.as_operator(A, gpu_ctx), hgmres.as_operator(B, gpu_ctx)
    S = hgmres.gmres_lambda_sweep(Ao, Bo, b, xt, tol, MAXIT, LAMBDAS, side, ctx=gpu_ctx, return_x=True)
    for l in (0, 7, 14):
        x, e, r, k = SINGLE[side](Ao, Bo, b, xt, tol, MAXIT, LAMBDAS[l], ctx=gpu_ctx)[:4]
        assert S.niters[l] == k
        hist_ok(S.res[:k, l], r, TOL)
        hist_ok(S.err[:k, l], e, TOL)
        assert rel(S.X[:, l], x) <= TOL
    # no x_true: the error surface stays NaN, everything else is unchanged
    N = hgmres.gmres_lambda_sweep(Ao, Bo, b, None, tol, MAXIT, LAMBDAS, side, ctx=gpu_ctx, return_x=True)
    assert np.all(np.isnan(N.err))
    assert np.array_equal(N.niters, S.niters)
    assert np.array_equal(N.res, S.res, equal_nan=True) and np.array_equal(N.sol, S.sol, equal_nan=True)
    assert np.array_equal(N.X, S.X)


# ---------------------------------------------------------------------------------------------
# 4. tiled operator pair (one-pass A*(B*q)), CGS2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["ab", "ba"])
def test_sweep_tiled_pair_matches_untiled(gpu_ctx, side):
    """Siddon N = 32 stored in 4 x 4 tiles with its device transpose: the AB side takes the one-pass
    fused_ab route, and X and x_true cross the stored pixel order.  Same results as the untiled pair."""
    P = tomo_problem(32, 16, noise=1e-2, seed=0)
    At = hgmres.SparseOperator.siddon(32, 16, gpu_ctx, order=(4, 0))
    Bt = At.T
    Ar = hgmres.SparseOperator.siddon(32, 16, gpu_ctx, order="reference")
    Br = Ar.T
    assert At.pixel_order("cols")[1] == 4 and Ar.pixel_order("cols")[0] == 0
    assert hgmres.fused_plan_info(At, Bt)["nslot"] > 0          # the pair has a one-pass plan
    St = hgmres.gmres_lambda_sweep(At, Bt, P.b, P.x_true, 0.05, MAXIT, LAMBDAS, side, ctx=gpu_ctx, return_x=True)
    Sr = hgmres.gmres_lambda_sweep(Ar, Br, P.b, P.x_true, 0.05, MAXIT, LAMBDAS, side, ctx=gpu_ctx, return_x=True)
    assert np.array_equal(St.niters, Sr.niters)
    for a, r in ((St.res, Sr.res), (St.err, Sr.err), (St.sol, Sr.sol)):
        hist_ok(a, r, TOL)
    for l in range(LAMBDAS.size):
        assert rel(St.X[:, l], Sr.X[:, l]) <= TOL
    # and the tiled sweep equals the single solver on the same pair
    x, e, r, k = SINGLE[side](At, Bt, P.b, P.x_true, 0.05, MAXIT, LAMBDAS[3], ctx=gpu_ctx)[:4]
    assert St.niters[3] == k and rel(St.X[:, 3], x) <= TOL
    hist_ok(St.err[:k, 3], e, TOL)


@pytest.mark.parametrize("side", ["ab", "ba"])
def test_sweep_cgs2_matches_oracle_cgs2(gpu_ctx, problems, monkeypatch, side):
    """orth = 'cgs2' against the oracle's solver with its CGS2 Arnoldi step in place of MGS."""
    A, B, b, xt = problems["tomo24_pixel.npz"]
    monkeypatch.setattr(R, "_mgs_arnoldi_step", R._cgs2_arnoldi_step)
    lams = LAMBDAS[::5]
    ref = _oracle_sweep(A, B, b, xt, 0.0, side, lambdas=lams)
    S = hgmres.gmres_lambda_sweep(A, B, b, xt, 0.0, MAXIT, lams, side, ctx=gpu_ctx, orth="cgs2", return_x=True,
                                  return_H=True)
    H_ok(S.H, ref[0][5])
    for l, (x, e, r, k, sol, H) in enumerate(ref):
        assert S.niters[l] == k
        hist_ok(S.res[:, l], r, TOL)
        hist_ok(S.err[:, l], e, TOL)
        hist_ok(S.sol[:, l], sol, TOL)
        assert rel(S.X[:, l], x) <= TOL


# ---------------------------------------------------------------------------------------------
# 5. refusals and breakdown
# ---------------------------------------------------------------------------------------------
def test_sweep_refusals(gpu_ctx, problems):
    A, B, b, xt = problems["tomo24_matched.npz"]
    args = (b, xt, 0.0, 4)
    A32 = hgmres.as_operator(A, gpu_ctx, dtype=L.HGM_F32)
    with pytest.raises(ValueError, match="fp64"):
        hgmres.gmres_lambda_sweep(A32, A32.T, *args, [1.0], "ba", ctx=gpu_ctx)
    with gpu_ctx.options(parity=1):
        with pytest.raises(ValueError, match="parity"):
            hgmres.gmres_lambda_sweep(A, B, *args, [1.0], "ab", ctx=gpu_ctx)
    with pytest.raises(ValueError, match="at least one lambda"):
        hgmres.gmres_lambda_sweep(A, B, *args, [], "ab", ctx=gpu_ctx)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite and >= 0"):
            hgmres.gmres_lambda_sweep(A, B, *args, [1.0, bad], "ab", ctx=gpu_ctx)
    with pytest.raises(ValueError):
        hgmres.gmres_lambda_sweep(A, B, *args, [1.0], "xy", ctx=gpu_ctx)
    # a context with a host all-reduce hook at world 2: HGM_E_UNSUPPORTED, and the hook is never called
    calls = []
    c2 = hgmres.Context(0)
    try:
        c2.set_host_allreduce(0, 2, lambda arr: calls.append(arr.size))
        with pytest.raises(hgmres.HgmError, match=f"status {L.HGM_E_UNSUPPORTED}"):
            hgmres.gmres_lambda_sweep(A, B, *args, [1.0], "ab", ctx=c2)
        assert calls == []
    finally:
        c2.close()
    # the context still solves after the refusals
    S = hgmres.gmres_lambda_sweep(A, B, *args, [1.0], "ab", ctx=gpu_ctx)
    assert S.niters[0] == 4


@pytest.mark.parametrize("side", ["ab", "ba"])
def test_sweep_zero_operator_breaks_like_single_solver(gpu_ctx, side):
    """An all-zero A: H(2,1) = 0 at the first step, x is never assigned -- the status of
    hgm_gmres_bounds on the same input (test_gpu_edge.py's empty operator)."""
    A = sp.csr_matrix((6, 4))
    B = sp.csr_matrix(np.ones((4, 6)))
    b, xt = np.arange(1.0, 7.0), np.ones(4)
    def status(call):
        try:
            call()
        except hgmres.HgmError as e:
            return type(e)
        return None

    single = status(lambda: SINGLE[side](A, B, b, xt, 1e-2, 3, 0.5, ctx=gpu_ctx))
    sweep = status(lambda: hgmres.gmres_lambda_sweep(A, B, b, xt, 1e-2, 3, [0.5, 2.0], side, ctx=gpu_ctx,
                                                     return_x=True))
    assert single is hgmres.OutputNotAssigned
    assert sweep is single


# ---------------------------------------------------------------------------------------------
# 6. pipeline
# ---------------------------------------------------------------------------------------------
def test_error_surface_matches_solver_loop(gpu_ctx, problems):
    A, B, b, xt = problems["tomo24_matched.npz"]
    lams = LAMBDAS[::2]
    E = analysis.error_surface(A, B, b, xt, lams, MAXIT, ctx=gpu_ctx)
    for side in ("ab", "ba"):
        surf = np.full((MAXIT, lams.size), np.nan)
        for l, lam in enumerate(lams):
            e = SINGLE[side](A, B, b, xt, 1e-10, MAXIT, lam, ctx=gpu_ctx)[1]
            surf[: e.size, l] = e
        hist_ok(E[f"error_surface_{side}"], surf, TOL)
        k, l = np.unravel_index(int(np.nanargmin(surf)), surf.shape)
        opt = E[f"optimal_{side}"]
        assert (opt["k"], opt["lambda"]) == (k + 1, lams[l])
        assert abs(opt["error"] - surf[k, l]) <= TOL * surf[k, l]


def test_analyze_regularization_sweep_keyword(gpu_ctx, problems):
    """sweep=True takes the six lambda-loop arrays from two sweeps; the rest of the pipeline is shared."""
    A, B, b, xt = problems["tomo24_matched.npz"]
    # (DeltaM = None: the final solves then skip outputs 5-8, which the pipeline discards, and with them
    # eight dense eigen-solves of dimension 408 / 576 that have nothing to do with the lambda loop)
    P = analysis.RegularizationProblem(A, b, A @ xt, xt, sp.csr_matrix(B - A.T), B, None, None)
    kw = dict(maxit=8, tol=0.05, lambda_range=LAMBDAS[::3], k_gcv=8, ctx=gpu_ctx)
    loop = analysis.analyze_regularization(P, **kw)
    swp = analysis.analyze_regularization(P, sweep=True, **kw)
    for key in ("res_norms_ab", "sol_norms_ab", "err_norms_ab", "res_norms_ba", "sol_norms_ba", "err_norms_ba"):
        assert swp[key].shape == loop[key].shape == (LAMBDAS[::3].size,)
        hist_ok(swp[key], loop[key], TOL)
    for key in ("lambda_true_optimal_ab", "lambda_true_optimal_ba", "lambda_gcv_ab", "lambda_gcv_ba"):
        assert swp[key] == loop[key]


def test_matlab_wrapper_runs_the_sweep(gpu_ctx, problems):
    """matlab/gmres_lambda_sweep.m through the gateway (the mx API stand-in): the Python binding's
    outputs, with and without X (the nargout <= 4 path never forms it)."""
    from mwrap import Function
    from test_mex_gateway import Mex
    A, B, b, xt = problems["tomo24_pixel.npz"]
    f = Function(os.path.join(ROOT, "matlab", "gmres_lambda_sweep.m"), Mex())
    S = hgmres.gmres_lambda_sweep(A, B, b, xt, 0.05, MAXIT, LAMBDAS, "ba", ctx=gpu_ctx, return_x=True)
    e, r, sn, ni, X = f(5, sp.csc_matrix(A), sp.csc_matrix(B), b, xt, 0.05, float(MAXIT), LAMBDAS, "ba")
    assert e.shape == r.shape == sn.shape == (MAXIT, LAMBDAS.size) and X.shape == S.X.shape
    assert np.array_equal(ni.astype(int), S.niters)
    for got, ref in ((e, S.err), (r, S.res), (sn, S.sol)):
        hist_ok(got, ref, 1e-12)
    assert rel(X, S.X) <= 1e-12                                # (the gateway hands A over as CSC)
    e4, r4, sn4, ni4 = f(4, sp.csc_matrix(A), sp.csc_matrix(B), b, xt, 0.05, float(MAXIT), LAMBDAS, "ba")
    assert np.array_equal(e4, e, equal_nan=True) and np.array_equal(r4, r, equal_nan=True)
    assert np.array_equal(ni4, ni)
    # x_true = []: the error surface stays NaN
    e0 = f(1, sp.csc_matrix(A), sp.csc_matrix(B), b, np.zeros((0, 0)), 0.05, float(MAXIT), LAMBDAS, "ba")[0]
    assert np.all(np.isnan(e0))
