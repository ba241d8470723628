"""Batched multi-RHS *_bounds solves (hgm_gmres_bounds_batch) and their multi-vector product
(hgm_spmm, csrc/spmm.hip), on the device.

* the kernel against scipy at a derived bound, its bitwise invariance under the vector count, the
  slot and the neighbours, and tiled operators against hgm_spmv;
* the batch against the oracle's four ``*_bounds`` solvers called once per column, at the project's
  bar 1e-10, with a stopping tolerance at which columns leave the batch at different iterations;
* the batch against itself, bitwise: one batch = its columns run alone, across repacked groups;
* the batch on operators in a stored pixel order against the reference-order pair, one x_true per column;
* breakdown inside a batch, refusals, and the noise-level pipeline and gateway command on top.
"""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, golden_problem
import hgmres
from hgmres import _lib as L
from hgmres import analysis
from hgmres.regtools import generate_test_problem
from oracle import restatement as R   # checker only
from tiled_pair import tiled_pair

pytestmark = pytest.mark.gpu

TOL = 1e-10                      # the project's bar (tests/test_gpu_sweep.py)
EPS = np.finfo(np.float64).eps
MAXIT = 12
NRHS = 5
LEVELS = np.logspace(-4, -1, NRHS)
LAMS = np.array([1e-2, 1e-1, 1.0, 10.0, 100.0])
# The oracle's residual histories of the five columns cross 2.2e-2 at different iterations (7 or 8 for
# the low noise levels, one or two later for level 1.8e-2, never within 12 for level 1e-1), each with a
# margin of more than 1 % (measured on the CPU); _oracle_batch asserts the spread on the oracle's result.
STOP = 2.2e-2
FIXTURES = ("tomo24_matched.npz", "tomo24_pixel.npz")
ORACLE = {("ab", True): R.ABgmres_hybrid_bounds, ("ba", True): R.BAgmres_hybrid_bounds,
          ("ab", False): R.ABgmres_nonhybrid_bounds, ("ba", False): R.BAgmres_nonhybrid_bounds}
SINGLE = {("ab", True): hgmres.ABgmres_hybrid_bounds, ("ba", True): hgmres.BAgmres_hybrid_bounds,
          ("ab", False): hgmres.ABgmres_nonhybrid_bounds, ("ba", False): hgmres.BAgmres_nonhybrid_bounds}
CASES = [("ab", True), ("ba", True), ("ab", False), ("ba", False)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def hist_ok(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    d = np.abs(a - b)[ok]
    s = np.maximum(np.abs(b), 1e-300)[ok]
    assert np.all(d <= tol * s + 1e-300), (d / s).max()


def padded_hist(h, maxit=MAXIT):
    out = np.full(maxit, np.nan)
    out[: len(h)] = h
    return out


def noisy_rhs(b, levels, seed=7):
    rng = np.random.default_rng(seed)
    nb = np.linalg.norm(b)
    cols = []
    for lv in levels:
        e = rng.standard_normal(b.size)
        cols.append(b + e / np.linalg.norm(e) * lv * nb)
    return np.stack(cols, axis=1)


def same_batch(a, b, cols_a=None, cols_b=None):
    """Two BatchResults equal bit for bit (on the given columns)."""
    ca = slice(None) if cols_a is None else cols_a
    cb = slice(None) if cols_b is None else cols_b
    assert np.array_equal(a.niters[ca], b.niters[cb])
    assert np.array_equal(a.status[ca], b.status[cb])
    assert np.array_equal(a.x[:, ca], b.x[:, cb], equal_nan=True)
    assert np.array_equal(a.error_norm[:, ca], b.error_norm[:, cb], equal_nan=True)
    assert np.array_equal(a.residual_norm[:, ca], b.residual_norm[:, cb], equal_nan=True)
    if a.H is not None and b.H is not None:
        assert np.array_equal(a.H[ca], b.H[cb])


# ---------------------------------------------------------------------------------------------
# 1. kernel against scipy
# ---------------------------------------------------------------------------------------------
def _random_csr(rows, cols, lens, seed):
    rng = np.random.default_rng(seed)
    indptr = np.zeros(rows + 1, dtype=np.int64)
    idx, val = [], []
    for i in range(rows):
        ln = int(lens[i % len(lens)])
        idx.append(np.sort(rng.choice(cols, size=ln, replace=False)))
        val.append(rng.standard_normal(ln))
        indptr[i + 1] = indptr[i] + ln
    return sp.csr_matrix((np.concatenate(val), np.concatenate(idx).astype(np.int32), indptr), shape=(rows, cols))


# rows x cols with the row lengths cycled: empty and one-entry rows, rows shorter than any group
# width (2, 3), rows of 300 and 5000 entries (a lane takes many strides), and > 65,536 columns
KERNEL_OPS = {
    "rows1": (1, 6000, [5000]),
    "rows7": (7, 6000, [0, 1, 3, 300, 5000, 2, 17]),
    "rows64": (64, 6000, [9, 0, 1, 300, 31, 33, 3, 64]),
    "rows65": (65, 6000, [2, 5000, 0, 1, 65, 300, 7]),
    "rows1000_wide": (1000, 70001, [12, 0, 1, 3, 40, 300, 5, 5000, 64, 29] + [20] * 90),
}


def _spmm_padded(ctx, Aop, X, pad):
    """hgm_spmm on device buffers with leading dimensions padded by `pad`, the padding NaN; returns the
    whole (rows + pad) x nvec output buffer."""
    lib = L.load()
    m, n = Aop.shape
    nv = X.shape[1]
    ldx, ldy = n + pad, m + pad
    Xb = np.full((ldx, nv), np.nan, order="F")
    Xb[:n, :] = X
    Yb = np.full((ldy, nv), np.nan, order="F")
    px, py = C.c_void_p(), C.c_void_p()
    try:
        for p_, cnt in ((px, ldx * nv), (py, ldy * nv)):
            assert lib.hgm_dev_alloc(ctx.handle, 8 * cnt, C.byref(p_)) == L.HGM_OK
        assert lib.hgm_memcpy_h2d(ctx.handle, px, Xb.ctypes.data_as(C.c_void_p), 8 * ldx * nv) == L.HGM_OK
        assert lib.hgm_memcpy_h2d(ctx.handle, py, Yb.ctypes.data_as(C.c_void_p), 8 * ldy * nv) == L.HGM_OK
        assert lib.hgm_spmm(ctx.handle, Aop._h, nv, px, ldx, py, ldy) == L.HGM_OK
        assert lib.hgm_memcpy_d2h(ctx.handle, Yb.ctypes.data_as(C.c_void_p), py, 8 * ldy * nv) == L.HGM_OK
    finally:
        for p_ in (px, py):
            if p_.value:
                lib.hgm_dev_free(ctx.handle, p_)
    return Yb


def _bound(A, X):
    """(2 len_i + 2) eps (|A||X|)_ir: two summations of len_i terms in different orders."""
    lens = np.diff(A.indptr).astype(np.float64)
    return (2.0 * lens + 2.0)[:, None] * EPS * (abs(A) @ np.abs(X))


@pytest.mark.parametrize("name", list(KERNEL_OPS))
def test_spmm_against_scipy(gpu_ctx, name):
    rows, cols, lens = KERNEL_OPS[name]
    A = _random_csr(rows, cols, lens, seed=rows)
    Aop = hgmres.SparseOperator.from_scipy(A, ctx=gpu_ctx)
    rng = np.random.default_rng(rows + 1)
    Xall = rng.standard_normal((cols, 8))
    for nv in range(1, 9):                                   # 3, 5, 6, 7 run with zero slots
        X = Xall[:, :nv]
        Yb = _spmm_padded(gpu_ctx, Aop, X, 6)
        got, padding = Yb[:rows, :], Yb[rows:, :]
        assert np.all(np.isfinite(got)), (name, nv)
        assert np.all(np.isnan(padding)), (name, nv)          # nothing written past the rows
        ref = A @ X
        excess = np.abs(got - ref) - _bound(A, X)
        assert np.all(excess <= 0), (name, nv, excess.max())


def test_spmm_bitwise_invariance(gpu_ctx):
    """A column's bits do not depend on the vector count, its slot, or the other columns."""
    rows, cols, lens = KERNEL_OPS["rows1000_wide"]
    A = _random_csr(rows, cols, lens, seed=5)
    Aop = hgmres.SparseOperator.from_scipy(A, ctx=gpu_ctx)
    X = np.random.default_rng(6).standard_normal((cols, 8))
    Y8 = hgmres.spmm(Aop, X)
    assert np.array_equal(Y8, hgmres.spmm(Aop, X))           # two identical calls
    for r in range(8):
        a, b = (r + 1) % 8, (r + 5) % 8
        assert np.array_equal(hgmres.spmm(Aop, X[:, [r]])[:, 0], Y8[:, r]), r           # alone
        assert np.array_equal(hgmres.spmm(Aop, X[:, [r, a, b]])[:, 0], Y8[:, r]), r     # slot 0 of nvec = 3
        assert np.array_equal(hgmres.spmm(Aop, X[:, [a, b, r]])[:, 2], Y8[:, r]), r     # last of nvec = 3
    perm = [1, 2, 3, 4, 5, 6, 7, 0]
    assert np.array_equal(hgmres.spmm(Aop, X[:, perm])[:, 7], Y8[:, 0])                 # last slot of 8


@pytest.mark.parametrize("transpose", [False, True])
def test_spmm_tiled_operator_matches_spmv(gpu_ctx, transpose):
    """Siddon N = 32 stored in 4 x 4 tiles and 16 x 16 super-blocks, and its transpose: the columns cross
    the stored pixel order on the way in (A) or out (A')."""
    A = hgmres.SparseOperator.siddon(32, 16, gpu_ctx, order=(4, 16))
    assert A.pixel_order("cols")[1:] == (4, 16)
    M = A.T if transpose else A
    S = M.to_scipy()
    X = np.random.default_rng(3).standard_normal((M.shape[1], 5))
    Y = hgmres.spmm(M, X)
    bound = _bound(S, X)
    for r in range(5):
        y1 = M @ X[:, r]
        assert np.all(np.abs(Y[:, r] - y1) <= bound[:, r]), r
        assert np.all(np.abs(Y[:, r] - S @ X[:, r]) <= bound[:, r]), r


# ---------------------------------------------------------------------------------------------
# 2. the batch against the oracle, column by column
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problems(gpu_ctx):
    out = {}
    for name in FIXTURES:
        A, B, b, xt, _ = golden_problem(name)
        out[name] = dict(A=A, B=B, b=b, xt=xt, Bm=noisy_rhs(b, LEVELS),
                         Ao=hgmres.SparseOperator.from_scipy(A, ctx=gpu_ctx),
                         Bo=hgmres.SparseOperator.from_scipy(B, ctx=gpu_ctx))
    return out


_ORACLE_CACHE = {}


def _oracle_batch(problems, name, side, hybrid, cgs2=False):
    """The oracle's solver once per column (computed once per case), and the check that the stopping
    tolerance spreads the columns: at least two distinct niters, at least one below maxit."""
    key = (name, side, hybrid, cgs2)
    if key not in _ORACLE_CACHE:
        P = problems[name]
        ref = []
        for j in range(NRHS):
            args = (P["A"], P["B"], P["Bm"][:, j], P["xt"], STOP, MAXIT) + ((LAMS[j],) if hybrid else ())
            ref.append(ORACLE[(side, hybrid)](*args, return_H=True)[:5])
        _ORACLE_CACHE[key] = ref
    ref = _ORACLE_CACHE[key]
    nit = [r[3] for r in ref]
    assert len(set(nit)) >= 2 and min(nit) < MAXIT, nit
    return ref


def _check_against_oracle(Rb, ref):
    assert np.all(Rb.status == L.HGM_OK)
    for j, (x, e, r, k, H) in enumerate(ref):
        assert Rb.niters[j] == k, (j, Rb.niters[j], k)
        hist_ok(Rb.residual_norm[:, j], padded_hist(r), TOL)
        hist_ok(Rb.error_norm[:, j], padded_hist(e), TOL)
        assert rel(Rb.x[:, j], x) <= TOL, j
        assert np.max(np.abs(Rb.H[j] - H)) <= TOL * np.max(np.abs(H)), j


@pytest.mark.parametrize("side,hybrid", CASES)
@pytest.mark.parametrize("name", FIXTURES)
def test_batch_matches_oracle(gpu_ctx, problems, name, side, hybrid):
    P = problems[name]
    ref = _oracle_batch(problems, name, side, hybrid)
    Rb = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], P["xt"], STOP, MAXIT, side,
                                   lambdas=LAMS if hybrid else None, ctx=gpu_ctx, return_H=True)
    _check_against_oracle(Rb, ref)


def test_batch_cgs2_matches_oracle_cgs2(gpu_ctx, problems, monkeypatch):
    """orth = 'cgs2' against the oracle's solver with its CGS2 Arnoldi step in place of MGS."""
    monkeypatch.setattr(R, "_mgs_arnoldi_step", R._cgs2_arnoldi_step)
    P = problems["tomo24_pixel.npz"]
    ref = _oracle_batch(problems, "tomo24_pixel.npz", "ab", True, cgs2=True)
    Rb = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], P["xt"], STOP, MAXIT, "ab", lambdas=LAMS, ctx=gpu_ctx,
                                   orth="cgs2", return_H=True)
    _check_against_oracle(Rb, ref)


@pytest.mark.parametrize("side,hybrid", CASES)
def test_batch_matches_single_solver(gpu_ctx, problems, side, hybrid):
    """The same pick against the library's own single solvers (the loop the batch replaces)."""
    P = problems["tomo24_matched.npz"]
    _oracle_batch(problems, "tomo24_matched.npz", side, hybrid)          # the spread of niters holds
    Rb = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], P["xt"], STOP, MAXIT, side,
                                   lambdas=LAMS if hybrid else None, ctx=gpu_ctx, return_H=True)
    for j in range(NRHS):
        args = (P["Ao"], P["Bo"], P["Bm"][:, j], P["xt"], STOP, MAXIT) + ((LAMS[j],) if hybrid else ())
        out = SINGLE[(side, hybrid)](*args, ctx=gpu_ctx, return_H=True)
        (x, e, r, k), H = out[:4], out[-1]
        assert Rb.niters[j] == k
        hist_ok(Rb.residual_norm[:, j], padded_hist(r), TOL)
        hist_ok(Rb.error_norm[:, j], padded_hist(e), TOL)
        assert rel(Rb.x[:, j], x) <= TOL
        assert np.max(np.abs(Rb.H[j] - H)) <= TOL * np.max(np.abs(H))


# ---------------------------------------------------------------------------------------------
# 3. batch composition, bitwise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", False)])
def test_batch_equals_its_columns_alone(gpu_ctx, problems, side, hybrid):
    P = problems["tomo24_pixel.npz"]
    kw = dict(ctx=gpu_ctx, return_H=True)
    Rb = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], P["xt"], STOP, MAXIT, side,
                                   lambdas=LAMS if hybrid else None, **kw)
    assert len(set(Rb.niters)) >= 2                          # columns left the batch at different steps
    for j in range(NRHS):
        R1 = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"][:, [j]], P["xt"], STOP, MAXIT, side,
                                       lambdas=LAMS[[j]] if hybrid else None, **kw)
        same_batch(Rb, R1, [j], [0])


def test_batch_of_two_groups_equals_its_columns_alone(gpu_ctx, problems):
    """11 columns: two packed groups (8 + 3), regrouped as columns finish."""
    P = problems["tomo24_matched.npz"]
    levels = np.logspace(-4, -1, 11)
    Bm = noisy_rhs(P["b"], levels, seed=11)
    lams = np.logspace(-2, 2, 11)
    kw = dict(ctx=gpu_ctx, return_H=True)
    Rb = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], Bm, P["xt"], STOP, MAXIT, "ab", lambdas=lams, **kw)
    assert len(set(Rb.niters)) >= 2 and min(Rb.niters) < MAXIT
    for j in range(11):
        R1 = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], Bm[:, [j]], P["xt"], STOP, MAXIT, "ab", lambdas=lams[[j]], **kw)
        same_batch(Rb, R1, [j], [0])


def test_shared_x_true_equals_repeated_column(gpu_ctx, problems):
    P = problems["tomo24_matched.npz"]
    XT = np.repeat(P["xt"][:, None], NRHS, axis=1)
    a = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], P["xt"], STOP, MAXIT, "ba", lambdas=LAMS, ctx=gpu_ctx)
    b = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], XT, STOP, MAXIT, "ba", lambdas=LAMS, ctx=gpu_ctx)
    same_batch(a, b)
    # no x_true: the error histories stay NaN, everything else is unchanged
    c = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], P["Bm"], None, STOP, MAXIT, "ba", lambdas=LAMS, ctx=gpu_ctx)
    assert np.all(np.isnan(c.error_norm))
    assert np.array_equal(c.x, a.x) and np.array_equal(c.residual_norm, a.residual_norm, equal_nan=True)


@pytest.fixture(scope="module")
def tiled(gpu_ctx):
    return tiled_pair(gpu_ctx)


@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", False)])
def test_batch_on_tiled_operators(gpu_ctx, tiled, side, hybrid):
    """The batch on operators with a stored pixel order against the same pair in the reference order, b, x_true
    and x in the reference order: three different x_true columns, so a permutation into the stored order that
    reaches the wrong column, or none, is an O(1) error in that column's error history; x comes back through
    the inverse permutation."""
    P = tiled["P"]
    xt = np.asarray(P.x_true, dtype=np.float64).ravel()
    Bm = noisy_rhs(np.asarray(P.b, dtype=np.float64).ravel(), LEVELS[[0, 2, 4]])
    XT = xt[:, None] * np.array([1.0, 0.5, -1.0])[None, :]
    lam = LAMS[:3] if hybrid else None
    run = lambda A, B, x_true: hgmres.gmres_bounds_batch(A, B, Bm, x_true, 0.0, 8, side, lambdas=lam, ctx=gpu_ctx,
                                                         return_H=True)
    for x_true in (XT, xt):                                  # one x_true per column, then one shared
        Rt, Rr = run(tiled["At"], tiled["Bt"], x_true), run(tiled["Ar"], tiled["Br"], x_true)
        assert np.array_equal(Rt.niters, Rr.niters) and np.all(Rt.niters == 8)
        for j in range(3):
            assert rel(Rt.x[:, j], Rr.x[:, j]) <= TOL
            hist_ok(Rt.residual_norm[:, j], Rr.residual_norm[:, j], TOL)
            hist_ok(Rt.error_norm[:, j], Rr.error_norm[:, j], TOL)
            assert np.max(np.abs(Rt.H[j] - Rr.H[j])) <= TOL * np.max(np.abs(Rr.H[j]))
        if x_true is XT:   # the columns' x_true are told apart: far more than the bar between their histories
            assert min(rel(Rr.error_norm[:, 1], Rr.error_norm[:, 0]), rel(Rr.error_norm[:, 2], Rr.error_norm[:, 0])) > 1e-3


# ---------------------------------------------------------------------------------------------
# 4. breakdown
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["ab", "ba"])
def test_batch_empty_operator_breaks_every_column(gpu_ctx, side):
    """An all-zero A (test_gpu_edge.py's empty operator): H(2,1) = 0 at the first step of every column."""
    A = sp.csr_matrix((6, 4))
    B = sp.csr_matrix(np.ones((4, 6)))
    Bm = np.arange(1.0, 19.0).reshape(6, 3, order="F")
    xt = np.ones(4)
    Ao, Bo = hgmres.as_operator(A, gpu_ctx), hgmres.as_operator(B, gpu_ctx)
    lib = L.load()
    X = np.full((4, 3), 7.0, order="F")
    err, res = np.zeros((3, 3), order="F"), np.zeros((3, 3), order="F")
    nit, st = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    lam = np.array([0.5, 1.0, 2.0])
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp)
    rc = lib.hgm_gmres_bounds_batch(gpu_ctx.handle, None, Ao._h, Bo._h, dp(np.asfortranarray(Bm)), 6, 3, dp(xt), 0, 1e-2, 3,
                                    dp(lam), L.HGM_SIDE_AB if side == "ab" else L.HGM_SIDE_BA, 1, dp(X), 4, dp(err),
                                    dp(res), nit.ctypes.data_as(ip), st.ctypes.data_as(ip))
    assert rc == L.HGM_E_NOT_ASSIGNED
    assert np.all(st == L.HGM_E_NOT_ASSIGNED) and np.all(nit == 1)
    assert np.all(X == 7.0)                                  # the X columns are left untouched
    Rb = hgmres.gmres_bounds_batch(Ao, Bo, Bm, xt, 1e-2, 3, side, lambdas=lam, ctx=gpu_ctx)
    assert np.all(Rb.status == L.HGM_E_NOT_ASSIGNED) and np.all(Rb.niters == 1) and np.all(np.isnan(Rb.x))


def test_batch_mid_run_breakdown_in_one_column(gpu_ctx):
    """A breakdown at k = 2 in one column of three, built as test_breakdown_gpu builds its own: a small explicit
    operator with an invariant subspace that the right-hand side reaches after two steps.  Here A*B maps
    e1 -> e2 -> 0, so for b = e1 every Arnoldi quantity is an exact 0 or 1 and H(3,2) == 0 holds in any
    summation order.  (On test_breakdown_gpu's diag(1,1,2,2), b = (2,2,1,1) that zero is a matter of rounding:
    the oracle's *_bounds solver stops at k = 2, the device's single solver, measured, runs all 4 iterations.)"""
    A2 = sp.identity(4, format="csr")
    B2 = sp.csr_matrix(np.array([[0.0, 0, 0, 0], [1.0, 0, 0, 0], [0, 0, 2.0, 0], [0, 0, 0, 3.0]]))
    b2 = np.array([1.0, 0.0, 0.0, 0.0])
    xt = np.ones(4)
    rng = np.random.default_rng(0)
    Bm = np.stack([rng.standard_normal(4), b2, rng.standard_normal(4)], axis=1)
    Ao, Bo = hgmres.as_operator(A2, gpu_ctx), hgmres.as_operator(B2, gpu_ctx)
    kw = dict(ctx=gpu_ctx, return_H=True)
    Rb = hgmres.gmres_bounds_batch(Ao, Bo, Bm, xt, 0.0, 4, "ab", **kw)
    out = hgmres.ABgmres_nonhybrid_bounds(Ao, Bo, b2, xt, 0.0, 4, ctx=gpu_ctx, return_H=True)
    (x, e, r, k), H = out[:4], out[-1]
    xr, er, rr, kr = R.ABgmres_nonhybrid_bounds(A2, B2, b2, xt, 0.0, 4)[:4]
    assert k == kr == 2 and r[1] == 0.0                      # the single solver broke down at k = 2
    assert Rb.niters[1] == 2 and Rb.status[1] == L.HGM_OK
    assert Rb.residual_norm[1, 1] == 0.0 and Rb.error_norm[1, 1] == 0.0 and np.all(np.isnan(Rb.residual_norm[2:, 1]))
    assert rel(Rb.x[:, 1], x) <= TOL and rel(Rb.x[:, 1], xr) <= TOL      # x is the previous iterate
    hist_ok(Rb.residual_norm[:2, 1], r, TOL)
    hist_ok(Rb.error_norm[:2, 1], e, TOL)
    assert np.max(np.abs(Rb.H[1] - H)) <= TOL * np.max(np.abs(H))
    for j in (0, 2):                                         # the neighbours are unaffected
        R1 = hgmres.gmres_bounds_batch(Ao, Bo, Bm[:, [j]], xt, 0.0, 4, "ab", **kw)
        same_batch(Rb, R1, [j], [0])
        assert Rb.niters[j] > 2


# ---------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------
def test_batch_refusals(gpu_ctx, problems):
    P = problems["tomo24_matched.npz"]
    A, B, Bm, xt = P["Ao"], P["Bo"], P["Bm"], P["xt"]
    lib = L.load()
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp) if a is not None else None
    m, n = A.shape
    Bf = np.asfortranarray(Bm)

    def call(ctx, Ah, Bh, nrhs, lam, hybrid, flags=0, Bsrc=Bf):
        o = L.hgm_opts()
        o.flags, o.orth, o.H_out = flags, L.HGM_MGS, None
        nit = np.zeros(max(nrhs, 1), dtype=np.int32)
        return lib.hgm_gmres_bounds_batch(ctx.handle, C.byref(o), Ah, Bh, dp(Bsrc), m, nrhs, dp(xt), 0, 0.0, 3, dp(lam),
                                          L.HGM_SIDE_AB, hybrid, None, n, None, None, nit.ctypes.data_as(ip), None)

    A32 = hgmres.as_operator(P["A"], gpu_ctx, dtype=L.HGM_F32)
    assert call(gpu_ctx, A32._h, A32.T._h, 2, None, 0) == L.HGM_E_ARG                    # fp32 operators
    with gpu_ctx.options(parity=1):
        assert call(gpu_ctx, A._h, B._h, 2, None, 0) == L.HGM_E_ARG                      # parity mode
    assert call(gpu_ctx, A._h, B._h, 2, None, 0, flags=L.HGM_DEVICE_PTRS) == L.HGM_E_ARG  # device pointers
    assert call(gpu_ctx, A._h, B._h, 0, None, 0) == L.HGM_E_ARG                          # nrhs < 1
    big = np.asfortranarray(np.repeat(Bm[:, :1], 65, axis=1))
    assert call(gpu_ctx, A._h, B._h, 65, None, 0, Bsrc=big) == L.HGM_E_ARG               # nrhs > 64
    for bad in (-1.0, np.nan, np.inf):
        assert call(gpu_ctx, A._h, B._h, 2, np.array([1.0, bad]), 1) == L.HGM_E_ARG      # bad lambda (hybrid)
        assert call(gpu_ctx, A._h, B._h, 2, np.array([1.0, bad]), 0) == L.HGM_OK         # ignored otherwise
    assert call(gpu_ctx, A._h, B._h, 2, None, 1) == L.HGM_E_ARG                          # hybrid needs lambdas
    # a context with a host all-reduce hook at world 2: HGM_E_UNSUPPORTED, and the hook is never called
    calls = []
    c2 = hgmres.Context(0)
    try:
        c2.set_host_allreduce(0, 2, lambda arr: calls.append(arr.size))
        A2 = hgmres.as_operator(P["A"], c2)
        assert call(c2, A2._h, A2.T._h, 2, None, 0) == L.HGM_E_UNSUPPORTED
        assert calls == []
    finally:
        c2.close()
    with pytest.raises(ValueError, match="fp64"):
        hgmres.spmm(A32, np.ones((n, 2)))
    assert lib.hgm_spmm(gpu_ctx.handle, A._h, 9, C.c_void_p(8), n, C.c_void_p(8), m) == L.HGM_E_ARG
    # the context still solves after the refusals
    Rb = hgmres.gmres_bounds_batch(A, B, Bm[:, :2], xt, 0.0, 3, "ab", ctx=gpu_ctx)
    assert np.all(Rb.niters == 3) and np.all(np.isfinite(Rb.x))


# ---------------------------------------------------------------------------------------------
# 6. pipeline
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gcv", [False, True])
def test_error_vs_noise_level_matches_solver_loop(gpu_ctx, problems, gcv):
    P = problems["tomo24_matched.npz"]
    levels = np.logspace(-3, -1, 4)
    b_exact = P["A"] @ P["xt"]
    lam_in = None if gcv else (np.array([1e-2, 0.1, 1.0, 10.0]), np.array([0.05, 0.5, 5.0, 50.0]))
    E = analysis.error_vs_noise_level(P["Ao"], P["Bo"], b_exact, P["xt"], levels, maxit=8, tol=0.05, k_gcv=8,
                                      lambdas=lam_in, seed=3, ctx=gpu_ctx)
    assert E["Bm"].shape == (P["A"].shape[0], 4)
    if gcv:
        for side in ("ab", "ba"):
            trace_m = P["A"].shape[0] if side == "ab" else P["A"].shape[1]
            for i in range(4):
                H, beta, _ = hgmres.arnoldi(P["Ao"], P["Bo"], E["Bm"][:, i], 8, side, ctx=gpu_ctx)
                assert E[f"lambda_gcv_{side}"][i] == hgmres.gcv_fminbnd(H, beta, trace_m, 1e-9, 1e-1, 1e-8)[0]
    else:
        assert np.array_equal(E["lambda_gcv_ab"], lam_in[0]) and np.array_equal(E["lambda_gcv_ba"], lam_in[1])
    for key, side, hybrid in (("hab", "ab", True), ("hba", "ba", True), ("nab", "ab", False), ("nba", "ba", False)):
        fin = np.zeros(4)
        for i in range(4):
            lam = (E[f"lambda_gcv_{side}"][i],) if hybrid else ()
            fin[i] = SINGLE[(side, hybrid)](P["Ao"], P["Bo"], E["Bm"][:, i], P["xt"], 0.05, 8, *lam, ctx=gpu_ctx)[1][-1]
        hist_ok(E[f"final_errors_{key}"], fin, TOL)


def test_error_vs_noise_level_smoke_on_shaw(gpu_ctx):
    """plot_error_vs_noise_level.m's own problem (shaw, n = 32, cond ~ 1e18): shapes and finiteness only.
    The late non-hybrid iterates are not comparable between summation orders there."""
    A, b_exact, x_true = generate_test_problem("shaw", 32)
    B = A.T + 1e-4 * np.random.default_rng(0).standard_normal(A.T.shape)
    levels = np.logspace(-4, -1, 6)
    E = analysis.error_vs_noise_level(sp.csr_matrix(A), sp.csr_matrix(B), b_exact, x_true, levels, maxit=32,
                                      ctx=gpu_ctx)
    assert E["Bm"].shape == (32, 6) and np.all(np.isfinite(E["Bm"]))
    for side in ("ab", "ba"):
        lam = E[f"lambda_gcv_{side}"]
        assert lam.shape == (6,) and np.all((lam >= 1e-9) & (lam <= 1e-1))
    for key in ("hab", "hba", "nab", "nba"):
        assert E[f"final_errors_{key}"].shape == (6,) and np.all(np.isfinite(E[f"final_errors_{key}"]))
        assert np.all((E[f"niters_{key}"] >= 1) & (E[f"niters_{key}"] <= 32))


def test_matlab_command_equals_python_call(gpu_ctx, problems):
    """matlab/gmres_bounds_batch.m through the gateway (the mx API stand-in) against the Python binding."""
    from mwrap import Function
    from test_mex_gateway import Mex
    P = problems["tomo24_pixel.npz"]
    A, B = sp.csr_matrix(P["A"]), sp.csr_matrix(P["B"])
    A.sort_indices()
    B.sort_indices()
    f = Function(os.path.join(ROOT, "matlab", "gmres_bounds_batch.m"), Mex())
    for side, lam in (("ab", LAMS), ("ba", None)):
        Rb = hgmres.gmres_bounds_batch(A, B, P["Bm"], P["xt"], STOP, MAXIT, side, lambdas=lam, ctx=gpu_ctx)
        args = (sp.csc_matrix(A), sp.csc_matrix(B), P["Bm"], P["xt"], STOP, float(MAXIT), side)
        X, e, r, ni, st = f(5, *(args + ((lam,) if lam is not None else ())))
        assert X.shape == Rb.x.shape and e.shape == r.shape == (MAXIT, NRHS)
        assert np.array_equal(ni.reshape(-1).astype(int), Rb.niters) and np.all(st == 0)
        assert np.array_equal(X, Rb.x)
        assert np.array_equal(e, Rb.error_norm, equal_nan=True) and np.array_equal(r, Rb.residual_norm, equal_nan=True)
