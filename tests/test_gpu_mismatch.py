"""Lockstep back-projector mismatch sweeps (hgm_gmres_bounds_mismatch, hgm_arnoldi_mismatch) and their perturbed
multi-vector product (hgm_spmm_pert, csrc/spmm.hip k_spmm_pert), on the device.

* the kernel against scipy at a derived bound for a same-pattern and an independent-pattern E, bit-equal to
  ``spmm(B0) + c * spmm(E)``, shared path == general path, invariant under the vector count, the slot and the
  neighbours' coefficients, and tiled operators;
* the sweep against the oracle's four ``*_bounds`` solvers called with explicit ``B + c_j E``, and against the
  library's single solvers on uploaded explicit operators, at the project's bar 1e-10;
* the sweep against itself, bitwise: one call = its levels alone, across repacked groups, and all-zero
  coefficients = ``gmres_bounds_batch`` with b replicated;
* the lockstep GCV Arnoldi, breakdown, refusals, the pipeline and the gateway command on top.

The helpers are those of test_gpu_batch.py (copied: that file stays as it is).
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

pytestmark = pytest.mark.gpu

TOL = 1e-10                      # the project's bar (tests/test_gpu_sweep.py)
EPS = np.finfo(np.float64).eps
MAXIT = 12
NCOEF = 5
LAMS = np.array([1e-2, 1e-1, 1.0, 10.0, 100.0])
# The oracle's residual histories of the five levels (c = logspace(-4, 0, 5) ||B||_F with ||E||_F = 1) cross
# 1.7e-2 at different iterations, no history entry closer to it than 1 % (measured on the CPU);
# _oracle_sweep asserts the spread and a margin of 1e-6 on the oracle's own result.
STOP = 1.7e-2
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
# 1. kernel
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


# test_gpu_batch.py's shapes: rows x cols with the row lengths cycled: empty and one-entry rows, rows shorter
# than any group width (2, 3), rows of 300 and 5000 entries (a lane takes many strides), and > 65,536 columns
KERNEL_OPS = {
    "rows1": (1, 6000, [5000]),
    "rows7": (7, 6000, [0, 1, 3, 300, 5000, 2, 17]),
    "rows64": (64, 6000, [9, 0, 1, 300, 31, 33, 3, 64]),
    "rows65": (65, 6000, [2, 5000, 0, 1, 65, 300, 7]),
    "rows1000_wide": (1000, 70001, [12, 0, 1, 3, 40, 300, 5, 5000, 64, 29] + [20] * 90),
}
COEFS8 = np.array([0.5, -2.0, 1e-3, 0.0, 7.25, -1e2, 1.0, 3e-7])


def _same_pattern(B0, seed):
    """Random values on B0's pattern."""
    return sp.csr_matrix((np.random.default_rng(seed).standard_normal(B0.nnz), B0.indices.copy(), B0.indptr.copy()),
                         shape=B0.shape)


def _other_pattern(B0, lens, seed):
    """A pattern of its own: B0's row lengths rotated by one row (so rows are empty where B0's are not, and
    long where B0's are short) -- unless no row of the rotation is empty: then every third row is emptied."""
    rows, cols = B0.shape
    rot = list(lens[1:]) + list(lens[:1])
    if 0 not in rot:
        rot = [0] + rot + [0]
    E = _random_csr(rows, cols, rot, seed)
    assert E.nnz != B0.nnz or not np.array_equal(E.indices, B0.indices)
    return E


_KOPS = {}


def _kernel_ops(ctx, name):
    """(B0, E on its pattern, E with its own pattern) as scipy matrices and device operators, built once."""
    if name not in _KOPS:
        rows, cols, lens = KERNEL_OPS[name]
        B0 = _random_csr(rows, cols, lens, seed=rows)
        Es = _same_pattern(B0, rows + 100)
        Eo = _other_pattern(B0, lens, rows + 200)
        if rows > 1:
            empty_in_E = np.diff(Eo.indptr) == 0
            assert np.any(empty_in_E & (np.diff(B0.indptr) > 0))     # an empty row of E where B0 has entries
        up = lambda M: hgmres.SparseOperator.from_scipy(M, ctx=ctx)
        _KOPS[name] = (B0, Es, Eo, up(B0), up(Es), up(Eo))
    return _KOPS[name]


def _spmm_pert_padded(ctx, Bop, Eop, coefs, X, pad):
    """hgm_spmm_pert on device buffers with leading dimensions padded by `pad`, the padding NaN; returns the
    whole (rows + pad) x nvec output buffer."""
    lib = L.load()
    m, n = Bop.shape
    nv = X.shape[1]
    ldx, ldy = n + pad, m + pad
    Xb = np.full((ldx, nv), np.nan, order="F")
    Xb[:n, :] = X
    Yb = np.full((ldy, nv), np.nan, order="F")
    cf = np.ascontiguousarray(coefs, dtype=np.float64)
    px, py = C.c_void_p(), C.c_void_p()
    try:
        for p_, cnt in ((px, ldx * nv), (py, ldy * nv)):
            assert lib.hgm_dev_alloc(ctx.handle, 8 * cnt, C.byref(p_)) == L.HGM_OK
        assert lib.hgm_memcpy_h2d(ctx.handle, px, Xb.ctypes.data_as(C.c_void_p), 8 * ldx * nv) == L.HGM_OK
        assert lib.hgm_memcpy_h2d(ctx.handle, py, Yb.ctypes.data_as(C.c_void_p), 8 * ldy * nv) == L.HGM_OK
        assert lib.hgm_spmm_pert(ctx.handle, Bop._h, Eop._h, nv, cf.ctypes.data_as(L.dp), px, ldx, py, ldy) == L.HGM_OK
        assert lib.hgm_memcpy_d2h(ctx.handle, Yb.ctypes.data_as(C.c_void_p), py, 8 * ldy * nv) == L.HGM_OK
    finally:
        for p_ in (px, py):
            if p_.value:
                lib.hgm_dev_free(ctx.handle, p_)
    return Yb


def _bound(B0, E, c, X):
    """(2 lenB_i + 2) eps (|B0||X|)_ir + |c_r| (2 lenE_i + 2) eps (|E||X|)_ir + 2 eps (|B0 X| + |c_r| |E X|)_ir:
    each product is two summations of len_i terms in different orders (test_gpu_batch.py's _bound), the
    second scaled by c_r; then the scaling and the final addition round once each, on both sides, each
    within eps of the terms' magnitudes."""
    lb = np.diff(B0.indptr).astype(np.float64)
    le = np.diff(E.indptr).astype(np.float64)
    c = np.abs(np.asarray(c, dtype=np.float64))[None, :]
    aX = np.abs(X)
    return ((2.0 * lb + 2.0)[:, None] * EPS * (abs(B0) @ aX) + c * (2.0 * le + 2.0)[:, None] * EPS * (abs(E) @ aX)
            + 2.0 * EPS * (np.abs(B0 @ X) + c * np.abs(E @ X)))


@pytest.mark.parametrize("pattern", ["same", "own"])
@pytest.mark.parametrize("name", list(KERNEL_OPS))
def test_spmm_pert_against_scipy(gpu_ctx, name, pattern):
    rows, cols, _ = KERNEL_OPS[name]
    B0, Es, Eo, Bop, Esop, Eoop = _kernel_ops(gpu_ctx, name)
    E, Eop = (Es, Esop) if pattern == "same" else (Eo, Eoop)
    Xall = np.random.default_rng(rows + 1).standard_normal((cols, 8))
    for nv in range(1, 9):                                   # 3, 5, 6, 7 run with zero slots
        X, c = Xall[:, :nv], COEFS8[:nv]
        Yb = _spmm_pert_padded(gpu_ctx, Bop, Eop, c, X, 6)
        got, padding = Yb[:rows, :], Yb[rows:, :]
        assert np.all(np.isfinite(got)), (name, nv)
        assert np.all(np.isnan(padding)), (name, nv)          # nothing written past the rows
        ref = B0 @ X + (E @ X) * c
        excess = np.abs(got - ref) - _bound(B0, E, c, X)
        assert np.all(excess <= 0), (name, pattern, nv, excess.max())


@pytest.mark.parametrize("name", list(KERNEL_OPS))
def test_spmm_pert_is_the_two_products_combined(gpu_ctx, name):
    """Same-pattern E: bit-equal to spmm(B0, X) + c * spmm(E, X) formed in numpy (two roundings), on the
    shared path and on the general one; c = 0 gives spmm(B0, X)."""
    rows, cols, _ = KERNEL_OPS[name]
    B0, Es, Eo, Bop, Esop, Eoop = _kernel_ops(gpu_ctx, name)
    X = np.random.default_rng(rows + 2).standard_normal((cols, 8))
    YB, YE = hgmres.spmm(Bop, X), hgmres.spmm(Esop, X)
    two = YB + COEFS8[None, :] * YE
    shared = hgmres.spmm_pert(Bop, Esop, COEFS8, X)
    assert np.array_equal(shared, two)
    with gpu_ctx.options(pert_shared=0):
        general = hgmres.spmm_pert(Bop, Esop, COEFS8, X)
        zero_general = hgmres.spmm_pert(Bop, Eoop, np.zeros(8), X)
    assert np.array_equal(general, shared)                   # option 39 = 0: the same bits
    assert np.array_equal(hgmres.spmm_pert(Bop, Esop, np.zeros(8), X), YB)
    assert np.array_equal(hgmres.spmm_pert(Bop, Eoop, np.zeros(8), X), YB)
    assert np.array_equal(zero_general, YB)


@pytest.mark.parametrize("pattern", ["same", "own"])
def test_spmm_pert_bitwise_invariance(gpu_ctx, pattern):
    """A column's bits do not depend on the vector count, its slot, the other columns or their coefficients."""
    B0, Es, Eo, Bop, Esop, Eoop = _kernel_ops(gpu_ctx, "rows1000_wide")
    Eop = Esop if pattern == "same" else Eoop
    X = np.random.default_rng(6).standard_normal((B0.shape[1], 8))
    c = COEFS8
    Y8 = hgmres.spmm_pert(Bop, Eop, c, X)
    assert np.array_equal(Y8, hgmres.spmm_pert(Bop, Eop, c, X))           # two identical calls
    for r in range(8):
        a, b = (r + 1) % 8, (r + 5) % 8
        assert np.array_equal(hgmres.spmm_pert(Bop, Eop, c[[r]], X[:, [r]])[:, 0], Y8[:, r]), r                   # alone
        assert np.array_equal(hgmres.spmm_pert(Bop, Eop, c[[r, a, b]], X[:, [r, a, b]])[:, 0], Y8[:, r]), r       # slot 0
        assert np.array_equal(hgmres.spmm_pert(Bop, Eop, c[[a, b, r]], X[:, [a, b, r]])[:, 2], Y8[:, r]), r       # last of 3
    perm = [1, 2, 3, 4, 5, 6, 7, 0]
    assert np.array_equal(hgmres.spmm_pert(Bop, Eop, c[perm], X[:, perm])[:, 7], Y8[:, 0])                        # last of 8
    other = c[::-1].copy()                                   # inside a group of 8 with other coefficients
    for r in (0, 3, 7):
        other[r] = c[r]
        assert np.array_equal(hgmres.spmm_pert(Bop, Eop, other, X)[:, r], Y8[:, r]), r


def test_spmm_pert_tiled_pair(gpu_ctx):
    """B0 = A' of a Siddon operator stored in 4 x 4 tiles and 16 x 16 super-blocks, E = the transpose of random
    values on A's pattern in the same stored order: the columns leave in the stored pixel order."""
    A = hgmres.SparseOperator.siddon(32, 16, gpu_ctx, order=(4, 16))
    S = A.to_scipy()
    S.sort_indices()
    Ev = _same_pattern(S, 9)
    EA = hgmres.SparseOperator.from_scipy_tiled(Ev, 32, 4, 16, ctx=gpu_ctx)
    B0, E = A.T, EA.T
    assert E.pixel_order("rows") == B0.pixel_order("rows") and B0.pixel_order("rows")[1:] == (4, 16)
    Bs, Es = sp.csr_matrix(S.T), sp.csr_matrix(Ev.T)
    X = np.random.default_rng(3).standard_normal((B0.shape[1], 5))
    c = COEFS8[:5]
    Y = hgmres.spmm_pert(B0, E, c, X)
    assert np.all(np.abs(Y - (Bs @ X + (Es @ X) * c)) <= _bound(Bs, Es, c, X))
    assert np.array_equal(Y, hgmres.spmm(B0, X) + c[None, :] * hgmres.spmm(E, X))
    with gpu_ctx.options(pert_shared=0):
        assert np.array_equal(hgmres.spmm_pert(B0, E, c, X), Y)


# ---------------------------------------------------------------------------------------------
# 2. the sweep against the oracle and the single solvers, level by level
# ---------------------------------------------------------------------------------------------
def _mismatch_E(B, seed=21):
    """Random normal values on B's pattern, scaled to ||E||_F = 1."""
    v = np.random.default_rng(seed).standard_normal(B.nnz)
    return sp.csr_matrix((v / np.linalg.norm(v), B.indices.copy(), B.indptr.copy()), shape=B.shape)


@pytest.fixture(scope="module")
def problems(gpu_ctx):
    out = {}
    for name in FIXTURES:
        A, B, b, xt, _ = golden_problem(name)
        A.sort_indices()
        B.sort_indices()
        E = _mismatch_E(B)
        coefs = np.logspace(-4, 0, NCOEF) * np.linalg.norm(B.data)
        up = lambda M: hgmres.SparseOperator.from_scipy(M, ctx=gpu_ctx)
        out[name] = dict(A=A, B=B, E=E, b=b, xt=xt, coefs=coefs, Ao=up(A), Bo=up(B), Eo=up(E),
                         Bc=[sp.csr_matrix(B + c * E) for c in coefs])
    return out


_ORACLE_CACHE = {}


def _oracle_sweep(problems, name, side, hybrid, cgs2=False):
    """The oracle's solver once per level on the explicit B + c_j E (computed once per case), and the checks
    on the oracle's own result: the stopping tolerance spreads the levels (at least two distinct niters, at
    least one below maxit) and no residual-history entry lies within 1e-6 (relative) of it."""
    key = (name, side, hybrid, cgs2)
    if key not in _ORACLE_CACHE:
        P = problems[name]
        ref = []
        for j in range(NCOEF):
            args = (P["A"], P["Bc"][j], P["b"], P["xt"], STOP, MAXIT) + ((LAMS[j],) if hybrid else ())
            ref.append(ORACLE[(side, hybrid)](*args, return_H=True)[:5])
        _ORACLE_CACHE[key] = ref
    ref = _ORACLE_CACHE[key]
    nit = [r[3] for r in ref]
    assert len(set(nit)) >= 2 and min(nit) < MAXIT, nit
    margin = min(np.min(np.abs(np.asarray(r[2]) - STOP)) for r in ref) / STOP
    assert margin >= 1e-6, margin
    return ref


def _check_against_oracle(Rb, ref):
    assert np.all(Rb.status == L.HGM_OK)
    for j, (x, e, r, k, H) in enumerate(ref):
        assert Rb.niters[j] == k, (j, Rb.niters[j], k)
        hist_ok(Rb.residual_norm[:, j], padded_hist(r), TOL)
        hist_ok(Rb.error_norm[:, j], padded_hist(e), TOL)
        assert rel(Rb.x[:, j], x) <= TOL, j
        assert np.max(np.abs(Rb.H[j] - H)) <= TOL * np.max(np.abs(H)), j


def _sweep(P, ctx, side, hybrid, cols=None, **kw):
    cols = slice(None) if cols is None else cols
    return hgmres.gmres_bounds_mismatch(P["Ao"], P["Bo"], P["Eo"], P["coefs"][cols], P["b"], P["xt"], STOP, MAXIT, side,
                                        lambdas=LAMS[cols] if hybrid else None, ctx=ctx, return_H=True, **kw)


@pytest.mark.parametrize("side,hybrid", CASES)
@pytest.mark.parametrize("name", FIXTURES)
def test_mismatch_matches_oracle(gpu_ctx, problems, name, side, hybrid):
    ref = _oracle_sweep(problems, name, side, hybrid)
    _check_against_oracle(_sweep(problems[name], gpu_ctx, side, hybrid), ref)


def test_mismatch_cgs2_matches_oracle_cgs2(gpu_ctx, problems, monkeypatch):
    """orth = 'cgs2' against the oracle's solver with its CGS2 Arnoldi step in place of MGS."""
    monkeypatch.setattr(R, "_mgs_arnoldi_step", R._cgs2_arnoldi_step)
    ref = _oracle_sweep(problems, "tomo24_pixel.npz", "ab", True, cgs2=True)
    _check_against_oracle(_sweep(problems["tomo24_pixel.npz"], gpu_ctx, "ab", True, orth="cgs2"), ref)


@pytest.mark.parametrize("side,hybrid", CASES)
@pytest.mark.parametrize("name", FIXTURES)
def test_mismatch_matches_single_solver(gpu_ctx, problems, name, side, hybrid):
    """The same sweep against the library's own single solvers on uploaded explicit B + c_j E (the loop the
    sweep replaces)."""
    P = problems[name]
    _oracle_sweep(problems, name, side, hybrid)              # the spread of niters holds
    Rb = _sweep(P, gpu_ctx, side, hybrid)
    for j in range(NCOEF):
        Bj = hgmres.SparseOperator.from_scipy(P["Bc"][j], ctx=gpu_ctx)
        args = (P["Ao"], Bj, P["b"], P["xt"], STOP, MAXIT) + ((LAMS[j],) if hybrid else ())
        out = SINGLE[(side, hybrid)](*args, ctx=gpu_ctx, return_H=True)
        (x, e, r, k), H = out[:4], out[-1]
        assert Rb.niters[j] == k
        hist_ok(Rb.residual_norm[:, j], padded_hist(r), TOL)
        hist_ok(Rb.error_norm[:, j], padded_hist(e), TOL)
        assert rel(Rb.x[:, j], x) <= TOL
        assert np.max(np.abs(Rb.H[j] - H)) <= TOL * np.max(np.abs(H))
        Bj.close()


# ---------------------------------------------------------------------------------------------
# 3. composition, bitwise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", False)])
def test_mismatch_equals_its_levels_alone(gpu_ctx, problems, side, hybrid):
    P = problems["tomo24_pixel.npz"]
    Rb = _sweep(P, gpu_ctx, side, hybrid)
    assert len(set(Rb.niters)) >= 2                          # levels left the sweep at different steps
    for j in range(NCOEF):
        same_batch(Rb, _sweep(P, gpu_ctx, side, hybrid, cols=[j]), [j], [0])
    with gpu_ctx.options(pert_shared=0):                     # the general path: the same bits
        same_batch(Rb, _sweep(P, gpu_ctx, side, hybrid))


def test_mismatch_of_two_groups_equals_its_levels_alone(gpu_ctx, problems):
    """11 levels: two packed groups (8 + 3), regrouped (coefficients with them) as levels finish."""
    P = problems["tomo24_matched.npz"]
    coefs = np.logspace(-4, 0, 11) * np.linalg.norm(P["B"].data)
    lams = np.logspace(-2, 2, 11)
    run = lambda cols: hgmres.gmres_bounds_mismatch(P["Ao"], P["Bo"], P["Eo"], coefs[cols], P["b"], P["xt"], STOP, MAXIT,
                                                    "ab", lambdas=lams[cols], ctx=gpu_ctx, return_H=True)
    Rb = run(slice(None))
    assert len(set(Rb.niters)) >= 2 and min(Rb.niters) < MAXIT
    for j in range(11):
        same_batch(Rb, run([j]), [j], [0])


@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", True), ("ab", False)])
def test_zero_coefficients_equal_the_batch_of_replicated_b(gpu_ctx, problems, side, hybrid):
    P = problems["tomo24_matched.npz"]
    lam = LAMS if hybrid else None
    a = hgmres.gmres_bounds_mismatch(P["Ao"], P["Bo"], P["Eo"], np.zeros(NCOEF), P["b"], P["xt"], STOP, MAXIT, side,
                                     lambdas=lam, ctx=gpu_ctx, return_H=True)
    Bm = np.repeat(P["b"][:, None], NCOEF, axis=1)
    b = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], Bm, P["xt"], STOP, MAXIT, side, lambdas=lam, ctx=gpu_ctx, return_H=True)
    same_batch(a, b)
    assert np.all(np.isfinite(a.x))


# ---------------------------------------------------------------------------------------------
# 4. the lockstep GCV Arnoldi
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["ab", "ba"])
def test_arnoldi_mismatch(gpu_ctx, problems, side):
    P = problems["tomo24_pixel.npz"]
    k = 8
    H, beta, kd = hgmres.arnoldi_mismatch(P["Ao"], P["Bo"], P["Eo"], P["coefs"], P["b"], k, side, ctx=gpu_ctx)
    assert H.shape == (NCOEF, k + 1, k) and beta.shape == (NCOEF,) and np.all(kd == k)
    for j in range(NCOEF):
        Bj = hgmres.SparseOperator.from_scipy(P["Bc"][j], ctx=gpu_ctx)
        H1, b1, k1 = hgmres.arnoldi(P["Ao"], Bj, P["b"], k, side, ctx=gpu_ctx)
        Bj.close()
        Hr, br = R.arnoldi(P["A"], P["Bc"][j], P["b"], k, side)
        for Href, bref in ((H1, b1), (Hr, br)):
            assert np.max(np.abs(H[j] - Href)) <= TOL * np.max(np.abs(Href)), j
            assert abs(beta[j] - bref) <= TOL * abs(bref), j
        assert k1 == k
        Ha, ba, ka = hgmres.arnoldi_mismatch(P["Ao"], P["Bo"], P["Eo"], P["coefs"][[j]], P["b"], k, side, ctx=gpu_ctx)
        assert np.array_equal(Ha[0], H[j]) and ba[0] == beta[j] and ka[0] == kd[j]       # the level alone


# ---------------------------------------------------------------------------------------------
# 5. breakdown
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["ab", "ba"])
def test_mismatch_empty_operator_breaks_every_level(gpu_ctx, side):
    """An all-zero A (test_gpu_batch.py's empty operator): H(2,1) = 0 at the first step of every level."""
    A = sp.csr_matrix((6, 4))
    B = sp.csr_matrix(np.ones((4, 6)))
    E = sp.csr_matrix(np.arange(1.0, 25.0).reshape(4, 6))
    b = np.arange(1.0, 7.0)
    xt = np.ones(4)
    Ao, Bo, Eo = (hgmres.as_operator(M, gpu_ctx) for M in (A, B, E))
    lib = L.load()
    X = np.full((4, 3), 7.0, order="F")
    err, res = np.zeros((3, 3), order="F"), np.zeros((3, 3), order="F")
    nit, st = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    lam = np.array([0.5, 1.0, 2.0])
    cf = np.array([0.0, 0.1, -3.0])
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp)
    rc = lib.hgm_gmres_bounds_mismatch(gpu_ctx.handle, None, Ao._h, Bo._h, Eo._h, dp(cf), 3, dp(b), dp(xt), 1e-2, 3,
                                       dp(lam), L.HGM_SIDE_AB if side == "ab" else L.HGM_SIDE_BA, 1, dp(X), 4, dp(err),
                                       dp(res), nit.ctypes.data_as(ip), st.ctypes.data_as(ip))
    assert rc == L.HGM_E_NOT_ASSIGNED
    assert np.all(st == L.HGM_E_NOT_ASSIGNED) and np.all(nit == 1)
    assert np.all(X == 7.0)                                  # the X columns are left untouched
    Rb = hgmres.gmres_bounds_mismatch(Ao, Bo, Eo, cf, b, xt, 1e-2, 3, side, lambdas=lam, ctx=gpu_ctx)
    assert np.all(Rb.status == L.HGM_E_NOT_ASSIGNED) and np.all(Rb.niters == 1) and np.all(np.isnan(Rb.x))


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def test_mismatch_refusals(gpu_ctx, problems):
    P = problems["tomo24_matched.npz"]
    A, B, E, b, xt = P["Ao"], P["Bo"], P["Eo"], P["b"], P["xt"]
    lib = L.load()
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp) if a is not None else None
    m, n = A.shape
    cf2 = np.array([0.1, 0.2])

    def solve(ctx, Ah, Bh, Eh, cf, lam, hybrid, flags=0):
        o = L.hgm_opts()
        o.flags, o.orth, o.H_out = flags, L.HGM_MGS, None
        nc = 0 if cf is None else cf.size
        nit = np.zeros(max(nc, 1), dtype=np.int32)
        return lib.hgm_gmres_bounds_mismatch(ctx.handle, C.byref(o), Ah, Bh, Eh, dp(cf), nc, dp(b), dp(xt), 0.0, 3, dp(lam),
                                             L.HGM_SIDE_AB, hybrid, None, n, None, None, nit.ctypes.data_as(ip), None)

    def arn(ctx, Ah, Bh, Eh, cf):
        nc = cf.size
        H, beta, kd = np.zeros(4 * 3 * max(nc, 1)), np.zeros(max(nc, 1)), np.zeros(max(nc, 1), dtype=np.int32)
        return lib.hgm_arnoldi_mismatch(ctx.handle, Ah, Bh, Eh, dp(cf), nc, dp(b), 3, L.HGM_SIDE_BA, 1e-12, L.HGM_MGS,
                                        dp(H), dp(beta), kd.ctypes.data_as(ip))

    A32 = hgmres.as_operator(P["A"], gpu_ctx, dtype=L.HGM_F32)
    E32 = hgmres.as_operator(P["E"], gpu_ctx, dtype=L.HGM_F32)
    for call in (lambda *a: solve(*a, None, 0), arn):
        assert call(gpu_ctx, A32._h, A32.T._h, E32._h, cf2) == L.HGM_E_ARG               # fp32 operators
        assert call(gpu_ctx, A._h, B._h, E32._h, cf2) == L.HGM_E_ARG                     # fp32 E
        with gpu_ctx.options(parity=1):
            assert call(gpu_ctx, A._h, B._h, E._h, cf2) == L.HGM_E_ARG                   # parity mode
        assert call(gpu_ctx, A._h, B._h, E._h, np.zeros(0)) == L.HGM_E_ARG               # ncoef < 1
        assert call(gpu_ctx, A._h, B._h, E._h, np.linspace(0, 1, 65)) == L.HGM_E_ARG     # ncoef > 64
        for bad in (np.nan, np.inf, -np.inf):
            assert call(gpu_ctx, A._h, B._h, E._h, np.array([0.1, bad])) == L.HGM_E_ARG  # non-finite coefficient
    assert solve(gpu_ctx, A._h, B._h, E._h, cf2, None, 0, flags=L.HGM_DEVICE_PTRS) == L.HGM_E_ARG   # device pointers
    for bad in (-1.0, np.nan, np.inf):
        assert solve(gpu_ctx, A._h, B._h, E._h, cf2, np.array([1.0, bad]), 1) == L.HGM_E_ARG        # bad lambda (hybrid)
        assert solve(gpu_ctx, A._h, B._h, E._h, cf2, np.array([1.0, bad]), 0) == L.HGM_OK           # ignored otherwise
    assert solve(gpu_ctx, A._h, B._h, E._h, cf2, None, 1) == L.HGM_E_ARG                            # hybrid needs lambdas
    # E of another shape
    Ebad = hgmres.as_operator(sp.csr_matrix((n, m + 1)), gpu_ctx)
    assert solve(gpu_ctx, A._h, B._h, Ebad._h, cf2, None, 0) == L.HGM_E_ARG
    assert arn(gpu_ctx, A._h, B._h, Ebad._h, cf2) == L.HGM_E_ARG
    with pytest.raises(ValueError, match="shape"):
        hgmres.spmm_pert(B, Ebad, cf2, np.ones((m, 2)))
    px = C.c_void_p(8)
    assert lib.hgm_spmm_pert(gpu_ctx.handle, B._h, Ebad._h, 2, dp(cf2), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert(gpu_ctx.handle, B._h, E._h, 9, dp(np.zeros(9)), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert(gpu_ctx.handle, B._h, E._h, 2, dp(np.array([1.0, np.nan])), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert(gpu_ctx.handle, B._h, E32._h, 2, dp(cf2), px, m, px, n) == L.HGM_E_ARG
    # E of B0's shape in another stored order: B0 = A' tiled (4, 16), E = the same values' transpose untiled
    At = hgmres.SparseOperator.siddon(32, 16, gpu_ctx, order=(4, 16))
    S = At.to_scipy()
    Eu = hgmres.SparseOperator.from_scipy(S, ctx=gpu_ctx).T
    assert Eu.shape == At.T.shape and Eu.pixel_order("rows") != At.T.pixel_order("rows")
    bt = np.ones(At.shape[0])
    nit = np.zeros(2, dtype=np.int32)
    assert lib.hgm_gmres_bounds_mismatch(gpu_ctx.handle, None, At._h, At.T._h, Eu._h, dp(cf2), 2, dp(bt), None, 0.0, 3, None,
                                         L.HGM_SIDE_AB, 0, None, At.shape[1], None, None, nit.ctypes.data_as(ip),
                                         None) == L.HGM_E_ARG
    pb = C.c_void_p(8)
    assert lib.hgm_spmm_pert(gpu_ctx.handle, At.T._h, Eu._h, 2, dp(cf2), pb, At.shape[0], pb, At.shape[1]) == L.HGM_E_ARG
    # a context with a host all-reduce hook at world 2: HGM_E_UNSUPPORTED, and the hook is never called
    calls = []
    c2 = hgmres.Context(0)
    try:
        c2.set_host_allreduce(0, 2, lambda arr: calls.append(arr.size))
        A2 = hgmres.as_operator(P["A"], c2)
        B2 = hgmres.as_operator(P["B"], c2)
        E2 = hgmres.as_operator(P["E"], c2)
        assert solve(c2, A2._h, B2._h, E2._h, cf2, None, 0) == L.HGM_E_UNSUPPORTED
        assert arn(c2, A2._h, B2._h, E2._h, cf2) == L.HGM_E_UNSUPPORTED
        assert calls == []
    finally:
        c2.close()
    # the context still solves after the refusals
    Rb = hgmres.gmres_bounds_mismatch(A, B, E, cf2, b, xt, 0.0, 3, "ab", ctx=gpu_ctx)
    assert np.all(Rb.niters == 3) and np.all(np.isfinite(Rb.x))


# ---------------------------------------------------------------------------------------------
# 7. pipeline and gateway
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gcv", [False, True])
def test_error_vs_mismatch_norm_matches_solver_loop(gpu_ctx, problems, gcv):
    P = problems["tomo24_matched.npz"]
    cr = P["coefs"][:4]
    lam_in = None if gcv else (np.array([1e-2, 0.1, 1.0, 10.0]), np.array([0.05, 0.5, 5.0, 50.0]))
    M = analysis.error_vs_mismatch_norm(P["Ao"], P["Bo"], P["Eo"], P["b"], P["xt"], cr, maxit=8, tol=0.05, k_gcv=8,
                                        lambdas=lam_in, solvers=("hab", "hba", "nab", "nba"), ctx=gpu_ctx)
    assert np.allclose(M["mismatch_norms"], np.abs(cr) * 1.0, rtol=1e-14)       # ||E||_F = 1
    if gcv:
        for side in ("ab", "ba"):
            trace_m = P["A"].shape[0] if side == "ab" else P["A"].shape[1]
            H, beta, _ = hgmres.arnoldi_mismatch(P["Ao"], P["Bo"], P["Eo"], cr, P["b"], 8, side, ctx=gpu_ctx)
            for i in range(4):
                assert M[f"lambda_gcv_{side}"][i] == hgmres.gcv_fminbnd(H[i], beta[i], trace_m, 1e-9, 1e-1, 1e-8)[0]
    else:
        assert np.array_equal(M["lambda_gcv_ab"], lam_in[0]) and np.array_equal(M["lambda_gcv_ba"], lam_in[1])
    Bj = [hgmres.SparseOperator.from_scipy(P["Bc"][i], ctx=gpu_ctx) for i in range(4)]
    for key, side, hybrid in (("hab", "ab", True), ("hba", "ba", True), ("nab", "ab", False), ("nba", "ba", False)):
        fin = np.zeros(4)
        for i in range(4):
            lam = (M[f"lambda_gcv_{side}"][i],) if hybrid else ()
            fin[i] = SINGLE[(side, hybrid)](P["Ao"], Bj[i], P["b"], P["xt"], 0.05, 8, *lam, ctx=gpu_ctx)[1][-1]
        hist_ok(M[f"final_errors_{key}"], fin, TOL)
    for o in Bj:
        o.close()


def test_error_vs_mismatch_norm_smoke_on_heat(gpu_ctx):
    """plot_error_vs_mismatch_norm.m's own problem (heat, n = 32, a dense E): shapes and finiteness only."""
    A, b_exact, x_true = generate_test_problem("heat", 32)
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(b_exact.shape)
    b = b_exact + noise / np.linalg.norm(noise) * 1e-2 * np.linalg.norm(b_exact)
    E = rng.standard_normal(A.T.shape)
    E /= np.linalg.norm(E)
    cr = np.logspace(-8, -1, 20)
    M = analysis.error_vs_mismatch_norm(sp.csr_matrix(A), sp.csr_matrix(A.T), E, b, x_true, cr, maxit=32, ctx=gpu_ctx)
    assert M["mismatch_norms"].shape == (20,) and np.allclose(M["mismatch_norms"], cr)
    for side in ("ab", "ba"):
        lam = M[f"lambda_gcv_{side}"]
        assert lam.shape == (20,) and np.all((lam >= 1e-9) & (lam <= 1e-1))
    for key in ("hab", "hba"):
        assert M[f"final_errors_{key}"].shape == (20,) and np.all(np.isfinite(M[f"final_errors_{key}"]))
        assert np.all((M[f"niters_{key}"] >= 1) & (M[f"niters_{key}"] <= 32))
    assert "final_errors_nab" not in M


def test_matlab_command_equals_python_call(gpu_ctx, problems):
    """matlab/gmres_bounds_mismatch.m through the gateway (the mx API stand-in) against the Python binding."""
    from mwrap import Function
    from test_mex_gateway import Mex
    P = problems["tomo24_pixel.npz"]
    A, B, E = P["A"], P["B"], P["E"]
    f = Function(os.path.join(ROOT, "matlab", "gmres_bounds_mismatch.m"), Mex())
    for side, lam in (("ab", LAMS), ("ba", None)):
        Rb = hgmres.gmres_bounds_mismatch(A, B, E, P["coefs"], P["b"], P["xt"], STOP, MAXIT, side, lambdas=lam, ctx=gpu_ctx)
        args = (sp.csc_matrix(A), sp.csc_matrix(B), sp.csc_matrix(E), P["coefs"], P["b"], P["xt"], STOP, float(MAXIT), side)
        X, e, r, ni, st = f(5, *(args + ((lam,) if lam is not None else ())))
        assert X.shape == Rb.x.shape and e.shape == r.shape == (MAXIT, NCOEF)
        assert np.array_equal(ni.reshape(-1).astype(int), Rb.niters) and np.all(st == 0)
        assert np.array_equal(X, Rb.x)
        assert np.array_equal(e, Rb.error_norm, equal_nan=True) and np.array_equal(r, Rb.residual_norm, equal_nan=True)
