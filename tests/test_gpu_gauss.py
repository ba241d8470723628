"""The matrix-free dense Gaussian back-projector perturbation (hgm_gauss_*, csrc/gauss.hip) on the device.

* the generator against its numpy twin (hgmres.problems.gaussian_entries), entry by entry, at 16 eps relative;
* the product G X against the twin's dense product at a derived bound, bit-invariant under the vector count, the
  slot, the neighbours and their coefficients, and bit-equal to its parts inside hgm_spmm_pert_gauss;
* a tiled (stored pixel order) B0 against the reference-order one: the same bits for the G part;
* the lockstep sweeps with G for E against the oracle's ``*_bounds`` solvers on the explicit dense
  ``B + c_j E_twin``, against the sparse path with E uploaded as a dense CSR, and against themselves bitwise;
* the lockstep GCV Arnoldi, breakdown, refusals, the pipeline and the gateway command.

The constants and helpers of the sweep tests are those of test_gpu_mismatch.py (copied: that file stays as it
is)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, golden_problem
import hgmres
from hgmres import _lib as L
from hgmres import analysis
from hgmres.problems import gaussian_entries, tomo_problem
from hgmres.regtools import generate_test_problem
from oracle import restatement as R   # checker only
from tiled_pair import tiled_pair

pytestmark = pytest.mark.gpu

TOL = 1e-10                      # the project's bar (tests/test_gpu_sweep.py)
EPS = np.finfo(np.float64).eps
MAXIT = 12
NCOEF = 5
LAMS = np.array([1e-2, 1e-1, 1.0, 10.0, 100.0])
# With E = GaussianPerturbation(576, 408, seed=21).normalized() the oracle's residual histories of the five levels
# cross 1.7e-2 at different iterations in all eight (fixture, side, hybrid) cases, no entry closer to it than
# 5e-3 relative (checked on the CPU with the twin); _oracle_sweep asserts the spread and a 1e-6 margin.
STOP = 1.7e-2
FIXTURES = ("tomo24_matched.npz", "tomo24_pixel.npz")
ORACLE = {("ab", True): R.ABgmres_hybrid_bounds, ("ba", True): R.BAgmres_hybrid_bounds,
          ("ab", False): R.ABgmres_nonhybrid_bounds, ("ba", False): R.BAgmres_nonhybrid_bounds}
SINGLE = {("ab", True): hgmres.ABgmres_hybrid_bounds, ("ba", True): hgmres.BAgmres_hybrid_bounds,
          ("ab", False): hgmres.ABgmres_nonhybrid_bounds, ("ba", False): hgmres.BAgmres_nonhybrid_bounds}
CASES = [("ab", True), ("ba", True), ("ab", False), ("ba", False)]
COEFS8 = np.array([0.5, -2.0, 1e-3, 0.0, 7.25, -1e2, 1.0, 3e-7])
SEED = 0x9e3779b97f4a7c15          # both key words in use


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
# 1. entries
# ---------------------------------------------------------------------------------------------
_TWIN = {}


def twin(rows, cols, seed=SEED):
    """The twin's rows x cols matrix: up to 1000 x 5003 the top-left block of that one (an entry depends on
    (seed, i, j) alone), which is computed once per seed."""
    if rows > 1000 or cols > 5003:
        return gaussian_entries(rows, cols, seed)
    if seed not in _TWIN:
        _TWIN[seed] = gaussian_entries(1000, 5003, seed)
    return _TWIN[seed][:rows, :cols]


def entries_ok(got, want):
    """|dg| <= 16 eps |g_twin|: log <= 1 ulp (halved by the sqrt), sqrt 1/2, sincospi <= 2, the product 1/2, on
    each side -- about 8 eps; the bar is twice that."""
    assert got.shape == want.shape
    bad = np.abs(got - want) > 16 * EPS * np.abs(want)
    assert not np.any(bad), (int(bad.sum()), np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (64, 256), (65, 257), (1000, 5003)])
def test_entries_match_the_twin(gpu_ctx, rows, cols):
    G = hgmres.GaussianPerturbation(rows, cols, SEED, ctx=gpu_ctx)
    assert G.shape == (rows, cols) and G.seed == SEED
    r, c, s = C.c_int64(), C.c_int64(), C.c_uint64()
    assert L.load().hgm_gauss_info(G._h, C.byref(r), C.byref(c), C.byref(s)) == L.HGM_OK
    assert (r.value, c.value, s.value) == (rows, cols, SEED)
    E = G.to_dense()
    entries_ok(E, twin(rows, cols))
    assert np.array_equal(E, G.entries())                        # repeatable
    G.close()


def test_entry_windows(gpu_ctx):
    """Windows at offsets not divisible by 4 are slices of the whole, bit for bit; leading dimension padding is
    left alone."""
    G = hgmres.GaussianPerturbation(65, 257, SEED, ctx=gpu_ctx)
    full = G.to_dense()
    for rs, cs in [(slice(0, 65), slice(1, 2)), (slice(3, 9), slice(5, 11)), (slice(64, 65), slice(254, 257)),
                   (slice(10, 40), slice(7, 202)), (slice(0, 1), slice(0, 1)), (slice(2, 2), slice(0, 4))]:
        assert np.array_equal(G.entries(rs, cs), full[rs, cs])
    out = np.full((9, 3), np.nan, order="F")
    assert L.load().hgm_gauss_entries(gpu_ctx.handle, G._h, 5, 6, 2, 3, out.ctypes.data_as(L.dp), 9) == L.HGM_OK
    assert np.array_equal(out[:6], full[5:11, 2:5]) and np.all(np.isnan(out[6:]))
    assert np.array_equal((G._with_scale(-0.25)).entries(slice(3, 9), slice(5, 11)), full[3:9, 5:11] * -0.25)


def test_entries_split_the_counter_at_64_bits(gpu_ctx):
    """A 16 x 16 window at i0 = 2^32 + 3, j0 = 2^34 + 6 of a 2^33 x 2^35 handle (no product runs on it)."""
    G = hgmres.GaussianPerturbation(1 << 33, 1 << 35, 9, ctx=gpu_ctx)
    i0, j0 = (1 << 32) + 3, (1 << 34) + 6
    E = G.entries(slice(i0, i0 + 16), slice(j0, j0 + 16))
    entries_ok(E, gaussian_entries(1 << 33, 1 << 35, 9, i0, 16, j0, 16))
    low = G.entries(slice(3, 19), slice(6, 22))
    entries_ok(low, gaussian_entries(1 << 33, 1 << 35, 9, 3, 16, 6, 16))
    assert not np.array_equal(E, low)
    with pytest.raises(ValueError):
        G.to_dense()


def test_seeds_that_differ_in_the_high_word(gpu_ctx):
    a = hgmres.GaussianPerturbation(16, 16, 5, ctx=gpu_ctx).to_dense()
    b = hgmres.GaussianPerturbation(16, 16, 5 + (1 << 32), ctx=gpu_ctx).to_dense()
    assert not np.array_equal(a, b)
    entries_ok(b, gaussian_entries(16, 16, 5 + (1 << 32)))


# ---------------------------------------------------------------------------------------------
# 2. product
# ---------------------------------------------------------------------------------------------
def _mm_padded(ctx, G, X, pad, coefs=None, B0=None):
    """hgm_gauss_mm (or, with B0, hgm_spmm_pert_gauss) on device buffers with leading dimensions padded by `pad`,
    the padding NaN; returns the whole (rows + pad) x nvec output buffer."""
    lib = L.load()
    m, n = G.shape
    nv = X.shape[1]
    ldx, ldy = n + pad, m + pad
    Xb = np.full((ldx, nv), np.nan, order="F")
    Xb[:n, :] = X
    Yb = np.full((ldy, nv), np.nan, order="F")
    cf = None if coefs is None else np.ascontiguousarray(coefs, dtype=np.float64)
    cp = None if cf is None else cf.ctypes.data_as(L.dp)
    px, py = C.c_void_p(), C.c_void_p()
    try:
        for p_, cnt in ((px, ldx * nv), (py, ldy * nv)):
            assert lib.hgm_dev_alloc(ctx.handle, 8 * cnt, C.byref(p_)) == L.HGM_OK
        assert lib.hgm_memcpy_h2d(ctx.handle, px, Xb.ctypes.data_as(C.c_void_p), 8 * ldx * nv) == L.HGM_OK
        assert lib.hgm_memcpy_h2d(ctx.handle, py, Yb.ctypes.data_as(C.c_void_p), 8 * ldy * nv) == L.HGM_OK
        if B0 is None:
            assert lib.hgm_gauss_mm(ctx.handle, G._h, nv, cp, px, ldx, py, ldy) == L.HGM_OK
        else:
            assert lib.hgm_spmm_pert_gauss(ctx.handle, B0._h, G._h, nv, cp, px, ldx, py, ldy) == L.HGM_OK
        assert lib.hgm_memcpy_d2h(ctx.handle, Yb.ctypes.data_as(C.c_void_p), py, 8 * ldy * nv) == L.HGM_OK
    finally:
        for p_ in (px, py):
            if p_.value:
                lib.hgm_dev_free(ctx.handle, p_)
    return Yb


def _product_check(ctx, rows, cols, Gt):
    """G X against the twin's dense product in long double for every vector count 1..8 (3, 5, 6, 7 run with zero
    slots), NaN-padded leading dimensions.  Bound: (2 cols + 2 + 16) eps (|G||X|): two summations of `cols`
    terms in different orders and the final scaling (test_gpu_batch.py's bound), plus the entries' 16 eps."""
    G = hgmres.GaussianPerturbation(rows, cols, SEED, ctx=ctx)
    Xall = np.random.default_rng(rows * 7919 + cols).standard_normal((cols, 8))
    ref = (Gt.astype(np.longdouble) @ Xall.astype(np.longdouble))
    bound = (2.0 * cols + 2.0 + 16.0) * EPS * (np.abs(Gt) @ np.abs(Xall))
    for nv in range(1, 9):
        Yb = _mm_padded(ctx, G, Xall[:, :nv], 5)
        got, padding = Yb[:rows], Yb[rows:]
        assert np.all(np.isfinite(got)), (rows, cols, nv)
        assert np.all(np.isnan(padding)), (rows, cols, nv)         # nothing written past the rows
        excess = np.abs((got.astype(np.longdouble) - ref[:, :nv]).astype(np.float64)) - bound[:, :nv]
        assert np.all(excess <= 0), (rows, cols, nv, excess.max())
    G.close()


# cols: the quad tail (1, 3, 5), one quad (4), the 64-lane x 4 stride edges (255, 256, 257), several strides with
# a tail (1027, 5003)
@pytest.mark.parametrize("cols", [1, 3, 4, 5, 255, 256, 257, 1027, 5003])
@pytest.mark.parametrize("rows", [1, 7, 64, 65, 1000])
def test_product_against_the_twin(gpu_ctx, rows, cols):
    _product_check(gpu_ctx, rows, cols, twin(rows, cols))


def test_product_of_many_row_blocks(gpu_ctx):
    """The kernel tiles the rows (4 per wave, 16 per block, no grid stride): 70,001 rows are 4,376 blocks, the last
    with one row; 9 columns."""
    rows, cols = 70001, 9
    _product_check(gpu_ctx, rows, cols, gaussian_entries(rows, cols, SEED))


def test_product_bitwise_invariance(gpu_ctx):
    """A column's bits do not depend on the vector count, its slot, the other columns or their coefficients, and a
    repeated call returns the same bits."""
    rows, cols = 257, 1027
    G = hgmres.GaussianPerturbation(rows, cols, SEED, ctx=gpu_ctx)
    X = np.random.default_rng(6).standard_normal((cols, 8))
    c = COEFS8
    Y8 = G.matmat(X, c)
    assert np.array_equal(Y8, G.matmat(X, c))                    # two identical calls
    P = G.matmat(X)                                              # coefs = None: the unscaled products
    assert np.array_equal(Y8, P * c[None, :])                    # the coefficient is one rounding on the sum
    assert np.array_equal(P, G.matmat(X, np.ones(8)))
    for r in range(8):
        a, b = (r + 1) % 8, (r + 5) % 8
        assert np.array_equal(G.matmat(X[:, [r]], c[[r]])[:, 0], Y8[:, r]), r                      # alone
        assert np.array_equal(G.matmat(X[:, [r, a, b]], c[[r, a, b]])[:, 0], Y8[:, r]), r          # slot 0
        assert np.array_equal(G.matmat(X[:, [a, b, r]], c[[a, b, r]])[:, 2], Y8[:, r]), r          # last of 3
    perm = [1, 2, 3, 4, 5, 6, 7, 0]
    assert np.array_equal(G.matmat(X[:, perm], c[perm])[:, 7], Y8[:, 0])                           # last of 8
    other = c[::-1].copy()                                       # inside a group of 8 with other coefficients
    for r in (0, 3, 7):
        other[r] = c[r]
        assert np.array_equal(G.matmat(X, other)[:, r], Y8[:, r]), r
    Xo = X.copy()                                                # ... and other neighbours
    Xo[:, 1:] = np.random.default_rng(7).standard_normal((cols, 7))
    assert np.array_equal(G.matmat(Xo, c)[:, 0], Y8[:, 0])
    # the bits of a row do not depend on the matrix's row count (the row tiling): a taller G, the same rows
    G2 = hgmres.GaussianPerturbation(rows + 6, cols, SEED, ctx=gpu_ctx)
    assert np.array_equal(G2.matmat(X, c)[:rows], Y8)
    # scale multiplies the coefficients on the host
    assert np.array_equal(G._with_scale(0.375).matmat(X, c), G.matmat(X, c * 0.375))


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


@pytest.mark.parametrize("rows,cols", [(7, 5), (65, 1027), (1000, 257)])
def test_spmm_pert_gauss_is_the_two_products_combined(gpu_ctx, rows, cols):
    """Bit-equal to spmm(B0, X) + c * G.matmat(X) formed in numpy (two roundings); c = 0 gives spmm(B0, X)."""
    B0 = _random_csr(rows, cols, [0, 1, 3, min(cols, 300), 2, min(cols, 17)], seed=rows)
    Bop = hgmres.SparseOperator.from_scipy(B0, ctx=gpu_ctx)
    G = hgmres.GaussianPerturbation(rows, cols, SEED, ctx=gpu_ctx)
    X = np.random.default_rng(rows + 2).standard_normal((cols, 8))
    YB, YG = hgmres.spmm(Bop, X), G.matmat(X)
    for nv in (1, 3, 8):
        got = hgmres.spmm_pert(Bop, G, COEFS8[:nv], X[:, :nv])
        assert np.array_equal(got, YB[:, :nv] + COEFS8[None, :nv] * YG[:, :nv]), nv
        Yb = _mm_padded(gpu_ctx, G, X[:, :nv], 3, COEFS8[:nv], B0=Bop)
        assert np.array_equal(Yb[:rows], got) and np.all(np.isnan(Yb[rows:]))
    assert np.array_equal(hgmres.spmm_pert(Bop, G, np.zeros(8), X), YB)
    Gs = G._with_scale(1.0 / 3.0)
    assert np.array_equal(hgmres.spmm_pert(Bop, Gs, COEFS8, X), YB + (COEFS8 * Gs.scale)[None, :] * YG)
    ref = B0 @ X + (twin(rows, cols) @ X) * COEFS8
    bound = ((2.0 * cols + 2.0 + 16.0) * EPS * (abs(B0) @ np.abs(X) + np.abs(COEFS8) * (np.abs(twin(rows, cols)) @ np.abs(X)))
             + 2.0 * EPS * np.abs(ref))
    assert np.all(np.abs(hgmres.spmm_pert(Bop, G, COEFS8, X) - ref) <= bound)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (65, 257), (1000, 5003)])
def test_frobenius_norm(gpu_ctx, rows, cols):
    G = hgmres.GaussianPerturbation(rows, cols, SEED, ctx=gpu_ctx)
    Gt = twin(rows, cols).astype(np.longdouble)
    want = float(np.sqrt(np.sum(Gt * Gt)))
    f = G.fro()
    assert abs(f - want) <= (cols + rows + 20) * EPS * want
    assert G.fro() == f                                          # cached: the same bits
    G2 = hgmres.GaussianPerturbation(rows, cols, SEED, ctx=gpu_ctx)
    assert G2.fro() == f                                         # and recomputed: the same bits
    N = G.normalized()
    assert N.shape == G.shape and N.seed == G.seed and N.scale == 1.0 / f
    assert abs(N.fro() - 1.0) <= 4 * EPS
    assert G._with_scale(-2.5).fro() == 2.5 * f
    assert np.array_equal(N.to_dense(), G.to_dense() * N.scale)


# ---------------------------------------------------------------------------------------------
# 3. stored pixel order
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled(gpu_ctx):
    """The tiled and the reference-order pair of tiled_pair.py, and B with its values zeroed in both orders."""
    T = tiled_pair(gpu_ctx)
    B = T["B"]
    Bz = sp.csr_matrix((np.zeros(B.nnz), B.indices.copy(), B.indptr.copy()), shape=B.shape)   # B's pattern, zeros
    Bzt = hgmres.SparseOperator.from_scipy_tiled(sp.csr_matrix((np.zeros(B.nnz), B.T.tocsr().indices, B.T.tocsr().indptr),
                                                               shape=B.T.shape), 32, 4, 16, ctx=gpu_ctx).T
    assert Bzt.pixel_order("rows")[1:] == (4, 16)
    return dict(T, Bzt=Bzt, Bzr=hgmres.SparseOperator.from_scipy(Bz, ctx=gpu_ctx))


def test_spmm_pert_gauss_on_a_tiled_operator(gpu_ctx, tiled):
    n, m = tiled["B"].shape
    G = hgmres.GaussianPerturbation(n, m, SEED, ctx=gpu_ctx)
    X = np.random.default_rng(3).standard_normal((m, 5))
    c = COEFS8[:5]
    # B0's values zeroed: the result is the G part alone, 0 + (c * acc) -- the same bits in both stored orders
    Zt, Zr = hgmres.spmm_pert(tiled["Bzt"], G, c, X), hgmres.spmm_pert(tiled["Bzr"], G, c, X)
    assert np.array_equal(Zt, Zr)
    assert np.array_equal(Zt, G.matmat(X, c))
    assert np.all(np.abs(Zt - (twin(n, m) @ X) * c) <= (2.0 * m + 18.0) * EPS * (np.abs(twin(n, m)) @ np.abs(X)) * np.abs(c))
    # the full product: each side is its own spmm(B0) plus the same G part
    Yt, Yr = hgmres.spmm_pert(tiled["Bt"], G, c, X), hgmres.spmm_pert(tiled["Br"], G, c, X)
    assert np.array_equal(Yt, hgmres.spmm(tiled["Bt"], X) + c[None, :] * G.matmat(X))
    assert np.array_equal(Yr, hgmres.spmm(tiled["Br"], X) + c[None, :] * G.matmat(X))
    assert rel(Yt, Yr) <= 1e-13


@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", False)])
def test_sweep_on_tiled_operators(gpu_ctx, tiled, side, hybrid):
    """The sweep on the tiled pair against the reference-order pair, x in the reference order: a missed
    stored -> reference map of G's rows is an O(1) error."""
    P = tiled["P"]
    n, m = tiled["B"].shape
    G = hgmres.GaussianPerturbation(n, m, 21, ctx=gpu_ctx).normalized()
    coefs = np.logspace(-3, 0, 4) * np.linalg.norm(tiled["B"].data)
    lam = np.array([1e-2, 1e-1, 1.0, 10.0]) if hybrid else None
    run = lambda A, B: hgmres.gmres_bounds_mismatch(A, B, G, coefs, P.b, P.x_true, 0.0, 8, side, lambdas=lam,
                                                    ctx=gpu_ctx, return_H=True)
    Rt, Rr = run(tiled["At"], tiled["Bt"]), run(tiled["Ar"], tiled["Br"])
    assert np.array_equal(Rt.niters, Rr.niters) and np.all(Rt.niters == 8)
    for j in range(4):
        assert rel(Rt.x[:, j], Rr.x[:, j]) <= TOL
        hist_ok(Rt.residual_norm[:, j], Rr.residual_norm[:, j], TOL)
        hist_ok(Rt.error_norm[:, j], Rr.error_norm[:, j], TOL)
        assert np.max(np.abs(Rt.H[j] - Rr.H[j])) <= TOL * np.max(np.abs(Rr.H[j]))
    # the perturbation is felt: the last level differs from the first by far more than the bar
    assert rel(Rr.x[:, 3], Rr.x[:, 0]) > 1e-3


# ---------------------------------------------------------------------------------------------
# 4. the sweep against the oracle, the sparse path and itself
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problems(gpu_ctx):
    out = {}
    for name in FIXTURES:
        A, B, b, xt, _ = golden_problem(name)
        A.sort_indices()
        B.sort_indices()
        assert B.shape == (576, 408)
        G = hgmres.GaussianPerturbation(576, 408, seed=21, ctx=gpu_ctx).normalized()
        Et = gaussian_entries(576, 408, 21) * G.scale           # the twin, with the device's scale
        coefs = np.logspace(-4, 0, NCOEF) * np.linalg.norm(B.data)
        up = lambda M: hgmres.SparseOperator.from_scipy(M, ctx=gpu_ctx)
        Bd = B.toarray()
        out[name] = dict(A=A, B=B, G=G, Et=Et, b=b, xt=xt, coefs=coefs, Ao=up(A), Bo=up(B),
                         Bc=[sp.csr_matrix(Bd + c * Et) for c in coefs])
    return out


_ORACLE_CACHE = {}


def _oracle_sweep(problems, name, side, hybrid, cgs2=False):
    """The oracle's solver once per level on the explicit dense B + c_j E_twin (computed once per case), and the
    checks on the oracle's own result: the stopping tolerance spreads the levels (at least two distinct niters,
    at least one below maxit) and no residual-history entry lies within 1e-6 (relative) of it."""
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


def _sweep(P, ctx, side, hybrid, cols=None, E=None, **kw):
    cols = slice(None) if cols is None else cols
    return hgmres.gmres_bounds_mismatch(P["Ao"], P["Bo"], P["G"] if E is None else E, P["coefs"][cols], P["b"], P["xt"],
                                        STOP, MAXIT, side, lambdas=LAMS[cols] if hybrid else None, ctx=ctx,
                                        return_H=True, **kw)


@pytest.mark.parametrize("side,hybrid", CASES)
@pytest.mark.parametrize("name", FIXTURES)
def test_gauss_sweep_matches_oracle(gpu_ctx, problems, name, side, hybrid):
    ref = _oracle_sweep(problems, name, side, hybrid)
    _check_against_oracle(_sweep(problems[name], gpu_ctx, side, hybrid), ref)


def test_gauss_sweep_cgs2_matches_oracle_cgs2(gpu_ctx, problems, monkeypatch):
    """orth = 'cgs2' against the oracle's solver with its CGS2 Arnoldi step in place of MGS."""
    monkeypatch.setattr(R, "_mgs_arnoldi_step", R._cgs2_arnoldi_step)
    ref = _oracle_sweep(problems, "tomo24_pixel.npz", "ab", True, cgs2=True)
    _check_against_oracle(_sweep(problems["tomo24_pixel.npz"], gpu_ctx, "ab", True, orth="cgs2"), ref)


@pytest.mark.parametrize("side,hybrid", CASES)
def test_gauss_sweep_matches_the_sparse_path(gpu_ctx, problems, side, hybrid):
    """The same sweep through hgm_gmres_bounds_mismatch with E uploaded as the fully dense CSR of G's entries
    (scaled): the summation order differs, so the project's bar and not bits."""
    P = problems["tomo24_pixel.npz"]
    Ed = sp.csr_matrix(P["G"].entries())
    assert Ed.nnz == 576 * 408
    Eo = hgmres.SparseOperator.from_scipy(Ed, ctx=gpu_ctx)
    a, b = _sweep(P, gpu_ctx, side, hybrid), _sweep(P, gpu_ctx, side, hybrid, E=Eo)
    assert np.array_equal(a.niters, b.niters) and np.all(a.status == L.HGM_OK)
    for j in range(NCOEF):
        hist_ok(a.residual_norm[:, j], b.residual_norm[:, j], TOL)
        hist_ok(a.error_norm[:, j], b.error_norm[:, j], TOL)
        assert rel(a.x[:, j], b.x[:, j]) <= TOL
        assert np.max(np.abs(a.H[j] - b.H[j])) <= TOL * np.max(np.abs(b.H[j]))
    Eo.close()


@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", False)])
def test_gauss_sweep_equals_its_levels_alone(gpu_ctx, problems, side, hybrid):
    P = problems["tomo24_pixel.npz"]
    Rb = _sweep(P, gpu_ctx, side, hybrid)
    assert len(set(Rb.niters)) >= 2                          # levels left the sweep at different steps
    for j in range(NCOEF):
        same_batch(Rb, _sweep(P, gpu_ctx, side, hybrid, cols=[j]), [j], [0])
    same_batch(Rb, _sweep(P, gpu_ctx, side, hybrid))          # repeatable


def test_gauss_sweep_of_two_groups_equals_its_levels_alone(gpu_ctx, problems):
    """11 levels: two packed groups (8 + 3), regrouped (coefficients with them) as levels finish."""
    P = problems["tomo24_matched.npz"]
    coefs = np.logspace(-4, 0, 11) * np.linalg.norm(P["B"].data)
    lams = np.logspace(-2, 2, 11)
    run = lambda cols: hgmres.gmres_bounds_mismatch(P["Ao"], P["Bo"], P["G"], coefs[cols], P["b"], P["xt"], STOP, MAXIT,
                                                    "ab", lambdas=lams[cols], ctx=gpu_ctx, return_H=True)
    Rb = run(slice(None))
    assert len(set(Rb.niters)) >= 2 and min(Rb.niters) < MAXIT
    for j in range(11):
        same_batch(Rb, run([j]), [j], [0])


@pytest.mark.parametrize("side,hybrid", [("ab", True), ("ba", True), ("ab", False)])
def test_zero_coefficients_equal_the_batch_of_replicated_b(gpu_ctx, problems, side, hybrid):
    P = problems["tomo24_matched.npz"]
    lam = LAMS if hybrid else None
    a = hgmres.gmres_bounds_mismatch(P["Ao"], P["Bo"], P["G"], np.zeros(NCOEF), P["b"], P["xt"], STOP, MAXIT, side,
                                     lambdas=lam, ctx=gpu_ctx, return_H=True)
    Bm = np.repeat(P["b"][:, None], NCOEF, axis=1)
    b = hgmres.gmres_bounds_batch(P["Ao"], P["Bo"], Bm, P["xt"], STOP, MAXIT, side, lambdas=lam, ctx=gpu_ctx, return_H=True)
    same_batch(a, b)
    assert np.all(np.isfinite(a.x))


# ---------------------------------------------------------------------------------------------
# 5. the lockstep GCV Arnoldi, breakdown
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["ab", "ba"])
def test_gauss_arnoldi_mismatch(gpu_ctx, problems, side):
    P = problems["tomo24_pixel.npz"]
    k = 8
    H, beta, kd = hgmres.arnoldi_mismatch(P["Ao"], P["Bo"], P["G"], P["coefs"], P["b"], k, side, ctx=gpu_ctx)
    assert H.shape == (NCOEF, k + 1, k) and beta.shape == (NCOEF,) and np.all(kd == k)
    for j in range(NCOEF):
        Hr, br = R.arnoldi(P["A"], P["Bc"][j], P["b"], k, side)
        assert np.max(np.abs(H[j] - Hr)) <= TOL * np.max(np.abs(Hr)), j
        assert abs(beta[j] - br) <= TOL * abs(br), j
        Ha, ba, ka = hgmres.arnoldi_mismatch(P["Ao"], P["Bo"], P["G"], P["coefs"][[j]], P["b"], k, side, ctx=gpu_ctx)
        assert np.array_equal(Ha[0], H[j]) and ba[0] == beta[j] and ka[0] == kd[j]       # the level alone


@pytest.mark.parametrize("side", ["ab", "ba"])
def test_gauss_mismatch_empty_operator_breaks_every_level(gpu_ctx, side):
    """An all-zero A (test_gpu_mismatch.py's empty operator): H(2,1) = 0 at the first step of every level; and the
    lockstep Arnoldi breaks at its first step."""
    A = sp.csr_matrix((6, 4))
    B = sp.csr_matrix(np.ones((4, 6)))
    b = np.arange(1.0, 7.0)
    xt = np.ones(4)
    Ao, Bo = (hgmres.as_operator(M, gpu_ctx) for M in (A, B))
    G = hgmres.GaussianPerturbation(4, 6, 3, ctx=gpu_ctx)
    lib = L.load()
    X = np.full((4, 3), 7.0, order="F")
    err, res = np.zeros((3, 3), order="F"), np.zeros((3, 3), order="F")
    nit, st = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    lam = np.array([0.5, 1.0, 2.0])
    cf = np.array([0.0, 0.1, -3.0])
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp)
    rc = lib.hgm_gmres_bounds_mismatch_gauss(gpu_ctx.handle, None, Ao._h, Bo._h, G._h, dp(cf), 3, dp(b), dp(xt), 1e-2, 3,
                                             dp(lam), L.HGM_SIDE_AB if side == "ab" else L.HGM_SIDE_BA, 1, dp(X), 4,
                                             dp(err), dp(res), nit.ctypes.data_as(ip), st.ctypes.data_as(ip))
    assert rc == L.HGM_E_NOT_ASSIGNED
    assert np.all(st == L.HGM_E_NOT_ASSIGNED) and np.all(nit == 1)
    assert np.all(X == 7.0)                                  # the X columns are left untouched
    Rb = hgmres.gmres_bounds_mismatch(Ao, Bo, G, cf, b, xt, 1e-2, 3, side, lambdas=lam, ctx=gpu_ctx)
    assert np.all(Rb.status == L.HGM_E_NOT_ASSIGNED) and np.all(Rb.niters == 1) and np.all(np.isnan(Rb.x))
    H, beta, kd = hgmres.arnoldi_mismatch(Ao, Bo, G, cf, b, 3, side, ctx=gpu_ctx)
    assert np.all(kd == 1) and np.all(H[:, 1, 0] == 0.0) and np.all(np.isfinite(beta))


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def test_gauss_refusals(gpu_ctx, problems):
    P = problems["tomo24_matched.npz"]
    A, B, G, b, xt = P["Ao"], P["Bo"], P["G"], P["b"], P["xt"]
    lib = L.load()
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp) if a is not None else None
    m, n = A.shape
    cf2 = np.array([0.1, 0.2])

    def solve(ctx, Ah, Bh, Gh, cf, lam, hybrid, flags=0):
        o = L.hgm_opts()
        o.flags, o.orth, o.H_out = flags, L.HGM_MGS, None
        nc = cf.size
        nit = np.zeros(max(nc, 1), dtype=np.int32)
        return lib.hgm_gmres_bounds_mismatch_gauss(ctx.handle, C.byref(o), Ah, Bh, Gh, dp(cf), nc, dp(b), dp(xt), 0.0, 3,
                                                   dp(lam), L.HGM_SIDE_AB, hybrid, None, n, None, None,
                                                   nit.ctypes.data_as(ip), None)

    def arn(ctx, Ah, Bh, Gh, cf):
        nc = cf.size
        H, beta, kd = np.zeros(4 * 3 * max(nc, 1)), np.zeros(max(nc, 1)), np.zeros(max(nc, 1), dtype=np.int32)
        return lib.hgm_arnoldi_mismatch_gauss(ctx.handle, Ah, Bh, Gh, dp(cf), nc, dp(b), 3, L.HGM_SIDE_BA, 1e-12,
                                              L.HGM_MGS, dp(H), dp(beta), kd.ctypes.data_as(ip))

    A32 = hgmres.as_operator(P["A"], gpu_ctx, dtype=L.HGM_F32)
    Gbad = hgmres.GaussianPerturbation(n, m + 1, 21, ctx=gpu_ctx)
    for call in (lambda *a: solve(*a, None, 0), arn):
        assert call(gpu_ctx, A32._h, A32.T._h, G._h, cf2) == L.HGM_E_ARG                 # fp32 operators
        with gpu_ctx.options(parity=1):
            assert call(gpu_ctx, A._h, B._h, G._h, cf2) == L.HGM_E_ARG                   # parity mode
        assert call(gpu_ctx, A._h, B._h, G._h, np.zeros(0)) == L.HGM_E_ARG               # ncoef < 1
        assert call(gpu_ctx, A._h, B._h, G._h, np.linspace(0, 1, 65)) == L.HGM_E_ARG     # ncoef > 64
        for bad in (np.nan, np.inf, -np.inf):
            assert call(gpu_ctx, A._h, B._h, G._h, np.array([0.1, bad])) == L.HGM_E_ARG  # non-finite coefficient
        assert call(gpu_ctx, A._h, B._h, Gbad._h, cf2) == L.HGM_E_ARG                    # G's shape is not B0's
    assert solve(gpu_ctx, A._h, B._h, G._h, cf2, None, 0, flags=L.HGM_DEVICE_PTRS) == L.HGM_E_ARG   # device pointers
    for bad in (-1.0, np.nan, np.inf):
        assert solve(gpu_ctx, A._h, B._h, G._h, cf2, np.array([1.0, bad]), 1) == L.HGM_E_ARG        # bad lambda (hybrid)
        assert solve(gpu_ctx, A._h, B._h, G._h, cf2, np.array([1.0, bad]), 0) == L.HGM_OK           # ignored otherwise
    assert solve(gpu_ctx, A._h, B._h, G._h, cf2, None, 1) == L.HGM_E_ARG                            # hybrid needs lambdas
    with pytest.raises(ValueError, match="shape"):
        hgmres.spmm_pert(B, Gbad, cf2, np.ones((m, 2)))
    # the products
    px = C.c_void_p(8)
    assert lib.hgm_spmm_pert_gauss(gpu_ctx.handle, B._h, Gbad._h, 2, dp(cf2), px, m + 1, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(gpu_ctx.handle, B._h, G._h, 9, dp(np.zeros(9)), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(gpu_ctx.handle, B._h, G._h, 0, dp(cf2), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(gpu_ctx.handle, B._h, G._h, 2, dp(np.array([1.0, np.nan])), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(gpu_ctx.handle, A32.T._h, G._h, 2, dp(cf2), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(gpu_ctx.handle, B._h, G._h, 2, dp(cf2), px, m - 1, px, n) == L.HGM_E_ARG   # ldx < cols
    assert lib.hgm_gauss_mm(gpu_ctx.handle, G._h, 9, None, px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(gpu_ctx.handle, G._h, 0, None, px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(gpu_ctx.handle, G._h, 2, dp(np.array([np.inf, 1.0])), px, m, px, n) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(gpu_ctx.handle, G._h, 2, None, px, m, px, n - 1) == L.HGM_E_ARG                  # ldy < rows
    # the handle and its blocks
    h = C.c_void_p()
    assert lib.hgm_gauss_create(gpu_ctx.handle, 0, 4, 1, C.byref(h)) == L.HGM_E_ARG and not h.value
    assert lib.hgm_gauss_create(gpu_ctx.handle, 4, 0, 1, C.byref(h)) == L.HGM_E_ARG and not h.value
    out = np.zeros(4)
    for i0, ni, j0, nj, ldo in ((-1, 1, 0, 1, 1), (0, 1, -1, 1, 1), (n - 1, 2, 0, 1, 2), (0, 1, m, 1, 1), (0, 2, 0, 2, 1)):
        assert lib.hgm_gauss_entries(gpu_ctx.handle, G._h, i0, ni, j0, nj, dp(out), ldo) == L.HGM_E_ARG
    big = hgmres.GaussianPerturbation(1 << 20, 1 << 20, 1, ctx=gpu_ctx)
    assert lib.hgm_gauss_entries(gpu_ctx.handle, big._h, 0, 1 << 14, 0, (1 << 13) + 1, dp(out), 1 << 14) == L.HGM_E_ARG
    # a context with a host all-reduce hook at world 2: HGM_E_UNSUPPORTED, and the hook is never called
    calls = []
    c2 = hgmres.Context(0)
    try:
        c2.set_host_allreduce(0, 2, lambda arr: calls.append(arr.size))
        A2 = hgmres.as_operator(P["A"], c2)
        B2 = hgmres.as_operator(P["B"], c2)
        G2 = hgmres.GaussianPerturbation(n, m, 21, ctx=c2)
        assert solve(c2, A2._h, B2._h, G2._h, cf2, None, 0) == L.HGM_E_UNSUPPORTED
        assert arn(c2, A2._h, B2._h, G2._h, cf2) == L.HGM_E_UNSUPPORTED
        assert calls == []
        G2.close()
    finally:
        c2.close()
    # the context still solves after the refusals
    Rb = hgmres.gmres_bounds_mismatch(A, B, G, cf2, b, xt, 0.0, 3, "ab", ctx=gpu_ctx)
    assert np.all(Rb.niters == 3) and np.all(np.isfinite(Rb.x))


# ---------------------------------------------------------------------------------------------
# 7. pipeline and gateway
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gcv", [False, True])
def test_error_vs_mismatch_norm_matches_solver_loop(gpu_ctx, problems, gcv):
    P = problems["tomo24_matched.npz"]
    cr = P["coefs"][:4]
    lam_in = None if gcv else (np.array([1e-2, 0.1, 1.0, 10.0]), np.array([0.05, 0.5, 5.0, 50.0]))
    M = analysis.error_vs_mismatch_norm(P["Ao"], P["Bo"], P["G"], P["b"], P["xt"], cr, maxit=8, tol=0.05, k_gcv=8,
                                        lambdas=lam_in, solvers=("hab", "hba", "nab", "nba"), ctx=gpu_ctx)
    assert np.all(np.abs(M["mismatch_norms"] - np.abs(cr)) <= 4 * EPS * np.abs(cr))      # ||E||_F = 1
    if gcv:
        for side in ("ab", "ba"):
            trace_m = P["A"].shape[0] if side == "ab" else P["A"].shape[1]
            H, beta, _ = hgmres.arnoldi_mismatch(P["Ao"], P["Bo"], P["G"], cr, P["b"], 8, side, ctx=gpu_ctx)
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


def test_error_vs_mismatch_norm_on_heat(gpu_ctx):
    """plot_error_vs_mismatch_norm.m's own case: heat, n = 32, c_range = logspace(-8, -1, 20) and the dense
    E = randn(size(A')) / norm(E, 'fro') of :16-17 as G.normalized()."""
    A, b_exact, x_true = generate_test_problem("heat", 32)
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(b_exact.shape)
    b = b_exact + noise / np.linalg.norm(noise) * 1e-2 * np.linalg.norm(b_exact)
    G = hgmres.GaussianPerturbation(32, 32, 0, ctx=gpu_ctx).normalized()
    cr = np.logspace(-8, -1, 20)
    M = analysis.error_vs_mismatch_norm(sp.csr_matrix(A), sp.csr_matrix(A.T), G, b, x_true, cr, maxit=32, ctx=gpu_ctx)
    assert M["mismatch_norms"].shape == (20,) and np.all(np.abs(M["mismatch_norms"] - np.abs(cr)) <= 4 * EPS * np.abs(cr))
    for side in ("ab", "ba"):
        lam = M[f"lambda_gcv_{side}"]
        assert lam.shape == (20,) and np.all((lam >= 1e-9) & (lam <= 1e-1))
    for key in ("hab", "hba"):
        assert M[f"final_errors_{key}"].shape == (20,) and np.all(np.isfinite(M[f"final_errors_{key}"]))
        assert np.all((M[f"niters_{key}"] >= 1) & (M[f"niters_{key}"] <= 32))
    assert "final_errors_nab" not in M


def test_matlab_command_equals_python_call(gpu_ctx, problems):
    """matlab/gmres_bounds_mismatch_gauss.m through the gateway (the mx API stand-in) against the Python binding."""
    from mwrap import Function
    from test_mex_gateway import Mex
    P = problems["tomo24_pixel.npz"]
    A, B, G = P["A"], P["B"], P["G"]
    f = Function(os.path.join(ROOT, "matlab", "gmres_bounds_mismatch_gauss.m"), Mex())
    for side, lam in (("ab", LAMS), ("ba", None)):
        Rb = hgmres.gmres_bounds_mismatch(A, B, G, P["coefs"], P["b"], P["xt"], STOP, MAXIT, side, lambdas=lam, ctx=gpu_ctx)
        args = (sp.csc_matrix(A), sp.csc_matrix(B), float(G.seed), G.scale, P["coefs"], P["b"], P["xt"], STOP,
                float(MAXIT), side)
        X, e, r, ni, st = f(5, *(args + ((lam,) if lam is not None else ())))
        assert X.shape == Rb.x.shape and e.shape == r.shape == (MAXIT, NCOEF)
        assert np.array_equal(ni.reshape(-1).astype(int), Rb.niters) and np.all(st == 0)
        assert np.array_equal(X, Rb.x)
        assert np.array_equal(e, Rb.error_norm, equal_nan=True) and np.array_equal(r, Rb.residual_norm, equal_nan=True)
