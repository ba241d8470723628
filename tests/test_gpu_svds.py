"""Device singular triplets and empirical filter factors (hgm_svds, hgm_basis_project, hgm_basis_rotate)
on the MI355X: the numeric part of plot_filter_factors.m:30-40 with svd(A,'econ') replaced by a
Golub-Kahan-Lanczos run started at b.

The yardsticks live here: ``twin`` is the numpy statement of the same loop (full reorthogonalisation by
CGS2, the same breakdown rule), ``Dense`` is numpy.linalg.svd of the operator.  Every operator is at most
612 x 576.  The inputs (tomo_problem(24, 18) parallel / fan, the 408 x 576 tomo24_matched operator) have a
simple leading spectrum, so a mode-by-mode comparison with the dense SVD is meaningful (with exactly
repeated singular values a single-vector Lanczos returns the projection of b on the singular subspace)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import hgmres
from conftest import golden_problem
from hgmres import _lib as L
from hgmres import analysis
from hgmres.problems import tomo_problem

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------
# yardsticks
# ---------------------------------------------------------------------------------------------
def _cgs2(w, Q):
    for _ in range(2):
        w = w - Q @ (Q.T @ w)
    return w


class Twin:
    """The loop of hgm_svds in numpy: sigma, resid, utb, U, V, steps_done (signs fixed so that utb >= 0)."""

    def __init__(self, A, b, steps, btol=1e-12):
        A = sp.csr_matrix(A) if sp.issparse(A) else np.asarray(A)
        m, n = A.shape
        kmax = min(steps, m, n)
        beta1 = np.linalg.norm(b)
        U = np.zeros((m, kmax + 1))
        V = np.zeros((n, kmax + 1))
        U[:, 0] = b / beta1
        alpha, beta = [], []
        big, k, broke, a_next, bt = 0.0, 0, False, 0.0, 0.0
        for j in range(kmax + 1):
            v = A.T @ U[:, j] - (bt * V[:, j - 1] if j else 0.0)
            v = _cgs2(v, V[:, :j])
            a = np.linalg.norm(v)
            if j == kmax:                                   # the extra half step: alpha_{k+1}
                a_next = a
                break
            if not a > btol * big:
                broke = True
                break
            big = max(big, a)
            V[:, j] = v / a
            u = A @ V[:, j] - a * U[:, j]
            u = _cgs2(u, U[:, :j + 1])
            bt = np.linalg.norm(u)
            alpha.append(a)
            beta.append(bt)
            k = j + 1
            if not bt > btol * big:
                broke = True
                break
            big = max(big, bt)
            U[:, j + 1] = u / bt
        self.steps_done, self.broke = k, broke
        B = np.zeros((k + 1, k))
        B[np.arange(k), np.arange(k)] = alpha
        B[np.arange(1, k + 1), np.arange(k)] = beta
        P, s, Qt = np.linalg.svd(B, full_matrices=False)
        sg = np.where(P[0] < 0, -1.0, 1.0)
        P, Q = P * sg, Qt.T * sg
        self.sigma = s
        self.utb = beta1 * P[0]
        self.resid = np.zeros(k) if broke else a_next * np.abs(P[k])
        self.U, self.V = U[:, :k + 1] @ P, V[:, :k] @ Q

    def nconv(self, tol=1e-10):
        bad = np.nonzero(~(self.resid <= tol * self.sigma[0]))[0]
        return int(bad[0]) if bad.size else self.resid.size

    def phi(self, X):
        d = self.utb.copy()
        d[np.abs(d) < 1e-12] = 1.0
        return self.sigma[:, None] * (self.V.T @ X) / d[:, None]


class Dense:
    def __init__(self, A, b):
        Ad = A.toarray() if sp.issparse(A) else np.asarray(A)
        self.U, self.s, Vt = np.linalg.svd(Ad, full_matrices=False)
        self.V = Vt.T
        self.d = self.U.T @ b
        self.d[np.abs(self.d) < 1e-12] = 1.0                  # plot_filter_factors.m:35

    def phi(self, X):
        return self.s[:, None] * (self.V.T @ X) / self.d[:, None]   # :31-40 (the signs of u_i, v_i cancel)


def phi_dev(Phi, Phi_dense, run):
    """max over the leading run of |Phi - Phi_dense| / max(1, |Phi_dense|)"""
    return float(np.max(np.abs(Phi[:run] - Phi_dense[:run]) / np.maximum(1.0, np.abs(Phi_dense[:run])), initial=0.0))


def solutions(A, b, x_true):
    """X = [lsqr 12 its, damped lsqr 12 its (damp 0.1), x_true]"""
    kw = dict(atol=0.0, btol=0.0, conlim=0.0, iter_lim=12)
    return np.column_stack([spla.lsqr(A, b, **kw)[0], spla.lsqr(A, b, damp=0.1, **kw)[0], x_true])


class Case:
    """One operator with everything the tests share: the solutions, the dense SVD, the twin (computed once)."""

    def __init__(self, A, b, x_true, steps, nsv):
        self.A, self.b, self.x_true, self.steps, self.nsv = A, b, x_true, steps, nsv
        self.X = solutions(A, b, x_true)
        self.dense = Dense(A, b)
        self.twin = Twin(A, b, steps)
        self._dev = None

    def device(self, ctx):
        if self._dev is None:
            self._dev = hgmres.svds(self.A, self.b, self.steps, self.nsv, X=self.X, return_vectors=True, ctx=ctx)
        return self._dev


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, kw in (("parallel", {}), ("fan", {"geometry_kind": "fan"})):
        P = tomo_problem(24, 18, noise=1e-2, seed=0, **kw)
        out[name] = Case(P.A, P.b, P.x_true, 60, 20)
    A, _, b, xt, _ = golden_problem("tomo24_matched.npz")     # 408 x 576: m < n
    out["mlt"] = Case(A, b, xt, 60, 20)
    return out


def _nan_padded(M, pad):
    """M as a view of a NaN-filled Fortran array with `pad` more rows (leading dimension rows + pad)."""
    buf = np.full((M.shape[0] + pad, M.shape[1]), np.nan, order="F")
    buf[:M.shape[0]] = M
    return buf[:M.shape[0]]


# ---------------------------------------------------------------------------------------------
# 1. the two block kernels
# ---------------------------------------------------------------------------------------------
ROWS = (1, 15, 16, 17, 63, 64, 65, 255, 1000, 65537)
KS = (1, 3, 4, 5, 80, 256)
PS = (1, 15, 16, 17, 64)


def _ld(a):
    return a.astype(np.longdouble)


@pytest.mark.parametrize("rows", ROWS)
def test_basis_project_against_longdouble(gpu_ctx, rows):
    """|C - C_ref| <= (rows + 2) eps sum|Q||X| per entry, NaN-filled padding in both leading dimensions (odd
    ones: no alignment is assumed).  Every k with every nx in 1..8 up to 1000 rows; at 65537 rows every k
    with nx = 8 (the group width) and nx = 3."""
    rng = np.random.default_rng(rows)
    for k in KS:
        Q = rng.standard_normal((rows, k))
        X8 = rng.standard_normal((rows, 8))
        for nx in (range(1, 9) if rows <= 1000 else (3, 8)):
            X = X8[:, :nx]
            Cm = hgmres.basis_project(_nan_padded(Q, 3), _nan_padded(X, 1), ctx=gpu_ctx)
            ref = _ld(Q).T @ _ld(X)
            bound = (rows + 2) * EPS * (np.abs(Q).T @ np.abs(X))
            err = np.abs(_ld(Cm) - ref)
            assert Cm.shape == (k, nx) and np.all(err <= bound), (rows, k, nx, float(np.max(err / bound)))


@pytest.mark.parametrize("rows", ROWS)
def test_basis_rotate_against_longdouble(gpu_ctx, rows):
    """|W - W_ref| <= (k + 2) eps sum|Q||Y| per entry and the device sum of squares within the same bound
    summed (plus the rows-term of its own fixed-order sum); NaN-filled padding in every leading dimension,
    W's padding comes back untouched.  Every k with every p up to 1000 rows; at 65537 rows every k with
    p = 17 and 64, the long-double reference on a sample of rows that holds the first and last tiles."""
    rng = np.random.default_rng(1000 + rows)
    for k in KS:
        Q = rng.standard_normal((rows, k))
        Y64 = rng.standard_normal((k, 64))
        sel = np.arange(rows) if rows <= 1000 else np.unique(np.concatenate(
            [np.arange(80), np.arange(rows - 80, rows), rng.integers(0, rows, 600)]))
        for p in (PS if rows <= 1000 else (17, 64)):
            Y = Y64[:, :p]
            W, ss = hgmres.basis_rotate(_nan_padded(Q, 3), _nan_padded(Y, 2), ldw=rows + 5, return_sumsq=True,
                                        ctx=gpu_ctx)
            assert W.shape == (rows + 5, p) and np.all(np.isnan(W[rows:])), "W's padding rows were written"
            W = W[:rows]
            assert np.all(np.isfinite(W))
            ref = _ld(Q[sel]) @ _ld(Y)
            bound = (k + 2) * EPS * (np.abs(Q[sel]) @ np.abs(Y))
            err = np.abs(_ld(W[sel]) - ref)
            assert np.all(err <= bound), (rows, k, p, float(np.max(err / bound)))
            # sum_i W_il^2 of the stored W itself: a sum of rows non-negative terms in some fixed order
            s_ref = np.sum(_ld(W) ** 2, axis=0)
            assert np.all(np.abs(_ld(ss) - s_ref) <= (rows + 2) * EPS * s_ref), (rows, k, p)


def test_block_kernels_are_reproducible_and_column_independent(gpu_ctx):
    """Two calls give the same bits; a column alone, among others (across the group width 8 / the MFMA block
    16), or in another position gives the same bits."""
    rng = np.random.default_rng(7)
    rows, k = 1000, 80
    Q = rng.standard_normal((rows, k))
    X = rng.standard_normal((rows, 11))
    C1 = hgmres.basis_project(Q, X, ctx=gpu_ctx)
    assert np.array_equal(C1, hgmres.basis_project(Q, X, ctx=gpu_ctx))
    for j in (0, 4, 7, 8, 10):
        assert np.array_equal(hgmres.basis_project(Q, X[:, [j]], ctx=gpu_ctx)[:, 0], C1[:, j]), j
    perm = rng.permutation(11)
    assert np.array_equal(hgmres.basis_project(Q, X[:, perm], ctx=gpu_ctx), C1[:, perm])
    assert np.array_equal(hgmres.basis_project(Q, X[:, :3], ctx=gpu_ctx), C1[:, :3])
    Y = rng.standard_normal((k, 33))
    W1, s1 = hgmres.basis_rotate(Q, Y, return_sumsq=True, ctx=gpu_ctx)
    W2, s2 = hgmres.basis_rotate(Q, Y, return_sumsq=True, ctx=gpu_ctx)
    assert np.array_equal(W1, W2) and np.array_equal(s1, s2)
    assert np.array_equal(hgmres.basis_rotate(Q, Y, ctx=gpu_ctx), W1)            # with or without the sums
    for j in (0, 15, 16, 32):
        Wj, sj = hgmres.basis_rotate(Q, Y[:, [j]], return_sumsq=True, ctx=gpu_ctx)
        assert np.array_equal(Wj[:, 0], W1[:, j]) and sj[0] == s1[j], j
    perm = rng.permutation(33)
    Wp, sp_ = hgmres.basis_rotate(Q, Y[:, perm], return_sumsq=True, ctx=gpu_ctx)
    assert np.array_equal(Wp, W1[:, perm]) and np.array_equal(sp_, s1[perm])


def test_block_kernels_agree_with_the_loop_of_one_vector_kernels(gpu_ctx):
    """The yardstick hooks (a loop of multidot / gemv launches, the code the block kernels replace) give the same
    products to the kernels' own bounds: each side is within (rows + 2) eps / (k + 2) eps of the exact value."""
    rng = np.random.default_rng(11)
    rows, k = 1000, 60
    Q, X, Y = rng.standard_normal((rows, k)), rng.standard_normal((rows, 4)), rng.standard_normal((k, 20))
    Cb, Cl = hgmres.basis_project(Q, X, ctx=gpu_ctx), hgmres.basis_project(Q, X, loop=True, ctx=gpu_ctx)
    assert np.all(np.abs(Cb - Cl) <= 2 * (rows + 2) * EPS * (np.abs(Q).T @ np.abs(X)))
    Wb, Wl = hgmres.basis_rotate(Q, Y, ctx=gpu_ctx), hgmres.basis_rotate(Q, Y, loop=True, ctx=gpu_ctx)
    assert np.all(np.abs(Wb - Wl) <= 2 * (k + 2) * EPS * (np.abs(Q) @ np.abs(Y)))


def test_block_kernels_refuse_bad_sizes(gpu_ctx):
    Q = np.ones((8, 2))
    with pytest.raises(ValueError, match="256"):
        hgmres.basis_project(np.ones((4, 257)), np.ones((4, 1)), ctx=gpu_ctx)
    with pytest.raises(ValueError, match="64 columns"):
        hgmres.basis_rotate(Q, np.ones((2, 65)), ctx=gpu_ctx)
    assert np.array_equal(hgmres.basis_project(Q, np.ones((8, 1)), ctx=gpu_ctx), np.full((2, 1), 8.0))


# ---------------------------------------------------------------------------------------------
# 2, 3, 5. triplets and empirical factors against the dense SVD
# ---------------------------------------------------------------------------------------------
NCONV_MIN = {"parallel": 10, "fan": 10, "mlt": 9}     # numpy's twin reaches 13, 11 and 11


@pytest.mark.parametrize("name", ["parallel", "fan", "mlt"])
def test_triplets_against_dense_svd(gpu_ctx, cases, name):
    c = cases[name]
    r = c.device(gpu_ctx)
    s1 = c.dense.s[0]
    run = r.nconv()
    dsig = float(np.max(np.abs(r.sigma[:run] - c.dense.s[:run]))) / s1
    print(f"{name}: steps_done {r.steps_done} nconv {run} (twin {c.twin.nconv()}) max|dsigma|/sigma1 {dsig:.2e}")
    assert r.steps_done == c.steps and r.sigma.shape == (c.nsv,)
    assert run >= NCONV_MIN[name]
    assert dsig <= 1e-12
    assert np.all(r.utb[:c.nsv] >= 0)
    U, V, A = r.U[:, :run], r.V[:, :run], c.A
    av = np.linalg.norm(A @ V - U * r.sigma[:run], axis=0)
    atu = np.linalg.norm(A.T @ U - V * r.sigma[:run], axis=0)
    print(f"{name}: max||Av - su||/s1 {av.max() / s1:.2e} max(||A'u - sv|| - resid)/s1 "
          f"{np.max(atu - r.resid[:run]) / s1:.2e} (largest resid/s1 in the run {r.resid[:run].max() / s1:.2e}) "
          f"||V'V - I|| {np.linalg.norm(r.V.T @ r.V - np.eye(c.nsv), 2):.2e} "
          f"||U'U - I|| {np.linalg.norm(r.U.T @ r.U - np.eye(c.nsv), 2):.2e}")
    assert np.all(av <= 1e-12 * s1)
    assert np.all(atu <= 1.01 * r.resid[:run] + 1e-12 * s1)
    # all nsv vectors are orthonormal, converged or not
    assert np.linalg.norm(r.V.T @ r.V - np.eye(c.nsv), 2) <= 1e-12
    assert np.linalg.norm(r.U.T @ r.U - np.eye(c.nsv), 2) <= 1e-12
    assert np.allclose(r.utb, r.U.T @ c.b, rtol=0, atol=1e-12 * np.linalg.norm(c.b))


@pytest.mark.parametrize("name", ["parallel", "fan", "mlt"])
def test_empirical_factors_against_dense_svd(gpu_ctx, cases, name):
    """Over the leading run, |Phi - Phi_dense| / max(1, |Phi_dense|) <= max(1e-12, 10 x the twin's own deviation)
    (the factor 10: the device's summation orders over 60 reorthogonalised steps)."""
    c = cases[name]
    E = hgmres.empirical_filter_factors(c.A, c.b, c.X, c.steps, c.nsv, ctx=gpu_ctx)
    sigma, Phi, resid, nconv = E
    r = c.device(gpu_ctx)
    assert np.array_equal(sigma, r.sigma) and np.array_equal(resid, r.resid) and nconv == r.nconv()
    d = np.where(np.abs(r.utb) < 1e-12, 1.0, r.utb)                               # plot_filter_factors.m:35
    assert np.array_equal(Phi, r.sigma[:, None] * r.VtX / d[:, None])
    pd = c.dense.phi(c.X)
    run = min(nconv, c.twin.nconv())
    dev, tw = phi_dev(Phi, pd, run), phi_dev(c.twin.phi(c.X), pd, run)
    print(f"{name}: Phi deviation from dense over {run} modes: device {dev:.2e} twin {tw:.2e}")
    assert nconv >= NCONV_MIN[name]
    assert dev <= max(1e-12, 10 * tw)
    assert phi_dev(Phi, pd, nconv) <= max(1e-12, 10 * phi_dev(c.twin.phi(c.X), pd, min(nconv, c.twin.sigma.size)))


# ---------------------------------------------------------------------------------------------
# 4. stored order
# ---------------------------------------------------------------------------------------------
def test_stored_order_operator_agrees_with_host_csr(gpu_ctx, cases):
    """The same parallel operator generated on the device in the automatic tiling (4 x 4 tiles), with its device
    transpose: sigma, VtX and V agree with the host-CSR run to 1e-11 relative over the leading run, so V and X
    are in the reference order at the boundary."""
    c = cases["parallel"]
    A = hgmres.SparseOperator.siddon(24, 18, ctx=gpu_ctx)
    assert A.pixel_order("cols")[1] == 4 and A.shape == c.A.shape
    r0 = c.device(gpu_ctx)
    r = hgmres.svds(A, c.b, c.steps, c.nsv, At=A.T, X=c.X, return_vectors=True, ctx=gpu_ctx)
    run = min(r.nconv(), r0.nconv())
    print(f"stored order (4 x 4 tiles) against host CSR over {run} modes: dsigma/s1 "
          f"{np.max(np.abs(r.sigma[:run] - r0.sigma[:run])) / r0.sigma[0]:.2e} dVtX "
          f"{np.max(np.abs(r.VtX[:run] - r0.VtX[:run])) / np.max(np.abs(r0.VtX[:run])):.2e} dV "
          f"{np.max(np.abs(r.V[:, :run] - r0.V[:, :run])):.2e} dU {np.max(np.abs(r.U[:, :run] - r0.U[:, :run])):.2e}")
    assert run >= 10
    assert np.max(np.abs(r.sigma[:run] - r0.sigma[:run])) <= 1e-11 * r0.sigma[0]
    assert np.max(np.abs(r.VtX[:run] - r0.VtX[:run])) <= 1e-11 * np.max(np.abs(r0.VtX[:run]))
    assert np.max(np.abs(r.V[:, :run] - r0.V[:, :run])) <= 1e-11
    assert np.max(np.abs(r.U[:, :run] - r0.U[:, :run])) <= 1e-11


# ---------------------------------------------------------------------------------------------
# 6. breakdown and clipping
# ---------------------------------------------------------------------------------------------
def test_breakdown_on_a_rank_3_operator(gpu_ctx):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, 3)) @ rng.standard_normal((3, 5))
    b = rng.standard_normal(6)
    sd = np.linalg.svd(A, compute_uv=False)
    r = hgmres.svds(sp.csr_matrix(A), b, 5, 5, ctx=gpu_ctx)
    assert r.steps_done == 3 == Twin(A, b, 5).steps_done
    assert np.max(np.abs(r.sigma[:3] - sd[:3])) <= 1e-13 * sd[0]
    assert np.all(np.isnan(r.sigma[3:])) and np.all(np.isnan(r.resid[3:])) and np.all(np.isnan(r.utb[3:]))
    assert np.all(r.resid[:3] == 0.0)


def test_steps_are_clipped_to_the_smaller_dimension(gpu_ctx):
    rng = np.random.default_rng(1)
    A = rng.standard_normal((6, 5))
    b = rng.standard_normal(6)
    r = hgmres.svds(sp.csr_matrix(A), b, 10, 7, X=np.eye(5), return_vectors=True, ctx=gpu_ctx)
    assert r.steps_done == 5
    sd = np.linalg.svd(A, compute_uv=False)
    assert np.max(np.abs(r.sigma[:5] - sd)) <= 1e-13 * sd[0]
    assert np.all(np.isnan(r.sigma[5:])) and np.all(np.isnan(r.VtX[5:])) and np.all(np.isnan(r.V[:, 5:]))
    assert np.all(np.isnan(r.U[:, 5:])) and np.all(np.isfinite(r.U[:, :5]))
    assert np.max(np.abs(r.VtX[:5] - r.V[:, :5].T)) <= 1e-14     # X = I: VtX is V' itself


@pytest.fixture(scope="module")
def shaw_problem():
    return analysis.regularization_problem(32, "shaw", noise_level=1e-3, mismatch=1e-4, seed=0)


def test_shaw_breaks_down_early_with_every_triplet_exact(gpu_ctx, shaw_problem):
    P = shaw_problem
    X = solutions(P.A, P.b, P.x_true)
    d, tw = Dense(P.A, P.b), Twin(P.A, P.b, 32)
    E = hgmres.empirical_filter_factors(P.A, P.b, X, 32, 32, ctx=gpu_ctx)
    r = E.svds
    print(f"shaw(32): steps_done {r.steps_done} (twin {tw.steps_done})")
    assert r.steps_done < 32 and np.all(np.isnan(r.sigma[r.steps_done:]))
    keep = np.nonzero(r.sigma[:r.steps_done] >= 1e-8 * d.s[0])[0]
    assert keep.size >= 8 and np.array_equal(keep, np.arange(keep.size))
    assert np.max(np.abs(r.sigma[keep] - d.s[keep])) <= 1e-12 * d.s[0]
    nk = min(keep.size, tw.sigma.size)
    dev, twd = phi_dev(E.Phi, d.phi(X), nk), phi_dev(tw.phi(X), d.phi(X), nk)
    print(f"shaw(32): Phi deviation from dense over {nk} modes: device {dev:.2e} twin {twd:.2e}")
    assert nk == keep.size and dev <= max(1e-12, 10 * twd)


# ---------------------------------------------------------------------------------------------
# 7. reproducibility
# ---------------------------------------------------------------------------------------------
def test_runs_are_reproducible_and_columns_independent(gpu_ctx, cases):
    c = cases["fan"]
    r0 = c.device(gpu_ctx)
    r1 = hgmres.svds(c.A, c.b, c.steps, c.nsv, X=c.X, return_vectors=True, ctx=gpu_ctx)
    for f in ("sigma", "resid", "utb", "VtX", "U", "V"):
        assert np.array_equal(getattr(r0, f), getattr(r1, f)), f
    r2 = hgmres.svds(c.A, c.b, c.steps, c.nsv, ctx=gpu_ctx)                      # X given or not
    assert r2.VtX is None and r2.U is None
    for f in ("sigma", "resid", "utb"):
        assert np.array_equal(getattr(r0, f), getattr(r2, f)), f
    rng = np.random.default_rng(3)
    X11 = np.column_stack([c.X, rng.standard_normal((c.A.shape[1], 8))])         # nx = 3 and nx = 11 (8 + 3)
    r3 = hgmres.svds(c.A, c.b, c.steps, c.nsv, X=X11, ctx=gpu_ctx)
    assert np.array_equal(r3.VtX[:, :3], r0.VtX)
    r4 = hgmres.svds(c.A, c.b, c.steps, c.nsv, X=X11[:, ::-1], ctx=gpu_ctx)
    assert np.array_equal(r4.VtX[:, ::-1], r3.VtX)


def test_default_start_vector(gpu_ctx, cases):
    c = cases["parallel"]
    r = hgmres.svds(c.A, None, c.steps, c.nsv, ctx=gpu_ctx)
    run = r.nconv()
    assert r.steps_done == c.steps and run >= 5
    assert np.max(np.abs(r.sigma[:run] - c.dense.s[:run])) <= 1e-12 * c.dense.s[0]
    assert np.array_equal(r.sigma, hgmres.svds(c.A, None, c.steps, c.nsv, ctx=gpu_ctx).sigma)


# ---------------------------------------------------------------------------------------------
# 8. refusals on the device
# ---------------------------------------------------------------------------------------------
def test_svds_refusals(gpu_ctx, cases):
    c = cases["mlt"]
    A = hgmres.as_operator(c.A, gpu_ctx)
    A32 = hgmres.as_operator(c.A, gpu_ctx, dtype=L.HGM_F32)
    with pytest.raises(ValueError, match="fp64"):
        hgmres.svds(A32, c.b, 4, 2, ctx=gpu_ctx)
    with gpu_ctx.options(parity=1):
        with pytest.raises(ValueError, match="parity"):
            hgmres.svds(A, c.b, 4, 2, ctx=gpu_ctx)
    with pytest.raises(ValueError, match="size"):
        hgmres.svds(A, c.b, 4, 2, At=A, ctx=gpu_ctx)                             # At is not size(A')
    for steps, nsv in ((0, 1), (4, 0), (4, 5)):
        with pytest.raises(ValueError):
            hgmres.svds(A, c.b, steps, nsv, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        hgmres.svds(A, c.b, 4, 2, X=np.ones((A.shape[1], 65)), ctx=gpu_ctx)
    lib, done, buf = hgmres.load_library(), C.c_int(0), (C.c_double * 8)()
    assert lib.hgm_svds(gpu_ctx.handle, A._h, None, None, 4, 2, 0.0, None, 1, 0, buf, buf, buf, None, None, 1, None, 1,
                        C.byref(done)) == L.HGM_E_ARG                            # At NULL
    # a context with a host all-reduce hook at world 2: HGM_E_UNSUPPORTED, and the hook is never called
    calls = []
    c2 = hgmres.Context(0)
    try:
        c2.set_host_allreduce(0, 2, lambda arr: calls.append(arr.size))
        with pytest.raises(hgmres.HgmError, match=f"status {L.HGM_E_UNSUPPORTED}"):
            hgmres.svds(c.A, c.b, 4, 2, ctx=c2)
        assert calls == []
    finally:
        c2.close()
    # the context still runs after the refusals
    assert hgmres.svds(A, c.b, 4, 2, ctx=gpu_ctx).steps_done == 4


# ---------------------------------------------------------------------------------------------
# 9. pipeline
# ---------------------------------------------------------------------------------------------
def test_filter_factor_comparison_pipeline(gpu_ctx, shaw_problem):
    """plot_filter_factors.m:14-40 on shaw(32) with B = A' + 1e-4 E: the four solutions are the existing *_bounds
    calls bit for bit, and Phi is the dense formula with the reference's guard over the modes with
    sigma >= 1e-8 sigma_1, under the bar of the empirical-factor test."""
    P = shaw_problem
    tol, maxit, lam = 1e-6, 32, 1e-3
    out = analysis.filter_factor_comparison(P.A, P.B_pert, P.b, P.x_true, maxit=maxit, tol=tol, lam=lam,
                                            DeltaM_AB=P.DeltaM_AB, DeltaM_BA=P.DeltaM_BA, steps=32, nsv=32,
                                            ctx=gpu_ctx)
    args = (P.A, P.B_pert, P.b, P.x_true, tol, maxit)
    direct = {"ab": hgmres.ABgmres_nonhybrid_bounds(*args, P.DeltaM_AB, ctx=gpu_ctx),
              "ba": hgmres.BAgmres_nonhybrid_bounds(*args, P.DeltaM_BA, ctx=gpu_ctx),
              "hab": hgmres.ABgmres_hybrid_bounds(*args, lam, P.DeltaM_AB, ctx=gpu_ctx),
              "hba": hgmres.BAgmres_hybrid_bounds(*args, lam, P.DeltaM_BA, ctx=gpu_ctx)}
    d, tw = Dense(P.A, P.b), Twin(P.A, P.b, 32)
    X = np.column_stack([direct[nm][0] for nm in ("ab", "ba", "hab", "hba")])
    keep = int(np.sum(out["sigma"][:out["steps_done"]] >= 1e-8 * d.s[0]))
    assert 8 <= keep <= tw.sigma.size
    bar = max(1e-12, 10 * phi_dev(tw.phi(X), d.phi(X), keep))
    for j, nm in enumerate(("ab", "ba", "hab", "hba")):
        assert np.array_equal(out[f"x_{nm}"], direct[nm][0]) and out[f"it_{nm}"] == direct[nm][3], nm
        assert np.array_equal(out[f"phi_{nm}"], direct[nm][4]) and np.array_equal(out[f"dphi_{nm}"], direct[nm][5])
        dev = phi_dev(out[f"Phi_emp_{nm}"][:, None], d.phi(X[:, [j]]), keep)
        print(f"shaw(32) {nm}: Phi_emp deviation from dense over {keep} modes {dev:.2e} (bar {bar:.2e})")
        assert dev <= bar, nm


# ---------------------------------------------------------------------------------------------
# 10. gateway
# ---------------------------------------------------------------------------------------------
def test_gateway_returns_the_binding_bits(gpu_ctx, cases):
    from conftest import ROOT
    from mwrap import Function
    from test_mex_gateway import Mex
    import os
    c = cases["mlt"]
    mex = Mex()
    steps, nsv = 30, 8
    A = sp.csr_matrix(c.A)
    A.sort_indices()                                   # the gateway hands MATLAB's CSC over: rows sorted by column
    r = hgmres.svds(A, c.b, steps, nsv, X=c.X, return_vectors=True, ctx=gpu_ctx)
    E = hgmres.empirical_filter_factors(A, c.b, c.X, steps, nsv, ctx=gpu_ctx)
    f = Function(os.path.join(ROOT, "matlab", "svds_gk.m"), mex)
    sigma, resid, utb, done, VtX, U, V = f(7, sp.csc_matrix(A), c.b, float(steps), float(nsv), c.X)
    assert int(done[0]) == r.steps_done == steps
    for got, want in ((sigma, r.sigma), (resid, r.resid), (utb, r.utb), (VtX, r.VtX), (U, r.U), (V, r.V)):
        assert np.array_equal(got, want)
    s3 = f(3, sp.csc_matrix(A), c.b, float(steps), float(nsv))                               # no X, no vectors
    assert np.array_equal(s3[0], r.sigma) and np.array_equal(s3[2], r.utb)
    g = Function(os.path.join(ROOT, "matlab", "empirical_filter_factors.m"), mex)
    sigma2, Phi, resid2, nconv = g(4, sp.csc_matrix(A), c.b, c.X, float(steps), float(nsv))
    assert np.array_equal(sigma2, E.sigma) and np.array_equal(Phi, E.Phi) and np.array_equal(resid2, E.resid)
    assert int(nconv[0]) == E.nconv
