"""Host side of the mismatch sweep (no GPU): the argument checks the Python bindings make before anything is
uploaded, ``mismatch_norms``, and the 64-level chunking of ``analysis.error_vs_mismatch_norm`` with the device
calls stubbed."""
import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from hgmres import analysis, core

M_, N_ = 6, 4


def _op(shape, dtype=L.HGM_F64):
    """A SparseOperator that owns nothing on a device (the checks under test run before any device call)."""
    return core.SparseOperator(None, None, shape, 0, dtype)


@pytest.fixture
def ops():
    return _op((M_, N_)), _op((N_, M_)), _op((N_, M_))


def test_spmm_pert_argument_checks(ops):
    _, B0, E = ops
    X = np.ones((M_, 2))
    with pytest.raises(ValueError, match="shape"):
        hgmres.spmm_pert(B0, _op((N_, M_ + 1)), [1.0, 2.0], X)
    with pytest.raises(ValueError, match="fp64"):
        hgmres.spmm_pert(B0, _op((N_, M_), L.HGM_F32), [1.0, 2.0], X)
    with pytest.raises(ValueError, match="fp64"):
        hgmres.spmm_pert(_op((N_, M_), L.HGM_F32), E, [1.0, 2.0], X)
    with pytest.raises(TypeError):
        hgmres.spmm_pert(sp.csr_matrix((N_, M_)), E, [1.0, 2.0], X)
    with pytest.raises(ValueError, match="expected"):
        hgmres.spmm_pert(B0, E, [1.0, 2.0], np.ones((M_ + 1, 2)))
    with pytest.raises(ValueError, match="1 to 8 vectors"):
        hgmres.spmm_pert(B0, E, np.ones(9), np.ones((M_, 9)))
    with pytest.raises(ValueError, match="coefficients"):
        hgmres.spmm_pert(B0, E, [1.0], X)                    # one coefficient per vector
    with pytest.raises(ValueError, match="finite"):
        hgmres.spmm_pert(B0, E, [1.0, np.inf], X)


@pytest.mark.parametrize("call", ["solve", "arnoldi"])
def test_mismatch_binding_argument_checks(ops, call):
    A, B0, E = ops
    b, xt = np.ones(M_), np.ones(N_)
    if call == "solve":
        run = lambda A_=A, B_=B0, E_=E, c=(0.1, 0.2), b_=b: hgmres.gmres_bounds_mismatch(A_, B_, E_, c, b_, xt, 0.0, 3, "ab")
    else:
        run = lambda A_=A, B_=B0, E_=E, c=(0.1, 0.2), b_=b: hgmres.arnoldi_mismatch(A_, B_, E_, c, b_, 3, "ab")
    with pytest.raises(ValueError, match="B0 is"):
        run(B_=_op((N_ + 1, M_)))
    with pytest.raises(ValueError, match="E has shape"):
        run(E_=_op((N_, M_ + 1)))
    with pytest.raises(ValueError, match="1 to 64 coefficients"):
        run(c=())
    with pytest.raises(ValueError, match="1 to 64 coefficients"):
        run(c=np.linspace(0, 1, 65))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            run(c=(0.1, bad))
    with pytest.raises(ValueError, match="b has length"):
        run(b_=np.ones(M_ + 1))


def test_mismatch_solve_argument_checks(ops):
    A, B0, E = ops
    b, xt = np.ones(M_), np.ones(N_)
    with pytest.raises(ValueError, match="side"):
        hgmres.gmres_bounds_mismatch(A, B0, E, [0.1], b, xt, 0.0, 3, "aa")
    with pytest.raises(ValueError, match="maxit"):
        hgmres.gmres_bounds_mismatch(A, B0, E, [0.1], b, xt, 0.0, 0, "ab")
    with pytest.raises(ValueError, match="one per coefficient"):
        hgmres.gmres_bounds_mismatch(A, B0, E, [0.1, 0.2], b, xt, 0.0, 3, "ab", lambdas=[1.0])
    with pytest.raises(ValueError, match="x_true has length"):
        hgmres.gmres_bounds_mismatch(A, B0, E, [0.1], b, np.ones(N_ + 1), 0.0, 3, "ab")
    with pytest.raises(ValueError, match="k must be"):
        hgmres.arnoldi_mismatch(A, B0, E, [0.1], b, 0, "ba")
    with pytest.raises(ValueError, match="side"):
        hgmres.arnoldi_mismatch(A, B0, E, [0.1], b, 3, "xx")


def test_option_39_is_declared():
    import os
    import re
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "hgmres.h")).read()
    assert L.option_id("pert_shared") == 39
    assert re.search(r"HGM_OPT_PERT_SHARED\s*=\s*39\b", txt)


# ---------------------------------------------------------------------------------------------
# error_vs_mismatch_norm with the device calls stubbed
# ---------------------------------------------------------------------------------------------
class _Stub:
    """Stands in for core.as_operator / arnoldi_mismatch / gmres_bounds_mismatch and records the calls.  The
    'solve' of level c ends after 1 + (index of the call's column) % 3 iterations with final error c + offset."""

    def __init__(self, maxit):
        self.maxit = maxit
        self.solves, self.arnoldis = [], []

    def as_operator(self, M, ctx=None, dtype=L.HGM_F64):
        return M

    def arnoldi_mismatch(self, A, B0, E, coefs, b, k, gcv_type="ba", *, ctx=None, **kw):
        coefs = np.asarray(coefs)
        assert 1 <= coefs.size <= 64
        self.arnoldis.append((gcv_type, coefs.copy(), k))
        H = np.zeros((coefs.size, k + 1, k))
        for j in range(coefs.size):
            H[j, :k, :] = np.eye(k) * (2.0 + coefs[j])
            H[j, np.arange(1, k + 1), np.arange(k)] = 0.5
        return H, np.ones(coefs.size), np.full(coefs.size, k)

    def gmres_bounds_mismatch(self, A, B0, E, coefs, b, x_true, tol, maxit, side, *, lambdas=None, ctx=None, **kw):
        coefs = np.asarray(coefs)
        nc = coefs.size
        assert 1 <= nc <= 64
        assert lambdas is None or len(lambdas) == nc
        self.solves.append((side, coefs.copy(), None if lambdas is None else np.asarray(lambdas).copy()))
        nit = 1 + np.arange(nc) % 3
        err = np.full((maxit, nc), np.nan)
        for j in range(nc):
            err[: nit[j], j] = 9.0
            err[nit[j] - 1, j] = coefs[j] + (0.25 if side == "ab" else 0.5) + (0.0 if lambdas is None else 1.0)
        return core.BatchResult(np.zeros((N_, nc)), err, err.copy(), nit, np.zeros(nc, dtype=int), None)


@pytest.fixture
def stubbed(monkeypatch):
    s = _Stub(5)
    for name in ("as_operator", "arnoldi_mismatch", "gmres_bounds_mismatch"):
        monkeypatch.setattr(core, name, getattr(s, name))
    return s


def _problem():
    rng = np.random.default_rng(0)
    A = sp.csr_matrix(rng.standard_normal((M_, N_)))
    E = sp.csr_matrix(rng.standard_normal((N_, M_)))
    return A, sp.csr_matrix(A.T), E, rng.standard_normal(M_), rng.standard_normal(N_)


def test_mismatch_norms_and_chunking(stubbed):
    A, B0, E, b, xt = _problem()
    cr = np.concatenate([np.logspace(-8, -1, 149), [-0.5]])            # 150 levels: calls of 64 + 64 + 22
    lab, lba = np.linspace(1, 2, 150), np.linspace(3, 4, 150)
    M = analysis.error_vs_mismatch_norm(A, B0, E, b, xt, cr, maxit=5, lambdas=(lab, lba),
                                        solvers=("hab", "hba", "nab", "nba"), ctx=object())
    fro = np.linalg.norm(E.toarray(), "fro")
    assert np.array_equal(M["c_range"], cr)
    # two orders of summing 24 squares: within 24 eps of each other
    assert np.allclose(M["mismatch_norms"], np.abs(cr) * fro, rtol=1e-14, atol=0) and M["mismatch_norms"][-1] > 0
    assert np.array_equal(M["mismatch_norms"], np.abs(cr) * analysis._fro(E))
    assert analysis._fro(E.toarray()) == pytest.approx(fro, rel=1e-14)
    assert stubbed.arnoldis == []                            # lambdas given: no GCV Arnoldi
    assert [(s, c.size) for s, c, _ in stubbed.solves] == [(sd, n) for sd in ("ab", "ba", "ab", "ba") for n in (64, 64, 22)]
    for (side, coefs, lam), lo in zip(stubbed.solves[:3], (0, 64, 128)):
        assert np.array_equal(coefs, cr[lo:lo + 64]) and np.array_equal(lam, lab[lo:lo + 64])
    for (side, coefs, lam), lo in zip(stubbed.solves[3:6], (0, 64, 128)):
        assert np.array_equal(lam, lba[lo:lo + 64])
    assert all(lam is None for _, _, lam in stubbed.solves[6:])
    # err(end) of every level, taken at its own niters, reassembled across the chunks
    assert np.array_equal(M["final_errors_hab"], cr + 0.25 + 1.0) and np.array_equal(M["final_errors_hba"], cr + 0.5 + 1.0)
    assert np.array_equal(M["final_errors_nab"], cr + 0.25) and np.array_equal(M["final_errors_nba"], cr + 0.5)
    want_nit = np.concatenate([1 + np.arange(n) % 3 for n in (64, 64, 22)])
    for key in ("hab", "hba", "nab", "nba"):
        assert np.array_equal(M[f"niters_{key}"], want_nit)
    assert np.array_equal(M["lambda_gcv_ab"], lab) and np.array_equal(M["lambda_gcv_ba"], lba)


def test_gcv_lambdas_come_from_the_lockstep_arnoldi(stubbed):
    A, B0, E, b, xt = _problem()
    cr = np.logspace(-3, -1, 70)                             # two Arnoldi calls per side: 64 + 6
    M = analysis.error_vs_mismatch_norm(A, B0, E, b, xt, cr, maxit=5, k_gcv=4, ctx=object())
    assert [(s, c.size, k) for s, c, k in stubbed.arnoldis] == [("ab", 64, 4), ("ab", 6, 4), ("ba", 64, 4), ("ba", 6, 4)]
    assert [(s, c.size) for s, c, _ in stubbed.solves] == [("ab", 64), ("ab", 6), ("ba", 64), ("ba", 6)]
    for side, trace_m in (("ab", M_), ("ba", N_)):
        for i in (0, 63, 64, 69):
            H, beta, _ = stubbed.arnoldi_mismatch(None, None, None, cr[[i]], b, 4, side)
            assert M[f"lambda_gcv_{side}"][i] == hgmres.gcv_fminbnd(H[0], beta[0], trace_m, 1e-9, 1e-1, 1e-8)[0]
    assert np.array_equal(np.concatenate([lam for s, _, lam in stubbed.solves if s == "ab"]), M["lambda_gcv_ab"])
    assert set(M) >= {"final_errors_hab", "final_errors_hba"} and "final_errors_nab" not in M
    # only the sides a hybrid solver asks for get an Arnoldi
    stubbed.arnoldis.clear()
    M2 = analysis.error_vs_mismatch_norm(A, B0, E, b, xt, cr[:3], maxit=5, k_gcv=4, solvers=("hba", "nab"), ctx=object())
    assert [s for s, _, _ in stubbed.arnoldis] == ["ba"] and np.all(np.isnan(M2["lambda_gcv_ab"]))


def test_error_vs_mismatch_norm_argument_checks(stubbed):
    A, B0, E, b, xt = _problem()
    run = lambda **kw: analysis.error_vs_mismatch_norm(
        kw.pop("A", A), kw.pop("B0", B0), kw.pop("E", E), kw.pop("b", b), kw.pop("xt", xt), kw.pop("cr", [0.1, 0.2]),
        maxit=5, ctx=object(), **kw)
    with pytest.raises(ValueError, match="empty"):
        run(cr=[])
    with pytest.raises(ValueError, match="finite"):
        run(cr=[0.1, np.nan])
    with pytest.raises(ValueError, match="one value per mismatch level"):
        run(lambdas=([1.0], [1.0, 2.0]))
    with pytest.raises(ValueError, match="solvers"):
        run(solvers=("hab", "lsqr"))
    with pytest.raises(ValueError, match="solvers"):
        run(solvers=())
    with pytest.raises(ValueError, match="shapes"):
        run(E=sp.csr_matrix((N_, M_ + 1)))
    with pytest.raises(ValueError, match="shapes"):
        run(B0=sp.csr_matrix((N_ + 1, M_)))
    with pytest.raises(ValueError, match="lengths"):
        run(b=np.ones(M_ + 1))
    with pytest.raises(ValueError, match="lengths"):
        run(xt=np.ones(N_ + 1))
    assert stubbed.solves == [] and stubbed.arnoldis == []   # nothing ran


# ---------------------------------------------------------------------------------------------
# the C ABI and the gateway command without a device
# ---------------------------------------------------------------------------------------------
def test_symbols_and_null_arguments():
    import ctypes as C
    lib = hgmres.load_library()
    for name in ("hgm_spmm_pert", "hgm_gmres_bounds_mismatch", "hgm_arnoldi_mismatch"):
        assert hasattr(lib, name) and name in L.declared_symbols(), name
    for name in ("spmm_pert", "gmres_bounds_mismatch", "arnoldi_mismatch"):
        assert name in hgmres.__all__, name
    one = (C.c_double * 1)(1.0)
    nit = (C.c_int * 1)(0)
    assert lib.hgm_spmm_pert(None, None, None, 1, one, None, 1, None, 1) == L.HGM_E_ARG
    for side, want in ((L.HGM_SIDE_AB, L.HGM_E_ARG), (L.HGM_SIDE_BA, L.HGM_E_ARG), (7, L.HGM_E_ARG)):
        assert lib.hgm_gmres_bounds_mismatch(None, None, None, None, None, one, 1, one, None, 0.0, 3, one, side, 1, None, 1,
                                             None, None, nit, None) == want
        assert lib.hgm_arnoldi_mismatch(None, None, None, None, one, 1, one, 3, side, 1e-12, L.HGM_MGS, one, one,
                                        nit) == want


def test_gateway_dispatches_the_mismatch_command():
    """The command exists (argument errors, not 'unknown function'), and it checks side, sizes, coefficients and
    lambdas before it touches a device."""
    from test_mex_gateway import Mex, MexError
    mex = Mex()
    A = sp.random(8, 6, density=0.5, random_state=0, format="csc")
    B = sp.csc_matrix(A.T)
    E = sp.csc_matrix(A.T * 0.5)
    cf, b, xt = np.array([0.1, 0.2, 0.3]), np.ones(8), np.ones(6)
    with pytest.raises(MexError) as e:
        mex(5, "gmres_bounds_mismatch", "ab", 0.0, A, B, E)
    assert e.value.ident == "hgmres:nargin"
    with pytest.raises(MexError) as e:
        mex(5, "gmres_bounds_mismatch", "sideways", 0.0, A, B, E, cf, b, xt, 0.0, 3.0)
    assert e.value.ident == "hgmres:arg"
    for bad in (np.array([1.0, -2.0, 3.0]), np.array([1.0, np.nan, 3.0]), np.array([1.0, 2.0])):
        with pytest.raises(MexError) as e:
            mex(5, "gmres_bounds_mismatch", "ba", 1.0, A, B, E, cf, b, xt, 0.0, 3.0, bad)
        assert e.value.ident == "hgmres:arg", e.value
    with pytest.raises(MexError) as e:                                   # hybrid without lambdas
        mex(5, "gmres_bounds_mismatch", "ba", 1.0, A, B, E, cf, b, xt, 0.0, 3.0)
    assert e.value.ident == "hgmres:arg"
    cases = ((sp.csc_matrix(A), E, cf, b, xt), (B, sp.csc_matrix((6, 9)), cf, b, xt), (B, E, np.zeros(0), b, xt),
             (B, E, np.linspace(0, 1, 65), b, xt), (B, E, np.array([0.1, np.inf]), b, xt), (B, E, cf, np.ones(7), xt),
             (B, E, cf, b, np.ones(5)))
    for bad_B, bad_E, bad_cf, bad_b, bad_xt in cases:
        with pytest.raises(MexError) as e:
            mex(5, "gmres_bounds_mismatch", "ab", 0.0, A, bad_B, bad_E, bad_cf, bad_b, bad_xt, 0.0, 3.0)
        assert e.value.ident == "hgmres:arg", e.value
