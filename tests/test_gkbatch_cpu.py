"""The lockstep Golub-Kahan solves' surface without a GPU: exported and declared symbols, argument
statuses that need no device, the Python signatures, shape validation ahead of any upload, and the
gateway command's dispatch and argument checks through the mx API stand-in."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from hgmres import analysis
from test_mex_gateway import Mex, MexError

SYMBOLS = ("hgm_mv_axpby_norms", "hgm_gk_batch")


def test_symbols_exported_and_declared():
    lib = hgmres.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.declared_symbols(), name
    assert (L.HGM_GK_LSQR, L.HGM_GK_LSMR) == (0, 1)


def _batch_null(lib, kind, hybrid=0):
    one = (C.c_double * 1)(1.0)
    nit = (C.c_int * 1)(0)
    return lib.hgm_gk_batch(None, None, None, None, one, 1, 1, None, 0, 0.0, 3, one, kind, hybrid, None, 1, None, None,
                            None, nit)


def test_null_context_and_bad_kind_are_argument_errors():
    lib = hgmres.load_library()
    one = (C.c_double * 1)(1.0)
    assert lib.hgm_mv_axpby_norms(None, 1, 1, one, None, 1, one, None, 1, None, 1, None) == L.HGM_E_ARG
    for kind in (L.HGM_GK_LSQR, L.HGM_GK_LSMR):
        for hybrid in (0, 1):
            assert _batch_null(lib, kind, hybrid) == L.HGM_E_ARG
    for kind in (-1, 2, 7):
        assert _batch_null(lib, kind) == L.HGM_E_ARG


def test_python_signatures():
    assert callable(hgmres.gk_batch) and callable(hgmres.mv_axpby_norms)
    for name in ("gk_batch", "mv_axpby_norms", "GKBatchResult"):
        assert name in hgmres.__all__, name
    sig = inspect.signature(hgmres.gk_batch)
    assert list(sig.parameters) == ["A", "Bm", "x_true", "tol", "maxit", "kind", "lambdas", "At", "ctx"]
    for kw in ("lambdas", "At", "ctx"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default is None
    sig = inspect.signature(hgmres.mv_axpby_norms)
    assert list(sig.parameters) == ["a", "X", "b", "Y", "ctx"] and sig.parameters["ctx"].default is None
    R = hgmres.GKBatchResult(1, 2, 3, 4, 5)
    assert (R.x, R.error_norm, R.residual_norm, R.ar_norm, R.niters) == (1, 2, 3, 4, 5)
    sig = inspect.signature(analysis.equivalence_vs_noise_level)
    assert list(sig.parameters)[:4] == ["A", "b_exact", "x_true", "noise_levels"]
    for kw, default in (("tol", 1e-6), ("lam", 1e-3), ("seed", 0), ("ctx", None)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert sig.parameters["maxit"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["maxit"].default is inspect.Parameter.empty


def test_python_wrappers_validate_before_the_device():
    """scipy operands: nothing has been uploaded when these raise (no context exists without a GPU)."""
    A = sp.random(8, 6, density=0.5, random_state=0, format="csr")
    xt = np.ones(6)
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((7, 3)), xt, 0.0, 3, "lsqr")                         # Bm is not m x nrhs
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 0)), xt, 0.0, 3, "lsmr")                         # no right-hand side
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 65)), xt, 0.0, 3, "lsqr")                        # more than 64
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 3)), xt, 0.0, 3, "hybrid_lsqr", lambdas=[1.0, 2.0])   # wrong length
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 3)), xt, 0.0, 3, "hybrid_lsmr")                  # hybrid needs lambdas
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones(8), xt, 0.0, 3, "hybrid_lsmr", lambdas=[1.0, -2.0])  # shared b, a negative lambda
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones(7), xt, 0.0, 3, "hybrid_lsqr", lambdas=[1.0, 2.0])   # shared b of the wrong length
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 3)), np.ones((6, 2)), 0.0, 3, "lsqr")            # x_true columns
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 3)), xt, 0.0, 3, "cgls")                         # a bad kind
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 3)), xt, 0.0, 0, "lsqr")                         # maxit < 1
    with pytest.raises(ValueError):
        hgmres.gk_batch(A, np.ones((8, 3)), xt, 0.0, 3, "lsqr", At=A)                   # At is not n x m
    with pytest.raises(ValueError):
        hgmres.mv_axpby_norms([1.0, 2.0], np.ones((5, 2)), [1.0, 2.0], np.ones((5, 3)))  # X and Y differ
    with pytest.raises(ValueError):
        hgmres.mv_axpby_norms(np.ones(9), np.ones((5, 9)), np.ones(9), np.ones((5, 9)))  # more than 8 vectors
    with pytest.raises(ValueError):
        hgmres.mv_axpby_norms([1.0], np.ones((5, 2)), [1.0, 2.0], np.ones((5, 2)))       # one coefficient per vector
    with pytest.raises(ValueError):
        analysis.equivalence_vs_noise_level(A, np.ones(7), xt, [1e-3], maxit=3)
    with pytest.raises(ValueError):
        analysis.equivalence_vs_noise_level(A, np.ones(8), xt, [], maxit=3)
    with pytest.raises(ValueError):
        analysis.equivalence_vs_noise_level(A, np.ones(8), xt, [1e-3], maxit=3, lam=-1.0)


@pytest.fixture(scope="module")
def mex():
    return Mex()


def test_gateway_dispatches_the_gk_batch_command(mex):
    """The command exists (argument errors, not 'unknown function'), and it checks the kind, sizes and
    lambdas before it touches a device."""
    A = sp.random(8, 6, density=0.5, random_state=0, format="csc")
    Bm, xt = np.ones((8, 3)), np.ones(6)
    with pytest.raises(MexError) as e:
        mex(5, "gk_batch", "lsqr", A, Bm)
    assert e.value.ident == "hgmres:nargin"
    with pytest.raises(MexError) as e:
        mex(5, "gk_batch", "cgls", A, Bm, xt, 0.0, 3.0)
    assert e.value.ident == "hgmres:arg"
    for bad in (np.array([1.0, -2.0, 3.0]), np.array([1.0, np.nan, 3.0]), np.array([1.0, 2.0])):
        with pytest.raises(MexError) as e:
            mex(5, "gk_batch", "hybrid_lsqr", A, Bm, xt, 0.0, 3.0, bad)
        assert e.value.ident == "hgmres:arg", e.value
    with pytest.raises(MexError) as e:                                   # hybrid without lambdas
        mex(5, "gk_batch", "hybrid_lsmr", A, Bm, xt, 0.0, 3.0)
    assert e.value.ident == "hgmres:arg"
    for bad_Bm, bad_xt in ((np.ones((7, 3)), xt), (Bm, np.ones(5)), (Bm, np.ones((6, 2))), (np.ones((8, 65)), xt)):
        with pytest.raises(MexError) as e:
            mex(5, "gk_batch", "lsmr", A, bad_Bm, bad_xt, 0.0, 3.0)
        assert e.value.ident == "hgmres:arg", e.value
    with pytest.raises(MexError) as e:
        mex(5, "gk_batch", "lsqr", A, Bm, xt, 0.0, 0.0)                  # maxit < 1
    assert e.value.ident == "hgmres:arg"
