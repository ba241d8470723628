"""The batched multi-RHS solves' surface without a GPU: exported and declared symbols, argument
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

SYMBOLS = ("hgm_spmm", "hgm_gmres_bounds_batch")


def test_symbols_exported_and_declared():
    lib = hgmres.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.declared_symbols(), name


def _batch_null(lib, side):
    one = (C.c_double * 1)(1.0)
    nit = (C.c_int * 1)(0)
    return lib.hgm_gmres_bounds_batch(None, None, None, None, one, 1, 1, None, 0, 0.0, 3, one, side, 1, None, 1, None,
                                      None, nit, None)


def test_null_context_and_bad_side_are_argument_errors():
    lib = hgmres.load_library()
    assert lib.hgm_spmm(None, None, 1, None, 1, None, 1) == L.HGM_E_ARG
    for side in (L.HGM_SIDE_AB, L.HGM_SIDE_BA):
        assert _batch_null(lib, side) == L.HGM_E_ARG
    assert _batch_null(lib, 7) == L.HGM_E_ARG


def test_python_signatures():
    assert callable(hgmres.spmm) and callable(hgmres.gmres_bounds_batch)
    for name in ("spmm", "gmres_bounds_batch", "BatchResult"):
        assert name in hgmres.__all__, name
    assert list(inspect.signature(hgmres.spmm).parameters) == ["A", "X"]
    sig = inspect.signature(hgmres.gmres_bounds_batch)
    assert list(sig.parameters)[:7] == ["A", "B", "Bm", "x_true", "tol", "maxit", "side"]
    for kw, default in (("lambdas", None), ("ctx", None), ("orth", "mgs"), ("return_H", False)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert callable(analysis.error_vs_noise_level)
    sig = inspect.signature(analysis.error_vs_noise_level)
    assert list(sig.parameters)[:5] == ["A", "B", "b_exact", "x_true", "noise_levels"]
    for kw, default in (("tol", 1e-6), ("k_gcv", 20), ("lambdas", None), ("seed", 0), ("ctx", None)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert sig.parameters["maxit"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["maxit"].default is inspect.Parameter.empty


def test_python_wrappers_validate_before_the_device():
    """scipy operands: nothing has been uploaded when these raise (no context exists without a GPU)."""
    A = sp.random(8, 6, density=0.5, random_state=0, format="csr")
    B = sp.csr_matrix(A.T)
    xt = np.ones(6)
    with pytest.raises(ValueError):
        hgmres.gmres_bounds_batch(A, B, np.ones((7, 3)), xt, 0.0, 3, "ab")            # Bm is not m x nrhs
    with pytest.raises(ValueError):
        hgmres.gmres_bounds_batch(A, B, np.ones((8, 0)), xt, 0.0, 3, "ab")            # no right-hand side
    with pytest.raises(ValueError):
        hgmres.gmres_bounds_batch(A, B, np.ones((8, 65)), xt, 0.0, 3, "ab")           # more than 64
    with pytest.raises(ValueError):
        hgmres.gmres_bounds_batch(A, B, np.ones((8, 3)), xt, 0.0, 3, "ab", lambdas=[1.0, 2.0])   # wrong length
    with pytest.raises(ValueError):
        hgmres.gmres_bounds_batch(A, B, np.ones((8, 3)), np.ones((6, 2)), 0.0, 3, "ba")          # x_true columns
    with pytest.raises(ValueError):
        hgmres.gmres_bounds_batch(A, B, np.ones((8, 3)), xt, 0.0, 3, "sideways")
    with pytest.raises(ValueError):
        analysis.error_vs_noise_level(A, B, np.ones(8), xt, [1e-3, 1e-2], maxit=3, lambdas=([1.0], [1.0, 2.0]))
    with pytest.raises(ValueError):
        analysis.error_vs_noise_level(A, B, np.ones(7), xt, [1e-3], maxit=3)


@pytest.fixture(scope="module")
def mex():
    return Mex()


def test_gateway_dispatches_the_batch_command(mex):
    """The command exists (argument errors, not 'unknown function'), and it checks side, sizes and
    lambdas before it touches a device."""
    A = sp.random(8, 6, density=0.5, random_state=0, format="csc")
    B = sp.csc_matrix(A.T)
    Bm, xt = np.ones((8, 3)), np.ones(6)
    with pytest.raises(MexError) as e:
        mex(5, "gmres_bounds_batch", "ab", 0.0, A, B)
    assert e.value.ident == "hgmres:nargin"
    with pytest.raises(MexError) as e:
        mex(5, "gmres_bounds_batch", "sideways", 0.0, A, B, Bm, xt, 0.0, 3.0)
    assert e.value.ident == "hgmres:arg"
    for bad in (np.array([1.0, -2.0, 3.0]), np.array([1.0, np.nan, 3.0]), np.array([1.0, 2.0])):
        with pytest.raises(MexError) as e:
            mex(5, "gmres_bounds_batch", "ba", 1.0, A, B, Bm, xt, 0.0, 3.0, bad)
        assert e.value.ident == "hgmres:arg", e.value
    with pytest.raises(MexError) as e:                                   # hybrid without lambdas
        mex(5, "gmres_bounds_batch", "ba", 1.0, A, B, Bm, xt, 0.0, 3.0)
    assert e.value.ident == "hgmres:arg"
    for bad_Bm, bad_xt, bad_B in ((np.ones((7, 3)), xt, B), (Bm, np.ones(5), B), (Bm, np.ones((6, 2)), B),
                                  (Bm, xt, sp.csc_matrix(A))):
        with pytest.raises(MexError) as e:
            mex(5, "gmres_bounds_batch", "ab", 0.0, A, bad_B, bad_Bm, bad_xt, 0.0, 3.0)
        assert e.value.ident == "hgmres:arg", e.value
