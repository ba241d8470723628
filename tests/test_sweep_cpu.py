"""The lambda sweep's surface without a GPU: exported and declared symbols, NULL-context status, the
pipeline entry points, and the gateway command's dispatch through the mx API stand-in."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from hgmres import analysis
from test_mex_gateway import Mex, MexError

SYMBOLS = ("hgm_gmres_bounds_sweep", "hgm_proj_norms", "hgm_proj_norms_loop")


def test_symbols_exported_and_declared():
    lib = hgmres.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.declared_symbols(), name


def test_null_context_is_an_argument_error():
    lib = hgmres.load_library()
    one = (C.c_double * 1)(1.0)
    nit = (C.c_int * 1)(0)
    assert lib.hgm_proj_norms(None, 4, 1, None, 4, None, 1, 1, None, one, None) == L.HGM_E_ARG
    assert lib.hgm_proj_norms_loop(None, 4, 1, None, 4, None, 1, 1, None, one) == L.HGM_E_ARG
    for side in (L.HGM_SIDE_AB, L.HGM_SIDE_BA):
        assert lib.hgm_gmres_bounds_sweep(None, None, None, None, None, None, 0.0, 3, one, 1, side, None, None, None,
                                          None, nit, None) == L.HGM_E_ARG
    assert lib.hgm_gmres_bounds_sweep(None, None, None, None, None, None, 0.0, 3, one, 1, 7, None, None, None, None,
                                      nit, None) == L.HGM_E_ARG


def test_pipeline_entry_points_exist():
    assert callable(hgmres.gmres_lambda_sweep) and callable(hgmres.proj_norms)
    assert "gmres_lambda_sweep" in hgmres.__all__ and "proj_norms" in hgmres.__all__
    sig = inspect.signature(hgmres.gmres_lambda_sweep)
    assert list(sig.parameters)[:8] == ["A", "B", "b", "x_true", "tol", "maxit", "lambdas", "side"]
    for kw, default in (("ctx", None), ("orth", "mgs"), ("return_x", False), ("return_H", False)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert callable(analysis.error_surface)
    assert inspect.signature(analysis.error_surface).parameters["tol"].default == 1e-10
    p = inspect.signature(analysis.analyze_regularization).parameters["sweep"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_python_wrappers_validate_before_the_device():
    with pytest.raises(ValueError):
        hgmres.proj_norms(np.ones((4, 2)), np.ones((3, 1)))          # Y is not k x L
    with pytest.raises(ValueError):
        hgmres.proj_norms(np.ones((0, 2)), np.ones((2, 1)))


@pytest.fixture(scope="module")
def mex():
    return Mex()


def test_gateway_dispatches_the_sweep_command(mex):
    """The command exists (argument errors, not 'unknown function'), and it checks the side and the
    lambdas before it touches a device."""
    A = sp.random(8, 6, density=0.5, random_state=0, format="csc")
    B = sp.csc_matrix(A.T)
    b, xt = np.ones(8), np.ones(6)
    with pytest.raises(MexError) as e:
        mex(4, "gmres_lambda_sweep", "ab", A, B)
    assert e.value.ident == "hgmres:nargin"
    with pytest.raises(MexError) as e:
        mex(4, "gmres_lambda_sweep", "sideways", A, B, b, xt, 0.0, 3.0, np.array([1.0, 2.0]))
    assert e.value.ident == "hgmres:arg"
    for bad in (np.array([1.0, -2.0]), np.array([np.nan]), np.zeros((0, 0))):
        with pytest.raises(MexError) as e:
            mex(4, "gmres_lambda_sweep", "ba", A, B, b, xt, 0.0, 3.0, bad)
        assert e.value.ident == "hgmres:arg", e.value
