"""The singular-triplet / empirical-filter-factor surface without a GPU: exported, declared and documented
symbols, argument refusals that need no device, the host SVD of a lower bidiagonal (hgm_bidiag_svd)
against numpy, the Python entry points, and the gateway command's argument checks."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import hgmres
from conftest import ROOT
from hgmres import _lib as L
from hgmres import analysis
from test_mex_gateway import Mex, MexError

SYMBOLS = ("hgm_svds", "hgm_bidiag_svd", "hgm_basis_project", "hgm_basis_rotate", "hgm_basis_project_loop",
           "hgm_basis_rotate_loop")
EPS = np.finfo(np.float64).eps


def test_symbols_exported_declared_and_documented():
    lib = hgmres.load_library()
    header = open(os.path.join(ROOT, "include", "hgmres.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.declared_symbols(), name
        assert f"HGM_API int {name}(" in header, name
    assert "plot_filter_factors.m:30" in header


def _svds(lib, ctx=None, A=None, At=None, steps=4, nsv=2, X=None, nx=0, sigma="ok", resid="ok", utb="ok", VtX=None):
    buf = (C.c_double * 64)()
    pick = lambda v: buf if v == "ok" else v     # noqa: E731
    done = C.c_int(0)
    return lib.hgm_svds(ctx, A, At, None, steps, nsv, 0.0, X, 8, nx, pick(sigma), pick(resid), pick(utb), VtX,
                        None, 8, None, 8, C.byref(done))


def test_null_arguments_are_argument_errors():
    lib = hgmres.load_library()
    one = (C.c_double * 4)()
    assert _svds(lib) == L.HGM_E_ARG                                      # no context, no operators
    assert lib.hgm_basis_project(None, 4, 1, None, 4, 1, None, 4, one) == L.HGM_E_ARG
    assert lib.hgm_basis_rotate(None, 4, 1, None, 4, 1, None, 1, None, 4, None) == L.HGM_E_ARG
    assert lib.hgm_basis_project_loop(None, 4, 1, None, 4, 1, None, 4, one) == L.HGM_E_ARG
    assert lib.hgm_basis_rotate_loop(None, 4, 1, None, 4, 1, None, 1, None, 4) == L.HGM_E_ARG
    assert lib.hgm_bidiag_svd(0, one, one, one, None, None) == L.HGM_E_ARG
    assert lib.hgm_bidiag_svd(2, None, one, one, None, None) == L.HGM_E_ARG
    assert lib.hgm_bidiag_svd(2, one, one, None, None, None) == L.HGM_E_ARG


@pytest.mark.parametrize("kw", [dict(steps=0), dict(nsv=0), dict(steps=3, nsv=4), dict(nx=-1), dict(nx=65),
                                dict(X="ok", nx=2, VtX=None), dict(sigma=None), dict(resid=None), dict(utb=None)])
def test_svds_refuses_bad_arguments_before_any_upload(kw):
    """Every scalar refusal of hgm_svds comes back as HGM_E_ARG with nothing on a device (there is none here:
    a call that reached an upload could not return an argument error)."""
    lib = hgmres.load_library()
    if kw.get("X") == "ok":
        kw = dict(kw, X=(C.c_double * 64)())
    assert _svds(lib, **kw) == L.HGM_E_ARG


def _bidiag(alpha, beta):
    k = alpha.size
    B = np.zeros((k + 1, k))
    B[np.arange(k), np.arange(k)] = alpha
    B[np.arange(1, k + 1), np.arange(k)] = beta
    return B


def _bidiag_cases():
    for k in (1, 2, 3, 17, 60):
        rng = np.random.default_rng(100 + k)
        yield f"random-{k}", rng.uniform(0.2, 1.0, k), rng.uniform(0.2, 1.0, k)
        a, b = rng.uniform(0.2, 1.0, k), rng.uniform(0.2, 1.0, k)
        b[k // 2] = 0.0                                                       # a zero beta in the middle
        yield f"zero-beta-{k}", a, b
        g = np.logspace(0, -12, 2 * k)                                        # graded entries spanning 1e-12 .. 1
        yield f"graded-{k}", g[0::2].copy(), g[1::2].copy()


@pytest.mark.parametrize("name,alpha,beta", list(_bidiag_cases()), ids=[c[0] for c in _bidiag_cases()])
def test_bidiag_svd_against_numpy(name, alpha, beta):
    k = alpha.size
    B = _bidiag(alpha, beta)
    s, P, Q = hgmres.bidiag_svd(alpha, beta)
    sd = np.linalg.svd(B, compute_uv=False)
    assert P.shape == (k + 1, k) and Q.shape == (k, k)
    assert np.all(np.diff(s) <= 0), "descending order"
    assert np.max(np.abs(s - sd)) <= 4 * EPS * k * sd[0], np.max(np.abs(s - sd)) / sd[0]
    assert np.linalg.norm(P.T @ P - np.eye(k), 2) <= 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(k), 2) <= 1e-13
    assert np.linalg.norm(B - P @ np.diag(s) @ Q.T, 2) / sd[0] <= 1e-13


def test_bidiag_svd_completes_a_zero_singular_value():
    """alpha_2 = beta_3 = 0 makes column 2 of B zero: sigma ends in an exact 0 and P still has orthonormal columns."""
    alpha, beta = np.array([1.0, 0.0, 0.5]), np.array([0.3, 0.0, 0.2])
    s, P, Q = hgmres.bidiag_svd(alpha, beta)
    assert s[-1] == 0.0
    assert np.linalg.norm(P.T @ P - np.eye(3), 2) <= 1e-13 and np.linalg.norm(Q.T @ Q - np.eye(3), 2) <= 1e-13
    assert np.linalg.norm(_bidiag(alpha, beta) - P @ np.diag(s) @ Q.T, 2) <= 1e-13


def test_python_entry_points():
    for name in ("svds", "empirical_filter_factors", "basis_project", "basis_rotate", "bidiag_svd", "SvdsResult"):
        assert callable(getattr(hgmres, name)) and name in hgmres.__all__, name
    sig = inspect.signature(hgmres.svds)
    assert list(sig.parameters)[:4] == ["A", "b", "steps", "nsv"]
    for kw, default in (("At", None), ("X", None), ("return_vectors", False), ("breakdown_tol", 0), ("ctx", None)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert list(inspect.signature(hgmres.empirical_filter_factors).parameters)[:5] == ["A", "b", "X", "steps", "nsv"]
    sig = inspect.signature(analysis.filter_factor_comparison)
    assert list(sig.parameters)[:4] == ["A", "B", "b", "x_true"]
    for kw in ("maxit", "tol", "lam", "DeltaM_AB", "DeltaM_BA", "steps", "nsv"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY, kw
    r = hgmres.SvdsResult(np.array([2.0, 1.0, 0.5, np.nan]), np.array([1e-12, 1e-11, 1e-3, np.nan]), None, None, None,
                          None, 3)
    assert r.nconv() == 2 and r.nconv(1e-2) == 3 and r.nconv(1e-13) == 0


def test_python_wrappers_validate_before_the_device():
    with pytest.raises(ValueError):
        hgmres.basis_project(np.ones((4, 2)), np.ones((3, 1)))       # X is not rows x nx
    with pytest.raises(ValueError):
        hgmres.basis_rotate(np.ones((4, 2)), np.ones((3, 1)))        # Y is not k x p
    with pytest.raises(ValueError):
        hgmres.basis_rotate(np.ones((4, 2)), np.ones((2, 1)), ldw=3)
    with pytest.raises(ValueError):
        hgmres.bidiag_svd(np.ones(3), np.ones(2))


@pytest.fixture(scope="module")
def mex():
    return Mex()


@pytest.mark.parametrize("args,ident", [
    (("svds_gk", np.eye(3)), "hgmres:nargin"),
    (("svds_gk", np.eye(3), np.ones(3), 2.0, 1.0, np.ones((3, 1)), 1.0), "hgmres:nargin"),
    (("svds_gk", np.eye(3), np.ones(4), 2.0, 1.0), "hgmres:arg"),              # b is not size(A,1) long
    (("svds_gk", np.eye(3), np.ones(3), 0.0, 1.0), "hgmres:arg"),              # steps < 1
    (("svds_gk", np.eye(3), np.ones(3), 2.5, 1.0), "hgmres:arg"),
    (("svds_gk", np.eye(3), np.ones(3), 2.0, 3.0), "hgmres:arg"),              # nsv > steps
    (("svds_gk", np.eye(3), np.ones(3), 2.0, 0.0), "hgmres:arg"),
    (("svds_gk", np.eye(3), np.ones(3), 2.0, 1.0, np.ones((4, 1))), "hgmres:arg"),   # X is not size(A,2) x nx
    (("svds_gk", np.eye(3), np.ones(3), 2.0, 1.0, np.ones((3, 65))), "hgmres:arg"),
])
def test_gateway_checks_arguments_before_the_device(mex, args, ident):
    with pytest.raises(MexError) as e:
        mex(1, *args)
    assert e.value.ident == ident
