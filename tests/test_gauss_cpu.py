"""The matrix-free dense Gaussian perturbation without a GPU: the Philox4x32-10 known answers, the numpy
twin of the device generator (hgmres.problems.gaussian_entries), the nine hgm_gauss_* symbols in the header,
the export table and the ctypes table, the NULL-argument refusals and the Python ValueErrors that are raised
before any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import hgmres
from hgmres import _lib as L
from hgmres.problems import gaussian_entries, philox4x32_10

GAUSS_SYMBOLS = ["hgm_gauss_create", "hgm_gauss_destroy", "hgm_gauss_info", "hgm_gauss_entries", "hgm_gauss_fro",
                 "hgm_gauss_mm", "hgm_spmm_pert_gauss", "hgm_gmres_bounds_mismatch_gauss",
                 "hgm_arnoldi_mismatch_gauss"]

KATS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KATS)
def test_philox_known_answers(ctr, key, want):
    got = philox4x32_10(*[np.uint64(v) for v in ctr + key])
    assert tuple(int(w) for w in got) == want


def test_philox_is_vectorised():
    c = np.array([[k[0][i] for k in KATS] for i in range(4)], dtype=np.uint64)
    k = np.array([[k[1][i] for k in KATS] for i in range(2)], dtype=np.uint64)
    got = philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1])
    for j, (_, _, want) in enumerate(KATS):
        assert tuple(int(w[j]) for w in got) == want


def test_twin_blocks_are_slices_of_larger_blocks():
    rows, cols, seed = 37, 53, 0x1234567890abcdef
    full = gaussian_entries(rows, cols, seed)
    assert full.shape == (rows, cols) and np.all(np.isfinite(full))
    # blocks that start and end inside column quads, single rows / columns, the last partial quad
    for i0, ni, j0, nj in [(0, 37, 0, 53), (5, 9, 1, 2), (5, 9, 3, 6), (36, 1, 50, 3), (0, 1, 0, 1), (7, 3, 2, 1),
                           (10, 20, 7, 41), (0, 37, 52, 1), (3, 0, 4, 5), (3, 4, 4, 0)]:
        blk = gaussian_entries(rows, cols, seed, i0, ni, j0, nj)
        assert blk.shape == (ni, nj)
        assert np.array_equal(blk, full[i0:i0 + ni, j0:j0 + nj])
    # an entry depends on (seed, i, j) alone: not on the matrix it is a part of
    assert np.array_equal(gaussian_entries(100, 200, seed, 0, rows, 0, cols), full)
    assert not np.array_equal(gaussian_entries(rows, cols, seed + 1), full)
    assert not np.array_equal(gaussian_entries(rows, cols, seed ^ (1 << 40)), full)      # the key's high word
    with pytest.raises(ValueError):
        gaussian_entries(rows, cols, seed, 30, 8, 0, 1)
    with pytest.raises(ValueError):
        gaussian_entries(0, 3, 1)


def test_twin_splits_the_counter_at_64_bits():
    lo = gaussian_entries(1 << 33, 1 << 35, 9, 3, 4, 6, 8)
    hi = gaussian_entries(1 << 33, 1 << 35, 9, (1 << 32) + 3, 4, (1 << 34) + 6, 8)
    hj = gaussian_entries(1 << 33, 1 << 35, 9, 3, 4, (1 << 34) + 6, 8)
    assert not np.array_equal(lo, hi) and not np.array_equal(lo, hj) and not np.array_equal(hi, hj)


def test_twin_moments():
    rows, cols = 1000, 5003
    G = gaussian_entries(rows, cols, 12345)
    N = rows * cols
    assert abs(G.mean()) <= 6.0 / np.sqrt(N)
    assert abs(np.sum(G * G) - N) <= 6.0 * np.sqrt(2.0 * N)          # chi^2 with N degrees of freedom, 6 sigma
    assert np.max(np.abs(G)) <= 6.77


def test_gauss_symbols_in_header_exports_and_ctypes():
    txt = open(os.path.join(ROOT, "include", "hgmres.h")).read()
    header = set(re.findall(r"HGM_API\s+[\w\s\*]+?\b(hgm_\w+)\s*\(", txt))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    declared = set(L.declared_symbols())
    lib = hgmres.load_library()
    for s in GAUSS_SYMBOLS:
        assert s in header and s in exported and s in declared, s
        assert hasattr(lib, s)
    assert {s for s in header | exported | declared if "gauss" in s} == set(GAUSS_SYMBOLS)


def test_null_arguments_are_refused_without_a_device():
    lib = hgmres.load_library()
    h = C.c_void_p()
    d = C.c_double()
    one = (C.c_double * 1)(1.0)
    nit = (C.c_int * 1)()
    fake = C.c_void_p(1)          # never dereferenced: another argument is NULL
    assert lib.hgm_gauss_create(None, 3, 4, 0, C.byref(h)) == L.HGM_E_ARG
    assert lib.hgm_gauss_create(fake, 3, 4, 0, None) == L.HGM_E_ARG
    assert lib.hgm_gauss_info(None, None, None, None) == L.HGM_E_ARG
    assert lib.hgm_gauss_entries(None, fake, 0, 1, 0, 1, one, 1) == L.HGM_E_ARG
    assert lib.hgm_gauss_entries(fake, None, 0, 1, 0, 1, one, 1) == L.HGM_E_ARG
    assert lib.hgm_gauss_entries(fake, fake, 0, 1, 0, 1, None, 1) == L.HGM_E_ARG
    assert lib.hgm_gauss_fro(None, fake, C.byref(d)) == L.HGM_E_ARG
    assert lib.hgm_gauss_fro(fake, None, C.byref(d)) == L.HGM_E_ARG
    assert lib.hgm_gauss_fro(fake, fake, None) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(None, fake, 1, None, fake, 1, fake, 1) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(fake, None, 1, None, fake, 1, fake, 1) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(fake, fake, 1, None, None, 1, fake, 1) == L.HGM_E_ARG
    assert lib.hgm_gauss_mm(fake, fake, 1, None, fake, 1, None, 1) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(None, fake, fake, 1, one, fake, 1, fake, 1) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(fake, None, fake, 1, one, fake, 1, fake, 1) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(fake, fake, None, 1, one, fake, 1, fake, 1) == L.HGM_E_ARG
    assert lib.hgm_spmm_pert_gauss(fake, fake, fake, 1, None, fake, 1, fake, 1) == L.HGM_E_ARG
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake),
                 (fake, fake, fake, None)):
        c, A, B0, G = args
        assert lib.hgm_gmres_bounds_mismatch_gauss(c, None, A, B0, G, one, 1, one, None, 0.0, 1, None, L.HGM_SIDE_BA,
                                                   0, None, 1, None, None, nit, None) == L.HGM_E_ARG
        assert lib.hgm_arnoldi_mismatch_gauss(c, A, B0, G, one, 1, one, 1, L.HGM_SIDE_BA, 0.0, L.HGM_MGS, one, one,
                                              nit) == L.HGM_E_ARG
    assert lib.hgm_gmres_bounds_mismatch_gauss(fake, None, fake, fake, fake, None, 1, one, None, 0.0, 1, None,
                                               L.HGM_SIDE_BA, 0, None, 1, None, None, nit, None) == L.HGM_E_ARG
    assert lib.hgm_arnoldi_mismatch_gauss(fake, fake, fake, fake, one, 1, None, 1, L.HGM_SIDE_BA, 0.0, L.HGM_MGS, one,
                                          one, nit) == L.HGM_E_ARG
    lib.hgm_gauss_destroy(None)    # a no-op


class _Shape:
    """Stands in for an operator or a perturbation where only the shape is looked at."""

    def __init__(self, *shape):
        self.shape = shape


def _fake_gauss(rows, cols, scale=1.0):
    G = object.__new__(hgmres.GaussianPerturbation)
    G.ctx, G.shape, G.seed, G.scale, G._handle, G._root = None, (rows, cols), 0, scale, None, G
    return G


def test_python_value_errors_before_any_device_call():
    with pytest.raises(ValueError):
        hgmres.GaussianPerturbation(0, 4)
    with pytest.raises(ValueError):
        hgmres.GaussianPerturbation(4, 0)
    with pytest.raises(ValueError):
        hgmres.GaussianPerturbation(4, 4, seed=-1)
    with pytest.raises(ValueError):
        hgmres.GaussianPerturbation(4, 4, seed=1 << 64)
    with pytest.raises(ValueError):
        hgmres.GaussianPerturbation(4, 4, scale=np.inf)
    A = sp.random(12, 9, density=0.5, format="csr", random_state=0)
    b = np.ones(12)
    for fn, tail in ((hgmres.gmres_bounds_mismatch, (b, None, 0.0, 3, "ba")), (hgmres.arnoldi_mismatch, (b, 3, "ba"))):
        with pytest.raises(ValueError, match="shape"):
            fn(A, A.T.tocsr(), _fake_gauss(9, 11), [1.0], *tail)               # G's shape is not B0's
        with pytest.raises(ValueError, match="expected size"):
            fn(A, _Shape(9, 11), _fake_gauss(9, 11), [1.0], *tail)             # B0 is not size(A')
        with pytest.raises(ValueError, match="finite"):
            fn(A, A.T.tocsr(), _fake_gauss(9, 12), [np.nan], *tail)
        with pytest.raises(ValueError, match="finite"):
            fn(A, A.T.tocsr(), _fake_gauss(9, 12, scale=1e308), [1e10], *tail)  # the scaled coefficient overflows
        with pytest.raises(ValueError, match="coefficients"):
            fn(A, A.T.tocsr(), _fake_gauss(9, 12), np.ones(65), *tail)
    with pytest.raises(ValueError, match="shapes"):
        hgmres.analysis.error_vs_mismatch_norm(A, A.T.tocsr(), _fake_gauss(9, 11), b, np.ones(9), [1e-3], maxit=3)
    G = _fake_gauss(9, 12)
    with pytest.raises(ValueError):
        G.matmat(np.ones((11, 2)))
    with pytest.raises(ValueError):
        G.matmat(np.ones((12, 9)))
    with pytest.raises(ValueError):
        G.matmat(np.ones((12, 2)), coefs=[1.0])
    with pytest.raises(ValueError):
        G.entries(slice(0, 9, 2))
    with pytest.raises(ValueError):
        _fake_gauss(1 << 20, 1 << 20).to_dense()
    with pytest.raises(ValueError):
        _fake_gauss(1 << 20, 1 << 20).entries()
