"""The unmatched fan-beam back-projector without a GPU: the numpy twin
(hgmres.problems.fan_pixel_backprojector) against its definition (include/hgmres.h,
hgm_mat_create_fan_backprojector), the problem builder and the binding's surface.

* structure at (N, n_angles) = (1,1), (2,3), (24,30), (32,90), (48,37): shape, sorted columns, values in
  (0, 1], per (pixel, source) an adjacent pair of weights summing to 1 within 2 ulp or nothing;
* the entry counts of a numpy prototype of the definition (32^2/90: every pair inside the fan,
  nnz = 2 * 90 * 1024; 24^2/30: two pairs outside, nnz = 34,556);
* the computed signs s(d) are monotone in d for every (pixel, source) of these shapes, which is what lets
  the device kernel start from a guess and still return the bisection's bracket;
* half the default span: rows lose pairs, the count is a brute-force evaluation's;
* B is a back-projector for the fan-beam A: cosine with A' >= 0.9 (a wrong orientation or index order
  fails it; the prototype gives 0.947), and the oracle's ABgmres_nonhybrid_bounds on (A, B) reaches a
  relative error <= 0.2 at k = 12 on the 1 % noise problem (the prototype gives 0.119);
* tomo_problem returns the pair and refuses the three mixed requests;
* symbols and signatures, as test_batch_cpu.py checks them.
"""
import functools
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from hgmres.problems import (DETECTOR_OFFSET, FAN_R, _fan_tables, fan_pixel_backprojector, fan_pixel_sides,
                             fanbeam_projector, geometry, tomo_problem)
from oracle import restatement as R   # checker only

SHAPES = [(1, 1), (2, 3), (24, 30), (32, 90), (48, 37)]
EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _twin(N, na, span=None):
    B = fan_pixel_backprojector(N, na, span=span)
    for a in (B.data, B.indices, B.indptr):
        a.setflags(write=False)
    return B


def _sides(N, na, span=None):
    """s(d) for every (pixel, source, d) of a small shape: N^2 x na x p."""
    p, D, cb, sb, co, so = _fan_tables(N, na, FAN_R, span, DETECTOR_OFFSET)
    along, across = fan_pixel_sides(N, np.arange(N * N), cb, sb, D)
    return p, across[:, :, None] * co[None, None, :] - along[:, :, None] * so[None, None, :]


def _pairs(B, p, na):
    """Dense n x na count, first column and weight sum of the entries of each (pixel, source)."""
    n = B.shape[0]
    row = np.repeat(np.arange(n), np.diff(B.indptr))
    a = B.indices // p
    cnt = np.zeros((n, na), dtype=np.int64)
    np.add.at(cnt, (row, a), 1)
    wsum = np.zeros((n, na))
    np.add.at(wsum, (row, a), B.data)
    return row, a, cnt, wsum


@pytest.mark.parametrize("N,na", SHAPES)
def test_twin_structure(N, na):
    B = _twin(N, na)
    p = geometry(N, na)[0]
    assert B.shape == (N * N, p * na)
    assert B.indptr[0] == 0 and B.indptr[-1] == B.nnz == B.data.size
    assert B.indices.min() >= 0 and B.indices.max() < p * na
    row, a, cnt, wsum = _pairs(B, p, na)
    assert np.all(np.diff(B.indices.astype(np.int64))[row[1:] == row[:-1]] > 0)   # columns increase within rows
    assert np.all(B.data > 0) and np.all(B.data <= 1.0)
    assert set(np.unique(cnt)) <= {0, 1, 2}
    has = cnt > 0
    assert np.all(np.abs(wsum[has] - 1.0) <= 2 * EPS), float(np.max(np.abs(wsum[has] - 1.0)))
    # the two columns of a pair are adjacent and of one source
    same = (row[1:] == row[:-1]) & (a[1:] == a[:-1])
    assert np.all(B.indices[1:][same] == B.indices[:-1][same] + 1)
    assert same.sum() == (cnt == 2).sum()
    d = B.indices % p
    assert np.all(d[1:][same] >= 1)                                       # the pair does not wrap to a next source
    print(f"[fan B {N}^2/{na}] nnz={B.nnz} single-entry pairs={(cnt == 1).sum()} empty pairs={(cnt == 0).sum()}")


def test_twin_entry_counts():
    p32, p24 = geometry(32, 90)[0], geometry(24, 30)[0]
    B = _twin(32, 90)
    assert B.nnz == 184_320 == 2 * 90 * 1024
    assert np.all(_pairs(B, p32, 90)[2] == 2)                             # no pair outside the fan
    B = _twin(24, 30)
    cnt = _pairs(B, p24, 30)[2]
    assert B.nnz == 34_556
    assert (cnt == 0).sum() == 2 and (cnt == 1).sum() == 0                # 2 * (30 * 576 - 2) = 34,556


@pytest.mark.parametrize("N,na", SHAPES)
def test_signs_are_monotone_in_d(N, na):
    """s(d) >= 0 up to some d and < 0 from there on, for every (pixel, source): then the last d with
    s(d) >= 0 is the bisection's d0, whatever bracket a search starts from."""
    for span in (None, 0.5 * 2.0 * np.arcsin(1.0 / (np.sqrt(2.0) * FAN_R))):
        p, S = _sides(N, na, span)
        ge = S >= 0
        assert np.all(ge[:, :, :-1] >= ge[:, :, 1:])                      # never back from < 0 to >= 0


def _brute(N, na, span):
    """The definition by exhaustive evaluation: d0 = (number of d with s(d) >= 0) - 1 (the signs are
    monotone), weights from s(d0), s(d0+1).  Returns nnz per pixel row and the dense matrix."""
    p, S = _sides(N, na, span)
    d0 = (S >= 0).sum(axis=2) - 1
    ok = (d0 >= 0) & (d0 < p - 1)
    dc = np.where(ok, d0, 0)
    s0 = np.take_along_axis(S, dc[:, :, None], axis=2)[:, :, 0]
    s1 = np.take_along_axis(S, dc[:, :, None] + 1, axis=2)[:, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = s0 / (s0 - s1)
    w0 = 1.0 - w1
    M = np.zeros((N * N, p * na))
    pix, a = np.nonzero(ok)
    M[pix, a * p + d0[pix, a]] = w0[pix, a]
    M[pix, a * p + d0[pix, a] + 1] = w1[pix, a]
    return ok, M


@pytest.mark.parametrize("N,na", [(24, 30), (32, 90)])
def test_half_span_drops_pairs_as_brute_force_does(N, na):
    half = 0.5 * 2.0 * np.arcsin(1.0 / (np.sqrt(2.0) * FAN_R))
    B = _twin(N, na, half)
    full = _twin(N, na)
    ok, M = _brute(N, na, half)
    rows_losing = np.diff(B.indptr) < np.diff(full.indptr)
    assert rows_losing.any() and not ok.all()
    assert B.nnz == np.count_nonzero(M)
    assert np.array_equal(np.diff(B.indptr), np.count_nonzero(M, axis=1))
    assert np.array_equal(B.toarray(), M)
    # and the default span against the same brute force
    assert np.array_equal(full.toarray(), _brute(N, na, None)[1])
    print(f"[fan B {N}^2/{na} half span] nnz {full.nnz} -> {B.nnz}, {int(rows_losing.sum())} rows lose pairs")


def test_non_default_geometry_arguments_reach_the_twin():
    a = fan_pixel_backprojector(24, 30)
    for kw in (dict(R=0.75), dict(det_offset=0.0), dict(span=0.6)):
        b = fan_pixel_backprojector(24, 30, **kw)
        assert b.shape == a.shape
        assert b.nnz != a.nnz or not np.array_equal(b.data, a.data), kw
    # the chunking is invisible
    c = fan_pixel_backprojector(24, 30, chunk_elems=1000)
    assert np.array_equal(c.indptr, a.indptr) and np.array_equal(c.indices, a.indices) and np.array_equal(c.data, a.data)


def test_it_is_a_backprojector_for_the_fan_projector():
    At = sp.csr_matrix(fanbeam_projector(32, 90).T)
    B = _twin(32, 90)
    cos = B.multiply(At).sum() / (sp.linalg.norm(B, "fro") * sp.linalg.norm(At, "fro"))
    mismatch = sp.linalg.norm(B - At, "fro") / sp.linalg.norm(At, "fro")
    print(f"[fan B 32^2/90] cos(B, A') = {cos:.4f} (bar >= 0.9), ||B - A'||_F / ||A'||_F = {mismatch:.3f}")
    assert cos >= 0.9
    assert mismatch > 0.05                                                # and it is not A'


def test_oracle_ab_gmres_converges_on_the_unmatched_pair():
    P = tomo_problem(32, 90, noise=1e-2, seed=0, backprojector="fanpixel", geometry_kind="fan")
    x, err, res, k = R.ABgmres_nonhybrid_bounds(P.A, P.B, P.b, P.x_true, 0.0, 12)
    print(f"[fan B 32^2/90] oracle ABgmres_nonhybrid_bounds: relative error {err[-1]:.4f} at k = {k} (bar <= 0.2)")
    assert k == 12 and err[-1] <= 0.2


def test_tomo_problem_pair_and_refusals():
    P = tomo_problem(24, 30, backprojector="fanpixel", geometry_kind="fan")
    A, B = fanbeam_projector(24, 30), _twin(24, 30)
    assert P.A.shape == A.shape and np.array_equal(P.A.data, A.data) and np.array_equal(P.A.indices, A.indices)
    assert P.B.shape == B.shape == (A.shape[1], A.shape[0])
    assert np.array_equal(P.B.indptr, B.indptr) and np.array_equal(P.B.indices, B.indices)
    assert np.array_equal(P.B.data, B.data)
    M = tomo_problem(24, 30, geometry_kind="fan")                         # the matched pair is what it was
    assert np.array_equal(M.b, P.b) and abs(M.B - M.A.T).max() == 0
    with pytest.raises(ValueError):
        tomo_problem(24, 30, backprojector="pixel", geometry_kind="fan")
    with pytest.raises(ValueError):
        tomo_problem(24, 30, backprojector="fanpixel", geometry_kind="parallel")
    with pytest.raises(ValueError):
        tomo_problem(24, 30, backprojector="fanpixel")                    # parallel is the default geometry
    with pytest.raises(ValueError):
        tomo_problem(24, 30, backprojector="nearest", geometry_kind="fan")


def test_symbol_and_signatures():
    lib = hgmres.load_library()
    name = "hgm_mat_create_fan_backprojector"
    assert hasattr(lib, name) and name in L.declared_symbols()
    assert lib.hgm_mat_create_fan_backprojector(None, 8, 4, 2.0, 0.0, 0.25, L.HGM_F64, 1, 0, None) == L.HGM_E_ARG
    sig = inspect.signature(hgmres.SparseOperator.fan_backprojector)
    assert list(sig.parameters) == list(inspect.signature(hgmres.SparseOperator.fanbeam).parameters)
    for kw, default in (("ctx", None), ("R", None), ("span", None), ("dtype", L.HGM_F64), ("det_offset", None),
                        ("order", "auto")):
        assert sig.parameters[kw].default == default, kw
    sig = inspect.signature(fan_pixel_backprojector)
    assert list(sig.parameters)[:5] == ["N", "n_angles", "R", "span", "det_offset"]
    assert sig.parameters["R"].default == FAN_R and sig.parameters["span"].default is None
    assert sig.parameters["det_offset"].default == DETECTOR_OFFSET
