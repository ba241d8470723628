"""Lockstep multi-RHS / multi-lambda LSQR and LSMR solves (hgm_gk_batch) and their interleaved vector
kernel (hgm_mv_axpby_norms, csrc/gkmv.hip), on the device.

* the kernel hook against numpy bit for bit, its sums at a bound that holds for any summation order, its
  lengths around every block / wave edge and past the grid-stride cap, and its bitwise invariance under
  the vector count, the slot and the neighbours;
* the batch against the oracle's four Golub-Kahan solvers called once per column, at the project's
  Golub-Kahan bar (test_gpu_parity._gkb_check), with stopping tolerances at which columns leave the
  batch at different iterations, and against the library's single solvers at the same bar; on an operator in
  a stored pixel order against the reference-order one at that bar, one x_true per column;
* the batch against itself, bitwise: one batch = its columns run alone, across re-gathered groups;
* b = 0 columns, maxit = 1, refusals, the equivalence pipeline and the gateway command on top.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, golden_problem
import hgmres
from hgmres import _lib as L
from hgmres import analysis
from oracle import restatement as R   # checker only
from test_gpu_batch import LAMS, LEVELS, MAXIT, NRHS, noisy_rhs
from test_gpu_parity import TOL, _Rounded, _gkb_check, rel
from tiled_pair import tiled_pair

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FIXTURES = ("tomo24_matched.npz", "tomo24_pixel.npz")
# kind -> (stopping tolerance, oracle, single solver, hybrid).  At these tolerances the oracle's columns
# leave at different iterations (lsqr [6, 6, 6, 7, 12], hybrid_lsqr [6, 6, 7, 12, 12], lsmr [7, 7, 7, 8, 12],
# hybrid_lsmr [6, 6, 6, 12, 12] on both fixtures, each deciding entry at least 2 % from the tolerance);
# _oracle_cols asserts the spread on the oracle's own result.
KINDS = {
    "lsqr": (2.5e-2, R.lsqr_solver, hgmres.lsqr_solver, False),
    "hybrid_lsqr": (2.5e-2, R.hybrid_lsqr_solver, hgmres.hybrid_lsqr_solver, True),
    "lsmr": (2.1e-2, R.lsmr_solver, hgmres.lsmr_solver, False),
    "hybrid_lsmr": (3.0e-2, R.hybrid_lsmr_solver, hgmres.hybrid_lsmr_solver, True),
}
NHIST = {"lsqr": 2, "hybrid_lsqr": 2, "lsmr": 3, "hybrid_lsmr": 2}


def _hists(Rb, kind, j, k=None):
    """Column j of a GKBatchResult as the single solver's tuple (x, histories truncated to niters)."""
    k = int(Rb.niters[j]) if k is None else k
    h = (Rb.error_norm[:k, j], Rb.residual_norm[:k, j]) + ((Rb.ar_norm[:k, j],) if kind == "lsmr" else ())
    return (Rb.x[:, j],) + h


def same_gk(a, b, cols_a=None, cols_b=None, err=True):
    """Two GKBatchResults equal bit for bit (on the given columns)."""
    ca = slice(None) if cols_a is None else cols_a
    cb = slice(None) if cols_b is None else cols_b
    assert np.array_equal(a.niters[ca], b.niters[cb])
    assert np.array_equal(a.x[:, ca], b.x[:, cb], equal_nan=True)
    assert np.array_equal(a.residual_norm[:, ca], b.residual_norm[:, cb], equal_nan=True)
    assert np.array_equal(a.ar_norm[:, ca], b.ar_norm[:, cb], equal_nan=True)
    if err:
        assert np.array_equal(a.error_norm[:, ca], b.error_norm[:, cb], equal_nan=True)


# ---------------------------------------------------------------------------------------------
# 1. the kernel hook
# ---------------------------------------------------------------------------------------------
# gkmv.hip gkmv_grid: min(ceil(n / BS), MAX_PARTS) blocks of BS threads with BS = 256 and MAX_PARTS = 1024
# (internal.h): past 262,144 rows a thread strides over more than one row.
GRID_CAP = 1024 * 256
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 65537)


def _axpby_padded(ctx, a, X, b, Y, pad=3):
    """hgm_mv_axpby_norms on device buffers with leading dimensions padded by `pad`, the padding NaN;
    returns the whole (n + pad) x nvec output buffer and the sums."""
    lib = L.load()
    n, nv = X.shape
    ld = n + pad
    bufs = []
    for src in (X, Y, None):
        Bf = np.full((ld, nv), np.nan, order="F")
        if src is not None:
            Bf[:n, :] = src
        bufs.append(Bf)
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    ss = np.zeros(nv)
    ptr = [C.c_void_p() for _ in range(3)]
    try:
        for p_, Bf in zip(ptr, bufs):
            assert lib.hgm_dev_alloc(ctx.handle, 8 * ld * nv, C.byref(p_)) == L.HGM_OK
            assert lib.hgm_memcpy_h2d(ctx.handle, p_, Bf.ctypes.data_as(C.c_void_p), 8 * ld * nv) == L.HGM_OK
        rc = lib.hgm_mv_axpby_norms(ctx.handle, n, nv, a.ctypes.data_as(L.dp), ptr[0], ld, b.ctypes.data_as(L.dp),
                                    ptr[1], ld, ptr[2], ld, ss.ctypes.data_as(L.dp))
        assert rc == L.HGM_OK, rc
        assert lib.hgm_memcpy_d2h(ctx.handle, bufs[2].ctypes.data_as(C.c_void_p), ptr[2], 8 * ld * nv) == L.HGM_OK
    finally:
        for p_ in ptr:
            if p_.value:
                lib.hgm_dev_free(ctx.handle, p_)
    return bufs[2], ss


def _check_axpby(ctx, n, nv, seed):
    rng = np.random.default_rng(seed)
    X, Y = rng.standard_normal((n, nv)), rng.standard_normal((n, nv))
    a, b = rng.standard_normal(nv), rng.standard_normal(nv)
    a[0] = 1.0                                              # the solver's A*v - alpha*u form
    Out, ss = _axpby_padded(ctx, a, X, b, Y)
    ref = a * X + b * Y                                     # numpy: product, product, sum -- three roundings
    assert np.array_equal(Out[:n], ref), (n, nv)
    assert np.all(np.isnan(Out[n:])), (n, nv)               # nothing written past row n
    s = np.sum(ref * ref, axis=0)
    assert np.all(np.abs(ss - s) <= (n + 1) * EPS * s), (n, nv, np.max(np.abs(ss - s) / s))


@pytest.mark.parametrize("n", LENGTHS)
def test_axpby_norms_matches_numpy(gpu_ctx, n):
    for nv in range(1, 9):
        _check_axpby(gpu_ctx, n, nv, 100 * n + nv)


@pytest.mark.parametrize("nv", [3, 8])
def test_axpby_norms_past_the_grid_stride_cap(gpu_ctx, nv):
    _check_axpby(gpu_ctx, GRID_CAP + 257, nv, nv)


@pytest.mark.parametrize("n", [257, 65537, GRID_CAP + 257])
def test_axpby_norms_invariance(gpu_ctx, n):
    """A column's elements and sum do not depend on the vector count, its slot or its neighbours."""
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal((n, 1)), rng.standard_normal((n, 1))
    a, b = 0.7, -1.3
    o1, s1 = hgmres.mv_axpby_norms([a], x, [b], y, ctx=gpu_ctx)
    o2, s2 = hgmres.mv_axpby_norms([a], x, [b], y, ctx=gpu_ctx)
    assert np.array_equal(o1, o2) and np.array_equal(s1, s2)               # two identical calls
    for nv, slot in ((3, 0), (3, 2), (8, 7)):
        X, Y = rng.standard_normal((n, nv)), rng.standard_normal((n, nv))
        av, bv = rng.standard_normal(nv), rng.standard_normal(nv)
        X[:, [slot]], Y[:, [slot]], av[slot], bv[slot] = x, y, a, b
        if nv == 8:
            X[:, 0] = np.nan                                               # a non-finite neighbour
        O, S = hgmres.mv_axpby_norms(av, X, bv, Y, ctx=gpu_ctx)
        assert np.array_equal(O[:, [slot]], o1), (nv, slot)
        assert S[slot] == s1[0], (nv, slot)


# ---------------------------------------------------------------------------------------------
# 2. the batch against the oracle, column by column
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problems(gpu_ctx):
    out = {}
    for name in FIXTURES:
        A, _, b, xt, _ = golden_problem(name)
        out[name] = dict(A=A, b=b, xt=xt, Bm=noisy_rhs(b, LEVELS), Ao=hgmres.SparseOperator.from_scipy(A, ctx=gpu_ctx))
    return out


def _oracle_fn(kind, b, xt, tol, maxit, lam):
    fn = KINDS[kind][1]
    if KINDS[kind][3]:
        return lambda AA: fn(AA, b, xt, tol, maxit, lam)
    return lambda AA: fn(AA, b, xt, tol, maxit)


_ORACLE_CACHE = {}


def _oracle_cols(problems, name, kind):
    """The oracle's solver once per column, and the check that the stopping tolerance spreads the columns."""
    key = (name, kind)
    if key not in _ORACLE_CACHE:
        P = problems[name]
        _ORACLE_CACHE[key] = [_oracle_fn(kind, P["Bm"][:, j], P["xt"], KINDS[kind][0], MAXIT, LAMS[j])(P["A"])
                              for j in range(NRHS)]
    ref = _ORACLE_CACHE[key]
    nit = [r[-1] for r in ref]
    assert len(set(nit)) >= 2 and min(nit) < MAXIT, nit
    return ref


def _batch(problems, name, kind, ctx, cols=slice(None), **kw):
    P = problems[name]
    lam = LAMS[cols] if KINDS[kind][3] else None
    return hgmres.gk_batch(P["Ao"], P["Bm"][:, cols], kw.pop("xt", P["xt"]), kw.pop("tol", KINDS[kind][0]),
                           kw.pop("maxit", MAXIT), kind, lambdas=lam, ctx=ctx, **kw)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", FIXTURES)
def test_gk_batch_matches_oracle(gpu_ctx, problems, name, kind):
    P = problems[name]
    ref = _oracle_cols(problems, name, kind)
    Rb = _batch(problems, name, kind, gpu_ctx)
    assert [int(k) for k in Rb.niters] == [r[-1] for r in ref], (Rb.niters, [r[-1] for r in ref])
    for j in range(NRHS):
        k = ref[j][-1]
        fn = _oracle_fn(kind, P["Bm"][:, j], P["xt"], KINDS[kind][0], MAXIT, LAMS[j])
        _gkb_check(fn, P["A"], _hists(Rb, kind, j), nhist=NHIST[kind], label=f"gk_batch {kind} {name} col {j}")
        for h in (Rb.error_norm, Rb.residual_norm) + ((Rb.ar_norm,) if kind == "lsmr" else ()):
            assert np.all(np.isnan(h[k:, j])) and np.all(np.isfinite(h[:k, j]))      # NaN past niters
    if kind != "lsmr":
        assert np.all(np.isnan(Rb.ar_norm))


# ---------------------------------------------------------------------------------------------
# 3. against the library's single solvers
# ---------------------------------------------------------------------------------------------
def _envelope(fn, A, nhist, seeds=tuple(range(1, 9)), k=100.0):
    """The Golub-Kahan bar of _gkb_check as numbers: max(1e-10, k x the oracle's own spread under the rounding
    model over 8 seeds), for x and per history entry."""
    ref = fn(A)
    sx, sh = 0.0, [np.zeros(np.size(r_)) for r_ in ref[1:1 + nhist]]
    for seed in seeds:
        p = fn(_Rounded(A, np.random.default_rng(seed)))
        sx = max(sx, rel(p[0], ref[0]))
        for i, (p_, r_) in enumerate(zip(p[1:1 + nhist], ref[1:1 + nhist])):
            with np.errstate(invalid="ignore"):
                d = np.abs(np.asarray(p_) - np.asarray(r_)) / np.maximum(np.abs(r_), 1e-300)
            sh[i] = np.maximum(sh[i], np.nan_to_num(d))
    return max(TOL, k * sx), [np.maximum(TOL, k * s) for s in sh]


def _close_as_the_oracle(out, single, fn, A, nhist, label):
    """`out` lies as close to `single` as either lies to the oracle: the same bar, `single` as the reference."""
    tx, th = _envelope(fn, A, nhist)
    dx = rel(out[0], single[0])
    assert dx <= tx, (label, dx, tx)
    worst = 0.0
    for i in range(nhist):
        a_, r_ = np.asarray(out[1 + i]), np.asarray(single[1 + i])
        assert a_.shape == r_.shape, label
        d = np.abs(a_ - r_) / np.maximum(np.abs(r_), 1e-300)
        assert np.all(d <= th[i]), (label, i, np.max(d / th[i]))
        worst = max(worst, np.max(d, initial=0.0))
    print(f"[gk_batch vs single {label}] x: dev {dx:.2e} tol {tx:.2e}; histories: max dev {worst:.2e}")


@pytest.mark.parametrize("kind,name", [("lsqr", FIXTURES[0]), ("hybrid_lsqr", FIXTURES[1]), ("lsmr", FIXTURES[1]),
                                       ("hybrid_lsmr", FIXTURES[0])])
def test_gk_batch_matches_single_solver(gpu_ctx, problems, kind, name):
    P = problems[name]
    tol, _, single, hybrid = KINDS[kind]
    _oracle_cols(problems, name, kind)                                   # the spread of niters holds
    Rb = _batch(problems, name, kind, gpu_ctx)
    for j in range(NRHS):
        args = (P["Ao"], P["Bm"][:, j], P["xt"], tol, MAXIT) + ((LAMS[j],) if hybrid else ())
        s = single(*args, ctx=gpu_ctx)
        assert Rb.niters[j] == s[-1], (j, Rb.niters[j], s[-1])
        fn = _oracle_fn(kind, P["Bm"][:, j], P["xt"], tol, MAXIT, LAMS[j])
        _close_as_the_oracle(_hists(Rb, kind, j), s, fn, P["A"], NHIST[kind], f"{kind} {name} col {j}")


@pytest.fixture(scope="module")
def tiled(gpu_ctx):
    return tiled_pair(gpu_ctx)


@pytest.mark.parametrize("kind", ["lsqr", "hybrid_lsmr"])
def test_gk_batch_on_tiled_operators(gpu_ctx, tiled, kind):
    """The batch on A in a stored pixel order (At its device transpose) against A in the reference order, b,
    x_true and x in the reference order, at the bar of the batch against the single solver with the
    reference-order run for `single` and the oracle on the reference-order matrix.  Three different x_true
    columns: a permutation into the stored order that reaches the wrong column, or none, is an O(1) error in that
    column's error history.  lsqr updates x in place, hybrid_lsmr forms x = V_k y; then one shared b (ldb = 0)
    with three lambdas for the hybrid kind."""
    P = tiled["P"]
    hybrid = KINDS[kind][3]
    xt = np.asarray(P.x_true, dtype=np.float64).ravel()
    Bm = noisy_rhs(np.asarray(P.b, dtype=np.float64).ravel(), LEVELS[[0, 2, 4]])
    XT = xt[:, None] * np.array([1.0, 0.5, -1.0])[None, :]
    lam = LAMS[:3] if hybrid else None
    maxit = 8
    for rhs in (Bm, Bm[:, 1]) if hybrid else (Bm,):          # one b per column, then one shared
        run = lambda Aop: hgmres.gk_batch(Aop, rhs, XT, 0.0, maxit, kind, lambdas=lam, ctx=gpu_ctx)
        Rt, Rr = run(tiled["At"]), run(tiled["Ar"])
        assert Rt.x.shape == (xt.size, 3)
        assert np.array_equal(Rt.niters, Rr.niters) and np.all(Rt.niters == maxit)
        for j in range(3):
            bj = rhs if rhs.ndim == 1 else rhs[:, j]
            fn = _oracle_fn(kind, bj, XT[:, j], 0.0, maxit, LAMS[j])
            _close_as_the_oracle(_hists(Rt, kind, j), _hists(Rr, kind, j), fn, tiled["A"], NHIST[kind],
                                 f"{kind} tiled {'shared b' if rhs.ndim == 1 else 'columns'} col {j}")


# ---------------------------------------------------------------------------------------------
# 4. composition, bitwise
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lsqr", "hybrid_lsmr"])
def test_gk_batch_equals_its_columns_alone(gpu_ctx, problems, kind):
    name = FIXTURES[1]
    Rb = _batch(problems, name, kind, gpu_ctx)
    assert len(set(Rb.niters)) >= 2 and min(Rb.niters) < MAXIT           # columns left the batch: re-gathered
    for j in range(NRHS):
        same_gk(Rb, _batch(problems, name, kind, gpu_ctx, cols=[j]), [j], [0])


@pytest.mark.parametrize("kind", ["lsmr", "hybrid_lsqr"])
def test_gk_batch_of_two_groups_equals_its_columns_alone(gpu_ctx, problems, kind):
    """11 columns: two groups (8 + 3), re-gathered as columns finish."""
    P = problems[FIXTURES[0]]
    Bm = noisy_rhs(P["b"], np.logspace(-4, -1, 11), seed=11)
    lams = np.logspace(-2, 2, 11) if KINDS[kind][3] else None
    tol = KINDS[kind][0]
    Rb = hgmres.gk_batch(P["Ao"], Bm, P["xt"], tol, MAXIT, kind, lambdas=lams, ctx=gpu_ctx)
    assert len(set(Rb.niters)) >= 2 and min(Rb.niters) < MAXIT, Rb.niters
    for j in range(11):
        R1 = hgmres.gk_batch(P["Ao"], Bm[:, [j]], P["xt"], tol, MAXIT, kind,
                             lambdas=None if lams is None else lams[[j]], ctx=gpu_ctx)
        same_gk(Rb, R1, [j], [0])


@pytest.mark.parametrize("kind", ["hybrid_lsqr", "hybrid_lsmr"])
def test_shared_b_equals_repeated_column(gpu_ctx, problems, kind):
    """One b with five lambdas (the lambda sweep) against the same b repeated as five columns."""
    P = problems[FIXTURES[0]]
    tol = KINDS[kind][0]
    b = P["Bm"][:, 2]
    a = hgmres.gk_batch(P["Ao"], b, P["xt"], tol, MAXIT, kind, lambdas=LAMS, ctx=gpu_ctx)
    r = hgmres.gk_batch(P["Ao"], np.repeat(b[:, None], NRHS, axis=1), P["xt"], tol, MAXIT, kind, lambdas=LAMS, ctx=gpu_ctx)
    assert a.x.shape == (P["A"].shape[1], NRHS)
    same_gk(a, r)


@pytest.mark.parametrize("kind", ["lsqr", "lsmr"])
def test_shared_x_true_equals_repeated_column(gpu_ctx, problems, kind):
    name = FIXTURES[0]
    P = problems[name]
    a = _batch(problems, name, kind, gpu_ctx)
    r = _batch(problems, name, kind, gpu_ctx, xt=np.repeat(P["xt"][:, None], NRHS, axis=1))
    same_gk(a, r)
    # no x_true: the error histories stay NaN, everything else is unchanged
    c = _batch(problems, name, kind, gpu_ctx, xt=None)
    assert np.all(np.isnan(c.error_norm))
    same_gk(a, c, err=False)


# ---------------------------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lsqr", "lsmr"])
def test_zero_rhs_column_between_ordinary_ones(gpu_ctx, problems, kind):
    """b = 0 in the middle column: the single solver's NaN pattern and niters (test_gpu_edge.py's convention);
    the neighbours are bitwise what they are alone."""
    P = problems[FIXTURES[0]]
    tol, _, single, _ = KINDS[kind]
    Bm = np.stack([P["Bm"][:, 0], np.zeros(P["A"].shape[0]), P["Bm"][:, 4]], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Rb = hgmres.gk_batch(P["Ao"], Bm, P["xt"], tol, 4, kind, ctx=gpu_ctx)
        s = single(P["Ao"], Bm[:, 1], P["xt"], tol, 4, ctx=gpu_ctx)
    assert Rb.niters[1] == s[-1] == 4
    for a_, b_ in zip(_hists(Rb, kind, 1), s[:-1]):
        a_, b_ = np.asarray(a_), np.asarray(b_)
        assert a_.shape == b_.shape
        assert np.array_equal(np.isnan(a_), np.isnan(b_)) and np.array_equal(np.isinf(a_), np.isinf(b_))
        assert np.all(np.isnan(a_))                                      # lsqr_solver.m:7-8 / lsmr_solver.m:44-46: 0/0
    for j in (0, 2):
        same_gk(Rb, hgmres.gk_batch(P["Ao"], Bm[:, [j]], P["xt"], tol, 4, kind, ctx=gpu_ctx), [j], [0])
        assert np.all(np.isfinite(Rb.x[:, j]))


@pytest.mark.parametrize("kind", list(KINDS))
def test_gk_batch_maxit_one(gpu_ctx, problems, kind):
    name = FIXTURES[1]
    P = problems[name]
    Rb = _batch(problems, name, kind, gpu_ctx, tol=0.0, maxit=1)
    assert np.all(Rb.niters == 1) and Rb.residual_norm.shape == (1, NRHS)
    for j in range(NRHS):
        fn = _oracle_fn(kind, P["Bm"][:, j], P["xt"], 0.0, 1, LAMS[j])
        ref = _gkb_check(fn, P["A"], _hists(Rb, kind, j), nhist=NHIST[kind], label=f"gk_batch maxit 1 {kind} col {j}")
        assert ref[-1] == 1


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def test_gk_batch_refusals(gpu_ctx, problems):
    P = problems[FIXTURES[0]]
    A, Bm, xt = P["Ao"], P["Bm"], P["xt"]
    At = A.T
    lib = L.load()
    ip = C.POINTER(C.c_int)
    dp = lambda a: a.ctypes.data_as(L.dp) if a is not None else None
    m, n = A.shape
    Bf = np.asfortranarray(Bm)

    def call(ctx, Ah, Ath, nrhs, lam, kind, hybrid, flags=0, Bsrc=Bf, maxit=3):
        o = L.hgm_opts()
        o.flags, o.orth, o.H_out = flags, L.HGM_MGS, None
        nit = np.zeros(max(nrhs, 1), dtype=np.int32)
        return lib.hgm_gk_batch(ctx.handle, C.byref(o), Ah, Ath, dp(Bsrc), m, nrhs, dp(xt), 0, 0.0, maxit, dp(lam), kind,
                                hybrid, None, n, None, None, None, nit.ctypes.data_as(ip))

    A32 = hgmres.as_operator(P["A"], gpu_ctx, dtype=L.HGM_F32)
    for kind in (L.HGM_GK_LSQR, L.HGM_GK_LSMR):
        assert call(gpu_ctx, A32._h, A32.T._h, 2, None, kind, 0) == L.HGM_E_ARG                # fp32 operators
        with gpu_ctx.options(parity=1):
            assert call(gpu_ctx, A._h, At._h, 2, None, kind, 0) == L.HGM_E_ARG                  # parity mode
        assert call(gpu_ctx, A._h, At._h, 2, None, kind, 0, flags=L.HGM_DEVICE_PTRS) == L.HGM_E_ARG
        assert call(gpu_ctx, A._h, At._h, 0, None, kind, 0) == L.HGM_E_ARG                      # nrhs < 1
        big = np.asfortranarray(np.repeat(Bm[:, :1], 65, axis=1))
        assert call(gpu_ctx, A._h, At._h, 65, None, kind, 0, Bsrc=big) == L.HGM_E_ARG           # nrhs > 64
        assert call(gpu_ctx, A._h, At._h, 2, None, kind, 0, maxit=0) == L.HGM_E_ARG             # maxit < 1
        assert call(gpu_ctx, A._h, None, 2, None, kind, 0) == L.HGM_E_ARG                       # At == NULL
        assert call(gpu_ctx, A._h, A._h, 2, None, kind, 0) == L.HGM_E_ARG                       # At of A's shape
        for bad in (-1.0, np.nan, np.inf):
            assert call(gpu_ctx, A._h, At._h, 2, np.array([1.0, bad]), kind, 1) == L.HGM_E_ARG  # bad lambda (hybrid)
            assert call(gpu_ctx, A._h, At._h, 2, np.array([1.0, bad]), kind, 0) == L.HGM_OK     # ignored otherwise
        assert call(gpu_ctx, A._h, At._h, 2, None, kind, 1) == L.HGM_E_ARG                      # hybrid needs lambdas
    assert call(gpu_ctx, A._h, At._h, 2, None, 2, 0) == L.HGM_E_ARG                             # a bad kind
    # a context with a host all-reduce hook at world 2: HGM_E_UNSUPPORTED, and the hook is never called
    calls = []
    c2 = hgmres.Context(0)
    try:
        c2.set_host_allreduce(0, 2, lambda arr: calls.append(arr.size))
        A2 = hgmres.as_operator(P["A"], c2)
        assert call(c2, A2._h, A2.T._h, 2, None, L.HGM_GK_LSQR, 0) == L.HGM_E_UNSUPPORTED
        assert calls == []
    finally:
        c2.close()
    one = np.ones(8)
    assert lib.hgm_mv_axpby_norms(gpu_ctx.handle, 1, 9, dp(one), C.c_void_p(8), 1, dp(one), C.c_void_p(8), 1,
                                  C.c_void_p(8), 1, None) == L.HGM_E_ARG
    # the context still solves after the refusals
    Rb = hgmres.gk_batch(A, Bm[:, :2], xt, 0.0, 3, "lsqr", ctx=gpu_ctx)
    assert np.all(Rb.niters == 3) and np.all(np.isfinite(Rb.x))


# ---------------------------------------------------------------------------------------------
# 7. pipeline
# ---------------------------------------------------------------------------------------------
def _gap(e1, e2):
    e1, e2 = np.asarray(e1), np.asarray(e2)
    return float(np.max(np.abs(e1 - e2) / np.abs(e2)))


def test_equivalence_vs_noise_level(gpu_ctx, problems):
    P = problems[FIXTURES[0]]
    A, xt = P["A"], P["xt"]
    levels = np.logspace(-3, -1, 4)
    lam, maxit = 1e-3, 12
    E = analysis.equivalence_vs_noise_level(P["Ao"], A @ xt, xt, levels, maxit=maxit, tol=0.0, lam=lam, seed=3, ctx=gpu_ctx)
    Bm = E["Bm"]
    assert Bm.shape == (A.shape[0], 4)
    Ao, Bo = P["Ao"], P["Ao"].T
    singles = {
        "ab": lambda b: hgmres.ABgmres_nonhybrid_bounds(Ao, Bo, b, xt, 0.0, maxit, ctx=gpu_ctx),
        "ba": lambda b: hgmres.BAgmres_nonhybrid_bounds(Ao, Bo, b, xt, 0.0, maxit, ctx=gpu_ctx),
        "hab": lambda b: hgmres.ABgmres_hybrid_bounds(Ao, Bo, b, xt, 0.0, maxit, lam, ctx=gpu_ctx),
        "hba": lambda b: hgmres.BAgmres_hybrid_bounds(Ao, Bo, b, xt, 0.0, maxit, lam, ctx=gpu_ctx),
        "lsqr": lambda b: hgmres.lsqr_solver(Ao, b, xt, 0.0, maxit, ctx=gpu_ctx),
        "lsmr": lambda b: hgmres.lsmr_solver(Ao, b, xt, 0.0, maxit, ctx=gpu_ctx),
        "hybrid_lsqr": lambda b: hgmres.hybrid_lsqr_solver(Ao, b, xt, 0.0, maxit, lam, ctx=gpu_ctx),
        "hybrid_lsmr": lambda b: hgmres.hybrid_lsmr_solver(Ao, b, xt, 0.0, maxit, lam, ctx=gpu_ctx),
    }
    oracle = {"ab": lambda AA, b: R.ABgmres_nonhybrid_bounds(AA, AA.T, b, xt, 0.0, maxit),
              "ba": lambda AA, b: R.BAgmres_nonhybrid_bounds(AA, AA.T, b, xt, 0.0, maxit),
              "hab": lambda AA, b: R.ABgmres_hybrid_bounds(AA, AA.T, b, xt, 0.0, maxit, lam),
              "hba": lambda AA, b: R.BAgmres_hybrid_bounds(AA, AA.T, b, xt, 0.0, maxit, lam),
              "lsqr": lambda AA, b: R.lsqr_solver(AA, b, xt, 0.0, maxit),
              "lsmr": lambda AA, b: R.lsmr_solver(AA, b, xt, 0.0, maxit),
              "hybrid_lsqr": lambda AA, b: R.hybrid_lsqr_solver(AA, b, xt, 0.0, maxit, lam),
              "hybrid_lsmr": lambda AA, b: R.hybrid_lsmr_solver(AA, b, xt, 0.0, maxit, lam)}
    for key, fn in singles.items():
        assert E[f"final_errors_{key}"].shape == (4,) and np.all(E[f"niters_{key}"] == maxit)
        for i in range(4):
            fin = fn(Bm[:, i])[1][-1]
            # bar 3 on the final error: the Golub-Kahan bar for the Golub-Kahan curves, 1e-10 for the GMRES ones
            tol = TOL
            if key in KINDS:
                _, th = _envelope(lambda AA, b=Bm[:, i], key=key: oracle[key](AA, b), A, 1)
                tol = th[0][-1]
            d = abs(E[f"final_errors_{key}"][i] - fin) / fin
            assert d <= tol, (key, i, d, tol)
    # AB-GMRES == LSQR and BA-GMRES == LSMR (run_equivalence_plots.m:12-22): the largest relative gap between
    # the two error histories, held to 100 x the gap of the oracle's own solver pair on the same data
    for pair, k1, k2 in (("ab_lsqr", "ab", "lsqr"), ("ba_lsmr", "ba", "lsmr")):
        og = max(_gap(oracle[k1](A, Bm[:, i])[1], oracle[k2](A, Bm[:, i])[1]) for i in range(4))
        print(f"[equivalence {pair}] device gap {E['gap_' + pair]:.2e}, oracle gap {og:.2e}")
        assert E["gap_" + pair] <= 100 * og, (pair, E["gap_" + pair], og)


# ---------------------------------------------------------------------------------------------
# 8. gateway
# ---------------------------------------------------------------------------------------------
def test_matlab_command_equals_python_call(gpu_ctx, problems):
    """matlab/gk_batch.m through the gateway (the mx API stand-in) against the Python binding."""
    from mwrap import Function
    from test_mex_gateway import Mex
    P = problems[FIXTURES[1]]
    A = sp.csr_matrix(P["A"])
    A.sort_indices()
    f = Function(os.path.join(ROOT, "matlab", "gk_batch.m"), Mex())
    for kind in ("lsqr", "hybrid_lsmr"):
        tol, _, _, hybrid = KINDS[kind]
        lam = LAMS if hybrid else None
        Rb = hgmres.gk_batch(A, P["Bm"], P["xt"], tol, MAXIT, kind, lambdas=lam, ctx=gpu_ctx)
        args = (sp.csc_matrix(A), P["Bm"], P["xt"], tol, float(MAXIT), kind)
        X, e, r, ar, ni = f(5, *(args + ((lam,) if lam is not None else ())))
        assert X.shape == Rb.x.shape and e.shape == r.shape == ar.shape == (MAXIT, NRHS)
        assert np.array_equal(ni.reshape(-1).astype(int), Rb.niters)
        assert np.array_equal(X, Rb.x)
        assert np.array_equal(e, Rb.error_norm, equal_nan=True) and np.array_equal(r, Rb.residual_norm, equal_nan=True)
        assert np.array_equal(ar, Rb.ar_norm, equal_nan=True)
