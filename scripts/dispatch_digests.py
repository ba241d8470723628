#!/usr/bin/env python3
"""sha256 of every output of a fixed walk over the kernel-dispatch surface: label, dtype, shape, digest.

Run once per library (HGM_LIB=/path/to/libhgmres.so selects one) and compare the two files: every
(variant, lanes) pair of the SpMV ladders, banded / column-strip / dual-strip operators, the
multi-vector products at every width, the Golub-Kahan vector kernels and both MGS ladders, each
through a product and short solves (their epilogues: ADD / SUB / RSUB / DIVH / ADDQ).

    python scripts/dispatch_digests.py > digests.txt

--brief prints one line per group of calls (one operator setting, one vector count, ...) instead of one per
output array: the group, the number of lines and the sha256 of those lines (what profiles/ keeps).
"""
import hashlib
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hybrid-gmres_amd"), os.path.join(ROOT, "tests")]

import hgmres  # noqa: E402
from conftest import golden_problem  # noqa: E402

ROW_GROUPS = (64, 32, 16, 8, 4)
STREAM_GROUPS = (64, 32, 16, 8, 2, 4)
# tests/test_gpu_parity.py's tune() pairs, then every lane count of every list with every load form
PAIRS = [(8, 8), (8, 16), (10, 32), (8, 64), (9, 4), (14, 4), (30, 4)] + \
        [(v, g) for g in (4, 8, 32) for v in (10, 26)] + \
        [(v, g) for v in (0, 1, 2, 3, 7) for g in ROW_GROUPS] + [(v, g) for v in (8, 11, 26) for g in STREAM_GROUPS]


BRIEF = "--brief" in sys.argv[1:]


_group = [None, []]   # --brief: the open group and its lines


def group(name):
    """close the open group (--brief: print its one line) and open `name`"""
    if BRIEF and _group[1]:
        print(f"{_group[0]}: {len(_group[1])} lines {hashlib.sha256(chr(10).join(_group[1]).encode()).hexdigest()}",
              flush=True)
    _group[:] = [name, []]


def out(line):
    if BRIEF:
        _group[1].append(line)
    else:
        print(line, flush=True)


def emit(label, *arrays):
    for i, a in enumerate(arrays):
        a = np.ascontiguousarray(np.asarray(a))
        out(f"{label}[{i}] {a.dtype} {a.shape} {hashlib.sha256(a.tobytes()).hexdigest()}")


def attempt(label, fn):
    """fn()'s arrays, or the refusal's type when the library refuses the call (the same on both sides)"""
    try:
        emit(label, *fn())
    except (hgmres.HgmError, ValueError) as e:
        out(f"{label} refused: {type(e).__name__}")


def ragged():
    rng = np.random.default_rng(20261021)
    n = 8192
    rows = []
    for length in rng.integers(200, 3001, 64):
        cols = np.sort(rng.choice(n, size=int(length), replace=False))
        rows.append(sp.csr_matrix((rng.standard_normal(cols.size), (np.zeros(cols.size, int), cols)), shape=(1, n)))
    return sp.vstack(rows).tocsr()


def walk(ctx, tag, A, B, b, xt, dtype, pairs, bands=()):
    """product and short solves of (A, B) for every (variant, lanes) pair and every band setting"""
    Ao = hgmres.SparseOperator.from_scipy(A, ctx, dtype=dtype)
    Bo = hgmres.SparseOperator.from_scipy(B, ctx, dtype=dtype)
    rng = np.random.default_rng(1)
    xa, xb = rng.standard_normal(A.shape[1]), rng.standard_normal(B.shape[1])

    def outputs(label):
        group(label)
        attempt(f"{label} A@x", lambda: [Ao @ xa])
        attempt(f"{label} B@x", lambda: [Bo @ xb])
        if dtype == 0:   # the GMRES solvers take fp64 operators only
            attempt(f"{label} hybrid_ab", lambda: [np.asarray(o) for o in hgmres.hybrid_ab_gmres_rtp(
                Ao, Bo, b, xt, 0.0, 6, 1e-2, ctx=ctx, return_H=True)])
        attempt(f"{label} lsqr", lambda: [np.asarray(o) for o in hgmres.lsqr_solver(Ao, b, xt, 0.0, 4, ctx=ctx, At=Bo)])

    for v, g in pairs:
        Ao.tune(v, g)
        Bo.tune(v, g)
        outputs(f"{tag} f{64 >> dtype} tune({v},{g})")
    Bo.tune(0, 0)
    for width, g, v in bands:
        label = f"{tag} f{64 >> dtype} bands({width},{g}) tune({v})"
        try:
            Ao.set_bands(width, g)
            Ao.tune(v, 0)
        except hgmres.HgmError as e:
            group(label)
            out(f"{label} refused: {type(e).__name__}")
            continue
        outputs(label)


def main():
    ctx = hgmres.default_context()
    At, Bt, bt, xtt, _ = golden_problem("tomo24_pixel.npz")
    R = ragged()
    rng = np.random.default_rng(2)
    br, xtr = rng.standard_normal(64), rng.standard_normal(8192)
    band_sets = [(100, g, v) for g in ROW_GROUPS for v in (0, 3)] + [(100, 0, v | 8) for v in (0, 2, 18)]
    for dtype in (0, 1):
        walk(ctx, "tomo24", At, Bt, bt, xtt, dtype, PAIRS, band_sets)
        walk(ctx, "ragged", R, R.T.tocsr(), br, xtr, dtype, PAIRS,
             [(1700, g, v) for g in ROW_GROUPS for v in (0, 1)] + [(1700, 0, 8), (1700, 0, 26)])

    # column and dual strips of a tiled ray-major operator (the streaming kernel over (band, row) segments)
    for dtype in (0, 1):
        N = 128
        S = hgmres.SparseOperator.siddon(N, 30, ctx=ctx, dtype=dtype)
        x = np.random.default_rng(5).standard_normal(N * N)
        for dual in (0, 1):
            group(f"siddon{N} f{64 >> dtype} dual={dual}")
            with ctx.options(band_dual=dual):
                S.set_bands(32 * N, 0)
            for v, g in ((14, 4), (30, 4), (8, 2), (10, 16), (0, 0), (3, 0)):
                S.tune(v, g)
                attempt(f"siddon{N} f{64 >> dtype} dual={dual} tune({v},{g})", lambda: [S @ x])
        if dtype == 0:
            bs = S.to_scipy() @ np.random.default_rng(6).random(N * N)
            S.tune(14, 4)
            attempt(f"siddon{N} dual strips hybrid_ab", lambda: [np.asarray(o) for o in hgmres.hybrid_ab_gmres_rtp(
                S, S.T, bs, np.ones(N * N), 0.0, 6, 1e-2, ctx=ctx, return_H=True)])

    # multi-vector products: every width, every lane count
    Bo = hgmres.SparseOperator.from_scipy(Bt, ctx)
    E_same = hgmres.SparseOperator.from_scipy(sp.csr_matrix((np.cos(np.arange(Bt.nnz)), Bt.indices, Bt.indptr),
                                                            shape=Bt.shape), ctx)
    E_own = hgmres.SparseOperator.from_scipy(sp.random(*Bt.shape, density=0.03, random_state=4, format="csr"), ctx)
    Ro = hgmres.SparseOperator.from_scipy(R, ctx)
    G = hgmres.GaussianPerturbation(Bt.shape[0], Bt.shape[1], seed=9, ctx=ctx)
    for nv in (1, 2, 3, 5, 8):
        group(f"multi-vector products nv={nv}")
        X = np.random.default_rng(nv).standard_normal((Bt.shape[1], nv))
        XR = np.random.default_rng(nv).standard_normal((8192, nv))
        cf = np.linspace(-0.5, 1.0, nv)
        for g in ROW_GROUPS:
            Bo.tune(0, g)
            Ro.tune(0, g)
            emit(f"spmm tomo24 B nv={nv} g={g}", hgmres.spmm(Bo, X))
            emit(f"spmm ragged nv={nv} g={g}", hgmres.spmm(Ro, XR))
            emit(f"spmm_pert shared nv={nv} g={g}", hgmres.spmm_pert(Bo, E_same, cf, X))
            emit(f"spmm_pert own nv={nv} g={g}", hgmres.spmm_pert(Bo, E_own, cf, X))
        emit(f"gauss matmat nv={nv}", G.matmat(X))
        emit(f"gauss matmat coefs nv={nv}", G.matmat(X, cf))
        emit(f"spmm_pert gauss nv={nv}", hgmres.spmm_pert(Bo, G, cf, X))
        Y = np.random.default_rng(nv + 20).standard_normal((8192, nv))
        emit(f"mv_axpby_norms nv={nv}", *hgmres.mv_axpby_norms(cf + 2.0, XR, cf - 3.0, Y, ctx=ctx))

    # Golub-Kahan vector kernels: 5 lockstep columns of each kind
    group("gk_batch")
    Ao = hgmres.SparseOperator.from_scipy(At, ctx)
    Bo.tune(0, 0)
    Bm = np.random.default_rng(7).standard_normal((At.shape[0], 5))
    lams = np.array([0.0, 1e-3, 1e-2, 1e-1, 1.0])
    for kind in ("lsqr", "lsmr", "hybrid_lsqr", "hybrid_lsmr"):
        r = hgmres.gk_batch(Ao, Bm, xtt, 0.0, 6, kind, lambdas=lams if kind.startswith("hybrid") else None, At=Bo,
                            ctx=ctx)
        emit(f"gk_batch {kind}", r.x, r.error_norm, r.residual_norm, r.ar_norm, r.niters)

    # MGS ladders: the one-workgroup sweep at two widths (576 and 8,192 rows), the tile widths of the
    # one-reduction form on short and long vectors
    RT = R.T.tocsr()

    def solves(label):
        group(label)
        attempt(f"{label} tomo24 hybrid_ba", lambda: [np.asarray(o) for o in hgmres.hybrid_ba_gmres_rtp(
            At, Bt, bt, xtt, 0.0, 8, 1e-2, ctx=ctx, return_H=True)])
        attempt(f"{label} ragged hybrid_ba", lambda: [np.asarray(o) for o in hgmres.hybrid_ba_gmres_rtp(
            R, RT, br, xtr, 0.0, 8, 1e-2, ctx=ctx, return_H=True)])

    with ctx.options(mgs_single=1):
        solves("mgs_single")
    for ppl in (1, 2, 4):
        with ctx.options(mgs_single=0, mgs1_ppl=ppl):
            solves(f"mgs1_ppl={ppl}")
            S = hgmres.SparseOperator.siddon(128, 30, ctx=ctx)
            bs = S.to_scipy() @ np.random.default_rng(6).random(128 * 128)
            for fn in (hgmres.hybrid_ab_gmres_rtp, hgmres.hybrid_ba_gmres_rtp):
                attempt(f"mgs1_ppl={ppl} siddon128 {fn.__name__}", lambda: [np.asarray(o) for o in fn(
                    S, S.T, bs, np.ones(128 * 128), 0.0, 8, 1e-2, ctx=ctx, return_H=True)])
    group(None)


if __name__ == "__main__":
    main()
