"""Every arm of the lane-count ladders reaches a kernel of its own (csrc/dispatch.h, the lists of
csrc/internal.h).  Two lane counts sum a row in different orders, so on rows of 200-3,000 entries
their products differ in rounding; if two arms ever launched the same instantiation (group 16
running the 32-lane kernel, say) every accuracy test would still pass and only this one would see it."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres

pytestmark = pytest.mark.gpu

ROW_GROUPS = (64, 32, 16, 8, 4)
STREAM_GROUPS = (64, 32, 16, 8, 2, 4)


@pytest.fixture(scope="module")
def ragged():
    """64 x 8,192 fp64 CSR, row lengths 200-3,000, with 3 vectors and their scipy products"""
    rng = np.random.default_rng(20261021)
    n = 8192
    rows = []
    for length in rng.integers(200, 3001, 64):
        cols = np.sort(rng.choice(n, size=int(length), replace=False))
        rows.append(sp.csr_matrix((rng.standard_normal(cols.size), (np.zeros(cols.size, int), cols)), shape=(1, n)))
    M = sp.vstack(rows).tocsr()
    X = rng.standard_normal((n, 3))
    return M, X, M @ X, np.abs(M) @ np.abs(X) + 1e-300


def _check_ladder(products, ref, scale):
    """products: {lanes: (first, second)} of one ladder"""
    for g, (y, again) in products.items():
        assert np.array_equal(y, again), g
        dev = np.max(np.abs(y - ref) / scale)
        print(f"lanes {g}: scaled deviation {dev:.2e}")
        assert dev < 1e-14, (g, dev)
    for g, h in itertools.combinations(products, 2):
        assert not np.array_equal(products[g][0], products[h][0]), (g, h)


@pytest.mark.parametrize("variant,groups", [(0, ROW_GROUPS), (1, ROW_GROUPS), (8, STREAM_GROUPS)])
def test_spmv_lane_counts_reach_their_own_kernels(gpu_ctx, ragged, variant, groups):
    M, X, ref, scale = ragged
    Mo = hgmres.SparseOperator.from_scipy(M, gpu_ctx)
    products = {}
    for g in groups:
        Mo.tune(variant, g)
        products[g] = (Mo @ X[:, 0], Mo @ X[:, 0])
    _check_ladder(products, ref[:, 0], scale[:, 0])


def test_spmm_lane_counts_reach_their_own_kernels(gpu_ctx, ragged):
    M, X, ref, scale = ragged
    Mo = hgmres.SparseOperator.from_scipy(M, gpu_ctx)
    products = {}
    for g in ROW_GROUPS:
        Mo.tune(0, g)
        products[g] = (hgmres.spmm(Mo, X), hgmres.spmm(Mo, X))
    _check_ladder(products, ref, scale)
