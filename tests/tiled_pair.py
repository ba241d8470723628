"""One operator pair in a non-trivial stored pixel order next to the same pair in the reference order, for the
tests of the lockstep solves and the multi-vector products on tiled operators (test_gpu_gauss.py,
test_gpu_batch.py, test_gpu_gkbatch.py)."""
import scipy.sparse as sp

import hgmres
from hgmres.problems import tomo_problem


def tiled_pair(ctx):
    """A 32^2 / 16-angle pair stored in 4 x 4 tiles and 16 x 16 super-blocks (as test_gpu_mismatch.py's
    test_spmm_pert_tiled_pair builds its pair) and the same pair in the reference order.  ``At`` / ``Bt``: the
    tiled operators; ``Ar`` / ``Br``: the reference-order ones; ``A`` / ``B``: the scipy matrices; ``P``: the
    problem."""
    P = tomo_problem(32, 16, noise=1e-2, seed=0, backprojector="pixel")
    A, B = sp.csr_matrix(P.A), sp.csr_matrix(P.B)
    A.sort_indices()
    B.sort_indices()
    At = hgmres.SparseOperator.from_scipy_tiled(A, 32, 4, 16, ctx=ctx)
    Bt = hgmres.SparseOperator.from_scipy_tiled(sp.csr_matrix(B.T), 32, 4, 16, ctx=ctx).T
    assert At.pixel_order("cols")[1:] == (4, 16) and Bt.pixel_order("rows")[1:] == (4, 16)
    up = lambda M: hgmres.SparseOperator.from_scipy(M, ctx=ctx)
    return dict(P=P, A=A, B=B, At=At, Bt=Bt, Ar=up(A), Br=up(B))
