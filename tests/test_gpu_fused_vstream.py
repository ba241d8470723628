"""The compact value stream of the one-pass A*(B*q) (HGM_OPT_FUSED_VSTREAM, csrc/fused.hip
k_fused_rw RP 5): the operator's most frequent value bit patterns become codes in
the free bits of the entries' slot words and only the other values are stored.

  * the decode is exact: with q = e_i every row sum has at most one non-zero term, so both outputs
    are bitwise the plain pass's (option 0);
  * a general q only permutes the operands of each row sum: within the row-pair tests' 1e-14 of
    the plain pass, bitwise equal across runs and across plan builds, host- and device-built plans
    with equal checksums;
  * solves against the two-pass path and the oracle at the fused tests' 1e-10;
  * edges, each asserting the path taken: all values equal (100 % coded, no value stream), values
    with a random perturbation (no repeated pattern: the plain plan, the bits of option 0), one row
    of each pair coded and the other stored, a pixel shard, a geometry whose plan is refused.

Option values: 0 plain, 1 compact when the entry bytes shrink enough, 3 compact whenever the
plan's shape allows it (the small geometries here repeat their patterns less than C4 does).

64^2 at 90 angles cannot take the compact stream: its pixel rows hold ~115 entries, no two fit one
128-entry chunk, so its plan is not a row-pair plan (the shape the compact kernel exists for).  Its
cases stay as the fall-back they are: the path is asserted to be the plain one, the numbers to be
those of option 0 (decode) and of the two-pass path and the oracle (solves).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres.core import stored_pixel_index
from hgmres.problems import shepp_logan
from oracle import restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-10          # solves: the bar of tests/test_gpu_fused.py
PROD = 1e-14         # products against the plain pass: the bar of the row-pair tests


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def hist_dev(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def _unit(m, i):
    q = np.zeros(m)
    q[i] = 1.0
    return q


def _corner_ray(As, N, R=32):
    """A ray through the two pixels diagonally across the corner (R, R) of the region grid."""
    Ac = As.tocsc()
    p0, p1 = (R - 1) + (R - 1) * N, R + R * N
    both = np.intersect1d(Ac.indices[Ac.indptr[p0]:Ac.indptr[p0 + 1]], Ac.indices[Ac.indptr[p1]:Ac.indptr[p1 + 1]])
    assert both.size, "no ray crosses the region corner"
    return int(both[0])


def _bitwise_on_unit_vectors(ctx, A, B, rays, compact=True):
    for i in rays:
        q = _unit(A.shape[0], i)
        with ctx.options(fused_ab=1, fused_vstream=0):
            bq0, ab0 = hgmres.spmv_ab(A, B, q)
        with ctx.options(fused_ab=1, fused_vstream=3):
            assert hgmres.fused_plan_info(A, B)["vstream"] == compact
            bq1, ab1 = hgmres.spmv_ab(A, B, q)
        assert np.array_equal(bq1, bq0) and np.array_equal(ab1, ab0), i
        assert np.any(bq0 != 0.0)


@pytest.mark.parametrize("N,na,compact", [(64, 90, False), (100, 17, True)])
def test_vstream_decode_is_exact(gpu_ctx, N, na, compact):
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    As = A.to_scipy()
    hit = np.flatnonzero(np.diff(As.indptr) > 0)         # rays that cross the image
    rays = [int(hit[0]), int(hit[-1]), _corner_ray(As, N), int(hit[len(hit) // 3]), int(hit[len(hit) // 2])]
    with gpu_ctx.options(fused_ab=1, fused_vstream=3):
        info = hgmres.fused_plan_info(A, B)
    print(f"[vstream decode N={N} angles={na}] coverage {info['vstream_coverage']:.3f}, rays {rays}")
    assert info["vstream"] == compact and (info["vstream_coverage"] > 0.0) == compact
    _bitwise_on_unit_vectors(gpu_ctx, A, B, rays, compact)
    A.close()
    B.close()


def test_vstream_general_q(gpu_ctx):
    N, na = 256, 47
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    q = np.random.default_rng(7).standard_normal(A.shape[0])
    with gpu_ctx.options(fused_ab=1, fused_vstream=0):
        i0 = hgmres.fused_plan_info(A, B)
        bq0, ab0 = hgmres.spmv_ab(A, B, q)
    assert not i0["vstream"] and i0["vstream_value_bytes"] == 0
    runs, infos = [], []
    for build in range(2):                               # (the option change drops the plan: two builds)
        with gpu_ctx.options(fused_ab=1, fused_vstream=3):
            infos.append(hgmres.fused_plan_info(A, B))
            runs.append(hgmres.spmv_ab(A, B, q))
            runs.append(hgmres.spmv_ab(A, B, q))
        with gpu_ctx.options(fused_ab=1, fused_vstream=0):
            hgmres.fused_plan_info(A, B)
    info = infos[0]
    print(f"[vstream general N={N} angles={na}] coverage {info['vstream_coverage']:.4f}, value bytes "
          f"{info['vstream_value_bytes']} ({info['vstream_value_bytes'] / A.nnz:.3f} B/nnz), plan bytes "
          f"{info['plan_bytes']} (plain {i0['plan_bytes']}); A(Bq) vs plain {rel(runs[0][1], ab0):.1e}, "
          f"Bq {rel(runs[0][0], bq0):.1e}")
    assert info["vstream"] and infos[1]["vstream"]
    # the full-chord lengths of 47 angles: about 28 % of the entries carry one of the 31 codes, and
    # a stored value costs 8 B plus the pair padding of its unit
    assert 0.2 < info["vstream_coverage"] < 0.4
    assert info["vstream_value_bytes"] < 8 * A.nnz * (1.0 - info["vstream_coverage"]) * 1.05
    assert info["plan_bytes"] > i0["plan_bytes"]
    assert rel(runs[0][0], bq0) <= PROD and rel(runs[0][1], ab0) <= PROD
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
    assert infos[0]["checksum"] == infos[1]["checksum"] != i0["checksum"]
    ck = {}
    for dev in (0, 1):
        with gpu_ctx.options(fused_ab=1, fused_vstream=3, fused_plan_dev=dev):
            pi = hgmres.fused_plan_info(A, B)
            assert pi["vstream"] and pi["device_built"] == bool(dev)
            ck[dev] = pi["checksum"]
            o = hgmres.spmv_ab(A, B, q)
            assert np.array_equal(o[0], runs[0][0]) and np.array_equal(o[1], runs[0][1])
    assert ck[0] == ck[1] == infos[0]["checksum"]
    with gpu_ctx.options(fused_ab=1, fused_vstream=1):
        auto = hgmres.fused_plan_info(A, B)
    print(f"[vstream general] option 1 takes the compact stream here: {auto['vstream']}")
    A.close()
    B.close()


@pytest.mark.parametrize("N,na,compact", [(64, 90, False), (256, 47, True)])
def test_vstream_solves_match_two_pass_and_oracle(gpu_ctx, N, na, compact):
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    xt = shepp_logan(N).ravel(order="F")
    b0 = A @ xt
    e = np.random.default_rng(0).standard_normal(A.shape[0])
    b = b0 + e / np.linalg.norm(e) * 1e-2 * np.linalg.norm(b0)
    k = 20
    with gpu_ctx.options(fused_ab=0):
        ref = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=gpu_ctx, return_H=True)
        refh = hgmres.ABgmres_hybrid_bounds(A, B, b, xt, 0.0, k, 1e-2, ctx=gpu_ctx, return_H=True)
    with gpu_ctx.options(fused_ab=1, fused_vstream=3):
        assert hgmres.fused_plan_info(A, B)["vstream"] == compact
        out = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=gpu_ctx, return_H=True)
        again = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=gpu_ctx, return_H=True)
        outh = hgmres.ABgmres_hybrid_bounds(A, B, b, xt, 0.0, k, 1e-2, ctx=gpu_ctx, return_H=True)
    for a_, b_ in zip(out, again):
        assert np.array_equal(np.asarray(a_), np.asarray(b_))
    As = A.to_scipy()
    Bs = As.T.tocsr()
    orc = R.ABgmres_nonhybrid_bounds(As, Bs, b, xt, 0.0, k, return_H=True)
    orch = R.ABgmres_hybrid_bounds(As, Bs, b, xt, 0.0, k, 1e-2, return_H=True)
    for name, got, two, ora in (("nonhybrid", out, ref, orc), ("hybrid", outh, refh, orch)):
        for what, r_ in (("two-pass", two), ("oracle", ora)):
            dH = float(np.max(np.abs(got[-1] - r_[-1])) / np.max(np.abs(r_[-1])))
            dx, de, dr = rel(got[0], r_[0]), hist_dev(got[1], r_[1]), hist_dev(got[2], r_[2])
            print(f"[vstream solve N={N} angles={na} {name} vs {what}] |dH| {dH:.1e} x {dx:.1e} err {de:.1e} res {dr:.1e}")
            assert got[3] == r_[3] == k
            assert dH <= TOL and dx <= TOL and de <= TOL and dr <= TOL
    A.close()
    B.close()


def _tiled_pair(ctx, N, na, values):
    """The Siddon pattern at (N, na) with values(data, stored column of each entry), as a tiled
    ray-major operator and its device transpose."""
    from hgmres.problems import siddon_projector
    S = sp.csr_matrix(siddon_projector(N, na))
    tile = hgmres.core.auto_pixel_order(N)[0]
    S.data = values(S.data.copy(), stored_pixel_index(N, tile)[S.indices])
    A = hgmres.SparseOperator.from_scipy_tiled(S, N, tile, ctx=ctx)
    return A, A.T, S


def _some_rays(S):
    hit = np.flatnonzero(np.diff(S.indptr) > 0)
    return [int(hit[0]), int(hit[len(hit) // 2]), int(hit[-1])]


def _check_against_plain(ctx, A, B, S, mode, want_on):
    q = np.random.default_rng(3).standard_normal(A.shape[0])
    with ctx.options(fused_ab=1, fused_vstream=0):
        hgmres.fused_plan_info(A, B)                     # the one pass is taken
        bq0, ab0 = hgmres.spmv_ab(A, B, q)
    with ctx.options(fused_ab=1, fused_vstream=mode):
        info = hgmres.fused_plan_info(A, B)
        bq1, ab1 = hgmres.spmv_ab(A, B, q)
    assert info["vstream"] == want_on
    ref = S.T @ q
    assert rel(bq0, ref) <= 1e-13                        # (the pair is the matrix that was handed over)
    return info, (bq0, ab0), (bq1, ab1)


def test_vstream_all_values_equal(gpu_ctx):
    A, B, S = _tiled_pair(gpu_ctx, 64, 30, lambda d, col: np.full_like(d, 0.75))
    info, plain, comp = _check_against_plain(gpu_ctx, A, B, S, 1, True)
    assert info["vstream_coverage"] == 1.0 and info["vstream_value_bytes"] == 0
    assert rel(comp[0], plain[0]) <= PROD and rel(comp[1], plain[1]) <= PROD
    _bitwise_on_unit_vectors(gpu_ctx, A, B, _some_rays(S))
    A.close()
    B.close()


def test_vstream_perturbed_values_keep_the_plain_plan(gpu_ctx):
    rng = np.random.default_rng(5)
    A, B, S = _tiled_pair(gpu_ctx, 64, 30, lambda d, col: d * (1.0 + 1e-3 * rng.random(d.size)))
    info, plain, comp = _check_against_plain(gpu_ctx, A, B, S, 1, False)
    assert info["vstream_coverage"] == 0.0 and info["vstream_value_bytes"] == 0
    assert np.array_equal(comp[0], plain[0]) and np.array_equal(comp[1], plain[1])
    A.close()
    B.close()


def test_vstream_one_row_coded_the_other_stored(gpu_ctx):
    rng = np.random.default_rng(6)
    # even stored pixels (B's rows): one repeated value; odd ones: values seen once
    A, B, S = _tiled_pair(gpu_ctx, 64, 30, lambda d, col: np.where(col % 2 == 0, 0.5, 0.25 + rng.random(d.size)))
    info, plain, comp = _check_against_plain(gpu_ctx, A, B, S, 1, True)
    even = float(np.mean(S.data == 0.5))
    print(f"[vstream row parity] coverage {info['vstream_coverage']:.4f} (entries of even pixels {even:.4f})")
    assert info["vstream_coverage"] == pytest.approx(even, abs=1e-12)
    assert rel(comp[0], plain[0]) <= PROD and rel(comp[1], plain[1]) <= PROD
    _bitwise_on_unit_vectors(gpu_ctx, A, B, _some_rays(S))
    A.close()
    B.close()


def test_vstream_pixel_shard(gpu_ctx):
    from hgmres.dist import tile_column_shards
    N, na = 256, 47
    A0 = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    Nn, tile, sup = A0.pixel_order("cols")
    lo, hi = tile_column_shards(N, 4, tile)[1]
    B = A0.T.row_slice(lo, hi)
    A = B.T
    q = np.random.default_rng(8).standard_normal(A.shape[0])
    with gpu_ctx.options(fused_ab=1, fused_vstream=0):
        hgmres.fused_plan_info(A, B)
        bq0, ab0 = hgmres.spmv_ab(A, B, q)
    with gpu_ctx.options(fused_ab=1, fused_vstream=3):
        info = hgmres.fused_plan_info(A, B)
        bq1, ab1 = hgmres.spmv_ab(A, B, q)
        bq2, ab2 = hgmres.spmv_ab(A, B, q)
    print(f"[vstream shard rows {lo}:{hi}] coverage {info['vstream_coverage']:.4f}, A(Bq) vs plain {rel(ab1, ab0):.1e}")
    assert info["vstream"] and 0.2 < info["vstream_coverage"] < 0.4
    assert rel(bq1, bq0) <= PROD and rel(ab1, ab0) <= PROD
    assert np.array_equal(bq1, bq2) and np.array_equal(ab1, ab2)
    _bitwise_on_unit_vectors(gpu_ctx, A, B, [int(np.argmax(np.abs(ab0)))])
    for M in (A, B, A0):
        M.close()


def test_vstream_refused_plan_falls_back(gpu_ctx):
    """70 x 70 regions at 47 angles (and the 35 x 35 retry) hold more rays than the largest LDS
    shape of the default library: no plan, the two-pass product, whatever the value-stream option."""
    A = hgmres.SparseOperator.siddon(256, 47, ctx=gpu_ctx)
    B = A.T
    q = np.random.default_rng(9).standard_normal(A.shape[0])
    with gpu_ctx.options(fused_ab=0):
        ref = hgmres.spmv_ab(A, B, q)
    with gpu_ctx.options(fused_ab=1, fused_kind=1, fused_wregion=70, fused_vstream=3):
        with pytest.raises((ValueError, hgmres.HgmError)):
            hgmres.fused_plan_info(A, B)
        out = hgmres.spmv_ab(A, B, q)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    A.close()
    B.close()
