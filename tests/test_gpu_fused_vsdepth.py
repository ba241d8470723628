"""The load ring of the compact one-pass A*(B*q) as its own knob (HGM_OPT_FUSED_VSDEPTH = 38,
csrc/fused.hip k_fused_rw RP 5).

The depth only changes how many batches of entries a wave has in flight: every sum is formed from
the same operands in the same order, so every output is bit for bit the same at every depth.

  * 256^2 / 47 angles, general q: spmv_ab and a 6-step AB-GMRES solve (which adds the side dot)
    array_equal between depth 2 and every depth the library carries, and on a repeat;
  * 36^2 and 40^2 at 30 angles (4 x 4 tiles, 32 x 32 regions): the corner region of 36^2 has 16 pixel
    rows, so its four waves get zero or one partial batch, fewer than any ring holds; the edge
    regions of 40^2 give 8-batch waves.  Equal to depth 2, within the row-pair bar of the plain pass;
  * the rows of shard 1 of a 4-way cut of 256^2 / 47;
  * the option itself: 5 is refused, a depth the default library does not carry is refused with the
    experiments-build message, and the Python name agrees with the header.
"""
import os
import re

import numpy as np
import pytest

import hgmres
from hgmres import _lib as L
from hgmres.problems import shepp_logan

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD = 1e-14         # products against the plain pass: the bar of the row-pair tests


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def _experiments():
    return bool(L.load().hgm_experiments())


def _carried(ctx):
    """The depths this library has kernels for: the default library refuses the others."""
    out = []
    prev = ctx.get_option("fused_vsdepth")
    for d in (2, 3, 4):
        try:
            ctx.set_option("fused_vsdepth", d)
            out.append(d)
        except (ValueError, hgmres.HgmError):
            pass
    ctx.set_option("fused_vsdepth", prev)
    assert 2 in out and int(prev) in out and (len(out) == 3 or not _experiments())
    return out


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and len(a) == len(b)


@gpu
def test_vsdepth_products_and_solve_equal_across_depths(gpu_ctx):
    N, na, k = 256, 47, 6
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    q = np.random.default_rng(11).standard_normal(A.shape[0])
    xt = shepp_logan(N).ravel(order="F")
    b0 = A @ xt
    e = np.random.default_rng(0).standard_normal(A.shape[0])
    b = b0 + e / np.linalg.norm(e) * 1e-2 * np.linalg.norm(b0)
    depths = _carried(gpu_ctx)
    prod, sol = {}, {}
    for d in depths:
        with gpu_ctx.options(fused_ab=1, fused_vstream=3, fused_vsdepth=d):
            assert hgmres.fused_plan_info(A, B)["vstream"]
            prod[d] = hgmres.spmv_ab(A, B, q)
            assert _same(hgmres.spmv_ab(A, B, q), prod[d]), d
            sol[d] = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=gpu_ctx, return_H=True)
    print(f"[vsdepth 256^2/47] depths {depths}, default {int(gpu_ctx.get_option('fused_vsdepth'))}")
    assert np.any(prod[2][1] != 0.0) and sol[2][3] == k
    for d in depths:
        assert _same(prod[d], prod[2]), d
        assert _same(sol[d], sol[2]), d
    A.close()
    B.close()


@gpu
@pytest.mark.parametrize("N", [36, 40])
def test_vsdepth_waves_with_fewer_batches_than_the_ring(gpu_ctx, N):
    na = 30
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    q = np.random.default_rng(12).standard_normal(A.shape[0])
    with gpu_ctx.options(fused_ab=1, fused_vstream=0):
        hgmres.fused_plan_info(A, B)
        plain = hgmres.spmv_ab(A, B, q)
    out = {}
    for d in _carried(gpu_ctx):
        with gpu_ctx.options(fused_ab=1, fused_vstream=3, fused_vsdepth=d):
            info = hgmres.fused_plan_info(A, B)
            assert info["vstream"], (N, d)
            out[d] = hgmres.spmv_ab(A, B, q)
    for d, o in out.items():
        print(f"[vsdepth N={N} angles={na} depth {d}] Bq vs plain {rel(o[0], plain[0]):.1e}, A(Bq) {rel(o[1], plain[1]):.1e}")
        assert _same(o, out[2]), d
        assert rel(o[0], plain[0]) <= PROD and rel(o[1], plain[1]) <= PROD
    assert np.any(plain[1] != 0.0)
    A.close()
    B.close()


@gpu
def test_vsdepth_pixel_shard(gpu_ctx):
    from hgmres.dist import tile_column_shards
    N, na = 256, 47
    A0 = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    Nn, tile, sup = A0.pixel_order("cols")
    lo, hi = tile_column_shards(N, 4, tile)[1]
    B = A0.T.row_slice(lo, hi)
    A = B.T
    q = np.random.default_rng(8).standard_normal(A.shape[0])
    out = {}
    for d in _carried(gpu_ctx):
        with gpu_ctx.options(fused_ab=1, fused_vstream=3, fused_vsdepth=d):
            assert hgmres.fused_plan_info(A, B)["vstream"]
            out[d] = hgmres.spmv_ab(A, B, q)
    assert np.any(out[2][1] != 0.0)
    for d, o in out.items():
        assert _same(o, out[2]), d
    for M in (A, B, A0):
        M.close()


@gpu
def test_vsdepth_option_values(gpu_ctx):
    default = gpu_ctx.get_option("fused_vsdepth")
    assert default in (2, 3, 4)
    for bad in (5, 1, 2.5):
        with pytest.raises(ValueError, match="fused_vsdepth"):
            gpu_ctx.set_option("fused_vsdepth", bad)
        assert L.load().hgm_ctx_set_option(gpu_ctx.handle, L.OPTIONS_37["fused_vsdepth"], float(bad)) == L.HGM_E_ARG
    assert gpu_ctx.get_option("fused_vsdepth") == default
    # (the plain streams and the row-pair plan keep their own depth)
    assert gpu_ctx.get_option("fused_depth") == 2


@gpu
def test_vsdepth_not_carried_is_refused(gpu_ctx):
    if _experiments():
        pytest.skip("the experiments build carries every depth")
    default = gpu_ctx.get_option("fused_vsdepth")
    missing = [d for d in (2, 3, 4) if d not in _carried(gpu_ctx)]
    assert missing and 2 not in missing and default not in missing
    for d in missing:
        with pytest.raises((ValueError, hgmres.HgmError), match="retired variant"):
            gpu_ctx.set_option("fused_vsdepth", d)
    assert gpu_ctx.get_option("fused_vsdepth") == default


def test_vsdepth_option_id_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "hgmres.h")).read()
    assert L.OPTIONS_37["fused_vsdepth"] == 38
    assert re.search(r"HGM_OPT_FUSED_VSDEPTH\s*=\s*38\b", txt)
    assert L.option_id("fused_vsdepth") == 38
    for name, val in L.OPTIONS_37.items():
        assert re.search(rf"HGM_OPT_{name.upper()}\s*=\s*{val}\b", txt), name
