"""The LDS layout of the one-pass A*(B*q) row-wave kernel (csrc/fused.hip k_fused_rw, DESIGN.md
§3.5): q, the code table and the lanes' dummy slots at LDS address 0, the waves' accumulators
behind them, in every instantiation; and the compact pass's batch set-up on per-wave bases.

Neither changes an operand or the order of a sum, so the checks are those of the passes themselves,
at the smallest geometry that reaches each slot shape (64^2, 4 x 4 tiles, 32 x 32 regions):

  * slot shapes: 17 / 30 / 35 / 47 angles give the 1,088 / 1,344 / 1,536 / 2,048-slot kernels, each
    with the compact stream (their rows pair); 90 angles (rows of ~115 entries, two chunks, no
    pairs) overflows the 32 x 32 regions of a four-wave workgroup (the library carries no
    4,096-slot kernel for four waves) and takes the plain pass on 16 x 16 regions.  The plan's own
    report (HGM_FUSED_VERBOSE) is asserted.  Per shape: spmv_ab and a 3-step AB-GMRES solve (the
    side dot goes through q's first slots) against the two-pass path at the product and solve bars of
    tests/test_gpu_fused.py, a bitwise repeat, and q = e_i bitwise against the plain pass;
  * a full q array: 31 and 48 angles leave 15 and 26 free q slots below the dummies, so the
    dictionary is cut to 14 and 25 codes and the lowest table entry abuts the last ray slot
    (found with the CPU twin hgmres.problems.siddon_projector, whose ray count is asserted too);
  * the fp32 production form: a 3-iteration lsqr_solver on the fp32 pair at 64^2 / 47;
  * shard 1 of a 4-way pixel cut of 64^2 / 47 (rows lo:hi of the unsharded operator), compact and
    plain, against the two-pass product and the host's sums over those rows.
"""
import re

import numpy as np
import pytest

import hgmres
from hgmres import _lib as L
from hgmres.problems import shepp_logan, siddon_projector
from oracle import restatement as R

pytestmark = pytest.mark.gpu

N = 64
TOL = 1e-10          # solves: the bar of tests/test_gpu_fused.py
BQ, ABQ = 1e-14, 1e-13   # products against the two-pass path (test_fused_on_pixel_shards)
SHAPES = (1088, 1344, 1536, 2048, 4096)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def hist_dev(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _problem(A, seed=0):
    xt = shepp_logan(N).ravel(order="F")
    b0 = A @ xt
    e = np.random.default_rng(seed).standard_normal(A.shape[0])
    return b0 + e / np.linalg.norm(e) * 1e-2 * np.linalg.norm(b0), xt


def _plan_report(capfd, monkeypatch, ctx, A, B, **opts):
    """(plan info, the plan build's own report) of a pair that has no plan yet."""
    monkeypatch.setenv("HGM_FUSED_VERBOSE", "1")
    capfd.readouterr()
    with ctx.options(**opts):
        info = hgmres.fused_plan_info(A, B)
    err = capfd.readouterr().err
    monkeypatch.delenv("HGM_FUSED_VERBOSE")
    m = re.findall(r"\[fused rw plan[^\]]*\] region (\d+) waves (\d+).*?max rays (\d+) \(LDS slots (\d+)\)", err)
    assert m, err
    rep = dict(zip(("region", "waves", "worst", "slots"), (int(v) for v in m[-1])))
    c = re.findall(r"value stream\] (\d+) codes", err)
    rep["codes"] = int(c[-1]) if c else None
    return info, rep


def _twin_regions(na, region=32):
    """Ray sets of the region x region pixel blocks of the CPU twin, fullest first."""
    Ac = siddon_projector(N, na).tocsc()
    p = np.arange(N * N)
    blk = (p % N) // region * (N // region) + (p // N) // region
    sets = [np.unique(np.concatenate([Ac.indices[Ac.indptr[c]:Ac.indptr[c + 1]] for c in np.flatnonzero(blk == g)]))
            for g in range((N // region) ** 2)]
    return sorted(sets, key=len, reverse=True)


def _decode_is_exact(ctx, A, B, rays, compact):
    for i in rays:
        q = np.zeros(A.shape[0])
        q[i] = 1.0
        with ctx.options(fused_ab=1, fused_vstream=0):
            plain = hgmres.spmv_ab(A, B, q)
        with ctx.options(fused_ab=1, fused_vstream=3):
            assert hgmres.fused_plan_info(A, B)["vstream"] == compact
            out = hgmres.spmv_ab(A, B, q)
        assert _same(out, plain), i
        assert np.any(plain[0] != 0.0), i


def _against_two_pass(ctx, A, B, opts, tag):
    q = np.random.default_rng(21).standard_normal(A.shape[0])
    b, xt = _problem(A)
    k = 3
    with ctx.options(fused_ab=0):
        bq2, ab2 = hgmres.spmv_ab(A, B, q)
        ref = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=ctx, return_H=True)
    with ctx.options(**opts):
        out = hgmres.spmv_ab(A, B, q)
        again = hgmres.spmv_ab(A, B, q)
        sol = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=ctx, return_H=True)
        sol2 = hgmres.ABgmres_nonhybrid_bounds(A, B, b, xt, 0.0, k, ctx=ctx, return_H=True)
    dH = float(np.max(np.abs(sol[-1] - ref[-1])) / np.max(np.abs(ref[-1])))
    devs = dict(bq=rel(out[0], bq2), abq=rel(out[1], ab2), H=dH, x=rel(sol[0], ref[0]), err=hist_dev(sol[1], ref[1]),
                res=hist_dev(sol[2], ref[2]))
    print(f"[lds layout {tag}] " + " ".join(f"{a}={v:.1e}" for a, v in devs.items()))
    assert np.any(ab2 != 0.0) and sol[3] == ref[3] == k
    assert _same(out, again) and _same(sol, sol2)
    assert devs["bq"] <= BQ and devs["abq"] <= ABQ
    assert max(devs["H"], devs["x"], devs["err"], devs["res"]) <= TOL


@pytest.mark.parametrize("na,slots,region,compact", [(17, 1088, 32, True), (30, 1344, 32, True), (35, 1536, 32, True),
                                                     (47, 2048, 32, True), (90, 2048, 16, False)])
def test_lds_layout_every_slot_shape(gpu_ctx, capfd, monkeypatch, na, slots, region, compact):
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    opts = dict(fused_ab=1, fused_vstream=3) if compact else dict(fused_ab=1)
    info, rep = _plan_report(capfd, monkeypatch, gpu_ctx, A, B, **opts)
    worst = len(_twin_regions(na, region)[0])
    print(f"[lds layout N={N} angles={na}] plan {rep}, compact {info['vstream']}, twin's fullest region {worst} rays")
    assert (rep["slots"], rep["region"], rep["waves"]) == (slots, region, 4)
    assert info["vstream"] == compact
    # the fewest slots that hold the fullest region's rays and the 64 dummies
    assert slots == next(s for s in SHAPES[:4] if worst <= s - 64)
    if region == 16:                               # (what sent the plan to the smaller regions)
        assert len(_twin_regions(na, 32)[0]) > SHAPES[3] - 64
    _against_two_pass(gpu_ctx, A, B, opts, f"angles={na} slots={slots}")
    hit = np.flatnonzero(np.diff(A.to_scipy().indptr) > 0)
    _decode_is_exact(gpu_ctx, A, B, [int(hit[0]), int(hit[len(hit) // 2]), int(hit[-1])], compact)
    A.close()
    B.close()


@pytest.mark.parametrize("na,slots,free", [(31, 1344, 15), (48, 2048, 26)])
def test_lds_layout_full_q_array_cuts_the_dictionary(gpu_ctx, capfd, monkeypatch, na, slots, free):
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B = A.T
    opts = dict(fused_ab=1, fused_vstream=3)
    info, rep = _plan_report(capfd, monkeypatch, gpu_ctx, A, B, fused_plan_dev=0, **opts)   # (the host build reports the rays)
    full = _twin_regions(na)[0]
    print(f"[lds layout full q N={N} angles={na}] plan {rep}, twin's fullest region {len(full)} rays")
    assert info["vstream"] and rep["slots"] == slots and rep["worst"] == len(full)
    assert slots - 64 - rep["worst"] == free and 1 <= free <= 30
    # code c sits at slot slots - 65 - c: the table keeps the codes the free slots hold, and its
    # lowest entry is the slot after the last ray's
    assert rep["codes"] == free - 1 < 31
    assert slots - 65 - rep["codes"] == rep["worst"]
    with gpu_ctx.options(**opts):
        dev = hgmres.fused_plan_info(A, B)         # (the default, device-built plan: the same bytes)
    assert dev["vstream"] and dev["checksum"] == info["checksum"]
    _against_two_pass(gpu_ctx, A, B, opts, f"full q angles={na}")
    # the fullest region's first and last ray slots (the last one next to the table), and its middle
    _decode_is_exact(gpu_ctx, A, B, [int(full[0]), int(full[len(full) // 2]), int(full[-1])], True)
    A.close()
    B.close()


def test_lds_layout_fp32_production_lsqr(gpu_ctx, capfd, monkeypatch):
    na, k = 47, 3
    A64 = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    b, xt = _problem(A64)
    A64.close()
    A = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx, dtype=L.HGM_F32)
    At = A.T
    info, rep = _plan_report(capfd, monkeypatch, gpu_ctx, A, At, fused_ab=1)     # the fp32 one pass is taken
    assert rep["slots"] == 2048 and not info["vstream"]
    with gpu_ctx.options(fused_ab=0):
        two = hgmres.lsqr_solver(A, b, xt, 0.0, k, ctx=gpu_ctx, At=At)
    with gpu_ctx.options(fused_ab=1):
        one = hgmres.lsqr_solver(A, b, xt, 0.0, k, ctx=gpu_ctx, At=At)
        again = hgmres.lsqr_solver(A, b, xt, 0.0, k, ctx=gpu_ctx, At=At)
    xo, eo, ro, ko = R.lsqr_solver_f32(A.to_scipy(), b, xt, 0.0, k)
    devs = dict(x_vs_two_pass=rel(one[0], two[0]), x=rel(one[0], xo), err=hist_dev(one[1], eo), res=hist_dev(one[2], ro))
    print(f"[lds layout fp32 lsqr N={N} angles={na} k={k}] " + " ".join(f"{a}={v:.1e}" for a, v in devs.items()))
    assert one[3] == two[3] == ko == k and _same(one, again)
    # the Golub-Kahan bars of test_fused_gkb_fp32_matches_oracle (the fp32 envelope)
    assert devs["err"] <= 1e-5 and devs["res"] <= 1e-5
    assert devs["x"] <= 1e-4 and devs["x_vs_two_pass"] <= 1e-4
    A.close()
    At.close()


def test_lds_layout_pixel_shard(gpu_ctx):
    from hgmres.dist import tile_column_shards
    na = 47
    A0 = hgmres.SparseOperator.siddon(N, na, ctx=gpu_ctx)
    B0 = A0.T
    Nn, tile, sup = A0.pixel_order("cols")
    lo, hi = tile_column_shards(N, 4, tile)[1]
    q = np.random.default_rng(22).standard_normal(A0.shape[0])
    B = B0.row_slice(lo, hi)                       # the unsharded operator's stored rows lo:hi
    A = B.T
    rows = B.to_scipy()
    assert rows.shape == (hi - lo, B0.shape[1]) and rows.nnz == B.nnz
    ref_bq = rows @ q
    ref_ab = rows.T @ ref_bq
    with gpu_ctx.options(fused_ab=0):
        two = hgmres.spmv_ab(A, B, q)
    for vs in (3, 0):
        with gpu_ctx.options(fused_ab=1, fused_vstream=vs):
            assert hgmres.fused_plan_info(A, B)["vstream"] == bool(vs)
            out = hgmres.spmv_ab(A, B, q)
            again = hgmres.spmv_ab(A, B, q)
        print(f"[lds layout shard rows {lo}:{hi} vstream={vs}] Bq {rel(out[0], ref_bq):.1e} A(Bq) {rel(out[1], ref_ab):.1e}, "
              f"vs two-pass {rel(out[0], two[0]):.1e} {rel(out[1], two[1]):.1e}")
        assert _same(out, again) and np.any(out[1] != 0.0)
        assert rel(out[0], two[0]) <= BQ and rel(out[1], two[1]) <= ABQ
        # (against scipy's sums over the same rows: the 1e-13 of the value-stream tests)
        assert rel(out[0], ref_bq) <= 1e-13 and rel(out[1], ref_ab) <= 1e-13
    for M in (A, B, B0, A0):
        M.close()
